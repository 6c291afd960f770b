"""Run as a subprocess with MPSFM_POISON=1 (tests/test_gpu_dense_matches.py): every device block the calls get is filled
with 0xFF first, so a kernel that reads what nobody wrote shows up as a wrong answer."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy_dense_matches as ND  # noqa: E402
from mpsfm_amd import capi  # noqa: E402


def main():
    assert os.environ.get("MPSFM_POISON") == "1"
    rng = np.random.default_rng(11)
    errors = []
    for rep in range(3):  # later calls get recycled, poisoned blocks
        n = (700, 1300, 257)[rep]
        pts, sc = rng.random((n, 2)) * [200, 150], np.round(rng.random(n) * 16)
        if not np.array_equal(np.flatnonzero(capi.radius_nms(pts, sc, 6.0)), ND.sparse_nms(pts, sc, 6.0)):
            errors.append(f"radius_nms {n}")
        s0, s1 = rng.random((80, 2)) * [200, 150], rng.random((80, 2)) * [200, 150]
        d1 = pts + rng.normal(0, 2, pts.shape)
        for flag in (True, False):
            got = np.flatnonzero(capi.thin_dense_matches_mask(pts, d1, sc, s0, s1, 6.0, reference_slice=flag))
            if not np.array_equal(got, ND.thin_dense_mask(pts, d1, sc, s0, s1, 6.0, flag)):
                errors.append(f"thin_dense_matches {n} slice={flag}")
        q = rng.random((3000, 2)) * [220, 170] - 10
        if not np.array_equal(capi.assign_keypoints_ids(q, pts, 5.0), ND.assign_keypoints(q, pts, 5.0)):
            errors.append(f"assign_keypoints {n}")
    print("errors:", errors)
    return 1 if errors else 0


if __name__ == "__main__":
    sys.exit(main())
