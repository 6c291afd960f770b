"""Run as a subprocess with MPSFM_POISON=1 (tests/test_gpu_descriptor_matches.py): every device block the calls get is filled
with 0xFF first, so a kernel that reads what nobody wrote shows up as a wrong answer."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy_descriptor_matches as NM  # noqa: E402
from mpsfm_amd import capi  # noqa: E402


def main():
    assert os.environ.get("MPSFM_POISON") == "1"
    rng = np.random.default_rng(12)
    errors = []
    for rep in range(3):  # later calls get recycled, poisoned blocks
        n0, n1, dim = ((130, 70, 24), (65, 200, 37), (257, 129, 64))[rep]
        d0, d1 = (rng.integers(-4, 5, (n0, dim)) / 8.0).astype(np.float32), (rng.integers(-4, 5, (n1, dim)) / 8.0).astype(np.float32)
        for kw in (dict(), dict(ratio_threshold=0.9, distance_threshold=1.1), dict(do_mutual_check=False)):
            m, s = capi.match_descriptors(d0, d1, **kw)
            rm, rs, _ = NM.match_descriptors(d0, d1, **kw)
            if not (np.array_equal(m, rm) and np.array_equal(s, rs)):
                errors.append(f"match_descriptors {n0} x {n1} x {dim} {kw}")
        H, W, C = 6 + rep, 9, 5 + rep
        maps = [(rng.integers(-4, 5, (H, W, C)) / 8.0).astype(np.float32) for _ in range(2)]
        confs = [(rng.integers(1, 9, (H, W)) / 8.0).astype(np.float32) for _ in range(2)]
        k0 = np.stack([rng.integers(-1, W + 1, 90), rng.integers(-1, H + 1, 90)], 1) + rng.integers(0, 4, (90, 2)) / 4.0
        k1 = np.stack([rng.integers(-1, W + 1, 70), rng.integers(-1, H + 1, 70)], 1) + rng.integers(0, 4, (70, 2)) / 4.0
        m, s = capi.match_map_descriptors(maps[0], confs[0], maps[1], confs[1], k0, k1, score_threshold=0.5)
        rm, rs, _ = NM.nns_sparse(maps[0], maps[1], confs[0], confs[1], k0, k1, 0.5)
        if not (np.array_equal(m, rm) and np.array_equal(s, rs)):
            errors.append(f"match_map_descriptors {H} x {W} x {C}")
    print("errors:", errors)
    return 1 if errors else 0


if __name__ == "__main__":
    sys.exit(main())
