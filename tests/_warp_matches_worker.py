"""Run as a subprocess with MPSFM_POISON=1 (tests/test_gpu_warp_matches.py): every device block the calls get is filled with 0xFF
first, so a kernel that reads what nobody wrote shows up as a wrong answer."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy_warp_matches as NW  # noqa: E402
from mpsfm_amd import capi  # noqa: E402


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def main():
    assert os.environ.get("MPSFM_POISON") == "1"
    rng = np.random.default_rng(12)
    errors = []
    for rep in range(3):  # later calls get recycled, poisoned blocks
        H, W, r = ((33, 70, 4), (65, 129, 8), (40, 64, 1))[rep]
        cert = (rng.integers(0, 9, (H, W)) / 8.0).astype(np.float32)
        if not same(capi.simple_nms_map(cert, r), NW.simple_nms(cert, r)):
            errors.append(f"simple_nms {H} x {W} r {r}")
        n, n0, n1 = 5000 + 77 * rep, 40 + rep, 30
        ids0, ids1 = rng.integers(-1, n0, n), rng.integers(-1, n1, n)
        sc = (rng.integers(-4, 5, n) / 8.0).astype(np.float32)
        m, s = capi.kpids_to_matches0_arrays(ids0, ids1, sc, n0, n1)
        rm, rs, _ = NW.kpids_to_matches0(ids0, ids1, sc)
        if not (same(m, rm) and same(s, rs)):
            errors.append(f"kpids_to_matches0 {n}")
        sizes = (90, 120, 80, 110)
        warp = (rng.random((H, W, 4)) * 2 - 1).astype(np.float32)
        kA, kB = NW.to_pixel_coordinates(warp, *sizes)
        rows = rng.permutation(H * W)[:150]
        s0, s1 = kA[rows] + rng.uniform(-0.7, 0.7, (150, 2)), kB[rows] + rng.uniform(-0.7, 0.7, (150, 2))
        got = capi.warp_matches(warp, cert, sizes, 3, skpts0=s0, skpts1=s1, nms_radius=r, sample_thresh=0.3)
        want = NW.warp_to_matches(warp, cert, sizes, True, True, s0, s1, nms_radius=r, sample_thresh=0.3)
        for k in got:
            if not same(got[k], want[k]):
                errors.append(f"warp_matches {H} x {W}: {k}")
    print("errors:", errors)
    return 1 if errors else 0


if __name__ == "__main__":
    sys.exit(main())
