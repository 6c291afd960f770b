"""Times the dense-match thinning (csrc/dense_matches.hip) beside its NumPy restatement (tests/numpy_dense_matches.py) on the
same inputs:

  mpsfm_radius_nms         5 000 / 20 000 / 100 000 float32 points uniform in 512 x 384, random scores, radius 6
  mpsfm_assign_keypoints   313 600 queries (a 560 x 560 warp) against 4 000 keypoints, max_error 4

Wall time of the capi call (uploads, launches, downloads) and device time (HIP events, first kernel to last); medians of N
calls after a warm-up; the restatement once (--host-n).  The results are compared while at it.  Prints one JSON line per size.

    python scripts/time_dense_matches.py [--n 7] [--host-n 1]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import numpy_dense_matches as ND  # noqa: E402
from mpsfm_amd import capi  # noqa: E402


def timed(fn, n, warmup):
    for _ in range(warmup):
        fn()
    wall, out = [], None
    for _ in range(n):
        t0 = time.perf_counter()
        out = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(wall)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=7)
    ap.add_argument("--host-n", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="*", default=[5000, 20000, 100000])
    ap.add_argument("--queries", type=int, default=313600)
    ap.add_argument("--keypoints", type=int, default=4000)
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("no gfx950 device: nothing to time")
    rng = np.random.default_rng(0)
    for m in a.sizes:
        pts = (rng.random((m, 2)) * [512, 384]).astype(np.float32)
        sc = rng.random(m).astype(np.float32)
        dev = []

        def call():
            keep, info = capi.radius_nms(pts, sc, 6.0, return_info=True)
            dev.append(info["ms"])
            return keep, info

        wall, (keep, info) = timed(call, a.n, a.warmup)
        host, want = timed(lambda: ND.sparse_nms(pts, sc, 6.0), a.host_n, 0) if a.host_n else (None, None)
        print(json.dumps(dict(entry="radius_nms", points=m, kept=int(keep.sum()), rounds=info["rounds"], launches=info["launches"],
                              cells=info["cells"], max_cell_points=info["max_cell_points"], hip_wall_ms_median=wall,
                              hip_device_ms_median=float(np.median(dev[a.warmup:])), numpy_host_ms=host,
                              equal=None if want is None else bool(np.array_equal(np.flatnonzero(keep), want)))), flush=True)
    side = int(round(a.queries ** 0.5))
    gx, gy = np.meshgrid(np.arange(side, dtype=np.float32), np.arange(side, dtype=np.float32))
    q = (np.stack([gx.ravel(), gy.ravel()], 1)[:a.queries] + rng.normal(0, 0.3, (min(a.queries, side * side), 2))).astype(np.float32)
    kps = (rng.random((a.keypoints, 2)) * side).astype(np.float32)
    dev = []

    def call():
        ids, ms = capi.assign_keypoints_ids(q, kps, 4.0, return_ms=True)
        dev.append(ms)
        return ids

    wall, ids = timed(call, a.n, a.warmup)
    host, want = timed(lambda: ND.assign_keypoints(q, kps, 4.0), a.host_n, 0) if a.host_n else (None, None)
    print(json.dumps(dict(entry="assign_keypoints", queries=len(q), keypoints=a.keypoints, assigned=int((ids >= 0).sum()),
                          hip_wall_ms_median=wall, hip_device_ms_median=float(np.median(dev[a.warmup:])), numpy_host_ms=host,
                          equal=None if want is None else bool(np.array_equal(ids, want)))), flush=True)


if __name__ == "__main__":
    main()
