"""Times one depth-consistency check of a query against 5 references at 290x387 (the reference's map size): the HIP
device time of the call (events around the launches), the wall time of capi.depth_consistency including uploads and the
count download, and the host time of the NumPy restatement (tests/numpy_depth_consistency.py).  Medians of N calls after
warm-up.  Prints one JSON line.

    python scripts/time_depth_consistency.py [--n 50] [--host-n 5]
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

import numpy_depth_consistency as NDC  # noqa: E402
from mpsfm_amd import capi  # noqa: E402
from test_gpu_depth_consistency import big_bundle  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--host-n", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("no gfx950 device: nothing to time")
    ims = big_bundle(a.seed)
    pairs = [(0, r) for r in range(1, 6)]
    for _ in range(a.warmup):
        capi.depth_consistency(ims, pairs)
    dev, wall = [], []
    for _ in range(a.n):
        t0 = time.perf_counter()
        counts, s = capi.depth_consistency(ims, pairs)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(s["ms"])
    host = []
    for _ in range(a.host_n):
        t0 = time.perf_counter()
        score_np, _, counts_np, _ = NDC.bundle([dict(im, depth=im["depth"].copy()) for im in ims], 0, list(range(1, 6)))
        host.append((time.perf_counter() - t0) * 1e3)
    score, _ = NDC.bundle_score(counts)
    print(json.dumps(dict(maps="290x387 query, refs 290x387 / 240x320", refs=5, pixels=int(s["n_pixels"]), calls=a.n,
                          hip_device_ms_median=float(np.median(dev)), hip_device_ms_min=float(np.min(dev)),
                          hip_wall_ms_median=float(np.median(wall)), hip_wall_ms_min=float(np.min(wall)),
                          numpy_host_ms_median=float(np.median(host)), score=score, score_numpy=score_np,
                          counts_equal=bool(np.array_equal(counts, counts_np)))))


if __name__ == "__main__":
    main()
