"""Times the two registration entry points (csrc/registration.hip) beside their NumPy restatement
(tests/numpy_registration.py) on the same inputs:

  mpsfm_registration_pairs     6 reference images with 290x387 maps, 2 000 / 20 000 / 100 000 matches EACH
  mpsfm_init_pair_candidates   an init pair with a 290x387 prior map, 2 000 / 20 000 / 100 000 matches

Wall time of the capi call (uploads of the maps and arrays, launch, downloads) and device time of the launch (HIP events);
medians of N calls after a warm-up.  Prints one JSON line per size.

    python scripts/time_registration.py [--n 7] [--host-n 5]
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

import numpy_registration as NR  # noqa: E402
from mpsfm_amd import capi  # noqa: E402
from test_gpu_registration import big_init, big_pairs  # noqa: E402


def timed(fn, n, warmup):
    for _ in range(warmup):
        fn()
    wall, dev = [], []
    for _ in range(n):
        t0 = time.perf_counter()
        ms = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(ms)
    return float(np.median(wall)), float(np.median(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=7)
    ap.add_argument("--host-n", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="*", default=[2000, 20000, 100000])
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("no gfx950 device: nothing to time")
    for m in a.sizes:
        p = big_pairs(1, n=6 * m, n_pts=max(m, 1000))
        wall, dev = timed(lambda: capi.registration_pairs(return_ms=True, **p)[2], a.n, a.warmup)
        host, _ = timed(lambda: NR.registration_pairs(**p) and 0.0, a.host_n, 1)
        print(json.dumps(dict(entry="registration_pairs", refs=6, maps="290x387", matches_per_ref=m, hip_wall_ms_median=wall,
                              hip_device_ms_median=dev, numpy_host_ms_median=host)), flush=True)
    for m in a.sizes:
        p = big_init(2, n=m)
        wall, dev = timed(lambda: capi.init_pair_candidates(**p)["ms"], a.n, a.warmup)
        host, _ = timed(lambda: NR.init_pair_candidates(**p) and 0.0, a.host_n, 1)
        wall2, dev2 = timed(lambda: capi.init_pair_candidates(what=capi.INIT_LIFT, rescale=0.5, **p)["ms"], a.n, a.warmup)
        print(json.dumps(dict(entry="init_pair_candidates", map="290x387", matches=m, hip_wall_ms_median=wall, hip_device_ms_median=dev,
                              numpy_host_ms_median=host, lift_only_wall_ms_median=wall2, lift_only_device_ms_median=dev2)), flush=True)


if __name__ == "__main__":
    main()
