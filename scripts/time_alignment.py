"""Times the 3D-3D alignment at N = 2 000 / 20 000 / 100 000 point pairs with 30 % and 60 % outliers, rigid and similarity
(tests/numpy_alignment.py:synthetic_problem): the HIP device time of capi.align3d_estimate (events around the launches) at trial
batches of 64 / 256 / 1024, the wall time of the call, the wall time of the NumPy restatement, and the restatement with
min = max = 5000 trials, the stand-in for the fixed 5000-iteration loop of the reference's icp/main.py (the script itself cannot
run: it reads its dataset at import).  Medians of --n calls after --warmup; the restatement runs --host-n times.  Prints one JSON
line per configuration.

    python scripts/time_alignment.py [--n 9] [--host-n 1] [--sizes 2000,20000,100000]
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

import numpy_alignment as NAL  # noqa: E402
from mpsfm_amd import capi  # noqa: E402


def _median(f, n, warmup):
    for _ in range(warmup):
        f()
    ts, outs = [], []
    for _ in range(n):
        t0 = time.perf_counter()
        outs.append(f())
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-n", type=int, default=1)
    ap.add_argument("--sizes", default="2000,20000,100000")
    ap.add_argument("--outliers", default="0.3,0.6")
    ap.add_argument("--batches", default="64,256,1024")
    a = ap.parse_args()
    for n in [int(s) for s in a.sizes.split(",")]:
        for out in [float(s) for s in a.outliers.split(",")]:
            for with_scale in (False, True):
                src, tgt, R, t, s, inl = NAL.synthetic_problem(n, out, n + int(100 * out), with_scale)
                row = dict(n=n, outliers=out, model="sim3d" if with_scale else "rigid3d")
                for b in [int(v) for v in a.batches.split(",")]:
                    wall, outs = _median(lambda: capi.align3d_estimate(src, tgt, with_scale, seed=1, batch_trials=b), a.n, a.warmup)
                    r = outs[-1]
                    row[f"batch{b}"] = dict(device_ms=float(np.median([o["ms"] for o in outs])), wall_ms=wall, batches=r["num_batches"],
                                            models=r["num_models"])
                wall, outs = _median(lambda: capi.align3d_estimate(src, tgt, with_scale, seed=1), a.n, a.warmup)
                r = outs[-1]
                row.update(default_batch=dict(device_ms=float(np.median([o["ms"] for o in outs])), wall_ms=wall, batches=r["num_batches"]),
                           trials=r["num_trials"], lo_rounds=r["lo_rounds"], num_inliers=r["num_inliers"], designed_inliers=int(inl.sum()))
                host, houts = _median(lambda: NAL.estimate(src, tgt, with_scale, seed=1), a.host_n, 0)
                row["numpy_ms"] = host
                row["numpy_agrees"] = bool(houts[-1]["num_trials"] == r["num_trials"] and houts[-1]["num_inliers"] == r["num_inliers"]
                                           and np.array_equal(houts[-1]["inlier_mask"], r["inlier_mask"]))
                row["numpy_fragile"] = len(houts[-1]["fragile"])
                fixed, _ = _median(lambda: NAL.estimate(src, tgt, with_scale, seed=1, min_num_trials=5000, max_num_trials=5000), a.host_n, 0)
                row["numpy_5000_trials_ms"] = fixed  # the stand-in for the reference's fixed loop
                fit_wall, fouts = _median(lambda: capi.align3d_fit(src, tgt, r["inlier_mask"], with_scale), a.n, a.warmup)
                row["fit"] = dict(device_ms=float(np.median([o["ms"] for o in fouts])), wall_ms=fit_wall)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
