"""Times the two-view geometry estimator at N = 2 000 / 20 000 / 100 000 matches with 30 % and 60 % outliers (general 3-D
scene, inliers with 0.5 px noise, compute_relative_pose on): the wall time of capi.two_view_geometry, the HIP device time
of its launches (the call scope's events), the per-leg trial counts, a sweep of the trial batch size, and the host time of
the NumPy restatement (tests/numpy_two_view_geometry.py) on the same input.  Medians of --n calls after --warmup; the
restatement runs --host-n times (0: skipped) and only up to --host-max-n matches.  Prints one JSON line per configuration.

    python scripts/time_two_view_geometry.py [--n 7] [--warmup 2] [--host-n 1] [--sizes 2000,20000,100000] [--batches 64,256,1024]
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

import numpy_two_view_geometry as TV  # noqa: E402
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
    ap.add_argument("--n", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-n", type=int, default=1)
    ap.add_argument("--host-max-n", type=int, default=20000)
    ap.add_argument("--sizes", default="2000,20000,100000")
    ap.add_argument("--outliers", default="0.3,0.6")
    ap.add_argument("--batches", default="64,256,1024")
    a = ap.parse_args()
    for n in [int(s) for s in a.sizes.split(",")]:
        for out in [float(s) for s in a.outliers.split(",")]:
            s = TV.synthetic_pair("general", n, out, seed=n + int(100 * out), noise_px=0.5)
            args = (s["points1"], s["points2"], s["intr1"], s["intr2"], s["size1"], s["size2"])
            call = lambda **o: capi.two_view_geometry(*args, seed=1, compute_relative_pose=True, **o)  # noqa: E731
            wall, outs = _median(call, a.n, a.warmup)
            r = outs[-1]
            row = dict(n=n, outliers=out, wall_ms=wall, device_ms=float(np.median([o["ms"] for o in outs])), config=r["config"],
                       num_inliers=r["num_inliers"], designed_inliers=int(s["inliers"].sum()),
                       trials={k: v["num_trials"] for k, v in r["legs"].items()}, lo_rounds={k: v["lo_rounds"] for k, v in r["legs"].items()},
                       batches={k: v["num_batches"] for k, v in r["legs"].items()},
                       rot_err=float(np.abs(r["cam2_from_cam1"][:, :3] - s["R"]).max()))
            for b in [int(v) for v in a.batches.split(",")]:
                wall, outs = _median(lambda: call(batch_trials=b), a.n, a.warmup)
                row[f"batch{b}"] = dict(device_ms=float(np.median([o["ms"] for o in outs])), wall_ms=wall)
            if a.host_n > 0 and n <= a.host_max_n:
                host, houts = _median(lambda: TV.estimate(*args, seed=1, compute_relative_pose=True), a.host_n, 0)
                h = houts[-1]
                row["numpy_ms"] = host
                row["numpy_agrees"] = bool(h["config"] == r["config"] and np.array_equal(h["inlier_mask"], r["inlier_mask"]) and
                                           all(h["legs"][k]["num_trials"] == r["legs"][k]["num_trials"] for k in "EFH"))
                row["numpy_fragile"] = len(h["fragile"])
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
