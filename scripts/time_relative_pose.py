"""Times the relative-pose estimator at N = 2 000 / 20 000 / 100 000 matches with 30 % and 60 % outliers (inliers with
0.5 px noise): the HIP device time of the estimation per trial batch size (events around the launches), the wall time of
capi.rel_pose_estimate and of RelativePose.__call__, and the host time of the NumPy restatement
(tests/numpy_relative_pose.py).  Medians of --n calls after --warmup; the restatement runs --host-n times (0: skipped).
Prints one JSON line per configuration.

    python scripts/time_relative_pose.py [--n 9] [--host-n 1] [--sizes 2000,20000,100000] [--batches 64,256,1024]
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

import numpy_relative_pose as NR  # noqa: E402
from mpsfm_amd import capi  # noqa: E402
from mpsfm_amd.sfm.estimators import RelativePose  # noqa: E402


class _Cam:
    def __init__(self, params):
        self.model, self.params = "PINHOLE", np.asarray(params, np.float64)


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
            p1, p2, K1, K2, R, t, inl = NR.synthetic_problem(n, out, seed=n + int(100 * out), noise_px=0.5)
            row = dict(n=n, outliers=out)
            for b in [int(s) for s in a.batches.split(",")]:
                wall, outs = _median(lambda: capi.rel_pose_estimate(p1, p2, K1, K2, seed=1, batch_trials=b), a.n, a.warmup)
                r = outs[-1]
                row[f"batch{b}"] = dict(device_ms=float(np.median([o["ms"] for o in outs])), wall_ms=wall, batches=r["num_batches"],
                                        models=r["num_models"])
            r = capi.rel_pose_estimate(p1, p2, K1, K2, seed=1)
            row.update(trials=r["num_trials"], lo_rounds=r["lo_rounds"], num_inliers=r["num_inliers"], designed_inliers=int(inl.sum()),
                       rot_err=float(np.abs(r["cam2_from_cam1"][:, :3] - R).max()))
            est = RelativePose({"colmap_options": {"random_seed": 1}})
            wall, _ = _median(lambda: est(p1, p2, _Cam(K1), _Cam(K2)), a.n, a.warmup)
            row["relative_pose_call_ms"] = wall
            if a.host_n > 0:
                host, houts = _median(lambda: NR.estimate(p1, p2, K1, K2, seed=1), a.host_n, 0)
                row["numpy_ms"] = host
                row["numpy_agrees"] = bool(houts[-1]["num_trials"] == r["num_trials"] and houts[-1]["num_inliers"] == r["num_inliers"]
                                           and np.array_equal(houts[-1]["inlier_mask"], r["inlier_mask"]))
                row["numpy_fragile"] = len(houts[-1]["fragile"])
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
