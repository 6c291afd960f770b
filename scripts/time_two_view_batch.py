"""Times the batched two-view geometry against the loop of single calls: P general pairs with distinct seeds (30 % outliers,
inliers with 0.5 px noise) and the reference's options (max_num_trials 20 000, min_inlier_ratio 0.1, compute_relative_pose on).
Per cell (P, n): the wall time of the loop of capi.two_view_geometry calls (the per-pair path, the baseline), the wall time of
one capi.two_view_geometry_batch call with the default grouping, its report (device ms, synchronisations, launches, groups)
and a sweep of pairs_per_group.  Medians of --n calls after --warmup (the loop: --loop-n after --loop-warmup).  Every batched
result is compared with the loop's; the script ends at the first difference or error.  Prints one JSON line per cell.  Run it
under a time limit:

    timeout -k 10 900 python scripts/time_two_view_batch.py [--n 7] [--warmup 2] [--pairs 1,16,64,256] [--sizes 500,2000]
        [--big-size 20000] [--big-max-pairs 16] [--groups 16,64,256]
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

OPTS = dict(max_num_trials=20000, min_inlier_ratio=0.1, compute_relative_pose=True, seed=1)


def _median(f, n, warmup):
    for _ in range(warmup):
        f()
    ts, outs = [], []
    for _ in range(n):
        t0 = time.perf_counter()
        outs.append(f())
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, outs


def _check(batch, loop):
    for k, (a, b) in enumerate(zip(batch, loop)):
        same = a["config"] == b["config"] and a["legs"] == b["legs"] and np.array_equal(a["inlier_mask"], b["inlier_mask"]) and all(
            a[f].tobytes() == b[f].tobytes() for f in ("E", "F", "H", "cam2_from_cam1")) and a["tri_angle"] == b["tri_angle"]
        if not same:
            raise SystemExit(f"pair {k}: the batched result differs from the single call")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-n", type=int, default=None)
    ap.add_argument("--loop-warmup", type=int, default=None)
    ap.add_argument("--pairs", default="1,16,64,256")
    ap.add_argument("--sizes", default="500,2000")
    ap.add_argument("--big-size", type=int, default=20000)
    ap.add_argument("--big-max-pairs", type=int, default=16)
    ap.add_argument("--groups", default="16,64,256")
    a = ap.parse_args()
    loop_n = a.n if a.loop_n is None else a.loop_n
    loop_warmup = a.warmup if a.loop_warmup is None else a.loop_warmup
    sizes = [int(s) for s in a.sizes.split(",") if s]
    for P in [int(s) for s in a.pairs.split(",")]:
        for n in sizes + ([a.big_size] if a.big_size > 0 and P <= a.big_max_pairs else []):
            pairs = []
            for k in range(P):
                s = TV.synthetic_pair("general", n, 0.3, seed=1000 * n + k, noise_px=0.5)
                pairs.append((s["points1"], s["points2"], s["intr1"], s["intr2"], s["size1"], s["size2"]))
            loop_ms, louts = _median(lambda: [capi.two_view_geometry(*p, **OPTS) for p in pairs], loop_n, loop_warmup)
            batch_ms, bouts = _median(lambda: capi.two_view_geometry_batch(pairs, return_report=True, **OPTS), a.n, a.warmup)
            res, rep = bouts[-1]
            _check(res, louts[-1])
            row = dict(pairs=P, n=n, loop_wall_ms=loop_ms, loop_device_ms=float(sum(r["ms"] for r in louts[-1])), batch_wall_ms=batch_ms,
                       speedup=loop_ms / batch_ms, report=rep, configs=sorted({r["config"] for r in res}),
                       trials={g: int(np.median([r["legs"][g]["num_trials"] for r in res])) for g in "EFH"},
                       lo_rounds={g: int(sum(r["legs"][g]["lo_rounds"] for r in res)) for g in "EFH"})
            for g in [int(v) for v in a.groups.split(",") if v]:
                if g > P and g != int(a.groups.split(",")[0]):
                    continue  # a group larger than the batch is the same call as the smallest such group
                wall, outs = _median(lambda: capi.two_view_geometry_batch(pairs, pairs_per_group=g, return_report=True, **OPTS), a.n, a.warmup)
                _check(outs[-1][0], louts[-1])
                row[f"group{g}"] = dict(wall_ms=wall, device_ms=outs[-1][1]["ms"], num_syncs=outs[-1][1]["num_syncs"],
                                        num_launches=outs[-1][1]["num_launches"], num_groups=outs[-1][1]["num_groups"])
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
