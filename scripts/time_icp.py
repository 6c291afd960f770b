"""Times the dense point-to-plane ICP (capi.depth_pair_icp) on tests/depth_icp_scenes.py's pair at 120 x 160, 240 x 320 and
480 x 640, stride 1 and 2, from the large perturbed start: the HIP device time of a call (events around the launches) and per
iteration, the wall time of the call from NumPy arrays, the wall time of the NumPy restatement on this machine's CPU, what the
launches enqueued past convergence cost (the same call with max_iterations = the iterations it takes), and
capi.depth_pair_register_dense against depth_pair_register followed by depth_pair_icp on 400 matched keypoints.  Medians of --n
calls after --warmup; the restatement runs --host-n times.  Prints one JSON line per configuration.

    python scripts/time_icp.py [--n 9] [--warmup 3] [--host-n 1] [--sizes 120x160,240x320,480x640]
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

import depth_icp_scenes as S  # noqa: E402
import numpy_alignment as NAL  # noqa: E402
import numpy_depth_icp as NDI  # noqa: E402
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


def _device_ms(outs, key=None):
    return float(np.median([(o if key is None else o[key])["ms"] for o in outs]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-n", type=int, default=1)
    ap.add_argument("--sizes", default="120x160,240x320,480x640")
    a = ap.parse_args()
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        s = S.render_pair(H, W, S.scene_intr(H, W))
        d0, d1, K = s["depth0"], s["depth1"], s["intr"]
        start = S.starts(s["R"], s["t"])[2]
        for stride in (1, 2):
            row = dict(H=H, W=W, stride=stride)
            wall, outs = _median(lambda: capi.depth_pair_icp(d0, K, d1, K, start, stride=stride), a.n, a.warmup)
            r = outs[-1]
            row.update(status=r["status"], iterations=r["iterations"], num_pairs=r["num_pairs"], device_ms=_device_ms(outs), wall_ms=wall)
            row["device_ms_per_iteration"] = row["device_ms"] / r["iterations"]
            # the same call without the launches that find `done` set; it ends as max_iterations on the same pose
            wall_k, outs_k = _median(lambda: capi.depth_pair_icp(d0, K, d1, K, start, stride=stride, max_iterations=r["iterations"]), a.n, a.warmup)
            row["no_enqueue_ahead"] = dict(device_ms=_device_ms(outs_k), wall_ms=wall_k,
                                           same_pose=bool(np.array_equal(outs_k[-1]["tgt_from_src"], r["tgt_from_src"])))
            host, houts = _median(lambda: NDI.icp(d0, K, d1, K, start, stride=stride), a.host_n, 0)
            row["numpy_ms"] = host
            row["numpy_agrees"] = bool(houts[-1]["status"] == r["status"] and houts[-1]["counts"] == r["trace"][:, 0].tolist()
                                       and np.abs(houts[-1]["tgt_from_src"] - r["tgt_from_src"]).max() < 1e-9)
            row["numpy_fragile"] = len(houts[-1]["fragile"])
            if stride == 1:
                rng = np.random.default_rng(H)
                kps0 = np.c_[rng.uniform(2, W - 3, 400), rng.uniform(2, H - 3, 400)]
                X0, ok = NAL.lift(d0, K, kps0)
                X1 = X0[ok] @ s["R"].T + s["t"]
                kps0, kps1 = kps0[ok], np.c_[X1[:, 0] / X1[:, 2] * K[0] + K[2], X1[:, 1] / X1[:, 2] * K[1] + K[3]]
                m = np.stack([np.arange(len(kps0))] * 2, 1).astype(np.int32)
                wall_d, outs_d = _median(lambda: capi.depth_pair_register_dense(d0, K, d1, K, kps0, kps1, m, seed=1), a.n, a.warmup)

                def two_calls():
                    first = capi.depth_pair_register(d0, K, d1, K, kps0, kps1, m, seed=1)
                    return first, capi.depth_pair_icp(d0, K, d1, K, first["tgt_from_src"], scale=first["scale"])

                wall_2, outs_2 = _median(two_calls, a.n, a.warmup)
                row["register_dense"] = dict(wall_ms=wall_d, ransac_device_ms=_device_ms(outs_d), icp_device_ms=_device_ms(outs_d, "refined"),
                                             iterations=outs_d[-1]["refined"]["iterations"])
                row["two_calls"] = dict(wall_ms=wall_2, ransac_device_ms=_device_ms(outs_2, 0), icp_device_ms=_device_ms(outs_2, 1),
                                        same_pose=bool(np.array_equal(outs_2[-1][1]["tgt_from_src"], outs_d[-1]["refined"]["tgt_from_src"])))
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
