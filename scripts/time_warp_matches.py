"""Times the warp-to-matches entry points against what the reference does per pair after the network.

  shape     the sp-roma configurations' 672 x 1344 certainty and 903 168-row warp: a smooth synthetic warp of one scene seen
            with a shift, certainty with saturated regions; 4096 sparse keypoints per image; r = 8, thresh 0.1, max_error 2
  ours      simple_nms on a device tensor; warp_to_matches (dense, sparse, both) from device tensors to host arrays
  yardstick simple_nms: five max_pool2d passes and the mask algebra in torch on the same device, input resident;
            the legs: the reference's path from device tensors to its outputs - the pooling, the mask and to_pixel_coordinates in
            torch, .cpu().numpy(), two SciPy KD-trees queried with every row, the rows grouped by id with argsort / split and a
            Python loop over the groups
Medians of 7 calls after 2 warm-ups; wall time ends in a device synchronise, device time is the call's own HIP-event time
(ours: info["ms"]; torch: events around the expression).  Every timed result is compared with the restatement
(tests/numpy_warp_matches.py); its brute-force lookup runs on every 64th row, and on all rows the KD-tree's ids stand in.

  python scripts/time_warp_matches.py [--out FILE.json] [--quick]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from scipy.spatial import KDTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy_dense_matches as ND  # noqa: E402
import numpy_warp_matches as NW  # noqa: E402
from mpsfm_amd import capi  # noqa: E402
from mpsfm_amd.extraction.pairwise import warp as WM  # noqa: E402

WARMUP, CALLS = 2, 7


def make_scene(H, W, sizes, ns, rng):
    x, y = np.meshgrid((np.arange(W) + 0.5) / W * 2 - 1, (np.arange(H) + 0.5) / H * 2 - 1)
    warp = np.stack([x, y, x + 0.11 + 0.02 * np.sin(3 * y), y - 0.07 + 0.02 * np.cos(2 * x)], -1).astype(np.float32)
    cert = np.clip(0.55 + 0.6 * np.sin(9 * x + 1) * np.cos(7 * y) + 0.05 * rng.random((H, W)), 0, 1).astype(np.float32)  # saturated at 0 and 1
    kA, kB = NW.to_pixel_coordinates(warp, *sizes)
    rows = rng.permutation(H * W)[:ns]
    s0 = kA[rows].astype(np.float64) + rng.uniform(-0.7, 0.7, (ns, 2))
    s1 = kB[rows].astype(np.float64) + rng.uniform(-0.7, 0.7, (ns, 2))
    s1[2 * ns // 3:] = rng.random((ns - 2 * ns // 3, 2)) * [sizes[3], sizes[2]]
    return warp, cert, s0, s1[rng.permutation(ns)]


def torch_simple_nms(s, r):
    def pool(x):
        return torch.nn.functional.max_pool2d(x[None, None], 2 * r + 1, 1, r)[0, 0]

    zero = torch.zeros_like(s)
    keep = s == pool(s)
    for _ in range(2):
        near = pool(keep.float()) > 0
        rest = torch.where(near, zero, s)
        keep = keep | ((rest == pool(rest)) & ~near)
    return torch.where(keep, s, zero)


def torch_pixels(w, sizes):
    HA, WA, HB, WB = sizes
    return (torch.stack((WA / 2 * (w[:, 0] + 1), HA / 2 * (w[:, 1] + 1)), -1), torch.stack((WB / 2 * (w[:, 2] + 1), HB / 2 * (w[:, 3] + 1)), -1))


def host_assign(q, kps, max_error):
    d, i = KDTree(kps).query(q, distance_upper_bound=max_error)
    i[d > max_error] = -1
    return i


def host_groups(ids):
    order = np.argsort(ids)
    _, first = np.unique(ids[order], return_index=True)
    return np.split(order, first[1:])


def host_unique(ids0, ids1, scores):
    ok = (ids0 != -1) & (ids1 != -1)
    pairs, sc = np.stack([ids0[ok], ids1[ok]], 1), scores[ok]
    if len(pairs) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.float16)
    a = [g[sc[g].argmax()] for g in host_groups(pairs[:, 0])]
    b = [g[sc[g].argmax()] for g in host_groups(pairs[:, 1])]
    keep = list(set(a).intersection(b))
    pairs, sc = pairs[keep], sc[keep]
    m, s = -np.ones(pairs[:, 0].max() + 1), np.zeros(pairs[:, 0].max() + 1)
    m[pairs[:, 0]], s[pairs[:, 0]] = pairs[:, 1], sc
    return m.astype(np.int32), s.astype(np.float16)


def yardstick(tw, tc, sizes, mode, s0, s1, r, thresh, max_error):
    out = {}
    w = tw.reshape(-1, 4)
    if "dense" in mode:
        nms = torch_simple_nms(tc, r).reshape(-1)
        sel = nms > thresh
        a, b = torch_pixels(w[sel], sizes)
        out.update(dkeypoints0=a.cpu().numpy(), dkeypoints1=b.cpu().numpy(), dscores=nms[sel].cpu().numpy())
    if "sparse" in mode:
        c = tc.reshape(-1).cpu().numpy()
        a, b = torch_pixels(w, sizes)
        ids0 = host_assign(a.cpu().numpy() * np.ones(2), s0, max_error)
        ids1 = host_assign(b.cpu().numpy() * np.ones(2), s1, max_error)
        out["smatches0"], out["smatching_scores0"] = host_unique(ids0, ids1, c)
        out["ids0"], out["ids1"] = ids0, ids1
    return out


def timed(fn, device_ms=None):
    """median wall ms (ending in a synchronise) and median device ms of CALLS calls after WARMUP"""
    wall, dev, last = [], [], None
    for k in range(WARMUP + CALLS):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = time.perf_counter()
        e0.record()
        last = fn()
        e1.record()
        torch.cuda.synchronize()
        if k >= WARMUP:
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(device_ms(last) if device_ms else e0.elapsed_time(e1))
    return statistics.median(wall), statistics.median(dev), last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="a 96 x 192 map and 512 keypoints")
    args = ap.parse_args()
    H, W, ns = (96, 192, 512) if args.quick else (672, 1344, 4096)
    sizes = (H, W // 2, H, W // 2)
    r, thresh, max_error = 8, 0.1, 2.0
    rng = np.random.default_rng(5)
    warp, cert, s0, s1 = make_scene(H, W, sizes, ns, rng)
    tw, tc = torch.from_numpy(warp).cuda(), torch.from_numpy(cert).cuda()
    rows, ok = [], True

    want_nms = NW.simple_nms(cert, r)
    o_wall, o_dev, got = timed(lambda: capi.simple_nms_map(tc, r, return_info=True), lambda x: x[1]["ms"])
    y_wall, y_dev, ref = timed(lambda: torch_simple_nms(tc, r))
    agree = bool(np.array_equal(got[0].cpu().numpy().view(np.uint32), want_nms.view(np.uint32)) and torch.equal(got[0], ref))
    rows.append(dict(what="simple_nms", ours_wall_ms=o_wall, ours_device_ms=o_dev, yardstick_wall_ms=y_wall, yardstick_device_ms=y_dev,
                     speedup_wall=y_wall / o_wall, speedup_device=y_dev / o_dev, agrees_with_restatement=agree, kept=int((want_nms != 0).sum())))
    ok &= agree

    sub = np.arange(0, H * W, 64)
    kA, kB = NW.to_pixel_coordinates(warp, *sizes)
    for mode in ("dense", "sparse", "sparse+dense"):
        kw = dict(skpts0=s0, skpts1=s1, nms_radius=r, sample_thresh=thresh, max_error=max_error)
        bits = (1 if "dense" in mode else 0) | (2 if "sparse" in mode else 0)
        o_wall, o_dev, got = timed(lambda: capi.warp_matches(tw, tc, sizes, bits, return_info=True, **kw), lambda x: x[1]["ms"])
        y_wall, _, ref = timed(lambda: yardstick(tw, tc, sizes, mode, s0, s1, r, thresh, max_error))
        agree, extra = True, {}
        if "dense" in mode:
            sel = want_nms.reshape(-1) > np.float32(thresh)
            for k, v in (("dkeypoints0", kA[sel]), ("dkeypoints1", kB[sel]), ("dscores", want_nms.reshape(-1)[sel])):
                agree &= bool(np.array_equal(got[0][k], v) and np.array_equal(ref[k], v))
        if "sparse" in mode:
            agree &= bool(np.array_equal(ND.assign_keypoints(kA[sub].astype(np.float64), s0, max_error), ref["ids0"][sub]))
            agree &= bool(np.array_equal(ND.assign_keypoints(kB[sub].astype(np.float64), s1, max_error), ref["ids1"][sub]))
            m, s, _ = NW.kpids_to_matches0(ref["ids0"], ref["ids1"], cert.reshape(-1))
            agree &= bool(np.array_equal(got[0]["smatches0"], m) and np.array_equal(got[0]["smatching_scores0"], s))
            # equal certainties (the saturated regions) tie inside a group: the yardstick's winner is then its argsort's, not the lowest row
            extra["yardstick_equals_restatement"] = bool(np.array_equal(ref["smatches0"], m) and np.array_equal(ref["smatching_scores0"], s.astype(np.float16)))
        rows.append(dict(what=mode, ours_wall_ms=o_wall, ours_device_ms=o_dev, yardstick_wall_ms=y_wall, speedup_wall=y_wall / o_wall,
                         agrees_with_restatement=agree, **extra, **{k: v for k, v in got[1].items() if k != "ms"}))
        ok &= agree
    pred = WM.warp_to_matches(tw, tc, sizes, "sparse+dense", s0, s1)
    ok &= pred["smatching_scores0"].dtype == np.float16
    result = dict(shape=[H, W], keypoints=ns, radius=r, rows=rows, all_agree=bool(ok))
    for row in rows:
        print(json.dumps(row))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
