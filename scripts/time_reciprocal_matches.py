"""Times the dense reciprocal matcher against the reference's own expression in torch on the same device.

  extract_correspondences   384 x 512 x 24 maps, subsample 8, four searches, one pair
from host arrays and from device tensors.  The yardstick is what the reference does per pair with MASt3R's fast_reciprocal_NNs,
restated in torch float32 on device-resident inputs: block-wise `A @ B.T` + max per block, and the NumPy round trips of the descent
loop (indices go to the host and back in every half-step), then merge_corres and the confidence product in NumPy.  Medians of 7
calls after 2 warm-ups; wall time ends in a device synchronise, device time is the call's own HIP-event time (ours: info["ms"];
torch: events around the expression, which include its host waits).

Agreement: the same descent in torch float64 with a top-2 gives every seed's pair and the smallest gap of its trajectory.  Ours must
give the float64 pairs exactly (no seed's gap is below tau64 = 4 C 2^-53, asserted); the float32 yardstick may differ on seeds
whose gap is below tau32 = 4 C 2^-24 and on no other.

  python scripts/time_reciprocal_matches.py [--out FILE.json] [--quick]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy_reciprocal_matches as NR  # noqa: E402
from mpsfm_amd import capi  # noqa: E402

WARMUP, CALLS = 2, 7
MAX_ITER, BLOCK = 10, 2 ** 13


def torch_nn(Q, M, top2):
    """per row of Q the best row of M (lowest index among equal maxima, block by block)[, best - second best]"""
    bv = torch.full((len(Q),), -torch.inf, dtype=Q.dtype, device=Q.device)
    bi = torch.zeros(len(Q), dtype=torch.int64, device=Q.device)
    sv = bv.clone()
    for c0 in range(0, len(M), BLOCK):
        sim = Q @ M[c0:c0 + BLOCK].T
        if top2:
            v, i = sim.topk(min(2, sim.shape[1]), dim=1)
            v1, i1, v2 = v[:, 0], i[:, 0], v[:, 1] if v.shape[1] > 1 else torch.full_like(bv, -torch.inf)
        else:
            v1, i1 = sim.max(1)
            v2 = v1
        better = v1 > bv
        if top2:
            sv = torch.where(better, torch.maximum(bv, v2), torch.maximum(sv, v1))
        bi = torch.where(better, i1 + c0, bi)
        bv = torch.where(better, v1, bv)
    return bi, bv - sv


def torch_descent(A, B, S, dtype, top2=False):
    """fast_reciprocal_NNs(A, B, subsample_or_initxy1=S, ret_xy=False) as upstream runs it: the state lives in NumPy, every
    half-step gathers the active rows on the device, takes the nearest neighbours there and brings the indices back."""
    C = A.shape[2]
    fa, fb = A.reshape(-1, C).to(dtype), B.reshape(-1, C).to(dtype)
    xy1 = NR.seed_pixels(A.shape[0], A.shape[1], S).astype(np.int64)
    xy2 = np.full(len(xy1), -1, np.int64)
    old1, old2 = xy1.copy(), xy2.copy()
    active = np.ones(len(xy1), bool)
    gap = np.full(len(xy1), np.inf)
    for _ in range(MAX_ITER):
        if not active.any():
            break
        for src, dst, old, fq, fm in ((xy1, xy2, old2, fa, fb), (xy2, xy1, old1, fb, fa)):
            a = np.flatnonzero(active)
            if len(a) == 0:
                break
            i, g = torch_nn(fq[torch.from_numpy(src[a]).to(fq.device)], fm, top2)
            dst[a] = i.cpu().numpy()
            if top2:
                gap[a] = np.minimum(gap[a], g.cpu().numpy())
            active[a] = dst[a] != old[a]
        old1, old2 = xy1.copy(), xy2.copy()
    return xy1, xy2, ~active, gap


def torch_extract(feats, qonfs, S, dtype=torch.float32):
    f11, f21, f22, f12 = feats
    q11, q21, q22, q12 = [q.cpu() for q in qonfs]
    idx1, idx2, q1, q2 = [], [], [], []
    for A, B, QA, QB in ((f11, f21, q11, q21), (f12, f22, q12, q22)):
        res = []
        for X, Y in ((A, B), (B, A)):
            xy1, xy2, conv, _ = torch_descent(X, Y, S, dtype)
            p = np.unique(np.stack([xy1[conv], xy2[conv]], 1), axis=0)
            res.append((p[:, 0].astype(np.int32), p[:, 1].astype(np.int32)))
        idx1.append(np.r_[res[0][0], res[1][1]])
        idx2.append(np.r_[res[0][1], res[1][0]])
        q1.append(QA.ravel()[idx1[-1]].numpy())
        q2.append(QB.ravel()[idx2[-1]].numpy())
    xy1, xy2, first = NR.merge_corres(np.concatenate(idx1), np.concatenate(idx2), tuple(f11.shape[:2]), tuple(f22.shape[:2]))
    return xy1, xy2, np.sqrt(np.concatenate(q1)[first] * np.concatenate(q2)[first])


def timed(fn):
    """medians of wall and device ms over CALLS calls; fn returns (result, device ms or None: measured here with events)"""
    wall, dev, res = [], [], None
    for it in range(WARMUP + CALLS):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        res, ms = fn()
        e1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if it >= WARMUP:
            wall.append(1e3 * (t1 - t0))
            dev.append(ms if ms is not None else e0.elapsed_time(e1))
    return res, statistics.median(wall), statistics.median(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="small shapes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    if not torch.cuda.is_available() or capi.device_count() < 1:
        raise SystemExit("no device: nothing here is measured without one")
    H, W, Cc, S = (384, 512, 24, 8) if not a.quick else (48, 64, 24, 4)
    shift = (4 * (W // 8) + 2, -4 * (H // 8) + 1)  # quarter pixels
    views = [NR.scene_maps(2024, H, W, Cc, sh, noise_seed=k, cell=96) for k, sh in enumerate(((0, 0), shift, shift, (0, 0)))]
    feats, qonfs = [v[0] for v in views], [v[1] for v in views]
    tf, tq = [torch.from_numpy(f).cuda() for f in feats], [torch.from_numpy(q).cuda() for q in qonfs]
    rows, shape = [], f"{H} x {W} x {Cc}, subsample {S}"

    def ours(f, q):
        xy1, xy2, sc, info = capi.dense_correspondences(f, q, S, MAX_ITER, return_info=True)
        return (xy1, xy2, sc, info), info["ms"]

    results = {}
    for name, fn in (("host arrays", lambda: ours(feats, qonfs)), ("device tensors", lambda: ours(tf, tq)),
                     ("torch float32, device tensors", lambda: (torch_extract(tf, tq, S), None))):
        res, wall, dev = timed(fn)
        results[name] = res
        rows.append(dict(call="extract_correspondences", shape=shape, path=name, wall_ms=wall, device_ms=dev, rows=len(res[0])))
        print(json.dumps(rows[-1]), flush=True)
    info = results["device tensors"][3]
    assert all(np.array_equal(x, y) for x, y in zip(results["host arrays"][:3], results["device tensors"][:3]))

    # agreement, search by search: float64 with gaps against ours (exact) and against the float32 yardstick (above tau32)
    t64, t32 = NR.tau64(Cc), NR.tau32(Cc)
    below64 = below32 = mismatch_above = seeds = 0
    for A, B in ((tf[0], tf[1]), (tf[1], tf[0]), (tf[3], tf[2]), (tf[2], tf[3])):
        x1, x2, conv, gap = torch_descent(A, B, S, torch.float64, top2=True)
        y1, y2, conv32, _ = torch_descent(A, B, S, torch.float32)
        differ = (x1 != y1) | (x2 != y2) | (conv != conv32)
        seeds += len(x1)
        below64 += int((gap <= t64).sum())
        below32 += int((gap <= t32).sum())
        mismatch_above += int((differ & (gap > t32)).sum())
        p = np.unique(np.stack([x1[conv], x2[conv]], 1), axis=0)
        i1, i2 = capi.reciprocal_nns(A, B, S, MAX_ITER)
        assert below64 > 0 or (np.array_equal(i1, p[:, 0]) and np.array_equal(i2, p[:, 1])), "the float64 descent and the library differ"
    rows.append(dict(call="extract_correspondences", shape=shape, path="agreement", seeds=seeds, seeds_below_tau64=below64, seeds_below_tau32=below32,
                     float32_mismatches_above_tau32=mismatch_above))
    print(json.dumps(rows[-1]), flush=True)

    # what a half-step moves and computes, from the shapes and the counters
    px, strip = H * W, 64
    strips0 = 4 * ((capi.recip_seed_count(H, W, S) + strip - 1) // strip)
    fma = 2.0 * info["nn_queries"] * px * Cc
    rows.append(dict(call="extract_correspondences", shape=shape, path="counts", n_seeds=info["n_seeds"], n_converged=info["n_converged"],
                     iterations=info["iterations"], nn_queries=info["nn_queries"], column_ranges=info["column_ranges"],
                     first_half_step_map_bytes_read=float(strips0) * px * Cc * 4, first_half_step_gathered_bytes=float(info["n_seeds"]) * Cc * 4 * info["column_ranges"],
                     fp64_flop=fma, fp64_tflops=fma / (rows[1]["device_ms"] * 1e-3) / 1e12, fp64_mfma_peak_fraction=fma / (rows[1]["device_ms"] * 1e-3) / 78.6e12))
    print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
