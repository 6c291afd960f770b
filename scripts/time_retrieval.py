"""Times retrieval against the reference's own expression in torch on the same device.

  retrieve_topk   2000 x 2000 x 4096, 10000 x 10000 x 4096 and 300 x 300 x 4096, k = 20, one set on both sides with the self mask
each from host arrays and from device tensors.  The yardstick is what the reference does, written with torch float32 on
device-resident inputs (the self mask included): einsum, masked_fill, topk.  Unit descriptors from a clustered generator.  Medians
of 7 calls after 2 warm-ups; wall time ends in a device synchronise, device time is the call's own HIP-event time (ours:
info["ms"]; torch: events around the expression).  Every timed result is compared with the fp64 restatement
(tests/numpy_retrieval.py) on the rows whose margin exceeds the bound of the arithmetic that produced it.  At these sizes the
restatement's similarity loop over k would run for many minutes, so its similarities are formed in fp64 by torch on the device
instead: another association order, within dim 2^-53 of the loop's like the kernel's own, and the margin bound for our results is
doubled for it (8 dim 2^-53).  --quick uses the loop itself.

  python scripts/time_retrieval.py [--out FILE.json] [--quick]
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
import numpy_retrieval as NR  # noqa: E402
from mpsfm_amd import capi  # noqa: E402

WARMUP, CALLS = 2, 7
FP64_MFMA_PEAK = 78.6e12  # FLOP/s


def clustered(rng, n, dim, per_place=25, spread=1.0):
    """unit descriptors of n / per_place places: the images of one place share a direction"""
    places = max(1, n // per_place)
    u = rng.normal(size=(places, dim))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    x = u[rng.integers(0, places, n)] + spread * rng.normal(size=(n, dim)) / np.sqrt(dim)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32) / np.float32(1.0 + 2.0 ** -20)


def torch_retrieval(q, db, invalid, k):
    """the reference's expression: the matrix, the masks, topk; returns (indices, valid)"""
    sim = torch.einsum("id,jd->ij", q, db)
    sim.masked_fill_(invalid | (sim < 0), float("-inf"))
    top = torch.topk(sim, k, dim=1)
    return top.indices, top.values.isfinite()


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


def restated(x, k, ids, quick):
    if quick:
        sim = NR.similarities(x, x)
    else:
        t = torch.from_numpy(x).cuda().double()
        sim = torch.cat([t[i:i + 1000] @ t.T for i in range(0, len(t), 1000)]).cpu().numpy()
    return NR.topk_similarities(sim, k, 0.0, ids, ids)


def agree(idx, cnt, ref_idx, ref_cnt, margin, bound):
    sure = margin > bound
    lists = [idx[i, :cnt[i]].tolist() for i in range(len(cnt))]
    ref = [ref_idx[i, :ref_cnt[i]].tolist() for i in range(len(ref_cnt))]
    return dict(rows=len(cnt), below_bound=int((~sure).sum()), mismatches_above_bound=int(sum(lists[i] != ref[i] for i in np.flatnonzero(sure))),
                pairs=int(ref_cnt.sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="small shapes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    if not torch.cuda.is_available() or capi.device_count() < 1:
        raise SystemExit("no device: nothing here is measured without one")
    rng = np.random.default_rng(2024)
    rows = []
    k = 20
    shapes = [(2000, 4096), (10000, 4096), (300, 4096)] if not a.quick else [(300, 64)]
    for n, dim in shapes:
        x = clustered(rng, n, dim)
        ids = np.arange(n, dtype=np.int32)
        ref_idx, _, ref_cnt, margin = restated(x, k, ids, a.quick)
        t = torch.from_numpy(x).cuda()
        invalid = torch.eye(n, dtype=torch.bool, device="cuda")

        def ours(v):
            idx, _, cnt, info = capi.retrieve_topk(v, v, k, 0.0, ids, ids, return_info=True)
            return (idx, cnt), info["ms"]

        def theirs():
            i, ok = torch_retrieval(t, t, invalid, k)
            return (i, ok), None

        t64 = (1 if a.quick else 2) * NR.tau(dim, NR.TAU64_EPS)
        for name, fn, bound in (("host arrays", lambda: ours(x), t64), ("device tensors", lambda: ours(t), t64),
                                ("torch float32, device tensors", theirs, NR.tau(dim, NR.TAU32_EPS))):
            (idx, cnt), wall, dev = timed(fn)
            if hasattr(idx, "cpu"):  # torch: indices and the valid mask; valid entries come first in a row
                idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy().sum(1)
            rows.append(dict(call="retrieve_topk", shape=f"{n} x {n} x {dim}, k = {k}", path=name, wall_ms=wall, device_ms=dev,
                             **agree(idx, cnt, ref_idx, ref_cnt, margin, bound)))
            if name != "torch float32, device tensors":
                rows[-1]["fp64_mfma_peak_fraction"] = 2.0 * n * n * dim / (dev * 1e-3) / FP64_MFMA_PEAK
            print(json.dumps(rows[-1]), flush=True)
        # what the fused kernel does not move
        rows.append(dict(call="retrieve_topk", shape=f"{n} x {n} x {dim}, k = {k}", path="counts", matrix_bytes_not_written=4.0 * n * n,
                         torch_bytes_moved_at_least=2 * 4.0 * n * n, fp64_fma=1.0 * n * n * dim))  # written once, read by topk
        print(json.dumps(rows[-1]), flush=True)
        del t, invalid
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
