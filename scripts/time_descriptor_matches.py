"""Times the descriptor matcher against the reference's own expression in torch on the same device.

  match_descriptors   4096 x 4096 x 256 and 2048 x 2048 x 24
  NNs_sparse          384 x 512 x 24 maps, 4096 keypoints per side
each from host arrays and from device tensors.  The yardstick is what the reference does per pair, written with torch on
device-resident inputs: einsum + topk(2) forwards and on the transpose + the tests + the mutual check, with grid_sample in
front for the sampled leg.  Medians of 7 calls after 2 warm-ups; wall time ends in a device synchronise, device time is the
call's own HIP-event time (ours: info["ms"]; torch: events around the expression).  Every timed result is compared with the
fp64 restatement (tests/numpy_descriptor_matches.py) on the rows whose margin exceeds the bound of the arithmetic that
produced it.

  python scripts/time_descriptor_matches.py [--out FILE.json] [--quick]
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
import numpy_descriptor_matches as NM  # noqa: E402
from mpsfm_amd import capi  # noqa: E402

WARMUP, CALLS = 2, 7


def planted(rng, n0, n1, dim):
    d1 = rng.normal(size=(n1, dim))
    d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
    d0 = rng.normal(size=(n0, dim))
    m = (2 * min(n0, n1)) // 3
    d0[:m] = d1[rng.permutation(n1)[:m]] + 0.3 * rng.normal(size=(m, dim)) / np.sqrt(dim)
    d0 /= np.linalg.norm(d0, axis=1, keepdims=True)
    s = np.float32(1.0 + 2.0 ** -20)
    return d0.astype(np.float32) / s, d1.astype(np.float32) / s


def torch_find_nn(sim, ratio, distance):
    v, i = sim.topk(2 if ratio else 1, dim=-1)
    dist = 2 * (1 - v)
    ok = torch.ones_like(i[:, 0], dtype=torch.bool)
    if ratio:
        ok &= dist[:, 0] <= ratio ** 2 * dist[:, 1]
    if distance:
        ok &= dist[:, 0] <= distance ** 2
    return torch.where(ok, i[:, 0], -1), torch.where(ok, (v[:, 0] + 1) / 2, 0.0)


def torch_match(d0, d1, ratio=None, distance=None):
    """d0 [n0, D], d1 [n1, D] on the device: the matrix, two top-k passes, the mutual check"""
    sim = torch.einsum("nd,md->nm", d0, d1)
    m0, s0 = torch_find_nn(sim, ratio, distance)
    m1, _ = torch_find_nn(sim.t(), ratio, distance)
    loop = m1.gather(0, m0.clamp(min=0))
    m0 = torch.where((m0 > -1) & (loop == torch.arange(len(m0), device=m0.device)), m0, -1)
    return m0, s0


def torch_sample(m, conf, kps):
    H, W, _ = m.shape
    k = torch.as_tensor(kps, dtype=torch.float32, device=m.device)
    grid = torch.stack([2.0 * k[:, 0] / (W - 1) - 1, 2.0 * k[:, 1] / (H - 1) - 1], -1)[None, :, None]
    d = torch.nn.functional.grid_sample(m.permute(2, 0, 1)[None], grid, align_corners=True, mode="bilinear")[0, :, :, 0].t()
    c = torch.nn.functional.grid_sample(conf[None, None], grid, align_corners=True, mode="bilinear")[0, 0, :, 0]
    return d, c


def torch_nns_sparse(m0, m1, c0, c1, k0, k1, thr):
    d0, s0 = torch_sample(m0, c0, k0)
    d1, s1 = torch_sample(m1, c1, k1)
    m, sc = torch_match(d0, d1)
    m = torch.where(sc < thr, -1, m)
    return m, torch.where(m > -1, torch.sqrt(s0 * s1[m.clamp(min=0)]), 0.0)


def timed(fn, device_ms=None):
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


def agree(m, ref_m, margin, bound):
    sure = margin > bound
    return dict(rows=len(m), below_bound=int((~sure).sum()), mismatches_above_bound=int((np.asarray(m)[sure] != ref_m[sure]).sum()),
                matched=int((ref_m >= 0).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="small shapes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    if not torch.cuda.is_available() or capi.device_count() < 1:
        raise SystemExit("no device: nothing here is measured without one")
    rng = np.random.default_rng(2024)
    rows = []
    shapes = [(4096, 4096, 256), (2048, 2048, 24)] if not a.quick else [(300, 260, 32)]
    for n0, n1, dim in shapes:
        d0, d1 = planted(rng, n0, n1, dim)
        ref_m, _, margin = NM.match_descriptors(d0, d1, 0.9)
        t0, t1 = torch.from_numpy(d0).cuda(), torch.from_numpy(d1).cuda()

        def ours(x, y):
            m, s, info = capi.match_descriptors(x, y, 0.9, return_info=True)
            return m, info["ms"]

        for name, fn, bound in (("host arrays", lambda: ours(d0, d1), NM.tau(dim, NM.TAU64_EPS)),
                                ("device tensors", lambda: ours(t0, t1), NM.tau(dim, NM.TAU64_EPS)),
                                ("torch, device tensors", lambda: (torch_match(t0, t1, 0.9)[0], None), NM.tau(dim, NM.TAU32_EPS))):
            m, wall, dev = timed(fn)
            m = m.cpu().numpy() if hasattr(m, "cpu") else m
            rows.append(dict(call="match_descriptors", shape=f"{n0} x {n1} x {dim}", path=name, wall_ms=wall, device_ms=dev,
                             **agree(m, ref_m, margin, bound)))
            print(json.dumps(rows[-1]), flush=True)
        # what the fused kernel does not move, and how busy the fp64 matrix pipe was
        matrix = 4.0 * n0 * n1
        rows.append(dict(call="match_descriptors", shape=f"{n0} x {n1} x {dim}", path="counts",
                         matrix_bytes_not_written=matrix, torch_bytes_moved_at_least=3 * matrix,  # written once, read by each top-k pass
                         fp64_fma=2.0 * n0 * n1 * dim))
        print(json.dumps(rows[-1]), flush=True)

    H, W, Cc, nk = (384, 512, 24, 4096) if not a.quick else (40, 50, 8, 200)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    fx, fy, ph = rng.uniform(-0.3, 0.3, Cc), rng.uniform(-0.3, 0.3, Cc), rng.uniform(0, 6.28, Cc)

    def view(off):
        f = np.sin(fx * (xx[..., None] + off[0]) + fy * (yy[..., None] + off[1]) + ph)
        f /= np.linalg.norm(f, axis=2, keepdims=True)
        return (f / (1.0 + 2.0 ** -20)).astype(np.float32), (0.6 + 0.3 * np.sin(xx / 70.0) * np.cos(yy / 50.0)).astype(np.float32)

    shift = np.array([W / 8.0 + 0.5, -H / 8.0 + 0.25])
    map0, conf0 = view((0.0, 0.0))
    map1, conf1 = view(shift)
    k0 = rng.random((nk, 2)) * [W - 1, H - 1]
    k1 = np.clip(k0 - shift + rng.normal(0, 0.05, k0.shape), 0, [W - 1, H - 1])[rng.permutation(nk)]
    ref_m, _, margin = NM.nns_sparse(map0, map1, conf0, conf1, k0, k1, 0.85)
    T = [torch.from_numpy(x).cuda() for x in (map0, map1, conf0, conf1)]

    def ours_maps(m0, m1, c0, c1):
        m, s, info = capi.match_map_descriptors(m0, c0, m1, c1, k0, k1, score_threshold=0.85, return_info=True)
        return m, info["ms"]

    for name, fn, bound in (("host arrays", lambda: ours_maps(map0, map1, conf0, conf1), NM.tau(Cc, NM.TAU64_EPS)),
                            ("device tensors", lambda: ours_maps(*T), NM.tau(Cc, NM.TAU64_EPS)),
                            ("torch, device tensors", lambda: (torch_nns_sparse(*T, k0, k1, 0.85)[0], None), 8.0 * Cc * NM.TAU32_EPS * W / 40)):
        m, wall, dev = timed(fn)
        m = m.cpu().numpy() if hasattr(m, "cpu") else m
        rows.append(dict(call="NNs_sparse", shape=f"{H} x {W} x {Cc}, {nk} keypoints", path=name, wall_ms=wall, device_ms=dev,
                         **agree(m, ref_m, margin, bound)))
        print(json.dumps(rows[-1]), flush=True)
    rows.append(dict(call="NNs_sparse", shape=f"{H} x {W} x {Cc}, {nk} keypoints", path="counts",
                     map_bytes_not_copied_with_device_tensors=4.0 * 2 * H * W * (Cc + 1)))
    print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
