"""Times the correspondence-graph build on one input of C5's shape (300 images, 1 M two-view matches plus 30 k
sparse tracks of length clip(2 + Poisson(3), 2, 30)): mpsfm_corr_graph_build from host arrays in to host arrays out, against what the
library offered before it, graph_arrays() over the NumPy stand-in graph of the tests.  Median of 5 after 2 warm-ups, both on this
machine; the two results are compared array by array.  DESIGN.md section 4s quotes the numbers.

    python scripts/time_correspondence_graph.py [--images 300] [--two-view 1000000] [--tracks 30000]
"""

import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mpsfm_amd import capi  # noqa: E402
from mpsfm_amd.sfm.mapper.track_engine import graph_arrays  # noqa: E402
from numpy_scene import NumpyCorrespondenceGraph  # noqa: E402 - the tests' stand-in IS the host path that is compared against

HBM_BYTES_PER_S = 8.0e12  # MI355X peak


def c5_input(n_images, n_two_view, n_tracks, seed=0):
    """kp_start and one match list per image pair: two-view matches between images up to 3 apart, each on two fresh keypoints; tracks
    over windows of consecutive images, every pair of a track's observations a match."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n_images, n_two_view)
    b = (a + rng.integers(1, 4, n_two_view)) % n_images
    k = np.clip(2 + rng.poisson(3.0, n_tracks), 2, min(30, n_images))
    t0 = rng.integers(0, n_images, n_tracks)
    # observations: (image, owner) with a fresh keypoint each; owners 0 .. n_two_view - 1 are the two-view matches
    tr_img = (np.repeat(t0, k) + (np.arange(k.sum()) - np.repeat(np.cumsum(k) - k, k))) % n_images
    obs_img = np.concatenate([a, b, tr_img])
    order = np.argsort(obs_img, kind="stable")
    nkp = np.bincount(obs_img, minlength=n_images)
    kp_start = np.concatenate([[0], np.cumsum(nkp)]).astype(np.int64)
    local = np.empty(len(obs_img), np.int64)
    local[order] = np.arange(len(obs_img)) - np.repeat(kp_start[:-1], nkp)
    ia, ib, ka, kb = [a], [b], [local[:n_two_view]], [local[n_two_view:2 * n_two_view]]
    base, first = 2 * n_two_view, np.cumsum(k) - k
    for L in np.unique(k):
        sel = np.flatnonzero(k == L)
        for i in range(L):
            for j in range(i + 1, L):
                oi, oj = base + first[sel] + i, base + first[sel] + j
                ia.append(obs_img[oi]); ib.append(obs_img[oj]); ka.append(local[oi]); kb.append(local[oj])
    ia, ib, ka, kb = (np.concatenate(x) for x in (ia, ib, ka, kb))
    swap = ia > ib
    ia, ib, ka, kb = np.where(swap, ib, ia), np.where(swap, ia, ib), np.where(swap, kb, ka), np.where(swap, ka, kb)
    key = ia * n_images + ib
    order = np.argsort(key, kind="stable")
    key, m = key[order], np.stack([ka[order], kb[order]], 1).astype(np.int32)
    pairs, start = np.unique(key, return_index=True)
    return kp_start, (pairs // n_images).astype(np.int32), (pairs % n_images).astype(np.int32), np.concatenate([start, [len(m)]]).astype(np.int64), m


def median_ms(fn, warmup=2, runs=5):
    for _ in range(warmup):
        out = fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=300)
    ap.add_argument("--two-view", type=int, default=1_000_000)
    ap.add_argument("--tracks", type=int, default=30_000)
    args = ap.parse_args()
    kp_start, li0, li1, lstart, m = c5_input(args.images, args.two_view, args.tracks)
    n_kp, M, E = int(kp_start[-1]), len(m), 2 * len(m)
    # the host path of the parent commit: the stand-in graph (filled outside the timing) walked by graph_arrays()
    cg = NumpyCorrespondenceGraph()
    nkp = np.diff(kp_start)
    for i in range(args.images):
        cg.add_image(i, int(nkp[i]))
    for l in range(len(li0)):
        cg.add_correspondences(int(li0[l]), int(li1[l]), m[lstart[l]:lstart[l + 1]])
    cam = SimpleNamespace(params=np.array([1200.0, 1200.0, 800.0, 600.0]), model=SimpleNamespace(name="PINHOLE"))
    xy = {i: np.zeros((int(nkp[i]), 2)) for i in range(args.images)}
    scene = SimpleNamespace(images={i: SimpleNamespace(points2D=range(int(nkp[i])), camera_id=0) for i in range(args.images)},
                            keypoints=lambda i: xy[i], rec=SimpleNamespace(cameras={0: cam}))
    host_ms, ga = median_ms(lambda: graph_arrays(cg, scene))
    gpu_ms, g = median_ms(lambda: capi.corr_graph_build(kp_start, li0, li1, lstart, m))
    same = bool(np.array_equal(ga["corr_start"], g["corr_start"]) and np.array_equal(ga["corr_kp"], g["corr_kp"]))
    # bytes the device moves (a model: every kernel's loads and stores, a radix pass per 8 key bits reading and writing key and value)
    kp_bits, im_bits = int(n_kp).bit_length(), int(args.images).bit_length()
    passes1, passes2 = -(-2 * kp_bits // 8), -(-2 * im_bits // 8)
    dev_bytes = (M * (8 + 1 + 4 + 16 + 8) + E * 2 * 12 * passes1 + E * (12 + 4 + 4) + (E + 1) * 8 + E * (12 + 8 + 8 + 16) + (n_kp + 1) * (8 + 4 * 22)
                 + n_kp * 25 + E * 2 * 16 * passes2 + E * 12 + (E + 1) * 8 + E * 12)
    xfer_bytes = m.nbytes + kp_start.nbytes + M + 8 * (n_kp + 1) + 8 * E + n_kp + 8 * M
    info = g["info"]
    print(json.dumps(dict(images=args.images, keypoints=n_kp, matches=M, lists=len(li0), directed_entries=len(g["corr_kp"]), identical=same,
                          host_graph_arrays_ms=round(host_ms, 2), gpu_call_ms=round(gpu_ms, 2), gpu_device_ms=round(info["ms"], 3),
                          launches=info["num_launches"], syncs=info["num_syncs"], device_bytes=int(dev_bytes), transfer_bytes=int(xfer_bytes),
                          hbm_fraction_of_device_time=round(dev_bytes / (info["ms"] * 1e-3) / HBM_BYTES_PER_S, 4),
                          hbm_fraction_of_call=round(dev_bytes / (gpu_ms * 1e-3) / HBM_BYTES_PER_S, 5))))
    if not same:
        raise SystemExit("the two paths disagree")


if __name__ == "__main__":
    main()
