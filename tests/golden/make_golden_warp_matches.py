"""Fixture for the warp-to-matches entry points (tests/golden/reference_warp_matches.npz), computed BY THE REFERENCE'S OWN CODE,
loaded by file path:

  mpsfm/extraction/pairwise/models/utils/warp.py     simple_nms, kpids_to_matches0 (get_unique_matches, matches_to_matches0),
                                                     assign_keypoints (SciPy KD-tree)

torch runs on the CPU in float32.  RoMa's to_pixel_coordinates is third-party and not in the tree: the generator writes the
expression `W / 2 * (x + 1)` in torch eager on a float32 tensor, which is the contract.

Cases (every condition a case rests on is asserted here; no row of any case is exempt, a drawn case that violates one is redrawn):
  nms_<map>_r<r>    simple_nms of 48 x 80 maps for r in 0, 1, 4, 8: `random` (smooth + noise), `quantised` (multiples of 1 / 8:
                    plateaus and multi-round chains), `saturated` (a block of 1.0 in a smooth map), `negative` (all below 0).
                    No condition: equality is bitwise.
  uniq_*            kpids_to_matches0 on 3000 rows over 60 x 50 ids with pairwise distinct scores, so no tie rule enters.
  roma_*            both legs of Roma._forward after the network on a 48 x 80 warp of one scene seen with a shift: certainty
                    with pairwise distinct values, 300 sparse keypoints per image, non-unit scale0.  Every query's nearest and
                    second nearest keypoint lie at different distances and no query-keypoint distance is within 1e-6 of
                    max_error, so the KD-tree and an exact fp64 brute force decide alike.  At least 100 matches survive and at
                    least 10 valid rows lose their group.
The file holds inputs and outputs only.

Run in the build container:  python tests/golden/make_golden_warp_matches.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_reference import ROOT, load_by_path  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy_warp_matches as NW  # noqa: E402

RADII = (0, 1, 4, 8)
H, W = 48, 80


def smooth(rng, h, w, k=6):
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    out = np.zeros((h, w))
    for _ in range(k):
        fx, fy, ph = rng.uniform(-0.5, 0.5, 2).tolist() + [rng.uniform(0, 2 * np.pi)]
        out += np.sin(fx * x + fy * y + ph)
    return out / k


def nms_maps(rng):
    rnd = (0.5 + 0.4 * smooth(rng, H, W) + 0.1 * rng.random((H, W))).astype(np.float32)
    quant = (np.round((0.5 + 0.5 * smooth(rng, H, W)) * 8) / 8).astype(np.float32)
    sat = (0.5 + 0.45 * smooth(rng, H, W)).astype(np.float32)
    sat[10:23, 30:52] = 1.0
    neg = (-0.6 + 0.35 * smooth(rng, H, W) - 0.05 * rng.random((H, W))).astype(np.float32)
    assert (neg < 0).all() and (sat <= 1).all() and len(np.unique(quant)) <= 9
    return dict(random=rnd, quantised=quant, saturated=sat, negative=neg)


def distances_ok(q, k, max_error):
    """nearest and second nearest at different distances, nothing within 1e-6 of max_error"""
    d = np.sqrt(((q[:, None, :] - k[None, :, :]) ** 2).sum(-1))
    d.sort(axis=1)
    return (d[:, 0] != d[:, 1]).all() and (np.abs(d - max_error) > 1e-6).all()


def main():
    ref = load_by_path("ref_warp", "mpsfm/extraction/pairwise/models/utils/warp.py")
    rng = np.random.default_rng(20241019)
    out = {}

    for name, m in nms_maps(rng).items():
        out[f"nms_{name}"] = m
        for r in RADII:
            got = ref.simple_nms(torch.from_numpy(m), r).numpy()
            assert got.dtype == np.float32 and got.shape == m.shape
            assert np.array_equal(got.view(np.uint32), NW.simple_nms(m, r).view(np.uint32)), (name, r)
            out[f"nms_{name}_r{r}"] = got
            print("nms", name, r, "kept", int((got != 0).sum()))
        assert (out[f"nms_{name}_r8"] != 0).sum() < (out[f"nms_{name}_r1"] != 0).sum() < H * W

    # rows over ids with pairwise distinct scores
    n, n0, n1 = 3000, 60, 50
    ids0, ids1 = rng.integers(-1, n0, n), rng.integers(-1, n1, n)
    ids0[ids0 == n0 - 1] = -1  # trailing unmatched ids: the output is shorter than n0
    scores = rng.permutation(n).astype(np.float32) / np.float32(4096) - np.float32(0.25)
    assert len(np.unique(scores)) == n and (scores < 0).any()
    m0, s0 = ref.kpids_to_matches0(ids0, ids1, scores)
    rm, rs, keep = NW.kpids_to_matches0(ids0, ids1, scores)
    assert m0.dtype == np.int32 and s0.dtype == np.float16
    assert np.array_equal(m0, rm) and np.array_equal(s0, rs.astype(np.float16)) and 10 <= len(keep) and len(m0) < n0
    out.update(uniq_ids0=ids0, uniq_ids1=ids1, uniq_scores=scores, uniq_matches0=m0, uniq_scores0=s0)
    print("uniq rows", n, "valid", int(((ids0 >= 0) & (ids1 >= 0)).sum()), "kept", len(keep), "length", len(m0))

    # one scene, two views
    sizes = (72, 120, 66, 110)  # H_A, W_A, H_B, W_B: about 1.5 px between neighbouring warp rows
    scale0, scale1, max_error, r, thresh = np.array([1.25, 1.5]), np.array([1.0, 1.0]), 2.0, 8, 0.1
    for attempt in range(50):
        x, y = np.meshgrid((np.arange(W) + 0.5) / W * 2 - 1, (np.arange(H) + 0.5) / H * 2 - 1)
        xb = x + 0.12 + 0.03 * smooth(rng, H, W, 3)
        yb = y - 0.08 + 0.03 * smooth(rng, H, W, 3)
        warp = np.stack([x, y, xb, yb], -1).astype(np.float32)
        cert = np.clip(0.45 + 0.5 * smooth(rng, H, W), 0.0, 1.0) * 0.9 + 0.1 * rng.random((H, W))
        cert = cert.astype(np.float32)
        if len(np.unique(cert)) != H * W:
            continue
        tw = torch.from_numpy(warp).reshape(-1, 4)
        HA, WA, HB, WB = sizes
        kA = torch.stack((WA / 2 * (tw[:, 0] + 1), HA / 2 * (tw[:, 1] + 1)), dim=-1).numpy()
        kB = torch.stack((WB / 2 * (tw[:, 2] + 1), HB / 2 * (tw[:, 3] + 1)), dim=-1).numpy()
        assert kA.dtype == np.float32
        pA, pB = NW.to_pixel_coordinates(warp, *sizes)
        assert np.array_equal(kA, pA) and np.array_equal(kB, pB)
        ns = 300
        rows = rng.permutation(H * W)[:ns]
        s0 = kA[rows].astype(np.float64) * scale0 + rng.uniform(-0.8, 0.8, (ns, 2))
        s1 = kB[rows].astype(np.float64) * scale1 + rng.uniform(-0.8, 0.8, (ns, 2))
        s1[200:] = rng.random((100, 2)) * [WB, HB]  # keypoints of image 1 without counterpart
        s1 = s1[rng.permutation(ns)]
        q0, q1 = kA * scale0, kB * scale1
        assert q0.dtype == np.float64
        if not (distances_ok(q0, s0, max_error) and distances_ok(q1, s1, max_error)):
            continue
        ids0 = ref.assign_keypoints(q0, s0, max_error)
        ids1 = ref.assign_keypoints(q1, s1, max_error)
        assert ids0.max() < ns and ids1.max() < ns and ids0.min() >= -1 and ids1.min() >= -1
        flat = cert.reshape(-1)
        m0, sc0 = ref.kpids_to_matches0(ids0, ids1, flat)
        valid = (ids0 >= 0) & (ids1 >= 0)
        nms = ref.simple_nms(torch.from_numpy(cert), r).reshape(-1)
        sel = nms > thresh
        d0, d1, ds = kA[sel.numpy()], kB[sel.numpy()], nms[sel].numpy()
        matched, lost = int((m0 >= 0).sum()), int(valid.sum()) - int((m0 >= 0).sum())
        print("roma attempt", attempt, "valid", int(valid.sum()), "matches", matched, "lost", lost, "dense", len(ds), "length", len(m0))
        if matched < 100 or lost < 10 or len(ds) < 5:
            continue
        mine = NW.warp_to_matches(warp, cert, sizes, True, True, s0, s1, scale0, scale1, r, thresh, max_error)
        assert np.array_equal(mine["ids0"], ids0) and np.array_equal(mine["ids1"], ids1)
        assert np.array_equal(mine["smatches0"], m0) and np.array_equal(mine["smatching_scores0"].astype(np.float16), sc0)
        assert np.array_equal(mine["dkeypoints0"], d0) and np.array_equal(mine["dkeypoints1"], d1) and np.array_equal(mine["dscores"], ds)
        out.update(roma_warp=warp, roma_certainty=cert, roma_sizes=np.array(sizes), roma_skpts0=s0, roma_skpts1=s1, roma_scale0=scale0,
                   roma_scale1=scale1, roma_max_error=np.array(max_error), roma_nms_radius=np.array(r), roma_sample_thresh=np.array(thresh),
                   roma_ids0=ids0.astype(np.int64), roma_ids1=ids1.astype(np.int64), roma_smatches0=m0, roma_smatching_scores0=sc0,
                   roma_dkeypoints0=d0, roma_dkeypoints1=d1, roma_dscores=ds)
        break
    else:
        raise AssertionError("no draw satisfied the conditions")

    path = os.path.join(HERE, "reference_warp_matches.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: (v.shape, str(v.dtype)) for k, v in out.items()})
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
