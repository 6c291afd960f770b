"""mpsfm_simple_nms / mpsfm_kpids_to_matches0 / mpsfm_warp_matches (csrc/warp_matches.hip) on the device against the NumPy
restatement (tests/numpy_warp_matches.py) and the fixture computed by the reference's own warp.py.

The rule.  Every decision of these entry points is a comparison of input values, or of float32 / float64 values rounded one
operation at a time, so device and restatement must agree BITWISE on every element of every case; nothing is exempt and there
is no tolerance anywhere in this file."""

import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import numpy_warp_matches as NW
from mpsfm_amd import capi
from mpsfm_amd.extraction.pairwise import warp as WM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "reference_warp_matches.npz"))
TW, TH = 64, 32  # outputs of a k_pool workgroup


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and (np.array_equal(bits(a), bits(b)) if a.dtype == np.float32 else np.array_equal(a, b))


def check_nms(s, r):
    got = capi.simple_nms_map(s, r)
    want = NW.simple_nms(s, r)
    assert got.dtype == np.float32 and got.shape == s.shape
    assert np.array_equal(bits(got), bits(want)), (s.shape, r, np.argwhere(bits(got) != bits(want))[:5])
    return got


def quantised(rng, h, w):
    return (rng.integers(-2, 9, (h, w)) / 8.0).astype(np.float32)


# ---- simple_nms -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [0, 1, 4, 8, 16])
def test_simple_nms_map_sizes_around_the_window_and_the_tile(r):
    sizes = sorted({1, 2, r, r + 1, 2 * r + 1, 63, 64, 65, 127, 128, 129} - {0})
    assert r == 0 or min(sizes) < 2 * r + 1  # maps smaller than the window
    rng = np.random.default_rng(100 + r)
    for h in sizes:
        for w in sizes:
            check_nms(quantised(rng, h, w), r)
    check_nms(rng.random((70, 150)).astype(np.float32), r)  # distinct values: isolated maxima


def test_simple_nms_plateaus_borders_and_constant_maps():
    rng = np.random.default_rng(7)
    for r in (1, 4, 8):
        s = (rng.random((2 * TH + 6, 2 * TW + 2)) * 0.5).astype(np.float32)
        s[TH - 4:TH + 4, TW - 4:TW + 4] = 0.75  # a plateau straddling a tile corner keeps every pixel
        out = check_nms(s, r)
        assert (out[TH - 4:TH + 4, TW - 4:TW + 4] == 0.75).all()
        s = (rng.random((40, 70)) * 0.5).astype(np.float32)
        s[0, 5], s[39, 60], s[17, 0], s[20, 69], s[0, 69], s[39, 0] = 1, 1, 1, 1, 1, 1  # maxima on the border and in the corners
        out = check_nms(s, r)
        assert out[0, 5] == out[39, 60] == out[17, 0] == out[20, 69] == out[0, 69] == out[39, 0] == 1
        for const in (0.5, 0.0, -0.25):
            out = check_nms(np.full((37, 71), const, np.float32), r)
            assert (out == np.float32(const)).all()
        neg = -(rng.random((50, 90)).astype(np.float32)) - np.float32(0.125)  # suppressed pixels become 0, ABOVE every score
        out = check_nms(neg, r)
        assert (out < 0).any() and (out == 0).any()
        mixed = quantised(rng, 50, 90)
        mixed[::7, ::5] *= -1  # -0.0 among the zeros
        check_nms(mixed, r)


def staircase(r, across_rows):
    """A map in which one pixel decides the output 5 r away, found by a search over the flip site: a descending staircase of
    isolated steps r apart on a low background.  With the top step present steps 0, 2, 4 survive (each recovered in one round);
    with it lowered steps 1, 3, 5 do.  Returns (map, flipped map, flip site, the changed pixel farthest from it)."""
    n, edge, axis = 2 * TW + 10, (TH if across_rows else TW), (0 if across_rows else 1)
    for x0 in range(edge - 5 * r - 2, edge):  # the search: the first site whose influence reaches across the tile edge
        line = np.full(n, -1.0, np.float32)
        for k in range(8):
            line[x0 + k * r] = 1.0 - k / 16.0
        flipped = line.copy()
        flipped[x0] = 0.001
        a, b = (line[:, None].copy(), flipped[:, None].copy()) if across_rows else (line[None, :].copy(), flipped[None, :].copy())
        changed = np.argwhere(NW.simple_nms(a, r) != NW.simple_nms(b, r))
        site = np.array([x0, 0] if across_rows else [0, x0])
        assert (np.argwhere(a != b) == site).all() and (a != b).sum() == 1  # one pixel differs
        dist = np.abs(changed - site).max(axis=1)
        far = changed[dist.argmax()]
        if dist.max() > 4 * r and site[axis] < edge <= far[axis]:
            return a, b, site, far
    raise AssertionError("no flip site found")


@pytest.mark.parametrize("across_rows", [False, True])
def test_simple_nms_one_pixel_decides_the_output_five_radii_away_across_a_tile_edge(across_rows):
    r = 4
    a, b, site, far = staircase(r, across_rows)
    assert np.abs(far - site).max() == 5 * r > 4 * r  # asserted on the CPU: a fused variant with a 4 r halo cannot pass
    oa, ob = check_nms(a, r), check_nms(b, r)
    assert oa[tuple(far)] != ob[tuple(far)]


@pytest.mark.parametrize("shape", [(65536 * TH + 37, 1), (1, 65536 * TW + 37), (70000 * TH + 5, 2)])
def test_simple_nms_maps_with_more_tiles_along_an_axis_than_a_grid_dimension_holds(shape):
    rng = np.random.default_rng(shape[0])
    s = quantised(rng, *shape)
    out = check_nms(s, 2)
    assert 0 < (out != 0).sum() < s.size


def test_simple_nms_in_place_on_the_device_is_refused():
    import ctypes as C
    import torch

    L = capi.lib()
    t = torch.rand(80, 70, device="cuda")
    u = torch.empty(81, 70, device="cuda")
    torch.cuda.synchronize()
    assert L.mpsfm_simple_nms(80, 70, t.data_ptr(), 4, 1, None, t.device.index, t.data_ptr(), None) == -1
    assert b"overlap" in L.mpsfm_last_error()
    u[1:] = t
    torch.cuda.synchronize()
    assert L.mpsfm_simple_nms(80, 70, u[1:].data_ptr(), 4, 1, None, t.device.index, u.data_ptr(), None) == -1  # shifted by one row
    assert L.mpsfm_simple_nms(80, 70, t.data_ptr(), 4, 1, None, t.device.index, u.data_ptr(), None) == 0
    assert same(u[:80].cpu().numpy(), NW.simple_nms(t.cpu().numpy(), 4))


@pytest.mark.parametrize("name", ["random", "quantised", "saturated", "negative"])
def test_simple_nms_fixture(name):
    import torch

    s = GOLD[f"nms_{name}"]
    for r in (0, 1, 4, 8):
        want = GOLD[f"nms_{name}_r{r}"]
        assert np.array_equal(bits(capi.simple_nms_map(s, r)), bits(want))
        out = WM.simple_nms(torch.from_numpy(s).cuda(), r)
        assert out.is_cuda and out.dtype == torch.float32 and np.array_equal(bits(out.cpu().numpy()), bits(want))
    out = WM.simple_nms(torch.from_numpy(s), 4)
    assert isinstance(out, torch.Tensor) and not out.is_cuda and np.array_equal(bits(out.numpy()), bits(GOLD[f"nms_{name}_r4"]))


# ---- unique matches -------------------------------------------------------------------------------------------------------
def check_unique(ids0, ids1, scores, n0=None, n1=None):
    ids0, ids1, scores = np.asarray(ids0, np.int64), np.asarray(ids1, np.int64), np.asarray(scores, np.float32)
    m, s, info = capi.kpids_to_matches0_arrays(ids0, ids1, scores, n0, n1, return_info=True)
    rm, rs, keep = NW.kpids_to_matches0(ids0, ids1, scores)
    assert same(m, rm) and same(s, rs), (m, rm)
    assert info["num_matches"] == len(keep) and info["num_valid"] == ((ids0 >= 0) & (ids1 >= 0)).sum()
    return m, s


def test_unique_matches_small_cases():
    m, s = check_unique([3], [5], [0.5])  # a single row; the output is as long as its id + 1
    assert m.tolist() == [-1, -1, -1, 5] and s.tolist() == [0, 0, 0, 0.5]
    m, _ = check_unique([-1, -1, 2], [0, 1, -1], [0.5, 0.25, 1.0])  # no valid row
    assert m.shape == (0,)
    m, _ = check_unique([4] * 9, list(range(9)), [0.1, 0.3, 0.2, 0.9, 0.5, 0.9, 0.0, -1.0, 0.4])  # one ids0 group, a tie at the top
    assert m.tolist() == [-1, -1, -1, -1, 3]
    m, _ = check_unique([0, 1, 1], [0, 0, 1], [0.9, 0.8, 0.7])  # row 1 wins its ids0 group and loses its ids1 group
    assert m.tolist() == [0]
    m, s = check_unique([0, 0, 1, 1, 2, 2], [0, 1, 2, 2, 3, 4], [0.5, 0.5, 0.25, 0.25, -0.0, 0.0])  # ties, -0.0 against +0.0
    assert m.tolist() == [0, 2, 3] and np.signbit(s[2])
    m, s = check_unique([2, 2], [4, 3], [0.0, -0.0])
    assert m.tolist() == [-1, -1, 4] and not np.signbit(s[2])
    m, _ = check_unique([0, 1, 7], [1, 0, -1], [0.5, 0.25, 1.0], n0=9, n1=3)  # trailing unmatched ids: 2 entries, not 9
    assert m.tolist() == [1, 0]
    m, _ = check_unique([0, 8], [1, 2], [0.5, 0.25], n0=9, n1=3)  # the largest id is n0 - 1
    assert m.tolist() == [1] + [-1] * 7 + [2]
    m, _ = check_unique([0, 1], [0, 1], [-3.0, -1e30])  # negative scores are scores like any other
    assert m.tolist() == [0, 1]


def test_unique_matches_groups_across_workgroups_with_ties():
    rng = np.random.default_rng(11)
    n = 300_001
    for n0, n1, levels in ((37, 29, 1 << 20), (37, 29, 5), (1, 40, 3), (2000, 1500, 64)):
        ids0, ids1 = rng.integers(-1, n0, n), rng.integers(-1, n1, n)
        scores = (rng.integers(-levels, levels + 1, n) / np.float32(levels)).astype(np.float32)  # few levels: ties in every group
        m, _ = check_unique(ids0, ids1, scores, n0, n1)
        assert (m >= 0).sum() >= 1
    m, _ = check_unique(ids0, np.zeros(n, np.int64), scores, n0, 1)  # every row in one ids1 group
    assert (m >= 0).sum() == 1


def test_unique_matches_fixture():
    m, s = WM.kpids_to_matches0(GOLD["uniq_ids0"], GOLD["uniq_ids1"], GOLD["uniq_scores"])
    assert same(m, GOLD["uniq_matches0"]) and same(s, GOLD["uniq_scores0"]) and s.dtype == np.float16


# ---- both legs ------------------------------------------------------------------------------------------------------------
def scene(rng, H, W, sizes, ns=200, shift=(0.1, -0.06)):
    """a smooth warp of one scene seen with a shift, a certainty with saturated regions, keypoints near warp rows"""
    x, y = np.meshgrid((np.arange(W) + 0.5) / W * 2 - 1, (np.arange(H) + 0.5) / H * 2 - 1)
    warp = np.stack([x, y, x + shift[0] + 0.02 * np.sin(3 * y), y + shift[1] + 0.02 * np.cos(2 * x)], -1).astype(np.float32)
    cert = np.clip(0.6 + 0.6 * np.sin(5 * x) * np.cos(4 * y), 0, 1)
    cert = (np.round(cert * 64) / 64).astype(np.float32)  # ties among the scores of a group, plateaus for the suppression
    kA, kB = NW.to_pixel_coordinates(warp, *sizes)
    rows = rng.permutation(H * W)[:ns]
    s0 = kA[rows].astype(np.float64) + rng.uniform(-0.7, 0.7, (ns, 2))
    s1 = (kB[rows].astype(np.float64) + rng.uniform(-0.7, 0.7, (ns, 2)))[rng.permutation(ns)]
    return warp, cert, s0, s1


def check_warp(warp, cert, sizes, mode=3, **kw):
    got, info = capi.warp_matches(warp, cert, sizes, mode, return_info=True, **kw)
    want = NW.warp_to_matches(warp, cert, sizes, bool(mode & 1), bool(mode & 2), **kw)
    keys = (["dkeypoints0", "dkeypoints1", "dscores"] if mode & 1 else []) + (["smatches0", "smatching_scores0"] if mode & 2 else [])
    assert sorted(got) == sorted(keys)
    for k in keys:
        assert same(got[k], want[k]), (k, got[k].shape, want[k].shape)
    if mode & 1:
        assert info["num_dense"] == len(want["dscores"])
    if mode & 2 and "ids0" in want:
        assert info["num_valid"] == ((want["ids0"] >= 0) & (want["ids1"] >= 0)).sum()
        assert info["num_matches"] == (want["smatches0"] >= 0).sum()
    return got, want


def test_both_legs_on_a_scene():
    rng = np.random.default_rng(21)
    sizes = (100, 150, 90, 140)
    warp, cert, s0, s1 = scene(rng, 70, 100, sizes)
    for mode in (1, 2, 3):
        got, want = check_warp(warp, cert, sizes, mode, skpts0=s0, skpts1=s1, nms_radius=4)
    assert len(got["dscores"]) > 20 and (got["smatches0"] >= 0).sum() > 50
    valid = ((want["ids0"] >= 0) & (want["ids1"] >= 0)).sum()
    assert valid - (got["smatches0"] >= 0).sum() > 50  # rows that lose their group, many of them through ties
    got, _ = check_warp(warp, cert, sizes, 2, skpts0=s0 * [1.25, 0.75], skpts1=s1 * [2.0, 3.0], scale0=(1.25, 0.75), scale1=(2.0, 3.0))
    assert (got["smatches0"] >= 0).sum() > 50  # non-unit scales
    check_warp(warp, cert, sizes, 2, skpts0=s0[:1], skpts1=s1[:1])
    check_warp(warp[:1, :1], cert[:1, :1], sizes, 3, skpts0=s0, skpts1=s1)  # a single row
    out = capi.warp_matches(warp, cert, sizes, 3, skpts0=s0, skpts1=np.zeros((0, 2)))  # an empty side beside the dense leg
    assert out["smatches0"].shape == (0,) and len(out["dscores"]) > 20


def test_dense_leg_selection_and_order():
    rng = np.random.default_rng(22)
    H, W, sizes = 100, 130, (300, 400, 280, 390)
    warp = (rng.random((H, W, 4)) * 2 - 1).astype(np.float32)
    cert = rng.random((H, W)).astype(np.float32)
    got, _ = check_warp(warp, cert, sizes, 1, nms_radius=0, sample_thresh=-1.0)  # all survivors, in row order across workgroups
    assert len(got["dscores"]) == H * W and np.array_equal(got["dscores"], cert.reshape(-1))
    got, _ = check_warp(warp, cert, sizes, 1, nms_radius=0, sample_thresh=0.5)  # thousands of survivors
    assert 5000 < len(got["dscores"]) < 8000
    got, _ = check_warp(warp, cert, sizes, 1, nms_radius=3, sample_thresh=2.0)  # none
    assert got["dkeypoints0"].shape == (0, 2) and got["dscores"].shape == (0,)
    # a certainty exactly at the threshold is dropped; the threshold is compared as torch does, rounded to float32
    cert[:] = 0.0
    cert[3, 4], cert[50, 60], cert[70, 80], cert[90, 100] = 0.5, np.float32(0.1), np.nextafter(np.float32(0.1), np.float32(1)), 0.75
    got, _ = check_warp(warp, cert, sizes, 1, nms_radius=2, sample_thresh=0.5)
    assert got["dscores"].tolist() == [0.75]
    got, _ = check_warp(warp, cert, sizes, 1, nms_radius=2, sample_thresh=0.1)
    assert got["dscores"].tolist() == [0.5, float(np.nextafter(np.float32(0.1), np.float32(1))), 0.75]
    got, _ = check_warp(warp, -cert, sizes, 1, nms_radius=0, sample_thresh=-0.2)  # negative values above a negative threshold
    assert len(got["dscores"]) == H * W - 2


def test_sparse_leg_boundaries_ties_and_float32_steps():
    sizes = (2000, 2000, 8, 8)
    # row 0: x_A = 3e-8 is lost in fl32(x + 1) = 1, so px is exactly 1000; in float64 it would be 1000.00003
    warp = np.array([[3e-8, 0.0, 0.0, 0.0], [0.5, 0.5, 0.0, 0.0], [-0.5, -0.5, 0.5, 0.5], [-0.25, 0.25, -0.5, -0.5]], np.float32).reshape(2, 2, 4)
    cert = np.array([[0.9, 0.8], [0.7, 0.6]], np.float32)
    kA, kB = NW.to_pixel_coordinates(warp, *sizes)
    assert kA[0].tolist() == [1000.0, 1000.0] and 1000.0 * (float(warp[0, 0, 0]) + 1.0) > 1000.00002
    s0 = np.array([[1002.00001, 1000.0],             # 2.00001 from row 0's float32 pixel (no match), 1.99998 from the float64 one
                   [1502.0, 1500.0],                 # exactly max_error from row 1: no match
                   [501.0, 500.0], [499.0, 500.0],   # equidistant from row 2: the lowest index
                   [750.0, 1251.5]])                 # 1.5 from row 3
    s1 = np.array([[4.0, 4.0], [6.5, 6.0], [2.0, 2.0]])
    got, want = check_warp(warp, cert, sizes, 2, skpts0=s0, skpts1=s1)
    assert want["ids0"].tolist() == [-1, -1, 2, 4] and want["ids1"].tolist() == [0, 0, 1, 2]
    assert got["smatches0"].tolist() == [-1, -1, 1, -1, 2]
    got, want = check_warp(warp, cert, sizes, 2, skpts0=s0, skpts1=s1, max_error=2.0000001)  # just above: rows 0 and 1 find theirs
    assert want["ids0"].tolist() == [-1, 1, 2, 4]
    got, want = check_warp(warp, cert, sizes, 2, skpts0=s0 * 0.5, skpts1=s1 * [3.0, 0.5], scale0=(0.5, 0.5), scale1=(3.0, 0.5), max_error=1.0)
    assert want["ids0"].tolist() == [-1, -1, 2, 4]  # the boundary and the tie scale with the keypoints


def test_both_legs_fixture():
    import torch

    g = {k[5:]: GOLD[k] for k in GOLD.files if k.startswith("roma_")}
    kw = dict(skpts0=g["skpts0"], skpts1=g["skpts1"], scale0=g["scale0"], scale1=g["scale1"], nms_radius=int(g["nms_radius"]),
              sample_thresh=float(g["sample_thresh"]), max_error=float(g["max_error"]))
    sizes = tuple(int(v) for v in g["sizes"])
    check_warp(g["warp"], g["certainty"], sizes, 3, **kw)
    for warp, cert in ((g["warp"], g["certainty"]), (torch.from_numpy(g["warp"]).cuda(), torch.from_numpy(g["certainty"]).cuda())):
        pred = WM.warp_to_matches(warp, cert, sizes, "sparse+dense", **kw)
        for k in ("dkeypoints0", "dkeypoints1", "dscores", "smatches0", "smatching_scores0"):
            assert same(pred[k], g[k]), k
        assert pred["smatching_scores0"].dtype == np.float16 and pred["smatches0"].dtype == np.int32
    assert set(WM.warp_to_matches(g["warp"], g["certainty"], sizes, "dense", **kw)) == {"dkeypoints0", "dkeypoints1", "dscores"}
    from mpsfm_amd.extraction.pairwise import assign_keypoints
    ids0 = assign_keypoints(NW.to_pixel_coordinates(g["warp"], *sizes)[0].astype(np.float64) * g["scale0"], g["skpts0"], kw["max_error"])
    assert np.array_equal(ids0, g["ids0"])


# ---- device tensors -------------------------------------------------------------------------------------------------------
def test_device_tensors_give_what_host_arrays_give():
    import torch

    rng = np.random.default_rng(31)
    sizes = (100, 150, 90, 140)
    warp, cert, s0, s1 = scene(rng, 70, 100, sizes)
    kw = dict(skpts0=s0, skpts1=s1, nms_radius=4)
    want = capi.warp_matches(warp, cert, sizes, 3, **kw)
    want_nms = capi.simple_nms_map(cert, 4)
    tw, tc = torch.from_numpy(warp).cuda(), torch.from_numpy(cert).cuda()
    torch.cuda.synchronize()

    def agree(w, c):
        got = capi.warp_matches(w, c, sizes, 3, **kw)
        assert all(same(got[k], want[k]) for k in want)
        out = capi.simple_nms_map(c, 4)
        assert out.is_cuda and same(out.cpu().numpy(), want_nms)

    agree(tw, tc)
    agree(tw.permute(2, 0, 1).contiguous().permute(1, 2, 0), tc.T.contiguous().T)  # not contiguous on the device
    h = capi.warp_matches(tw.half(), tc.half(), sizes, 3, **kw)  # float16 tensors: what the float16 values give on the host
    hh = capi.warp_matches(warp.astype(np.float16), cert.astype(np.float16), sizes, 3, **kw)
    assert all(same(h[k], hh[k]) for k in hh)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        x = torch.ones(2048, 2048, device="cuda")
        for _ in range(20):
            x = (x @ x) * (1.0 / 2048)  # the stream is busy when the inputs are enqueued
        agree(tw * x[0, 0], tc * x[1, 1])  # x == 1 exactly: written behind the products, just before the call
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        capi.warp_matches(tw, cert, sizes, 1)
    with pytest.raises(ValueError):
        capi.simple_nms_map(tc, 4, device=tc.device.index + 1)


def test_device_inputs_are_scanned():
    import torch

    sizes = (30, 40, 30, 40)
    warp, cert = torch.zeros(9, 70, 4, device="cuda"), torch.full((9, 70), 0.5, device="cuda")
    k = np.ones((3, 2))
    bad_w, bad_c = warp.clone(), cert.clone()
    bad_w[8, 69, 3] = float("nan")
    bad_c[8, 69] = float("inf")
    torch.cuda.synchronize()
    for w, c in ((bad_w, cert), (warp, bad_c)):
        for mode in (1, 2):
            with pytest.raises(capi.MpsfmHipError) as e:
                capi.warp_matches(w, c, sizes, mode, skpts0=k, skpts1=k)
            assert e.value.code == -1
    with pytest.raises(capi.MpsfmHipError) as e:
        capi.simple_nms_map(bad_c, 2)
    assert e.value.code == -1
    assert len(capi.warp_matches(warp, cert, sizes, 1, nms_radius=0)["dscores"]) == 9 * 70


def test_unique_matches_from_device_tensors():
    import torch

    rng = np.random.default_rng(33)
    n, n0, n1 = 70_001, 50, 40
    ids0, ids1 = rng.integers(-1, n0, n), rng.integers(-1, n1, n)
    sc = (rng.integers(0, 17, n) / 16.0).astype(np.float32)
    want = capi.kpids_to_matches0_arrays(ids0, ids1, sc, n0, n1)
    t0, t1, ts = torch.from_numpy(ids0).cuda(), torch.from_numpy(ids1).cuda(), torch.from_numpy(sc).cuda()
    torch.cuda.synchronize()
    got = capi.kpids_to_matches0_arrays(t0, t1, ts, n0, n1)
    assert same(got[0], want[0]) and same(got[1], want[1]) and (want[0] >= 0).sum() > 5
    half = capi.kpids_to_matches0_arrays(ids0, ids1, sc.astype(np.float16), n0, n1)
    # other widths and strided views are converted on the device, on the DEFAULT stream behind a queue of work: the call must see
    # the converted ids (the library's stream does not order itself against the default stream; the wrapper synchronises it)
    x = torch.ones(2048, 2048, device="cuda")
    for _ in range(20):
        x = (x @ x) * (1.0 / 2048)
    wide0, wide1 = torch.stack([t0, t0 + 1], 1).int() * x[0, 0].int(), torch.stack([t1 - 1, t1], 1).int() * x[0, 0].int()
    got = capi.kpids_to_matches0_arrays(wide0[:, 0], wide1[:, 1], ts.half() * x[1, 1].half(), n0, n1)
    assert same(got[0], half[0]) and same(got[1], half[1])
    with pytest.raises(TypeError):
        capi.kpids_to_matches0_arrays(t0.float(), t1, ts, n0, n1)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        x = torch.ones(2048, 2048, device="cuda")
        for _ in range(20):
            x = (x @ x) * (1.0 / 2048)
        got = capi.kpids_to_matches0_arrays(t0 * x[0, 0].long(), t1 * x[0, 0].long(), ts * x[1, 1], n0, n1)  # produced just before the call
    assert same(got[0], want[0]) and same(got[1], want[1])
    torch.cuda.synchronize()
    for bad0, bads in ((n0, 0.5), (-2, 0.5), (3, float("nan"))):  # an id outside -1 .. n0 - 1, a non-finite score
        b0, bs = t0.clone(), ts.clone()
        b0[n - 1], bs[n - 1] = bad0, bads
        torch.cuda.synchronize()
        with pytest.raises(capi.MpsfmHipError) as e:
            capi.kpids_to_matches0_arrays(b0, t1, bs, n0, n1)
        assert e.value.code == -1
    with pytest.raises(ValueError):
        capi.kpids_to_matches0_arrays(t0, ids1, ts, n0, n1)


# ---- determinism ------------------------------------------------------------------------------------------------------------
def test_results_are_identical_run_to_run_and_across_host_threads():
    rng = np.random.default_rng(41)
    sizes = (100, 150, 90, 140)
    warp, cert, s0, s1 = scene(rng, 64, 96, sizes)
    n = 50_000
    ids0, ids1 = rng.integers(-1, 40, n), rng.integers(-1, 30, n)
    sc = (rng.integers(0, 9, n) / 8.0).astype(np.float32)

    def work():
        out = capi.warp_matches(warp, cert, sizes, 3, skpts0=s0, skpts1=s1, nms_radius=4)
        return [out[k] for k in sorted(out)] + list(capi.kpids_to_matches0_arrays(ids0, ids1, sc, 40, 30)) + [capi.simple_nms_map(cert, 8)]

    first = work()
    assert all(same(a, b) for a, b in zip(first, work()))
    res = [None, None]

    def run(slot):
        res[slot] = [work() for _ in range(3)]

    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for rs in res:
        assert rs is not None
        for r in rs:
            assert all(same(a, b) for a, b in zip(first, r))


def test_results_do_not_depend_on_what_the_device_blocks_held():
    env = dict(os.environ, MPSFM_POISON="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_warp_matches_worker.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_info_reports_counts_and_the_device_time():
    rng = np.random.default_rng(51)
    sizes = (100, 150, 90, 140)
    warp, cert, s0, s1 = scene(rng, 40, 60, sizes)
    out, info = capi.warp_matches(warp, cert, sizes, 3, skpts0=s0, skpts1=s1, return_info=True)
    assert info["num_dense"] == len(out["dscores"]) > 0 and info["num_matches"] == (out["smatches0"] >= 0).sum() > 0
    assert info["num_valid"] >= info["num_matches"] and info["ms"] > 0
    _, info = capi.simple_nms_map(cert, 8, return_info=True)
    assert info["ms"] > 0
