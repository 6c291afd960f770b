"""mpsfm_match_descriptors / mpsfm_match_map_descriptors (csrc/descriptor_matches.hip) on the device against the fp64 restatement
(tests/numpy_descriptor_matches.py) and the fixture computed by the reference's own code.

The rule.  Device and restatement both accumulate fp64 similarities of the same values, in different association orders, so
for descriptors with |d| <= 1 the two differ by at most dim 2^-53 per similarity, and every decision is the same on every row
whose margin (numpy_descriptor_matches.py) exceeds tau64 = 4 dim 2^-53.  On those rows matches must be EQUAL and scores agree
to tau64; every random case asserts that no row lies below tau64, so nothing is exempt.  Tie cases are built from small dyadic
values: all sums are exact, and everything is compared bitwise, on every row."""

import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import numpy_descriptor_matches as NM
from mpsfm_amd import capi
from mpsfm_amd.extraction.pairwise import NearestNeighbor, NNs_sparse

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "reference_descriptor_matches.npz"))
STRIP = 64  # rows of a workgroup and columns of a tile in k_sim_top2


def unit(rng, n, dim):
    x = rng.normal(size=(n, dim))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x = x.astype(np.float32)
    return x / np.float32(1.0 + 2.0 ** -20)  # the float32 rounding may leave a norm above 1


def planted(rng, n0, n1, dim, noise=0.15):
    """unit descriptors: the first min(n0, n1) * 2 / 3 rows of both sets are noisy copies of each other (shuffled), the rest have
    no counterpart"""
    d1 = unit(rng, n1, dim).astype(np.float64)
    d0 = unit(rng, n0, dim).astype(np.float64)
    m = (2 * min(n0, n1)) // 3
    cols = rng.permutation(n1)[:m]
    d0[:m] = d1[cols] + noise * rng.normal(size=(m, dim)) / np.sqrt(dim)
    d0 /= np.linalg.norm(d0, axis=1, keepdims=True)
    return (d0.astype(np.float32) / np.float32(1.0 + 2.0 ** -20)), d1.astype(np.float32)


def dyadic(rng, n, dim, lo=-4, hi=4):
    return (rng.integers(lo, hi + 1, (n, dim)) / 8.0).astype(np.float32)


def check(d0, d1, exact=False, **kw):
    got_m, got_s = capi.match_descriptors(d0, d1, **kw)
    m, s, margin = NM.match_descriptors(d0, d1, **kw)
    assert got_m.dtype == np.int64 and got_m.shape == m.shape and got_s.shape == s.shape
    if exact:
        assert np.array_equal(got_m, m), np.flatnonzero(got_m != m)[:10]
        assert np.array_equal(got_s, s)
    else:
        t = NM.tau(d0.shape[1], NM.TAU64_EPS)
        assert (margin > t).all(), (margin.min(), t)
        assert np.array_equal(got_m, m), np.flatnonzero(got_m != m)[:10]
        assert np.abs(got_s - s).max() <= t
    return got_m, got_s


OPTION_SETS = [dict(), dict(ratio_threshold=0.8), dict(ratio_threshold=0.9, distance_threshold=0.7), dict(do_mutual_check=False),
               dict(ratio_threshold=0.9, do_mutual_check=False)]


# ---- shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0,n1", [(1, 1), (1, 2), (2, 1), (1, 65), (65, 1), (2, 2), (15, 17), (16, 16), (17, 15), (63, 65), (64, 64),
                                   (65, 63), (2 * STRIP - 1, 2 * STRIP + 1), (2 * STRIP, 2 * STRIP), (2 * STRIP + 1, 2 * STRIP - 1)])
def test_set_sizes_around_the_tile_and_the_strip(n0, n1):
    rng = np.random.default_rng(1000 * n0 + n1)
    d0, d1 = planted(rng, n0, n1, 24)
    for kw in OPTION_SETS:
        check(d0, d1, **kw)
    e0, e1 = dyadic(rng, n0, 24), dyadic(rng, n1, 24)
    for kw in OPTION_SETS[:3]:
        check(e0, e1, exact=True, **kw)


def test_a_thousand_by_thirteen_hundred():
    rng = np.random.default_rng(7)
    d0, d1 = planted(rng, 1000, 1300, 24)
    for kw in OPTION_SETS[1:4]:
        m, _ = check(d0, d1, **kw)
        assert 100 < (m >= 0).sum() < 1000 or not kw.get("do_mutual_check", True)


# ---- several column tiles per workgroup ------------------------------------------------------------------------------------
# Up to a few thousand descriptors every workgroup of k_sim_top2 gets ONE column tile (the tiles of a strip are shared out
# until the device is full), so the running top-2 carried across tiles, the accumulator reset and the barrier between the
# last slice of a tile and the first of the next only run at the sizes below.  info["column_ranges"] tells how many
# workgroups shared a strip; each case asserts that a range held more than one tile.
def tiles_per_range(n_cols, info):
    tiles = -(-n_cols // STRIP)
    per = -(-tiles // info["column_ranges"])
    return tiles, per


def check_sim(d0, d1, sim, exact, **kw):
    """check() against similarities computed once for all option sets of a case"""
    got_m, got_s, info = capi.match_descriptors(d0, d1, return_info=True, **kw)
    m, s, margin = NM.match_similarities(sim, kw.get("ratio_threshold"), kw.get("distance_threshold"), kw.get("do_mutual_check", True))
    if not exact:
        t = NM.tau(d0.shape[1], NM.TAU64_EPS)
        assert (margin > t).all(), (margin.min(), t)
    assert np.array_equal(got_m, m), np.flatnonzero(got_m != m)[:10]
    assert np.array_equal(got_s, s) if exact else np.abs(got_s - s).max() <= t
    return got_m, got_s, info


def test_two_tiles_per_workgroup_with_planted_neighbours_and_duplicates():
    rng = np.random.default_rng(61)
    n, dim = 36 * STRIP + 26, 8  # 37 tiles: ranges of two tiles and a last range of one, partial, tile
    d0, d1 = dyadic(rng, n, dim), dyadic(rng, n, dim)
    for d in (d0, d1):  # nothing random comes within 1.875 of a vector of eight +-0.5 (length^2 2)
        d[(np.abs(d) == 0.5).sum(1) >= 7] *= 0.5
    span = 2 * STRIP
    best, second = [], []
    for i in range(36):  # row i: the nearest and the second nearest column in the two tiles of range i % 18, in either order
        u = np.array([0.5 if (i >> k) & 1 else -0.5 for k in range(dim)], np.float32)
        lo, hi = span * (i % 18) + i // 18, span * (i % 18) + STRIP + 7 + i // 18
        b, sc = (lo, hi) if i % 2 == 0 else (hi, lo)
        d0[i], d1[b], d1[sc] = u, u, u * np.array([1, 1, 1, 1, 1, 1, 1, 0.5], np.float32)  # similarities 2 and 1.875
        best.append(b)
        second.append(sc)
    v = np.full(dim, 0.5, np.float32)  # duplicates across the tile edge inside range 5, and in the last range
    dup = [span * 5 + STRIP - 1, span * 5 + STRIP, n - 10]
    for c in dup:
        d0[c], d1[c] = v, v
    sim = NM.similarities(d0, d1)
    rest = sim[:36].copy()
    assert rest.argmax(1).tolist() == best
    rest[np.arange(36), best] = -np.inf
    assert rest.argmax(1).tolist() == second and (rest.max(1) == 1.875).all()
    m, _, info = check_sim(d0, d1, sim, True)
    tiles, per = tiles_per_range(n, info)
    assert tiles == 37 and per == 2 and tiles % per == 1, info  # premise of the case: it holds on a device of 256 compute units
    assert m[:36].tolist() == best
    assert m[dup].tolist() == [dup[0], -1, -1]  # the lowest index wins in both directions
    for kw in (dict(ratio_threshold=0.9), dict(ratio_threshold=0.9, distance_threshold=1.2)):
        check_sim(d0, d1, sim, True, **kw)
    fm, _, _ = check_sim(d0, d1, sim, True, do_mutual_check=False)  # one tile per workgroup again: the same forward answer
    assert fm[:36].tolist() == best and fm[dup].tolist() == [dup[0]] * 3


def test_three_tiles_per_workgroup_in_one_direction():
    rng = np.random.default_rng(62)
    n = 65 * STRIP + 40  # 66 tiles
    e0, e1 = dyadic(rng, n, 4), dyadic(rng, n, 4)
    _, _, info = check_sim(e0, e1, NM.similarities(e0, e1), True, do_mutual_check=False)  # ties everywhere: the lowest index
    tiles, per = tiles_per_range(n, info)
    assert tiles == 66 and per == 3, info  # premise of the case: it holds on a device of 256 compute units
    d0, d1 = planted(rng, n, n, 8)
    sim = NM.similarities(d0, d1)
    m, _, _ = check_sim(d0, d1, sim, False, do_mutual_check=False)
    check_sim(d0, d1, sim, False, ratio_threshold=0.9, do_mutual_check=False)
    assert (m >= 0).all()


@pytest.mark.parametrize("dim", [1, 3, 4, 5, 24, 63, 64, 65, 256, 257, 1024])
def test_descriptor_lengths_around_the_step_and_the_slice(dim):
    rng = np.random.default_rng(dim)
    hi = 4 if dim <= 64 else 1  # |sim| stays far below 2^53 / 64: every sum exact
    e0, e1 = dyadic(rng, 70, dim, -hi, hi), dyadic(rng, 67, dim, -hi, hi)
    check(e0, e1, exact=True)
    check(e0, e1, exact=True, ratio_threshold=0.9, distance_threshold=1.2)
    if dim >= 3:
        d0, d1 = planted(rng, 70, 67, dim)
        check(d0, d1)
        check(d0, d1, ratio_threshold=0.9, distance_threshold=0.7)


# ---- where the best and the second best sit ---------------------------------------------------------------------------------
def with_neighbours(rng, n0, n1, dim, best, second):
    """row i of set 0 is nearest to column best[i] and second nearest to column second[i]"""
    d1 = unit(rng, n1, dim).astype(np.float64)
    d0 = np.zeros((n0, dim))
    for i in range(n0):
        v = d1[best[i]] + 0.8 * d1[second[i]] + 0.01 * rng.normal(size=dim)
        d0[i] = v / np.linalg.norm(v)
    return (d0.astype(np.float32) / np.float32(1.0 + 2.0 ** -20)), d1.astype(np.float32)


@pytest.mark.parametrize("name,n1,best,second", [
    ("best in the last partial tile", STRIP + 5, lambda i: STRIP + i % 5, lambda i: i % STRIP),
    ("best and second in different tiles", 3 * STRIP + 9, lambda i: i % STRIP, lambda i: 2 * STRIP + (i * 7) % (STRIP + 9)),
    ("best and second in one lane", 2 * STRIP, lambda i: i % 16, lambda i: i % 16 + 16 * (1 + i % 3)),
    ("best and second in one 16-lane group", 2 * STRIP, lambda i: 16 + i % 15, lambda i: 16 + i % 15 + 1),
    ("second before best", 2 * STRIP + 3, lambda i: STRIP + 2 + i % 60, lambda i: i % 50),
])
def test_best_and_second_best_in_chosen_places(name, n1, best, second):
    rng = np.random.default_rng(len(name))
    n0 = 40
    b, s = [best(i) for i in range(n0)], [second(i) for i in range(n0)]
    d0, d1 = with_neighbours(rng, n0, n1, 128, b, s)
    m, _ = check(d0, d1, do_mutual_check=False)
    assert m.tolist() == b
    sim = NM.similarities(d0, d1)
    sim[np.arange(n0), b] = -np.inf
    assert sim.argmax(1).tolist() == s  # the construction holds: the ratio test below reads that column
    for kw in OPTION_SETS[1:]:
        check(d0, d1, **kw)


def test_duplicates_across_a_tile_edge_and_a_strip_edge_go_to_the_lowest_index():
    rng = np.random.default_rng(5)
    n0, n1, dim = 2 * STRIP + 6, 3 * STRIP + 8, 16
    d0, d1 = dyadic(rng, n0, dim), dyadic(rng, n1, dim)
    v = np.zeros(dim, np.float32)
    v[:8] = 0.5  # longer than every other descriptor's projection on it can reach: |v|^2 = 2
    for c in (10, STRIP - 1, STRIP, 2 * STRIP + 70):
        d1[c] = v
    for r in (STRIP - 1, STRIP, 2 * STRIP + 3):
        d0[r] = v
    # bounded so that v . v = 2 beats every other similarity with v
    d0[np.abs(d0 @ v) >= 2] *= 0.5
    d1[np.abs(d1 @ v) >= 2] *= 0.5
    for c in (10, STRIP - 1, STRIP, 2 * STRIP + 70):
        d1[c] = v
    for r in (STRIP - 1, STRIP, 2 * STRIP + 3):
        d0[r] = v
    m, s = check(d0, d1, exact=True, do_mutual_check=False)
    assert m[STRIP - 1] == 10 and m[STRIP] == 10 and m[2 * STRIP + 3] == 10
    m, s = check(d0, d1, exact=True)  # reverse direction: column 10's nearest rows tie, the lowest is STRIP - 1
    assert m[STRIP - 1] == 10 and m[STRIP] == -1 and m[2 * STRIP + 3] == -1
    mr, _ = check(d1, d0, exact=True, do_mutual_check=False)
    assert mr[10] == STRIP - 1 and mr[STRIP - 1] == STRIP - 1 and mr[STRIP] == STRIP - 1 and mr[2 * STRIP + 70] == STRIP - 1
    check(d0, d1, exact=True, ratio_threshold=0.9)  # top-2 of a duplicated best is its twin: dist0 == dist1 fails ratio < 1


def test_all_similarities_negative():
    rng = np.random.default_rng(6)
    d0 = (rng.integers(1, 5, (70, 12)) / 8.0).astype(np.float32)
    d1 = -(rng.integers(1, 5, (90, 12)) / 8.0).astype(np.float32)
    m, s = check(d0, d1, exact=True, do_mutual_check=False)
    assert (m >= 0).all() and (s < 0.5).all()
    check(d0, d1, exact=True)
    check(d0, d1, exact=True, ratio_threshold=0.95)


def test_ratio_and_distance_tests_include_their_boundary():
    e = np.float32(2.0 ** -20)

    def sets(sim0, sim1):
        d0 = np.array([[1, 0, 0, 0], [0, 0, 0, 1]], np.float32)
        d1 = np.array([[sim0, 0, 0, 0], [sim1, 0, 0, 0], [0, 0, 0, 0.25]], np.float32)
        return d0, d1

    # dist0 = 2 (1 - 0.75) = 0.5 = 0.25 * 2 (1 - 0)
    m, s = check(*sets(0.75, 0.0), exact=True, ratio_threshold=0.5, do_mutual_check=False)
    assert m[0] == 0 and s[0] == 0.875
    m, s = check(*sets(np.float32(0.75) - e, 0.0), exact=True, ratio_threshold=0.5, do_mutual_check=False)
    assert m[0] == -1 and s[0] == 0.0
    # dist0 = 2 (1 - 0.875) = 0.25 = 0.5^2
    m, s = check(*sets(0.875, 0.0), exact=True, distance_threshold=0.5, do_mutual_check=False)
    assert m[0] == 0 and s[0] == 0.9375
    m, s = check(*sets(np.float32(0.875) - e, 0.0), exact=True, distance_threshold=0.5, do_mutual_check=False)
    assert m[0] == -1 and s[0] == 0.0
    # a single descriptor on the other side: the ratio test is skipped, as in the reference
    d0, d1 = sets(0.75, 0.0)
    m, _ = check(d0, d1[:1], exact=True, ratio_threshold=0.1, do_mutual_check=False)
    assert m.tolist() == [0, 0]
    m, _ = check(d0[:1], d1, exact=True, ratio_threshold=0.1)
    assert m.tolist() == [0]


def test_the_mutual_check_removes_a_match_and_leaves_its_score():
    d0 = np.array([[1, 0], [0.5, 0], [0, 1]], np.float32)
    d1 = np.array([[1, 0], [0, 0.5]], np.float32)
    m, s = check(d0, d1, exact=True)
    assert m.tolist() == [0, -1, 1] and s.tolist() == [1.0, 0.75, 0.75]
    m, s = check(d0, d1, exact=True, do_mutual_check=False)
    assert m.tolist() == [0, 0, 1]
    m, s = capi.match_descriptors(d0, d1, score_threshold=0.8)  # the score threshold removes matches and keeps scores too
    assert m.tolist() == [0, -1, -1] and s.tolist() == [1.0, 0.75, 0.75]


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
DESC_CASES = ["plain", "ratio", "ratio_distance", "no_mutual"]


def case_options(case):
    o = {}
    if float(GOLD[f"{case}_ratio"]) > 0:
        o["ratio_threshold"] = float(GOLD[f"{case}_ratio"])
    if float(GOLD[f"{case}_distance"]) > 0:
        o["distance_threshold"] = float(GOLD[f"{case}_distance"])
    o["do_mutual_check"] = bool(GOLD[f"{case}_mutual"])
    return o


@pytest.mark.parametrize("case", DESC_CASES)
def test_descriptor_fixture(case):
    d0, d1 = GOLD["desc0"].astype(np.float32), GOLD["desc1"].astype(np.float32)
    kw = case_options(case)
    m, s = check(d0, d1, **kw)
    _, _, margin = NM.match_descriptors(d0, d1, **kw)
    t32 = NM.tau(d0.shape[1], NM.TAU32_EPS)
    sure = margin > t32
    assert sure.mean() >= 0.99
    assert np.array_equal(m[sure], GOLD[f"{case}_matches0"][sure])
    assert np.abs(s - GOLD[f"{case}_scores0"])[sure].max() <= t32
    # the class, batch of two, torch in and out
    import torch

    nn = NearestNeighbor({k: v for k, v in kw.items()})
    data = {"descriptors0": torch.from_numpy(np.stack([d0.T, d0.T[:, ::-1].copy()])),
            "descriptors1": torch.from_numpy(np.stack([d1.T, d1.T]))}
    out = nn(data)
    assert isinstance(out["matches0"], torch.Tensor) and out["matches0"].dtype == torch.int64 and out["matches0"].shape == (2, len(d0))
    assert np.array_equal(out["matches0"][0].numpy(), m) and np.array_equal(out["matches0"][1].numpy(), m[::-1])
    assert np.array_equal(out["matching_scores0"][0].numpy(), s)
    half = nn({"descriptors0": d0.T[None].astype(np.float16), "descriptors1": d1.T[None].astype(np.float16)})
    assert isinstance(half["matches0"], np.ndarray) and np.array_equal(half["matches0"][0], m)  # the fixture's values are float16 values


def test_sampled_fixture():
    g = {k: GOLD[f"maps_{k}"] for k in ("map0", "map1", "conf0", "conf1", "kps0", "kps1", "matches0", "scores0")}
    thr = float(GOLD["maps_scores_thresh"])
    m, s = NNs_sparse(g["map0"], g["map1"], g["conf0"], g["conf1"], g["kps0"], g["kps1"], thr)
    rm, rs, margin = NM.nns_sparse(g["map0"], g["map1"], g["conf0"], g["conf1"], g["kps0"], g["kps1"], thr)
    C = g["map0"].shape[2]
    assert (margin > NM.tau(C, NM.TAU64_EPS)).all()
    assert np.array_equal(m, rm) and np.allclose(s, rs, rtol=2.0 ** -50, atol=0)
    sure = margin > 8.0 * C * NM.TAU32_EPS
    assert sure.mean() >= 0.99
    assert np.array_equal(m[sure], g["matches0"][sure])
    both = sure & (m >= 0)
    assert np.abs(s - g["scores0"])[both].max() <= 8.0 * C * NM.TAU32_EPS


# ---- sampling ---------------------------------------------------------------------------------------------------------------
def unit_maps(rng, H, W, C):
    m = rng.normal(size=(H, W, C))
    m /= np.linalg.norm(m, axis=2, keepdims=True)
    return (m.astype(np.float32) / np.float32(1.0 + 2.0 ** -20)), rng.random((H, W)).astype(np.float32)


def check_maps(map0, conf0, map1, conf1, k0, k1, thr=None, duplicates=False, **kw):
    """duplicates: the case holds keypoints with bitwise equal samples (the same float32 pixel, zero padding).  Their similarities
    tie bitwise on the device as in the restatement, the margin of the rows they decide is exactly 0, and the lowest index must
    win: such rows are compared like all others, and no row may lie between 0 and tau64."""
    m, s = capi.match_map_descriptors(map0, conf0, map1, conf1, k0, k1, score_threshold=thr, **kw)
    rm, rs, margin = NM.nns_sparse(map0, map1, conf0, conf1, k0, k1, thr, **kw)
    t = NM.tau(map0.shape[2], NM.TAU64_EPS)
    assert ((margin > t) | (duplicates & (margin == 0.0))).all()
    assert np.array_equal(m, rm), np.flatnonzero(m != rm)[:10]
    assert np.allclose(s, rs, rtol=2.0 ** -50, atol=0)
    return m, s


def test_keypoints_on_pixels_feed_the_double_path_the_float_path_s_values():
    rng = np.random.default_rng(21)
    map0, conf0 = unit_maps(rng, 9, 11, 24)
    map1, conf1 = unit_maps(rng, 10, 8, 24)
    map1[:6, :8] = map0[3:9, 2:10] + np.float32(0.01) * rng.normal(size=(6, 8, 24)).astype(np.float32)
    k0 = np.stack(np.meshgrid(np.arange(11.0), np.arange(9.0)), -1).reshape(-1, 2)   # every pixel, last row and column included
    k1 = np.stack(np.meshgrid(np.arange(8.0), np.arange(10.0)), -1).reshape(-1, 2)
    for kw in (dict(), dict(ratio_threshold=0.9), dict(do_mutual_check=False)):
        m, s = check_maps(map0, conf0, map1, conf1, k0, k1, **kw)
        fm, _ = capi.match_descriptors(map0.reshape(-1, 24), map1.reshape(-1, 24), **kw)  # the samples ARE the pixels
        assert np.array_equal(m, fm) and (m >= 0).sum() > 20
        ok = m >= 0
        assert np.array_equal(s[ok], np.sqrt(conf0.reshape(-1).astype(np.float64)[ok] * conf1.reshape(-1).astype(np.float64)[m[ok]]))


def test_keypoints_between_pixels_on_the_border_outside_and_changed_by_float32_rounding():
    rng = np.random.default_rng(22)
    H, W, C = 12, 14, 8
    map0, conf0 = unit_maps(rng, H, W, C)
    map1, conf1 = map0.copy(), conf0.copy()
    inner = rng.random((150, 2)) * [W - 1, H - 1]
    border = np.array([[W - 1, 3.3], [4.7, H - 1], [W - 1, H - 1], [0, 0], [W - 1 - 1e-9, H - 1 - 1e-9], [W - 0.5, 2.0], [3.0, H - 0.25]])
    outside = np.array([[-0.5, 3.0], [-1.0, -1.0], [-7.0, 2.0], [W + 0.5, 1.0], [3.0, H + 2.0], [1e6, 1e6], [-1e30, 4.0]])
    k0 = np.concatenate([inner, border, outside])
    assert (k0.astype(np.float32).astype(np.float64) != k0).any(axis=1).sum() > 100  # float64 keypoints that float32 rounding moves
    k1 = np.concatenate([inner[::-1] + rng.normal(0, 0.01, inner.shape), border, outside[:3]])
    got = NM.sample_map(map0, k0)
    assert (got[-5:] == 0).all() and (got[len(inner) + 5] != 0).any() and (got[len(inner) + len(border)] != 0).any()
    for thr in (0.85, None):
        m, s = check_maps(map0, conf0, map1, conf1, k0, k1, thr, duplicates=True)
    assert 50 < (m >= 0).sum()
    assert m[len(inner) + 2] == len(inner) + 2 and m[len(inner) + 4] == -1  # two keypoints on one float32 pixel: the lower index keeps the match
    check_maps(map0, conf0, map1, conf1, k0[:1], k1[:1], 0.85)  # a single keypoint per side: defined here
    check_maps(map0[:2, :2], conf0[:2, :2], map1, conf1, k0[:5], k1, duplicates=True)  # the smallest map


# ---- device tensors -------------------------------------------------------------------------------------------------------
def test_device_tensors_give_what_host_arrays_give():
    import torch

    rng = np.random.default_rng(31)
    d0, d1 = planted(rng, 300, 340, 128)
    kw = dict(ratio_threshold=0.9)
    hm, hs = capi.match_descriptors(d0, d1, **kw)
    t0, t1 = torch.from_numpy(d0).cuda(), torch.from_numpy(d1).cuda()
    torch.cuda.synchronize()
    for a, b in ((t0, t1), (t0.half().float().half(), t1.half().float().half())):
        if a.dtype == torch.float16:
            hm, hs = capi.match_descriptors(d0.astype(np.float16), d1.astype(np.float16), **kw)
        m, s = capi.match_descriptors(a, b, **kw)
        assert np.array_equal(m, hm) and np.array_equal(s, hs)
    hm, hs = capi.match_descriptors(d0, d1, **kw)
    # not contiguous on the device, (b, D, N) through the class, results as device tensors
    out = NearestNeighbor(kw)({"descriptors0": t0.T[None], "descriptors1": t1.T[None]})
    assert out["matches0"].is_cuda and np.array_equal(out["matches0"][0].cpu().numpy(), hm)
    assert np.array_equal(out["matching_scores0"][0].cpu().numpy(), hs)
    # produced on the caller's stream immediately before the call
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        w = torch.ones(2048, 2048, device="cuda")
        for _ in range(20):
            w = (w @ w) * (1.0 / 2048)  # the stream is busy when the descriptors are enqueued
        a = t0 * w[0, 0]  # w == 1 exactly: a == t0, written behind the products
        b = t1 * w[1, 1]
        m, s = capi.match_descriptors(a, b, **kw)
    assert np.array_equal(m, hm) and np.array_equal(s, hs)
    torch.cuda.synchronize()
    # maps
    map0, conf0 = unit_maps(rng, 20, 24, 24)
    map1, conf1 = map0[::-1].copy(), conf0[::-1].copy()
    # near pixel centres, where the samples of a map with independent pixels keep a norm close to 1 and pass the score threshold
    k0 = np.stack([rng.integers(0, 24, 200), rng.integers(0, 20, 200)], 1) + rng.uniform(-0.04, 0.04, (200, 2))
    k1 = np.stack([rng.integers(0, 24, 220), rng.integers(0, 20, 220)], 1) + rng.uniform(-0.04, 0.04, (220, 2))
    k1[:150] = k0[:150] * [1, -1] + [0, 19]
    hm, hs = NNs_sparse(map0, map1, conf0, conf1, k0, k1)
    tm0, tm1 = torch.from_numpy(map0).cuda(), torch.from_numpy(map1).cuda()
    tc0, tc1 = torch.from_numpy(conf0).cuda(), torch.from_numpy(conf1).cuda()
    torch.cuda.synchronize()
    m, s = NNs_sparse(tm0, tm1, tc0, tc1, k0, k1)
    assert np.array_equal(m, hm) and np.array_equal(s, hs) and (m >= 0).sum() > 50
    m, s = NNs_sparse(tm0.permute(2, 0, 1).contiguous().permute(1, 2, 0), tm1, tc0, tc1, k0, k1)  # channel-first in memory
    assert np.array_equal(m, hm) and np.array_equal(s, hs)
    with torch.cuda.stream(side):
        m, s = NNs_sparse(tm0 * w[0, 0], tm1 * w[0, 0], tc0 * w[0, 0], tc1 * w[0, 0], k0, k1)
    assert np.array_equal(m, hm) and np.array_equal(s, hs)
    torch.cuda.synchronize()


def test_device_inputs_are_scanned_and_checked():
    import torch

    d = torch.zeros(70, 8, device="cuda")
    d[69, 7] = float("nan")
    ok = torch.ones(5, 8, device="cuda")
    torch.cuda.synchronize()
    for a, b in ((d, ok), (ok, d)):
        with pytest.raises(capi.MpsfmHipError) as e:
            capi.match_descriptors(a, b)
        assert e.value.code == -1
    with pytest.raises(ValueError):
        capi.match_descriptors(ok, np.ones((5, 8), np.float32))
    with pytest.raises(TypeError):
        capi.match_descriptors(ok.double(), ok.double())
    with pytest.raises(ValueError):  # the tensors' own device is used: naming another one is refused, not overridden
        capi.match_descriptors(ok, ok, device=ok.device.index + 1)
    m, _ = capi.match_descriptors(ok, ok, device=ok.device.index)
    assert m.shape == (5,)


# ---- determinism ------------------------------------------------------------------------------------------------------------
def test_results_are_identical_run_to_run_and_across_host_threads():
    rng = np.random.default_rng(41)
    d0, d1 = planted(rng, 500, 450, 64)
    map0, conf0 = unit_maps(rng, 16, 16, 24)
    k0, k1 = rng.random((300, 2)) * 15, rng.random((310, 2)) * 15

    def work():
        return capi.match_descriptors(d0, d1, ratio_threshold=0.9) + capi.match_map_descriptors(map0, conf0, map0, conf0, k0, k1, 0.5)

    first = work()
    assert all(np.array_equal(a, b) for a, b in zip(first, work()))
    out = [None, None]

    def run(slot):
        out[slot] = [work() for _ in range(3)]

    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for res in out:
        assert res is not None
        for r in res:
            assert all(np.array_equal(a, b) for a, b in zip(first, r))


def test_results_do_not_depend_on_what_the_device_blocks_held():
    env = dict(os.environ, MPSFM_POISON="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_descriptor_matches_worker.py")], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_info_reports_the_matches_and_the_device_time():
    rng = np.random.default_rng(51)
    d0, d1 = planted(rng, 130, 140, 24)
    m, _, info = capi.match_descriptors(d0, d1, return_info=True)
    assert info["num_matches"] == (m >= 0).sum() > 0 and info["ms"] > 0
