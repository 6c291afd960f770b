"""mpsfm_retrieve_topk (csrc/retrieval.hip, csrc/sim_topk.h) on the device against the fp64 restatement (tests/numpy_retrieval.py)
and the fixture computed by the reference's own code.

The rule.  Device and restatement both accumulate fp64 similarities of the same values, in different association orders, so for
descriptors with |d| <= 1 the two differ by at most dim 2^-53 per similarity, and every list is the same on every row whose margin
(numpy_retrieval.py) exceeds tau64 = 4 dim 2^-53.  On those rows indices and counts must be EQUAL and scores agree to tau64; every
random case asserts that no row lies below tau64, so nothing is exempt.  Tie cases are built from small dyadic values: all sums are
exact, and everything is compared bitwise, on every row."""

import importlib
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import numpy_retrieval as NR
from mpsfm_amd import capi
from mpsfm_amd.extraction import pairs as P
from mpsfm_amd.extraction.pairwise import match_pairs, names_to_pair
from mpsfm_amd.utils.parsers import read_unique_pairs
from test_retrieval_cpu import ALL_CASES, assert_lists_agree, load_case, mappings

pytestmark = pytest.mark.gpu

R = importlib.import_module("mpsfm_amd.extraction.pairs.pairs_from_retrieval")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIP = 64  # rows of a workgroup and columns of a tile in k_sim_topk
ND = 3 * STRIP + 5  # three full column tiles and a partial one


def unit(rng, n, dim):
    x = rng.normal(size=(n, dim))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32) / np.float32(1.0 + 2.0 ** -20)  # the float32 rounding may leave a norm above 1


def clustered(rng, n, dim, places=5, spread=1.0):
    """unit descriptors of a few places: the images of one place share a direction"""
    u = rng.normal(size=(places, dim))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    x = u[rng.integers(0, places, n)] + spread * rng.normal(size=(n, dim)) / np.sqrt(dim)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32) / np.float32(1.0 + 2.0 ** -20)


def dyadic(rng, n, dim, lo=-4, hi=4):
    return (rng.integers(lo, hi + 1, (n, dim)) / 8.0).astype(np.float32)


def check(q, db, k, exact=False, min_score=0.0, qi=None, di=None, sim=None, **kw):
    """one call against the restatement (sim: similarities computed once for several calls of a case)"""
    idx, val, cnt = capi.retrieve_topk(q, db, k, min_score, qi, di, **kw)
    if sim is None:
        sim = NR.similarities(q, db)
    ridx, rval, rcnt, margin = NR.topk_similarities(sim, k, min_score, qi, di)
    assert idx.dtype == np.int64 and idx.shape == ridx.shape and val.shape == rval.shape and cnt.shape == rcnt.shape
    if not exact:
        t = NR.tau(q.shape[1], NR.TAU64_EPS)
        assert (margin > t).all(), (margin.min(), t)
    assert np.array_equal(cnt, rcnt), np.flatnonzero(cnt != rcnt)[:10]
    assert np.array_equal(idx, ridx), np.flatnonzero((idx != ridx).any(1))[:10]
    assert np.array_equal(val, rval) if exact else np.abs(val - rval).max() <= t
    return idx, val, cnt


# ---- shapes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nd", [(1, 1), (1, 2), (2, 1), (1, 65), (65, 1), (2, 2), (15, 17), (16, 16), (17, 15), (63, 65), (64, 64), (65, 63),
                                   (2 * STRIP - 1, 2 * STRIP + 1), (2 * STRIP, 2 * STRIP), (2 * STRIP + 1, 2 * STRIP - 1)])
def test_set_sizes_around_the_tile_and_the_strip(nq, nd):
    rng = np.random.default_rng(1000 * nq + nd)
    q, db = unit(rng, nq, 24), unit(rng, nd, 24)
    e0, e1 = dyadic(rng, nq, 24), dyadic(rng, nd, 24)
    sim, esim = NR.similarities(q, db), NR.similarities(e0, e1)
    for k in sorted({1, min(nd, 3), min(nd, 17)}):
        for ms in (0.0, None):
            check(q, db, k, min_score=ms, sim=sim)
            check(e0, e1, k, exact=True, min_score=ms, sim=esim)
        check(e0, e1, k, exact=True, sim=esim, column_ranges=1)  # one workgroup carries the list over all tiles


@pytest.mark.parametrize("k", [1, 2, 15, 16, 17, 63, 64, 65, 127, 128])
def test_list_lengths_around_the_lane_group_the_tile_and_the_cap(k):
    rng = np.random.default_rng(k)
    q, db = unit(rng, 70, 16), unit(rng, 200, 16)
    e0, e1 = dyadic(rng, 70, 16), dyadic(rng, 200, 16)
    sim, esim = NR.similarities(q, db), NR.similarities(e0, e1)
    for cr in (0, 1):
        _, _, cnt = check(q, db, k, min_score=None, sim=sim, column_ranges=cr)
        assert (cnt == k).all()
        check(q, db, k, sim=sim, column_ranges=cr)
        check(e0, e1, k, exact=True, min_score=None, sim=esim, column_ranges=cr)
        check(e0, e1, k, exact=True, sim=esim, column_ranges=cr)


@pytest.mark.parametrize("dim", [1, 3, 4, 5, 63, 64, 65, 1024, 1025, 4096])
def test_descriptor_lengths_around_the_step_and_the_slice(dim):
    rng = np.random.default_rng(dim)
    hi = 4 if dim <= 64 else 1  # |sim| stays far below 2^53 / 64: every sum exact
    e0, e1 = dyadic(rng, 70, dim, -hi, hi), dyadic(rng, 67, dim, -hi, hi)
    esim = NR.similarities(e0, e1)
    check(e0, e1, 5, exact=True, sim=esim)
    check(e0, e1, 20, exact=True, min_score=None, sim=esim, column_ranges=1)
    if dim >= 3:
        q, db = unit(rng, 70, dim), unit(rng, 67, dim)
        sim = NR.similarities(q, db)
        check(q, db, 5, sim=sim)
        check(q, db, 20, min_score=None, sim=sim, column_ranges=1)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,case", ALL_CASES, ids=[t for t, _ in ALL_CASES])
def test_fixture_through_the_call_the_pair_list_and_main(tag, case, tmp_path):
    q, db, qn, dn, num, pairs, scores = load_case(tag, case)
    k = min(num, len(q))
    qi, di = NR.name_ids(qn, dn)
    idx, val, cnt = capi.retrieve_topk(q, db, k, 0.0, qi, di)
    ridx, rval, rcnt, margin = NR.retrieve_topk(q, db, k, 0.0, qi, di)
    t64 = NR.tau(q.shape[1], NR.TAU64_EPS)
    assert (margin > t64).all()
    assert np.array_equal(idx, ridx) and np.array_equal(cnt, rcnt) and np.abs(val - rval).max() <= t64
    assert_lists_agree(tag, idx, val, cnt, margin, q, pairs, scores, NR.tau(q.shape[1], NR.TAU32_EPS), 0.95)
    listed = R.pairs_from_descriptors(q, db, num, 0, qi, di)
    assert listed == NR.pairs_of(idx, cnt)
    sure = margin > NR.tau(q.shape[1], NR.TAU32_EPS)
    assert [p for p in listed if sure[p[0]]] == [(int(i), int(j)) for i, j in pairs if sure[i]]
    if case is None:
        descriptors = {n: {"global_descriptor": d} for n, d in zip(qn, q)}
        dbs = None if qn == dn else {n: {"global_descriptor": d} for n, d in zip(dn, db)}
        args = {}
    else:
        descriptors, dbs = mappings(case)
        args = dict(query_prefix=case["query_prefix"], query_list=case["query_list"], db_prefix=case["db_prefix"], db_list=case["db_list"])
    out = tmp_path / "pairs.txt"
    named = P.pairs_from_retrieval(descriptors, out, num, db_descriptors=dbs, **args)
    assert named == [(qn[i], dn[j]) for i, j in listed]
    assert out.read_text() == "\n".join(f"{a} {b}" for a, b in named)
    if case is not None:  # every row of the name cases is decided: the file is the reference's, byte for byte
        assert sure.all() and out.read_bytes() == case["text"].encode()


# ---- carrying the list across tiles -------------------------------------------------------------------------------------------------
def planted(winners, nq=70, nd=ND):
    """Exact similarities: row i scores 0.5 * (17 + p_i(j)) / 16 with winner j (p_i a rotation of 0 .. m - 1, so every row has its own
    order) and (c % 7) / 64 with every other column c: ties among the rest, all below the winners."""
    m = len(winners)
    db = np.zeros((nd, 24), np.float32)
    db[:, 16] = (np.arange(nd) % 7) / 8.0
    q = np.zeros((nq, 24), np.float32)
    q[:, 16] = 1 / 8.0
    want = []
    for j, w in enumerate(winners):
        db[w] = 0
        db[w, j] = 0.5
    for i in range(nq):
        p = (np.arange(m) + i) % m
        q[i, :m] = (17 + p) / 16.0
        want.append([winners[j] for j in np.argsort(-p)])
    return q, db, want


@pytest.mark.parametrize("name,winners", [
    ("one per tile", [10, STRIP + 20, 2 * STRIP + 30, 3 * STRIP + 2]),
    ("all in the last partial tile", [3 * STRIP + c for c in range(5)]),
    ("all in one lane", [3 + 16 * j for j in range(12)]),
    ("all in one 16-lane group", [STRIP + 16 + c for c in range(16)]),
])
def test_winners_in_chosen_places(name, winners):
    q, db, want = planted(winners)
    sim = NR.similarities(q, db)
    m = len(winners)
    for cr in (1, 2, 0):
        idx, _, _ = check(q, db, m, exact=True, min_score=None, sim=sim, column_ranges=cr)
        assert idx.tolist() == want
        idx, _, cnt = check(q, db, m + 7, exact=True, sim=sim, column_ranges=cr)  # behind the winners: ties, the lowest indices
        assert idx[:, :m].tolist() == want and (cnt == m + 7).all()


def test_a_list_that_fills_only_in_the_last_tile():
    db = np.zeros((ND, 8), np.float32)
    c = np.arange(ND)
    db[:, 0] = np.where(c % 6 == 0, (c % 5 + 1) / 8.0, -(c % 3 + 1) / 8.0)
    db[3 * STRIP:, 0] = (np.arange(5) + 2) / 8.0
    q = np.zeros((66, 8), np.float32)
    q[:, 0] = (np.arange(66) % 4 + 1) / 4.0
    assert (db[:3 * STRIP, 0] > 0).sum() == 32
    for cr in (1, 2, 0):
        _, _, cnt = check(q, db, 35, exact=True, column_ranges=cr)
        assert (cnt == 35).all()
        _, _, cnt = check(q, db, 40, exact=True, column_ranges=cr)
        assert (cnt == 37).all()


def test_a_threshold_that_rises_in_every_tile():
    db = np.zeros((ND, 4), np.float32)
    db[:, 1] = (np.arange(ND) + 1) / 256.0  # ascending: every tile replaces the whole list
    q = np.zeros((65, 4), np.float32)
    q[:, 1] = (np.arange(65) % 8 + 1) / 8.0
    for k in (1, 10, 64, 100):
        for cr in (1, 2, 0):
            idx, _, _ = check(q, db, k, exact=True, column_ranges=cr)
            assert (idx == np.arange(ND - 1, ND - 1 - k, -1)).all()


# ---- column ranges ----------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_column_ranges():
    rng = np.random.default_rng(7)
    q, db = clustered(rng, 1000, 64), clustered(rng, 1300, 64)
    sim = NR.similarities(q, db)
    first = check(q, db, 20, sim=sim)
    tiles = -(-1300 // STRIP)
    seen = {}
    for cr in (1, 2, 3, 7, 0):
        idx, val, cnt, info = capi.retrieve_topk(q, db, 20, column_ranges=cr, return_info=True)
        assert np.array_equal(idx, first[0]) and np.array_equal(val, first[1]) and np.array_equal(cnt, first[2])
        assert info["column_ranges"] == (cr or info["column_ranges"]) and info["num_pairs"] == cnt.sum() and info["num_syncs"] == 1
        assert info["num_launches"] == 2 and info["ms"] > 0
        seen[cr] = (info["column_ranges"], -(-tiles // info["column_ranges"]))
    assert seen[1] == (1, tiles) and seen[3] == (3, 7) and seen[7] == (7, 3)  # more than one range, more than one tile per range
    assert capi.retrieve_topk(q, db, 20, column_ranges=10 ** 6, return_info=True)[3]["column_ranges"] == tiles  # one workgroup per tile
    assert np.array_equal(capi.retrieve_topk(q, db, 20, column_ranges=10 ** 6)[0], first[0])
    assert np.array_equal(capi.retrieve_topk(q, db, 20, column_ranges=8)[0], first[0])  # 21 tiles in 8 ranges of 3: the last range is empty


# ---- exact ties -------------------------------------------------------------------------------------------------------------------
def test_tie_groups_across_a_tile_edge_a_range_edge_and_the_list_end():
    rng = np.random.default_rng(5)
    db = dyadic(rng, ND, 16, -2, 2)
    v = np.zeros(16, np.float32)
    v[:8] = 0.5  # |v|^2 = 2: no other descriptor reaches that similarity with v
    tile_edge, range_edge = [STRIP - 2, STRIP - 1, STRIP, STRIP + 1], [2 * STRIP - 1, 2 * STRIP, 2 * STRIP + 1]  # 4 tiles in 2 ranges: columns 128 on
    w = np.zeros(16, np.float32)
    w[8:] = 0.5
    for c in tile_edge:
        db[c] = v
    for c in range_edge:
        db[c] = w
    q = dyadic(rng, 70, 16, -2, 2)
    q[0], q[1], q[69] = v, w, v + w
    sim = NR.similarities(q, db)
    for cr in (2, 1, 0):
        for k in (1, 2, 3, 4, 6, 9):
            idx, val, _ = check(q, db, k, exact=True, min_score=None, sim=sim, column_ranges=cr)
            assert idx[0, :4].tolist() == tile_edge[:k][:4] and idx[1, :3].tolist() == range_edge[:k][:3]  # the lowest indices stay
            assert idx[69, :7].tolist() == sorted(tile_edge + range_edge)[:k][:7]
    dup = dyadic(rng, ND, 16)  # duplicated db descriptors everywhere
    dup[1::2] = dup[0:-1:2]
    check(q, dup, 20, exact=True, sim=NR.similarities(q, dup), column_ranges=1)
    check(q, dup, 20, exact=True, min_score=None, sim=NR.similarities(q, dup))


def test_a_row_whose_candidates_are_all_equal():
    db = np.tile((np.arange(8) / 8.0).astype(np.float32), (ND, 1))
    q = np.tile((np.arange(8) / 8.0).astype(np.float32), (3, 1))
    q[1] *= -1
    for cr in (1, 2, 0):
        idx, val, cnt = check(q, db, 70, exact=True, column_ranges=cr)
        assert idx[0].tolist() == list(range(70)) and cnt.tolist() == [70, 0, 70] and (val[0] == val[0, 0]).all()
        idx, _, _ = check(q, db, 70, exact=True, min_score=None, column_ranges=cr)
        assert idx[1].tolist() == list(range(70))


# ---- identity ---------------------------------------------------------------------------------------------------------------------
def test_identity_removes_columns_before_the_selection():
    rng = np.random.default_rng(9)
    db = dyadic(rng, ND, 16, -2, 2)
    v = np.zeros(16, np.float32)
    v[:8] = 0.5
    db[70], db[140], db[141] = v, v, v  # a duplicate group of the best column
    q = dyadic(rng, 5, 16, -2, 2)
    q[:] = v
    di = np.arange(ND, dtype=np.int32) + 100
    di[[3, 71, 150]] = 7  # several db columns share id 7
    qi = np.array([170, 240, 7, 99, 5], np.int32)  # row 0: column 70, row 1: column 140, row 2: three columns, rows 3 and 4: none
    sim = NR.similarities(q, db)
    for cr in (1, 2, 0):
        idx, _, cnt = check(q, db, 3, exact=True, qi=qi, di=di, sim=sim, column_ranges=cr)
        assert idx[0].tolist()[:2] == [140, 141] and idx[1].tolist()[:2] == [70, 141] and idx[3].tolist() == [70, 140, 141]
        assert not np.isin(idx[2], [3, 71, 150]).any() and np.array_equal(idx[3], idx[4])
        big, _, bcnt = check(q, db, 128, exact=True, min_score=None, qi=qi, di=di, sim=sim, column_ranges=cr)
        assert (bcnt == 128).all() and 70 not in big[0] and 140 not in big[1]
    every = np.full(ND, 7, np.int32)  # every column excluded for row 2
    idx, val, cnt = check(q, db, 4, exact=True, qi=qi, di=every, sim=sim)
    assert cnt.tolist() == [4, 4, 0, 4, 4] and (idx[2] == -1).all() and (val[2] == 0).all()
    idx, _, cnt = check(q, db, 4, exact=True, min_score=None, qi=np.full(5, 7, np.int32), di=every, sim=sim, column_ranges=1)
    assert (cnt == 0).all() and (idx == -1).all()


# ---- the score test -----------------------------------------------------------------------------------------------------------------
def test_the_score_test_keeps_its_boundary_and_drops_one_step_below():
    db = np.zeros((ND, 4), np.float32)
    db[:, 0] = np.where(np.arange(ND) % 3 == 0, 0.25, np.where(np.arange(ND) % 3 == 1, 0.5, -0.125))
    q = np.zeros((2, 4), np.float32)
    q[0, 0], q[1, 0] = 1.0, -1.0
    thirds = [c for c in range(ND) if c % 3 == 1] + [c for c in range(ND) if c % 3 == 0]
    for cr in (1, 0):
        idx, val, cnt = check(q, db, 128, exact=True, min_score=0.25, column_ranges=cr)  # similarities equal to min_score are kept
        assert cnt.tolist() == [128, 0] and idx[0].tolist() == thirds[:128] and val[0, 127] == 0.25
        idx, val, cnt = check(q, db, 128, exact=True, min_score=float(np.nextafter(0.25, 1.0)), column_ranges=cr)  # one fp64 step above them
        assert cnt.tolist() == [sum(c % 3 == 1 for c in range(ND)), 0] and (val[0, :cnt[0]] == 0.5).all()
        assert (idx[0, cnt[0]:] == -1).all() and (val[0, cnt[0]:] == 0).all()  # fewer than k valid candidates: counts and padding
        idx, val, cnt = check(q, db, 100, exact=True, min_score=None, column_ranges=cr)  # no score test: negative similarities are listed
        assert cnt.tolist() == [100, 100] and val[1, 0] == 0.125 and (val[1, 70:] < 0).all()
        idx, val, cnt = check(-np.abs(q), np.abs(db) + np.float32(0.125), 5, exact=True, column_ranges=cr)  # all negative, min_score 0
        assert (cnt == 0).all() and (idx == -1).all() and (val == 0).all()


# ---- query is db --------------------------------------------------------------------------------------------------------------------
def test_one_set_gives_what_two_equal_sets_give():
    rng = np.random.default_rng(13)
    a = clustered(rng, 300, 64)
    ids = np.arange(300, dtype=np.int32)
    one = capi.retrieve_topk(a, a, 20, query_ids=ids, db_ids=ids)
    two = capi.retrieve_topk(a, a.copy(), 20, query_ids=ids, db_ids=ids)
    assert all(np.array_equal(x, y) for x, y in zip(one, two))
    assert not (one[0] == np.arange(300)[:, None]).any() and (one[2] == 20).all()
    check(a, a, 20, qi=ids, di=ids)
    idx, val, _ = capi.retrieve_topk(a, a, 1)  # without ids every image finds itself
    assert idx[:, 0].tolist() == list(range(300))


# ---- device tensors -----------------------------------------------------------------------------------------------------------------
def test_device_tensors_give_what_host_arrays_give():
    import torch

    rng = np.random.default_rng(31)
    q, db = clustered(rng, 300, 128), clustered(rng, 340, 128)
    ids = (np.arange(300, dtype=np.int32), np.arange(340, dtype=np.int32)[::-1].copy())
    host = capi.retrieve_topk(q, db, 20, query_ids=ids[0], db_ids=ids[1])
    tq, tdb = torch.from_numpy(q).cuda(), torch.from_numpy(db).cuda()
    torch.cuda.synchronize()
    dev = capi.retrieve_topk(tq, tdb, 20, query_ids=ids[0], db_ids=ids[1])
    assert all(np.array_equal(x, y) for x, y in zip(host, dev))
    half = capi.retrieve_topk(q.astype(np.float16), db.astype(np.float16), 20)
    assert all(np.array_equal(x, y) for x, y in zip(half, capi.retrieve_topk(tq.half(), tdb.half(), 20)))
    # not contiguous on the device
    dev = capi.retrieve_topk(tq.T.contiguous().T, tdb.T.contiguous().T, 20, query_ids=ids[0], db_ids=ids[1])
    assert all(np.array_equal(x, y) for x, y in zip(host, dev))
    # one device tensor on both sides
    assert all(np.array_equal(x, y) for x, y in zip(capi.retrieve_topk(q, q, 20), capi.retrieve_topk(tq, tq, 20)))
    assert R.pairs_from_descriptors(tq, tdb, 20, 0, *ids) == NR.pairs_of(host[0], host[2])
    # produced on the caller's stream immediately before the call
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        w = torch.ones(2048, 2048, device="cuda")
        for _ in range(20):
            w = (w @ w) * (1.0 / 2048)  # the stream is busy when the descriptors are enqueued
        a = tq * w[0, 0]  # w == 1 exactly: a == tq, written behind the products
        b = tdb * w[1, 1]
        dev = capi.retrieve_topk(a, b, 20, query_ids=ids[0], db_ids=ids[1])
    assert all(np.array_equal(x, y) for x, y in zip(host, dev))
    torch.cuda.synchronize()


def test_device_inputs_are_scanned_and_checked():
    import torch

    d = torch.zeros(70, 8, device="cuda")
    d[69, 7] = float("nan")
    ok = torch.ones(5, 8, device="cuda")
    torch.cuda.synchronize()
    for a, b in ((d, ok), (ok, d), (d, d)):
        with pytest.raises(capi.MpsfmHipError) as e:
            capi.retrieve_topk(a, b, 2)
        assert e.value.code == -1 and "non-finite" in str(e.value)
    with pytest.raises(ValueError):
        capi.retrieve_topk(ok, np.ones((5, 8), np.float32), 2)
    with pytest.raises(TypeError):
        capi.retrieve_topk(ok.double(), ok.double(), 2)
    with pytest.raises(ValueError):  # the tensors' own device is used: naming another one is refused, not overridden
        capi.retrieve_topk(ok, ok, 2, device=ok.device.index + 1)
    idx, _, cnt = capi.retrieve_topk(ok, ok, 2, device=ok.device.index)
    assert idx.tolist() == [[0, 1]] * 5 and cnt.tolist() == [2] * 5


# ---- determinism ------------------------------------------------------------------------------------------------------------------
def test_results_are_identical_run_to_run_and_across_host_threads():
    rng = np.random.default_rng(41)
    q, db = clustered(rng, 500, 64), clustered(rng, 450, 64)
    e = dyadic(rng, 200, 8, -1, 1)  # ties everywhere

    def work():
        return capi.retrieve_topk(q, db, 20) + capi.retrieve_topk(e, e, 50, min_score=None) + capi.retrieve_topk(q, db, 128, column_ranges=3)

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
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_retrieval_worker.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


# ---- the chain --------------------------------------------------------------------------------------------------------------------
def test_retrieval_feeds_the_matcher(tmp_path):
    rng = np.random.default_rng(51)
    names = [f"im{i}.jpg" for i in range(6)]
    glob = clustered(rng, 6, 64, places=2)
    feats = {n: {"global_descriptor": g, "descriptors": unit(rng, 50, 32).T.copy()} for n, g in zip(names, glob)}
    path = tmp_path / "pairs.txt"
    listed = P.pairs_from_retrieval(feats, path, 3)
    assert len(listed) > 0 and all(a != b for a, b in listed)
    pairs = read_unique_pairs(path)
    assert {frozenset(p) for p in pairs} == {frozenset(p) for p in listed} and len(pairs) <= len(listed)
    matches = match_pairs({}, [tuple(p) for p in pairs], feats)
    for a, b in pairs:  # every retrieved pair gets a match list
        m = matches[names_to_pair(a, b)]
        assert m["matches0"].shape == (1, 50) and m["matching_scores0"].shape == (1, 50) and (m["matches0"] >= 0).any()
