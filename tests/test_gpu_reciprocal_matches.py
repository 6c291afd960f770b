"""Dense reciprocal matches on the GPU (csrc/reciprocal_matches.hip) against the fp64 restatement (tests/numpy_reciprocal_matches.py):
EQUALITY of indices, scores (bitwise) and counters on every case.  tests/test_reciprocal_matches_cpu.py asserts that every seed of
the random inputs is decided (0 undecided seeds is the cap of this comparison); the planted cases are exact sums of dyadic values,
where equal similarities are equal bitwise and the tie rule decides."""

import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import numpy_reciprocal_matches as NR
from mpsfm_amd import capi
from mpsfm_amd.extraction.pairwise import extract_correspondences, fast_reciprocal_NNs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "reference_reciprocal_matches.npz"))


def same_search(got, r):
    i1, i2, info = got
    assert i1.dtype == np.int32 and i2.dtype == np.int32
    assert np.array_equal(i1, r["idx1"]) and np.array_equal(i2, r["idx2"])
    assert (info["n_seeds"], info["n_converged"], info["iterations"], info["nn_queries"]) == (r["n_seeds"], r["n_converged"], r["iterations"], r["nn_queries"])


@pytest.fixture(scope="module")
def fixtures():
    out = {}
    for name in NR.FIXTURE_CASES:
        feats, qonfs, S = NR.fixture_inputs(name)
        assert NR.digest(*feats, *qonfs) == str(GOLD[f"{name}_digest"])
        out[name] = (feats, qonfs, S)
    return out


# ---- the fixtures -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(NR.FIXTURE_CASES))
def test_fixture_through_the_single_search_entry(fixtures, name):
    (f11, f21, f22, f12), _, S = fixtures[name]
    for s, (A, B) in enumerate(((f11, f21), (f21, f11), (f12, f22), (f22, f12))):
        i1, i2, info = capi.reciprocal_nns(A, B, S, return_info=True)
        assert np.array_equal(i1, GOLD[f"{name}_search{s}_idx1"]) and np.array_equal(i2, GOLD[f"{name}_search{s}_idx2"])
        assert [info["n_seeds"], info["n_converged"], info["iterations"], info["nn_queries"]] == GOLD[f"{name}_search{s}_stats"].tolist()
        assert info["ms"] > 0 and info["column_ranges"] >= 1
        j1, j2 = fast_reciprocal_NNs(A, B, subsample_or_initxy1=S, ret_xy=False, device="cuda", dist="dot", block_size=2 ** 13)
        assert np.array_equal(j1, i1) and np.array_equal(j2, i2)
        x1, x2 = fast_reciprocal_NNs(A, B, S)
        assert x1.dtype == np.int64 and np.array_equal(x1[:, 1] * A.shape[1] + x1[:, 0], i1) and np.array_equal(x2[:, 1] * B.shape[1] + x2[:, 0], i2)


@pytest.mark.parametrize("name", list(NR.FIXTURE_CASES))
def test_fixture_through_the_four_search_entry_and_the_python_functions(fixtures, name):
    feats, qonfs, S = fixtures[name]
    xy1, xy2, sc, info = capi.dense_correspondences(feats, qonfs, S, return_info=True)
    for got, key in ((xy1, "xy1"), (xy2, "xy2"), (sc, "scores")):
        assert got.dtype == GOLD[f"{name}_{key}"].dtype and np.array_equal(got, GOLD[f"{name}_{key}"])
    stats = np.stack([GOLD[f"{name}_search{s}_stats"] for s in range(4)])
    assert (info["n_seeds"], info["n_converged"], info["nn_queries"]) == (stats[:, 0].sum(), stats[:, 1].sum(), stats[:, 3].sum())
    assert info["iterations"] == stats[:, 2].max()
    px1, px2, ps = extract_correspondences(feats, qonfs, subsample=S)
    assert np.array_equal(px1, xy1) and np.array_equal(px2, xy2) and np.array_equal(ps, sc) and ps.dtype == np.float32


def test_the_four_search_call_equals_four_single_calls(fixtures):
    feats, qonfs, S = fixtures["small"]
    f11, f21, f22, f12 = feats
    runs = [capi.reciprocal_nns(A, B, S, return_info=True) for A, B in ((f11, f21), (f21, f11), (f12, f22), (f22, f12))]
    idx1 = np.r_[runs[0][0], runs[1][1], runs[2][0], runs[3][1]]
    idx2 = np.r_[runs[0][1], runs[1][0], runs[2][1], runs[3][0]]
    q1 = np.r_[qonfs[0].ravel()[np.r_[runs[0][0], runs[1][1]]], qonfs[3].ravel()[np.r_[runs[2][0], runs[3][1]]]]
    q2 = np.r_[qonfs[1].ravel()[np.r_[runs[0][1], runs[1][0]]], qonfs[2].ravel()[np.r_[runs[2][1], runs[3][0]]]]
    rx1, rx2, first = NR.merge_corres(idx1, idx2, f11.shape[:2], f22.shape[:2])
    xy1, xy2, sc, info = capi.dense_correspondences(feats, qonfs, S, return_info=True)
    assert np.array_equal(xy1, rx1) and np.array_equal(xy2, rx2) and np.array_equal(sc, np.sqrt(q1[first] * q2[first]))
    assert info["nn_queries"] == sum(r[2]["nn_queries"] for r in runs) and info["n_converged"] == sum(r[2]["n_converged"] for r in runs)


# ---- shapes and parameters -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(NR.SWEEP_CASES))
def test_random_maps_over_seed_counts_channels_subsamples_and_iteration_caps(name):
    A, B, S, max_iter = NR.sweep_inputs(name)
    r = NR.fast_reciprocal_nns(A, B, S, max_iter)
    same_search(capi.reciprocal_nns(A, B, S, max_iter, return_info=True), r)
    if name == "S1":  # every pixel a seed: the full mutual nearest-neighbour set
        sim = NR.NM.similarities(A.reshape(-1, 24), B.reshape(-1, 24))
        fwd, bwd = sim.argmax(1), sim.argmax(0)
        mutual = [(i, j) for i, j in enumerate(fwd) if bwd[j] == i]
        assert sorted(zip(r["idx1"].tolist(), r["idx2"].tolist())) == mutual
    if name == "seeds90":  # the four-search entry on maps of different sizes, two strips
        q1, q2 = NR.random_maps(77, *A.shape[:2], 1)[..., 0] * 0.25 + 0.5, NR.random_maps(78, *B.shape[:2], 1)[..., 0] * 0.25 + 0.5
        feats, qonfs = (A, B, B[::-1].copy(), A[::-1].copy()), (q1, q2, q2[::-1].copy(), q1[::-1].copy())
        want = NR.extract_correspondences(feats, qonfs, S, max_iter)
        got = capi.dense_correspondences(feats, qonfs, S, max_iter)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)) and len(got[2]) > 100


# ---- planted exact cases -----------------------------------------------------------------------------------------------------------
def seed_index(H, W, S, pixel):
    return int(np.flatnonzero(NR.seed_pixels(H, W, S) == pixel)[0])


@pytest.mark.parametrize("n", [1, 2, 3, 11])
def test_descent_chains(n):
    pa, pb = [10 + 2 * i for i in range(n)], [40 - 3 * i for i in range(n)]
    A, B = NR.planted(6, 9, 7, 8, 2 * n, NR.chain_links(pa, pb))
    for max_iter in (10, 11, 2):
        r = NR.fast_reciprocal_nns(A, B, 1, max_iter)
        assert r["converged"][seed_index(6, 9, 1, pa[0])] == (n <= max_iter)  # the longest chain is dropped at 10 and kept at 11
        i1, i2, info = capi.reciprocal_nns(A, B, 1, max_iter, return_info=True)
        same_search((i1, i2, info), r)
        assert (pa[-1], pb[-1]) in set(zip(i1.tolist(), i2.tolist()))  # the chain's last pixel is a seed too


def test_duplicates_of_the_best_column_across_a_tile_edge_and_two_seeds_on_one_pair():
    H1, W1, H2, W2, Cn = 6, 9, 40, 48, 8
    links = [(10, 63, 0, 0.5, 0.25), (None, 64, 0, 0, 0.25), (None, 200, 0, 0, 0.25),  # across a tile edge: 63 wins
             (12, 1279, 1, 0.5, 0.5), (None, 1280, 1, 0, 0.5), (None, 1290, 1, 0, 0.5),
             (20, 300, 2, 0.25, 0.25), (22, 300, 2, 0.25, 0.25), (30, 300, 3, 0.5, 0.5), (30, 333, 4, 1.0, 1.0)]  # 20 and 22 end on (30, 333)
    A, B = NR.planted(H1, W1, H2, W2, Cn, links)
    r = NR.fast_reciprocal_nns(A, B, 1, 10)
    pairs = list(zip(r["idx1"].tolist(), r["idx2"].tolist()))
    assert pairs == [(0, 0), (10, 63), (12, 1279), (30, 333)] and r["n_converged"] == H1 * W1
    assert r["gap"][seed_index(H1, W1, 1, 10)] == 0.0 and r["gap"][seed_index(H1, W1, 1, 12)] == 0.0
    same_search(capi.reciprocal_nns(A, B, 1, return_info=True), r)
    # the other direction: the duplicates are seeds themselves and tie on the way back
    r = NR.fast_reciprocal_nns(B, A, 1, 10)
    same_search(capi.reciprocal_nns(B, A, 1, return_info=True), r)


def test_workload_size_map_with_the_best_column_at_the_ends_of_a_column_range():
    H, W, Cn, S = 384, 512, 24, 64
    zeros = np.zeros((H, W, Cn), np.float32)
    ranges = capi.reciprocal_nns(zeros, zeros, S, return_info=True)[2]["column_ranges"]  # they depend on the shapes only
    tiles = H * W // 64
    per = (tiles + ranges - 1) // ranges * 64  # columns of a range
    assert per > 64 and ranges > 3, "a range holds more than one column tile"
    seeds = NR.seed_pixels(H, W, S).tolist()
    assert len(seeds) == 48
    first, last = per + 5, 2 * per - 3  # in the first and in the last tile of range 1
    links = [(seeds[3], first, 0, 0.5, 0.5), (seeds[40], last, 1, 0.5, 0.5), (seeds[47], H * W - 1, 3, 0.5, 0.5),
             (seeds[17], 3 * per - 1, 2, 0.5, 0.5), (None, 3 * per, 2, 0, 0.5), (None, H * W - 2, 2, 0, 0.5)]  # duplicates across a range edge
    A, B = NR.planted(H, W, H, W, Cn, links)
    r = NR.fast_reciprocal_nns(A, B, S, 10)
    want = {(seeds[3], first), (seeds[40], last), (seeds[47], H * W - 1), (seeds[17], 3 * per - 1)}
    assert want <= set(zip(r["idx1"].tolist(), r["idx2"].tolist())) and r["gap"][17] == 0.0
    i1, i2, info = capi.reciprocal_nns(A, B, S, return_info=True)
    same_search((i1, i2, info), r)
    assert info["column_ranges"] == ranges


# ---- call paths ------------------------------------------------------------------------------------------------------------------------
def test_device_tensors_give_what_host_arrays_give(fixtures):
    import torch

    feats, qonfs, S = fixtures["small"]
    want = capi.dense_correspondences(feats, qonfs, S)
    tf, tq = [torch.from_numpy(f).cuda() for f in feats], [torch.from_numpy(q).cuda() for q in qonfs]
    torch.cuda.synchronize()
    got = extract_correspondences(tf, tq, subsample=S)
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want))
    # channel-first in memory
    got = capi.dense_correspondences([t.permute(2, 0, 1).contiguous().permute(1, 2, 0) for t in tf], [q.T.contiguous().T for q in tq], S)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    # float16 on both paths
    h16, q16 = [f.astype(np.float16) for f in feats], [q.astype(np.float16) for q in qonfs]
    want16 = capi.dense_correspondences(h16, q16, S)
    got = capi.dense_correspondences([t.half() for t in tf], [q.half() for q in tq], S)
    assert all(np.array_equal(a, b) for a, b in zip(got, want16))
    w1 = capi.reciprocal_nns(h16[0], h16[1], S)
    assert all(np.array_equal(a, b) for a, b in zip(capi.reciprocal_nns(tf[0].half(), tf[1].half(), S), w1))
    # produced on the caller's stream immediately before the call
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        w = torch.ones(2048, 2048, device="cuda")
        for _ in range(20):
            w = (w @ w) * (1.0 / 2048)  # the stream is busy when the maps are enqueued
        got = capi.dense_correspondences([t * w[0, 0] for t in tf], [q * w[1, 1] for q in tq], S)  # w == 1 exactly
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        capi.reciprocal_nns(tf[0], feats[1], S)
    with pytest.raises(ValueError):
        capi.reciprocal_nns(tf[0], tf[1], S, device=tf[0].device.index + 1)


def test_a_nan_in_a_device_input_is_refused():
    import torch

    A, B = torch.rand(12, 13, 8, device="cuda"), torch.rand(9, 17, 8, device="cuda")
    qa, qb = torch.rand(12, 13, device="cuda"), torch.rand(9, 17, device="cuda")
    torch.cuda.synchronize()
    for k in range(2):
        bad = [A.clone(), B.clone()]
        bad[k][-1, -1, -1] = float("nan")
        with pytest.raises(capi.MpsfmHipError) as e:
            capi.reciprocal_nns(bad[0], bad[1], 2)
        assert e.value.code == -1
    bq = qb.clone()
    bq[3, 3] = float("inf")
    with pytest.raises(capi.MpsfmHipError) as e:
        capi.dense_correspondences((A, B, B, A), (qa, qb, bq, qa), 2)
    assert e.value.code == -1
    assert len(capi.dense_correspondences((A, B, B, A), (qa, qb, qb, qa), 2)[2]) > 0


def test_results_are_identical_run_to_run_and_across_host_threads(fixtures):
    feats, qonfs, S = fixtures["small"]
    A, B, S2, _ = NR.sweep_inputs("S1")

    def work():
        return capi.dense_correspondences(feats, qonfs, S) + capi.reciprocal_nns(A, B, S2)

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
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_reciprocal_matches_worker.py")], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
