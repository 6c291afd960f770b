"""Dense reciprocal matching without a GPU: the fp64 restatement (tests/numpy_reciprocal_matches.py) against the fixture that the
reference's own merge_corres / extract_correspondences computed (tests/golden/make_golden_reciprocal_matches.py), the tie and
chain rules on the restatement, the decidedness of every input the GPU test compares on, the entry points' argument checks,
which come before any device is touched, and the wrappers' types and refusals.

The cap of the GPU comparison is set here: every seed of every random case is decided (the gap between the best and the second
best similarity exceeds tau64 = 4 C 2^-53 at every query of its trajectory), so the GPU test may ask for equality on all of them."""

import ctypes as C
import os

import numpy as np
import pytest

import numpy_reciprocal_matches as NR
from mpsfm_amd import capi
from mpsfm_amd.extraction import pairwise
from mpsfm_amd.extraction.pairwise import extract_correspondences, fast_reciprocal_NNs, map_keypoints_to_original_after_crop, merge_corres

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_reciprocal_matches.npz"))
EINVAL, ENODEVICE = -1, -2


@pytest.mark.parametrize("name", list(NR.FIXTURE_CASES))
def test_restatement_equals_the_fixture_exactly(name):
    feats, qonfs, S = NR.fixture_inputs(name)
    assert NR.digest(*feats, *qonfs) == str(GOLD[f"{name}_digest"]), "this machine does not build the fixture's maps bit for bit"
    case = NR.FIXTURE_CASES[name]
    assert GOLD[f"{name}_case"].tolist() == [case[0], *case[1], *case[2], case[3], case[4], *case[5]]
    xy1, xy2, scores, runs = NR.extract_correspondences(feats, qonfs, S, return_runs=True)
    for got, key in ((xy1, "xy1"), (xy2, "xy2"), (scores, "scores")):
        assert got.dtype == GOLD[f"{name}_{key}"].dtype and np.array_equal(got, GOLD[f"{name}_{key}"])
    for s, r in enumerate(runs):
        assert np.array_equal(r["idx1"], GOLD[f"{name}_search{s}_idx1"]) and np.array_equal(r["idx2"], GOLD[f"{name}_search{s}_idx2"])
        assert [r["n_seeds"], r["n_converged"], r["iterations"], r["nn_queries"]] == GOLD[f"{name}_search{s}_stats"].tolist()
        assert r["gap"].min() > NR.tau64(case[3])
    assert max(r["iters_of_seed"].max() for r in runs) >= 3


def test_python_merge_corres_is_the_restatement_s_and_keeps_first_occurrences():
    rng = np.random.default_rng(5)
    i1, i2 = rng.integers(0, 30, 400).astype(np.int32), rng.integers(0, 6, 400).astype(np.int32)
    xy1, xy2, first = merge_corres(i1, i2, (5, 6), (2, 3), ret_index=True)
    r1, r2, rfirst = NR.merge_corres(i1, i2, (5, 6), (2, 3))
    assert xy1.dtype == np.int64 and xy1.shape == (len(first), 2) and len(first) < 400
    assert np.array_equal(xy1, r1) and np.array_equal(xy2, r2) and np.array_equal(first, rfirst)
    key = i1.astype(np.int64) * 64 + i2
    assert all(f == np.flatnonzero(key == key[f])[0] for f in first) and (np.diff(key[first]) > 0).all()
    assert np.array_equal(xy1[:, 1] * 6 + xy1[:, 0], i1[first]) and np.array_equal(xy2[:, 1] * 3 + xy2[:, 0], i2[first])
    p1, p2 = merge_corres(i1, i2, ret_xy=False)
    assert p1.dtype == np.int32 and np.array_equal(p1, i1[first]) and np.array_equal(p2, i2[first])
    (y1, x1), _ = merge_corres(i1, i2, (5, 6), (2, 3), ret_xy="y_x")
    assert np.array_equal(x1, xy1[:, 0]) and np.array_equal(y1, xy1[:, 1])
    with pytest.raises(AssertionError):
        merge_corres(i1.astype(np.int64), i2)


def test_restatement_ties_go_to_the_lowest_index():
    H, W, Cn = 3, 70, 4
    A, B = NR.planted(H, W, H, W, Cn, [(71, 63, 0, 0.5, 0.25), (None, 64, 0, 0.0, 0.25), (None, 130, 0, 0.0, 0.25)])
    r = NR.fast_reciprocal_nns(A, B, 1, 10)
    j = int(np.flatnonzero(NR.seed_pixels(H, W, 1) == 71)[0])
    assert r["seeds_xy2"][j] == 63 and r["converged"][j] and r["gap"][j] == 0.0  # three equal best columns: undecided, lowest wins
    # background seeds: every column ties at 0, pixel 0 wins, and pixel 0 answers pixel 0
    k = int(np.flatnonzero(NR.seed_pixels(H, W, 1) == 100)[0])
    assert (r["seeds_xy1"][k], r["seeds_xy2"][k]) == (0, 0) and r["iters_of_seed"][k] == 2


def _chain_case(n, S=1):
    """A chain of n pixels of A (the first one a seed) and n of B on 6 x 9 maps; C = 2 n links + background."""
    pa, pb = [10 + 2 * i for i in range(n)], [40 - 3 * i for i in range(n)]
    Cn = 2 * n
    return NR.planted(6, 9, 7, 8, Cn, NR.chain_links(pa, pb)), pa, pb


@pytest.mark.parametrize("n", [1, 2, 3, 11])
def test_restatement_descent_chains_need_their_length_in_iterations(n):
    (A, B), pa, pb = _chain_case(n)
    r = NR.fast_reciprocal_nns(A, B, 1, 10)
    j = int(np.flatnonzero(NR.seed_pixels(6, 9, 1) == pa[0])[0])
    assert r["iters_of_seed"][j] == min(n, 10)
    if n <= 10:
        assert r["converged"][j] and (r["seeds_xy1"][j], r["seeds_xy2"][j]) == (pa[-1], pb[-1])
    else:  # dropped at max_iter, kept when it is raised
        assert not r["converged"][j]
        r = NR.fast_reciprocal_nns(A, B, 1, 11)
        assert r["converged"][j] and (r["seeds_xy1"][j], r["seeds_xy2"][j]) == (pa[-1], pb[-1]) and r["iterations"] == 11
    pairs = set(zip(r["idx1"].tolist(), r["idx2"].tolist()))
    assert (pa[-1], pb[-1]) in pairs and (0, 0) in pairs
    assert (np.diff(r["idx1"].astype(np.int64) * 1000 + r["idx2"]) > 0).all()  # unique, sorted by (idx1, idx2)


def test_restatement_two_seeds_converge_onto_one_pair():
    links = [(10, 30, 0, 0.25, 0.25), (12, 30, 0, 0.25, 0.25), (20, 30, 1, 0.5, 0.5), (20, 33, 2, 1.0, 1.0)]
    A, B = NR.planted(6, 9, 7, 8, 4, links)
    r = NR.fast_reciprocal_nns(A, B, 1, 10)
    seeds = NR.seed_pixels(6, 9, 1)
    for p in (10, 12, 20):
        j = int(np.flatnonzero(seeds == p)[0])
        assert r["converged"][j] and (r["seeds_xy1"][j], r["seeds_xy2"][j]) == (20, 33)
    assert r["n_converged"] == 54 and sorted(zip(r["idx1"].tolist(), r["idx2"].tolist())) == [(0, 0), (20, 33)]


@pytest.mark.parametrize("name", list(NR.SWEEP_CASES))
def test_every_seed_of_the_gpu_tests_random_inputs_is_decided(name):
    A, B, S, max_iter = NR.sweep_inputs(name)
    assert np.abs(A).max() <= 1 and np.abs(B).max() <= 1
    r = NR.fast_reciprocal_nns(A, B, S, max_iter)
    assert r["n_seeds"] == capi.recip_seed_count(A.shape[0], A.shape[1], S) == len(NR.seed_pixels(A.shape[0], A.shape[1], S))
    undecided = int((r["gap"] <= NR.tau64(A.shape[2])).sum())
    print(name, "seeds", r["n_seeds"], "converged", r["n_converged"], "undecided", undecided, "min gap", r["gap"].min() if r["n_seeds"] else None)
    assert undecided == 0
    if name.startswith("seeds"):
        assert r["n_seeds"] == int(name[5:])


P = lambda a: None if a is None else a.ctypes.data  # noqa: E731


def test_default_options_and_seed_counts():
    o = capi.CRecipOptions(1, 1, 1, 5)
    capi.lib().mpsfm_recip_default_options(C.addressof(o))
    assert (o.subsample, o.max_iter, o.inputs_on_device, o.stream) == (8, 10, 0, None)
    assert capi.lib().mpsfm_abi_version() == 2
    for H, W, S in ((384, 512, 8), (37, 45, 2), (5, 5, 4), (5, 5, 10), (5, 5, 11), (1, 1, 1), (3, 100, 7)):
        assert capi.recip_seed_count(H, W, S) == len(range(S // 2, H, S)) * len(range(S // 2, W, S))
    assert capi.recip_seed_count(384, 512, 8) == 3072 and capi.recip_seed_count(0, 5, 1) == 0 and capi.recip_seed_count(5, 5, 0) == 0


def test_reciprocal_nns_checks_arguments_before_any_device():
    L = capi.lib()
    a, b = np.ones((3, 4, 5), np.float32), np.ones((2, 6, 5), np.float32)
    i1, i2, n = np.zeros(12, np.int32), np.zeros(12, np.int32), C.c_int64(7)

    def call(A=a, H1=3, W1=4, B=b, H2=2, W2=6, Cc=5, S=1, it=10, cap=12, o1=i1, o2=i2, nn=n, opts=True):
        o = capi._recip_options(S, it)
        return L.mpsfm_reciprocal_nns(P(A), H1, W1, P(B), H2, W2, Cc, C.addressof(o) if opts else None, 0, cap, P(o1), P(o2),
                                      None if nn is None else C.addressof(nn), None)

    for kw in (dict(A=None), dict(B=None), dict(o1=None), dict(o2=None), dict(nn=None), dict(Cc=0), dict(Cc=1025), dict(H1=0), dict(W1=0), dict(H2=0),
               dict(W2=-1), dict(H1=4097, W1=4097), dict(H2=1 << 13, W2=(1 << 11) + 1), dict(S=0), dict(S=-2), dict(it=0), dict(it=1025), dict(cap=11)):
        assert call(**kw) == EINVAL, kw
    for bad in (np.nan, np.inf, -np.inf):
        x = a.copy(); x[2, 3, 4] = bad
        y = b.copy(); y[0, 0, 0] = bad
        assert call(A=x) == EINVAL and call(B=y) == EINVAL and b"non-finite" in L.mpsfm_last_error()
    # no seed: nothing to do, no device needed
    info = capi.CRecipInfo(5, 5, 5, 5, 5, 5.0, 0)
    o = capi._recip_options(8, 10)
    assert L.mpsfm_reciprocal_nns(P(a), 3, 4, P(b), 2, 6, 5, C.addressof(o), 0, 0, None, None, C.addressof(n), C.addressof(info)) == 0
    assert n.value == 0 and (info.n_seeds, info.n_converged, info.iterations, info.nn_queries, info.ms) == (0, 0, 0, 0, 0.0)
    # a valid call, with the default options too (subsample 8 on 17 x 17: four seeds): computed with a device, refused loudly without one
    want = 0 if capi.device_count() > 0 else ENODEVICE
    big = np.ones((17, 17, 5), np.float32)
    assert call() == want and call(A=big, H1=17, W1=17, opts=False) == want


def test_dense_correspondences_checks_arguments_before_any_device():
    L = capi.lib()
    f1, f2, q1, q2 = np.ones((3, 4, 5), np.float32), np.ones((2, 6, 5), np.float32), np.ones((3, 4), np.float32), np.ones((2, 6), np.float32)
    cap = 2 * (12 + 12)
    x1, x2, sc, n = np.zeros((cap, 2), np.int32), np.zeros((cap, 2), np.int32), np.zeros(cap, np.float32), C.c_int64(7)
    names = ("f11", "f21", "f22", "f12", "c11", "c21", "c22", "c12")

    def call(H1=3, W1=4, H2=2, W2=6, Cc=5, S=1, it=10, cp=cap, o1=x1, o2=x2, os=sc, nn=n, **maps):
        m = dict(zip(names, (f1, f2, f2, f1, q1, q2, q2, q1)))
        m.update(maps)
        o = capi._recip_options(S, it)
        return L.mpsfm_dense_correspondences(*[P(m[k]) for k in names], H1, W1, H2, W2, Cc, C.addressof(o), 0, cp, P(o1), P(o2), P(os),
                                             None if nn is None else C.addressof(nn), None)

    for k in names:
        assert call(**{k: None}) == EINVAL
        bad = (f1 if k in ("f11", "f12") else f2 if k[0] == "f" else q1 if k in ("c11", "c12") else q2).copy()
        bad.flat[-1] = np.nan
        assert call(**{k: bad}) == EINVAL and b"non-finite" in L.mpsfm_last_error()
    for kw in (dict(o1=None), dict(o2=None), dict(os=None), dict(nn=None), dict(Cc=0), dict(Cc=1025), dict(H1=0), dict(W2=0), dict(S=0), dict(it=0),
               dict(cp=cap - 1), dict(H2=4097, W2=4097)):
        assert call(**kw) == EINVAL, kw
    assert call(S=16, cp=0, o1=None, o2=None, os=None) == 0 and n.value == 0
    assert call() == (0 if capi.device_count() > 0 else ENODEVICE)


def test_wrappers_return_types_refusals_and_empty_seed_calls():
    import torch

    A, B = np.ones((5, 6, 4), np.float32), np.ones((4, 7, 4), np.float16)
    i1, i2 = fast_reciprocal_NNs(A, B, subsample_or_initxy1=16, ret_xy=False, device="cuda", dist="dot", block_size=2 ** 13)
    assert i1.dtype == np.int32 and i2.dtype == np.int32 and i1.shape == (0,) and i2.shape == (0,)
    x1, x2 = fast_reciprocal_NNs(torch.from_numpy(A), torch.from_numpy(B), 16, workers=32)
    assert x1.dtype == np.int64 and x1.shape == (0, 2) and x2.shape == (0, 2)
    i1, i2, info = capi.reciprocal_nns(A, B, 16, return_info=True)
    assert info == dict(n_seeds=0, n_converged=0, iterations=0, nn_queries=0, column_ranges=0, ms=0.0)
    q1, q2 = np.ones((5, 6), np.float32), np.ones((4, 7), np.float32)
    xy1, xy2, sc = extract_correspondences((A, B, B, A), (q1, q2, q2, q1), subsample=16)
    assert xy1.dtype == np.int64 and xy2.dtype == np.int64 and sc.dtype == np.float32 and xy1.shape == (0, 2) and xy2.shape == (0, 2) and sc.shape == (0,)
    for kw in (dict(subsample_or_initxy1=np.zeros((3, 2), np.int64)), dict(pixel_tol=1), dict(ret_basin=True), dict(dist="l2"), dict(subsample_or_initxy1=True)):
        with pytest.raises(NotImplementedError):
            fast_reciprocal_NNs(A, B, **kw)
    with pytest.raises(TypeError):
        fast_reciprocal_NNs(A, B, 16, bogus=1)
    with pytest.raises(NotImplementedError):
        extract_correspondences((A, B, B, A), (q1, q2, q2, q1), ptmap_key="pts3d")
    with pytest.raises(ValueError):
        extract_correspondences((A, B, A, A), (q1, q2, q2, q1), subsample=16)
    with pytest.raises(ValueError):
        capi.reciprocal_nns(A, np.ones((4, 7, 3), np.float32), 16)
    with pytest.raises(TypeError):
        capi.reciprocal_nns(A.astype(np.float64), B, 16)
    with pytest.raises(capi.MpsfmHipError) as err:
        capi.reciprocal_nns(A, B, 0)
    assert err.value.code == EINVAL
    k = map_keypoints_to_original_after_crop(np.array([[1, 2], [3, 4]]), 100, 80, 96, 72)
    assert k.tolist() == [[5, 10], [7, 12]]
    assert {"fast_reciprocal_NNs", "merge_corres", "extract_correspondences", "map_keypoints_to_original_after_crop"} <= set(pairwise.__all__)


def test_calls_fail_loudly_without_a_device():
    if capi.device_count() > 0:
        return  # with a device the same calls are computed: tests/test_gpu_reciprocal_matches.py
    feats, qonfs, S = NR.fixture_inputs("small")
    for call in (lambda: fast_reciprocal_NNs(feats[0], feats[1], S, ret_xy=False), lambda: extract_correspondences(feats, qonfs, subsample=S),
                 lambda: capi.dense_correspondences(feats, qonfs, S)):
        with pytest.raises(capi.MpsfmHipError) as e:
            call()
        assert e.value.code == ENODEVICE
