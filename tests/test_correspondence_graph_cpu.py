"""The correspondence graph without a GPU: the restatement (tests/numpy_correspondence_graph.py) on cases small enough to write out
by hand, the entry point's argument checks and empty returns, which come before any device is touched, COLMAP's pair id, and
Correspondences' gathering and score sums against the fixture computed by the reference's own code
(tests/golden/make_golden_correspondences.py)."""

import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

import numpy_correspondence_graph as NG
from mpsfm_amd import capi
from mpsfm_amd.sfm.scene import correspondence_graph as CG
from mpsfm_amd.sfm.scene.correspondences import CorrespondenceStore, Correspondences, matches_from_matches0, sequential_sum

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_correspondences.npz"))
META = json.loads(str(GOLD["meta"]))
EINVAL, ENODEVICE, EUNSUPPORTED = -1, -2, -6


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_restatement_two_images_by_hand():
    # image 0: 2 keypoints (global 0, 1), image 1: 3 keypoints (global 2, 3, 4)
    g = NG.build([0, 2, 5], *NG.lists_of([(0, 1, [[0, 0], [1, 2], [0, 0], [0, 1], [2, 0], [0, 3], [-1, 0]]), (1, 0, [[2, 1], [1, 1]]), (1, 1, [[0, 1]])]))
    assert g["match_status"].tolist() == [0, 0, 3, 0, 1, 1, 1, 3, 0, 2]
    assert g["corr_start"].tolist() == [0, 2, 4, 5, 7, 8] and g["corr_kp"].tolist() == [2, 3, 3, 4, 0, 0, 1, 1]
    assert g["image_num_correspondences"].tolist() == [4, 4] and g["image_num_observations"].tolist() == [2, 3]
    assert g["kp_two_view"].tolist() == [0, 0, 0, 0, 0]
    assert (g["pair_image0"].tolist(), g["pair_image1"].tolist(), g["pair_start"].tolist()) == ([0], [1], [0, 4])
    assert g["pair_matches"].tolist() == [[0, 0], [0, 1], [1, 1], [1, 2]]


def test_restatement_two_view_observations_and_the_pair_view_by_hand():
    # three images of 2 keypoints: (0,0)-(1,0) alone; (0,1)-(1,1)-(2,1) a chain; image 2's keypoint 0 unmatched
    g = NG.build([0, 2, 4, 6], *NG.lists_of([(2, 1, [[1, 1]]), (1, 0, [[0, 0], [1, 1]])]))
    assert g["match_status"].tolist() == [0, 0, 0]
    assert g["corr_start"].tolist() == [0, 1, 2, 3, 5, 5, 6] and g["corr_kp"].tolist() == [2, 3, 0, 1, 5, 3]
    assert g["kp_two_view"].tolist() == [1, 0, 1, 0, 0, 0]  # (0, 1) has one partner, but that partner has two
    assert g["image_num_observations"].tolist() == [2, 2, 1] and g["image_num_correspondences"].tolist() == [2, 3, 1]
    assert list(zip(g["pair_image0"].tolist(), g["pair_image1"].tolist())) == [(0, 1), (1, 2)] and g["pair_start"].tolist() == [0, 2, 3]
    assert g["pair_matches"].tolist() == [[0, 0], [1, 1], [1, 1]]
    empty = NG.build([0], *NG.lists_of([]))
    assert empty["corr_start"].tolist() == [0] and len(empty["corr_kp"]) == 0 and empty["pair_start"].tolist() == [0]


def test_pair_id_is_colmaps():
    assert CG.MAX_NUM_IMAGES == 2147483647
    assert CG.image_pair_to_pair_id(3, 8) == CG.image_pair_to_pair_id(8, 3) == 3 * 2147483647 + 8
    assert CG.pair_id_to_image_pair(CG.image_pair_to_pair_id(41, 7)) == (7, 41)
    assert CG.image_pair_to_pair_id(1, 1) == 2147483648


# ---- the entry point without a device ---------------------------------------------------------------------------------------------------
Pt = lambda a: None if a is None else a.ctypes.data  # noqa: E731


def test_corr_graph_build_checks_arguments_before_any_device():
    L = capi.lib()
    kp = np.array([0, 2, 5], np.int64)
    li0, li1, ls = np.array([0], np.int32), np.array([1], np.int32), np.array([0, 2], np.int64)
    m = np.array([[0, 0], [1, 2]], np.int32)
    st, cs, ck, nc = np.zeros(2, np.uint8), np.zeros(6, np.int64), np.zeros(4, np.int64), C.c_int64(7)
    ic, io, tv, npairs = np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(5, np.uint8), C.c_int64(7)
    p0, p1, ps, pm = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(2, np.int64), np.zeros((2, 2), np.int32)
    base = dict(n_images=2, kp=kp, n_lists=1, li0=li0, li1=li1, ls=ls, m=m, st=st, cs=cs, ck=ck, nc=C.addressof(nc), ic=ic, io=io, tv=tv,
                npairs=C.addressof(npairs), p0=p0, p1=p1, ps=ps, pm=pm, info=None)

    def call(**kw):
        a = dict(base, **kw)
        ptr = lambda v: v if v is None or isinstance(v, int) else Pt(v)  # noqa: E731
        return L.mpsfm_corr_graph_build(a["n_images"], ptr(a["kp"]), a["n_lists"], ptr(a["li0"]), ptr(a["li1"]), ptr(a["ls"]), ptr(a["m"]), 0,
                                        ptr(a["st"]), ptr(a["cs"]), ptr(a["ck"]), a["nc"], ptr(a["ic"]), ptr(a["io"]), ptr(a["tv"]), a["npairs"],
                                        ptr(a["p0"]), ptr(a["p1"]), ptr(a["ps"]), ptr(a["pm"]), None if a["info"] is None else C.addressof(a["info"]))

    assert call(n_images=-1) == EINVAL and call(n_lists=-1) == EINVAL
    for name in ("kp", "li0", "li1", "ls", "m", "st", "cs", "ck", "nc", "ic", "io", "tv", "npairs", "p0", "p1", "ps", "pm"):
        assert call(**{name: None}) == EINVAL, name
        assert b"NULL" in L.mpsfm_last_error()
    assert call(kp=np.array([1, 2, 5], np.int64)) == EINVAL and call(ls=np.array([1, 2], np.int64)) == EINVAL
    assert call(kp=np.array([0, 5, 2], np.int64)) == EINVAL and b"kp_start" in L.mpsfm_last_error()
    assert call(n_lists=2, li0=np.array([0, 0], np.int32), li1=np.array([1, 1], np.int32), ls=np.array([0, 2, 1], np.int64)) == EINVAL
    for bad in (-1, 2):
        assert call(li0=np.array([bad], np.int32)) == EINVAL and call(li1=np.array([bad], np.int32)) == EINVAL
        assert b"out of range" in L.mpsfm_last_error()
    # the limits: read from the two start arrays, nothing of that size is touched
    assert call(kp=np.array([0, 2, 1 << 31], np.int64)) == EUNSUPPORTED
    assert call(ls=np.array([0, 1 << 30], np.int64)) == EUNSUPPORTED
    assert b"2^31" in L.mpsfm_last_error()
    # a valid call: computed with a device, refused loudly without one
    want = 0 if capi.device_count() > 0 else ENODEVICE
    assert call() == want
    if want == ENODEVICE:
        with pytest.raises(capi.MpsfmHipError) as e:
            capi.corr_graph_build(kp, li0, li1, ls, m)
        assert e.value.code == ENODEVICE
        g = CG.HipCorrespondenceGraph()
        g.add_image(1, 2)
        g.add_image(2, 3)
        g.add_correspondences(1, 2, m)
        with pytest.raises(capi.MpsfmHipError):  # the build is the first query's
            g.num_correspondences_for_image(1)


def test_empty_inputs_return_without_a_device():
    e = capi.corr_graph_build([0], [], [], [0], np.zeros((0, 2), np.int32))  # no image
    assert e["corr_start"].tolist() == [0] and e["pair_start"].tolist() == [0] and len(e["corr_kp"]) == 0 and len(e["match_status"]) == 0
    assert e["info"] == dict(num_added=0, num_invalid=0, num_self_pairs=0, num_duplicates=0, num_launches=0, num_syncs=0, ms=0.0)
    e = capi.corr_graph_build([0, 3, 5], [0, 1], [1, 0], [0, 0, 0], np.zeros((0, 2), np.int32))  # lists without a match
    assert e["corr_start"].tolist() == [0] * 6 and e["kp_two_view"].tolist() == [0] * 5 and e["image_num_correspondences"].tolist() == [0, 0]
    assert e["image_num_observations"].tolist() == [0, 0] and len(e["pair_image0"]) == 0 and e["pair_matches"].shape == (0, 2)
    args = ([0, 0, 0], *NG.lists_of([(0, 1, [[0, 0], [1, -1]]), (1, 1, [[0, 0]])]))  # images without keypoints: no index is in range
    e = capi.corr_graph_build(*args)
    NG.assert_equal(e, NG.build(*args))
    assert e["match_status"].tolist() == [1, 1, 2] and e["info"]["num_invalid"] == 2 and e["info"]["num_self_pairs"] == 1
    with pytest.raises(ValueError):
        capi.corr_graph_build([0, 3], [0], [0], [0, 2], [[0, 0]])
    with pytest.raises(ValueError):
        capi.corr_graph_build([0, 3], [0], [0, 0], [0, 1], [[0, 0]])
    g = CG.HipCorrespondenceGraph()  # the class on an empty graph: no device either
    g.add_image(5, 0)
    g.add_image(2, 0)
    g.add_correspondences(5, 2, [[0, 0]])
    assert g.num_correspondences_for_image(5) == 0 and g.rejected() == {"invalid": 1, "self_pair": 0, "duplicate": 0}
    assert g.num_images() == 2 and g.exists_image(5)
    g.finalize()
    assert g.num_images() == 0 and not g.exists_image(5) and g.image_pairs() == [] and g.num_correspondences_between_all_images() == {}
    assert g.csr()["image_ids"] == [2, 5] and g.csr()["corr_start"].tolist() == [0]
    with pytest.raises(RuntimeError):
        g.add_image(9, 1)
    with pytest.raises(KeyError):
        g.num_correspondences_for_image(5)


# ---- Correspondences against the reference's own code ---------------------------------------------------------------------------------------
def store_of(matcher):
    """the fixture's inputs as a CorrespondenceStore; pair 0 is stored under the other order of its names, pair 1 in the hloc layout"""
    store = CorrespondenceStore([tuple(p) for p in META["pairs"]], matcher_type=matcher)
    for name in META["names"]:
        store.set_sparse_keypoints(name, GOLD[f"in/skp/{name}"])
    for k, (n0, n1) in enumerate(META["stored"]):
        store.set_sparse_matches(n0, n1, GOLD[f"in/sm/{k}"], GOLD[f"in/ss/{k}"])
        store.set_dense(n0, n1, GOLD[f"in/dk0/{k}"], GOLD[f"in/dk1/{k}"], GOLD[f"in/dm/{k}"], GOLD[f"in/ds/{k}"])
        store.set_cached_scores(n0, n1, GOLD[f"in/dm/{k}"], GOLD[f"in/cs/{k}"])
    return store


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("mode", list(META["modes"]))
def test_gathering_and_score_sums_equal_the_reference_s(mode):
    matcher, matches_mode = META["modes"][mode]
    pairs = [tuple(p) for p in META["pairs"]]
    c = Correspondences({"matches_mode": matches_mode}, None, store_of(matcher))
    before = {k: GOLD[k].copy() for k in GOLD.files if k.startswith("in/")}
    kps, matches, scores, masks = c.gather_correspondences(pairs, set(META["names"]))
    assert set(kps) == set(META["names"]) and list(matches) == pairs
    for name in META["names"]:
        assert same(kps[name], GOLD[f"{mode}/kp/{name}"]), name
        if matcher == "dense":
            assert same(masks[name], GOLD[f"{mode}/mask/{name}"]), name
    assert (masks is None) == (matcher == "sparse")
    for k, pair in enumerate(pairs):
        assert same(matches[pair], GOLD[f"{mode}/m/{k}"]), pair
        assert same(scores[frozenset(pair)], GOLD[f"{mode}/s/{k}"]), pair
    assert len(matches[pairs[META["empty"]]]) == 0
    store = c.extractor  # gathering left the store as it was
    assert all(same(store.sparse_keypoints[n], before[f"in/skp/{n}"]) for n in META["names"])
    assert all(same(store.matches["dense"][tuple(p)][0], before[f"in/dm/{k}"]) for k, p in enumerate(META["stored"]))
    # the score sums over the fixture's inlier masks
    c.sparse_im_masks = masks
    c._two_view_geom = {pair: SimpleNamespace(inlier_matches=matches[pair][GOLD[f"{mode}/inl/{k}"]]) for k, pair in enumerate(pairs)}
    inlier = {pair: GOLD[f"{mode}/inl/{k}"] for k, pair in enumerate(pairs)}
    for cached in (False, True):
        if f"{mode}/sum{int(cached)}/0" not in GOLD.files:
            assert cached and matcher == "sparse"
            continue
        c.conf.cached_dense_scores = cached
        sums = c.gather_matches_scores(inlier, scores, matches)
        assert list(sums) == [frozenset(p) for p in pairs]
        for k, pair in enumerate(pairs):
            assert same(sums[frozenset(pair)], GOLD[f"{mode}/sum{int(cached)}/{k}"]), (pair, cached)


def test_sequential_sum_is_python_s_sum_and_the_hloc_layout():
    x = (np.random.default_rng(1).uniform(0.1, 1, 1000)).astype(np.float32)
    assert sequential_sum(x) == sum(x) and type(sequential_sum(x)) is np.float32
    assert sequential_sum(x[:0]) == 0 and sequential_sum(x.astype(np.float16)) == sum(x.astype(np.float16))
    m, s = matches_from_matches0(np.array([-1, 4, -1, 0]), np.array([0.0, 0.5, 0.0, 0.25], np.float16))
    assert m.tolist() == [[1, 4], [3, 0]] and s.tolist() == [0.5, 0.25] and s.dtype == np.float16
    store = CorrespondenceStore([("a", "b")])
    store.set_sparse_matches("a", "b", matches0=[-1, 4, -1, 0], matching_scores0=np.array([0.0, 0.5, 0.0, 0.25], np.float16))
    assert store.get_matches("sparse", "b", "a")[0].tolist() == [[4, 1], [0, 3]]
    with pytest.raises(ValueError):
        store.get_matches("sparse", "a", "c")


def test_two_view_geom_of_both_orientations_and_the_pass_through():
    from mpsfm_amd.sfm.estimators.two_view_geometry import TwoViewGeometry

    c = Correspondences(None, None, CorrespondenceStore([]))
    F = np.arange(9.0).reshape(3, 3)
    c._two_view_geom["a", "b"] = TwoViewGeometry(3, F=F, inlier_matches=np.array([[1, 2], [3, 4]], np.uint32))
    tvg, ok = c.two_view_geom("a", "b")
    assert ok and tvg is c._two_view_geom["a", "b"]
    inv, ok = c.two_view_geom("b", "a")
    assert ok and np.array_equal(inv.F, F.T) and inv.inlier_matches.tolist() == [[2, 1], [4, 3]]
    assert np.array_equal(c._two_view_geom["a", "b"].F, F)  # the stored copy stays
    assert c.two_view_geom("a", "c") == (None, False)
    assert c.num_image_pairs() == 0 and c.exists_image(1) is False  # passed through to cg, an empty graph
    with pytest.raises(AttributeError):
        c.no_such_method
    with pytest.raises(KeyError):
        Correspondences({"no_such_key": 1})


def test_graph_arrays_takes_the_csr_only_from_a_graph_of_the_scene_s_images():
    from mpsfm_amd.sfm.mapper.track_engine import graph_arrays

    cam = SimpleNamespace(params=np.array([1200.0, 1200.0, 800.0, 600.0]))
    scene = SimpleNamespace(images={i: SimpleNamespace(points2D=range(n), camera_id=0) for i, n in ((4, 2), (9, 3))},
                            keypoints=lambda i: np.zeros((len(scene.images[i].points2D), 2)), rec=SimpleNamespace(cameras={0: cam}))
    g = CG.HipCorrespondenceGraph()  # no match: built without a device
    g.add_image(4, 2)
    g.add_image(9, 3)
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ga = graph_arrays(g, scene)
    assert ga["corr_start"].tolist() == [0] * 6 and len(ga["corr_kp"]) == 0 and ga["kp_start"].tolist() == [0, 2, 5]
    short = CG.HipCorrespondenceGraph()  # an image left out: the arrays would index other keypoints
    short.add_image(9, 3)
    with pytest.warns(RuntimeWarning, match="pair by pair"):
        ga = graph_arrays(short, scene)
    assert ga["corr_start"].tolist() == [0] * 6
