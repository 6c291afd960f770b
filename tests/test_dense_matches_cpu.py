"""Dense-match thinning without a GPU: the NumPy restatement (tests/numpy_dense_matches.py) against the fixture computed by
the reference's own sparse_nms / assign_keypoints (tests/golden/make_golden_dense_matches.py), and the entry points' argument
checks, which come before any device is touched."""

import ctypes as C
import os

import numpy as np
import pytest

import numpy_dense_matches as ND
from mpsfm_amd import capi
from mpsfm_amd.extraction.pairwise import utils as U

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_dense_matches.npz"))
RADIUS = float(GOLD["radius"])
EINVAL, ENODEVICE = -1, -2


@pytest.mark.parametrize("case", ["float_distinct", "int_distinct", "ties"])
def test_restatement_equals_the_reference_nms(case):
    pts, sc, want = GOLD[f"{case}_points"], GOLD[f"{case}_scores"], GOLD[f"{case}_kept"]
    order = GOLD[f"{case}_order"] if f"{case}_order" in GOLD else None
    assert np.array_equal(ND.sparse_nms(pts, sc, RADIUS, order=order), want)
    if case != "ties":  # distinct scores: the order is determined, with or without `order`
        assert np.array_equal(ND.sparse_nms(pts, sc, RADIUS), want)


def test_restatement_equals_the_reference_two_pass_leg():
    g = {k: GOLD[f"combined_separated_{k}"] for k in ("sparse0", "sparse1", "dense0", "dense1", "dscores", "kept")}
    for flag in (True, False):  # every sparse point survives: the slice is exact
        got = ND.thin_dense_mask(g["dense0"], g["dense1"], g["dscores"], g["sparse0"], g["sparse1"], RADIUS, flag)
        assert np.array_equal(got, g["kept"])


def test_restatement_equals_the_reference_assignment():
    got = ND.assign_keypoints(GOLD["assign_query"], GOLD["assign_kps"], float(GOLD["assign_max_error"]))
    assert np.array_equal(got, GOLD["assign_ids"])


def test_restatement_alive_mask_is_the_compacted_problem():
    """Points that start out suppressed neither keep nor suppress: the suppression over the rest, in the same relative order."""
    rng = np.random.default_rng(5)
    pts, sc = rng.random((400, 2)) * 60, np.round(rng.random(400) * 6)
    alive = rng.random(400) < 0.6
    sub = np.flatnonzero(alive)
    assert np.array_equal(ND.sparse_nms(pts, sc, 6.0, alive=alive), sub[ND.sparse_nms(pts[sub], sc[sub], 6.0)])


def _nms(n, pts, sc, order, radius, keep, kept, info=None, device=0):
    L = capi.lib()
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    return L.mpsfm_radius_nms(n, p(pts), p(sc), p(order), radius, device, p(keep), p(kept), info)


def test_radius_nms_checks_arguments_before_any_device():
    pts, sc = np.array([[0.0, 0.0], [1.0, 1.0], [9.0, 9.0]]), np.array([3.0, 2.0, 1.0])
    keep, kept = np.zeros(3, np.uint8), np.zeros(1, np.int64)
    assert _nms(-1, pts, sc, None, 6.0, keep, kept) == EINVAL
    assert _nms(3, None, sc, None, 6.0, keep, kept) == EINVAL
    assert _nms(3, pts, None, None, 6.0, keep, kept) == EINVAL
    assert _nms(3, pts, sc, None, 6.0, None, kept) == EINVAL
    assert _nms(3, pts, sc, None, 6.0, keep, None) == EINVAL
    for bad in (np.nan, np.inf, -np.inf):
        assert _nms(3, pts, sc, None, bad, keep, kept) == EINVAL
        q = pts.copy(); q[1, 1] = bad
        assert _nms(3, q, sc, None, 6.0, keep, kept) == EINVAL
        s = sc.copy(); s[2] = bad
        assert _nms(3, pts, s, None, 6.0, keep, kept) == EINVAL
    assert _nms(3, pts, sc, None, -1.0, keep, kept) == EINVAL
    for order in ([0, 1, 1], [0, 1, 3], [-1, 0, 1]):
        assert _nms(3, pts, sc, np.array(order, np.int64), 6.0, keep, kept) == EINVAL
        assert b"permutation" in capi.lib().mpsfm_last_error()
    wide = np.array([[-1.7e308, 0.0], [1.7e308, 0.0], [0.0, 0.0]])
    assert _nms(3, wide, sc, None, 6.0, keep, kept) == EINVAL
    assert _nms((1 << 27) + 1, pts, sc, None, 6.0, keep, kept) == EINVAL
    # a valid call: computed with a device, refused loudly without one
    rc = _nms(3, pts, sc, np.array([2, 1, 0], np.int64), 6.0, keep, kept)
    assert rc == (0 if capi.device_count() > 0 else ENODEVICE)


def test_thin_and_assign_check_arguments_before_any_device():
    L = capi.lib()
    s, d, sc = np.zeros((2, 2)), np.arange(8.0).reshape(4, 2), np.ones(4)
    keep, kept = np.zeros(4, np.uint8), np.zeros(1, np.int64)
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def thin(ns=2, s0=s, s1=s, nd=4, d0=d, d1=d, scores=sc, radius=6.0, k=keep, nk=kept):
        return L.mpsfm_thin_dense_matches(ns, P(s0), P(s1), nd, P(d0), P(d1), P(scores), radius, 1, 0, P(k), P(nk), None)

    assert thin(ns=-1) == EINVAL and thin(nd=-1) == EINVAL
    assert thin(s0=None) == EINVAL and thin(s1=None) == EINVAL and thin(d0=None) == EINVAL and thin(d1=None) == EINVAL
    assert thin(scores=None) == EINVAL and thin(k=None) == EINVAL and thin(nk=None) == EINVAL
    assert thin(radius=np.nan) == EINVAL and thin(radius=-2.0) == EINVAL
    bad = d.copy(); bad[3, 0] = np.inf
    assert thin(d1=bad) == EINVAL
    assert thin(scores=np.array([1.0, np.nan, 1.0, 1.0])) == EINVAL
    assert thin(s1=np.array([[0.0, np.nan], [0.0, 0.0]])) == EINVAL
    assert thin(nd=0) == 0 and kept[0] == 0  # nothing to thin: no device needed
    assert thin() == (0 if capi.device_count() > 0 else ENODEVICE)

    q, k, ids = np.zeros((3, 2)), np.ones((2, 2)), np.zeros(3, np.int64)

    def assign(nq=3, qq=q, nk=2, kk=k, err=2.0, out=ids):
        return L.mpsfm_assign_keypoints(nq, P(qq), nk, P(kk), err, 0, P(out), None)

    assert assign(nq=-1) == EINVAL and assign(nk=-1) == EINVAL
    assert assign(qq=None) == EINVAL and assign(kk=None) == EINVAL and assign(out=None) == EINVAL
    assert assign(err=np.nan) == EINVAL and assign(err=np.inf) == EINVAL and assign(err=-1.0) == EINVAL
    assert assign(qq=np.array([[0.0, 0.0], [np.nan, 0.0], [0.0, 0.0]])) == EINVAL
    assert assign(kk=np.array([[0.0, 0.0], [0.0, -np.inf]])) == EINVAL
    assert assign(nq=0) == 0
    ids[:] = 7
    assert assign(nk=0) == 0 and ids.tolist() == [-1, -1, -1]  # no keypoints: all -1 without a launch
    assert assign() == (0 if capi.device_count() > 0 else ENODEVICE)


def test_python_layer_handles_empty_inputs_without_a_device():
    e2, e1 = np.zeros((0, 2), np.float32), np.zeros(0, np.float32)
    assert U.sparse_nms(e2, e1, 6.0).tolist() == []
    assert capi.radius_nms(e2, e1, 6.0).tolist() == []
    assert U.assign_keypoints(e2, np.ones((3, 2)), 4.0).tolist() == []
    assert U.assign_keypoints(np.ones((3, 2)), e2, 4.0).tolist() == [-1, -1, -1]
    assert capi.assign_keypoints_ids(np.ones((3, 2)), e2, 4.0).tolist() == [-1, -1, -1]
    a, b, c = U.thin_dense_matches(e2, e2, e1, np.ones((2, 2)), np.ones((2, 2)))
    assert a.shape == (0, 2) and b.shape == (0, 2) and c.shape == (0,)
    assert capi.thin_dense_matches_mask(e2, e2, e1, np.ones((2, 2)), np.ones((2, 2))).tolist() == []
    with pytest.raises(ValueError):
        U.thin_dense_matches(np.ones((2, 2)), np.ones((2, 2)), np.ones(2), skpts0_matched=np.ones((1, 2)))
    with pytest.raises(ValueError):
        capi.radius_nms(np.ones((3, 2)), np.ones(2), 6.0)


def test_calls_fail_loudly_without_a_device():
    if capi.device_count() > 0:
        return  # with a device the same calls are computed: tests/test_gpu_dense_matches.py
    pts, sc = GOLD["float_distinct_points"][:50], GOLD["float_distinct_scores"][:50]
    for call in (lambda: U.sparse_nms(pts, sc, RADIUS), lambda: U.assign_keypoints(pts, pts[:10], 4.0),
                 lambda: U.thin_dense_matches(pts, pts, sc, pts[:5], pts[:5])):
        with pytest.raises(capi.MpsfmHipError) as e:
            call()
        assert e.value.code == ENODEVICE
