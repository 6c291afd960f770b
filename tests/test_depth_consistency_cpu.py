"""Depth-consistency check without a device: the NumPy restatement against vectors computed by the reference's own
DepthConsistencyChecker (tests/golden/make_golden_depth_consistency.py), the argument checks of
mpsfm_depth_consistency, and the host bookkeeping of the drop-in checker."""

import ctypes as C
import os
import types

import numpy as np
import pytest

import numpy_depth_consistency as NDC
from mpsfm_amd import capi
from mpsfm_amd.sfm.mapper import DepthConsistencyChecker

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_depth_consistency.npz")


def fixture_images(z):
    """The fixture's images as capi.depth_consistency entries (fresh copies of the unclamped maps)."""
    out = []
    for k in range(int(z["n_images"])):
        intr, (sx, sy) = z[f"im{k}_intr"], z[f"im{k}_sxsy"]
        out.append(dict(depth=z[f"im{k}_depth"].astype(np.float64), variance=z[f"im{k}_variance"].astype(np.float64),
                        prior_std_multiplier=float(z[f"im{k}_psm"]),
                        intr_scaled=(intr[0] * sx, intr[1] * sy, intr[2] * sx, intr[3] * sy), intr=intr,
                        cam_from_world=z[f"im{k}_cam_from_world"]))
    return out


def unpack(bits, shape):
    return np.unpackbits(bits)[: shape[0] * shape[1]].reshape(shape).astype(bool)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_fixture_is_small_and_has_the_cases(golden):
    assert os.path.getsize(GOLDEN) < 200_000
    shapes = {golden[f"im{k}_depth"].shape for k in range(int(golden["n_images"]))}
    assert len(shapes) == 2  # maps of different sizes
    assert (golden["im0_depth"] <= 0).any() and len(golden["clamped0_index"]) > 0


@pytest.mark.parametrize("si", [0, 1])
def test_restatement_equals_reference_masks(golden, si):
    s = float(golden["thresholds"][si])
    for pi, (a, b) in enumerate(golden["pairs"]):
        ims = fixture_images(golden)
        l12, l21 = NDC.pair(ims, int(a), int(b), s=s)
        assert not l12["near"].any() and not l21["near"].any()
        got = NDC.masks(l12, l21)
        for key in NDC.MASK_KEYS:
            shape = ims[int(a) if key.endswith("1") or key.startswith("valid1") else int(b)]["depth"].shape
            want = unpack(golden[f"s{si}_pair{pi}_{key}"], got[key].shape)
            assert want.shape == shape or key.endswith("mask")
            np.testing.assert_array_equal(got[key], want, err_msg=f"pair {pi} {key}")


@pytest.mark.parametrize("si", [0, 1])
def test_restatement_equals_reference_bundle_score(golden, si):
    s = float(golden["thresholds"][si])
    ims = fixture_images(golden)
    score, sums, counts, _ = NDC.bundle(ims, 0, [1, 2, 3], s=s)
    assert abs(score - float(golden[f"s{si}_bundle_score"])) <= 1e-12
    assert tuple(sums) == tuple(int(v) for v in golden[f"s{si}_bundle_sums"])
    assert counts[:, :, 1:].sum() > 0 and counts[:, :, 2].sum() > 0 and counts[:, :, 3].sum() > 0  # every class occurs


def test_restatement_clamps_in_place_like_the_reference(golden):
    ims = fixture_images(golden)
    before = ims[0]["depth"].copy()
    NDC.pair(ims, 0, 1)
    idx = golden["clamped0_index"]
    np.testing.assert_array_equal(ims[0]["depth"].ravel()[idx], golden["clamped0_value"])
    keep = np.ones(before.size, bool)
    keep[idx] = False
    np.testing.assert_array_equal(ims[0]["depth"].ravel()[keep], before.ravel()[keep])


def test_last_writer_wins_not_the_minimum():
    """find_min_buffer's effective semantics, which the restatement (and the kernel) implement: for colliding source
    pixels the buffer holds the depth of the largest source index, not the smallest depth."""
    chk = DepthConsistencyChecker.__new__(DepthConsistencyChecker)
    D = np.array([3.0, 1.0, 2.0, 5.0])
    P = np.array([[1, 0], [1, 0], [1, 0], [0, 1]])
    buf, mask = chk.find_min_buffer(D, P, (2, 2))
    assert mask.all()
    assert buf[0, 1] == 2.0 and buf[1, 0] == 5.0 and np.isinf(buf[0, 0])


# -- the C entry point: argument checks before any device work -------------------------------------------------------
def _raw(images, pa, pb, counts=None, n_images=None, n_pairs=None):
    arr = (capi.CDcImage * max(len(images), 1))()
    keep = []
    for k, im in enumerate(images):
        arr[k].H, arr[k].W = im["depth"].shape
        arr[k].depth, arr[k].variance = im["depth"].ctypes.data, im["variance"].ctypes.data
        arr[k].prior_std_multiplier = 1.0
        keep.append(im)
    pa = np.ascontiguousarray(pa, np.int32)
    pb = np.ascontiguousarray(pb, np.int32)
    cnt = np.zeros((max(len(pa), 1), 2, 4), np.int64) if counts is None else counts
    L = capi.lib()
    return L.mpsfm_depth_consistency(len(images) if n_images is None else n_images, C.addressof(arr),
                                     len(pa) if n_pairs is None else n_pairs, pa.ctypes.data, pb.ctypes.data, 15.0, 0.6, 0,
                                     cnt.ctypes.data if counts is not False else None, None, None)


def _tiny(n=3):
    return [dict(depth=np.full((4, 5), 2.0), variance=np.full((4, 5), 0.01), prior_std_multiplier=1.0,
                 intr_scaled=(5.0, 5.0, 2.0, 1.5), intr=(50.0, 50.0, 20.0, 15.0),
                 cam_from_world=np.hstack([np.eye(3), [[0.1 * k], [0.0], [0.0]]])) for k in range(n)]


def test_entry_point_is_exported():
    assert "mpsfm_depth_consistency" in capi.EXPORTS
    assert capi.lib().mpsfm_abi_version() == 2


@pytest.mark.parametrize("case", ["a_eq_b", "a_out_of_range", "b_negative", "null_counts", "zero_height", "negative_pairs",
                                  "null_depth"])
def test_bad_arguments_are_rejected_before_touching_the_device(case):
    ims = _tiny()
    pa, pb, kw = [0, 1], [1, 2], {}
    if case == "a_eq_b":
        pb = [1, 1]
        pa = [0, 1]
    elif case == "a_out_of_range":
        pa = [0, 3]
    elif case == "b_negative":
        pb = [1, -1]
    elif case == "null_counts":
        kw["counts"] = False
    elif case == "zero_height":
        ims[2]["depth"] = np.zeros((0, 5))
    elif case == "negative_pairs":
        kw["n_pairs"] = -1
    before = [im["depth"].copy() for im in ims]
    if case == "null_depth":
        arr = (capi.CDcImage * 2)()
        arr[0].H = arr[0].W = arr[1].H = arr[1].W = 4
        pa_, pb_ = np.array([0], np.int32), np.array([1], np.int32)
        cnt = np.zeros((1, 2, 4), np.int64)
        rc = capi.lib().mpsfm_depth_consistency(2, C.addressof(arr), 1, pa_.ctypes.data, pb_.ctypes.data, 15.0, 0.6, 0,
                                                cnt.ctypes.data, None, None)
    else:
        rc = _raw(ims, pa, pb, **kw)
    assert rc == -1, (case, rc, capi.lib().mpsfm_last_error())
    for im, b in zip(ims, before):  # nothing was clamped or written
        np.testing.assert_array_equal(im["depth"], b)


def test_empty_pair_list_is_a_no_op():
    ims = _tiny()
    ims[0]["depth"][0, 0] = -1.0
    assert _raw(ims, [], [], n_pairs=0) == 0
    assert ims[0]["depth"][0, 0] == -1.0  # no device work, no clamp
    counts, summary = capi.depth_consistency(ims, [])
    assert counts.shape == (0, 2, 4) and summary["n_legs"] == 0


def test_no_device_is_a_loud_failure_not_a_fallback():
    if capi.device_count() > 0:
        pytest.skip("a gfx950 device is visible")
    ims = _tiny()
    with pytest.raises(capi.MpsfmHipError) as e:
        capi.depth_consistency(ims, [(0, 1)])
    assert e.value.code == -2


# -- host bookkeeping of the drop-in checker (reference depthconsistency.py:26-51, :174-222) ---------------------------
def _host_scene(n=3):
    ims = {k: types.SimpleNamespace(name=f"im{k}", ignore_matches_AP={"x": 1}, failed_dc_check=True, last_dc_score=None,
                                    dc_times_inliers_resampled=0) for k in range(1, n + 1)}
    return types.SimpleNamespace(images=ims, last_ap_inlier_masks={})


def test_default_conf_and_attributes_are_the_references():
    chk = DepthConsistencyChecker({}, _host_scene(), None)
    assert dict(chk.conf) == {"depth_cons_valid_thresh": 0.6, "depth_cons_thresh": 0.15, "init_depth_cons_thresh": 0.09,
                              "init_valid_thresh": 0.8, "depth_consistency_resample": False, "verbose": 0}
    assert chk.depth_cons_thresh == 0.15 and chk.reg_batch_dc_times_failed == 0
    assert chk.cons_thresh_times_increased == 0 and chk.skip_dc_check is False
    for name in ("at_registration_success", "relax_thresholds", "find_min_buffer", "check_depth_consistency", "init_pair",
                 "pre_fail", "at_failure", "check_image", "check_bundle_depth_concistency"):
        assert callable(getattr(chk, name))


def test_relax_and_reset():
    rec = _host_scene()
    chk = DepthConsistencyChecker({"depth_cons_thresh": 0.2}, rec, None)
    chk.reg_batch_dc_times_failed = 4
    chk.relax_thresholds()
    chk.relax_thresholds()
    assert chk.depth_cons_thresh == 0.2 * 1.3 * 1.3
    assert chk.cons_thresh_times_increased == 2 and chk.reg_batch_dc_times_failed == 0
    assert all(im.ignore_matches_AP == {} and im.failed_dc_check is False for im in rec.images.values())
    chk.skip_dc_check = True
    chk.reg_batch_dc_times_failed = 3
    rec.images[2].failed_dc_check = True
    chk.at_registration_success()
    assert chk.depth_cons_thresh == 0.2 and chk.cons_thresh_times_increased == 0
    assert chk.reg_batch_dc_times_failed == 0 and chk.skip_dc_check is False
    assert rec.images[2].failed_dc_check is False


def test_failure_bookkeeping():
    rec = _host_scene()
    chk = DepthConsistencyChecker({}, rec, None)
    chk.at_failure(2)
    assert rec.images[2].failed_dc_check is True and chk.reg_batch_dc_times_failed == 1
    assert rec.images[2].dc_times_inliers_resampled == 0
    rs = DepthConsistencyChecker({"depth_consistency_resample": True}, rec, None)
    m = np.array([True, False, True])
    rec.last_ap_inlier_masks = {1: m.copy(), 3: np.zeros(0, bool)}
    rs.at_failure(2)
    assert rec.images[2].dc_times_inliers_resampled == 1 and rs.reg_batch_dc_times_failed == 1
    np.testing.assert_array_equal(rec.images[2].ignore_matches_AP[1], m)
    assert 3 not in rec.images[2].ignore_matches_AP
    rec.last_ap_inlier_masks = {1: np.array([True])}  # indexes the still-used entries
    rs.at_failure(2)
    np.testing.assert_array_equal(rec.images[2].ignore_matches_AP[1], [True, True, True])


def test_pre_fail():
    rec = _host_scene()
    chk = DepthConsistencyChecker({}, rec, None)
    assert chk.pre_fail(1) is False  # never checked
    rec.images[1].last_dc_score = 0.5
    chk.skip_dc_check = True
    assert chk.pre_fail(1) is False
    rs = DepthConsistencyChecker({"depth_consistency_resample": True}, rec, None)
    assert rs.pre_fail(1) is False  # inliers not resampled yet
    chk.skip_dc_check = False
    with pytest.raises(NotImplementedError):
        chk.pre_fail(1)


def test_empty_bundle_needs_no_device():
    chk = DepthConsistencyChecker({}, _host_scene(), None)
    score, sums = chk.check_bundle_depth_concistency(1, {"optim_ids": {1}})
    assert score == 0.0 and sums == (0, 0)
