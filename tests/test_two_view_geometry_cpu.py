"""CPU checks of the two-view geometry estimator: the NumPy restatement's mathematics against independent facts, COLMAP's
decision table on one synthetic pair per configuration, the host logic of the drop-ins (estimate_calibrated_two_view_geometry,
TwoViewGeometry.invert, geometric_verification) driven through the restatement, the argument checks of
mpsfm_two_view_geometry before any device is touched, the cand_start[0] check of mpsfm_tri_estimate_batch, and the resource
use of the new kernels."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import numpy_relative_pose as NR
import numpy_two_view_geometry as TV
from mpsfm_amd import capi
from mpsfm_amd.sfm.estimators import TwoViewGeometry, TwoViewGeometryConfig, estimate_calibrated_two_view_geometry
from mpsfm_amd.sfm.scene.correspondences import geometric_verification, process_pair


def _true_F(s):
    t, R = s["t"], s["R"]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return TV.canonical(np.linalg.inv(TV.Kmat(NR.INTR2)).T @ tx @ R @ np.linalg.inv(TV.Kmat(NR.INTR1)))


# ---- the restatement's mathematics ---------------------------------------------------------------------------------------
def test_seven_point_models_satisfy_their_constraints_and_contain_the_truth():
    s = TV.synthetic_pair("general", 7, 0.0, seed=3)
    p1, p2 = s["points1"], s["points2"]
    models = TV.seven_point(p1, p2)
    assert 1 <= len(models) <= 3
    Q = TV._q_rows(p1, p2)
    for F in models:
        assert abs(np.linalg.norm(F) - 1) < 1e-12 and F.reshape(-1)[np.argmax(np.abs(F))] > 0
        # unit-norm F against rows of pixel monomials: the constraint relative to the row's own length
        assert np.abs(Q @ F.reshape(-1) / np.linalg.norm(Q, axis=1)).max() < 1e-10
        assert abs(np.linalg.det(F)) < 1e-10
    keys = [tuple(F.reshape(-1)) for F in models]
    assert keys == sorted(keys)
    assert min(np.abs(F - _true_F(s)).max() for F in models) < 1e-6  # seven unnormalised pixel rows are ill-conditioned
    assert TV.seven_point(np.tile(p1[:1], (7, 1)), np.tile(p2[:1], (7, 1))) == []  # rank 1: no model


def test_four_point_homography_maps_its_sample_and_refuses_collinear_points():
    s = TV.synthetic_pair("planar", 4, 0.0, seed=5)
    p1, p2 = s["points1"], s["points2"]
    (H,) = TV.homography_dlt(p1, p2)
    assert abs(np.linalg.norm(H) - 1) < 1e-12
    assert TV.h_residual(H, p1, p2).max() < 1e-16
    q1 = p1.copy()
    q1[2] = 0.5 * (q1[0] + q1[1])
    assert TV.homography_dlt(q1, p2) == []
    assert TV.homography_dlt(p1, np.tile(p2[:1], (4, 1))) == []
    assert TV.h_residual(np.array([[1.0, 0, 0], [0, 1, 0], [0, 0, 0]]), p1, p2).min() == TV.DBL_MAX


def test_homography_decomposition_contains_the_truth():
    rng = np.random.default_rng(2)
    K1, K2 = np.array(NR.INTR1), np.array(NR.INTR2)
    for _ in range(5):
        R = NR._rot(rng.normal(size=3), rng.uniform(0.05, 0.4))
        t = rng.normal(size=3)
        nrm = np.array([0, 0, 1.0]) + 0.3 * rng.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        d = rng.uniform(4, 9)
        H = TV.Kmat(K2) @ (R + np.outer(t, nrm) / d) @ np.linalg.inv(TV.Kmat(K1))
        for sign in (1.0, -3.0):  # any scale, either sign
            cands = TV.decompose_homography(sign * H, K1, K2)
            assert len(cands) == 4
            assert min(max(np.abs(Rc - R).max(), np.abs(tc - t / d).max()) for Rc, tc in cands) < 1e-9
            for Rc, _ in cands:
                assert np.abs(Rc @ Rc.T - np.eye(3)).max() < 1e-9 and abs(np.linalg.det(Rc) - 1) < 1e-9
            (Ra, ta), (Rb, tb), (Rc, tc), (Rd, td) = cands  # OUR order
            assert tuple(Ra.reshape(-1)) < tuple(Rb.reshape(-1)) and np.array_equal(Ra, Rc) and np.array_equal(Rb, Rd)
            assert np.array_equal(ta, -tc) and np.array_equal(tb, -td) and ta[np.argmax(np.abs(ta))] > 0 and tb[np.argmax(np.abs(tb))] > 0
        # a pure rotation: the single candidate with t = 0
        (single,) = TV.decompose_homography(-2.0 * TV.Kmat(K2) @ R @ np.linalg.inv(TV.Kmat(K1)), K1, K2)
        assert np.abs(single[0] - R).max() < 1e-12 and not single[1].any()


def test_eight_point_recovers_the_true_fundamental_matrix_by_both_routes():
    s = TV.synthetic_pair("general", 60, 0.0, seed=9)
    for route in ("svd", "gram"):
        (F,) = TV.eight_point(s["points1"], s["points2"], route=route)
        assert np.abs(F - _true_F(s)).max() < 1e-8
        assert abs(np.linalg.det(F)) < 1e-15
    assert TV.eight_point(s["points1"][:7], s["points2"][:7]) == []


def test_triangulation_angle_is_the_geometric_one():
    X = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1e9], [0.5, 0.0, 0.0]])
    a = TV.triangulation_angle(np.zeros(3), np.array([1.0, 0.0, 0.0]), X)
    assert abs(a[0] - np.pi / 4) < 1e-15 and a[1] < 1e-8 and a[2] == 0.0  # pi folds to 0


# ---- the decision table ------------------------------------------------------------------------------------------------------
def _estimate(s, **o):
    return TV.estimate(s["points1"], s["points2"], s["intr1"], s["intr2"], s["size1"], s["size2"], compute_relative_pose=True, **o)


@pytest.mark.parametrize("kind,config", [("general", 2), ("wrong_intrinsics", 3), ("planar", 4), ("rotation", 5), ("watermark", 7)])
def test_decision_table(kind, config):
    s = TV.synthetic_pair(kind, 150, 0.3, seed=1, noise_px=0.5)
    r = _estimate(s, seed=1)
    L = r["legs"]
    print(kind, "config", r["config"], {k: (v["num_inliers"], v["num_trials"]) for k, v in L.items() if v})
    assert r["config"] == config == s["expect"] and r["success"]
    nE, nF, nH = (L[k]["num_inliers"] for k in "EFH")
    if kind == "wrong_intrinsics":
        assert nE / nF <= 0.95  # E loses more than 5 % of F's inliers
    if kind in ("general", "wrong_intrinsics"):
        assert nH / max(nE, nF) <= 0.8 and r["tri_angle"] > 0
    if kind == "general":
        assert np.abs(r["cam2_from_cam1"][:, :3] - s["R"]).max() < 5e-3 and r["num_cheirality_points"] == r["num_inliers"]
        assert (r["inlier_mask"] & s["inliers"]).sum() >= 0.95 * s["inliers"].sum()
    if kind == "planar":
        P = r["cam2_from_cam1"]
        assert np.abs(P[:, :3] - s["R"]).max() < 5e-3 and P[:, 3] @ s["t"] > 0.99 * np.linalg.norm(P[:, 3])
    if kind == "rotation":
        assert not r["cam2_from_cam1"][:, 3].any() and r["tri_angle"] == 0.0 and r["num_cheirality_points"] == 0
    if kind == "watermark":
        assert r["watermark"] and L["T"]["num_inliers"] >= 0.7 * r["num_inliers"]
        assert np.array_equal(r["cam2_from_cam1"], np.eye(3, 4)) and r["tri_angle"] == 0.0
        assert _estimate(s, seed=1, detect_watermark=False)["config"] in (4, 5)


def test_random_and_too_few_matches_are_degenerate():
    s = TV.synthetic_pair("random", 60, 0.0, seed=2)
    r = _estimate(s, max_num_trials=600)
    assert r["config"] == 1 and not r["success"] and not r["inlier_mask"].any()
    assert max(r["legs"][k]["num_inliers"] for k in "EFH") < 15
    assert np.array_equal(r["cam2_from_cam1"], np.eye(3, 4)) and r["tri_angle"] == 0.0
    s = TV.synthetic_pair("general", 14, 0.0, seed=2)
    r = _estimate(s)
    assert r["config"] == 1 and r["legs"]["E"] is None and len(r["inlier_mask"]) == 14 and not r["inlier_mask"].any()


# ---- the drop-ins' host logic, the restatement as the backend ---------------------------------------------------------------
class Restatement:
    """numpy_two_view_geometry behind capi.two_view_geometry's signature"""

    def __init__(self):
        self.calls = []

    def two_view_geometry(self, p1, p2, K1, K2, s1, s2, device=0, batch_trials=0, **o):
        self.calls.append(dict(o, n=len(p1), size1=tuple(s1), size2=tuple(s2)))
        r = TV.estimate(p1, p2, K1, K2, s1, s2, **o)
        z = np.zeros((3, 3))
        return dict(r, E=z if r["E"] is None else r["E"], F=z if r["F"] is None else r["F"], H=z if r["H"] is None else r["H"])


class _Cam:
    def __init__(self, params, model="PINHOLE", size=None):
        self.model, self.params = model, np.asarray(params, np.float64)
        if size is not None:
            self.width, self.height = size


class _Image:
    def __init__(self, name, image_id, camera_id):
        self.name, self.image_id, self.camera_id = name, image_id, camera_id


class _Reconstruction:
    def __init__(self):
        self.images, self.cameras = {}, {}


def _pair_data(kind="general", n=120, seed=4, shuffle=True):
    """keypoints of two images and the match rows into them, the matches in shuffled keypoint order"""
    s = TV.synthetic_pair(kind, n, 0.25, seed=seed, noise_px=0.5)
    rng = np.random.default_rng(seed)
    o0, o1 = (rng.permutation(n), rng.permutation(n)) if shuffle else (np.arange(n), np.arange(n))
    kps0, kps1 = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
    kps0[o0], kps1[o1] = s["points1"], s["points2"]
    return s, kps0, kps1, np.c_[o0, o1].astype(np.int32)


def test_estimate_returns_what_the_reference_reads():
    s, kps0, kps1, m = _pair_data()
    be = Restatement()
    cams = _Cam(s["intr1"], size=s["size1"]), _Cam(s["intr2"], size=s["size2"])
    tvg = estimate_calibrated_two_view_geometry(cams[0], kps0, cams[1], kps1, m,
                                                {"ransac": {"max_num_trials": 20000, "min_inlier_ratio": 0.1, "max_error": 4.0},
                                                 "compute_relative_pose": True}, backend=be)
    call = be.calls[0]
    assert call["seed"] == 0 and call["max_num_trials"] == 20000 and call["min_inlier_ratio"] == 0.1 and call["confidence"] == 0.999
    assert call["compute_relative_pose"] is True and call["min_num_inliers"] == 15 and call["size1"] == s["size1"]
    assert isinstance(tvg, TwoViewGeometry) and isinstance(tvg.config, TwoViewGeometryConfig)
    assert tvg.config == 2 and tvg.config in (2, 3) and tvg.config not in (4, 5) and int(tvg.config) == 2  # find_init_pairs' plain ints
    assert tvg.inlier_matches.dtype == m.dtype and tvg.inlier_matches.shape[1] == 2 and len(tvg.inlier_matches) >= 80
    assert set(map(tuple, tvg.inlier_matches)) <= set(map(tuple, m))
    M = tvg.cam2_from_cam1.matrix()
    assert np.abs(M[:, :3] - s["R"]).max() < 5e-3 and 0 < tvg.tri_angle < np.pi / 2
    assert tvg.E.shape == tvg.F.shape == tvg.H.shape == (3, 3)
    # a negative seed maps to 0, another seed is passed on
    estimate_calibrated_two_view_geometry(cams[0], kps0, cams[1], kps1, m[:10], {"ransac": {"random_seed": 7}}, backend=be)
    assert be.calls[-1]["seed"] == 7 and be.calls[-1]["compute_relative_pose"] is False
    with pytest.raises(NotImplementedError):
        estimate_calibrated_two_view_geometry(_Cam([800, 640, 480, 0.01], "SIMPLE_RADIAL"), kps0, cams[1], kps1, m, backend=be)
    with pytest.raises(NotImplementedError):
        estimate_calibrated_two_view_geometry(cams[0], kps0, cams[1], kps1, m, {"multiple_models": True}, backend=be)
    with pytest.raises(KeyError):
        estimate_calibrated_two_view_geometry(cams[0], kps0, cams[1], kps1, m, {"ransac": {"max_eror": 2}}, backend=be)
    with pytest.raises(IndexError):
        estimate_calibrated_two_view_geometry(cams[0], kps0[:5], cams[1], kps1, m, backend=be)
    empty = estimate_calibrated_two_view_geometry(cams[0], kps0, cams[1], kps1, np.zeros((0, 2), np.int32), backend=be)
    assert empty.config == 1 and empty.inlier_matches.shape == (0, 2)


def test_invert_round_trips():
    s, kps0, kps1, m = _pair_data("planar", seed=6)
    tvg = process_pair(dict(cam0=_Cam(s["intr1"], size=s["size1"]), cam1=_Cam(s["intr2"], size=s["size2"]), kps0=kps0, kps1=kps1, matches=m,
                            name0="a", name1="b"), 4.0, backend=Restatement())[0]
    assert tvg.config == 4
    E, F, H, M, im = tvg.E.copy(), tvg.F.copy(), tvg.H.copy(), tvg.cam2_from_cam1.matrix().copy(), tvg.inlier_matches.copy()
    tvg.invert()
    assert np.array_equal(tvg.E, E.T) and np.array_equal(tvg.F, F.T) and np.abs(tvg.H @ H - np.eye(3) * (tvg.H @ H)[0, 0]).max() < 1e-9
    Mi = tvg.cam2_from_cam1.matrix()
    assert np.abs(Mi[:, :3] @ M[:, :3] - np.eye(3)).max() < 1e-12 and np.abs(Mi[:, :3] @ M[:, 3] + Mi[:, 3]).max() < 1e-12
    assert np.array_equal(tvg.inlier_matches, im[:, ::-1])
    tvg.invert()
    assert np.abs(tvg.E - E).max() == 0 and np.abs(tvg.H - H).max() < 1e-12 and np.abs(tvg.cam2_from_cam1.matrix() - M).max() < 1e-12
    assert np.array_equal(tvg.inlier_matches, im)


def test_geometric_verification_masks_equal_the_references_isin_expression():
    rec = _Reconstruction()
    kps, matches, truth = {}, {}, {}
    names = [("a.jpg", "b.jpg"), ("c.jpg", "d.jpg")]
    for k, (n0, n1) in enumerate(names):
        s, k0, k1, m = _pair_data(seed=10 + k)
        if k == 1:  # a duplicated match row (an outlier and an inlier one): every copy shares one answer
            out, inl = np.nonzero(~s["inliers"])[0][0], np.nonzero(s["inliers"])[0][0]
            m = np.r_[m, m[[out, inl]]]
        for j, (name, kp, intr, size) in enumerate(((n0, k0, s["intr1"], s["size1"]), (n1, k1, s["intr2"], s["size2"]))):
            iid = 2 * k + j + 1
            rec.images[iid] = _Image(name, iid, iid)
            rec.cameras[iid] = _Cam(intr, size=size)
            kps[name] = kp
        matches[n0, n1] = m
        truth[n0, n1] = s
    be = Restatement()
    masks, cache = geometric_verification(rec, names, max_error=4.0, keypoints=kps, matches=matches, backend=be)
    assert set(masks) == set(cache) == set(names)
    assert [c["n"] for c in be.calls] == [120, 122] and all(c["max_num_trials"] == 20000 and c["compute_relative_pose"] for c in be.calls)
    for key in names:
        m, tvg = matches[key], cache[key]
        want = np.isin(m.view([("", m.dtype)] * 2), tvg.inlier_matches.view([("", tvg.inlier_matches.dtype)] * 2))[:, 0]
        assert masks[key].dtype == bool and masks[key].shape == (len(m),) and np.array_equal(masks[key], want)
        assert tvg.config == 2 and masks[key].sum() >= 80
        assert np.array_equal(masks[key], tvg.estimate["inlier_mask"])
    m = matches[names[1]]
    assert masks[names[1]][120] == masks[names[1]][np.nonzero((m[:120] == m[120]).all(axis=1))[0][0]]
    assert masks[names[1]][121] == masks[names[1]][np.nonzero((m[:120] == m[121]).all(axis=1))[0][0]]
    assert masks[names[1]][121] and not masks[names[1]][120]


# ---- the entry point's argument checks ------------------------------------------------------------------------------------
def _default_options():
    L = capi.lib()
    o = capi.CTwoViewOptions()
    L.mpsfm_two_view_default_options(C.byref(o))
    return o


def _call(n, p1, p2, K1, K2, s1=(1280, 960), s2=(1200, 1000), o=None, mask=True, res=True):
    L = capi.lib()
    if o is None:
        o = _default_options()
    m = np.zeros(max(n, 1) if n < 2**20 else 1, np.uint8)
    r = capi.CTwoViewResult()
    s1 = None if s1 is None else np.asarray(s1, np.int32)
    s2 = None if s2 is None else np.asarray(s2, np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    return L.mpsfm_two_view_geometry(n, ptr(p1), ptr(p2), ptr(K1), ptr(K2), ptr(s1), ptr(s2), C.byref(o) if o is not False else None, 0,
                                     m.ctypes.data if mask else None, C.byref(r) if res else None)


def test_default_options_are_colmaps():
    o = _default_options()
    d = capi.TWO_VIEW_DEFAULTS
    for k in ("max_error", "min_inlier_ratio", "confidence", "dyn_num_trials_multiplier", "min_num_trials", "max_num_trials", "seed",
              "batch_trials"):
        assert getattr(o.ransac, k) == d[k]
    for k in ("min_num_inliers", "min_E_F_inlier_ratio", "max_H_inlier_ratio", "watermark_min_inlier_ratio", "watermark_border_size",
              "detect_watermark", "compute_relative_pose"):
        assert getattr(o, k) == d[k]
    assert (d["max_error"], d["min_inlier_ratio"], d["confidence"], d["min_num_trials"], d["max_num_trials"]) == (4.0, 0.25, 0.999, 100, 10000)
    assert (d["min_num_inliers"], d["min_E_F_inlier_ratio"], d["max_H_inlier_ratio"]) == (15, 0.95, 0.8)
    assert {k: v for k, v in TV.DEFAULT_OPTIONS.items()} == {k: v for k, v in d.items() if k != "batch_trials"}


def test_entry_point_validates_arguments_first():
    p1, p2, K1, K2, *_ = NR.synthetic_problem(20, 0.0, seed=1)
    p1, p2, K1, K2 = (np.ascontiguousarray(a) for a in (p1, p2, K1, K2))
    einval = -1
    assert _call(20, None, p2, K1, K2) == einval
    assert _call(20, p1, None, K1, K2) == einval
    assert _call(20, p1, p2, None, K2) == einval
    assert _call(20, p1, p2, K1, None) == einval
    assert _call(20, p1, p2, K1, K2, s1=None) == einval
    assert _call(20, p1, p2, K1, K2, s2=None) == einval
    assert _call(20, p1, p2, K1, K2, o=False) == einval
    assert _call(20, p1, p2, K1, K2, mask=False) == einval
    assert _call(20, p1, p2, K1, K2, res=False) == einval
    for n in (-1, 2**31):
        assert _call(n, p1, p2, K1, K2) == einval
    assert _call(20, p1, p2, K1, K2, s1=(0, 960)) == einval and _call(20, p1, p2, K1, K2, s2=(1200, -1)) == einval
    for which, k in ((0, 0), (0, 7), (1, 3), (1, 39)):
        args = [p1.copy(), p2.copy()]
        args[which].reshape(-1)[k] = np.nan if k % 2 else np.inf
        assert _call(20, *args, K1, K2) == einval
    for which in (0, 1):
        Ks = [K1.copy(), K2.copy()]
        Ks[which][which] = 0.0  # a zero focal length
        assert _call(20, p1, p2, *Ks) == einval
        Ks = [K1.copy(), K2.copy()]
        Ks[which][2] = np.nan
        assert _call(20, p1, p2, *Ks) == einval
    for field, value in (("max_error", 0.0), ("min_inlier_ratio", 0.0), ("min_inlier_ratio", 1.5), ("confidence", 1.5),
                         ("dyn_num_trials_multiplier", 0.0), ("min_num_trials", -1), ("max_num_trials", 10), ("batch_trials", -3),
                         ("batch_trials", 1 << 20)):
        o = _default_options()
        setattr(o.ransac, field, value)
        assert _call(20, p1, p2, K1, K2, o=o) == einval
    for field, value in (("min_num_inliers", -1), ("min_E_F_inlier_ratio", 1.5), ("min_E_F_inlier_ratio", float("nan")),
                         ("max_H_inlier_ratio", -0.1), ("watermark_min_inlier_ratio", 0.0), ("watermark_border_size", 0.7),
                         ("detect_watermark", 2), ("compute_relative_pose", -1)):
        o = _default_options()
        setattr(o, field, value)
        assert _call(20, p1, p2, K1, K2, o=o) == einval
    assert b"options" in capi.lib().mpsfm_last_error()
    with pytest.raises(KeyError):
        capi.two_view_geometry(p1, p2, K1, K2, (1280, 960), (1200, 1000), max_eror=3.0)
    with pytest.raises(ValueError):
        capi.two_view_geometry(p1, p2[:5], K1, K2, (1280, 960), (1200, 1000))
    with pytest.raises(capi.MpsfmHipError) as e:
        capi.two_view_geometry(p1, p2, K1, K2, (1280, 0), (1200, 1000))
    assert e.value.code == -1


def test_entry_point_without_device_fails_loudly():
    if capi.device_count() > 0:
        pytest.skip("a gfx950 device is visible")
    p1, p2, K1, K2, *_ = NR.synthetic_problem(20, 0.0, seed=1)
    with pytest.raises(capi.MpsfmHipError) as e:
        capi.two_view_geometry(p1, p2, K1, K2, (1280, 960), (1200, 1000))
    assert e.value.code == -2


def test_tri_estimate_batch_rejects_a_first_offset_other_than_zero():
    P = np.tile(np.eye(3, 4).reshape(1, 12), (4, 1))
    K = np.tile([[800.0, 800.0, 640.0, 480.0]], (4, 1))
    xy = np.tile([[640.0, 480.0]], (4, 1))
    for cs in ([1, 3, 4], [-1, 2, 4]):
        with pytest.raises(capi.MpsfmHipError) as e:
            capi.tri_estimate_batch(cs, P, K, xy, 0.0, 0.03)
        assert e.value.code == -1
        # the library's own check, without the wrapper's
        cs_ = np.asarray(cs, np.int64)
        c = capi.CTriCandidates(2, cs_.ctypes.data, P.ctypes.data, K.ctypes.data, xy.ctypes.data, 0.0, 0.03, 0, None)
        xyz, ok, inl = np.zeros((2, 3)), np.zeros(2, np.uint8), np.zeros(4, np.uint8)
        L = capi.lib()
        assert L.mpsfm_tri_estimate_batch(C.byref(c), 0, xyz.ctypes.data, ok.ctypes.data, inl.ctypes.data) == -1
        assert b"cand_start[0]" in L.mpsfm_last_error()


# ---- the kernels ------------------------------------------------------------------------------------------------------------
NEW_KERNELS = ("k_tv_f7", "k_tv_h4", "k_tv_t1", "k_tv_moments", "k_tv_gram", "k_tv_tsum", "k_tv_pose")


def test_new_kernels_compile_for_gfx950_without_scratch():
    from mpsfm_amd import build

    assert "two_view.hip" in build.SOURCES and {"two_view_math.h", "rel_pose_problem.h"} <= set(build.HEADERS)
    src = os.path.join(build.CSRC, "two_view.hip")
    r = subprocess.run([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", src, "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    found = {}
    for name, body, lds in re.findall(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", r.stdout, flags=re.S):
        for k in NEW_KERNELS + ("k_lo_score", "k_lo_mask", "k_rp_five"):
            if k in name:
                tag = k + ("<H>" if "Lb1" in name else "<F>" if "Lb0" in name else "<T>" if "TvTranslation" in name else
                           "<E>" if "RpProblem" in name else "")
                found[tag] = (int(re.search(r"VGPRs: (\d+)", body).group(1)), int(lds),
                              int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", body).group(1)))
    print("kernel: (VGPRs, LDS bytes, scratch bytes)")
    for k, v in sorted(found.items()):
        print(f"  {k}: {v}")
    for k in NEW_KERNELS:
        hits = [v for name, v in found.items() if name.startswith(k)]
        assert hits, (k, r.stdout)
        assert all(scratch == 0 for _, _, scratch in hits), (k, hits)
    for tag in ("k_lo_score<F>", "k_lo_score<H>", "k_lo_score<T>", "k_lo_mask<F>", "k_lo_mask<H>"):
        assert found[tag][2] == 0
    assert found["k_tv_f7"][1] <= 64 * 1024 and found["k_tv_h4"][1] <= 64 * 1024  # the per-thread LDS slices fit a workgroup's 64 KiB
