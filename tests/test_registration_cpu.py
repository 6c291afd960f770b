"""CPU checks of registration (mpsfm_amd/sfm/mapper/registration.py, csrc/registration.hip) against
tests/golden/reference_registration.npz, which the reference's own MpsfmRegistration methods computed (see
tests/golden/make_golden_registration.py): the NumPy restatement of the two kernels, the drop-in's host logic driven through
that restatement, the argument checks of the two entry points, and the kernels' resource use.

Bounds (derived, not measured).  Integers, booleans, ids and orderings: exact.  Lifted points: per component
|d| <= 16 eps (|ray d| + |t|), eps = 2^-52: the lift is a division, a product, a subtraction and a three-term dot product per
component, each rounding relative to at most that size, and the reference rotates with R^T p - R^T t where the kernels use
R^T (p - t).  Angles: 32 eps / sqrt(1 - c^2) radians with c the argument of acos: the lengths, their sum and the quotient
carry a few eps of relative error, and acos amplifies an error of c by 1 / sqrt(1 - c^2).  Triangulated points: 1e-9
relative, as the estimator tests use (two routes to the null vector of a 4 x 4 system)."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import numpy_registration as NR
from mpsfm_amd import capi
from mpsfm_amd.sfm.mapper import MpsfmRegistration
from mpsfm_amd.sfm.mapper.registration import merge_candidates
from numpy_scene import Rigid3d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0**-52
KEYS = ("pt2d_id_1", "pt2d_id_2", "tri_angle", "posdepth1", "posdepth2", "xyz")
COLMAP_OPTIONS = {"init_min_tri_angle": 16.0, "abs_pose_min_num_inliers": 30}


@pytest.fixture(scope="module")
def Z():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_registration.npz"))


def spec_of(Z, tag):
    pre = f"{tag}_spec_"
    return {k[len(pre):]: Z[k] for k in Z.files if k.startswith(pre)}


def angle_bound_deg(c):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.rad2deg(32 * EPS / np.sqrt(1.0 - np.asarray(c) ** 2))


def assert_lift_close(got, want, scale):
    assert np.all(np.abs(got - want) <= 16 * EPS * scale[:, None]), np.abs(got - want).max()


class ScaleRecorder:
    """the restatement as the drop-in's backend, keeping the error scale of the lifted rows of every call"""

    def __init__(self):
        self.pairs = []

    def registration_pairs(self, refs, match_ref, ref_xy, match_pt, pts, pt_risky=None, lifted_registration=True, device=0):
        r = NR.registration_pairs(refs, match_ref, ref_xy, match_pt, pts, pt_risky, lifted_registration)
        self.pairs.append(r)
        return r["xyz"], r["kind"]

    init_pair_candidates = staticmethod(NR.init_pair_candidates)


def ap_answers(Z, tag):
    out = []
    for i in range(int(Z[f"{tag}_ap_calls"])):
        if bool(Z[f"{tag}_ap{i}_none"]):
            out.append(None)
            continue
        mask, pose = Z[f"{tag}_ap{i}_mask"], Z[f"{tag}_ap{i}_pose"]
        out.append({"cam_from_world": Rigid3d(pose[:4], pose[4:]), "num_inliers": int(mask.sum()), "inlier_mask": mask})
    return out


def make_next(Z, tag):
    min_inliers, half, best, lifted, resample = (int(v) for v in Z[f"{tag}_conf"])
    scene, corr = NR.registration_scene(spec_of(Z, "next"), risky_ids=Z["next_risky"])
    scene.best_next_ref_imid = best
    backend = ScaleRecorder()
    reg = MpsfmRegistration({"lifted_registration": bool(lifted), "resample_bunlde": bool(resample), "verbose": -1,
                             "colmap_options": dict(COLMAP_OPTIONS, abs_pose_min_num_inliers=min_inliers)}, scene, corr, None, backend=backend)
    reg.half_ap_min_inliers = half
    reg.absolute_pose_estimator = NR.ReplayEstimator(ap_answers(Z, tag))
    return scene, reg, backend


# ---- the restatement against the reference's rows ---------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["next_lifted", "next_plain"])
def test_restatement_reproduces_the_2D3D_pairs(Z, tag):
    scene, reg, backend = make_next(Z, tag)
    p2, p3, order, lifted, ids3d, sizes = reg._gather_2D3D_pairs(6, [5, 3, 1, 2, 4, 3])
    assert order == list(Z[f"{tag}_pass0_order"]) == [1, 2, 3, 4, 5]
    assert np.array_equal(lifted, Z[f"{tag}_pass0_lifted"])
    assert np.array_equal(ids3d, Z[f"{tag}_pass0_ids3d"])
    assert np.array_equal(p2, Z[f"{tag}_pass0_points2D"])
    want = Z[f"{tag}_pass0_points3D"]
    assert np.array_equal(p3[~lifted], want[~lifted])  # gathered points: copies
    r = backend.pairs[0]
    keep = r["kind"] != NR.DROPPED
    assert_lift_close(p3[lifted], want[lifted], r["scale"][keep][lifted])
    assert sizes[4] == 0 and sum(sizes) == len(p2)  # reference 5 has no matches
    assert scene.risky_calls == (1 if tag == "next_lifted" else 0)  # one call for the union of all references' ids
    if tag == "next_lifted":
        assert lifted.sum() > 300 and (r["d"][r["kind"] == NR.LIFTED] <= 0).any()  # zero padding / non-positive depths are lifted too
        risky = set(int(v) for v in Z["next_risky"])
        assert risky and not risky & set(ids3d.tolist())
    else:
        assert not lifted.any() and len(np.unique(ids3d)) < len(ids3d)


def check_init_candidates(Z, kind, fn):
    """`fn` (the restatement, or capi.init_pair_candidates on a device) against every candidate list the reference built"""
    tag = f"init_{kind}"
    spec = spec_of(Z, tag)
    m = spec["pair0_matches"]
    xy1, xy2 = spec["im1_kps"][m[:, 0]], spec["im2_kps"][m[:, 1]]
    maps = dict(prior_map=spec["im1_data_prior"], valid_map=spec["im1_valid"], sx=64 / 512.0, sy=48 / 384.0)
    E = Rigid3d(Z[f"{tag}_answer_E_quat"], Z[f"{tag}_answer_E_t"]).matrix()
    e_mask = Z[f"{tag}_answer_E_mask"]
    restated = NR.init_pair_candidates(xy1, xy2, spec["im1_intr"], spec["im2_intr"], E, **maps)
    assert not NR.fragile_init(restated)[e_mask].any() and not NR.near_valid(restated).any()
    first = fn(xy1, xy2, spec["im1_intr"], spec["im2_intr"], E, **maps)

    def check(rec, rows, o, P2, what):
        got = {k: Z[f"{tag}_rec{rec}_{k}"] for k in KEYS}
        assert str(Z[f"{tag}_rec{rec}_kind"]) == what
        assert np.array_equal(got["pt2d_id_1"], m[rows, 0]) and np.array_equal(got["pt2d_id_2"], m[rows, 1])
        assert len(rows) > 100
        pre = "tri" if what == "tri" else "lift"
        assert np.array_equal(got["posdepth1"], o[f"{pre}_posdepth1"][rows]) and np.array_equal(got["posdepth2"], o[f"{pre}_posdepth2"][rows])
        if what == "tri":
            assert np.allclose(got["xyz"], o["tri_xyz"][rows], rtol=1e-9, atol=0)
        else:
            assert_lift_close(o["lift_xyz"][rows], got["xyz"], np.sqrt((got["xyz"] ** 2).sum(1)))
        mm = NR.candidate_measures(P2, got["xyz"])  # the angle formula on the reference's own points
        assert np.all(np.abs(mm["angle"] - got["tri_angle"]) <= angle_bound_deg(mm["c"]))
        assert np.all(np.abs(o[f"{pre}_angle_deg"][rows] - got["tri_angle"]) <= 1e-9 * np.maximum(1, got["tri_angle"]))
        return got

    tri_rows = np.flatnonzero(e_mask & first["tri_ok"])
    check(0, tri_rows, first, E, "tri")
    if kind == "low":
        AP = Rigid3d(Z[f"{tag}_pp_ap0_pose"][:4], Z[f"{tag}_pp_ap0_pose"][4:]).matrix()
        rows = np.flatnonzero(first["valid"])[Z[f"{tag}_pp_ap0_mask"]]
        sel = np.zeros(len(m), np.uint8)
        sel[rows] = 1
        second = fn(xy1, xy2, spec["im1_intr"], spec["im2_intr"], AP, select=sel, **maps)
        assert not second["tri_ok"][sel == 0].any() and not second["lift_xyz"][sel == 0].any()
        check(1, rows, second, AP, "lift")
        check(2, rows[second["tri_ok"][rows]], second, AP, "tri")
        below = Z[f"{tag}_rec1_tri_angle"] < 1.5
        assert below.any() and (~below).any()  # the merge threshold divides the case
    else:
        # the lift's bound holds at the reference's own rescale (its triangulated depths over the sampled priors); the
        # rescale from `fn`'s triangulation agrees with it to the triangulation's tolerance
        with np.errstate(divide="ignore"):
            rescale = np.median(Z[f"{tag}_rec0_xyz"][:, 2] / first["d_prior"][tri_rows])
            own = np.median(first["tri_xyz"][tri_rows, 2] / first["d_prior"][tri_rows])
        assert abs(own - rescale) <= 1e-9 * abs(rescale)
        assert np.isfinite(rescale) and rescale > 0 and abs(rescale - 1) > 0.1  # the rescale matters
        rows = np.flatnonzero(e_mask & first["valid"])
        sel = np.zeros(len(m), np.uint8)
        sel[rows] = 1
        second = fn(xy1, xy2, spec["im1_intr"], spec["im2_intr"], E, rescale=rescale, select=sel, what=2, **maps)
        check(1, rows, second, E, "lift")
    # the absolute pose saw the valid lifted points of ALL matches, unscaled
    valid_rows = np.flatnonzero(first["valid"])
    assert (~first["valid"]).sum() > 10
    assert np.array_equal(Z[f"{tag}_pp_ap0_points2D"], xy2[valid_rows])
    assert_lift_close(first["lift_xyz"][valid_rows], Z[f"{tag}_pp_ap0_points3D"], np.sqrt((Z[f"{tag}_pp_ap0_points3D"] ** 2).sum(1)))


@pytest.mark.parametrize("kind", ["high", "low", "none"])
def test_restatement_reproduces_the_init_candidates(Z, kind):
    check_init_candidates(Z, kind, NR.init_pair_candidates)


def test_reference_angle_is_not_the_geometric_angle():
    # baseline 1, depths 4 to 8: about 22.6 degrees where the angle between the rays is about 8.4
    rng = np.random.default_rng(3)
    X = np.stack([rng.uniform(-1, 1, 20000), rng.uniform(-1, 1, 20000), rng.uniform(4, 8, 20000)], 1)
    C2 = np.array([1.0, 0.0, 0.0])
    ang, c = NR.reference_angle_deg(np.zeros(3), C2, X)
    u, w = X / np.linalg.norm(X, axis=1)[:, None], (X - C2) / np.linalg.norm(X - C2, axis=1)[:, None]
    true = np.rad2deg(np.arccos((u * w).sum(1)))
    assert 20 < ang.mean() < 25 and 7 < true.mean() < 10
    assert not np.isnan(ang).any() and (np.abs(c) <= 1).all()
    assert NR.reference_angle_deg(np.zeros(3), np.zeros(3), np.zeros((1, 3)))[0][0] == 0.0  # zero denominator
    a, _ = NR.reference_angle_deg(np.zeros(3), np.array([10.0, 0, 0]), np.array([[5.0, 0, 1e-9]]))
    assert np.isnan(a[0]) or a[0] >= 0  # acos argument below -1 by rounding would be NaN, as min(nan, x) in Python


def test_merge_pairs_common_candidates_by_position_and_judges_by_the_unfiltered_angles():
    def cand(ids, ang, base):
        n = len(ids)
        return {"pt2d_id_1": np.array(ids), "pt2d_id_2": np.arange(n) + base, "tri_angle": np.array(ang, float),
                "posdepth1": np.ones(n, bool), "posdepth2": np.ones(n, bool), "xyz": np.arange(3 * n, dtype=float).reshape(n, 3) + base}
    lifted = cand([5, 9, 7, 3, 9], [0.5, 9.0, 0.2, 1.0, 2.0], 100)
    tri = cand([8, 9, 5, 1], [0.1, 7.0, 3.0, 1.2], 200)
    out = merge_candidates(lifted, tri, 1.5)
    # common lifted rows (ids 5, 9, 9) pair with common triangulated rows (ids 9, 5) by position and are judged by the first
    # angles of the whole triangulated list (0.1 -> lifted, 7.0 -> triangulated); then lifted-only below 1.5 (ids 7, 3), then
    # triangulated-only at or above it (none: 0.1 and 1.2 are below)
    assert out["pt2d_id_1"].tolist() == [5, 5, 7, 3]
    assert out["pt2d_id_2"].tolist() == [100, 202, 102, 103]
    assert out["xyz"].shape == (4, 3) and out["posdepth1"].dtype == bool


# ---- the drop-in's host logic, the restatement in place of the two C calls -------------------------------------------------------
@pytest.mark.parametrize("tag", ["next_lifted", "next_plain", "next_resample", "next_resample_taken", "next_few", "next_forced", "next_none"])
def test_register_next_image_reproduces_the_reference(Z, tag):
    scene, reg, backend = make_next(Z, tag)
    ok = reg.register_next_image(6)
    assert ok == bool(Z[f"{tag}_return"])
    ap = reg.absolute_pose_estimator
    assert len(ap.calls) == int(Z[f"{tag}_ap_calls"]) == len(backend.pairs)
    for i, (p2, p3, camera) in enumerate(ap.calls):
        src = tag if f"{tag}_ap{i}_points2D" in Z.files else "next_lifted"
        assert camera is scene.rec.cameras[6]
        assert np.array_equal(p2, Z[f"{src}_ap{i}_points2D"])
        want = Z[f"{src}_ap{i}_points3D"]
        r = backend.pairs[i]
        n_tri = len(np.unique(Z[f"{src}_pass{i}_ids3d"]))
        assert np.array_equal(p3[:n_tri], want[:n_tri])  # triangulated block first, de-duplicated, first occurrence
        assert_lift_close(p3[n_tri:], want[n_tri:], r["scale"][r["kind"] == NR.LIFTED])
    if bool(Z[f"{tag}_has_masks"]):
        masks = scene.last_ap_inlier_masks
        assert list(masks) == list(Z[f"{tag}_mask_refs"])
        assert [len(v) for v in masks.values()] == list(Z[f"{tag}_mask_sizes"])
        assert np.array_equal(np.concatenate(list(masks.values())), Z[f"{tag}_mask_values"])
    else:
        assert scene.last_ap_inlier_masks is None
    ign = scene.images[6].ignore_matches_AP
    assert sorted(ign) == list(Z[f"{tag}_ignore_refs"])
    for r in ign:
        assert np.array_equal(ign[r], Z[f"{tag}_ignore_ref{r}"])
    assert scene.registration_order == list(Z[f"{tag}_registered"])
    assert scene.images[6].has_pose == ok
    if ok:
        assert np.array_equal(scene.images[6].cam_from_world.matrix(), Z[f"{tag}_pose"])
    if tag == "next_resample_taken":
        assert len(ap.calls) == 2 and set(ign) == {1, 2, 3, 4}  # the branch was taken once and wrote the ignore masks


def test_register_and_triangulate_next_image_calls_the_triangulator(Z):
    scene, reg, _ = make_next(Z, "next_lifted")

    class Tri:
        def triangulate_image(self, imid, **kw):
            return ("triangulated", imid)

    reg.triangulator = Tri()
    assert reg.register_and_triangulate_next_image(6) == ("triangulated", 6)
    scene, reg, _ = make_next(Z, "next_none")
    reg.triangulator = Tri()
    assert reg.register_and_triangulate_next_image(6) is False


def make_init(Z, tag):
    scene, corr = NR.registration_scene(spec_of(Z, tag))
    reg = MpsfmRegistration({"colmap_options": COLMAP_OPTIONS, "verbose": -1}, scene, corr, None, backend=NR.NumpyBackend())
    E = {"cam2_from_cam1": Rigid3d(Z[f"{tag}_answer_E_quat"], Z[f"{tag}_answer_E_t"]), "inlier_mask": Z[f"{tag}_answer_E_mask"]}
    reg.relative_pose_estimator = NR.ReplayEstimator([E])
    reg.absolute_pose_estimator = NR.ReplayEstimator(ap_answers(Z, f"{tag}_pp"))
    return scene, corr, reg


@pytest.mark.parametrize("kind", ["high", "low", "none"])
def test_init_pair_reproduces_the_reference(Z, kind):
    tag = f"init_{kind}"
    scene, corr, reg = make_init(Z, tag)
    cand, pose = reg._init_pair_points_and_pose(imid1=1, imid2=2, kps1=scene.keypoints(1), kps2=scene.keypoints(2),
                                                matches=corr.matches(1, 2), camera1=scene.camera(1), camera2=scene.camera(2))
    assert list(cand) == list(KEYS) and all(isinstance(v, list) for v in cand.values())
    want = {k: Z[f"{tag}_cand_{k}"] for k in KEYS}
    assert len({len(v) for v in cand.values()}) == 1
    for k in ("pt2d_id_1", "pt2d_id_2", "posdepth1", "posdepth2"):
        assert np.array_equal(np.array(cand[k]), want[k]), k
    assert np.allclose(np.array(cand["xyz"]), want["xyz"], rtol=1e-9, atol=1e-12)
    assert np.allclose(np.array(cand["tri_angle"]), want["tri_angle"], rtol=1e-9, atol=0)
    assert np.array_equal(pose.matrix(), Z[f"{tag}_cand_pose"])
    assert len(reg.absolute_pose_estimator.calls) == 1 and len(reg.relative_pose_estimator.calls) == 1

    scene, corr, reg = make_init(Z, tag)
    assert reg.register_and_triangulate_init_pair(1, 2) == bool(Z[f"{tag}_return"])
    assert scene.registration_order == list(Z[f"{tag}_registered"]) == [1, 2]
    assert np.array_equal(scene.images[1].cam_from_world.matrix(), Z[f"{tag}_pose1"])
    assert np.array_equal(scene.images[2].cam_from_world.matrix(), Z[f"{tag}_pose2"])
    new = sorted(p for p in scene.points3D if p not in (7, 11))
    tracks = np.array([[e.point2D_idx for e in scene.points3D[p].track.elements] for p in new], np.int64).reshape(-1, 2)
    assert np.array_equal(tracks, Z[f"{tag}_added_tracks"])  # added in the reference's order
    assert np.allclose(np.array([scene.points3D[p].xyz for p in new]).reshape(-1, 3), Z[f"{tag}_added_xyz"], rtol=1e-9, atol=1e-12)
    if kind != "low":
        assert len(new) > 100 and len(new) < len(want["xyz"])  # keypoints that carried a point or were matched twice are skipped


def test_init_pair_without_relative_pose_returns_false_and_leaves_the_scene(Z):
    scene, corr, reg = make_init(Z, "init_high")
    reg.relative_pose_estimator = NR.ReplayEstimator([None])
    before = (scene.images[1].cam_from_world, scene.images[2].cam_from_world, len(scene.points3D))
    assert reg.register_and_triangulate_init_pair(1, 2) is False
    assert (scene.images[1].cam_from_world, scene.images[2].cam_from_world, len(scene.points3D)) == before
    assert scene.registration_order == [] and not reg.absolute_pose_estimator.calls


def test_configuration_and_attributes_of_the_drop_in(Z):
    assert set(MpsfmRegistration.default_conf) == {"lifted_registration", "absolute_pose", "relative_pose", "reduce_min_inliers_at_failure",
                                                   "parallax_thresh", "combined_triangle_thresh", "robust_triangles", "resample_bunlde",
                                                   "colmap_options", "verbose"}
    from mpsfm_amd.sfm.estimators import AbsolutePose, RelativePose

    scene, corr = NR.registration_scene(spec_of(Z, "init_high"))
    reg = MpsfmRegistration({"colmap_options": COLMAP_OPTIONS}, scene, corr, "tri")
    assert isinstance(reg.absolute_pose_estimator, AbsolutePose) and isinstance(reg.relative_pose_estimator, RelativePose)
    assert reg.half_ap_min_inliers == 0 and reg.registration_cache["x"] == {} and reg.triangulator == "tri"
    assert reg.conf.reduce_min_inliers_at_failure == 6 and reg.backend is capi
    with pytest.raises(KeyError):
        MpsfmRegistration({"no_such_key": 1}, scene, corr, None)


# ---- the two entry points ---------------------------------------------------------------------------------------------------------
def _pairs_args(n=8, n_pts=4):
    rng = np.random.default_rng(0)
    refs = [dict(depth_map=rng.uniform(1, 5, (6, 8)), sx=0.1, sy=0.1, intr=[50, 50, 40, 30], quat_xyzw=[0, 0, 0, 1], t=[0, 0, 0]) for _ in range(2)]
    return dict(refs=refs, match_ref=rng.integers(0, 2, n), ref_xy=rng.uniform(0, 60, (n, 2)), match_pt=rng.integers(-1, n_pts, n),
                pts=rng.normal(size=(n_pts, 3)))


def test_wrappers_check_arguments_before_the_library_is_touched(monkeypatch):
    def no_lib():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(capi, "lib", no_lib)
    a = _pairs_args()
    for bad in (dict(match_ref=np.full(8, 2)), dict(match_ref=np.full(8, -1)), dict(match_pt=np.full(8, 4)), dict(match_pt=np.full(8, -2)),
                dict(ref_xy=np.zeros((7, 2))), dict(pt_risky=np.zeros(3, bool)),
                dict(refs=[dict(a["refs"][0], depth_map=np.ones((1, 8))), a["refs"][1]])):
        with pytest.raises(ValueError):
            capi.registration_pairs(**dict(a, **bad))
    xy = np.zeros((5, 2))
    K, P = [50, 50, 40, 30], np.eye(3, 4)
    maps = dict(prior_map=np.ones((4, 4)), valid_map=np.ones((4, 4)))
    for kw in (dict(xy2=np.zeros((4, 2))), dict(select=np.ones(4)), dict(what=0), dict(what=4), dict(prior_map=None),
               dict(prior_map=np.ones((1, 4)), valid_map=np.ones((1, 4))), dict(valid_map=np.ones((4, 5)))):
        args = dict(dict(xy1=xy, xy2=xy, intr1=K, intr2=K, cam2_from_cam1=P, **maps), **kw)
        with pytest.raises(ValueError):
            capi.init_pair_candidates(**args)


def test_entry_points_validate_on_the_host_and_need_a_device():
    L = capi.lib()
    ref = capi.CRegImage()
    m = np.ones((4, 4))
    ref.map_h, ref.map_w, ref.depth_map, ref.sx, ref.sy = 4, 4, m.ctypes.data, 1.0, 1.0
    ref.intr, ref.quat_xyzw = (C.c_double * 4)(1, 1, 0, 0), (C.c_double * 4)(0, 0, 0, 1)
    mr, mp = np.zeros(3, np.int32), np.array([0, -1, 1], np.int32)
    xy, pts, xyz, kind = np.zeros((3, 2)), np.zeros((2, 3)), np.zeros((3, 3)), np.zeros(3, np.uint8)

    def call(n_refs=1, n=3, mr=mr, mp=mp, n_pts=2, refp=C.addressof(ref), xyzp=xyz.ctypes.data, lifted=1):
        return L.mpsfm_registration_pairs(n_refs, refp, n, mr.ctypes.data, xy.ctypes.data, mp.ctypes.data, None, n_pts, pts.ctypes.data, lifted, 0,
                                          xyzp, kind.ctypes.data, None)

    assert call(n=-1) == -1 and call(n_refs=-1) == -1 and call(n_pts=-1) == -1
    assert call(refp=None) == -1 and call(xyzp=None) == -1
    assert call(mr=np.array([0, 1, 0], np.int32)) == -1 and call(mr=np.array([0, -1, 0], np.int32)) == -1
    assert call(mp=np.array([0, 2, 0], np.int32)) == -1 and call(mp=np.array([0, -2, 0], np.int32)) == -1
    ref.map_h = 1
    assert call() == -1
    ref.map_h = 4
    P, O = capi.CInitPair(), capi.CInitCandidates()
    assert L.mpsfm_init_pair_candidates(None, 0, C.byref(O)) == -1 and L.mpsfm_init_pair_candidates(C.byref(P), 0, None) == -1
    P.n_matches, P.what = 3, 3
    assert L.mpsfm_init_pair_candidates(C.byref(P), 0, C.byref(O)) == -1  # NULL arrays
    P.n_matches, P.what = -1, 1
    assert L.mpsfm_init_pair_candidates(C.byref(P), 0, C.byref(O)) == -1
    P.n_matches, P.what = 0, 5
    assert L.mpsfm_init_pair_candidates(C.byref(P), 0, C.byref(O)) == -1
    # well-formed calls: results with a device, MPSFM_ENODEVICE without one (no fallback)
    a = _pairs_args()
    xy1 = np.random.default_rng(1).uniform(0, 60, (6, 2))
    init = dict(xy1=xy1, xy2=xy1 + 1.0, intr1=[50, 50, 40, 30], intr2=[50, 50, 40, 30], cam2_from_cam1=np.c_[np.eye(3), [-1.0, 0, 0]],
                prior_map=np.full((6, 8), 4.0), valid_map=np.ones((6, 8)), sx=0.1, sy=0.1)
    if capi.device_count() > 0:
        xyz, kind = capi.registration_pairs(**a)
        assert set(kind.tolist()) <= {1, 2} and capi.init_pair_candidates(**init)["valid"].any()
    else:
        for fn, kw in ((capi.registration_pairs, a), (capi.init_pair_candidates, init)):
            with pytest.raises(capi.MpsfmHipError) as e:
                fn(**kw)
            assert e.value.code == -2


def test_kernels_compile_for_gfx950_without_scratch_or_lds():
    from mpsfm_amd import build

    assert "registration.hip" in build.SOURCES and "bilinear_sample.h" in build.HEADERS
    src = os.path.join(build.CSRC, "registration.hip")
    r = subprocess.run([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", src, "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    found = {}
    for name, body in re.findall(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (?:\d+)", r.stdout, flags=re.S):
        k = "k_reg_pairs" if "k_reg_pairs" in name else "k_init_candidates" if "k_init_candidates" in name else None
        if k:
            found[k] = (int(re.search(r"VGPRs: (\d+)", body).group(1)), int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", body).group(1)))
    assert set(found) == {"k_reg_pairs", "k_init_candidates"}, r.stdout
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stdout)]
    print("VGPRs, scratch:", found, "LDS:", lds)
    assert all(s == 0 for _, s in found.values()) and all(v == 0 for v in lds)
    assert all(v <= 128 for v, _ in found.values())  # at least 4 waves per SIMD
