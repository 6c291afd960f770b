"""CPU tests of the scene filter: every rule of mpsfm_filter_scene (include/mpsfm_hip.h) by hand through the restatement
(tests/numpy_scene_filter.py), the drop-in BundleFilter (mpsfm_amd/sfm/mapper/filtering.py) end to end against the reference's call
sequence as tests/mapper_replay.py replays it over HipObservationManager, and the refusals that need no device."""

import copy

import numpy as np
import pytest

import numpy_scene_filter as N
import scene_filter_scenes as S
from mapper_replay import MapperReplay
from numpy_scene import ObservationManager
from mpsfm_amd import capi
from mpsfm_amd.sfm.mapper.filtering import BundleFilter
from mpsfm_amd.sfm.scene.observations import HipObservationManager
from mpsfm_amd.sfm.scene.scene_queries import SceneQueries
from oracle import cpu_oracle as O

MAPPER_ANGLE = 0.001  # degrees


# ---- the rules by hand ------------------------------------------------------------------------------------------------------------------
def test_step0_counts_what_the_sequential_deletions_count():
    f, b = [0, 1, 2, 3], [4, 5, 6]  # cameras in front of the point / with the point behind them
    cams = S.line_cams(7, behind=b)
    tracks = {(2, 1): [f[0], b[0]], (3, 1): [f[0], f[1], b[0]], (3, 2): [f[0], b[0], b[1]], (4, 2): [f[0], f[1], b[0], b[1]],
              (4, 3): [f[0], b[0], b[1], b[2]]}
    args, kp_of = S.build(cams, [(S.POINT, S.track(t)) for t in tracks.values()])
    out = S.run_restatement(args, MAPPER_ANGLE)
    np.testing.assert_array_equal(out["point_fate"], [2, 1, 2, 1, 2])
    assert out["info"]["num_negative"] == 1 + 1 + 2 + 2 + 3
    assert out["info"]["n_points_deleted"] == 3 and out["info"]["n_observations_deleted"] == 3
    marks = {k: int(out["kp_deleted"][v]) for k, v in kp_of.items()}
    assert marks[(1, 4, 0)] == 1 and marks[(3, 4, 0)] == 1 and marks[(3, 5, 0)] == 1 and sum(marks.values()) == 3
    assert out["info"]["num_changed_a"] == 0 and out["info"]["num_changed_b"] == 0
    # without the step nothing is removed on its own: each of those points loses its elements behind a camera in pass B or dies there
    out = S.run_restatement(args, MAPPER_ANGLE, negative_depth=False)
    np.testing.assert_array_equal(out["point_fate"], [5, 1, 5, 1, 5])
    assert out["info"]["num_negative"] == 0 and out["info"]["num_changed_b"] == 2 + 1 + 3 + 2 + 4


def test_a_pass_removes_up_to_L_minus_2_bad_observations_and_kills_from_L_minus_1():
    cams = S.line_cams(4)
    args, kp_of = S.build(cams, [(S.POINT, S.track(range(4), bad=(0, 3))), (S.POINT, S.track(range(4), bad=(0, 1, 3))),
                                 (S.POINT, S.track([2])), (S.POINT, S.track(range(4)))])
    out = S.run_restatement(args, MAPPER_ANGLE, negative_depth=False)
    np.testing.assert_array_equal(out["point_fate"], [1, 5, 5, 0])
    assert out["info"]["num_changed_b"] == 2 + 4 + 1
    assert out["kp_deleted"][kp_of[(0, 0, 0)]] == 3 and out["kp_deleted"][kp_of[(0, 3, 0)]] == 3 and out["kp_deleted"].sum() == 6
    assert out["point_max_angle"][1] == 0.0 and 0 < out["point_max_angle"][0] < out["point_max_angle"][3]  # cameras 1, 2 / 0 .. 3


def test_the_error_bound_is_strict_and_the_cheirality_bound_is_not():
    cams = S.line_cams(3)
    on, above = [(0, 4.0, 0.0, False), (1, 0.0, 0.0, False), (2, 0.0, 0.0, False)], [(0, 4.0, 2.0**-24, False), (1, 0.0, 0.0, False), (2, 0.0, 0.0, False)]
    args, kp_of = S.build(cams, [(S.POINT, on), (S.POINT, above)])
    details = {}
    out = N.filter_scene(max_reproj_error=4.0, min_tri_angle_deg=MAPPER_ANGLE, details=details, **args)
    assert details["sq_err"][kp_of[(0, 0, 0)]] == 16.0 and details["sq_err"][kp_of[(1, 0, 0)]] == np.nextafter(16.0, 32.0)
    np.testing.assert_array_equal(out["point_fate"], [0, 1])
    assert out["kp_deleted"][kp_of[(1, 0, 0)]] == 3 and out["info"]["num_changed_b"] == 1
    # depths of exactly 2^-52 (in front), 2^-53 and 0 (not): the point (0, 1, 0) seen from (+-1, 0, -zc)
    cams = [(-1.0, 0.0, -(2.0**-52)), (1.0, 0.0, -(2.0**-52)), (2.0, 0.0, -(2.0**-53)), (4.0, 0.0, 0.0)]
    args, kp_of = S.build(cams, [((0.0, 1.0, 0.0), S.track(range(4)))])
    details = {}
    out = N.filter_scene(max_reproj_error=4.0, min_tri_angle_deg=MAPPER_ANGLE, details=details, **args)
    S.check_margins(details, args["kp_point"])
    np.testing.assert_array_equal(details["zc"][[kp_of[(0, i, 0)] for i in range(4)]], [2.0**-52, 2.0**-52, 2.0**-53, 0.0])
    np.testing.assert_array_equal(out["kp_deleted"][[kp_of[(0, i, 0)] for i in range(4)]], [0, 0, 1, 1])
    assert out["point_fate"][0] == 1 and out["info"]["num_negative"] == 2 and out["point_max_angle"][0] == pytest.approx(np.pi / 2, abs=1e-15)


@pytest.mark.parametrize("bundle, risky", [((0,), [1, 1, 1, 1, 1]), ((0, 1), [0, 1, 1, 1, 0]), ((0, 1, 2), [0, 0, 1, 0, 0]), ((0, 1, 6), [0, 0, 0, 0, 0])])
def test_the_risky_set_is_the_intersection_over_the_bundle_images(bundle, risky):
    args, _ = S.risky_scene(bundle)
    out = S.run_restatement(args, MAPPER_ANGLE, risky_deg=MAPPER_ANGLE)
    np.testing.assert_array_equal(out["point_risky"], risky)
    if bundle == (0, 1, 6):  # step 0 took the flagged element of image 6: without the step the point is a member
        out = S.run_restatement(args, MAPPER_ANGLE, risky_deg=MAPPER_ANGLE, negative_depth=False)
        np.testing.assert_array_equal(out["point_risky"], [0, 0, 0, 1, 0])


def test_a_flagged_keypoint_without_a_point_and_a_missing_bundle_make_no_member():
    args, _ = S.risky_scene((0,))
    assert args["kp_invalid_depth"][0] == 1 and args["kp_point"][0] == -1  # the first keypoint of image 0
    args["in_bundle"][:] = 0
    assert S.run_restatement(args, MAPPER_ANGLE)["point_risky"].sum() == 0
    args["in_bundle"] = None
    assert S.run_restatement(args, MAPPER_ANGLE)["point_risky"].sum() == 0


def test_a_point_in_both_sets_gets_both_passes_in_that_order():
    # images 0 and 1 see the point under 2^-9 rad = 0.11 degrees: below the 1.5 degrees of pass A, above the mapper's 0.001
    cams = S.line_cams(4)
    pair = S.track([0, 1], flagged=(0, 1))
    args, _ = S.build(cams, [(S.POINT, pair), (S.POINT, S.track([0, 1])), (S.POINT, pair), (S.POINT, S.track([0, 1]))], bundle=(0, 1))
    sel = np.array([0, 1, 1, 0], np.uint8)  # A only, B only, both, neither
    out = S.run_restatement(args, MAPPER_ANGLE, point_sel=sel)
    np.testing.assert_array_equal(out["point_risky"], [1, 0, 1, 0])
    np.testing.assert_array_equal(out["point_fate"], [4, 0, 4, 0])
    assert out["info"]["num_changed_a"] == 2 and out["info"]["num_changed_b"] == 0
    np.testing.assert_array_equal(out["point_max_angle"] > 0, [True, True, True, False])  # the point in neither set is not tested
    # every point selected (point_sel == NULL), and a pass A as lenient as pass B: all four stay
    out = S.run_restatement(args, MAPPER_ANGLE, risky_deg=MAPPER_ANGLE)
    np.testing.assert_array_equal(out["point_fate"], [0, 0, 0, 0])
    assert np.all(out["point_max_angle"] > 0)
    # pass A lets the point through and pass B does not
    out = S.run_restatement(args, 1.5, point_sel=sel, risky_deg=MAPPER_ANGLE)
    np.testing.assert_array_equal(out["point_fate"], [0, 6, 6, 0])
    assert out["info"]["num_changed_a"] == 0 and out["info"]["num_changed_b"] == 2


# ---- the drop-in end to end ---------------------------------------------------------------------------------------------------------------
def oracle_numerics(tracks, xyz, device):
    return O.filter_tracks(tracks, xyz)


class HostSceneQueries(SceneQueries):
    """The gathered arrays of a SceneQueries with the stand-in's local bundle in place of the library's."""

    def find_local_bundle_ids(self, refimid, num_images=None):
        return self.rec.find_local_bundle_ids(refimid, num_images or MapperReplay.local_ba_num_images)


def _pair(seed, prepare=None):
    a = S.make_filter_scene(seed)
    if prepare is not None:
        prepare(a)
    b = copy.deepcopy(a)
    b.obs = HipObservationManager(b, ObservationManager(b), numerics=oracle_numerics)
    return a, BundleFilter({}, a, HostSceneQueries(a, S.empty_graph(a)), backend=N.filter_scene), b, MapperReplay(b, None)


def test_filter_bundle_of_the_drop_in_equals_the_replayed_sequence():
    a, bf, b, replay = _pair(2)
    bundle = S.fixed_bundle(a)
    got, want = bf.filter_bundle(bundle), replay.filter_bundle(copy.deepcopy(bundle))
    fates = np.bincount(bf.last_result["point_fate"], minlength=7)
    print("fates 0 .. 6:", fates.tolist(), "risky:", int(bf.last_result["point_risky"].sum()), "returned:", got)
    assert np.all(fates > 0), "the scene must bring out every fate"
    assert got == want and got[0] > 50
    S.assert_same_scene(a, b)
    S.assert_same_errors(a, b)
    assert -1.0 in {p.error for p in a.points3D.values()}  # points outside both sets were not looked at
    # what is left is filtered again, with nothing but the second pass on every point
    got, want = bf.filter_all(), replay.filter_all()
    assert got == want
    S.assert_same_scene(a, b)
    S.assert_same_errors(a, b)
    assert min(p.error for p in a.points3D.values()) >= 0.0  # every point a pass looked at and kept has its mean reprojection error


def test_filter_all_and_the_two_point_filters_equal_the_replayed_sequence():
    a, bf, b, replay = _pair(3)
    got, want = bf.filter_all(), replay.filter_all()
    fates = np.bincount(bf.last_result["point_fate"], minlength=7)
    print("fates 0 .. 6:", fates.tolist(), "returned:", got)
    assert np.all(fates[[0, 1, 2, 5, 6]] > 0) and fates[3] == fates[4] == 0  # no bundle, no pass A
    assert got == want and got[0] > 50
    S.assert_same_scene(a, b)
    a, bf, b, replay = _pair(8)
    bundle = replay.find_local_bundle(2, 2)
    assert bf.filter_local_points3D(bundle, 4.0, 0.001) == replay.filter_local_points3D(bundle, 4.0, 0.001)
    S.assert_same_scene(a, b)
    assert bf.filter_all_points3D(4.0, 1.5) == (b.obs.filter_all_points3D(4.0, 1.5), True)
    S.assert_same_scene(a, b)
    S.assert_same_errors(a, b)
    assert bf.filter_images() == replay.filter_images() == set()


def test_an_image_that_loses_its_points_is_reported_as_filtered():
    def all_keypoints_off(sc):  # every observation of image 6 misses by a thousand pixels
        sc.images[6].kps += 1000.0

    a, bf, b, replay = _pair(5, all_keypoints_off)
    bundle = replay.find_global_bundle()
    got, want = bf.filter_bundle(bundle), replay.filter_bundle(bundle)
    assert got == want and 6 in got[1]
    S.assert_same_scene(a, b)


def test_the_bundles_equal_the_stand_ins():
    a, bf, b, replay = _pair(6)
    assert bf.find_global_bundle() == replay.find_global_bundle()
    for ref in (1, 4):
        for num in (None, 2):
            assert bf.find_local_bundle(ref, num) == replay.find_local_bundle(ref, num)
    assert bf.find_local_bundle(3, 0, return_points=False) == {"optim_ids": {3}}
    local = replay.find_local_bundle(2, 1)
    assert bf.find_subset_bundle(local) == replay.find_subset_bundle(local)
    a.images[5].has_pose = b.images[5].has_pose = False  # an image without a pose does not join a subset bundle ...
    for sc in (a, b):
        for pid in set(sc.images[5].point3D_ids(sc.images[5].get_observation_point2D_idxs()).tolist()):
            sc.obs.delete_point3D(pid)                   # ... and has no points
    assert bf.find_subset_bundle(local) == replay.find_subset_bundle(local)
    assert bf.find_global_bundle() == replay.find_global_bundle()
    got, want = bf.find_invalid_depth_points([1, 4]), replay.find_invalid_depth_points([1, 4])
    assert got == want and len(got[0]) > len(got[1]) > 0


def test_a_pointed_keypoint_in_an_unregistered_image_is_refused_by_name():
    a, bf, _, _ = _pair(6)
    a.images[4].has_pose = False
    with pytest.raises(ValueError, match="image 4"):
        bf.filter_all()
    with pytest.raises(ValueError, match="image 4"):
        bf.find_subset_bundle({"optim_ids": {1}})


# ---- refusals of the wrapper and of the library that need no device ------------------------------------------------------------------------
def test_the_empty_scenes_answer_without_a_device():
    v = S.valid_call()
    out = capi.filter_scene(**dict(v, xyz=np.zeros((0, 3)), kp_point=np.full(len(v["kp_point"]), -1)))
    assert out["info"]["num_syncs"] == 0 and len(out["point_fate"]) == 0 and not out["kp_deleted"].any() and not out["kp_sq_err"].any()
    n = len(v["registered"])
    out = capi.filter_scene(**dict(v, kp_start=np.zeros(n + 1, np.int64), kp_xy=np.zeros((0, 2)), kp_point=[], kp_invalid_depth=None, in_bundle=None))
    assert out["info"]["num_syncs"] == 0 and len(out["kp_deleted"]) == 0 and not out["point_fate"].any() and not out["point_max_angle"].any()


@pytest.mark.parametrize("change", [
    dict(max_reproj_error=-1.0), dict(max_reproj_error=np.nan), dict(max_reproj_error=np.inf), dict(min_tri_angle_deg=-1.0),
    dict(min_tri_angle_deg=np.nan), dict(risky_min_tri_angle_deg=-0.5), dict(risky_min_tri_angle_deg=np.inf),
    "kp_start_first", "kp_start_decreasing", "kp_point_large", "kp_point_small", "nan_xyz", "inf_pose", "nan_quat", "nan_intr", "unregistered"])
def test_the_library_refuses_bad_values_before_it_looks_for_a_device(change):
    v = S.valid_call()
    if isinstance(change, dict):
        v.update(change)
    elif change == "kp_start_first":
        v["kp_start"] = v["kp_start"].copy(); v["kp_start"][0] = 1
    elif change == "kp_start_decreasing":
        v["kp_start"] = v["kp_start"].copy(); v["kp_start"][1], v["kp_start"][2] = v["kp_start"][2], v["kp_start"][1]
    elif change == "kp_point_large":
        v["kp_point"] = v["kp_point"].copy(); v["kp_point"][1] = len(v["xyz"])
    elif change == "kp_point_small":
        v["kp_point"] = v["kp_point"].copy(); v["kp_point"][1] = -2
    elif change == "nan_xyz":
        v["xyz"] = v["xyz"].copy(); v["xyz"][2, 1] = np.nan
    elif change == "inf_pose":
        v["cam_t"] = v["cam_t"].copy(); v["cam_t"][3, 0] = np.inf
    elif change == "nan_quat":
        v["cam_quat_xyzw"] = v["cam_quat_xyzw"].copy(); v["cam_quat_xyzw"][0, 3] = np.nan
    elif change == "nan_intr":
        v["intr"] = v["intr"].copy(); v["intr"][5, 0] = np.nan
    elif change == "unregistered":
        v["registered"] = v["registered"].copy(); v["registered"][1] = 0
    with pytest.raises(capi.MpsfmHipError) as e:
        capi.filter_scene(**v)
    assert e.value.code == -1, str(e.value)  # MPSFM_EINVAL, not MPSFM_ENODEVICE


@pytest.mark.parametrize("change", [dict(in_bundle=np.zeros(3, np.uint8)), dict(kp_invalid_depth=np.zeros(2, np.uint8)), dict(point_sel=np.zeros(1, np.uint8)),
                                    dict(registered=np.ones(2, np.uint8)), dict(kp_point=np.zeros(3, np.int64)), dict(kp_start=[])])
def test_the_wrapper_refuses_arrays_of_the_wrong_length(change):
    with pytest.raises(ValueError, match="filter_scene"):
        capi.filter_scene(**dict(S.valid_call(), **change))
