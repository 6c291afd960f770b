"""GPU tests of mpsfm_filter_scene (csrc/scene_filter.hip) against the sequential restatement tests/numpy_scene_filter.py on the
hand-built scenes of tests/scene_filter_scenes.py, and of BundleFilter on the library against the reference's call sequence over
HipObservationManager on the library's own mpsfm_filter_tracks.

Bounds (derived, not measured).  kp_deleted, point_fate, point_risky and every count: exact.  That is a legitimate demand because the
scene builders assert margins on the restatement's own values (scene_filter_scenes.check_margins): every depth and every squared
error is exactly on its bound by construction (identity rotations, power-of-two coordinates: no operation rounds) or 1e-9 away from
it, every compared angle a keeps |a - thr| >= 1e3 eps / min(a, thr) or is exactly 0.
kp_sq_err: exact.  The kernel is compiled with contraction off and evaluates, per element, the same sequence of IEEE-754 additions,
multiplications and divisions as the restatement, each correctly rounded on both sides; there is nothing left to differ.
point_max_angle: 6 * 2^-51.  The argument of acos is the result of such a sequence too, so it is the same number on both sides;
the two acos implementations are within 4 ulp (the device library's documented bound) and 1 ulp (the host's) of the true value, which
is at most pi, where an ulp is 2^-51; pi - a adds at most half an ulp on each side; the maximum of values that close is that close."""

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

pytestmark = pytest.mark.gpu

ANGLE_BOUND = 6 * 2.0**-51
COUNTS = ("num_negative", "num_changed_a", "num_changed_b", "n_points_deleted", "n_observations_deleted")
worst = {"angle": 0.0}


def compare(args, min_deg, risky_deg=1.5, point_sel=None, negative_depth=True):
    """One call on the device against the restatement; returns both answers."""
    want = S.run_restatement(args, min_deg, point_sel=point_sel, negative_depth=negative_depth, risky_deg=risky_deg)
    got = capi.filter_scene(max_reproj_error=S.MAX_ERR, min_tri_angle_deg=min_deg, risky_min_tri_angle_deg=risky_deg, point_sel=point_sel,
                            negative_depth=negative_depth, **args)
    dev = float(np.max(np.abs(got["point_max_angle"] - want["point_max_angle"]), initial=0.0))
    worst["angle"] = max(worst["angle"], dev)
    fin = np.isfinite(want["kp_sq_err"])
    err_dev = float(np.max(np.abs(got["kp_sq_err"][fin] - want["kp_sq_err"][fin]), initial=0.0))
    print(f"max angle deviation {dev:.3e} (so far {worst['angle']:.3e}, bound {ANGLE_BOUND:.3e}), max sq_err deviation {err_dev:.3e}; "
          f"fates {np.bincount(want['point_fate'], minlength=7).tolist()}, risky {int(want['point_risky'].sum())}")
    for k in ("kp_deleted", "point_fate", "point_risky"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert {k: got["info"][k] for k in COUNTS} == {k: want["info"][k] for k in COUNTS}
    assert got["info"]["num_syncs"] == 1
    np.testing.assert_array_equal(np.isfinite(got["kp_sq_err"]), fin)
    np.testing.assert_array_equal(got["kp_sq_err"][fin], want["kp_sq_err"][fin])
    assert dev <= ANGLE_BOUND
    np.testing.assert_array_equal(got["point_max_angle"] == 0.0, want["point_max_angle"] == 0.0)
    return got, want


def length_points(L):
    """Tracks of length L in the images 0 .. L - 1: bad elements at the positions 0, 63, 64 and last, the whole-point boundary,
    flagged elements in the first and in later chunks, and a point index without elements."""
    ims = list(range(L))
    pos = sorted({0, 63, 64, L - 1} & set(ims))
    later = [p for p in (0, 70, 130) if p < L]
    tracks = [S.track(ims)] + [S.track(ims, bad=(p,)) for p in pos] + [S.track(ims, bad=pos)]
    if L >= 3:
        tracks += [S.track(ims, bad=range(1, L - 1)), S.track(ims, bad=range(1, L)), S.track(ims, bad=range(L)),
                   S.track(ims, bad=range(1, L - 1), flagged=range(L)), S.track(ims, bad=range(1, L), flagged=range(L))]
    tracks += [S.track(ims, flagged=range(L)), S.track(ims, flagged=(0,)), S.track(ims, flagged=later), S.track(ims, bad=(0,), flagged=range(L)),
               S.track(ims, bad=(L - 1,), flagged=later), []]
    return [(S.POINT, t) for t in tracks], later


@pytest.mark.parametrize("L", S.LENGTHS)
def test_tracks_of_every_length_against_the_restatement(L):
    points, later = length_points(L)
    cams = S.line_cams(L + 1)  # the last image has no keypoints
    fates = np.zeros(7, np.int64)
    for bundle in ((0,), tuple(later), tuple(sorted(set(later) | {L - 1}))):
        args, _ = S.build(cams, points, bundle=bundle, empty_images=(L,))
        assert args["kp_start"][-1] == args["kp_start"][-2] and len(args["kp_point"]) <= 4000
        _, want = compare(args, 0.001)
        fates += np.bincount(want["point_fate"], minlength=7)
        assert want["point_risky"].sum() > 0
    sel = (np.arange(len(points)) % 2).astype(np.uint8)
    _, want = compare(args, 1.5, risky_deg=0.001, point_sel=sel, negative_depth=False)
    fates += np.bincount(want["point_fate"], minlength=7)
    # the same tracks with the point behind the cameras 0, 63, 64 and the last: removed in step 0, or as bad elements without it
    behind = sorted({0, 63, 64, L - 1} & set(range(L)))
    args, _ = S.build(S.line_cams(L + 1, behind=behind), points, bundle=tuple(later), empty_images=(L,))
    for negative_depth in (True, False):
        got, want = compare(args, 0.001, negative_depth=negative_depth)
        fates += np.bincount(want["point_fate"], minlength=7)
        assert (want["info"]["num_negative"] > 0) == negative_depth
    print("fates over the calls:", fates.tolist())
    if L >= 63:  # long tracks keep a wide pair: none dies by its angle
        assert np.all(fates[[0, 1, 3, 5]] > 0)
    if L in (2, 3):  # seen under 0.11 / 0.22 degrees
        assert fates[4] > 0 and fates[6] > 0


def test_step0_at_the_edge_of_a_chunk():
    # 65 elements of which 63 / 64 are not in front: two stay (63 observations removed) / one stays (the point dies, 64 calls counted)
    cams = S.line_cams(130, behind=list(range(2, 65)) + list(range(66, 130)))
    args, kp_of = S.build(cams, [(S.POINT, S.track(range(65))), (S.POINT, S.track(range(65, 130)))])
    got, want = compare(args, 0.001)
    np.testing.assert_array_equal(want["point_fate"], [1, 2])
    assert want["info"]["num_negative"] == 63 + 64 and want["info"]["n_observations_deleted"] == 63
    assert got["kp_deleted"][kp_of[(0, 64, 0)]] == 1 and got["kp_deleted"][kp_of[(0, 1, 0)]] == 0


@pytest.mark.parametrize("L, i, j", [(200, 0, 199), (65, 63, 64), (66, 64, 65), (129, 0, 128)])
def test_the_pair_that_carries_the_largest_angle(L, i, j):
    # every camera at the origin but two, 2^-3 to either side: that pair sees the point under 2 atan(2^-6) = 1.79 degrees, every other
    # pair under half of it or under 0
    cams = [(0.0, 0.0, 0.0)] * L
    cams[i], cams[j] = (-(2.0**-3), 0.0, 0.0), (2.0**-3, 0.0, 0.0)
    args, _ = S.build(cams, [(S.POINT, S.track(range(L))), (S.POINT, S.track([k for k in range(L) if k != j])), (S.POINT, S.track([k for k in range(L) if k not in (i, j)]))])
    got, want = compare(args, 1.5)
    np.testing.assert_array_equal(want["point_fate"], [0, 6, 6])
    assert want["point_max_angle"][0] == pytest.approx(2 * np.arctan(2.0**-6), abs=1e-14) and want["point_max_angle"][2] == 0.0
    compare(args, 0.001)


def test_two_runs_are_bitwise_equal():
    points, later = length_points(129)
    args, _ = S.build(S.line_cams(130, behind=(5, 64)), points, bundle=tuple(later), empty_images=(129,))
    kw = dict(max_reproj_error=S.MAX_ERR, min_tri_angle_deg=0.001, **args)
    first, second = capi.filter_scene(**kw), capi.filter_scene(**kw)
    for k in ("kp_deleted", "point_fate", "point_risky", "point_max_angle", "kp_sq_err"):
        assert first[k].tobytes() == second[k].tobytes(), k
    assert {k: first["info"][k] for k in COUNTS} == {k: second["info"][k] for k in COUNTS}
    # the values are optional outputs
    bare = capi.filter_scene(return_values=False, **kw)
    assert bare["kp_sq_err"] is None and bare["point_max_angle"] is None
    np.testing.assert_array_equal(bare["point_fate"], first["point_fate"])
    np.testing.assert_array_equal(bare["kp_deleted"], first["kp_deleted"])


def test_refused_inputs_on_a_machine_with_a_device():
    for change in (dict(max_reproj_error=np.nan), dict(min_tri_angle_deg=-1.0), dict(risky_min_tri_angle_deg=np.inf)):
        with pytest.raises(capi.MpsfmHipError) as e:
            capi.filter_scene(**dict(S.valid_call(), **change))
        assert e.value.code == -1
    v = S.valid_call()
    v["registered"] = v["registered"].copy()
    v["registered"][1] = 0
    with pytest.raises(capi.MpsfmHipError) as e:
        capi.filter_scene(**v)
    assert e.value.code == -1
    with pytest.raises(capi.MpsfmHipError):
        capi.filter_scene(device=99, **S.valid_call())
    out = capi.filter_scene(**S.valid_call())  # and the valid call is answered
    assert out["info"]["num_syncs"] == 1 and out["info"]["ms"] >= out["info"]["ms_tracks"] > 0


def test_bundle_filter_on_the_library_equals_the_sequence_on_filter_tracks():
    a = S.make_filter_scene(20, n_cams=12)
    b = copy.deepcopy(a)
    b.obs = HipObservationManager(b, ObservationManager(b))  # the library's mpsfm_filter_tracks, one launch per filter
    bf, replay = BundleFilter({}, a, SceneQueries(a, S.empty_graph(a))), MapperReplay(b, None)
    # a scene with rotated cameras against the restatement first: the same call, the same arrays
    st, _ = bf._state()
    in_bundle, flags = bf._invalid_depth_flags({1, 2, 3}, st)
    kw = dict(kp_start=bf.sq.kp_start, kp_xy=bf.sq.kp_xy, intr=bf.sq.intr, registered=st["registered"], cam_quat_xyzw=st["cam_quat_xyzw"], cam_t=st["cam_t"],
              kp_point=st["kp_point"], xyz=st["xyz"], max_reproj_error=4.0, min_tri_angle_deg=0.001, in_bundle=in_bundle, kp_invalid_depth=flags)
    got, want = capi.filter_scene(**kw), N.filter_scene(**kw)
    fin = np.isfinite(want["kp_sq_err"])
    print("rotated cameras: max sq_err deviation", float(np.max(np.abs(got["kp_sq_err"][fin] - want["kp_sq_err"][fin]))), "max angle deviation",
          float(np.max(np.abs(got["point_max_angle"] - want["point_max_angle"]))), "fates", np.bincount(want["point_fate"], minlength=7).tolist())
    for k in ("kp_deleted", "point_fate", "point_risky"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    np.testing.assert_array_equal(got["kp_sq_err"][fin], want["kp_sq_err"][fin])
    assert np.max(np.abs(got["point_max_angle"] - want["point_max_angle"])) <= ANGLE_BOUND
    # then the drop-in against the reference's sequence
    bundle = S.fixed_bundle(a)
    got, want = bf.filter_bundle(bundle), replay.filter_bundle(copy.deepcopy(bundle))
    fates = np.bincount(bf.last_result["point_fate"], minlength=7)
    print("fates 0 .. 6:", fates.tolist(), "returned:", got, bf.last_info)
    assert np.all(fates > 0) and bf.last_info["num_syncs"] == 1
    assert got == want and got[0] > 50
    S.assert_same_scene(a, b)
    S.assert_same_errors(a, b)
    got, want = bf.filter_all(), replay.filter_all()
    assert got == want
    S.assert_same_scene(a, b)
