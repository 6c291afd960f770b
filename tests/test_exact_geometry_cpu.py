"""The exact reference of tests/exact_geometry.py, validated on the CPU before a GPU sees it: against the C oracle on
the friendly scenes, against hand-made exact cases, and on the case sets of tests/test_gpu_exact_geometry.py (every
forward-checked case is informative; the unaltered oracle and the NumPy evaluation pass every criterion)."""

import math

import mpmath as mp
import numpy as np
import pytest

import exact_geometry as G
from mpsfm_amd.problem import Tracks
from mpsfm_amd.sfm.scene.observations import reprojection_decisions
from mpsfm_amd.synthetic import make_scene
from oracle import cpu_oracle as O


@pytest.fixture(scope="module")
def friendly():
    prob, truth = make_scene(15, 300, False, seed=9, outlier_frac=0.0)
    order = np.argsort(prob.obs_pt, kind="stable")
    start = np.searchsorted(prob.obs_pt[order], np.arange(prob.n_pts + 1))
    tr = Tracks(truth["cam_quat"], truth["cam_t"], prob.cam_intr, prob.cam_intr_idx, start, prob.obs_cam[order], prob.obs_xy[order])
    return prob, tr


def test_reference_triangulation_agrees_with_oracle_on_friendly_scene(friendly):
    _, tr = friendly
    ref = G.triangulation_reference(tr)
    xyz = O.triangulate_tracks(tr)
    assert all(G.triangulation_informative(r, G.C_T) for r in ref)
    for k, (back, fwd) in enumerate(G.triangulation_ratios(ref, xyz)):
        assert back <= G.C_T and fwd <= G.C_T, (k, back, fwd)


def test_reference_filters_agree_with_oracle_on_friendly_scene(friendly):
    _, tr = friendly
    xyz = O.triangulate_tracks(tr)
    ref = G.filter_reference(tr, xyz)
    ang, err, front = O.filter_tracks(tr, xyz)
    for k, r in enumerate(ref):
        e0, e1 = int(tr.track_start[k]), int(tr.track_start[k + 1])
        assert G.angle_ratio(r, ang[k]) <= G.C_A, k
        assert max(G.sq_err_ratios(r, err[e0:e1])) <= G.C_E, k
        assert [bool(f) for f in r["front"]] == front[e0:e1].tolist(), k


def test_reference_point_hessians_agree_with_oracle_on_friendly_scene(friendly):
    prob, _ = friendly
    prob = prob.copy()
    prob.reproj_loss_magnitude = 0.25
    ref = G.point_hessians(prob)
    assert all(r["inv"] is not None for r in ref)
    assert max(G.cov_ratios(ref, O.point_covs(prob))) <= G.C_P


def test_reference_angle_on_hand_made_cases():
    with mp.workdps(G.DPS):
        tiny = mp.mpf(10) ** -50
        zero = [mp.mpf(0)] * 3
        a, _ = G.angle_pair([mp.mpf(3), 0, 0], [0, mp.mpf(4), 0], zero)  # 3-4-5: the rays are the two legs
        assert abs(a - mp.pi / 2) < tiny
        a, _ = G.angle_pair([mp.mpf(1), 2, 3], [mp.mpf(1), 2, 3], [mp.mpf(7), -1, 2])  # coincident centres
        assert a == 0
        a, _ = G.angle_pair([mp.mpf(2), 0, 0], [-mp.mpf(3) / 2, 3 * mp.sqrt(3) / 2, 0], zero)  # 120 degrees folds to 60
        assert abs(a - mp.pi / 3) < tiny
        a, k = G.angle_pair(zero, [mp.mpf(1), 0, 0], zero)  # the point at a centre: a ray of zero length
        assert a == 0 and k == 1
        a, _ = G.angle_pair([mp.mpf(0), 0, -10], [mp.mpf(0), 0, 13], zero)  # 180 degrees folds to 0
        assert a == 0


def test_reference_front_is_the_plain_comparison_with_two_to_the_minus_52():
    tr, xyz = G.filter_cases(0.0)
    ref = G.filter_case_reference(0.0)
    seen = {}
    for lab, X, r in zip(tr.labels, xyz, ref):
        if lab.startswith("front_z="):
            assert r["zc"][0] == mp.mpf(float(X[2]))  # identity rotation, t = 0: zc is X[2] exactly
            seen[float(X[2])] = bool(r["front"][0])
    e = 2.0 ** -52
    assert seen == {e: True, math.nextafter(e, 0.0): False, math.nextafter(e, 1.0): True, 0.0: False, -1.0: False, 1e-300: False, 1e300: True}


def test_every_forward_checked_case_is_informative():
    """A condition on the inputs, computed from the reference alone: the friendly, block-edge, large-rotation,
    two-intrinsics and 1e-2 low-parallax tracks carry a forward bound worth asserting."""
    b, groups = G.triangulation_cases()
    ref = G.triangulation_case_reference()
    for name in G.TRI_FORWARD_GROUPS:
        for k in groups[name]:
            assert G.triangulation_informative(ref[k], G.C_T), (name, b.labels[k])
    assert len(groups["friendly"]) >= G.BLOCK_EDGES[-1] and groups["friendly"][: G.BLOCK_EDGES[-1]] == list(range(G.BLOCK_EDGES[-1]))
    tr = b.tracks()
    assert {int(i) for i in tr.cam_intr_idx[tr.el_cam[: tr.track_start[G.BLOCK_EDGES[-1]]]]} == {0, 1}  # both rows in use


@pytest.mark.parametrize("name", ["oracle", "numpy"])
def test_cases_pass_through_cpu_implementations(name):
    """No case of the GPU tests flags the unaltered C oracle (the kernels' arithmetic without FMA contraction) or the
    NumPy evaluation the constants were measured with."""
    impl = {"oracle": (O.triangulate_tracks, O.filter_tracks, O.point_covs),
            "numpy": (G.numpy_triangulate, G.numpy_filter, G.numpy_point_covs)}[name]
    stats = []
    assert {k: v for k, v in G.all_failures(*impl, stats=stats).items() if v} == {}
    assert {kind for _, kind, _ in stats} == {"backward", "forward", "angle", "sq_err", "cov"}


def test_criteria_flag_a_wrong_answer():
    """The comparison functions can fail: an implementation that is off by a few 1e-9, or answers a short track."""
    assert G.triangulation_failures(lambda tr: np.nan_to_num(O.triangulate_tracks(tr)) + 3e-9)
    assert G.filter_failures(lambda tr, x: tuple(a + (1e-9 if a.dtype == np.float64 else 0) for a in O.filter_tracks(tr, x)))
    assert G.filter_failures(lambda tr, x: (lambda a, e, f: (a, e, ~f))(*O.filter_tracks(tr, x)))
    assert G.cov_failures(lambda p: O.point_covs(p) * (1 + 1e-9), G.friendly_cov_problem, 4.0)
    assert G.cov_failures(lambda p: np.nan_to_num(O.point_covs(p)), G.hard_cov_problem)


def test_short_tracks_and_landmarks_contract_of_the_oracle():
    b, groups = G.triangulation_cases()
    xyz = O.triangulate_tracks(b.tracks())
    assert np.isnan(xyz[groups["short"]]).all() and np.isfinite(xyz[groups["friendly"]]).all()
    prob, labels = G.hard_cov_problem()
    covs = O.point_covs(prob)
    for lab, c in zip(labels, covs):
        assert np.isnan(c).all() == (lab in ("no_obs", "one_obs")), lab


def test_an_element_behind_its_camera_is_bad_whatever_its_error():
    """el_sq_err is the plain formula for zc < eps (small for a mirrored point, inf or NaN for zc == 0): the decision is
    safe only because reprojection_decisions ORs in ~front."""
    tr, xyz = G.filter_cases(0.0)
    _, err, front = O.filter_tracks(tr, xyz)
    _, bad = reprojection_decisions(tr.track_start, err, front, 4.0)
    assert (~front).sum() >= 8 and bad[~front].all()
    behind = err[~front]
    assert np.isnan(behind).any() and np.isinf(behind).any() and (behind < 1e-12).any()
