"""tests/numpy_lm_step.py, the reference of the update sweep's one-step test, checked without a device: its residual blocks against the
oracle's single-block evaluators, its losses against tests/golden/loss_table.npz, its float64 run against oracle.reduced_system, the
yardsticks of tests/lm_step_cases.py against what the float64 run measures here, and the coverage of the loss-pair scene
(tests/loss_pair_scenes.py), so that tests/test_gpu_update_once.py cannot pass on a narrow band of robust weights."""

import os

import numpy as np
import pytest

import lm_step_cases as LC
import loss_pair_scenes as LP
import numpy_lm_step as NS
from conftest import GOLDEN
from oracle import cpu_oracle as O

LD = np.longdouble


def test_losses_match_the_golden_table():
    z = np.load(os.path.join(GOLDEN, "loss_table.npz"))
    a, s = z["a"][:, None], z["s"][None, :]
    for name, kind in (("soft_l1", NS.SOFT_L1), ("cauchy", NS.CAUCHY)):
        for dtype, rel in ((LD, 1e-12), (np.float64, 1e-12)):
            rho, rho1 = NS.loss(kind, a, s, dtype)
            # rel 1e-12, and the floor of the table's own values: its soft-L1 rho 2 a^2 (sqrt(1 + s / a^2) - 1) is a difference of numbers
            # near a^2 and carries their rounding, 4e-16 a^2 (tests/test_oracle_golden.py), which the form used here does not
            assert (np.abs(rho.astype(np.float64) - z[f"{name}_rho0"]) <= 1e-12 * np.abs(z[f"{name}_rho0"]) + 4e-16 * a * a).all()
            np.testing.assert_allclose(rho1.astype(np.float64), z[f"{name}_rho1"], rtol=rel, atol=0)
    rho, rho1 = NS.loss(NS.TRIVIAL, 2.0, np.array([3.5]))
    assert rho[0] == 3.5 and rho1[0] == 1.0
    assert NS.loss(NS.CAUCHY, 1e-3, np.array([1e302]))[1][0] == NS.DBL_MIN  # the clamp of rho'


@pytest.mark.parametrize("shift", [False, True])
def test_blocks_match_the_oracle(shift):
    """Raw residuals and Jacobians (unit scales, trivial losses with magnitude 1: weight 1) of every 7th block of the loss-pair scene."""
    prob = LP.problem("trivial", "trivial", shift_logscale=shift)
    prob.reproj_loss_magnitude = 1.0
    prob.dobs_magnitude[:] = 1.0
    L = NS.Layout(prob)
    lin = NS.linearize(prob, L, prob.cam_quat, prob.cam_t, prob.pts, np.ones((prob.n_cams, 6)), np.ones((prob.n_pts, 3)), LD)
    worst = 0.0
    for b in range(0, L.n_blocks, 7):
        c, p, src = int(L.cam[b]), int(L.pt[b]), int(L.src[b])
        q, t, X = prob.cam_quat[c], prob.cam_t[c], prob.pts[p]
        if L.kind[b] == 0:
            r, Jc, Jp = O.reproj_block(q, t, prob.cam_intr[prob.cam_intr_idx[c]], X, prob.obs_xy[src])
            rows, terms = 2, np.abs(prob.obs_xy[src]).max()
        else:
            sl = prob.shift_logscale[c] if shift else (0.0, 0.0)
            ok, r, Jc, Jp = O.depth_block(q, t, X, prob.dobs_depth[src], sl[0], sl[1])
            assert ok == 1
            rows, terms = 1, 1.0 + abs(np.log(prob.dobs_depth[src]))
        # (a residual is a difference: its rounding is that of its terms, the projection and the measurement)
        for got, want, floor in ((lin["r"][b, :rows], r, terms), (lin["Jc"][b, :rows], Jc, 0.0), (lin["Jp"][b, :rows], Jp, 0.0)):
            scale = max(np.abs(want).max(), floor) + 1e-300
            worst = max(worst, float(np.abs(got.astype(np.float64) - want).max() / scale))
        assert not lin["r"][b, rows:].any() and not lin["Jc"][b, rows:].any()
    print(f"blocks vs oracle: worst difference {worst:.3e} of the block's largest entry")
    assert worst <= 1e-14  # the oracle rounds in double: some 20 operations per entry


@pytest.mark.parametrize("name", LC.NAMES)
def test_float64_run_agrees_with_the_oracle(name):
    """oracle.reduced_system's landmark step and model cost change for its own camera step, by the measures and bounds of the GPU test."""
    for radius in LC.RADII:
        ref = LC.oracle_systems(name)[radius]
        S = LC.reference(name, radius, "solve")
        assert S.bad_lin == 0 and not S.failed.any()
        np.testing.assert_array_equal(ref["pt_scale"] != 0, S.L.pvar[:, None] & np.ones(3, bool))
        np.testing.assert_array_equal((ref["cam_scale"] != 0).any(1), S.L.cam_var)
        S64 = NS.LMStep(LC.problem(name), ref["cam_scale"], ref["pt_scale"], ref["yc"], radius, dtype=np.float64)
        eta_o, eta_f = float(S.eta_p(ref["yp"]).max()), float(S.eta_p(S64.yp).max())
        mcc_o, mcc_f = float(S.mcc_measure(ref["model_cost_change"])), float(S.mcc_measure(S64.mcc))
        print(f"{name} radius {radius:g}: eta_p oracle {eta_o:.2e} float64 {eta_f:.2e}; mcc measure oracle {mcc_o:.2e} float64 {mcc_f:.2e}")
        assert eta_o <= LC.ETA_BOUND and eta_f <= LC.ETA_F64
        assert mcc_o <= LC.MCC_BOUND and mcc_f <= LC.MCC_F64
        assert float(S.mcc) > 0
        # the oracle's candidate landmarks are the restatement's to a forward error the conditioning explains (not a bound of the GPU test)
        np.testing.assert_allclose(ref["yp"], S.yp.astype(np.float64), rtol=0, atol=1e-9 * np.abs(ref["yp"]).max())


def test_yardsticks_are_what_the_float64_run_measures():
    """ETA_F64 and MCC_F64 over every scene, radius and camera step: not exceeded, and not more than 1.5 times the measurement."""
    eta = mcc = 0.0
    for name in LC.NAMES:
        prob = LC.problem(name)
        for radius in LC.RADII:
            ref = LC.oracle_systems(name)[radius]
            for step, f in LC.STEPS.items():
                S = LC.reference(name, radius, step)
                S64 = NS.LMStep(prob, ref["cam_scale"], ref["pt_scale"], ref["yc"] * f, radius, dtype=np.float64)
                eta, mcc = max(eta, float(S.eta_p(S64.yp).max())), max(mcc, float(S.mcc_measure(S64.mcc)))
    print(f"float64 yardsticks: eta_p {eta:.3e} (recorded {LC.ETA_F64:.1e}), mcc measure {mcc:.3e} (recorded {LC.MCC_F64:.1e})")
    assert eta <= LC.ETA_F64 <= 1.5 * eta
    assert mcc <= LC.MCC_F64 <= 1.5 * mcc


def test_loss_pair_scene_covers_the_regimes():
    prob = LP.problem()
    assert prob.n_cams == 5 and prob.n_pts == 300 and prob.n_dobs == prob.n_obs
    tracks = np.bincount(prob.obs_pt)
    assert tracks.min() == 2 and tracks.max() == 4
    assert 1e-3 <= prob.dobs_param.min() < 2e-3 and 5.0 < prob.dobs_param.max() <= 10.0
    assert 1e-2 <= prob.dobs_magnitude.min() < 2e-2 and 5e3 < prob.dobs_magnitude.max() <= 1e4
    both_sides_in_one_call, near, far = False, 0, 0
    for name in LC.LP_NAMES:
        for radius in LC.RADII:
            S = LC.reference(name, radius, "solve")
            z = (S.lin["s"] / S.lin["lscale"] ** 2).astype(np.float64)
            rep = S.L.kind == 0
            # s / a^2 of both residual kinds spans [1e-4, 1e4] at the linearisation point, whatever the pair
            assert z[rep].min() <= 1e-4 and z[rep].max() >= 1e4, (name, z[rep].min(), z[rep].max())
            assert z[~rep].min() <= 1e-4 and z[~rep].max() >= 1e4, (name, z[~rep].min(), z[~rep].max())
            # the robust weight is far from 1 on a share of the blocks and the clamp of rho' is not what bounds it
            if S.prob.depth_loss_type != NS.TRIVIAL:
                assert (S.lin["rho1"][~rep] < 1e-2).sum() >= 20 and (S.lin["rho1"][~rep] > 0.99).sum() >= 20
            big = LC.reference(name, radius, "large")
            d2 = ((big.cs * big.ycam)[:, :3].astype(np.float64) ** 2).sum(1)[big.L.cam_var]
            near, far = near + int((d2 <= LP.ZMAX).sum()), far + int((d2 > LP.ZMAX).sum())
            both_sides_in_one_call |= bool((d2 <= LP.ZMAX).any() and (d2 > LP.ZMAX).any())
            assert big.bad_lin == 0
    print(f"large-step candidate cameras: {near} on quat_plus' polynomials, {far} beyond")
    assert both_sides_in_one_call and near >= 10 and far >= 10


def test_bad_record_case_has_a_known_count():
    """The large step of the default pair at radius 1e3 puts exactly three landmarks behind a camera (depth blocks with Z <= 0) that
    every block can be evaluated for at the linearisation point; the plain step of the same call leaves none."""
    S = LC.reference("lp:softl1:cauchy", 1e3, "large")
    assert S.bad_lin == 0
    blk = dict(cam=S.L.cam, pt=S.L.pt, kind=S.L.kind, src=S.L.src)
    rows = NS.residual_rows(S.prob, blk, S.q2, S.t2, S.pts2)
    behind = (rows["Z"] <= 0).astype(bool)
    assert S.cost_at(S.q2, S.t2, S.pts2)[1] == 3 and int((behind & (S.L.kind == 1)).sum()) == 3
    assert (rows["Z"][S.L.kind == 1] > 0).sum() == S.prob.n_dobs - 3
    plain = LC.reference("lp:softl1:cauchy", 1e3, "solve")
    assert plain.cost_at(plain.q2, plain.t2, plain.pts2)[1] == 0
