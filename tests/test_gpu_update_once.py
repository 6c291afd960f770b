"""ONE update sweep (mpsfm_debug_update_once: k_update_sweep<true / false>, k_long_update_sweep, k_cam_update or the fused camera
update, behind the solver's own track sweep) against tests/numpy_lm_step.py in long double, on the scenes, radii and camera steps of
tests/lm_step_cases.py.  Every form the handle can take is called with the same camera step; a form it cannot take must be refused.

What is asserted, per call (u = 2^-53):
  landmark step    yp = (pts2 - pts) / ps of EVERY variable landmark: the componentwise backward error eta_p in the reference's system
                   (LMStep.eta_p) is at most ETA_BOUND = 8 x the float64 yardstick.  pts2 = fl(X + ps yp) is a rounded number: u |X2| / ps
                   of yp is representation, not arithmetic, and is taken out of the numerator (|V + D| times it) before the comparison.
                   Constant landmarks: pts2 == pts bit for bit.
  model cost change  |mcc - ref| / sum |m| (|r| + |m| / 2) at most MCC_BOUND = 8 x the float64 yardstick
  candidate cost   against the reference's cost at the GPU's OWN q2, t2, pts2, rel 1e-12 (the suite's eval_cost tolerance; the fused
                   form must take the cost at exactly the pose workgroup 0 writes out), and against the reference at ITS candidate
                   with a tolerance formed from the reference alone (cost_tolerance): a step with eta_p <= ETA_BOUND has its candidate
                   landmarks within dX = ps |(V + D)^-1| (ETA_BOUND (|V + D| |yp| + sum |Jp|^T |r + Jc yc|) + |V + D| u |X2| / ps) + u |X2|
                   of the reference's (LMStep.candidate_tolerance; asserted entry by entry as well), its cameras within 1e-15 plus the
                   scales' tolerance times |yc|; the cost then differs by at most |dcost/dX| dX + |dcost/dcam| dcam, doubled for what
                   first order leaves out, plus 1e-12 of the cost.  Both only where no block is invalid at the candidate
  U_BAD            zero where the reference counts no invalid block at the candidate, non-zero where it counts one
  norms            U_STEP_SQ_* and U_XN_SQ_* against the long-double sums over the GPU's own candidates.  n terms summed in any order
                   with rounded squares: (n + 8) u of the sum; the landmark step norm sums fl(ps yp)^2, not (X2 - X)^2, which differ
                   by the rounding of X2: 2 u sum |X2 - X| |X2| more
  cameras          against the formula x [+] cs .* yc with the cs the handle ran with (the hook returns them): | |q2| - |q| | <= 4e-16
                   and |q2 - formula| <= 1e-15 (the bounds of test_gpu_lean_math.py), |t2 - formula| <= 1e-15 (from |t2| = 16 on, where
                   that is less than half a spacing: the two roundings of fl(t + fl(cs y))); constant cameras and the zero step: bit
                   for bit the cameras.  (The reference's own cs, the oracle's, differ from the handle's by some 1e-15 relative: sums
                   in another order.  Against those the cameras of the large step would be off by more than 1e-15.)
  scales           the cs and ps the hook returns against the reference's inputs, the oracle's: both are float64 computations of
                   1 / (1 + sqrt(sum J^2)); LMStep.scale_tolerances bounds their difference (Jacobian entries within 64 u of their terms
                   in absolute value, the robust weight moved by the rounding of its residual, 16 u of the residual's terms, the sum,
                   root and quotient; twice, for the two sides): about 1e-12 relative, of which 2 % is used
  U_GMAX_CAMS      the maximum over |x [+] g - x| and |g_t| of g = -g_c / cs, with g_c = sum Jc^T r summed by the track sweep in its own
                   order from terms of some 30 operations each: camera c's entries are off by at most (rows_c + 64) u sum |Jc|^T |r| /
                   cs, quat_plus moves by no more than its argument (factor 2 for the three components), sweep_div and the maximum
                   add 4 ulp.  (4 ulp alone cannot hold: g_c is a sum of up to thousands of terms of both signs.)
  part2            every row's five columns finite (the hook fills the table with NaN first) and their sums the scalars, (rows + 8) u
  across forms     every output of hand-off against recompute and of fused against separate camera update: pts2 within 2 dX, mcc within
                   MCC_BOUND, cost, gradient maximum and norms within twice their bounds, the scales bit for bit; fused and separate
                   camera update: q2 and t2 bit for bit
  state            behind the last call of a scene get_state returns the cameras and landmarks the handle was created with

Float64 yardsticks (tests/lm_step_cases.py, measured on the CPU): eta_p 4.79e-13, mcc measure 3.70e-15; bounds 4.0e-12 and 3.2e-14.
Measured on the MI355X, largest over radii and camera steps, eta_p / mcc measure (per form where the forms differ; DESIGN.md §4a-4
has the whole table): two_view 4.74e-14 / 5.24e-17; pairs16 5.87e-14 / 5.55e-16 (hand-off 6.80e-16); mixed16 2.50e-14 / 3.54e-16;
one_var 5.75e-14 / 5.39e-16; g17_40 4.03e-14 / 6.31e-17; dup_aab 3.73e-14 / 1.43e-16; dup_aa 1.31e-13 / 2.27e-16; r252_253 3.93e-14 /
2.28e-16; lp trivial:trivial 2.72e-14 / 1.62e-16, trivial:softl1 2.68e-14 / 2.35e-16, trivial:cauchy 2.66e-14 / 4.39e-16,
softl1:trivial 1.05e-13 / 2.28e-16, softl1:softl1 1.08e-13 / 1.98e-16, softl1:cauchy 1.08e-13 / 1.80e-16 (with shift_logscale
1.10e-13 / 3.21e-16), cauchy:trivial 2.20e-13 / 3.80e-15, cauchy:softl1 2.32e-13 / 9.49e-16 (hand-off 8.34e-16), cauchy:cauchy
2.70e-13 / 6.07e-16 (hand-off 7.22e-16).  The fused and the separate camera update give the same figures."""

import numpy as np
import pytest

import lm_step_cases as LC
import numpy_lm_step as NS
from build_table_cases import environment
from mpsfm_amd import capi

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = LD(2.0) ** -53
FORMS = {"recompute": (False, False), "recompute+fused": (False, True), "handoff": (True, False), "handoff+fused": (True, True)}
UNSUPPORTED = -6  # MPSFM_EUNSUPPORTED


def ulp(x):
    return float(np.spacing(np.float64(abs(x))))


def cost_tolerance(S, dX, cs_tol):
    """What the cost at the candidate of a step within the bounds of this test may differ from the cost at the reference's candidate by,
    formed from the reference alone: |dcost/dX| dX over the landmarks (dX: LMStep.candidate_tolerance(ETA_BOUND)) and |dcost/dcam| times
    the cameras' bound, 1e-15 for the formula plus cs_tol |yc| for the scales it is evaluated with (a rotation step d moves q by |d|: the
    three gradients times the 2-norm, doubled for the norm of the quaternion's four entries); twice that, for what first order leaves out."""
    gp, gc = S.cost_gradient_at(S.q2, S.t2, S.pts2)
    dcam = LD(1e-15) + cs_tol * np.abs(S.ycam)
    dcam[:, 3:] += U * np.abs(S.t2)
    dq = 2 * np.sqrt((dcam[:, :3] ** 2).sum(1))
    return 2 * ((gp * dX).sum() + (gc[:, :3].sum(1) * dq).sum() + (gc[:, 3:] * dcam[:, 3:]).sum())


def check_call(tag, S, out, step):
    """One call's outputs against the reference S (built with the same camera step); returns (eta_p, mcc measure)."""
    prob, L = S.prob, S.L
    X, q, t = (np.asarray(v, LD) for v in (prob.pts, prob.cam_quat, prob.cam_t))
    X2, q2, t2 = (out[k].astype(LD) for k in ("pts2", "q2", "t2"))
    assert S.bad_lin == 0 and not S.failed.any()
    for k in ("pts2", "q2", "t2"):
        assert np.isfinite(out[k]).all(), (tag, k)
    np.testing.assert_array_equal(out["pts"], prob.pts)  # the state of the handle is not changed
    np.testing.assert_array_equal(out["q"], prob.cam_quat)
    np.testing.assert_array_equal(out["t"], prob.cam_t)

    # ---- landmark step: every variable landmark
    pv = L.pvar
    np.testing.assert_array_equal(out["pts2"][~pv], prob.pts[~pv])
    with np.errstate(all="ignore"):
        yp = np.where(pv[:, None], (X2 - X) / np.where(S.ps > 0, S.ps, 1), 0)
        slack = np.where(pv[:, None], U * np.abs(X2) / np.where(S.ps > 0, S.ps, 1), 0)
    eta = S.eta_p(yp, slack)[pv]
    assert eta.shape == (int(pv.sum()),) and np.isfinite(eta.astype(np.float64)).all()
    eta_max = float(eta.max())
    assert eta_max <= LC.ETA_BOUND, (tag, eta_max, int(np.flatnonzero(pv)[int(np.argmax(eta))]))

    # ---- model cost change
    mcc_meas = float(S.mcc_measure(out["mcc"]))
    assert mcc_meas <= LC.MCC_BOUND, (tag, mcc_meas, out["mcc"], float(S.mcc))

    # ---- the column scales the sweeps ran with against the reference's (the oracle's), both float64 computations: LMStep.scale_tolerances
    cs_g, ps_g = out["cs"].astype(LD), out["ps"].astype(LD)
    np.testing.assert_array_equal(out["cs"] != 0, S.cs != 0)
    np.testing.assert_array_equal(out["ps"] != 0, S.ps != 0)
    cs_tol, ps_tol = S.scale_tolerances()
    assert (np.abs(cs_g - S.cs) <= cs_tol).all() and (np.abs(ps_g - S.ps) <= ps_tol).all(), (tag, float(np.abs(cs_g - S.cs).max()), float(np.abs(ps_g - S.ps).max()))

    # ---- candidate cameras: the formula x [+] cs .* yc with the handle's own cs
    cv = L.cam_var
    np.testing.assert_array_equal(out["q2"][~cv], prob.cam_quat[~cv])
    np.testing.assert_array_equal(out["t2"][~cv], prob.cam_t[~cv])
    if step == "zero":
        np.testing.assert_array_equal(out["q2"], prob.cam_quat)
        np.testing.assert_array_equal(out["t2"], prob.cam_t)
    d = cs_g * S.ycam
    q_f, t_f = np.where(cv[:, None], NS.quat_plus(q, d[:, :3]), q), t + d[:, 3:]
    unit = np.abs(np.sqrt((q2 * q2).sum(1)) - np.sqrt((q * q).sum(1))).astype(np.float64)
    dq = np.abs(q2 - q_f).max(1).astype(np.float64)
    assert unit.max() <= 4e-16 and dq.max() <= 1e-15, (tag, unit.max(), dq.max())
    # (1e-15 is less than half a spacing of doubles from 16 on: there the bound is the two roundings of fl(t + fl(cs y)))
    tol_t = np.maximum(LD(1e-15), np.spacing(np.abs(t_f).astype(np.float64)).astype(LD) / 2 + U * np.abs(d[:, 3:]))
    assert (np.abs(t2 - t_f) <= tol_t).all(), (tag, float(np.abs(t2 - t_f).max()))

    # ---- candidate cost and bad count
    dX_tol = S.candidate_tolerance(LC.ETA_BOUND)
    tol_cost = cost_tolerance(S, dX_tol, cs_tol)
    assert (np.abs(X2 - S.pts2) <= dX_tol).all(), (tag, float((np.abs(X2 - S.pts2) - dX_tol).max()))  # (what eta_p <= ETA_BOUND implies)
    cost_own, bad_own = S.cost_at(q2, t2, X2)
    cost_ref, bad_ref = S.cost_at(S.q2, S.t2, S.pts2)
    assert (bad_own == 0) == (bad_ref == 0), (tag, bad_own, bad_ref)
    assert (out["bad"] == 0.0) == (bad_ref == 0), (tag, out["bad"], bad_ref)
    if bad_ref == 0:
        assert abs(LD(out["cand_cost"]) - cost_own) <= LD(1e-12) * cost_own, (tag, out["cand_cost"], float(cost_own))
        assert abs(LD(out["cand_cost"]) - cost_ref) <= tol_cost + LD(1e-12) * cost_ref, (tag, out["cand_cost"], float(cost_ref), float(tol_cost))

    # ---- step and state norms from the GPU's own candidates
    sp, xp, sc, xc = S.norms(q2, t2, X2)
    npv, ncv = 3 * int(pv.sum()), 7 * int(cv.sum())
    dX = np.abs(X2 - X)[pv]
    tol_sp = 2 * U * ((dX + U * np.abs(X2[pv])) * np.abs(X2[pv])).sum() + (U * np.abs(X2[pv])).sum() ** 2 + (npv + 8) * U * sp
    assert abs(LD(out["step_sq_pts"]) - sp) <= tol_sp, (tag, out["step_sq_pts"], float(sp), float(tol_sp))
    assert abs(LD(out["xn_sq_pts"]) - xp) <= (npv + 8) * U * xp, (tag, out["xn_sq_pts"], float(xp))
    assert abs(LD(out["step_sq_cams"]) - sc) <= (ncv + 8) * U * sc, (tag, out["step_sq_cams"], float(sc))
    assert abs(LD(out["xn_sq_cams"]) - xc) <= (ncv + 8) * U * xc, (tag, out["xn_sq_cams"], float(xc))
    if step == "zero":
        assert out["step_sq_cams"] == 0.0

    # ---- camera gradient maximum
    e_cam = 2 * (S.cam_rows + 64) * U * S.gu_abs.max(1)
    tol_g = float(e_cam[cv].max()) + 4 * ulp(float(S.gmax)) if cv.any() else 0.0
    assert abs(LD(out["gmax_cams"]) - S.gmax) <= tol_g, (tag, out["gmax_cams"], float(S.gmax), tol_g)

    # ---- per-chunk rows
    rows = out["part2"]
    assert np.isfinite(rows).all(), (tag, np.argwhere(~np.isfinite(rows))[:4])
    for col, key in enumerate(capi.BAHandle.UPDATE_SCALARS[:5]):
        tot, mag = rows[:, col].astype(LD).sum(), np.abs(rows[:, col]).astype(LD).sum()
        assert abs(LD(out[key]) - tot) <= (rows.shape[0] + 8) * U * mag, (tag, key, out[key], float(tot))
    return eta_max, mcc_meas, dict(dX=dX_tol, cost=tol_cost + LD(1e-12) * cost_ref, gmax=tol_g)


def check_pair(tag, S, a, b, same_cams, tols):
    """Two forms of the same call against each other, every output: each is within `tols` of the reference, so within twice that of
    the other (the norms: each form's own candidates, so the same sums to the candidates' difference)."""
    assert abs(LD(a["mcc"]) - LD(b["mcc"])) <= LC.MCC_BOUND * S.mcc_scale, (tag, a["mcc"], b["mcc"])
    assert (a["bad"] == 0.0) == (b["bad"] == 0.0)
    if a["bad"] == 0.0:
        assert abs(LD(a["cand_cost"]) - LD(b["cand_cost"])) <= 2 * tols["cost"], (tag, a["cand_cost"], b["cand_cost"], float(tols["cost"]))
    pa, pb = a["pts2"].astype(LD), b["pts2"].astype(LD)
    assert (np.abs(pa - pb) <= 2 * tols["dX"]).all(), (tag, float(np.abs(pa - pb).max()))
    np.testing.assert_array_equal(a["cs"], b["cs"])  # the same prepare_scales
    np.testing.assert_array_equal(a["ps"], b["ps"])
    assert abs(a["gmax_cams"] - b["gmax_cams"]) <= 2 * tols["gmax"]
    # |sum da^2 - sum db^2| <= sum |da - db| (|da| + |db|), the sums' own rounding as in check_call
    n, da = 3 * int(S.L.pvar.sum()), np.abs(pa - np.asarray(S.prob.pts, LD))
    for key, base, extra in (("step_sq_pts", da, 4 * U * ((da + U * np.abs(pa)) * np.abs(pa)).sum()), ("xn_sq_pts", np.abs(pa), 0)):
        tol = ((base + 2 * tols["dX"]) * 4 * tols["dX"]).sum() + 2 * (n + 8) * U * LD(max(a[key], b[key])) + extra
        assert abs(LD(a[key]) - LD(b[key])) <= tol, (tag, key, a[key], b[key], float(tol))
    for key in ("step_sq_cams", "xn_sq_cams"):
        assert abs(a[key] - b[key]) <= 2 * (7 * int(S.L.cam_var.sum()) + 8) * float(U) * max(a[key], b[key]) + (0 if same_cams else 1e-300), (tag, key, a[key], b[key])
    if same_cams:  # fused and separate camera update: the same arithmetic (camera_candidate)
        np.testing.assert_array_equal(a["q2"], b["q2"])
        np.testing.assert_array_equal(a["t2"], b["t2"])


def run_scene(name):
    """Every call of the scene: (chunk counts, [(radius, step, yc, {form: outputs})]).  The camera step is the handle's own dense
    solution at the radius, times the factors of lm_step_cases.STEPS."""
    calls = []
    with environment(LC.environment_of(name)), capi.BAHandle(LC.problem(name)) as h:
        for radius in LC.RADII:
            h.sweep_once(radius)
            parts = h.sweep_parts()
            all_dense = parts["general_chunks"] == 0 and parts["long_tracks"] == 0 and parts["dense_chunks"] > 0
            assert all_dense == (name in LC.ALL_DENSE or name.startswith("lp:")) and all_dense == h.pt_handoff()
            assert (parts["long_tracks"] > 0) == (name == "r252_253")
            h.dense_solve_once()
            y = h.dense_solution()
            assert np.isfinite(y).all() and np.abs(y).max() > 0
            if not all_dense:  # a form the handle cannot take is refused, not replaced
                for handoff, fused in ((True, False), (False, True), (True, True)):
                    with pytest.raises(capi.MpsfmHipError) as err:
                        h.update_once(radius, y, handoff=handoff, fused_cam=fused)
                    assert err.value.code == UNSUPPORTED
            forms = FORMS if all_dense else {"recompute": (False, False)}
            for step, f in LC.STEPS.items():
                calls.append((radius, step, y * f, {form: h.update_once(radius, y * f, handoff=ho, fused_cam=fu) for form, (ho, fu) in forms.items()}))
        after = LC.problem(name)
        after.pts[:], after.cam_quat[:], after.cam_t[:] = np.nan, np.nan, np.nan
        h.get_state(after)  # behind the last call: the state is still the one the handle was created with
    parts["state_after"] = (after.pts, after.cam_quat, after.cam_t)
    return parts, calls


def check_scene(name, parts, calls):
    prob, scales, worst = LC.problem(name), LC.oracle_systems(name), {}
    for got, want in zip(parts["state_after"], (prob.pts, prob.cam_quat, prob.cam_t)):
        np.testing.assert_array_equal(got, want)
    for radius, step, yc, outs in calls:
        S = NS.LMStep(prob, scales[radius]["cam_scale"], scales[radius]["pt_scale"], yc, radius)
        for form, out in outs.items():
            eta, mcc, tols = check_call(f"{name} r={radius:g} {step} {form}", S, out, step)
            w = worst.setdefault(form, [0.0, 0.0])
            w[0], w[1] = max(w[0], eta), max(w[1], mcc)
        if len(outs) == 4:
            for a, b, same in (("recompute", "recompute+fused", True), ("handoff", "handoff+fused", True), ("recompute", "handoff", False),
                               ("recompute+fused", "handoff+fused", False)):
                check_pair(f"{name} r={radius:g} {step} {a} | {b}", S, outs[a], outs[b], same, tols)
    for form, (eta, mcc) in worst.items():
        print(f"{name} [{form}] dense {parts['dense_chunks']} general {parts['general_chunks']} long {parts['long_tracks']}: "
              f"eta_p {eta:.2e} (bound {LC.ETA_BOUND:.1e})  mcc measure {mcc:.2e} (bound {LC.MCC_BOUND:.1e})")
    return worst


@pytest.mark.parametrize("name", LC.NAMES)
def test_update_once(name):
    parts, calls = run_scene(name)
    assert len(calls) == len(LC.RADII) * len(LC.STEPS)
    assert all(len(outs) == (4 if name in LC.ALL_DENSE or name.startswith("lp:") else 1) for _, _, _, outs in calls)
    check_scene(name, parts, calls)


def test_arguments_are_checked():
    name = "one_var"
    with environment(LC.environment_of(name)), capi.BAHandle(LC.problem(name)) as h:
        n = h.reduced_dim
        bad = np.zeros(n)
        bad[0] = np.nan
        for radius, yc in ((0.0, np.zeros(n)), (np.inf, np.zeros(n)), (1e3, bad)):
            with pytest.raises(capi.MpsfmHipError) as err:
                h.update_once(radius, yc)
            assert err.value.code == -1  # MPSFM_EINVAL
        with pytest.raises(AssertionError):
            h.update_once(1e3, np.zeros(n + 6))
