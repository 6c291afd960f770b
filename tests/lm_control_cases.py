"""One step of the Levenberg-Marquardt controller, stated twice and independently of csrc/lm_decide.h.

`lm_step` restates what one decision launch has to do, from the loop of oracle/ba_oracle.c (oracle_ba_solve: the iteration-0 block
and the body of `while (term < 0)`) and the rules of Ceres' TrustRegionMinimizer and LevenbergMarquardtStrategy.  `ROWS` is a table
of (block before, scalars, options) -> expected values written out by hand.  tests/test_lm_control_cpu.py asserts that the
restatement reproduces every literal of the table; tests/test_gpu_lm_control.py runs every row through the decision kernels.

How a decision launch maps onto the oracle's loop.  Launch k (the block holds iter == k - 1) sees the scalars of iteration k: cost,
invalid count and gradient maxima at the current point x, and the candidate's cost, model cost change and step norms.  It
  1. (k == 1) does the oracle's iteration-0 block: an initial point that cannot be evaluated is a numeric error; cost and trace entry 0;
  2. tests the gradient tolerance where the oracle does: at iteration 0 and after an accepted step (the flag check_gradient);
  3. (k == 1) does the first pass of the loop's head: iteration limit, then radius limit;
  4. does the loop body for iteration k;
  5. does the loop's head for iteration k + 1, unless the body ended the solve.
Two rules are Ceres' where the oracle's C differs in form: the gradient test is `gmax <= tolerance` (a NaN maximum goes on), and
the cube of the radius rule is a product.

The counters follow the work the device does, not the oracle's: every launch stands for one linearisation (n_jac_evals) and one
candidate evaluation (n_cost_evals) of an iteration that was enqueued whole; an ending found before the step is looked at (gradient
tolerance, the limits at iteration 0) takes the iteration and its candidate evaluation back.  A numeric error leaves them as entered.
An initial point where a residual cannot be evaluated arrives as a cost that is not finite; a landmark block that could not be
factored (x_bad with a finite cost) is a failed linear solve: an invalid step, as in Ceres, also at iteration 1."""

import math
import sys

DBL_MAX = sys.float_info.max
NAN, INF = math.nan, math.inf
MAX_TRACE = 64
RUNNING, NUMERIC_ERROR = -1, -2
FUNCTION_TOLERANCE, GRADIENT_TOLERANCE, PARAMETER_TOLERANCE, MAX_ITERATIONS, MIN_RADIUS, INVALID_STEPS = 0, 1, 2, 3, 4, 5

# the 16 scalar slots by name (csrc/common.h, U_*); 12-15 are not read by a decision
SCALAR_SLOTS = {"cand": 0, "bad": 1, "mcc": 2, "step_sq_pts": 3, "xn_sq_pts": 4, "step_sq_cams": 5, "xn_sq_cams": 6, "gmax_cams": 7, "x_cost": 8,
                "x_bad": 9, "gmax_pts": 10, "chol_fail": 11}
HEAD_DOUBLES = ("radius", "decrease_factor", "x_norm", "cur_cost", "fixed_cost", "initial_cost", "last_x_cost", "last_cand", "last_rel", "last_step_norm",
                "last_mcc")
HEAD_INTS = ("term", "iter", "invalid_run", "check_gradient", "accepted", "n_success", "n_unsuccess", "n_cost_evals", "n_jac_evals", "last_chol_fail",
             "trace_len")

# ---- the three starting points of the table ------------------------------------------------------------------------------------------
# a block before the first decision (what solve_impl uploads, x_norm and fixed_cost as the device fills them in)
START = dict(radius=1e4, decrease_factor=2.0, x_norm=3.5, cur_cost=0.0, fixed_cost=0.5, initial_cost=0.0, last_x_cost=0.0, last_cand=0.0, last_rel=0.0,
             last_step_norm=0.0, last_mcc=0.0, term=RUNNING, iter=0, invalid_run=0, check_gradient=1, accepted=0, n_success=0, n_unsuccess=0,
             n_cost_evals=0, n_jac_evals=0, last_chol_fail=0, trace_len=0)
# a block in the middle of a run, after a rejected step (`accepted` still holds the 1 of an earlier launch: every launch resets it)
MID = dict(radius=16.0, decrease_factor=2.0, x_norm=3.5, cur_cost=10.0, fixed_cost=0.5, initial_cost=20.5, last_x_cost=10.0, last_cand=12.0, last_rel=-1.0,
           last_step_norm=1.0, last_mcc=2.0, term=RUNNING, iter=3, invalid_run=0, check_gradient=0, accepted=1, n_success=2, n_unsuccess=1,
           n_cost_evals=3, n_jac_evals=3, last_chol_fail=0, trace_len=4)
# scalars of a step that is accepted with gain ratio (10 - 9) / 2 = 0.5 (the radius stays), |step| = 2, new |x| = 4
SCALARS = dict(cand=9.0, bad=0.0, mcc=2.0, step_sq_pts=3.0, step_sq_cams=1.0, xn_sq_pts=9.0, xn_sq_cams=7.0, gmax_cams=1.0, gmax_pts=0.5, x_cost=10.0,
               x_bad=0.0, chol_fail=0.0)
OPTIONS = dict(function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8, min_relative_decrease=1e-3, max_radius=1e16,
               min_radius=1e-32, max_iterations=50, max_invalid_steps=5)


def _fmax(a, b):
    """C's fmax: a NaN operand is ignored."""
    if a != a:
        return b
    if b != b:
        return a
    return max(a, b)


def _sqrt(v):
    return NAN if v != v or v < 0.0 else math.sqrt(v)  # (math.sqrt(inf) is inf)


def _div(a, b):
    """IEEE division (Python raises on a zero divisor; none of the table's steps divides by zero)."""
    return a / b


def lm_step(block, scalars, options, reached=None):
    """(block after, [(index, cost, radius, accepted) of every trace entry written]) of one decision launch.  reached (a list): receives
    "step", "gain" and "accepted" as the step's norm, its gain ratio and its acceptance are computed."""
    b, s, o = dict(block), scalars, options
    written = []
    reached = [] if reached is None else reached

    def trace(cost, radius, acc):
        if b["trace_len"] < MAX_TRACE:
            written.append((b["trace_len"], cost, radius, acc))
            b["trace_len"] += 1

    def loop_head():  # `while (term < 0)`: the iteration limit, then the radius limit
        if b["term"] != RUNNING:
            return
        if b["iter"] >= o["max_iterations"]:
            b["term"] = MAX_ITERATIONS
        elif b["radius"] <= o["min_radius"]:
            b["term"] = MIN_RADIUS

    if b["term"] != RUNNING:  # a launch queued behind the end of the solve
        return b, written
    first = b["iter"] == 0
    x_cost, fixed = s["x_cost"], b["fixed_cost"]
    b["accepted"] = 0
    b["iter"] += 1
    b["n_jac_evals"] += 1
    b["n_cost_evals"] += 1
    b["last_chol_fail"] = 1 if s["chol_fail"] != 0.0 else 0
    b["last_x_cost"] = x_cost
    if first:  # ---- iteration 0
        if not math.isfinite(x_cost):
            b["term"] = NUMERIC_ERROR
            return b, written
        b["initial_cost"] = x_cost + fixed
        b["cur_cost"] = x_cost
        trace(x_cost + fixed, b["radius"], 1)
    if b["check_gradient"]:
        b["check_gradient"] = 0
        if _fmax(s["gmax_cams"], s["gmax_pts"]) <= o["gradient_tolerance"]:
            b["term"] = GRADIENT_TOLERANCE
            b["iter"] -= 1
            b["n_cost_evals"] -= 1
            return b, written
    if first:  # the loop's head before iteration 1
        if o["max_iterations"] <= 0 or b["radius"] <= o["min_radius"]:
            b["term"] = MAX_ITERATIONS if o["max_iterations"] <= 0 else MIN_RADIUS
            b["iter"] = 0
            b["n_cost_evals"] -= 1
            return b, written
    # ---- the loop body
    mcc = s["mcc"]
    b["last_mcc"] = mcc
    solve_ok = not (s["x_bad"] > 0.0) and s["chol_fail"] == 0.0 and math.isfinite(mcc)  # compute_step's `ok`
    if not (solve_ok and mcc > 0.0):
        b["invalid_run"] += 1
        b["n_unsuccess"] += 1
        if b["invalid_run"] >= o["max_invalid_steps"]:
            b["term"] = INVALID_STEPS
        b["radius"] = b["radius"] / b["decrease_factor"]
        b["decrease_factor"] *= 2.0
        trace(b["cur_cost"] + fixed, b["radius"], 0)
        b["last_cand"], b["last_rel"], b["last_step_norm"] = DBL_MAX, 0.0, 0.0
        loop_head()
        return b, written
    b["invalid_run"] = 0
    cand = DBL_MAX if (s["bad"] > 0.0 or not math.isfinite(s["cand"])) else s["cand"]
    step_norm = _sqrt(s["step_sq_pts"] + s["step_sq_cams"])
    b["last_cand"], b["last_step_norm"] = cand, step_norm
    reached.append("step")
    if step_norm <= o["parameter_tolerance"] * (b["x_norm"] + o["parameter_tolerance"]):
        b["term"] = PARAMETER_TOLERANCE
        return b, written
    cost_change = x_cost - cand
    if abs(cost_change) <= o["function_tolerance"] * x_cost:
        b["term"] = FUNCTION_TOLERANCE
        return b, written
    rel = _div(cost_change, mcc)
    b["last_rel"] = rel
    reached.append("gain")
    if rel > o["min_relative_decrease"]:
        b["accepted"] = 1
        reached.append("accepted")
        b["x_norm"] = _sqrt(s["xn_sq_pts"] + s["xn_sq_cams"])
        b["cur_cost"] = cand
        u = 2.0 * rel - 1.0
        b["radius"] = min(o["max_radius"], _div(b["radius"], max(1.0 / 3.0, 1.0 - u * u * u)))
        b["decrease_factor"] = 2.0
        b["n_success"] += 1
        b["check_gradient"] = 1
        trace(cand + fixed, b["radius"], 1)
    else:
        b["radius"] = b["radius"] / b["decrease_factor"]
        b["decrease_factor"] *= 2.0
        b["n_unsuccess"] += 1
        trace(b["cur_cost"] + fixed, b["radius"], 0)
    loop_head()
    return b, written


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
def _below(v):
    return math.nextafter(v, -INF)


def _above(v):
    return math.nextafter(v, INF)


EXPECTED_FIELDS = ("term", "accepted", "iter", "invalid_run", "n_success", "n_unsuccess", "n_cost_evals", "n_jac_evals", "check_gradient", "trace_len",
                   "trace", "radius", "decrease_factor", "cur_cost", "x_norm")


def E(term, accepted, iter, invalid_run, n_success, n_unsuccess, n_cost_evals, n_jac_evals, check_gradient, trace_len, trace, radius, decrease_factor,
      cur_cost, x_norm):
    """The expected values of a row.  trace: the entries written, (cost, radius, accepted) each, from the block's trace_len on."""
    return dict(zip(EXPECTED_FIELDS, (term, accepted, iter, invalid_run, n_success, n_unsuccess, n_cost_evals, n_jac_evals, check_gradient, trace_len,
                                      tuple(trace), radius, decrease_factor, cur_cost, x_norm)))


ROWS = []


def row(name, expected, base=MID, block=None, scalars=None, options=None, unchanged=False):
    assert name not in [r["name"] for r in ROWS], name
    ROWS.append(dict(name=name, block={**base, **(block or {})}, scalars={**SCALARS, **(scalars or {})}, options={**OPTIONS, **(options or {})},
                     expected=expected, unchanged=unchanged))


# Outcomes that many rows share, each written out once.  From MID: iteration 4, the counters one up.
MID_ACCEPT = E(RUNNING, 1, 4, 0, 3, 1, 4, 4, 1, 5, [(9.5, 16.0, 1)], 16.0, 2.0, 9.0, 4.0)     # gain ratio 0.5: the radius stays
MID_REJECT = E(RUNNING, 0, 4, 0, 2, 2, 4, 4, 0, 5, [(10.5, 8.0, 0)], 8.0, 4.0, 10.0, 3.5)     # radius / 2, the next rejection divides by 4
MID_INVALID = E(RUNNING, 0, 4, 1, 2, 2, 4, 4, 0, 5, [(10.5, 8.0, 0)], 8.0, 4.0, 10.0, 3.5)    # the same and one invalid step counted
START_ACCEPT = E(RUNNING, 1, 1, 0, 1, 0, 1, 1, 1, 2, [(10.5, 1e4, 1), (9.5, 1e4, 1)], 1e4, 2.0, 9.0, 4.0)
START_NUMERIC = E(NUMERIC_ERROR, 0, 1, 0, 0, 0, 1, 1, 1, 0, [], 1e4, 2.0, 0.0, 3.5)
START_ENDS_AT_0 = dict(accepted=0, iter=0, invalid_run=0, n_success=0, n_unsuccess=0, n_cost_evals=0, n_jac_evals=1, check_gradient=0, trace_len=1,
                       trace=((10.5, 1e4, 1),), radius=1e4, decrease_factor=2.0, cur_cost=10.0, x_norm=3.5)  # ended before iteration 1

# ---- iteration 1
row("start_accept", START_ACCEPT, START)
row("start_cost_nan", START_NUMERIC, START, scalars=dict(x_cost=NAN))
row("start_cost_inf", START_NUMERIC, START, scalars=dict(x_cost=INF))
row("start_cost_minus_inf", START_NUMERIC, START, scalars=dict(x_cost=-INF))
row("start_cost_nan_and_x_bad", START_NUMERIC, START, scalars=dict(x_cost=NAN, x_bad=1.0))  # a residual that cannot be evaluated: both signs
row("start_x_bad_is_an_invalid_step", E(RUNNING, 0, 1, 1, 0, 1, 1, 1, 0, 2, [(10.5, 1e4, 1), (10.5, 5e3, 0)], 5e3, 4.0, 10.0, 3.5), START,
    scalars=dict(x_bad=3.0))
row("start_gradient_below", {"term": GRADIENT_TOLERANCE, **START_ENDS_AT_0}, START, scalars=dict(gmax_cams=1e-11, gmax_pts=5e-12))
row("start_no_iterations", {"term": MAX_ITERATIONS, **START_ENDS_AT_0}, START, options=dict(max_iterations=0))
row("start_negative_iterations", {"term": MAX_ITERATIONS, **START_ENDS_AT_0}, START, options=dict(max_iterations=-1))
row("start_radius_equals_min", {"term": MIN_RADIUS, **START_ENDS_AT_0}, START, options=dict(min_radius=1e4))
row("start_radius_ulp_above_min", START_ACCEPT, START, options=dict(min_radius=_below(1e4)))
row("start_radius_ulp_below_min", {"term": MIN_RADIUS, **START_ENDS_AT_0}, START, options=dict(min_radius=_above(1e4)))
# the order of the tests at the start: gradient, then iterations, then radius
row("start_order_gradient_first", {"term": GRADIENT_TOLERANCE, **START_ENDS_AT_0}, START, scalars=dict(gmax_cams=1e-11, gmax_pts=5e-12),
    options=dict(max_iterations=0, min_radius=1e4))
row("start_order_iterations_before_radius", {"term": MAX_ITERATIONS, **START_ENDS_AT_0}, START, options=dict(max_iterations=0, min_radius=1e4))
row("start_one_iteration", {**START_ACCEPT, "term": MAX_ITERATIONS}, START, options=dict(max_iterations=1))  # the accepted step still counts

# ---- invalid steps
row("invalid_chol_fail", MID_INVALID, scalars=dict(chol_fail=1.0))
row("invalid_x_bad", MID_INVALID, scalars=dict(x_bad=1.0))
row("invalid_mcc_zero", MID_INVALID, scalars=dict(mcc=0.0))
row("invalid_mcc_negative", MID_INVALID, scalars=dict(mcc=-1.0))
row("invalid_mcc_nan", MID_INVALID, scalars=dict(mcc=NAN))
row("invalid_mcc_inf", MID_INVALID, scalars=dict(mcc=INF))
row("invalid_mcc_minus_inf", MID_INVALID, scalars=dict(mcc=-INF))
row("invalid_ignores_the_candidate", MID_INVALID, scalars=dict(chol_fail=1.0, cand=NAN, bad=7.0, step_sq_pts=NAN))
row("invalid_run_one_below_the_limit", E(RUNNING, 0, 4, 4, 2, 2, 4, 4, 0, 5, [(10.5, 8.0, 0)], 8.0, 4.0, 10.0, 3.5), block=dict(invalid_run=3),
    scalars=dict(chol_fail=1.0))
row("invalid_run_reaches_the_limit", E(INVALID_STEPS, 0, 4, 5, 2, 2, 4, 4, 0, 5, [(10.5, 8.0, 0)], 8.0, 4.0, 10.0, 3.5), block=dict(invalid_run=4),
    scalars=dict(chol_fail=1.0))
row("invalid_limit_of_one", E(INVALID_STEPS, 0, 4, 1, 2, 2, 4, 4, 0, 5, [(10.5, 8.0, 0)], 8.0, 4.0, 10.0, 3.5), scalars=dict(mcc=0.0),
    options=dict(max_invalid_steps=1))
row("invalid_second_in_a_row_divides_by_4", E(RUNNING, 0, 4, 2, 2, 2, 4, 4, 0, 5, [(10.5, 2.0, 0)], 2.0, 8.0, 10.0, 3.5),
    block=dict(invalid_run=1, radius=8.0, decrease_factor=4.0), scalars=dict(chol_fail=1.0))
row("valid_after_invalid_resets_the_run", MID_ACCEPT, block=dict(invalid_run=2, decrease_factor=8.0))
row("rejected_after_invalid_resets_the_run", E(RUNNING, 0, 4, 0, 2, 2, 4, 4, 0, 5, [(10.5, 2.0, 0)], 2.0, 16.0, 10.0, 3.5),
    block=dict(invalid_run=2, decrease_factor=8.0), scalars=dict(cand=11.0))
row("invalid_then_the_iteration_limit", {**MID_INVALID, "term": MAX_ITERATIONS, "iter": 50}, block=dict(iter=49), scalars=dict(chol_fail=1.0))
row("invalid_limit_before_the_iteration_limit", E(INVALID_STEPS, 0, 50, 5, 2, 2, 4, 4, 0, 5, [(10.5, 8.0, 0)], 8.0, 4.0, 10.0, 3.5),
    block=dict(iter=49, invalid_run=4), scalars=dict(chol_fail=1.0))
row("invalid_lands_on_min_radius", {**MID_INVALID, "term": MIN_RADIUS}, scalars=dict(mcc=0.0), options=dict(min_radius=8.0))

# ---- the candidate's cost
row("candidate_bad_count", MID_REJECT, scalars=dict(bad=2.0))
row("candidate_cost_nan", MID_REJECT, scalars=dict(cand=NAN))
row("candidate_cost_inf", MID_REJECT, scalars=dict(cand=INF))
row("candidate_cost_minus_inf", MID_REJECT, scalars=dict(cand=-INF))  # not a decrease: not finite
row("candidate_worse", MID_REJECT, scalars=dict(cand=11.0))

# ---- comparisons on their boundary, values exact in binary64; _below / _above: one ulp to either side
PARAMETER_END = E(PARAMETER_TOLERANCE, 0, 4, 0, 2, 1, 4, 4, 0, 4, [], 16.0, 2.0, 10.0, 3.5)
row("step_norm_equals_bound", PARAMETER_END, options=dict(parameter_tolerance=0.5))  # sqrt(3 + 1) = 2 = 0.5 (3.5 + 0.5)
row("step_norm_bound_ulp_smaller", MID_ACCEPT, block=dict(x_norm=_below(3.5)), options=dict(parameter_tolerance=0.5))  # 0.5 * 3.9999999999999996 < 2
row("step_norm_ulp_smaller", PARAMETER_END, scalars=dict(step_sq_pts=_below(4.0), step_sq_cams=0.0), options=dict(parameter_tolerance=0.5))
row("step_norm_larger", MID_ACCEPT, scalars=dict(step_sq_pts=3.0, step_sq_cams=1.5), options=dict(parameter_tolerance=0.5))
FUNCTION_END = E(FUNCTION_TOLERANCE, 0, 4, 0, 2, 1, 4, 4, 0, 4, [], 16.0, 2.0, 8.0, 3.5)
FTOL = dict(block=dict(cur_cost=8.0), scalars=dict(x_cost=8.0, cand=7.0))  # |8 - 7| = 1 = 0.125 * 8
row("cost_change_equals_bound", FUNCTION_END, **FTOL, options=dict(function_tolerance=0.125))
row("cost_change_bound_ulp_smaller", E(RUNNING, 1, 4, 0, 3, 1, 4, 4, 1, 5, [(7.5, 16.0, 1)], 16.0, 2.0, 7.0, 4.0), **FTOL,
    options=dict(function_tolerance=_below(0.125)))
row("cost_change_bound_ulp_larger", FUNCTION_END, **FTOL, options=dict(function_tolerance=_above(0.125)))
row("cost_increase_within_bound", FUNCTION_END, block=dict(cur_cost=8.0), scalars=dict(x_cost=8.0, cand=9.0), options=dict(function_tolerance=0.125))
row("parameter_before_function_tolerance", E(PARAMETER_TOLERANCE, 0, 4, 0, 2, 1, 4, 4, 0, 4, [], 16.0, 2.0, 8.0, 3.5), **FTOL,
    options=dict(function_tolerance=0.125, parameter_tolerance=0.5))
REL = dict(scalars=dict(mcc=8.0))  # (10 - 9) / 8 = 0.125
row("gain_ratio_equals_bound_rejects", MID_REJECT, **REL, options=dict(min_relative_decrease=0.125))
row("gain_ratio_bound_ulp_larger", MID_REJECT, **REL, options=dict(min_relative_decrease=_above(0.125)))
# accepted with u = 2 * 0.125 - 1 = -0.75, 1 - u^3 = 1.421875 (exact): radius 16 / 1.421875
row("gain_ratio_bound_ulp_smaller", E(RUNNING, 1, 4, 0, 3, 1, 4, 4, 1, 5, [(9.5, 11.252747252747254, 1)], 11.252747252747254, 2.0, 9.0, 4.0), **REL,
    options=dict(min_relative_decrease=_below(0.125)))
GRAD = dict(block=dict(check_gradient=1), scalars=dict(gmax_cams=2.0 ** -30, gmax_pts=2.0 ** -31))
GRADIENT_END = E(GRADIENT_TOLERANCE, 0, 3, 0, 2, 1, 3, 4, 0, 4, [], 16.0, 2.0, 10.0, 3.5)  # iteration and candidate evaluation taken back
row("gradient_equals_tolerance", GRADIENT_END, **GRAD, options=dict(gradient_tolerance=2.0 ** -30))
row("gradient_equals_tolerance_on_the_landmarks", GRADIENT_END, block=dict(check_gradient=1), scalars=dict(gmax_cams=2.0 ** -31, gmax_pts=2.0 ** -30),
    options=dict(gradient_tolerance=2.0 ** -30))
row("gradient_tolerance_ulp_smaller", MID_ACCEPT, **GRAD, options=dict(gradient_tolerance=_below(2.0 ** -30)))
row("gradient_tolerance_ulp_larger", GRADIENT_END, **GRAD, options=dict(gradient_tolerance=_above(2.0 ** -30)))
row("gradient_not_looked_at_after_a_rejection", MID_ACCEPT, scalars=dict(gmax_cams=0.0, gmax_pts=0.0))  # check_gradient is 0 in MID
row("gradient_nan_goes_on", MID_ACCEPT, block=dict(check_gradient=1), scalars=dict(gmax_cams=NAN, gmax_pts=NAN))
row("gradient_one_nan_is_ignored", GRADIENT_END, block=dict(check_gradient=1), scalars=dict(gmax_cams=NAN, gmax_pts=1e-11))
REJECT = dict(scalars=dict(cand=11.0))
row("rejection_lands_on_min_radius", {**MID_REJECT, "term": MIN_RADIUS}, **REJECT, options=dict(min_radius=8.0))
row("rejection_ulp_above_min_radius", MID_REJECT, **REJECT, options=dict(min_radius=_below(8.0)))
row("rejection_ulp_below_min_radius", {**MID_REJECT, "term": MIN_RADIUS}, **REJECT, options=dict(min_radius=_above(8.0)))
row("rejection_then_the_iteration_limit", {**MID_REJECT, "term": MAX_ITERATIONS, "iter": 50}, block=dict(iter=49), **REJECT)
row("iteration_limit_before_min_radius", {**MID_REJECT, "term": MAX_ITERATIONS, "iter": 50}, block=dict(iter=49), **REJECT, options=dict(min_radius=8.0))
row("acceptance_then_the_iteration_limit", {**MID_ACCEPT, "term": MAX_ITERATIONS, "iter": 50}, block=dict(iter=49))

# ---- the radius rule of an accepted step: radius / max(1/3, 1 - (2 rel - 1)^3), clamped
TRIPLED = E(RUNNING, 1, 4, 0, 3, 1, 4, 4, 1, 5, [(8.5, 48.0, 1)], 48.0, 2.0, 8.0, 4.0)
row("gain_ratio_one_triples", TRIPLED, scalars=dict(cand=8.0))  # u = 1: 16 / (1/3) rounds to 48
row("gain_ratio_above_one_triples", E(RUNNING, 1, 4, 0, 3, 1, 4, 4, 1, 5, [(4.5, 48.0, 1)], 48.0, 2.0, 4.0, 4.0), scalars=dict(cand=4.0))
row("gain_ratio_half_keeps_the_radius", MID_ACCEPT)
# rel = 2^-9 just above 1e-3: u = -255/256, 1 - u^3 = 33358591 / 16777216 (exact): the radius about halves
row("gain_ratio_just_above_min", E(RUNNING, 1, 4, 0, 3, 1, 4, 4, 1, 5, [(10.498046875, 8.046966252261674, 1)], 8.046966252261674, 2.0, 9.998046875, 4.0),
    scalars=dict(cand=9.998046875, mcc=1.0))
row("accepted_onto_min_radius", E(MIN_RADIUS, 1, 4, 0, 3, 1, 4, 4, 1, 5, [(10.498046875, 8.046966252261674, 1)], 8.046966252261674, 2.0, 9.998046875, 4.0),
    scalars=dict(cand=9.998046875, mcc=1.0), options=dict(min_radius=9.0))
row("max_radius_clamps", E(RUNNING, 1, 4, 0, 3, 1, 4, 4, 1, 5, [(8.5, 40.0, 1)], 40.0, 2.0, 8.0, 4.0), scalars=dict(cand=8.0), options=dict(max_radius=40.0))
row("max_radius_equal_to_the_new_radius", TRIPLED, scalars=dict(cand=8.0), options=dict(max_radius=48.0))
row("max_radius_below_the_old_radius", E(RUNNING, 1, 4, 0, 3, 1, 4, 4, 1, 5, [(9.5, 12.0, 1)], 12.0, 2.0, 9.0, 4.0), options=dict(max_radius=12.0))
row("accepted_resets_the_decrease_factor", MID_ACCEPT, block=dict(decrease_factor=16.0))
row("model_change_denormal", E(RUNNING, 1, 4, 0, 3, 1, 4, 4, 1, 5, [(9.5, 48.0, 1)], 48.0, 2.0, 9.0, 4.0), scalars=dict(mcc=5e-324))  # rel = +inf

# steps whose gain ratio, norms and radius factor are all inexact (the literals: binary64 with correctly rounded sqrt and division)
row("inexact_quantities_a", E(RUNNING, 1, 4, 0, 3, 1, 4, 4, 1, 5, [(9.8, 14.393418647166355, 1)], 14.393418647166355, 2.0, 9.3, 4.049691346263317),
    scalars=dict(cand=9.3, mcc=2.7, step_sq_pts=3.3, step_sq_cams=1.1, xn_sq_pts=9.1, xn_sq_cams=7.3))
row("inexact_quantities_b", E(RUNNING, 1, 4, 0, 3, 1, 4, 4, 1, 5, [(3.4, 40.155067396706016, 1)], 40.155067396706016, 2.0, 2.9, 447.2135966179919),
    scalars=dict(cand=2.9, mcc=7.7, step_sq_pts=0.3, step_sq_cams=0.07, xn_sq_pts=1e-3, xn_sq_cams=2e5))
row("inexact_quantities_c", E(RUNNING, 1, 4, 0, 3, 1, 4, 4, 1, 5, [(10.49, 18.960086299891486, 1)], 18.960086299891486, 2.0, 9.99, 11.115574659008862),
    scalars=dict(cand=9.99, mcc=0.013, step_sq_pts=1e-7, step_sq_cams=3e-9, xn_sq_pts=123.456, xn_sq_cams=0.1))

# ---- NaN and infinities in the remaining scalars
row("step_norm_nan_goes_on", MID_ACCEPT, scalars=dict(step_sq_pts=NAN))
row("state_norm_inf", {**MID_ACCEPT, "x_norm": INF}, scalars=dict(xn_sq_cams=INF))
row("cost_nan_in_the_run_rejects", MID_REJECT, scalars=dict(x_cost=NAN))  # only the first launch takes a cost that is not finite for an error

# ---- the trace
row("trace_last_slot", {**MID_ACCEPT, "trace_len": 64}, block=dict(trace_len=63))
row("trace_full", {**MID_ACCEPT, "trace_len": 64, "trace": ()}, block=dict(trace_len=64))
row("trace_full_rejection", {**MID_REJECT, "trace_len": 64, "trace": ()}, block=dict(trace_len=64), **REJECT)
row("trace_fills_during_the_first_launch", E(RUNNING, 1, 1, 0, 1, 0, 1, 1, 1, 64, [(10.5, 1e4, 1)], 1e4, 2.0, 9.0, 4.0), START,
    block=dict(trace_len=63))

# ---- a block that is already decided comes back bit for bit, and so do the scalars
for _term in (FUNCTION_TOLERANCE, MAX_ITERATIONS, INVALID_STEPS, NUMERIC_ERROR):
    row(f"already_decided_{_term if _term >= 0 else 'numeric_error'}", E(_term, 1, 3, 0, 2, 1, 3, 3, 0, 4, [], 16.0, 2.0, 10.0, 3.5), block=dict(term=_term),
        unchanged=True)


# ---- the four quantities that go through the device's sqrt, its division and 1 - u^3, at 60 digits ------------------------------------------
def exact_quantities(r):
    """{radius, x_norm, last_step_norm, last_rel} of row r's step as mpmath values; None: this step does not compute it, or an operand
    is not finite (IEEE fixes the result then, and the comparison is exact)."""
    import mpmath as mp

    reached, s, o = [], r["scalars"], r["options"]
    after, _ = lm_step(r["block"], s, o, reached)
    out = dict(radius=None, x_norm=None, last_step_norm=None, last_rel=None)
    with mp.workdps(60):
        if "step" in reached and math.isfinite(after["last_step_norm"]):
            out["last_step_norm"] = mp.sqrt(mp.mpf(s["step_sq_pts"]) + mp.mpf(s["step_sq_cams"]))
        if "gain" in reached and math.isfinite(after["last_rel"]):
            out["last_rel"] = (mp.mpf(s["x_cost"]) - mp.mpf(after["last_cand"])) / mp.mpf(s["mcc"])
        if "accepted" in reached and math.isfinite(after["x_norm"]):
            out["x_norm"] = mp.sqrt(mp.mpf(s["xn_sq_pts"]) + mp.mpf(s["xn_sq_cams"]))
        if "accepted" in reached and math.isfinite(after["last_rel"]):
            u = 2 * mp.mpf(after["last_rel"]) - 1  # the rule starts from the rounded gain ratio
            out["radius"] = min(mp.mpf(o["max_radius"]), mp.mpf(r["block"]["radius"]) / max(mp.mpf(1.0 / 3.0), 1 - u ** 3))
    return out


def ulp_distance(value, exact):
    """|value - exact| in units of the spacing of binary64 at `exact`."""
    import mpmath as mp

    with mp.workdps(60):
        if exact == 0:
            return 0.0 if value == 0.0 else INF
        e = int(mp.floor(mp.log(abs(exact), 2)))
        return float(abs(mp.mpf(value) - exact) / mp.mpf(2) ** (e - 52))
