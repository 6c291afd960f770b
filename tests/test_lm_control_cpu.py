"""The table of controller steps (tests/lm_control_cases.py) against the restatement in the same module: every hand-written expected
value of every row must be what `lm_step` computes, so each expectation of tests/test_gpu_lm_control.py is stated twice.  Also that
the table reaches what it is there for: every termination code, every boundary with both neighbours, every special value."""

import math

import pytest

import lm_control_cases as LC


def _same(a, b):
    return (a != a and b != b) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))


@pytest.mark.parametrize("r", LC.ROWS, ids=[r["name"] for r in LC.ROWS])
def test_restatement_reproduces_the_rows_literals(r):
    after, written = LC.lm_step(r["block"], r["scalars"], r["options"])
    want = r["expected"]
    assert set(want) == set(LC.EXPECTED_FIELDS)
    for f in LC.EXPECTED_FIELDS:
        if f == "trace":
            continue
        if isinstance(want[f], float):
            assert _same(float(after[f]), want[f]), (f, after[f], want[f])
        else:
            assert type(after[f]) is int and after[f] == want[f], (f, after[f], want[f])
    # the entries written start at the block's trace_len and are consecutive; past the arrays nothing is written
    assert [w[0] for w in written] == list(range(r["block"]["trace_len"], r["block"]["trace_len"] + len(written)))
    assert all(w[0] < LC.MAX_TRACE for w in written) and after["trace_len"] == r["block"]["trace_len"] + len(written) <= LC.MAX_TRACE
    assert len(written) == len(want["trace"])
    for (_, cost, radius, acc), (wc, wr, wa) in zip(written, want["trace"]):
        assert _same(cost, wc) and _same(radius, wr) and acc == wa, (written, want["trace"])
    if r["unchanged"]:
        assert after == r["block"] and not written


def test_the_table_reaches_every_branch():
    terms = {r["expected"]["term"] for r in LC.ROWS}
    assert terms == {LC.RUNNING, LC.NUMERIC_ERROR, LC.FUNCTION_TOLERANCE, LC.GRADIENT_TOLERANCE, LC.PARAMETER_TOLERANCE, LC.MAX_ITERATIONS, LC.MIN_RADIUS,
                     LC.INVALID_STEPS}
    assert len(LC.ROWS) >= 40
    first = [r for r in LC.ROWS if r["block"]["iter"] == 0]
    assert {r["expected"]["term"] for r in first} >= {LC.NUMERIC_ERROR, LC.GRADIENT_TOLERANCE, LC.MAX_ITERATIONS, LC.MIN_RADIUS, LC.RUNNING}
    values = [v for r in LC.ROWS for v in r["scalars"].values()]
    assert any(v != v for v in values) and LC.INF in values and -LC.INF in values
    assert any(r["expected"]["decrease_factor"] == 8.0 for r in LC.ROWS), "a second invalid step in a row divides by 4"
    assert any(r["block"]["invalid_run"] > 0 and r["expected"]["invalid_run"] == 0 for r in LC.ROWS)
    assert {r["block"]["trace_len"] for r in LC.ROWS} >= {63, 64}
    assert sum(r["unchanged"] for r in LC.ROWS) >= 2


def test_every_boundary_has_both_neighbours():
    """A row on the boundary and rows one ulp to either side that decide differently on at least one side."""
    by = {r["name"]: r["expected"]["term"] for r in LC.ROWS}
    acc = {r["name"]: r["expected"]["accepted"] for r in LC.ROWS}
    assert (by["step_norm_equals_bound"], by["step_norm_bound_ulp_smaller"], by["step_norm_ulp_smaller"]) == (LC.PARAMETER_TOLERANCE, LC.RUNNING,
                                                                                                             LC.PARAMETER_TOLERANCE)
    assert (by["cost_change_equals_bound"], by["cost_change_bound_ulp_smaller"], by["cost_change_bound_ulp_larger"]) == (LC.FUNCTION_TOLERANCE, LC.RUNNING,
                                                                                                                       LC.FUNCTION_TOLERANCE)
    assert (acc["gain_ratio_equals_bound_rejects"], acc["gain_ratio_bound_ulp_smaller"], acc["gain_ratio_bound_ulp_larger"]) == (0, 1, 0)
    assert (by["gradient_equals_tolerance"], by["gradient_tolerance_ulp_smaller"], by["gradient_tolerance_ulp_larger"]) == (LC.GRADIENT_TOLERANCE, LC.RUNNING,
                                                                                                                          LC.GRADIENT_TOLERANCE)
    assert (by["rejection_lands_on_min_radius"], by["rejection_ulp_above_min_radius"], by["rejection_ulp_below_min_radius"]) == (LC.MIN_RADIUS, LC.RUNNING,
                                                                                                                               LC.MIN_RADIUS)
    assert (by["start_radius_equals_min"], by["start_radius_ulp_above_min"], by["start_radius_ulp_below_min"]) == (LC.MIN_RADIUS, LC.RUNNING, LC.MIN_RADIUS)
    assert (by["invalid_run_one_below_the_limit"], by["invalid_run_reaches_the_limit"]) == (LC.RUNNING, LC.INVALID_STEPS)


def test_exact_quantities_agree_with_binary64_on_the_host():
    """The mpmath evaluation the GPU test measures against.  On the host the gain ratio is one correctly rounded division (half an ulp),
    a norm is a rounded sum under a correctly rounded root (half an ulp each at most: one ulp), and the radius chains five roundings
    behind the rounded gain ratio, the subtraction from 1 amplifying them by up to 3 (the factor is at least 1/3): within the 8 ulp
    the GPU test never exceeds."""
    n = 0
    for r in LC.ROWS:
        after, _ = LC.lm_step(r["block"], r["scalars"], r["options"])
        for f, exact in LC.exact_quantities(r).items():
            if exact is not None:
                assert LC.ulp_distance(after[f], exact) <= {"radius": 8.0, "last_rel": 0.5}.get(f, 1.0), (r["name"], f)
                n += 1
    assert n >= 100
