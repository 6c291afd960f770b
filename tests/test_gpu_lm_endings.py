"""The rare endings of the trust-region loop through the real solve, in every form of the solver: the launch chain with the whole
iteration, its front half or nothing enqueued ahead (solve_impl, csrc/ba_solver.hip), the single-launch solver (csrc/local_lm.hip) and a
handle with an all-reduce hook (k_lm_decide on the all-reduced tail).  Each case is a scene and options that drive the CPU oracle into
one branch — minimum radius mid-run and at iteration 0, consecutive invalid steps, the maximum-radius clamp, a non-default
min_relative_decrease, the parameter tolerance, a trace longer than MPSFM_MAX_TRACE — and every form must take the oracle's decisions.
What the oracle does is asserted too, so that a scene which stops producing its branch fails here and not silently.

The invalid-step cases overflow the damping (min_lm_diagonal / radius = 1e300 / 1e-300 = +inf): no landmark block can be factored and the
reduced system is not finite, so every decision is forced by IEEE arithmetic.  Ceres counts a failed linear solve as an invalid step; the
initial point itself is evaluable.  Numeric errors are the other side of that line: a landmark coordinate that is NaN, and a depth prior
that sees a negative depth.

The file runs the chain forms first and the single-launch solver last."""

import functools

import numpy as np
import pytest

from mpsfm_amd import capi
from mpsfm_amd.abi import ALLREDUCE_FN
from mpsfm_amd.synthetic import make_scene
from oracle import cpu_oracle as O
from test_gpu_level_entry import _Env
from test_gpu_lm_split import K_CHOL_LEVEL, launch_counts
from test_gpu_local_lm import local_iterations

pytestmark = pytest.mark.gpu

MPSFM_ENUMERIC = -5
_SWITCHES = ("MPSFM_LOCAL_LM", "MPSFM_LM_SPLIT", "MPSFM_LM_SPECULATE")
# form -> (environment, dead level launches per solve or None: not a chain setting, hook?)
FORMS = {
    "whole": ({"MPSFM_LOCAL_LM": "0", "MPSFM_LM_SPLIT": "0", "MPSFM_LM_SPECULATE": None}, 1, False),
    "split": ({"MPSFM_LOCAL_LM": "0", "MPSFM_LM_SPLIT": "1", "MPSFM_LM_SPECULATE": None}, 0, False),
    "no_speculation": ({"MPSFM_LOCAL_LM": "0", "MPSFM_LM_SPLIT": None, "MPSFM_LM_SPECULATE": "0"}, 0, False),
    "hook": ({k: None for k in _SWITCHES}, None, True),
    "single_launch": ({k: None for k in _SWITCHES}, None, False),
}
CHAIN_FORMS = ["whole", "split", "no_speculation", "hook"]
_HOOK = ALLREDUCE_FN(lambda user, buf, count, on_device, stream: 0)  # one rank: the sum is what is there


def scene(which):
    """S: test_gpu_local_lm.py::test_rejected_steps_and_the_iteration_limit's start; U: the same scene unperturbed; D: with depth priors."""
    prob = make_scene(8, 1200, which == "D", seed=13)[0]
    if which == "S":
        rng = np.random.default_rng(3)
        prob.pts += rng.normal(0, 0.3, prob.pts.shape)
        q = prob.cam_quat[1:] + rng.normal(0, 0.25, prob.cam_quat[1:].shape)
        prob.cam_quat[1:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return prob


_OVERFLOW = dict(initial_trust_region_radius=1e-300, min_trust_region_radius=0.0, min_lm_diagonal=1e300, max_lm_diagonal=1e308)
# name -> (scene, options, what the oracle does: termination, iterations, successful, unsuccessful, trace length)
CASES = {
    "min_radius_after_5": ("S", dict(initial_trust_region_radius=1e16, min_trust_region_radius=1e14), ("min_radius", 5, 1, 4, 6)),
    "min_radius_after_7": ("S", dict(initial_trust_region_radius=1e16, min_trust_region_radius=1e10, max_num_iterations=30), ("min_radius", 7, 1, 6, 8)),
    "min_radius_at_0": ("U", dict(initial_trust_region_radius=1.0, min_trust_region_radius=1.0), ("min_radius", 0, 0, 0, 1)),
    "invalid_steps_after_5": ("S", _OVERFLOW, ("invalid_steps", 5, 0, 5, 6)),
    "invalid_steps_after_1": ("S", dict(_OVERFLOW, max_num_consecutive_invalid_steps=1), ("invalid_steps", 1, 0, 1, 2)),
    "max_radius_clamp": ("U", dict(max_trust_region_radius=2e4, max_num_iterations=10), ("max_iterations", 10, 10, 0, 11)),
    "min_relative_decrease": ("S", dict(initial_trust_region_radius=1e16, min_relative_decrease=0.75, max_num_iterations=30), ("max_iterations", 30, 21, 9, 31)),
    "parameter_tolerance": ("U", dict(parameter_tolerance=1e-3), ("parameter_tolerance", 3, 2, 0, 3)),
    "trace_overflow": ("U", dict(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0, max_num_iterations=80), ("max_iterations", 80, 80, 0, 64)),
}
STATE_UNTOUCHED = ("invalid_steps_after_5", "invalid_steps_after_1", "min_radius_at_0")


@functools.lru_cache(maxsize=None)
def oracle(case):
    which, opts, (term, its, good, bad, tlen) = CASES[case]
    p = scene(which)
    s = O.solve(p, O.default_options(**opts))
    assert (s["termination"], s["num_iterations"], s["num_successful_steps"], s["num_unsuccessful_steps"], len(s["trace_cost"])) == (term, its, good, bad, tlen), s
    acc, rad = list(s["trace_accepted"]), np.array(s["trace_radius"])
    if case == "min_radius_after_5":
        assert acc == [1, 1, 0, 0, 0, 0] and s["final_radius"] == 1e16 / 1024
    if case == "invalid_steps_after_5":
        assert acc == [1, 0, 0, 0, 0, 0] and list(rad) == [1e-300 / d for d in (1, 2, 8, 64, 1024, 32768)]
    if case == "invalid_steps_after_1":
        assert acc == [1, 0] and list(rad) == [1e-300, 5e-301]
    if case == "max_radius_clamp":
        assert rad[0] == 1e4 and (rad[1:] == 2e4).all() and s["final_radius"] == 2e4
    if case == "min_radius_at_0":
        assert acc == [1] and s["final_radius"] == 1.0
    return s, p


def noise_from(case):
    """First iteration whose oracle |cost change| / cost is below 1e-9: from there on the accept flags are rounding noise (None: never)."""
    if case != "trace_overflow":
        return None
    c = np.array(oracle(case)[0]["trace_cost"])
    small = np.nonzero(np.abs(np.diff(c)) / c[:-1] < 1e-9)[0]
    assert len(small) and small[0] + 1 > 20, "the scene is meant to converge long before the trace is full, and not at once"
    return int(small[0]) + 1


def solve(form, prob, opts):
    """(summary, state after, launch counts, levels, iterations inside the single launch or -1)."""
    env, _, hook = FORMS[form]
    o = capi.default_options(**opts, **(dict(allreduce=_HOOK, world_size=1, rank=0) if hook else {}))
    out = prob.copy()
    with _Env(env), capi.BAHandle(prob.copy(), o) as h:
        levels = h.dense_plan()["levels"]
        s = h.solve()
        h.get_state(out)
        return s, out, launch_counts(h), levels, local_iterations(h)


def assert_states_close(a, b, atol):
    np.testing.assert_allclose(a.pts, b.pts, atol=atol)
    np.testing.assert_allclose(a.cam_t, b.cam_t, atol=atol)
    sign = np.sign(np.sum(a.cam_quat * b.cam_quat, axis=1, keepdims=True))
    np.testing.assert_allclose(a.cam_quat, sign * b.cam_quat, atol=atol)


def check_case(form, case):
    which, opts, _ = CASES[case]
    so, po = oracle(case)
    start = scene(which)
    s, out, counts, levels, local_its = solve(form, start, opts)
    print(f"ENDING {case} [{form}]: {s['termination']} after {s['num_iterations']}, {s['num_successful_steps']} + {s['num_unsuccessful_steps']}, trace {len(s['trace_cost'])}, "
          f"final radius {s['final_radius']:.6g} (oracle {so['final_radius']:.6g}), level launches {counts[K_CHOL_LEVEL]} at {levels} levels, local {local_its}")
    assert (local_its >= 0) == (form == "single_launch"), "the form under test is not the one that ran"
    assert s["termination"] == so["termination"] and s["num_iterations"] == so["num_iterations"]
    n = noise_from(case)
    if n is None:
        n = len(so["trace_cost"])
        assert s["num_successful_steps"] == so["num_successful_steps"] and s["num_unsuccessful_steps"] == so["num_unsuccessful_steps"]
        assert s["final_radius"] == pytest.approx(so["final_radius"], rel=1e-6)
    else:
        assert s["num_iterations"] == 80 and len(s["trace_cost"]) == 64 and s["num_successful_steps"] + s["num_unsuccessful_steps"] == 80
    assert len(s["trace_cost"]) == len(so["trace_cost"])
    assert list(s["trace_accepted"])[:n] == list(so["trace_accepted"])[:n]
    np.testing.assert_allclose(s["trace_radius"][:n], so["trace_radius"][:n], rtol=1e-6)
    np.testing.assert_allclose(s["trace_cost"][:n], so["trace_cost"][:n], rtol=1e-7)
    assert_states_close(out, po, 1e-6)
    if case in STATE_UNTOUCHED:  # no step was accepted: not a bit of the state may have moved
        for a, b in ((out.pts, start.pts), (out.cam_t, start.cam_t), (out.cam_quat, start.cam_quat)):
            assert a.tobytes() == b.tobytes()
    dead = FORMS[form][1]
    if dead is not None:
        # one set of level launches per decision launch that ran, and `dead` sets behind the end; a solve that ends at iteration 0 has
        # run one decision launch all the same
        assert counts[K_CHOL_LEVEL] == levels * (max(s["num_iterations"], 1) + dead), (counts, levels)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("form", CHAIN_FORMS)
def test_ending_in_the_launch_chain(form, case):
    check_case(form, case)


# ---- an initial point that cannot be evaluated ---------------------------------------------------------------------------------------------
def _rotation(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def bad_start(kind):
    p = scene("D")
    if kind == "nan_coordinate":
        p.pts[5, 1] = np.nan
    else:  # the landmark of the first depth prior, reflected through that camera's centre: depth -> -depth
        i, c = int(p.dobs_pt[0]), int(p.dobs_cam[0])
        centre = -_rotation(p.cam_quat[c]).T @ p.cam_t[c]
        p.pts[i] = 2.0 * centre - p.pts[i]
    return p


@functools.lru_cache(maxsize=None)
def oracle_refuses(kind):
    with pytest.raises(RuntimeError, match=f"failed with {MPSFM_ENUMERIC}"):
        O.solve(bad_start(kind))
    return True


def check_numeric_error(form, kind):
    assert oracle_refuses(kind)
    good, bad = scene("D"), bad_start(kind)
    env, _, hook = FORMS[form]
    o = capi.default_options(**(dict(allreduce=_HOOK, world_size=1, rank=0) if hook else {}))
    fresh_s, fresh, _, _, fresh_local = solve(form, good, {})
    again = good.copy()
    with _Env(env), capi.BAHandle(bad.copy(), o) as h:
        with pytest.raises(capi.MpsfmHipError) as e:
            h.solve()
        assert e.value.code == MPSFM_ENUMERIC
        h.set_state(good)
        s = h.solve()
        h.get_state(again)
        assert (local_iterations(h) >= 0) == (form == "single_launch") == (fresh_local >= 0)
    # the handle solves as a fresh one: the same decisions, numbers within what the order of the sweeps' atomic sums leaves open
    assert s["termination"] == fresh_s["termination"] and s["num_iterations"] == fresh_s["num_iterations"] >= 3
    assert list(s["trace_accepted"]) == list(fresh_s["trace_accepted"])
    np.testing.assert_allclose(s["trace_cost"], fresh_s["trace_cost"], rtol=1e-9)
    np.testing.assert_allclose(s["trace_radius"], fresh_s["trace_radius"], rtol=1e-6)
    assert_states_close(again, fresh, 1e-7)


@pytest.mark.parametrize("kind", ["nan_coordinate", "negative_depth"])
@pytest.mark.parametrize("form", CHAIN_FORMS)
def test_numeric_error_in_the_launch_chain(form, kind):
    check_numeric_error(form, kind)


# ---- the single-launch solver, last: its workgroups must agree on every ending, or they would wait for each other at a grid barrier --------
@pytest.mark.parametrize("case", list(CASES))
def test_ending_in_the_single_launch(case):
    check_case("single_launch", case)


@pytest.mark.parametrize("kind", ["nan_coordinate", "negative_depth"])
def test_numeric_error_in_the_single_launch(kind):
    check_numeric_error("single_launch", kind)
