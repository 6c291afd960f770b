"""The host enqueues the front half of iteration i + 1 (sweeps, slab reduction) ahead of the news about iteration i and the back
half (dense solve ... decision) only once that news says "go on" (solve_impl, csrc/ba_solver.hip; MPSFM_LM_SPLIT=1 forces it,
=0 forces the whole iteration ahead, MPSFM_LM_SPECULATE=0 enqueues nothing ahead).  The three settings run the same kernels on
the same data in the same order, so they must agree in everything a solve reports; what differs is how many launches the end of
a solve leaves dead, which the handle's launch counter (code 34 of mpsfm_debug_table) shows.

Scene: 24 cameras, 2 000 landmarks on the launch chain, every chunk dense."""

import ctypes as C
import functools

import numpy as np
import pytest

from mpsfm_amd import capi
from mpsfm_amd.abi import ALLREDUCE_FN
from mpsfm_amd.synthetic import make_scene
from test_gpu_level_entry import CHAIN, _Env

pytestmark = pytest.mark.gpu

K_CHOL_LEVEL = 3  # LaunchFamily of csrc/ba_launch.h


def launch_counts(h):
    """Code 34 of mpsfm_debug_table: the launches the handle's last solve enqueued, per kernel family."""
    v = (C.c_int64 * 9)()
    assert capi.lib().mpsfm_debug_table(h._h, 34, v, C.sizeof(v)) == C.sizeof(v)
    return [int(x) for x in v]

SETTINGS = {"split": {"MPSFM_LM_SPLIT": "1", "MPSFM_LM_SPECULATE": None}, "whole": {"MPSFM_LM_SPLIT": "0", "MPSFM_LM_SPECULATE": None},
            "no_speculation": {"MPSFM_LM_SPLIT": None, "MPSFM_LM_SPECULATE": "0"}}
ENDINGS = {"tolerance": {}, "one_iteration": {"max_num_iterations": 1}, "two_iterations": {"max_num_iterations": 2},
           "rejected_steps": {"initial_trust_region_radius": 1e16, "max_num_iterations": 15}}


def _scene(ending="tolerance"):
    prob = make_scene(24, 2000, True, seed=11)[0]
    if ending == "rejected_steps":  # far from the optimum under a huge initial radius, as test_gpu_local_lm.py provokes rejections
        rng = np.random.default_rng(3)
        prob.pts += rng.normal(0, 1.0, prob.pts.shape)
        q = prob.cam_quat[1:] + rng.normal(0, 0.5, prob.cam_quat[1:].shape)
        prob.cam_quat[1:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return prob


@functools.lru_cache(maxsize=None)
def _solves(ending, setting):
    """Two solves on one handle from the same state: [(summary, cam_t, cam_quat, pts, launch counts, levels)] * 2."""
    prob = _scene(ending)
    out = []
    with _Env({**CHAIN, **SETTINGS[setting]}), capi.BAHandle(prob, capi.default_options(**ENDINGS[ending])) as h:
        assert h.pt_handoff(), "every chunk dense, no long track"
        levels = h.dense_plan()["levels"]
        for _ in range(2):
            h.reset_state()
            s = h.solve()
            h.get_state()
            out.append((s, prob.cam_t.copy(), prob.cam_quat.copy(), prob.pts.copy(), launch_counts(h), levels))
    return out


@pytest.mark.parametrize("ending", list(ENDINGS))
def test_endings_are_what_they_are_named_for(ending):
    s = _solves(ending, "whole")[0][0]
    print(f"ENDING {ending}: {s['num_iterations']} iterations, {s['termination']}, {s['num_unsuccessful_steps']} unsuccessful")
    if ending == "tolerance":
        assert s["termination"] in ("function_tolerance", "gradient_tolerance", "parameter_tolerance") and s["num_iterations"] >= 3
    elif ending == "one_iteration":
        assert s["num_iterations"] == 1 and s["termination"] == "max_iterations"
    elif ending == "two_iterations":
        assert s["num_iterations"] == 2 and s["termination"] == "max_iterations"
    else:
        assert list(s["trace_accepted"]).count(0) >= 3 and s["num_successful_steps"] >= 1, "the scene is meant to produce rejected steps"


@pytest.mark.parametrize("second", [False, True], ids=["first_solve", "second_solve"])
@pytest.mark.parametrize("setting", ["split", "no_speculation"])
@pytest.mark.parametrize("ending", list(ENDINGS))
def test_settings_agree(ending, setting, second):
    (sa, ta, qa, pa, _, _), (sb, tb, qb, pb, _, _) = _solves(ending, "whole")[int(second)], _solves(ending, setting)[int(second)]
    assert sa["num_iterations"] == sb["num_iterations"] and sa["termination"] == sb["termination"]
    assert list(sa["trace_accepted"]) == list(sb["trace_accepted"])
    np.testing.assert_allclose(sa["trace_cost"], sb["trace_cost"], rtol=1e-9)
    np.testing.assert_allclose(ta, tb, atol=1e-7)
    np.testing.assert_allclose(qa, qb, atol=1e-7)
    np.testing.assert_allclose(pa, pb, atol=1e-7)


@pytest.mark.parametrize("second", [False, True], ids=["first_solve", "second_solve"])
@pytest.mark.parametrize("ending", list(ENDINGS))
def test_level_launches_follow_the_setting(ending, second):
    for setting, dead in (("split", 0), ("whole", 1), ("no_speculation", 0)):
        s, _, _, _, counts, levels = _solves(ending, setting)[int(second)]
        assert counts[K_CHOL_LEVEL] == levels * (s["num_iterations"] + dead), (setting, counts, levels, s["num_iterations"])


def test_a_sharded_handle_ignores_the_forced_split():
    hook = ALLREDUCE_FN(lambda user, buf, count, on_device, stream: 0)  # one rank: the sum is what is there
    prob = _scene()
    with _Env({**CHAIN, **SETTINGS["split"]}), capi.BAHandle(prob, capi.default_options(allreduce=hook, world_size=1, rank=0)) as h:
        levels = h.dense_plan()["levels"]
        s = h.solve()
        counts = launch_counts(h)
    ref = _solves("tolerance", "whole")[0][0]
    assert s["num_iterations"] == ref["num_iterations"] and s["termination"] == ref["termination"]
    assert counts[K_CHOL_LEVEL] == levels * (s["num_iterations"] + 1)
