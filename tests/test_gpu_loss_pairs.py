"""Whole solves and cost evaluation under all nine (reprojection loss, depth loss) pairs on the scene of tests/loss_pair_scenes.py,
whose robust weights run from 1 down to 1e-3 on either residual kind (tests/test_lm_step_cpu.py asserts that).  The single-launch
solver (k_local_lm) runs the update sweep's body with the camera rows in LDS and cannot be stopped after one step, so what
tests/test_gpu_update_once.py pins step by step for the launch chain is compared here through solves: in the single launch and in the
chain (MPSFM_LOCAL_LM=0), each with and without the hand-off of the landmark factors (MPSFM_PT_HANDOFF=0), against the CPU oracle
(test_gpu_pt_handoff.assert_matches_oracle, and trace_radius rtol 1e-6, which that helper leaves out) and against each other
(assert_same_solve); once more with max_num_iterations=1 from a radius at which the step is accepted, landmarks and cameras at atol
1e-9; eval_cost (k_cost_records) rel 1e-12, also with fixed records (two more constant cameras, every third landmark constant)."""

import functools

import numpy as np
import pytest

import loss_pair_scenes as LP
from mpsfm_amd import capi
from oracle import cpu_oracle as O
from test_gpu_pt_handoff import assert_matches_oracle, assert_same_solve, gpu_solve, oracle_solve

pytestmark = pytest.mark.gpu

PAIR_IDS = [f"{r}-{d}" for r, d in LP.PAIRS]


@functools.lru_cache(maxsize=None)
def oracle_of(reproj, depth, **opts):
    return oracle_solve(LP.problem(reproj, depth), **opts)


@pytest.mark.parametrize("reproj,depth", LP.PAIRS, ids=PAIR_IDS)
def test_full_solve(reproj, depth, monkeypatch):
    so, po = oracle_of(reproj, depth)
    assert so["num_iterations"] >= 10
    prob = LP.problem(reproj, depth)
    solves = {}
    for local in (True, False):
        for handoff in (True, False):
            env = {} if local else {"LOCAL_LM": "0"}
            if not handoff:
                env["PT_HANDOFF"] = "0"
            sg, pg, has_buffer, was_local = gpu_solve(prob, monkeypatch, **env)
            assert has_buffer and was_local == local
            print(f"{reproj}/{depth} {'single launch' if local else 'chain'} {'hand-off' if handoff else 'recompute'}: {sg['num_iterations']} iterations, "
                  f"final cost {sg['final_cost']:.9g} (oracle {so['final_cost']:.9g})")
            assert_matches_oracle(sg, pg, so, po)
            n = min(len(sg["trace_radius"]), len(so["trace_radius"]))
            assert n == len(so["trace_radius"])
            np.testing.assert_allclose(sg["trace_radius"][:n], so["trace_radius"][:n], rtol=1e-6)
            np.testing.assert_allclose(np.abs(np.sum(pg.cam_quat * po.cam_quat, axis=1)), 1.0, atol=1e-10)
            solves[(local, handoff)] = (sg, pg)
    first = solves[(True, True)]
    for key, other in solves.items():
        if key != (True, True):
            assert_same_solve(*first, *other)


@pytest.mark.parametrize("reproj,depth", LP.PAIRS, ids=PAIR_IDS)
def test_one_iteration(reproj, depth, monkeypatch):
    """One ACCEPTED iteration from the same start: nothing has contracted an error of the step yet.  Under the trivial reprojection loss
    the gross observations make the model poor at the default radius 1e4 and the oracle rejects the first three steps; those pairs
    start from radius 100, where the first step is accepted.  The step must be accepted and move a landmark by more than one unit (the
    oracle moves them by 4.5, 2.6 and 12 units under the trivial, soft-L1 and Cauchy reprojection loss), so that the comparison at atol
    1e-9 is never one of the start state with itself."""
    opts = dict(max_num_iterations=1)
    if reproj == "trivial":
        opts["initial_trust_region_radius"] = 100.0
    so, po = oracle_of(reproj, depth, **opts)
    prob = LP.problem(reproj, depth)
    moved = np.abs(po.pts - prob.pts).max()
    assert list(so["trace_accepted"]) == [1, 1] and moved > 1.0 and np.abs(po.cam_t - prob.cam_t).max() > 0.05
    for env in ({}, {"LOCAL_LM": "0"}):
        sg, pg, _, was_local = gpu_solve(prob, monkeypatch, options=capi.default_options(**opts), **env)
        assert was_local == (not env)
        assert sg["num_iterations"] == so["num_iterations"] == 1 and sg["termination"] == so["termination"]
        assert list(sg["trace_accepted"]) == [1, 1]
        assert np.abs(pg.pts - prob.pts).max() > 1.0
        print(f"{reproj}/{depth} {'chain' if env else 'single launch'}: landmarks moved by up to {moved:.3g}, max |pts - oracle| {np.abs(pg.pts - po.pts).max():.3e}, "
              f"max |cam_t - oracle| {np.abs(pg.cam_t - po.cam_t).max():.3e}")
        np.testing.assert_allclose(pg.pts, po.pts, rtol=0, atol=1e-9)
        np.testing.assert_allclose(pg.cam_t, po.cam_t, rtol=0, atol=1e-9)
        np.testing.assert_allclose(pg.cam_quat, po.cam_quat, rtol=0, atol=1e-9)


@pytest.mark.parametrize("fixed", [False, True], ids=["all-variable", "fixed-records"])
def test_eval_cost(fixed):
    for reproj, depth in LP.PAIRS:
        prob = LP.problem(reproj, depth, fixed=fixed)
        ocr, ocd = O.eval_cost(prob)
        with capi.BAHandle(prob.copy()) as h:
            cr, cd = h.eval_cost()
            if fixed:
                nfixed = capi.lib().mpsfm_debug_table(h._h, 11, None, 0) // 4
                assert nfixed > 100  # blocks of a constant camera and a constant landmark: the fx_* records
        print(f"{reproj}/{depth} fixed {fixed}: reprojection {cr:.12g} (rel {abs(cr / ocr - 1):.1e}) depth {cd:.12g} (rel {abs(cd / ocd - 1):.1e})")
        assert cr == pytest.approx(ocr, rel=1e-12) and cd == pytest.approx(ocd, rel=1e-12)
