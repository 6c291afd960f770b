"""A handle on a camera graph where the dissection to a given chain (csrc/chol_plan.hip: refit) decides the plan: an orbit of 120
cameras that each share landmarks with the 10 next ones.  The legacy order has 12 levels, the greedy window-separator tree 10,
the refitted one 9 (tests/test_chol_plan_balance_cpu.py holds the device-free plan of the same graph to that).  Here the handle's
plan is the device-free one, the level launches solve a random system of that block pattern to test_gpu_dense_graphs.py's bound
(rho <= C_RHO against the refined reference of refined_solve.py) with the inverse accumulators and with the back levels, and a
full solve follows the CPU oracle (test_gpu_pt_handoff.py: assert_matches_oracle)."""

import functools

import numpy as np
import pytest

import graph_scenes as G
from chol_plan_interp import _plan
from mpsfm_amd import capi
from refined_solve import C_RHO, Reference
from test_chol_plan_balance_cpu import PARENT
from test_gpu_pt_handoff import assert_matches_oracle, oracle_solve

pytestmark = pytest.mark.gpu

N, REACH = 120, 10


@functools.lru_cache(maxsize=None)
def _scene():
    adj = G.ring_graph(N, REACH)
    return adj, G.graph_scene(adj, per_edge=2, seed=N)


@functools.lru_cache(maxsize=None)
def _system():
    """A random SPD system with the block pattern of the graph in the caller's camera order, its right-hand side and its refined
    reference (formed once)."""
    adj, _ = _scene()
    rng = np.random.default_rng(14)
    n = 6 * N
    S = np.zeros((n, n))
    for i, j in zip(*np.nonzero(np.triu(adj, 1))):
        B = 0.3 * rng.standard_normal((6, 6))
        S[6 * i:6 * i + 6, 6 * j:6 * j + 6] = B
        S[6 * j:6 * j + 6, 6 * i:6 * i + 6] = B.T
    for i in range(N):
        B = rng.standard_normal((6, 6))
        S[6 * i:6 * i + 6, 6 * i:6 * i + 6] = 0.5 * (B + B.T)
    S[np.diag_indices(n)] = 0.0
    S[np.diag_indices(n)] = np.abs(S).sum(1) + 1.0
    rhs = rng.standard_normal(n)
    return S, rhs, Reference(S, rhs)


@pytest.mark.parametrize("inverse", [True, False])
def test_plan_and_level_launches(inverse, monkeypatch):
    adj, prob = _scene()
    if not inverse:
        monkeypatch.setenv("MPSFM_CHOL_INVERSE", "0")
    P = _plan(adj, depth=-3, pinv_max_tiles=64 if inverse else 0)
    assert P["nlevels"] <= PARENT[N, REACH] and P["nlevels"] <= _plan(adj, depth=-2)["nlevels"] - 2  # the search engages
    S, rhs, ref = _system()
    with capi.BAHandle(prob.copy()) as h:
        plan = h.dense_plan()
        print(f"ring {N}/{REACH} inverse={inverse}: handle levels={plan['levels']} tiles={plan['tile_columns']} items={plan['work_items']} "
              f"products={plan['tile_products']} | device-free levels={P['nlevels']} tiles={P['nt']}")
        assert plan["slots"] == N
        assert (plan["levels"], plan["tile_columns"], plan["work_items"], plan["tile_products"]) == (P["nlevels"], P["nt"], P["n_items"], P["products"])
        assert plan["inverse_accumulators"] == int(inverse)
        h.sweep_once(1e4)
        assert not h.dense_solve_given(S, rhs)
        y = h.dense_solution()
    rho = ref.rho(y)
    print(f"RHO ring {N}/{REACH} inverse={inverse} n={S.shape[0]} cond={ref.cond:.3g} rho={rho:.3f} eta={ref.eta(y):.2e}")
    assert np.isfinite(y).all()
    assert rho <= C_RHO, (rho, C_RHO)


def test_full_solve_matches_oracle():
    _, prob = _scene()
    pg = prob.copy()
    sg = capi.ba_solve(pg)
    so, po = oracle_solve(prob)
    assert sg["num_iterations"] >= 2
    assert_matches_oracle(sg, pg, so, po)
