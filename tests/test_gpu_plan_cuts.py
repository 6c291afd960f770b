"""A handle's camera order with and without the window-separator candidates (csrc/chol_plan.hip; MPSFM_CHOL_CUTS=0 turns them
off), on a closed orbit of 120 cameras that each share landmarks with the 6 next ones — a graph on which they win (10 -> 8
levels, test_chol_plan_cuts_cpu.py).  The scene is built the way level_entry_scenes.problem builds its orbits.

The handle's plan is held to the device-free plan of depth -3 (with the switch off: depth -2); the dense solution of the
handle's own reduced system to test_gpu_level_entry.py's bound against numpy.linalg.solve, rho <= C_RHO, with inverse
accumulators and with MPSFM_CHOL_INVERSE=0; and the level launches of a whole solve are counted: levels x iterations (the
split LM loop is forced, which leaves no dead iteration behind, see test_gpu_lm_split.py)."""

import functools

import numpy as np
import pytest

import chunk_cap_scenes as CC
import graph_scenes as G
import level_entry_scenes as LE
from mpsfm_amd import capi
from refined_solve import C_RHO, U
from test_gpu_level_entry import CHAIN, _Env
from test_gpu_lm_split import K_CHOL_LEVEL, launch_counts

pytestmark = pytest.mark.gpu

N, REACH = 120, 6
CUTS = {"cuts": {"MPSFM_CHOL_CUTS": None}, "no_cuts": {"MPSFM_CHOL_CUTS": "0"}}
DEPTH = {"cuts": -3, "no_cuts": -2}


@functools.lru_cache(maxsize=None)
def _ring():
    adj = G.ring_graph(N, REACH)
    ei, ej = np.nonzero(np.triu(adj, 1))
    # camera 0 is constant, node i is camera i + 1; two landmarks per edge, two per camera shared with camera 0 only
    tracks = [(int(a) + 1, int(b) + 1) for a, b in zip(ei, ej) for _ in range(2)] + [(0, i + 1) for i in range(N) for _ in range(2)]
    return adj, CC.scene(N + 1, tracks, seed=100 + N)


@functools.lru_cache(maxsize=None)
def _dense(cuts, inverse):
    """One handle: its plan, its reduced system after one sweep and the dense solution of it."""
    adj, prob = _ring()
    with _Env({**CUTS[cuts], "MPSFM_CHOL_INVERSE": None if inverse else "0"}), capi.BAHandle(prob.copy()) as h:
        plan = h.dense_plan()
        h.sweep_once(1e4)
        S, rhs = h.reduced_system()
        h.dense_solve_once()
        y = h.dense_solution()
    return plan, S, rhs, y


def _rho(S, rhs, y):
    """Forward error against numpy.linalg.solve over u times Skeel's condition number, as test_gpu_level_entry.py forms it."""
    ref = np.linalg.solve(S, rhs)
    scale = float(np.abs(ref).max())
    cond = float((np.abs(np.linalg.inv(S)) @ (np.abs(S) @ np.abs(ref) + np.abs(rhs))).max()) / scale
    return float(np.abs(y - ref).max()) / scale / (U * cond), cond


@pytest.mark.parametrize("inverse", [True, False], ids=["accumulators", "back_levels"])
@pytest.mark.parametrize("cuts", list(CUTS))
def test_the_handle_takes_the_plan_of_its_setting(cuts, inverse):
    adj, _ = _ring()
    plan = _dense(cuts, inverse)[0]
    P = LE.plan_with_heads(adj, depth=DEPTH[cuts], pinv_max_tiles=64 if inverse else 0)
    assert (plan["tile_columns"], plan["levels"], plan["work_items"], plan["tile_products"], plan["inverse_roles"]) == \
        (P["nt"], P["nlevels"], P["n_items"], P["products"], P["roles"])
    assert plan["inverse_accumulators"] == int(inverse) == P["use_pinv"] and plan["nd_depth"] == P["nd_depth"]
    if cuts == "cuts":
        assert plan["levels"] < _dense("no_cuts", inverse)[0]["levels"]


@pytest.mark.parametrize("inverse", [True, False], ids=["accumulators", "back_levels"])
@pytest.mark.parametrize("cuts", list(CUTS))
def test_the_dense_solution_meets_the_bound(cuts, inverse):
    plan, S, rhs, y = _dense(cuts, inverse)
    assert S.shape == (6 * N, 6 * N)
    rho, cond = _rho(S, rhs, y)
    print(f"RHO ring{N}/{REACH} {cuts} inverse={inverse} n={S.shape[0]} tiles={plan['tile_columns']} levels={plan['levels']} cond={cond:.3g} rho={rho:.3f}")
    assert np.isfinite(y).all()
    assert rho <= C_RHO


@pytest.mark.parametrize("cuts", list(CUTS))
def test_level_launches_are_levels_times_iterations(cuts):
    _, prob = _ring()
    with _Env({**CHAIN, **CUTS[cuts], "MPSFM_LM_SPLIT": "1", "MPSFM_LM_SPECULATE": None}), capi.BAHandle(prob.copy()) as h:
        levels = h.dense_plan()["levels"]
        s = h.solve()
        counts = launch_counts(h)
    assert s["num_iterations"] >= 2
    assert counts[K_CHOL_LEVEL] == levels * s["num_iterations"], (counts, levels, s["num_iterations"])
