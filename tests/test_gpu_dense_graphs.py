"""The dense reduced-camera solve (dense_chol.hip, chol_plan.hip, run_dense in ba_solver.hip) on camera graphs and sizes
that no make_scene orbit reaches: every factorisation path (level schedule, per-step skyline, outer panels with the 2 x 2
tile update and the second-stream look-ahead) and every substitution path (inverse accumulators, back levels, groups of
four tile rows), each selected through the handle's own switches and each PROVEN selected through dense_plan().

Per case and radius (1e4: the first LM iteration, kappa_2 ~ 1e10 from the damped gauge direction; 1e-1: heavy damping):
  (a) dense_plan() shows the path under test;
  (b) y is finite and rho(y) <= C against the refined reference of the S and rhs the handle itself returned
      (refined_solve.py: fp64 Cholesky + refinement with a long-double residual; rho = forward error / (u * Skeel cond));
  (c) S and rhs equal the oracle's block-wise at 1e-11, blocks the oracle leaves exactly zero are exactly zero.
Nothing is compared bitwise between runs or paths: k_inv_y accumulates with atomics.

C = 8 x the largest rho of three fp64 NumPy solvers on the same systems (test_dense_graphs_cpu.py measures them and holds
the NumPy rows below to their committed literals).  Largest rho over all cases and both radii, NumPy rows on
the oracle's S, device rows on the handle's S:

  solver / path family                          largest rho   at
  NumPy LU (np.linalg.solve)                        8.23       complete343, radius 1e-1
  NumPy Cholesky (cho_solve)                        5.37       path90, radius 1e4
  NumPy plan interpreter, accumulators              6.99       path90, radius 1e4
  NumPy plan interpreter, back levels               6.99       path90, radius 1e4
  C = 8 x 8.23                                     65.84
  MI355X levels + accumulators (k_inv_y)           13.3        grid144, radius 1e-1        (radius 1e4: 0.97, star70 skyline)
  MI355X levels + back levels (k_back_level)       13.8        grid144, radius 1e-1        (radius 1e4: 0.35, grid144)
  MI355X per-step skyline / outer panels           20.2        complete343 NB=7, 1e-1      (radius 1e4: 0.68, complete2)
  largest eta on the MI355X 2.2e-15 (complete343); last correction of the reference at most 5e-20 |y| on every case.
Per case: DESIGN.md 4a-2.
"""

import functools

import numpy as np
import pytest

import graph_scenes as G
from mpsfm_amd import capi
from oracle import cpu_oracle as O
from refined_solve import C_RHO, Reference

pytestmark = pytest.mark.gpu

RADII = (1e4, 1e-1)

ENV = {
    "default": {},
    "back_levels": {"MPSFM_CHOL_INVERSE": "0"},
    "per_step": {"MPSFM_CHOL_LEVEL": "0"},
    "skyline": {"MPSFM_CHOL_GRAPH": "0"},
    "no_overlap": {"MPSFM_CHOL_OVERLAP": "0"},
    "no_big_update": {"MPSFM_CHOL_BIG": "0"},
    "panels_of_3": {"MPSFM_CHOL_NB": "3"},
    "panels_of_7": {"MPSFM_CHOL_NB": "7"},
}
# tile columns of the complete graphs: no padding (one dense chain, nothing to dissect).  1..5 are all there; 16 cameras are
# 96 = 3 * 32 columns exactly; 16 | 17 is the single-launch solver's limit; 4 and 5 tile columns cross the group of four tile
# rows of k_backsub_group (t0 == 0 | t0 > 0)
TILE_COLUMNS = {1: 1, 2: 1, 5: 1, 6: 2, 16: 3, 17: 4, 21: 4, 22: 5}
assert set(TILE_COLUMNS.values()) == {1, 2, 3, 4, 5} and all(v == (6 * k + 31) // 32 for k, v in TILE_COLUMNS.items())


def _groups(nt):  # launches of the substitution in groups of four tile rows (k_z_init + k_backsub_group)
    return (nt + 3) // 4 + 1


@functools.lru_cache(maxsize=4)
def _oracle(name, radius):
    return O.reduced_system(G.case(name)[1], radius=radius)


_refs = {}


def _reference(name, radius, S, rhs):
    """The refined reference of (S, rhs); kept per case and radius while the handle returns the same numbers (the sweep does
    not depend on the dense-solve switches), so that the inverse of a 2000 x 2000 system is formed once."""
    hit = _refs.get((name, radius))
    if hit is None or not (np.array_equal(hit.S, S) and np.array_equal(hit.rhs, rhs)):
        for k in [k for k in _refs if k[0] != name]:
            del _refs[k]
        hit = _refs[(name, radius)] = Reference(S, rhs)
    return hit


def _assert_same_system(S, rhs, ref):
    n = S.shape[0]
    nb = n // 6
    assert ref["S"].shape == (n, n) and n == 6 * nb
    blocks = lambda M: np.abs(M).reshape(nb, 6, nb, 6)
    scale = np.abs(ref["S"]).max()
    diff = blocks(S - ref["S"]).max(axis=(1, 3))
    rowmax = blocks(ref["S"]).max(axis=(1, 2, 3))
    assert (diff <= 1e-11 * rowmax[:, None] + 1e-14 * scale).all(), float((diff / rowmax[:, None]).max())
    np.testing.assert_allclose(rhs, ref["rhs"], rtol=0, atol=1e-11 * np.abs(ref["rhs"]).max())
    zero_ref = blocks(ref["S"]).max(axis=(1, 3)) == 0
    assert (blocks(S).max(axis=(1, 3))[zero_ref] == 0).all(), "a block the oracle leaves exactly zero is not zero"
    return float(zero_ref.mean())


def _run(name, variant, monkeypatch, check_plan):
    adj, prob = G.case(name)
    for k, v in ENV[variant].items():
        monkeypatch.setenv(k, v)
    with capi.BAHandle(prob.copy()) as h:
        assert h.reduced_dim == 6 * adj.shape[0]
        plan = h.dense_plan()
        assert plan["slots"] == adj.shape[0] and plan["tile_columns"] >= (6 * plan["slots"] + 31) // 32
        check_plan(plan)
        for radius in RADII:
            h.sweep_once(radius)
            S, rhs = h.reduced_system()
            h.dense_solve_once()
            y = h.dense_solution()
            zeros = _assert_same_system(S, rhs, _oracle(name, radius))
            ref = _reference(name, radius, S, rhs)
            rho, eta = ref.rho(y), ref.eta(y)
            print(f"RHO {name} {variant} radius={radius:g} n={S.shape[0]} tiles={plan['tile_columns']} levels={plan['levels']} "
                  f"pinv={plan['inverse_accumulators']} s_blocks={plan['s_blocks']} zero_blocks={zeros:.3f} cond={ref.cond:.3g} "
                  f"stall={ref.stall:.1e} rho={rho:.3f} eta={eta:.2e}")
            assert np.isfinite(y).all()
            assert rho <= C_RHO, (rho, C_RHO)


# ---- tile edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["default", "per_step"])
@pytest.mark.parametrize("n", list(TILE_COLUMNS))
def test_tile_edges(n, variant, monkeypatch):
    nt = TILE_COLUMNS[n]

    def check(plan):
        assert plan["tile_columns"] == nt and plan["levels"] == nt  # a complete graph is one chain
        if variant == "default":
            assert plan["inverse_accumulators"] == 1 and plan["backsub_launches"] == 1  # k_chol_level, then k_inv_y
        else:
            assert plan["inverse_accumulators"] == 0 and plan["backsub_launches"] == _groups(nt)  # k_chol_step, k_backsub_group

    _run(f"complete{n}", variant, monkeypatch, check)


# ---- graph kinds, at most 64 tile columns -----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["default", "back_levels", "per_step"])
@pytest.mark.parametrize("name", list(G.KINDS))
def test_graph_kinds(name, variant, monkeypatch):
    def check(plan):
        nt = plan["tile_columns"]
        assert nt <= 64
        if variant == "per_step":
            assert plan["levels"] == nt and plan["inverse_accumulators"] == 0 and plan["backsub_launches"] == _groups(nt)
            return
        assert plan["work_items"] > 0 and 1 <= plan["levels"] <= nt
        if variant == "default":
            assert plan["inverse_accumulators"] == 1 and plan["inverse_roles"] > 0 and plan["backsub_launches"] == 1
        else:  # k_back_level: one launch per level
            assert plan["inverse_accumulators"] == 0 and plan["inverse_roles"] == 0 and plan["backsub_launches"] == plan["levels"]
        if name == "two_rings60":
            assert plan["levels"] < nt  # two chains advance in the same launches
        if name == "complete40":
            assert plan["levels"] == nt  # nothing to gain: one dense chain, whatever the order

    _run(name, variant, monkeypatch, check)


@pytest.mark.parametrize("name", ["star70", "star70_hub_last"])
def test_stars_without_the_camera_graph(name, monkeypatch):
    """The skyline of the caller's order: full when the hub comes first (every camera reaches back to slot 0), nearly empty
    when it comes last."""
    def check(plan):
        assert plan["nd_depth"] == -1 and plan["tile_columns"] == (6 * plan["slots"] + 31) // 32
        assert plan["inverse_accumulators"] == 1
        if name == "star70":
            assert plan["s_blocks"] == 70 * 71 // 2 and plan["levels"] == plan["tile_columns"]

    _run(name, "skyline", monkeypatch, check)


@pytest.mark.parametrize("name", list(G.KINDS))
def test_graph_kinds_full_solve(name):
    prob = G.case(name)[1]
    sg, so = capi.ba_solve(prob.copy()), O.solve(prob.copy())
    assert sg["num_iterations"] == so["num_iterations"] and sg["termination"] == so["termination"]
    assert sg["trace_accepted"] == so["trace_accepted"]
    np.testing.assert_allclose(sg["trace_cost"], so["trace_cost"], rtol=1e-9)


# ---- more than 64 tile columns, structured: k_back_level by default ------------------------------------------------------------
@pytest.mark.parametrize("name,variant", [("ring343_links", "default"), ("grid19x19", "default"), ("ring343_links", "per_step")])
def test_large_structured(name, variant, monkeypatch):
    def check(plan):
        nt = plan["tile_columns"]
        assert nt > 64 and plan["inverse_accumulators"] == 0
        if variant == "default":
            assert plan["levels"] < nt and plan["backsub_launches"] == plan["levels"]
        else:  # the skyline in outer panels of 8 tile columns
            assert plan["levels"] == nt and plan["backsub_launches"] == _groups(nt)

    _run(name, variant, monkeypatch, check)


# ---- more than 64 tile columns without structure: the handle leaves the level schedule by itself ------------------------------
@pytest.mark.parametrize("name,variant", [("complete343", "default"), ("complete343", "no_overlap"), ("complete343", "no_big_update"),
                                          ("complete343", "panels_of_3"), ("complete343", "panels_of_7"), ("complete348", "default")])
def test_large_dense_outer_panels(name, variant, monkeypatch):
    def check(plan):
        nt = plan["tile_columns"]
        # 65 tile columns are nine panels of 8: the ring of four events wraps twice; 66 gives k_big_update's 2 x 2 blocks the
        # other parity of tile rows
        assert nt == {"complete343": 65, "complete348": 66}[name]
        assert plan["levels"] == nt and plan["inverse_accumulators"] == 0 and plan["backsub_launches"] == _groups(nt)
        assert plan["tile_products"] > 0.5 * nt ** 3 / 6  # why the handle took the outer panels

    _run(name, variant, monkeypatch, check)
