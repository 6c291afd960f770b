"""The stacked panel factorisation of the dense solve by four waves (stacked_panel_wg, csrc/dense_tile.h) against the one-wave
path (stacked_panel), through the probe mpsfm_debug_panel_factor (one workgroup, the device function both k_chol_level and
k_chol_step call) and through whole solves under both settings of MPSFM_CHOL_PANEL_WAVES.

Probe inputs, the stacked 64 x 32 matrix [D; X]:
  (a) D = B B^T + 32 I of a seeded 32 x 32 B, X random;
  (b) the same D, X = I (the workgroup that owns the diagonal tile: X L^-T = L^-T);
  (c) D with kappa_2 = 1e10 (the smallest eigenvalue of (a) scaled down, as the damped gauge direction does at radius 1e4);
  (d) four matrices: D of (a) with one diagonal entry lowered so that the pivot of column 3, 12, 20 or 29 turns negative — one
      column of every wave.

Every element receives the same operations with the same operands in the same order in both paths, so on (a)-(c) the lower
triangle of L and all of X L^-T are equal as 64-bit patterns.

Backward errors (largest entry of |D - L L^T| / (|L| |L^T|) and of |X - Xh L^T| / (|Xh| |L^T|), residuals in long double):
                                                       factor      solve
  MI355X, one wave (= four waves, bitwise)   (a)   5.6413e-16  4.5503e-16
                                             (b)   5.6413e-16  2.7884e-16
                                             (c)   4.2595e-16  4.4875e-16
  numpy.linalg.cholesky + solve_triangular   (a)   2.5309e-16  3.9119e-16
                                             (b)   2.5309e-16  1.9091e-16
                                             (c)   2.5619e-16  3.3166e-16
  BACKWARD_BOUND = 2 x 5.6413e-16, the largest one-wave figure.  (Theory allows gamma_33 = 33 u = 3.7e-15 for 32 columns.)
"""

import functools

import numpy as np
import pytest

import graph_scenes as G
from mpsfm_amd import capi
from refined_solve import C_RHO, Reference

BACKWARD_BOUND = 2 * 5.6413e-16  # twice what the one-wave path needs on these inputs (measured, see above)
BAD_COLUMNS = (3, 12, 20, 29)
WAVES_ENV = "MPSFM_CHOL_PANEL_WAVES"


@functools.lru_cache(maxsize=None)
def _base():
    rng = np.random.default_rng(20240404)
    B = rng.standard_normal((32, 32))
    D = B @ B.T + 32.0 * np.eye(32)
    return 0.5 * (D + D.T), rng.standard_normal((32, 32))


@functools.lru_cache(maxsize=None)
def panel_input(name):
    """The stacked [D; X] of a named input; D symmetric with both triangles stored."""
    D, X = _base()
    if name == "a":
        pass
    elif name == "b":
        X = np.eye(32)
    elif name == "c":
        w, V = np.linalg.eigh(D)
        w = w.copy()
        w[0] = w[-1] * 1e-10
        D = (V * w) @ V.T
        D = 0.5 * (D + D.T)
        assert 0.5e10 < np.linalg.cond(D) < 2e10
    elif name.startswith("d"):
        j = int(name[1:])
        L = np.linalg.cholesky(D)
        pivot = D[j, j] - L[j, :j] @ L[j, :j]
        assert pivot > 0
        D = D.copy()
        D[j, j] -= 1.5 * pivot  # the pivot of column j becomes -pivot / 2
    else:
        raise KeyError(name)
    out = np.ascontiguousarray(np.vstack([D, X]))
    out.setflags(write=False)
    return out


def backward_errors(dx, L, Xh):
    """Largest componentwise backward errors of the factor and of the solve; a zero denominator asks for a zero residual."""
    D, X = dx[:32].astype(np.longdouble), dx[32:].astype(np.longdouble)
    Ll, Xl = L.astype(np.longdouble), Xh.astype(np.longdouble)
    worst = []
    for num, den in ((np.abs(D - Ll @ Ll.T), np.abs(Ll) @ np.abs(Ll.T)), (np.abs(X - Xl @ Ll.T), np.abs(Xl) @ np.abs(Ll.T))):
        assert (num[den == 0] == 0).all()
        worst.append(float((num[den > 0] / den[den > 0]).max()))
    return tuple(worst)


@functools.lru_cache(maxsize=None)
def _probe(name, waves):
    out, ok = capi.debug_panel_factor(panel_input(name), waves)
    out.setflags(write=False)
    return out, ok


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_probe_paths_agree_bitwise(name):
    (o1, ok1), (o4, ok4) = _probe(name, 1), _probe(name, 4)
    assert ok1 and ok4
    low = np.tril(np.ones((32, 32), bool))
    assert np.array_equal(o1[:32][low].view(np.uint64), o4[:32][low].view(np.uint64))
    assert np.array_equal(o1[32:].view(np.uint64), o4[32:].view(np.uint64))
    assert np.isfinite(o4[:32][low]).all() and np.isfinite(o4[32:]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("j", BAD_COLUMNS)
def test_probe_bad_pivot_is_reported_by_its_wave(j):
    assert not _probe(f"d{j}", 1)[1]
    assert not _probe(f"d{j}", 4)[1]


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_probe_backward_error(name, waves):
    out, ok = _probe(name, waves)
    assert ok
    e_fac, e_sol = backward_errors(panel_input(name), np.tril(out[:32]), out[32:])
    print(f"BACKWARD {name} waves={waves} factor={e_fac:.3e} solve={e_sol:.3e}")
    assert e_fac <= BACKWARD_BOUND and e_sol <= BACKWARD_BOUND, (e_fac, e_sol)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_numpy_stays_below_the_bound(name):
    """The literal is not tailored to the device: LAPACK's factor and triangular solve of the same inputs stay below it."""
    from scipy.linalg import solve_triangular

    dx = panel_input(name)
    L = np.linalg.cholesky(dx[:32])
    Xh = solve_triangular(L, dx[32:].T, lower=True).T
    e_fac, e_sol = backward_errors(dx, L, Xh)
    print(f"BACKWARD {name} numpy factor={e_fac:.3e} solve={e_sol:.3e}")
    assert e_fac <= BACKWARD_BOUND and e_sol <= BACKWARD_BOUND, (e_fac, e_sol)


# ---- whole solves under both settings of the switch ------------------------------------------------------------------------------
RADII = (1e4, 1e-1)
VARIANTS = {
    "default": {},
    "back_levels": {"MPSFM_CHOL_INVERSE": "0"},
    "per_step": {"MPSFM_CHOL_LEVEL": "0"},     # k_chol_step
    "panels_of_3": {"MPSFM_CHOL_NB": "3"},     # k_chol_step in outer panels
}
_refs = {}


def _reference(name, radius, S, rhs):
    hit = _refs.get((name, radius))
    if hit is None or not (np.array_equal(hit.S, S) and np.array_equal(hit.rhs, rhs)):
        hit = _refs[(name, radius)] = Reference(S, rhs)
    return hit


def _solve(name, variant, waves, monkeypatch):
    prob = G.case(name)[1]
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    if waves is None:
        monkeypatch.delenv(WAVES_ENV, raising=False)
    else:
        monkeypatch.setenv(WAVES_ENV, waves)
    with capi.BAHandle(prob.copy()) as h:
        plan = h.dense_plan()
        for radius in RADII:
            h.sweep_once(radius)
            S, rhs = h.reduced_system()
            h.dense_solve_once()
            y = h.dense_solution()
            rho = _reference(name, radius, S, rhs).rho(y)
            print(f"RHO {name} {variant} waves={waves} radius={radius:g} n={S.shape[0]} tiles={plan['tile_columns']} rho={rho:.3f}")
            assert np.isfinite(y).all()
            assert rho <= C_RHO, (rho, C_RHO)
    return plan


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ["complete2", "complete6", "complete22", "path90"])
def test_solve_under_both_settings(name, variant, monkeypatch):
    plan4 = _solve(name, variant, None, monkeypatch)
    plan1 = _solve(name, variant, "1", monkeypatch)
    assert plan1 == plan4
    if name.startswith("complete"):
        assert plan4["tile_columns"] == {"complete2": 1, "complete6": 2, "complete22": 5}[name]
