"""The three forms of the track sweep (k_track_sweep_dense, k_track_sweep, k_long_track_sweep) and their update sweeps against the
CPU oracle on chunks built to sit on every cap of csrc/common.h: the scenes of tests/chunk_cap_scenes.py, whose shapes
tests/test_chunk_caps_cpu.py pins.  Every handle is created under the scene's environment.

Tolerances are the suite's own: cost rel 1e-12; S and rhs atol 1e-11 max|ref| for all-dense handles (test_gpu_ba.py) and
1e-10 max|ref| for handles with general chunks or long tracks (test_gpu_more.py); dense solve, full solve and point covariances
as test_gpu_ba.py / test_gpu_pt_handoff.py / test_gpu_more.py::test_point_covs_match_oracle.  The Jacobi scales inside S come from
the MODE_DIAG sweep over the same chunks, so the parity of S covers that sweep as well (mpsfm_point_covs has kernels of its own).

Measured on the MI355X, max |S - ref| / max|ref| over both radii: 1.9e-15 .. 3.8e-15 on the all-dense scenes, 2.5e-15 .. 6.0e-15 with
general chunks, 9.7e-15 on r252_253 (the 252-camera chunk's atomics and the long tracks); rhs 9.6e-16 .. 5.8e-15.  No bound had to
be derived from the oracle's own rounding.  Per scene: DESIGN.md §4a-3."""

import ctypes as C
import functools

import numpy as np
import pytest

import chunk_cap_scenes as CS
from build_table_cases import LOG_TABLES, environment, handle_tables, host_tables
from mpsfm_amd import capi
from oracle import cpu_oracle as O
from test_gpu_pt_handoff import SWITCHES, assert_matches_oracle, assert_same_solve

pytestmark = pytest.mark.gpu

NAMES = list(CS.SCENES)
RADII = (1e3, 3.0)


@functools.lru_cache(maxsize=None)
def oracle_systems(name):
    prob = CS.problem(name)
    return O.eval_cost(prob), {r: O.reduced_system(prob, radius=r) for r in RADII}


@functools.lru_cache(maxsize=None)
def oracle_solve(name):
    po = CS.problem(name)
    return O.solve(po), po


def blocks_nonzero(S):
    n = S.shape[0] // 6
    return (S.reshape(n, 6, n, 6) != 0.0).any(axis=(1, 3))


def local_iterations(h):
    """Iterations the handle's last solve ran inside the single launch; -1: the handle does not take that path."""
    L = capi.lib()
    clk = (C.c_int64 * 12)()
    return int(clk[6]) if L.mpsfm_debug_local_clocks(h._h, clk) else -1


def gpu_solve(name, monkeypatch, **env):
    """Resident solve of the scene under its environment and the given switches (name without MPSFM_ -> value); returns
    (summary, final problem, hands off?, iterations inside the single launch or -1)."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in {**CS.environment_of(name), **{"MPSFM_" + k: v for k, v in env.items()}}.items():
        monkeypatch.setenv(k, v)
    prob = CS.problem(name)
    out = prob.copy()
    with capi.BAHandle(prob) as h:
        s = h.solve()
        h.get_state(out)
        handoff, its = h.pt_handoff(), local_iterations(h)
    return s, out, handoff, its


@pytest.mark.parametrize("name", NAMES)
def test_reduced_system_block_by_block(name):
    (ocr, ocd), refs = oracle_systems(name)
    all_dense = name in CS.ALL_DENSE
    tol = 1e-11 if all_dense else 1e-10
    with environment(CS.environment_of(name)), capi.BAHandle(CS.problem(name)) as h:
        cr, cd = h.eval_cost()
        assert cr == pytest.approx(ocr, rel=1e-12) and cd == pytest.approx(ocd, rel=1e-12, abs=1e-12)
        for radius in RADII:
            ref = refs[radius]
            h.sweep_once(radius)
            parts = h.sweep_parts()
            S, rhs = h.reduced_system()
            s_scale, r_scale = np.abs(ref["S"]).max(), np.abs(ref["rhs"]).max()
            print(f"{name} radius {radius:g}: dense {parts['dense_chunks']} general {parts['general_chunks']} long {parts['long_tracks']} "
                  f"hand-off {int(h.pt_handoff())}; S err {np.abs(S - ref['S']).max() / s_scale:.3e} rhs err {np.abs(rhs - ref['rhs']).max() / r_scale:.3e}")
            assert (parts["general_chunks"] == 0 and parts["long_tracks"] == 0) == all_dense and parts["dense_chunks"] > 0
            assert (parts["long_tracks"] > 0) == (name == "r252_253")
            np.testing.assert_allclose(S, ref["S"], rtol=0, atol=tol * s_scale)
            np.testing.assert_allclose(rhs, ref["rhs"], rtol=0, atol=tol * r_scale)
            # a dropped or misrouted block that the global scale would hide
            np.testing.assert_array_equal(blocks_nonzero(S), blocks_nonzero(ref["S"]))
            h.dense_solve_once()
            y = h.dense_solution()
            y_np = np.linalg.solve(S, rhs)
            print(f"   y err vs numpy {np.abs(y - y_np).max() / np.abs(y_np).max():.3e} vs oracle {np.abs(y - ref['yc']).max() / np.abs(ref['yc']).max():.3e}")
            np.testing.assert_allclose(y, y_np, rtol=0, atol=1e-8 * np.abs(y_np).max())
            np.testing.assert_allclose(y, ref["yc"], rtol=0, atol=1e-7 * np.abs(ref["yc"]).max())


@pytest.mark.parametrize("name", NAMES)
def test_full_solve(name, monkeypatch):
    """Every form the scene's handle can take against the oracle: all-dense handles with and without the hand-off of the landmark
    factors, in the single launch (at most 16 variable cameras: all four all-dense scenes) and in the launch chain; the others in the
    launch chain, recomputing."""
    so, po = oracle_solve(name)
    assert so["termination"] == "function_tolerance" and so["num_iterations"] > 3
    if name not in CS.ALL_DENSE:
        sg, pg, handoff, its = gpu_solve(name, monkeypatch)
        assert not handoff and its == -1
        assert_matches_oracle(sg, pg, so, po)
        np.testing.assert_allclose(np.abs(np.sum(pg.cam_quat * po.cam_quat, axis=1)), 1.0, atol=1e-10)
        return
    for env in ({}, {"PT_HANDOFF": "0"}):
        sl, pl, handoff, its = gpu_solve(name, monkeypatch, **env)
        assert handoff and its == sl["num_iterations"]       # the flag says the buffer exists; PT_HANDOFF=0 recomputes per solve
        sc, pc, handoff, its = gpu_solve(name, monkeypatch, LOCAL_LM="0", **env)
        assert handoff and its == -1
        for s, p in ((sl, pl), (sc, pc)):
            assert_matches_oracle(s, p, so, po)
            np.testing.assert_allclose(np.abs(np.sum(p.cam_quat * po.cam_quat, axis=1)), 1.0, atol=1e-10)
            np.testing.assert_array_equal(p.pts[po.pt_const != 0], CS.problem(name).pts[po.pt_const != 0])
        assert_same_solve(sl, pl, sc, pc)


@pytest.mark.parametrize("name", NAMES)
def test_point_covs(name):
    """Tolerance of test_gpu_more.py::test_point_covs_match_oracle.  A landmark whose blocks all come from one camera (dup_aa's
    track (1, 1)) has a Hessian of rank 2: whether its last pivot comes out positive is rounding in either implementation
    (csrc/tri_kernels.hip), so those rows are left out."""
    prob = CS.problem(name)
    cams = [set() for _ in range(prob.n_pts)]
    for c, p in zip(prob.obs_cam.tolist(), prob.obs_pt.tolist()):
        cams[p].add(c)
    defined = np.array([len(c) >= 2 for c in cams])
    assert defined.sum() >= 150
    with environment(CS.environment_of(name)):
        c_g = capi.point_covs(prob)
    c_o = O.point_covs(prob)
    print(f"{name}: covs max rel err {np.nanmax(np.abs(c_g[defined] / c_o[defined] - 1.0)):.3e}")
    assert np.isfinite(c_o[defined]).all()
    np.testing.assert_allclose(c_g[defined], c_o[defined], rtol=1e-9, atol=1e-18)
    assert np.all(np.linalg.eigvalsh(c_g[defined]) > 0)


@pytest.mark.parametrize("name", NAMES)
def test_device_build_equals_host_build(name):
    """Where the handle says it was built on the device its tables are the host phases' bit for bit (rec_d / fx_d = log depth within 4
    spacings, tests/test_gpu_devbuild.py); a track of more than kObsMax blocks sends the build to the host."""
    with environment(CS.environment_of(name)):
        td = handle_tables(CS.problem(name))
        th = host_tables(CS.problem(name))
    on_device = int(td["built_on_device"][0])
    print(f"{name}: built on device {on_device}")
    assert on_device == (0 if name == "r252_253" else 1)
    for tname in th:
        if tname == "built_on_device":
            continue
        a, b = th[tname], td[tname]
        assert a.shape == b.shape, tname
        if tname in LOG_TABLES and on_device:
            assert np.all(np.abs(a - b) <= 4 * np.spacing(np.abs(a))), tname
        else:
            np.testing.assert_array_equal(a, b, err_msg=tname)
