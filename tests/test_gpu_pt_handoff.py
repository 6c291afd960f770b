"""The hand-off of the landmark factors from the dense track sweep to the update sweep of the same iteration (SweepArgs::pt_fac:
F = chol(V + D)^-1 and g_p per landmark) against the form that recomputes them (MPSFM_PT_HANDOFF=0) and against the CPU oracle, in
the launch chain and in the single launch, with the tolerances of test_gpu_ba.py::test_full_solve_matches_oracle."""

import ctypes as C
import dataclasses
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from mpsfm_amd import capi
from mpsfm_amd.synthetic import CX, CY, FX, FY, R_from_quat, make_scene
from oracle import cpu_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("MPSFM_PT_HANDOFF", "MPSFM_FUSE_PROLOGUE", "MPSFM_LOCAL_LM")


def gpu_solve(prob, monkeypatch, options=None, **env):
    """Resident solve with the given switches (name without MPSFM_ -> value); returns (summary, final problem, hands off?, single launch?)."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv("MPSFM_" + k, v)
    out = prob.copy()
    L = capi.lib()
    with capi.BAHandle(prob.copy(), options=options) as h:
        s = h.solve()
        h.get_state(out)
        handoff = h.pt_handoff()
        local = bool(L.mpsfm_debug_local_clocks(h._h, (C.c_int64 * 12)()))
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return s, out, handoff, local


def assert_matches_oracle(sg, pg, so, po):
    assert sg["num_iterations"] == so["num_iterations"]
    assert sg["termination"] == so["termination"]
    assert list(sg["trace_accepted"]) == list(so["trace_accepted"])
    n = min(len(sg["trace_cost"]), len(so["trace_cost"]))
    err = np.abs(np.asarray(sg["trace_cost"][:n]) / np.asarray(so["trace_cost"][:n]) - 1.0).max()
    print(f"trace_cost max rel err {err:.3e}, pts max abs err {np.abs(pg.pts - po.pts).max():.3e}")
    np.testing.assert_allclose(sg["trace_cost"][:n], so["trace_cost"][:n], rtol=1e-9)
    np.testing.assert_allclose(pg.pts, po.pts, atol=1e-6)
    np.testing.assert_allclose(pg.cam_t, po.cam_t, atol=1e-6)


def assert_same_solve(sa, pa, sb, pb, rtol=1e-10):
    """tests/test_gpu_local_lm.py's comparison of the single launch with the chain."""
    assert sa["termination"] == sb["termination"]
    assert sa["num_iterations"] == sb["num_iterations"]
    assert sa["num_successful_steps"] == sb["num_successful_steps"]
    assert sa["initial_cost"] == pytest.approx(sb["initial_cost"], rel=1e-13)
    assert sa["final_cost"] == pytest.approx(sb["final_cost"], rel=rtol)
    np.testing.assert_allclose(sa["trace_cost"], sb["trace_cost"], rtol=rtol)
    np.testing.assert_allclose(sa["trace_radius"], sb["trace_radius"], rtol=1e-6)
    assert list(sa["trace_accepted"]) == list(sb["trace_accepted"])
    np.testing.assert_allclose(pa.pts, pb.pts, atol=1e-9)
    np.testing.assert_allclose(pa.cam_t, pb.cam_t, atol=1e-9)
    np.testing.assert_allclose(np.abs(np.sum(pa.cam_quat * pb.cam_quat, axis=1)), 1.0, atol=1e-12)


def oracle_solve(prob, **opts):
    po = prob.copy()
    return O.solve(po, O.default_options(**opts)) if opts else O.solve(po), po


# ---- the problems: built once, their oracle solves shared ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_scene():
    """21 cameras (the first is the gauge: 20 variable ones, beyond the single launch), 1 500 landmarks with depth priors."""
    prob = make_scene(21, 1500, True, seed=5)[0]
    return prob, oracle_solve(prob)


def constant_scenes():
    """The problems of test_constant_points_and_fixed_cost and test_fix_pose_point_refinement (tests/test_gpu_ba.py)."""
    a = make_scene(8, 500, True, seed=3)[0]
    a.pose_const[:3] = 1
    a.pt_const[::3] = 1
    b = make_scene(6, 300, True, seed=2)[0]
    b.pose_const[:] = 1
    b.gauge_axis_cam = -1
    b.depth_loss_type = 0
    return a, b


@functools.lru_cache(maxsize=None)
def rejected_scene():
    """tests/test_gpu_local_lm.py::test_rejected_steps_and_the_iteration_limit's problem and options."""
    prob = make_scene(8, 1200, False, seed=13)[0]
    rng = np.random.default_rng(3)
    prob.pts += rng.normal(0, 0.3, prob.pts.shape)
    q = prob.cam_quat[1:] + rng.normal(0, 0.25, prob.cam_quat[1:].shape)
    prob.cam_quat[1:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    kw = dict(initial_trust_region_radius=1e16, max_num_iterations=15)
    return prob, kw, oracle_solve(prob, **kw)


@functools.lru_cache(maxsize=None)
def split_scene():
    """Landmarks with 2 and with 12 records side by side: 12-camera tracks, every other landmark cut down to its first two cameras."""
    prob = make_scene(21, 1200, True, seed=9, max_track=12, track_mean=40.0)[0]
    short = np.arange(prob.n_pts) % 2 == 1

    def keep(pt):  # the first two blocks of a short landmark, every block of the others
        order = np.argsort(pt, kind="stable")
        rank = np.empty(len(pt), np.int64)
        start = np.searchsorted(pt[order], pt[order], side="left")
        rank[order] = np.arange(len(pt)) - start
        return ~short[pt] | (rank < 2)

    ko = keep(prob.obs_pt)
    kd = np.isin(prob.dobs_cam.astype(np.int64) * prob.n_pts + prob.dobs_pt, prob.obs_cam[ko].astype(np.int64) * prob.n_pts + prob.obs_pt[ko])
    prob = dataclasses.replace(prob, obs_cam=prob.obs_cam[ko], obs_pt=prob.obs_pt[ko], obs_xy=prob.obs_xy[ko], dobs_cam=prob.dobs_cam[kd],
                               dobs_pt=prob.dobs_pt[kd], dobs_depth=prob.dobs_depth[kd], dobs_magnitude=prob.dobs_magnitude[kd],
                               dobs_param=prob.dobs_param[kd])
    counts = np.bincount(prob.obs_pt, minlength=prob.n_pts)
    assert (counts[short] == 2).all() and (counts[~short] == 12).mean() > 0.9, np.bincount(counts)
    return prob, oracle_solve(prob)


@functools.lru_cache(maxsize=None)
def long_track_scene():
    """chain_scene with landmark 0 seen by more than 16 cameras: its chunk is a general one."""
    prob = chain_scene()[0].copy()
    Xc = np.einsum("nij,j->ni", R_from_quat(prob.cam_quat), prob.pts[0]) + prob.cam_t
    have = set(prob.obs_cam[prob.obs_pt == 0].tolist())
    add = np.array([c for c in range(prob.n_cams) if c not in have and Xc[c, 2] > 0.5], np.int32)
    assert len(have) + len(add) > 16
    xy = np.stack([FX * Xc[add, 0] / Xc[add, 2] + CX, FY * Xc[add, 1] / Xc[add, 2] + CY], axis=1) + 0.5
    prob = dataclasses.replace(prob, obs_cam=np.concatenate([prob.obs_cam, add]), obs_pt=np.concatenate([prob.obs_pt, np.zeros(len(add), np.int32)]),
                               obs_xy=np.concatenate([prob.obs_xy, xy]))
    return prob, oracle_solve(prob)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse_prologue", ["1", "0"])
def test_chain_both_forms_match_the_oracle(fuse_prologue, monkeypatch):
    """Launch chain: hand-off and recompute form each against the oracle, and the same decisions in both; also where the adoption of the
    accepted candidate is a launch of its own (MPSFM_FUSE_PROLOGUE=0)."""
    prob, (so, po) = chain_scene()
    sh, ph, handoff, local = gpu_solve(prob, monkeypatch, FUSE_PROLOGUE=fuse_prologue)
    assert handoff and not local
    sr, pr, _, _ = gpu_solve(prob, monkeypatch, FUSE_PROLOGUE=fuse_prologue, PT_HANDOFF="0")
    assert_matches_oracle(sh, ph, so, po)
    assert_matches_oracle(sr, pr, so, po)
    assert sh["num_iterations"] == sr["num_iterations"] and list(sh["trace_accepted"]) == list(sr["trace_accepted"])


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
def check_constant_scenes(solve):
    """solve(prob, **switches) -> (summary, final problem); shared with the poisoned subprocess (tests/_pt_handoff_worker.py)."""
    a, b = constant_scenes()
    (soa, poa), (sob, pob) = oracle_solve(a), oracle_solve(b)
    for env in ({}, {"LOCAL_LM": "0"}, {"LOCAL_LM": "0", "PT_HANDOFF": "0"}):
        sg, pg = solve(a, **env)
        assert soa["fixed_cost"] > 0 and sg["fixed_cost"] == pytest.approx(soa["fixed_cost"], rel=1e-12)
        assert_matches_oracle(sg, pg, soa, poa)
        np.testing.assert_array_equal(pg.pts[::3], a.pts[::3])
        np.testing.assert_array_equal(pg.cam_quat[:3], a.cam_quat[:3])
        sg, pg = solve(b, **env)
        assert sg["reduced_dim"] == 0
        assert_matches_oracle(sg, pg, sob, pob)
        np.testing.assert_array_equal(pg.cam_quat, b.cam_quat)


def test_constant_landmarks_and_cameras(monkeypatch):
    check_constant_scenes(lambda prob, **env: gpu_solve(prob, monkeypatch, **env)[:2])


def test_constant_landmarks_and_cameras_on_poisoned_blocks():
    """A constant landmark's slot of the hand-off buffer is never written: nothing of it may reach the result."""
    env = dict(os.environ, MPSFM_POISON="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_pt_handoff_worker.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_rejected_step_rewrites_the_buffer(monkeypatch):
    """After a rejection the next track sweep runs at the same state with the new radius and rewrites the buffer: the trace equals the
    oracle's through the rejections."""
    prob, kw, (so, po) = rejected_scene()
    assert so["trace_accepted"].count(0) >= 3, "the scene is meant to produce rejected steps"
    sg, pg, handoff, local = gpu_solve(prob, monkeypatch, capi.default_options(**kw), LOCAL_LM="0")
    assert handoff and not local
    assert_matches_oracle(sg, pg, so, po)
    sr, pr, _, _ = gpu_solve(prob, monkeypatch, capi.default_options(**kw), LOCAL_LM="0", PT_HANDOFF="0")
    assert list(sr["trace_accepted"]) == list(sg["trace_accepted"])


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_landmarks_split_across_rows_and_waves(monkeypatch):
    """Runs of 2 and of 12 records: they start and end inside a 16-lane row, cross rows and cross the 64-lane boundary."""
    prob, (so, po) = split_scene()
    sg, pg, handoff, local = gpu_solve(prob, monkeypatch)
    assert handoff and not local
    assert_matches_oracle(sg, pg, so, po)
    sr, pr, _, _ = gpu_solve(prob, monkeypatch, PT_HANDOFF="0")
    assert_matches_oracle(sr, pr, so, po)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncam,npts", [(12, 4000), (3, 300)])
def test_single_launch_follows(ncam, npts, monkeypatch):
    """The single launch routes the same nine doubles from phase A to phase D: it equals the chain in either form."""
    prob = make_scene(ncam, npts, True, seed=5)[0]
    for env in ({}, {"PT_HANDOFF": "0"}):
        sc, pc, handoff, local = gpu_solve(prob, monkeypatch, LOCAL_LM="0", **env)
        assert handoff and not local
        sl, pl, handoff, local = gpu_solve(prob, monkeypatch, **env)
        assert handoff and local and sl["num_iterations"] > 3
        assert_same_solve(sl, pl, sc, pc)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_handle_with_a_general_chunk_recomputes(monkeypatch):
    prob, (so, po) = long_track_scene()
    sg, pg, handoff, local = gpu_solve(prob, monkeypatch)
    assert not handoff and not local
    assert_matches_oracle(sg, pg, so, po)
