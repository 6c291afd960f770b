"""The entry of the two sweeps (csrc/sweep_dense_body.h, sweep_update_body.h; k_track_sweep_dense and k_update_sweep): the control
block, the chunk header and the chunk's records are requested in batches, `term` is tested behind the requests, the candidate rows
of the fused camera update are formed by the last lanes of the workgroup beside the landmark loads.  Nothing of that changes a
number, so every test here is a comparison with the CPU oracle on the chunk shapes and solve histories where a hoisted load could
go wrong: a chunk with fewer records than one wave, a chunk of exactly kObsMax records, a short last chunk, no depth blocks, sweeps
at `pts` after a rejection and at `pts2` after an acceptance, the iteration queued ahead of the end of a solve, and the candidate
poses of the fused update.

Tolerances are the suite's own for the same quantities: cost rel 1e-12, S and rhs 1e-11 max|ref| (test_gpu_ba.py, all-dense handles),
iteration counts and accepted flags exact, cost trace rel 1e-9, state 1e-7."""

import dataclasses
import functools

import numpy as np
import pytest

import chunk_cap_scenes as CS
from build_table_cases import environment, handle_tables
from mpsfm_amd import capi
from mpsfm_amd.synthetic import FX, FY, CX, CY, make_scene
from oracle import cpu_oracle as O
from test_gpu_chunk_caps import blocks_nonzero, local_iterations, oracle_systems

pytestmark = pytest.mark.gpu

SWITCHES = ("MPSFM_FUSE_PROLOGUE", "MPSFM_FUSE_CAM", "MPSFM_PT_HANDOFF", "MPSFM_LM_SPECULATE")
ALL_SWITCHES = SWITCHES + ("MPSFM_LOCAL_LM",)
RADII = (1e3, 3.0)


def env_of(base=None, **switches):
    """Environment of a handle: every switch unset except the given ones (name without MPSFM_ -> value)."""
    e = {k: None for k in ALL_SWITCHES}
    e.update(base or {})
    e.update({"MPSFM_" + k: v for k, v in switches.items()})
    return e


def gpu_solve(prob, env, options=None):
    """(summary, final problem, iterations inside the single launch or -1) of a resident solve under `env`."""
    out = prob.copy()
    with environment(env), capi.BAHandle(prob.copy(), options=options) as h:
        s = h.solve()
        h.get_state(out)
        its = local_iterations(h)
    return s, out, its


def oracle_solve(prob, **opts):
    po = prob.copy()
    return (O.solve(po, O.default_options(**opts)) if opts else O.solve(po)), po


def assert_solve_matches(sg, pg, so, po):
    assert sg["termination"] == so["termination"]
    assert sg["num_iterations"] == so["num_iterations"]
    assert list(sg["trace_accepted"]) == list(so["trace_accepted"])
    assert sg["initial_cost"] == pytest.approx(so["initial_cost"], rel=1e-12)
    n = min(len(sg["trace_cost"]), len(so["trace_cost"]))
    assert n > 0
    err = np.abs(np.asarray(sg["trace_cost"][:n]) / np.asarray(so["trace_cost"][:n]) - 1.0).max()
    print(f"trace_cost max rel err {err:.3e}, pts max abs err {np.abs(pg.pts - po.pts).max():.3e}, t {np.abs(pg.cam_t - po.cam_t).max():.3e}")
    np.testing.assert_allclose(sg["trace_cost"][:n], so["trace_cost"][:n], rtol=1e-9)
    np.testing.assert_allclose(pg.pts, po.pts, atol=1e-7)
    np.testing.assert_allclose(pg.cam_t, po.cam_t, atol=1e-7)
    np.testing.assert_allclose(np.abs(np.sum(pg.cam_quat * po.cam_quat, axis=1)), 1.0, atol=1e-10)


def assert_system_matches(prob, env, refs, cost_ref, want_shape):
    """sweep_once (no control block: the radius comes with the arguments) against the oracle's reduced system at both radii."""
    with environment(env):
        shape = CS.shapes(handle_tables(prob))
        print("dense chunks (nrec, npt, ncam, nent):", shape["dense"])
        assert not shape["general"] and not shape["long"]
        want_shape([r[0] for r in shape["dense"]])
        with capi.BAHandle(prob.copy()) as h:
            cr, cd = h.eval_cost()
            assert cr == pytest.approx(cost_ref[0], rel=1e-12) and cd == pytest.approx(cost_ref[1], rel=1e-12, abs=1e-12)
            for radius in RADII:
                ref = refs[radius]
                h.sweep_once(radius)
                S, rhs = h.reduced_system()
                s_scale, r_scale = np.abs(ref["S"]).max(), np.abs(ref["rhs"]).max()
                print(f"radius {radius:g}: S err {np.abs(S - ref['S']).max() / s_scale:.3e} rhs err {np.abs(rhs - ref['rhs']).max() / r_scale:.3e}")
                np.testing.assert_allclose(S, ref["S"], rtol=0, atol=1e-11 * s_scale)
                np.testing.assert_allclose(rhs, ref["rhs"], rtol=0, atol=1e-11 * r_scale)
                np.testing.assert_array_equal(blocks_nonzero(S), blocks_nonzero(ref["S"]))


def systems_of(prob):
    return O.eval_cost(prob), {r: O.reduced_system(prob, radius=r) for r in RADII}


# ---- the problems: built once, their oracle results shared -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def short_scene():
    """One chunk of 36 records (3 cameras, the first constant; 12 landmarks seen by all): waves 1 to 3 hold no record."""
    prob = CS.scene(3, [(0, 1, 2)] * 12, seed=41)
    return prob, systems_of(prob), oracle_solve(prob)


@functools.lru_cache(maxsize=None)
def reproj_scene():
    prob = make_scene(8, 600, False, seed=4)[0]
    assert len(prob.dobs_cam) == 0
    return prob, systems_of(prob), oracle_solve(prob)


REJECT_OPTS = dict(initial_trust_region_radius=1e16, max_num_iterations=15)


@functools.lru_cache(maxsize=None)
def adoption_scene():
    """21 cameras (20 variable: the launch chain), 1 500 landmarks with depth priors, perturbed so far and started at so large a radius
    that the oracle's own history holds accepted and rejected steps."""
    prob = make_scene(21, 1500, True, seed=5)[0]
    rng = np.random.default_rng(5)
    prob.pts += rng.normal(0, 0.3, prob.pts.shape)
    q = prob.cam_quat[1:] + rng.normal(0, 0.25, prob.cam_quat[1:].shape)
    prob.cam_quat[1:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return prob, oracle_solve(prob, **REJECT_OPTS)


@functools.lru_cache(maxsize=None)
def chain_scene():
    prob = make_scene(21, 1500, True, seed=5)[0]
    return prob


@functools.lru_cache(maxsize=None)
def queued_oracle(key):
    opts = {"one": dict(max_num_iterations=1), "two": dict(max_num_iterations=2), "tolerance": {}}[key]
    return opts, oracle_solve(chain_scene(), **opts)


def fused_scenes():
    """Constant cameras among the variable ones (shared intrinsics, as make_scene builds them), and two intrinsics rows of
    different values dealt to the cameras alternately."""
    a = make_scene(21, 1200, True, seed=11)[0]
    a.pose_const[[0, 4, 9]] = 1
    b = make_scene(21, 1200, True, seed=12)[0]
    b = dataclasses.replace(b, cam_intr=np.array([[FX, FY, CX, CY], [1.01 * FX, 0.99 * FY, CX + 3.0, CY - 2.0]]),
                            cam_intr_idx=(np.arange(b.n_cams) % 2).astype(np.int32))
    return {"constant_cameras": a, "two_intrinsics": b}


# ---- 1: short chunk -----------------------------------------------------------------------------------------------------------------------
def test_short_chunk_reduced_system():
    prob, (cost, refs), _ = short_scene()

    def one_short(nrecs):
        assert len(nrecs) == 1 and nrecs[0] < 64

    assert_system_matches(prob, env_of(), refs, cost, one_short)


@pytest.mark.parametrize("local", ["0", "1"])
def test_short_chunk_solve(local):
    """Through a solve: in the launch chain the control block is read on the device; the single launch shares the bodies."""
    prob, _, (so, po) = short_scene()
    sg, pg, its = gpu_solve(prob, env_of(LOCAL_LM=local))
    assert (its == -1) == (local == "0")
    assert_solve_matches(sg, pg, so, po)


# ---- 2: full chunk, short last chunk ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed16", "two_view"])
def test_full_and_last_chunk(name):
    cost, refs = oracle_systems(name)

    def shape(nrecs):
        if name == "mixed16":
            assert max(nrecs) == 252 and nrecs.count(252) >= 1
        assert nrecs[-1] < max(nrecs)  # the last chunk's records end where the arrays end

    assert_system_matches(CS.problem(name), env_of(CS.environment_of(name)), refs, cost, shape)


# ---- 3: no depth blocks --------------------------------------------------------------------------------------------------------------------
def test_reprojection_only():
    prob, (cost, refs), (so, po) = reproj_scene()
    assert cost[1] == 0.0
    assert_system_matches(prob, env_of(), refs, cost, lambda nrecs: None)
    sg, pg, its = gpu_solve(prob, env_of(LOCAL_LM="0"))
    assert its == -1
    assert_solve_matches(sg, pg, so, po)


# ---- 4: both adoption branches ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [None] + [s[len("MPSFM_"):] for s in SWITCHES])
def test_solve_through_rejections_and_acceptances(off):
    prob, (so, po) = adoption_scene()
    acc = list(so["trace_accepted"])[1:]
    assert acc.count(0) >= 1 and acc.count(1) >= 1, acc   # the sweep runs at `pts` after a rejection and at `pts2` after an acceptance
    sg, pg, its = gpu_solve(prob, env_of(**({off: "0"} if off else {})), capi.default_options(**REJECT_OPTS))
    assert its == -1
    assert_solve_matches(sg, pg, so, po)


# ---- 5: the iteration queued ahead ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("speculate", ["1", "0"])
@pytest.mark.parametrize("key", ["one", "two", "tolerance"])
def test_iteration_queued_ahead(key, speculate):
    """The kernels of the iteration that was queued before the end of the solve was known leave no trace: the state is the oracle's,
    and a second solve from the reset state repeats the first."""
    opts, (so, po) = queued_oracle(key)
    assert so["termination"] == ("function_tolerance" if key == "tolerance" else "max_iterations")
    prob = chain_scene()
    out1, out2 = prob.copy(), prob.copy()
    with environment(env_of(LM_SPECULATE=speculate)), capi.BAHandle(prob.copy(), options=capi.default_options(**opts)) as h:
        s1 = h.solve()
        h.get_state(out1)
        assert local_iterations(h) == -1
        h.reset_state()
        s2 = h.solve()
        h.get_state(out2)
    assert_solve_matches(s1, out1, so, po)
    assert s2["termination"] == s1["termination"] and s2["num_iterations"] == s1["num_iterations"]
    assert list(s2["trace_accepted"]) == list(s1["trace_accepted"])
    np.testing.assert_allclose(s2["trace_cost"], s1["trace_cost"], rtol=1e-9)
    np.testing.assert_allclose(out2.pts, out1.pts, atol=1e-7)
    np.testing.assert_allclose(out2.cam_t, out1.cam_t, atol=1e-7)
    np.testing.assert_allclose(np.abs(np.sum(out2.cam_quat * out1.cam_quat, axis=1)), 1.0, atol=1e-10)


# ---- 6: fused candidate rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["constant_cameras", "two_intrinsics"])
def test_fused_candidate_rows(name):
    """One accepted iteration with the camera update fused into the update sweep: the state read back is the candidate workgroup 0
    wrote (q2, t2), the final cost is the candidate cost the update sweep summed from ITS rows in LDS.  Both equal the oracle's after
    its first step, and the cost of the state read back, evaluated by a kernel of its own from the table built from q2 and t2, is that
    candidate cost: the rows every workgroup formed are the poses workgroup 0 wrote."""
    prob = fused_scenes()[name]
    opts = dict(max_num_iterations=1)
    so, po = oracle_solve(prob, **opts)
    assert list(so["trace_accepted"])[1:] == [1]
    out = prob.copy()
    with environment(env_of(FUSE_CAM="1")), capi.BAHandle(prob.copy(), options=capi.default_options(**opts)) as h:
        sg = h.solve()
        h.get_state(out)
        assert local_iterations(h) == -1
        cr, cd = h.eval_cost()
    assert_solve_matches(sg, out, so, po)
    np.testing.assert_allclose(out.cam_quat * np.sign(np.sum(out.cam_quat * po.cam_quat, axis=1))[:, None], po.cam_quat, atol=1e-7)
    if name == "constant_cameras":
        np.testing.assert_array_equal(out.cam_quat[[0, 4, 9]], prob.cam_quat[[0, 4, 9]])
        np.testing.assert_array_equal(out.cam_t[[0, 4, 9]], prob.cam_t[[0, 4, 9]])
    # the candidate cost of the update sweep against the oracle's at the same step, and against the cost of the state it became
    # (the oracle's final cost is the sum of its two cost parts to 4e-16)
    assert sg["final_cost"] == pytest.approx(so["final_cost"], rel=1e-9)
    assert sg["trace_cost"][-1] == pytest.approx(so["trace_cost"][-1], rel=1e-9)
    print(f"candidate cost {sg['final_cost']!r}, cost of the state read back {cr + cd!r}")
    assert cr + cd == pytest.approx(sg["final_cost"], rel=1e-12)
