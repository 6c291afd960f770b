"""The single-launch solver (csrc/local_lm.hip) with one workgroup held back at a phase point (mpsfm_debug_local_skew) while the others
run ahead as far as the grid barriers let them.  Every workgroup takes the trust-region decision itself, so the solve is right only if
every buffer one workgroup reads was ordered after the other workgroups' writes by a barrier or by iteration parity:
a skewed solve must still equal the launch chain (MPSFM_LOCAL_LM=0) and the CPU oracle."""

import ctypes as C

import numpy as np
import pytest

from mpsfm_amd import capi
from mpsfm_amd.synthetic import local_window, make_scene
from oracle import cpu_oracle as O
from test_gpu_local_lm import assert_same_solve

pytestmark = pytest.mark.gpu

POINTS = {"P": 1, "A": 2, "B": 4, "D": 8, "E": 16}  # after barrier 0, track sweep, after barrier 1, update sweep, after barrier 2
TICKS = 30000  # 300 us of the 100 MHz wall clock: longer than a whole iteration of the other workgroups (at most ~85 us)
MAX_TICKS = 200000
SHAPES = [(3, 300, True), (7, 900, False), (12, 4000, True), (16, 6000, True)]  # one, two and three tile columns; ~24 chunks and more


def set_skew(chunk, mask, ticks) -> int:
    L = capi.lib()
    return L.mpsfm_debug_local_skew(chunk, mask, ticks)


@pytest.fixture
def skew():
    """Arms the hook; it is process-wide, so whatever the test does, it is off again afterwards."""

    def arm(chunk, mask, ticks):
        assert set_skew(chunk, mask, ticks) == 0, (chunk, mask, ticks)

    yield arm
    assert set_skew(0, 0, 0) == 0


def local_clocks(h):
    """The phase clocks of the handle's last single-launch solve: [6] iterations, [11] ticks the skew hook waited; None: the chain."""
    L = capi.lib()
    clk = (C.c_int64 * 12)()
    return [int(x) for x in clk] if L.mpsfm_debug_local_clocks(h._h, clk) else None


def dense_chunks(h) -> int:
    L = capi.lib()
    info = (C.c_int64 * 4)()
    assert L.mpsfm_ba_sweep_parts(h._h, None, info) == 0
    return int(info[0])


def solve_local(prob, options=None, arm=None):
    """(summary, state, clocks) of a solve on a new handle (MPSFM_LOCAL_LM unset: the caller's monkeypatch cleared it); arm(chunks)
    runs between the handle's creation and the launch, which reads the hook."""
    out = prob.copy()
    with capi.BAHandle(prob.copy(), options=options) as h:
        if arm is not None:
            arm(dense_chunks(h))
        s = h.solve()
        h.get_state(out)
        return s, out, local_clocks(h)


def solve_chain(prob, options=None):
    out = prob.copy()
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MPSFM_LOCAL_LM", "0")
        with capi.BAHandle(prob.copy(), options=options) as h:
            s = h.solve()
            h.get_state(out)
            assert local_clocks(h) is None
    return s, out


def skew_arm(skew, which, point, ticks=TICKS):
    """Holds back the first, a middle or the last workgroup (the last one counted from the end: the kernel reduces modulo the grid)."""
    return lambda nchunks: skew({"first": 0, "middle": nchunks // 2, "last": -1}[which], POINTS[point], ticks)


def assert_waited(clk, point, ticks):
    """The hook really held the workgroup back: the wait covers every pass through the point (the prologue's P: one)."""
    passes = 1 if point == "P" else clk[6]
    assert clk[11] >= ticks * passes, (clk[11], ticks, passes)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"{s[0]}cams-{s[1]}pts{'' if s[2] else '-nodepth'}")
def reference(request):
    """The problem of a shape, its launch-chain solve and its oracle solve: computed once for every skew of the shape."""
    ncam, npts, depth = request.param
    prob = make_scene(ncam, npts, depth, seed=5)[0]
    sc, pc = solve_chain(prob)
    po = prob.copy()
    so = O.solve(po)
    return prob, (sc, pc), (so, po)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("point", list(POINTS))
@pytest.mark.parametrize("which", ["first", "middle", "last"])
def test_skewed_single_launch_equals_the_chain_and_the_oracle(reference, which, point, skew, monkeypatch):
    monkeypatch.delenv("MPSFM_LOCAL_LM", raising=False)
    prob, (sc, pc), (so, po) = reference
    sl, pl, clk = solve_local(prob, arm=skew_arm(skew, which, point))
    assert clk is not None and clk[6] == sl["num_iterations"] > 3
    assert_waited(clk, point, TICKS)
    assert_same_solve(sl, pl, sc, pc)
    # (the tolerances of test_single_launch_solve_equals_the_oracle)
    assert sl["initial_cost"] == pytest.approx(so["initial_cost"], rel=1e-12)
    assert sl["final_cost"] == pytest.approx(so["final_cost"], rel=1e-8)
    assert sl["num_iterations"] == so["num_iterations"] and sl["termination"] == so["termination"]
    n = min(len(sl["trace_cost"]), len(so["trace_cost"]))
    np.testing.assert_allclose(sl["trace_cost"][:n], so["trace_cost"][:n], rtol=1e-9)
    np.testing.assert_allclose(pl.pts, po.pts, atol=1e-6)
    np.testing.assert_allclose(pl.cam_t, po.cam_t, atol=1e-6)


def rejecting_problem():
    """test_rejected_steps_and_the_iteration_limit's start: far from the optimum, a huge initial radius."""
    prob = make_scene(8, 1200, False, seed=13)[0]
    rng = np.random.default_rng(3)
    prob.pts += rng.normal(0, 0.3, prob.pts.shape)
    q = prob.cam_quat[1:] + rng.normal(0, 0.25, prob.cam_quat[1:].shape)
    prob.cam_quat[1:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return prob


@pytest.mark.timeout(300)
@pytest.mark.parametrize("which", ["first", "middle", "last"])
def test_rejected_steps_and_the_iteration_limit_under_skew(which, skew, monkeypatch):
    """Rejections, radius cuts and the iteration limit: each one a decision every workgroup must take alike."""
    monkeypatch.delenv("MPSFM_LOCAL_LM", raising=False)
    prob = rejecting_problem()
    for o, rtol in ((capi.default_options(initial_trust_region_radius=1e16, max_num_iterations=15), 1e-8),
                    (capi.default_options(max_num_iterations=0), 1e-9), (capi.default_options(max_num_iterations=1), 1e-9)):
        sc, pc = solve_chain(prob, o)
        sl, pl, clk = solve_local(prob, o, arm=skew_arm(skew, which, "E"))
        assert clk is not None and clk[6] >= max(sl["num_iterations"], 1)  # (a limit of 0: one pass, ended by its decision)
        assert_waited(clk, "E", TICKS)
        assert_same_solve(sl, pl, sc, pc, rtol=rtol)
        if o.max_num_iterations == 15:
            assert clk[6] == sl["num_iterations"]
            assert list(sl["trace_accepted"]).count(0) >= 3, "the scene is meant to produce rejected steps"


@pytest.mark.timeout(300)
@pytest.mark.parametrize("which", ["first", "middle", "last"])
def test_local_window_under_skew(which, skew, monkeypatch):
    """Optimizer.ba(mode='local')'s problem: constant cameras outside the window, constant landmarks, fixed blocks."""
    monkeypatch.delenv("MPSFM_LOCAL_LM", raising=False)
    base = make_scene(40, 9000, True, seed=6)[0]
    loc = local_window(base, window_cams=[10, 11, 12, 13, 14, 15], ref_cam=15)[0]
    sc, pc = solve_chain(loc)
    sl, pl, clk = solve_local(loc, arm=skew_arm(skew, which, "E"))
    assert clk is not None and clk[6] == sl["num_iterations"]
    assert_waited(clk, "E", TICKS)
    assert_same_solve(sl, pl, sc, pc)
    np.testing.assert_array_equal(pl.cam_quat[loc.pose_const != 0], loc.cam_quat[loc.pose_const != 0])
    np.testing.assert_array_equal(pl.pts[loc.pt_const != 0], loc.pts[loc.pt_const != 0])


@pytest.mark.timeout(300)
def test_hook_off_is_a_no_op(skew, monkeypatch):
    """After a skewed solve and a reset, a solve on a new handle waits nowhere and takes the decisions of a solve before the hook was
    touched.  (Bit equality is not the bar: the reduced system is summed with device-scope atomics in arrival order.)"""
    monkeypatch.delenv("MPSFM_LOCAL_LM", raising=False)
    prob = make_scene(12, 4000, True, seed=5)[0]
    s0, p0, c0 = solve_local(prob)
    assert c0 is not None and c0[11] == 0 and c0[6] > 3
    skew(-1, sum(POINTS.values()), TICKS)
    s1, p1, c1 = solve_local(prob)
    assert c1[11] >= TICKS * (4 * c1[6] + 1)  # P once, A B D E every iteration
    assert_same_solve(s1, p1, s0, p0)
    skew(0, 0, 0)
    s2, p2, c2 = solve_local(prob)
    assert c2[11] == 0 and c2[6] == s2["num_iterations"]
    assert_same_solve(s2, p2, s0, p0)
    np.testing.assert_allclose(s2["trace_cost"], s0["trace_cost"], rtol=1e-12)
    # an armed mask with zero ticks is off as well
    skew(0, sum(POINTS.values()), 0)
    s3, p3, c3 = solve_local(prob)
    assert c3[11] == 0
    assert_same_solve(s3, p3, s0, p0)

