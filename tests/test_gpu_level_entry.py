"""The entry of the level launches of the dense solve (k_chol_level, csrc/dense_chol.hip): launch records and operands requested
ahead (the default) against the list-walking entry it replaced (MPSFM_CHOL_ENTRY=list), on problems whose items sit on every
cap of the record: the five stars of level_entry_scenes.py in the caller's camera order (source lists of 2, kInlineSrc - 1,
kInlineSrc, kInlineSrc + 1 and 2 kInlineSrc + 1: the unrolled form, a full record, the tail read from the list), an orbit of 40
cameras under the default order and a problem of one tile column.  test_level_heads_cpu.py asserts from the device-free plan
that the stars reach those list lengths; here the handle's plan is held to the same numbers.

Both entries issue the same products in the same order on the same operands, so without inverse accumulators (k_back_level sums
in a fixed order) the solutions are equal as 64-bit patterns.  With them k_inv_y adds its four splits with atomics and two runs of
ONE entry already differ in the last bits: there every solution is held to test_gpu_dense_graphs.py's bound, rho <= C_RHO
(refined_solve.py: forward error over u times Skeel's condition number), against numpy.linalg.solve of the system the handle
returned, and so is the difference of the two entries."""

import functools
import os

import numpy as np
import pytest

import level_entry_scenes as LE
from mpsfm_amd import capi
from refined_solve import C_RHO, U
from test_gpu_panel_waves import panel_input

pytestmark = pytest.mark.gpu

ENTRY_ENV = "MPSFM_CHOL_ENTRY"
CASES = {f"star{L}": (("star", L), LE.ORDER_ENV) for L in LE.STAR_LEAVES}
CASES.update({"orbit40": (("orbit", 40), {}), "one_tile": (("clique", 4), {})})
CHAIN = {"MPSFM_LOCAL_LM": "0"}  # the launch chain also where the single-launch solver would take the problem (one_tile)


class _Env:
    """os.environ with `values` set (None: unset) inside the block."""

    def __init__(self, values):
        self.values = values

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.values}
        for k, v in self.values.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _entry(name):
    return _Env({ENTRY_ENV: None if name == "default" else name})


@functools.lru_cache(maxsize=None)
def _dense(case, inverse):
    """One handle, one sweep_once, then dense_solve_once under default, list and default again: (plan, S, rhs, {entry: y})."""
    key, env = CASES[case]
    adj, prob = LE.problem(*key)
    with _Env({**env, "MPSFM_CHOL_INVERSE": None if inverse else "0"}), capi.BAHandle(prob) as h:
        plan = h.dense_plan()
        h.sweep_once(1e4)
        S, rhs = h.reduced_system()
        ys = {}
        for tag, entry in (("default", "default"), ("list", "list"), ("default_again", "default")):
            with _entry(entry):
                h.dense_solve_once()
                ys[tag] = h.dense_solution()
    return plan, S, rhs, ys


@functools.lru_cache(maxsize=None)
def _numpy(case):
    """numpy.linalg.solve of the handle's system and Skeel's condition number with it (the sweep does not depend on the switches)."""
    _, S, rhs, _ = _dense(case, True)
    y = np.linalg.solve(S, rhs)
    scale = float(np.abs(y).max())
    cond = float((np.abs(np.linalg.inv(S)) @ (np.abs(S) @ np.abs(y) + np.abs(rhs))).max()) / scale
    return y, scale, cond


def _rho(case, d):
    _, scale, cond = _numpy(case)
    return float(np.abs(d).max()) / scale / (U * cond)


@pytest.mark.parametrize("case", list(CASES))
def test_plan_is_the_one_the_case_is_built_for(case):
    key, env = CASES[case]
    adj, _ = LE.problem(*key)
    plan = _dense(case, False)[0]
    P = LE.plan_with_heads(adj, depth=-1 if env else -2, pinv_max_tiles=0)
    assert (plan["tile_columns"], plan["levels"], plan["work_items"], plan["tile_products"]) == (P["nt"], P["nlevels"], P["n_items"], P["products"])
    assert plan["inverse_accumulators"] == 0 and _dense(case, True)[0]["inverse_accumulators"] == 1
    longest = max(it["nsrc"] for it in P["items"] if it["type"] != 2)
    if key[0] == "star":
        assert longest == key[1] and plan["nd_depth"] == -1
    if case == "one_tile":
        assert plan["tile_columns"] == 1 and longest == 0


@pytest.mark.parametrize("case", list(CASES))
def test_entries_agree_bitwise_without_accumulators(case):
    _, S, rhs, ys = _dense(case, False)
    assert np.isfinite(ys["default"]).all()
    assert np.array_equal(ys["default"].view(np.uint64), ys["list"].view(np.uint64))
    assert np.array_equal(ys["default"].view(np.uint64), ys["default_again"].view(np.uint64))
    rho = _rho(case, ys["default"] - _numpy(case)[0])
    print(f"RHO {case} back levels n={S.shape[0]} rho={rho:.3f}")
    assert rho <= C_RHO


@pytest.mark.parametrize("case", list(CASES))
def test_entries_meet_the_bound_with_accumulators(case):
    _, S, rhs, ys = _dense(case, True)
    ref = _numpy(case)[0]
    rhos = {k: _rho(case, y - ref) for k, y in ys.items()}
    between = _rho(case, ys["default"] - ys["list"])
    print(f"RHO {case} accumulators n={S.shape[0]} cond={_numpy(case)[2]:.3g} " + " ".join(f"{k}={v:.3f}" for k, v in rhos.items()) +
          f" default-list={between:.3f} default-default={_rho(case, ys['default'] - ys['default_again']):.3f}")
    assert all(np.isfinite(y).all() for y in ys.values())
    assert max(rhos.values()) <= C_RHO and between <= C_RHO


@pytest.mark.parametrize("case", list(CASES))
def test_full_solves_agree(case):
    key, env = CASES[case]
    out = {}
    for entry in ("default", "list"):
        prob = LE.problem(*key)[1]
        with _Env({**env, **CHAIN}), _entry(entry):
            out[entry] = (capi.ba_solve(prob), prob)
    (sd, pd), (sl, pl) = out["default"], out["list"]
    assert sd["num_iterations"] == sl["num_iterations"] >= 2 and sd["termination"] == sl["termination"]
    assert list(sd["trace_accepted"]) == list(sl["trace_accepted"])
    np.testing.assert_allclose(sd["trace_cost"], sl["trace_cost"], rtol=1e-9)
    np.testing.assert_allclose(pd.cam_t, pl.cam_t, atol=1e-9)


@pytest.mark.parametrize("entry", ["default", "list"])
def test_a_bad_pivot_in_a_two_source_panel_raises_the_flag(entry):
    """The first hub column of the two-leaf star is a panel with two sources.  The given system is the identity with the probe
    input of test_gpu_panel_waves.py on that tile (the leaves are decoupled: the sources contribute exact zeros)."""
    adj, prob = LE.problem("star", 2)
    P = LE.plan_with_heads(adj, depth=-1)
    hub = 3 * 2
    assert all(it["nsrc"] == 2 for it in P["items"] if it["type"] == 0 and it["tk"] == hub)
    with _Env(LE.ORDER_ENV), capi.BAHandle(prob) as h:
        assert h.dense_plan()["nd_depth"] == -1
        h.sweep_once(1e4)
        n = h.reduced_dim
        rhs = np.arange(1.0, n + 1.0)
        with _entry(entry):
            for name, bad in (("a", False), ("d3", True), ("d12", True), ("d29", True), ("a", False)):
                S = np.eye(n)
                S[32 * hub:32 * hub + 32, 32 * hub:32 * hub + 32] = panel_input(name)[:32]
                assert h.dense_solve_given(S, rhs) == bad, name
                if not bad:
                    y = h.dense_solution()
                    np.testing.assert_allclose(y, np.linalg.solve(S, rhs), rtol=1e-12)


@pytest.mark.parametrize("entry", ["default", "list"])
def test_trace_buffer_still_fills(entry):
    import torch

    _, prob = LE.problem("orbit", 40)
    L = capi.lib()
    with capi.BAHandle(prob) as h, _entry(entry):
        nt = h.dense_plan()["tile_columns"]
        h.sweep_once(1e4)
        buf = torch.zeros((nt + 1) * 2 * 8, dtype=torch.int64, device="cuda")
        assert L.mpsfm_debug_set_chol_trace(buf.data_ptr()) == 0
        try:
            h.dense_solve_once()
            torch.cuda.synchronize()
        finally:
            L.mpsfm_debug_set_chol_trace(None)
        t = buf.cpu().numpy().reshape(nt + 1, 2, 8)
        assert (t[:nt, 0, 0] != 0).all(), "the first stamp of a diagonal item is missing"
        assert (t[:nt, 0, 4] >= t[:nt, 0, 0]).all()  # stored after entered
        before = t.copy()
        h.dense_solve_once()  # unregistered: nothing is stamped any more
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy().reshape(nt + 1, 2, 8), before)
