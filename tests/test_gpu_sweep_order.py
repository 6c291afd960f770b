"""k_track_sweep_dense takes its chunk from the order table (SweepArgs::order: heaviest first) instead of blockIdx.x + chunk0;
MPSFM_SWEEP_ORDER=0, read per solve and per probe, switches back.  Nothing is computed differently: every chunk does the same work
into the same slab, the same `part` row and the same pt_fac slots, so these are equal as bit patterns under both settings (the
slabs: wherever two sweeps of ONE setting give the same bits, see test_per_chunk_outputs_are_the_same_bits); the reduced system is
assembled by atomics and agrees to the tolerance tests/test_gpu_ba.py uses for it; a solve reports the same
under both settings to the bounds of tests/test_gpu_lm_split.py.

Scenes: 24 cameras / 2 000 landmarks under MPSFM_CHUNK_RECORDS=64 (over a hundred chunks of 3-8 cameras, every one dense: the sweep
also adopts and zero-fills), and the general-chunk scene of build_table_cases (the table covers the dense chunks only, the general
kernel takes the rest from chunk0 = n_dense).  MPSFM_SLAB_TABLES_HOST=0 makes a handle of this size form its slab tables, and with
them the order table, on the device (DevBuilder::sweep_order); the host's comes from mpsfm_debug_host_build."""

import functools

import numpy as np
import pytest

from build_table_cases import CASES, environment
from mpsfm_amd import capi
from mpsfm_amd.synthetic import make_scene
from test_gpu_level_entry import CHAIN

pytestmark = pytest.mark.gpu

ON, OFF = {"MPSFM_SWEEP_ORDER": None}, {"MPSFM_SWEEP_ORDER": "0"}
SCENES = {
    "many_chunks": (lambda: make_scene(24, 2000, True, seed=3)[0], {"MPSFM_CHUNK_RECORDS": "64"}),
    "general_chunks": (CASES["g"][0], CASES["g"][1]),
}
DEVICE_TABLES = {"MPSFM_SLAB_TABLES_HOST": "0"}
TOLERANCE_ENDINGS = ("function_tolerance", "gradient_tolerance", "parameter_tolerance")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


UNUSED, DIAG, OFFDIAG, CAMVEC = 0, 1, 2, 3


def _slab_word_kinds(hdr, n_dense, n_words):
    """What every word of the slab buffer holds (slab_doubles in csrc/common.h): a block of two cameras (OFFDIAG), the upper triangle
    of a camera's own block (DIAG), the camera vectors g_c | W V^-1 g_p | diag U (CAMVEC), or nothing (UNUSED: the lower triangle of a
    diagonal block, which k_reduce_slabs never reads, and the padding between slabs)."""
    kind = np.full(n_words, UNUSED, np.int8)
    upper = np.where((np.arange(6)[:, None] <= np.arange(6)[None, :]).ravel(), DIAG, UNUSED)
    for H in hdr[:n_dense]:
        ncam, s0 = int(H[5]), int(H[11]) * 18
        nb = ncam * (ncam + 1) // 2
        kind[s0:s0 + nb * 36] = OFFDIAG
        kind[s0 + nb * 36:s0 + nb * 36 + ncam * 18] = CAMVEC
        for c in range(ncam):
            d = s0 + (c * (c + 1) // 2 + c) * 36
            kind[d:d + 36] = upper
    return kind


@functools.lru_cache(maxsize=None)
def _probe(scene):
    """One handle per scene: its tables, and one sweep_once / update_once per setting of the switch from the same state."""
    make, env = SCENES[scene]
    prob = make()
    out = {}
    with environment({**CHAIN, **env, **DEVICE_TABLES, "MPSFM_SWEEP_ORDER": None}):
        out["host_order"] = capi.host_build_table(prob, 35, np.int32)
        with capi.BAHandle(prob.copy()) as h:
            out["built_on_device"] = bool(h.debug_table(22, np.uint8)[0])
            out["order"] = h.sweep_order()
            out["cost"] = h.debug_table(36, np.int32)
            out["hdr"] = h.debug_table(0, np.int32).reshape(-1, 12)
            dense = out["hdr"][:, 10]  # ChunkHdr::dense
            out["n_dense"], out["n_general"] = int(np.sum(dense == 1)), int(np.sum(dense == 0))
            out["handoff"] = h.pt_handoff()
            for name, setting in (("on", ON), ("off", OFF), ("on_again", ON)):
                with environment(setting):
                    h.sweep_once(1e4)
                    r = dict(part=h.debug_table(26, np.float64).reshape(-1, 4)[:out["n_dense"], :3].copy(), slab=h.debug_table(37, np.float64))
                    r["S"], r["rhs"] = h.reduced_system()
                    if out["handoff"]:
                        u = h.update_once(1e4, np.zeros(h.reduced_dim), handoff=True)
                        r["pt_fac"], r["pts2"] = h.debug_table(38, np.float64), u["pts2"]
                out[name] = r
    return out


@pytest.mark.parametrize("scene", list(SCENES))
def test_device_built_table_equals_the_hosts(scene):
    p = _probe(scene)
    assert p["built_on_device"], "the scene is meant to take the device build"
    n = p["n_dense"]
    assert n >= 30 and (p["n_general"] > 0) == (scene == "general_chunks")
    assert len(p["order"]) == n and np.array_equal(p["order"], p["host_order"])
    assert np.array_equal(np.sort(p["order"]), np.arange(n))
    assert not np.array_equal(p["order"], np.arange(n)), "the scene is meant to hold chunks of unequal cost out of order"
    assert np.all(np.diff(p["cost"][p["order"]].astype(np.int64)) <= 0)


@pytest.mark.parametrize("scene", list(SCENES))
def test_per_chunk_outputs_are_the_same_bits(scene):
    p = _probe(scene)
    on, off = p["on"], p["off"]
    assert on["slab"].size > 0 and np.isfinite(on["part"]).all()
    kind = _slab_word_kinds(p["hdr"], p["n_dense"], on["slab"].size)
    differ = _bits(on["slab"]) != _bits(off["slab"])
    again = _bits(on["slab"]) != _bits(p["on_again"]["slab"])
    count = lambda m: {n: int(m[kind == k].sum()) for n, k in (("unused", UNUSED), ("diag", DIAG), ("offdiag", OFFDIAG), ("camvec", CAMVEC))}  # noqa: E731
    print(f"SLABS {scene}: words by kind {count(np.ones_like(differ))}; that differ on against off {count(differ)}, on against on {count(again)}")
    used = kind != UNUSED
    assert used.sum() > 0.8 * used.size and np.isfinite(on["slab"][used]).all()
    # the products of two cameras' Z rows: sums on the matrix pipe in a fixed order
    assert not differ[kind == OFFDIAG].any() and not again[kind == OFFDIAG].any()
    # what a chunk sums per CAMERA (U_c, g_c, W V^-1 g_p) goes through LDS atomics of all its waves.  With the records of a chunk in ONE
    # wave (many_chunks: at most 64) the adds arrive in lane order and the sums are the same bits from sweep to sweep; with four waves
    # (general_chunks: up to 252 records) their order is the hardware's, and two sweeps of ONE setting differ in the last bits (measured
    # there: 19 312 of 1 630 398 words between two sweeps with the table, 20 404 between one with and one without).  Like the reduced
    # system, these are held to 1e-11 of the largest entry instead.
    summed = (kind == DIAG) | (kind == CAMVEC)
    if scene == "many_chunks":
        assert int(p["hdr"][:p["n_dense"], 1].max()) <= 64
        assert not differ[summed].any() and not again[summed].any()
    else:
        np.testing.assert_allclose(on["slab"][summed], off["slab"][summed], rtol=0, atol=1e-11 * np.abs(off["slab"][summed]).max())
    for name in ("part",) + (("pt_fac", "pts2") if p["handoff"] else ()):
        assert np.array_equal(_bits(on[name]), _bits(off[name])), name
        assert np.array_equal(_bits(on[name]), _bits(p["on_again"][name])), name
    if scene == "many_chunks":
        assert p["handoff"] and np.any(on["pt_fac"] != 0.0), "every chunk dense: the sweep hands the landmark factors on"


@pytest.mark.parametrize("scene", list(SCENES))
def test_reduced_system_agrees(scene):
    p = _probe(scene)
    on, off = p["on"], p["off"]
    np.testing.assert_allclose(on["S"], off["S"], rtol=0, atol=1e-11 * np.abs(off["S"]).max())
    np.testing.assert_allclose(on["rhs"], off["rhs"], rtol=0, atol=1e-11 * np.abs(off["rhs"]).max())


@functools.lru_cache(maxsize=None)
def _solve(setting):
    make, env = SCENES["many_chunks"]
    prob = make()
    with environment({**CHAIN, **env, **(ON if setting == "on" else OFF)}), capi.BAHandle(prob) as h:
        fused = h.pt_handoff() and h.direct_front()
        s = h.solve()
        h.get_state()
    return s, prob.cam_t.copy(), prob.cam_quat.copy(), prob.pts.copy(), fused


def test_a_solve_under_the_new_order_adopts_and_ends_on_a_tolerance():
    s, _, _, _, fused = _solve("on")
    print(f"SOLVE: {s['num_iterations']} iterations, {s['termination']}, {s['num_successful_steps']} successful")
    assert fused, "every chunk dense: the dense sweep adopts the accepted candidate and zero-fills what the reduction adds into"
    assert s["termination"] in TOLERANCE_ENDINGS and s["num_successful_steps"] >= 2
    assert s["final_cost"] < s["initial_cost"]


def test_solves_agree_under_both_settings():
    (sa, ta, qa, pa, _), (sb, tb, qb, pb, _) = _solve("on"), _solve("off")
    assert sa["num_iterations"] == sb["num_iterations"] and sa["termination"] == sb["termination"]
    assert list(sa["trace_accepted"]) == list(sb["trace_accepted"])
    np.testing.assert_allclose(sa["trace_cost"], sb["trace_cost"], rtol=1e-9)
    np.testing.assert_allclose(ta, tb, atol=1e-7)
    np.testing.assert_allclose(qa, qb, atol=1e-7)
    np.testing.assert_allclose(pa, pb, atol=1e-7)
