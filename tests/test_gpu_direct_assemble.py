"""The direct form of the front of the dense solve (DirectAsm, csrc/common.h): k_reduce_slabs adds the sums of the slabs straight
into the tile-major system that k_chol_level reads, the dense sweep zeroes what k_assemble used to zero, and the first level launch
adds the damping (its panel items to the diagonal tile they factor, a few workgroups more to the diagonal tiles of the later columns) —
no Sblk, no k_assemble launch.  MPSFM_ASSEMBLE=launch forces the form with k_assemble.

Tolerances: those of test_gpu_sweep_entry.py and test_gpu_lm_split.py, which faced the same kind of change — tiles to 1e-11 of the
system's scale (the two forms add the same slab sums, the atomics meet in another order), solves: equal decisions, trace to rtol
1e-9, state to atol 1e-7."""

import dataclasses
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import level_entry_scenes as LE
from mpsfm_amd import capi
from mpsfm_amd.abi import ALLREDUCE_FN
from mpsfm_amd.synthetic import CX, CY, FX, FY, R_from_quat, make_scene
from test_gpu_level_entry import CHAIN, _Env
from test_gpu_lm_split import ENDINGS, K_CHOL_LEVEL, _scene, launch_counts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_ASSEMBLE = 2  # LaunchFamily of csrc/ba_launch.h
LAUNCH = {"MPSFM_ASSEMBLE": "launch"}
DIRECT = {"MPSFM_ASSEMBLE": None}


# ---- tile parity ---------------------------------------------------------------------------------------------------------------------
def _parity_scene(name):
    if name == "one_tile":  # 3 cameras (2 variable, 12 columns) / 300 landmarks
        return make_scene(3, 300, True, seed=2)[0]
    if name == "six_cameras":  # 6 cameras / 1 500 landmarks
        return make_scene(6, 1500, True, seed=4)[0]
    if name == "straddle":  # 6 VARIABLE cameras, 36 columns: the last one lies across the first tile boundary
        return make_scene(7, 1500, True, seed=4)[0]
    if name == "orbit40":  # 40 cameras on an orbit: the plan is a nested dissection, padding columns end its parts on tile boundaries
        return LE.problem("orbit", 40)[1]
    prob = make_scene(24, 2000, name != "chain_no_depth", seed=11)[0]
    if name == "chain_constant":  # two more constant cameras: slot -1 in the chunks' camera lists
        prob.pose_const[[5, 9]] = 1
    return prob


PARITY = ["one_tile", "six_cameras", "straddle", "chain", "chain_constant", "chain_no_depth", "orbit40"]


def check_parity(name, radius=1e4):
    prob = _parity_scene(name)
    with _Env({**CHAIN, **DIRECT}), capi.BAHandle(prob) as h:
        assert h.direct_front(), "every chunk dense, one rank, level plan"
        r = h.direct_assemble(radius)
    nt, n, live, ap, ad, damp = r["nt"], r["n"], r["live"], r["parent"], r["direct"], r["damp"]
    tile = lambda ti, tj: ti * (ti + 1) // 2 + tj  # noqa: E731
    assert live.sum() == r["n_live"] and all(live[tile(t, t)] and live[tile(nt, t)] for t in range(nt))
    assert np.isfinite(ap[live]).all() and np.isfinite(ad[live]).all(), "a live tile was not zeroed / written"
    scale = np.abs(ap[live]).max()
    # dead tiles and accumulators: exactly zero (no sum lands outside the live tiles; the sweep's zero fill reaches everything)
    assert not ap[~live].any() and not ad[~live].any()
    assert r["unzeroed"] == 0
    # direct + damping == parent on the diagonal, padding diagonals exactly 1, everything else as it is
    want = ad.copy()
    pad = damp < 0
    for g in range(32 * nt):
        d = want[tile(g >> 5, g >> 5)]
        if pad[g]:
            assert d[g & 31, g & 31] == 0.0 and not d[g & 31, :].any() and not d[:, g & 31].any()
            assert ap[tile(g >> 5, g >> 5)][g & 31, g & 31] == 1.0
            d[g & 31, g & 31] = 1.0
        else:
            d[g & 31, g & 31] += damp[g]
    assert pad[n:].all() and (damp[~pad] > 0).all()
    err = np.abs(want[live] - ap[live]).max() / scale
    rhs_rows = [tile(nt, t) for t in range(nt)]
    err_rhs = np.abs(ad[rhs_rows] - ap[rhs_rows]).max() / max(np.abs(ap[rhs_rows]).max(), 1e-300)
    print(f"PARITY {name}: nt {nt}, n {n}, {int(live.sum())} live tiles, {int(pad[:n].sum())} padding columns inside, scale {scale:.3e}, "
          f"tiles {err:.2e}, rhs {err_rhs:.2e}")
    assert err <= 1e-11 and err_rhs <= 1e-11
    assert not ad[rhs_rows][:, 1:, :].any(), "only row 0 of the right-hand-side tiles is written"
    return dict(r, pad_inside=int(pad[:n].sum()))


@pytest.mark.parametrize("name", PARITY)
def test_tiles_are_what_k_assemble_writes(name):
    r = check_parity(name)
    if name == "one_tile":
        assert r["nt"] == 1
    if name == "straddle":
        assert r["n"] > 32 and r["nt"] >= 2
    if name.startswith("chain"):
        assert r["nt"] >= 3
    if name == "orbit40":
        assert r["pad_inside"] > 0, "the scene is meant to have padding columns between the dissection's parts"


def test_tiles_at_a_small_radius():
    check_parity("chain", radius=3.0)


# ---- solves --------------------------------------------------------------------------------------------------------------------------
SWITCHES = {"default": {}, "list_entry": {"MPSFM_CHOL_ENTRY": "list"}, "one_wave_panel": {"MPSFM_CHOL_PANEL_WAVES": "1"},
            "no_speculation": {"MPSFM_LM_SPECULATE": "0"}, "whole_ahead": {"MPSFM_LM_SPLIT": "0"}, "split": {"MPSFM_LM_SPLIT": "1"}}


@functools.lru_cache(maxsize=None)
def _solves(ending, switch, form):
    """Two solves on one handle from the same state: [(summary, cam_t, cam_quat, pts, launch counts, levels, direct?)] * 2."""
    prob = _scene(ending)
    out = []
    with _Env({**CHAIN, **SWITCHES[switch], **(DIRECT if form == "direct" else LAUNCH)}), capi.BAHandle(prob, capi.default_options(**ENDINGS[ending])) as h:
        levels, direct = h.dense_plan()["levels"], h.direct_front()
        for _ in range(2):
            h.reset_state()
            s = h.solve()
            h.get_state()
            out.append((s, prob.cam_t.copy(), prob.cam_quat.copy(), prob.pts.copy(), launch_counts(h), levels, direct))
    return out


def assert_same(a, b):
    (sa, ta, qa, pa), (sb, tb, qb, pb) = a[:4], b[:4]
    assert sa["num_iterations"] == sb["num_iterations"] and sa["termination"] == sb["termination"]
    assert list(sa["trace_accepted"]) == list(sb["trace_accepted"])
    np.testing.assert_allclose(sa["trace_cost"], sb["trace_cost"], rtol=1e-9)
    np.testing.assert_allclose(ta, tb, atol=1e-7)
    np.testing.assert_allclose(qa, qb, atol=1e-7)
    np.testing.assert_allclose(pa, pb, atol=1e-7)


@pytest.mark.parametrize("second", [False, True], ids=["first_solve", "second_solve"])
@pytest.mark.parametrize("switch", ["default", "list_entry", "one_wave_panel", "no_speculation", "whole_ahead"])
@pytest.mark.parametrize("ending", list(ENDINGS))
def test_direct_solves_agree_with_the_assemble_launch(ending, switch, second):
    d, l = _solves(ending, switch, "direct")[int(second)], _solves(ending, switch, "launch")[int(second)]
    assert d[6] and not l[6]
    assert_same(d, l)


@pytest.mark.parametrize("switch", ["default", "list_entry"])
def test_direct_solve_with_padding_columns(switch):
    """The first level launch sets the diagonal of a padding column to 1 (orbit40: a dissected plan)."""
    out = {}
    for form in ("direct", "launch"):
        prob = _parity_scene("orbit40")
        with _Env({**CHAIN, **SWITCHES[switch], **(DIRECT if form == "direct" else LAUNCH)}), capi.BAHandle(prob) as h:
            assert h.direct_front() == (form == "direct") and h.dense_plan()["nd_depth"] >= 1
            runs = []
            for _ in range(2):
                h.reset_state()
                s = h.solve()
                h.get_state()
                runs.append((s, prob.cam_t.copy(), prob.cam_quat.copy(), prob.pts.copy()))
            out[form] = runs
    assert out["launch"][0][0]["num_iterations"] >= 2
    for second in (0, 1):
        assert_same(out["direct"][second], out["launch"][second])


@pytest.mark.parametrize("second", [False, True], ids=["first_solve", "second_solve"])
@pytest.mark.parametrize("switch", ["split", "whole_ahead", "no_speculation"])
@pytest.mark.parametrize("ending", list(ENDINGS))
def test_launch_counts(ending, switch, second):
    (sd, _, _, _, cd, levels, _), (sl, _, _, _, cl, _, _) = _solves(ending, switch, "direct")[int(second)], _solves(ending, switch, "launch")[int(second)]
    assert cd[K_ASSEMBLE] == 0
    assert cl[K_CHOL_LEVEL] % levels == 0 and cl[K_ASSEMBLE] == cl[K_CHOL_LEVEL] // levels  # one per enqueued iteration
    assert cd[K_CHOL_LEVEL] == cl[K_CHOL_LEVEL] == levels * (sl["num_iterations"] + (1 if switch == "whole_ahead" else 0))


# ---- fallbacks: each reports and takes the path with k_assemble -------------------------------------------------------------------------
def _fallback(prob, env, options=None, reference_prob=None):
    """(the handle's solve under `env`, the same handle kind under MPSFM_ASSEMBLE=launch); asserts that both launch k_assemble."""
    out = []
    for form in (DIRECT, LAUNCH):
        p = prob.copy()
        with _Env({**CHAIN, **env, **form}), capi.BAHandle(p, options() if options else None) as h:
            assert not h.direct_front()
            levels = h.dense_plan()["levels"]
            s = h.solve()
            h.get_state()
            counts = launch_counts(h)
        assert counts[K_ASSEMBLE] >= s["num_iterations"] >= 1
        if counts[K_CHOL_LEVEL]:
            assert counts[K_ASSEMBLE] == counts[K_CHOL_LEVEL] // levels
        out.append((s, p.cam_t.copy(), p.cam_quat.copy(), p.pts.copy()))
    assert_same(out[0], out[1])
    return out[0]


def test_a_sharded_handle_keeps_the_assemble_launch():
    hook = ALLREDUCE_FN(lambda user, buf, count, on_device, stream: 0)  # one rank: the sum is what is there
    got = _fallback(_scene(), {}, lambda: capi.default_options(allreduce=hook, world_size=1, rank=0))
    assert_same(got, _solves("tolerance", "default", "launch")[0])


def _general_chunk_scene():
    """The chain scene with landmark 0 seen by every camera in front of it: more than 16 cameras, so its chunk is a general one
    (as long_track_scene of test_gpu_pt_handoff.py)."""
    prob = _scene()
    Xc = np.einsum("nij,j->ni", R_from_quat(prob.cam_quat), prob.pts[0]) + prob.cam_t
    have = set(prob.obs_cam[prob.obs_pt == 0].tolist())
    add = np.array([c for c in range(prob.n_cams) if c not in have and Xc[c, 2] > 0.5], np.int32)
    assert len(have) + len(add) > 16
    xy = np.stack([FX * Xc[add, 0] / Xc[add, 2] + CX, FY * Xc[add, 1] / Xc[add, 2] + CY], axis=1) + 0.5
    return dataclasses.replace(prob, obs_cam=np.concatenate([prob.obs_cam, add]), obs_pt=np.concatenate([prob.obs_pt, np.zeros(len(add), np.int32)]),
                               obs_xy=np.concatenate([prob.obs_xy, xy]))


def test_a_general_chunk_keeps_the_assemble_launch():
    _fallback(_general_chunk_scene(), {})


def test_no_inverse_accumulators_keep_the_assemble_launch():
    got = _fallback(_scene(), {"MPSFM_CHOL_INVERSE": "0"})
    assert_same(got, _solves("tolerance", "default", "launch")[0])


# ---- poisoned allocations ------------------------------------------------------------------------------------------------------------
def test_on_poisoned_blocks():
    """Every block the handle gets is filled with 0xFF first: a tile, accumulator or vector the direct form reads without having zeroed
    it shows up as a wrong answer (tests/_direct_assemble_worker.py)."""
    env = dict(os.environ, MPSFM_POISON="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_direct_assemble_worker.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
