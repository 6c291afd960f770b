"""The integration's linear system and both CG kernel forms (one and two pixels per thread, MPSFM_INT_PIX) at map sizes on the
indexing edges of csrc/int_kernels.hip: 2x2, two rows, two columns, pixel counts on either side of a 256- and a 512-pixel
workgroup.  Sparse points sit on the corners and border lines, one corner twice (tests/integration_cases.py).

Every bound is made from the reference alone (tests/test_integration_system_cpu.py prints them; pytest -s), never from HIP's
output.  One IRLS step at cg_tol 1e-10, scale_filter off:
  true res      |b - A z_cg|_2 / |b|_2 of the oracle's SciPy PCG, in long double
  d_cg, d_ref   |z_cg - z_direct|_inf, |z_direct - z_direct_unrefined|_inf (sparse LU, one long-double refinement step)
  z bound       10 max(d_cg, d_ref, 1e-15);  E1 / w bound: 10 x (oracle at cg_tol 1e-10 against 1e-12), floor 1e-12

| HxW | N | cond(A) | CG its | true res | d_cg | d_ref | z bound | E1 bound | w bound |
|---|---|---|---|---|---|---|---|---|---|
| 2x2 | 4 | 1.9e+01 | 4 | 1.6e-16 | 2.2e-16 | 4.4e-16 | 1.0e-14 | 1.0e-11 | 1.0e-11 |
| 2x3 | 6 | 3.5e+01 | 6 | 1.6e-15 | 4.4e-16 | 4.4e-16 | 1.0e-14 | 1.0e-11 | 1.0e-11 |
| 3x2 | 6 | 3.3e+01 | 6 | 3.5e-15 | 4.4e-16 | 2.2e-16 | 1.0e-14 | 1.0e-11 | 1.0e-11 |
| 15x17 | 255 | 1.1e+04 | 118 | 6.0e-11 | 3.1e-12 | 6.7e-15 | 3.1e-11 | 1.0e-11 | 2.9e-11 |
| 16x16 | 256 | 9.1e+03 | 117 | 6.7e-11 | 2.7e-12 | 1.3e-14 | 2.7e-11 | 1.0e-11 | 3.2e-11 |
| 2x129 | 258 | 6.0e+05 | 422 | 9.4e-11 | 3.7e-11 | 1.1e-12 | 3.7e-10 | 4.1e-10 | 7.1e-09 |
| 129x2 | 258 | 2.2e+03 | 186 | 6.9e-11 | 1.0e-11 | 8.7e-15 | 1.0e-10 | 1.0e-11 | 3.9e-11 |
| 7x73 | 511 | 1.9e+05 | 221 | 8.9e-11 | 1.1e-11 | 1.4e-14 | 1.1e-10 | 2.4e-11 | 8.5e-10 |
| 16x32 | 512 | 3.5e+04 | 182 | 6.3e-11 | 9.5e-12 | 6.2e-14 | 9.5e-11 | 2.2e-11 | 8.9e-11 |
| 19x27 | 513 | 2.8e+04 | 175 | 9.3e-11 | 7.8e-12 | 8.3e-14 | 7.8e-11 | 1.0e-11 | 1.1e-10 |
| 24x32 | 768 | 4.7e+04 | 212 | 9.5e-11 | 1.2e-11 | 2.0e-14 | 1.2e-10 | 2.1e-11 | 1.5e-10 |
| 22x35 | 770 | 5.1e+04 | 221 | 7.7e-11 | 1.6e-11 | 7.7e-14 | 1.6e-10 | 1.3e-11 | 1.7e-10 |
| 2x300 | 600 | 1.4e+06 | 2698 | 8.4e-11 | 1.5e-08 | 2.0e-11 | 1.5e-07 | 1.9e-07 | 3.2e-06 |

HIP must reach |b - A z|_2 <= 10 cg_tol |b|_2 (1: the CG test on the recurrence residual; 10: room for its gap to the true
residual, which the reference's own runs put at about 1x at 1e-10), |z - z_direct|_inf <= z bound, energies[0] to 1e-12,
energies[1] and the weights to their bounds.

The maps are drawn with a focal length of 0.3 map widths (integration_cases.FOCAL).  With `make_maps`' own 1.1 the oracle at
cg_tol 1e-12 does not converge at 2x300 within its 5000 iterations, the bounds made from that run mean nothing, and both the
two-pixel form (energies[1] 1.78e-07 off, bound 6.48e-08, 4671 iterations where the oracle takes 4823) and the oracle's own PCG
with its sums reordered (the same 1.78e-07 in 9 of 60 orders) miss them; the CPU twin now asserts that the reference converges
at 1e-12 and meets these bounds under reordered sums at every size."""

import os

import numpy as np
import pytest
from scipy.sparse.linalg import spsolve

import integration_cases as IC
from conftest import GOLDEN
from mpsfm_amd import capi
from oracle import integration_oracle as IO

pytestmark = pytest.mark.gpu

PIX = pytest.mark.parametrize("pix", [1, 2])
SIZE = pytest.mark.parametrize("size", IC.SIZES, ids=IC.SIZE_IDS)


def _hip(maps, **kw):
    return capi.integrate_depth(maps["depth_prior"], maps["depth_uncertainty"], maps["valid"], maps["normals"], IC.normals_var(maps),
                                maps["depth_init"], maps["K"], maps["kps"], maps["depth3d"], maps["zvars3d"], **kw)


def _item(maps, **extra):
    d = dict(depth_prior=maps["depth_prior"], depth_uncertainty=maps["depth_uncertainty"], valid=maps["valid"], normals=maps["normals"],
             normals_var=IC.normals_var(maps), depth_init=maps["depth_init"], K=maps["K"], kps=maps["kps"], depth3d=maps["depth3d"],
             zvars3d=maps["zvars3d"])
    d.update(extra)
    return d


# ---- a. one IRLS step, tight -----------------------------------------------------------------------------------------------

def _one_step(size, pix, monkeypatch):
    """Runs one IRLS step under the given kernel form and holds it to the reference's bounds; returns z."""
    monkeypatch.setenv("MPSFM_INT_PIX", str(pix))
    R = IC.step_reference(*size)
    depth, s, wu, wv = _hip(R["maps"], conf=IC.STEP_CONF)
    assert s["changed"] and s["irls_iterations"] == 1
    z = np.log(depth).ravel()
    tol = IC.STEP_CONF["cg_tol"]
    res = IC.true_residual(R["A"], R["b"], z)
    dz = float(np.max(np.abs(z - R["z_direct"])))
    o = R["o10"]
    e0 = abs(s["energies"][0] - o["energies"][0]) / o["energies"][0]
    e1 = abs(s["energies"][1] - o["energies"][1]) / o["energies"][1]
    dw = max(float(np.max(np.abs(wu - o["wu"]))), float(np.max(np.abs(wv - o["wv"]))))
    print(f"\n{size[0]}x{size[1]} pix {pix}: cg {s['cg_iters']} (oracle {o['cg_iters']}) res/|b| {res:.2e} (<= {10 * tol:.0e})  "
          f"|z - z_direct| {dz:.2e} (<= {R['z_bound']:.1e})  E0 {e0:.1e} (<= 1e-12)  E1 {e1:.1e} (<= {R['e1_bound']:.1e})  "
          f"w {dw:.1e} (<= {R['w_bound']:.1e})")
    assert res <= 10 * tol
    assert dz <= R["z_bound"]
    assert e0 <= 1e-12
    assert e1 <= R["e1_bound"]
    assert dw <= R["w_bound"]
    return z


@PIX
@SIZE
def test_one_irls_step_solves_the_oracles_system(size, pix, monkeypatch):
    _one_step(size, pix, monkeypatch)


# ---- f. the two forms against each other -----------------------------------------------------------------------------------

@SIZE
def test_the_two_kernel_forms_agree(size, monkeypatch):
    """Each within the bounds of the one-step test, and within twice its z bound of each other (not bit for bit: the partial
    sums are grouped differently)."""
    z1 = _one_step(size, 1, monkeypatch)
    z2 = _one_step(size, 2, monkeypatch)
    assert np.max(np.abs(z1 - z2)) <= 2 * IC.step_reference(*size)["z_bound"]


# ---- b. several IRLS steps -------------------------------------------------------------------------------------------------

@PIX
@pytest.mark.parametrize("scale_filter", [True, False])
@pytest.mark.parametrize("size", [(19, 27), (22, 35)], ids=["19x27", "22x35"])
def test_four_irls_steps(size, scale_filter, pix, monkeypatch):
    monkeypatch.setenv("MPSFM_INT_PIX", str(pix))
    maps = IC.with_outlier(IC.step_reference(*size)["maps"])
    conf = dict(max_iter=4, tol=0, cg_tol=1e-10, scale_filter=scale_filter)
    o10, o12 = IC.steps_reference(size[0], size[1], scale_filter)
    assert o10["changed"] == o12["changed"] and len(o10["energies"]) == len(o12["energies"])
    depth, s, wu, wv = _hip(maps, conf=conf)
    assert s["changed"] == o10["changed"]
    assert s["irls_iterations"] == len(o10["cg_iters"]) and len(s["energies"]) == len(o10["energies"])
    np.testing.assert_allclose(s["energies"][0], o10["energies"][0], rtol=1e-12)
    for i in range(1, len(s["energies"])):
        bound = 10 * IC.rel_gap(o10["energies"][i], o12["energies"][i])
        got = abs(s["energies"][i] - o10["energies"][i]) / o10["energies"][i]
        print(f"\n{size} filter {scale_filter} pix {pix}: E{i} {got:.1e} (<= {bound:.1e})")
        assert got <= bound
    if o10["changed"]:
        bound = 10 * IC.abs_gap(o10["z"], o12["z"])
        got = float(np.max(np.abs(np.log(depth).ravel() - o10["z"])))
        print(f"{size} filter {scale_filter} pix {pix}: |z - z_oracle| {got:.1e} (<= {bound:.1e})")
        assert got <= bound
    else:
        assert depth is None


# ---- c. iteration limits around the host's 16-iteration poll ---------------------------------------------------------------

@PIX
@pytest.mark.parametrize("k", [1, 15, 16, 17, 33])
def test_cg_iteration_limit_around_the_poll(k, pix, monkeypatch):
    """An unreachable cg_tol: exactly cg_max_iter iterations, and the iterate is the long-double PCG's after as many."""
    monkeypatch.setenv("MPSFM_INT_PIX", str(pix))
    R = IC.step_reference(16, 32)
    depth, s, *_ = _hip(R["maps"], conf=dict(IC.STEP_CONF, cg_tol=1e-300, cg_max_iter=k))
    assert s["cg_iters"] == [k]
    assert s["changed"]
    zl = np.asarray(IC.pcg_ld(R["A"], R["b"], R["z0"], R["diag"], k), np.float64)
    zs, its = IC.scipy_pcg(R["A"], R["b"], R["z0"], R["diag"], 1e-300, maxiter=k)
    assert its == k
    bound = 10 * max(float(np.max(np.abs(zl - zs))), 1e-15)
    got = float(np.max(np.abs(np.log(depth).ravel() - zl)))
    print(f"\n16x32, {k} iterations, pix {pix}: |z - z_ld| {got:.2e} (<= {bound:.2e})")
    assert got <= bound


# ---- d. batches under a forced kernel form ---------------------------------------------------------------------------------

def _same(single, batched):
    (d1, s1, wu1, wv1), (d2, s2, wu2, wv2) = single, batched
    for key in ("changed", "irls_iterations", "cg_iters", "energies", "energy_old", "integrated"):
        assert s1[key] == s2[key], key
    if d1 is None:
        assert d2 is None
    else:
        np.testing.assert_array_equal(d1, d2)
    np.testing.assert_array_equal(wu1, wu2)
    np.testing.assert_array_equal(wv1, wv2)


@PIX
def test_batch_of_eight_equals_single_calls(pix, monkeypatch):
    """19x27 = 513 pixels: the last workgroup holds one pixel.  Six different images (one without sparse points), a repeat of the
    first, and a frame fed back in its integrated state, which is skipped."""
    monkeypatch.setenv("MPSFM_INT_PIX", str(pix))
    H, W = 19, 27
    cases = [IC.build_maps(H, W, seed=10 + i, n_interior=[6, 0, 15, 2, 25, 10][i], sparse=i != 3) for i in range(6)]
    assert len({len(m["kps"]) for m in cases}) == 6 and len(cases[3]["kps"]) == 0
    singles = [_hip(m) for m in cases]
    d2, s2, wu2, wv2 = singles[2]
    assert s2["changed"]
    again = dict(cases[2], depth_init=d2)
    extra = dict(init=True, integrated=True, energy_old=s2["energy_old"], wu=wu2, wv=wv2)
    single_again = _hip(again, **extra)
    assert single_again[0] is None and not single_again[1]["changed"]
    batch = capi.integrate_depth_batch([_item(m) for m in cases] + [_item(cases[0]), _item(again, **extra)])
    assert len(batch) == 8
    for one, got in zip(singles + [singles[0], single_again], batch):
        _same(one, got)
    _same(batch[0], batch[6])  # the repeat, bit for bit
    assert batch[7][0] is None and not batch[7][1]["changed"] and batch[7][1]["irls_iterations"] == 0
    assert any(s["changed"] for _, s, _, _ in batch[:6])
    assert len({tuple(s["cg_iters"]) for _, s, _, _ in batch[:6]}) > 1  # one image's CG really ends before another's


@PIX
def test_batch_of_a_solved_and_an_aborted_frame(pix, monkeypatch):
    """The reference's case c and its "energy increased, skipping this frame" input in one batch of two."""
    from test_reference_fixtures_cpu import reference_integration_maps

    monkeypatch.setenv("MPSFM_INT_PIX", str(pix))
    ri = np.load(os.path.join(GOLDEN, "reference_integration.npz"))
    normal = reference_integration_maps(ri, "c")
    abort = reference_integration_maps(ri, "c", depth_init=ri["int_abort_depth_init"])
    singles = [_hip(normal), _hip(abort)]
    batch = capi.integrate_depth_batch([_item(normal), _item(abort)])
    for one, got in zip(singles, batch):
        _same(one, got)
    assert batch[0][1]["changed"]
    assert batch[1][1]["changed"] is False and batch[1][0] is None
    assert batch[1][1]["energy_old"] == pytest.approx(float(ri["int_abort_energy_old"]), rel=1e-6)


# ---- e. the variance solve -------------------------------------------------------------------------------------------------

@PIX
@pytest.mark.parametrize("use_sparse", [False, True])
@pytest.mark.parametrize("size", IC.VARIANCE_SIZES, ids=[f"{h}x{w}" for h, w in IC.VARIANCE_SIZES])
def test_variance_field_equals_the_direct_solve(size, use_sparse, pix, monkeypatch):
    monkeypatch.setenv("MPSFM_INT_PIX", str(pix))
    H, W = size
    maps = IC.step_reference(H, W)["maps"]
    Hm = IO.calculate_hessian(IC.inputs(maps), ignore_depths=not use_sparse)
    want = spsolve(Hm.tocsc(), np.ones(H * W))
    rng = np.random.default_rng(H * 1000 + W)
    q = np.concatenate([[(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)], np.stack([rng.integers(0, W, 12), rng.integers(0, H, 12)], 1)])
    args = (maps["depth_prior"], maps["depth_uncertainty"], maps["valid"], maps["normals"], IC.normals_var(maps), maps["depth_init"], maps["K"])
    kw = dict(kps=maps["kps"], depth3d=maps["depth3d"], zvars3d=maps["zvars3d"], use_sparse=use_sparse, rtol=1e-12, return_field=True)
    got, s, field = capi.integration_variances(*args, q, **kw)
    print(f"\n{H}x{W} sparse {use_sparse} pix {pix}: cg {s['cg_iterations']}, field rel {np.max(np.abs(field.ravel() / want - 1)):.1e}")
    assert s["converged"]
    np.testing.assert_allclose(field.ravel(), want, rtol=1e-7)
    np.testing.assert_array_equal(got, field[q[:, 1], q[:, 0]])
    none, s0, field0 = capi.integration_variances(*args, np.zeros((0, 2), np.int64), **kw)
    assert none.shape == (0,) and s0["converged"] and s0["cg_iterations"] == s["cg_iterations"]
    np.testing.assert_array_equal(field0, field)
