"""The reference side of tests/test_gpu_integration_system.py, alone: at every block-edge map size the oracle's own SciPy PCG,
a sparse direct solve and the same with one long-double refinement step agree on the linear system of IRLS step 0.  The numbers
printed here (pytest -s) are what the GPU bounds are made from; their table stands in DESIGN.md §4b and in the GPU module."""

import numpy as np
import pytest

import integration_cases as IC
from oracle import integration_oracle as IO


@pytest.mark.parametrize("size", IC.SIZES, ids=IC.SIZE_IDS)
def test_builder_places_sparse_points_on_the_border_and_invalid_pixels(size):
    H, W = size
    m = IC.build_maps(H, W)
    assert m["depth_prior"].shape == (H, W) and m["normals"].shape == (H, W, 3) and m["normals_uncertainty"].shape == (H, W, 3, 3)
    assert m["K"][2:] == ((H - 1) / 2.0, (W - 1) / 2.0)
    invalid = ~m["valid"]
    assert invalid.any() and m["valid"].any()
    if H * W > 4:
        assert invalid[H - 1].any() and invalid[:, W - 1].any()  # the last row and the last column have one each
    px = {(int(x), int(y)) for x, y in m["kps"]}
    assert {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)} <= px
    if W >= 3:
        assert {(W // 2, 0), (W // 2, H - 1)} <= px
    if H >= 3:
        assert {(0, H // 2), (W - 1, H // 2)} <= px
    assert all(x in (0, W - 1) or y in (0, H - 1) for x, y in px)
    # the first corner twice, with two depths
    assert tuple(m["kps"][0]) == tuple(m["kps"][-1]) == (0, 0) and m["depth3d"][-1] != m["depth3d"][0]
    # further draws: interior points on request, none at all on request
    assert len(IC.build_maps(H, W, sparse=False)["kps"]) == 0
    if min(H, W) >= 15:
        more = IC.build_maps(H, W, seed=3, n_interior=5)
        assert len(more["kps"]) == len(m["kps"]) + 5


@pytest.mark.parametrize("size", IC.SIZES, ids=IC.SIZE_IDS)
def test_system_is_the_one_the_oracle_solves(size):
    """`system` against the `record=` hook of the oracle's IRLS loop, the "last write wins" rule on the repeated corner, and
    the cached PCG solution against the oracle's own integrate()."""
    R = IC.step_reference(*size)
    rec = []
    IO.integrate(IC.inputs(R["maps"], IC.STEP_CONF), record=rec)
    np.testing.assert_array_equal(rec[0]["b"], R["b"])
    np.testing.assert_array_equal(rec[0]["A_diag"], R["diag"])
    np.testing.assert_array_equal(rec[0]["z_in"], R["z0"])
    np.testing.assert_array_equal(R["A"].diagonal(), R["diag"])
    assert abs(R["A"] - R["A"].T).max() == 0.0
    # the corner's sparse term is the LAST entry's alone
    m = R["maps"]
    none = dict(m, kps=m["kps"][1:-1], depth3d=m["depth3d"][1:-1], zvars3d=m["zvars3d"][1:-1])
    A0, b0, d0, _ = IC.system(none, IC.STEP_CONF)
    prec = (1 / m["zvars3d"][-1]) * m["depth3d"][-1] ** 2
    assert R["diag"][0] - d0[0] == pytest.approx(prec, rel=1e-9)
    assert R["b"][0] - b0[0] == pytest.approx(prec * np.log(m["depth3d"][-1]), rel=1e-9)
    np.testing.assert_array_equal(R["diag"][1:], d0[1:])
    assert R["o10"]["changed"] and R["o10"]["cg_iters"] == [R["cg_iters"]]
    np.testing.assert_allclose(R["o10"]["z"], R["z_cg"], rtol=0, atol=2e-15)  # exp and log back


def test_reference_solutions_agree_at_every_size():
    """The oracle's SciPy PCG at cg_tol 1e-10 has a true residual <= 2 cg_tol |b| and agrees with both direct routes."""
    tol = IC.STEP_CONF["cg_tol"]
    print("\n| HxW | N | cond(A) | CG its | true res / |b| | |z_cg - z_dir|inf | |z_dir - z_dir0|inf | z bound | E1 bound | w bound |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for H, W in IC.SIZES:
        R = IC.step_reference(H, W)
        cond = np.linalg.cond(R["A"].toarray())
        print(f"| {H}x{W} | {H * W} | {cond:.1e} | {R['cg_iters']} | {R['res_cg']:.1e} | {R['d_cg']:.1e} | {R['d_refine']:.1e} | "
              f"{R['z_bound']:.1e} | {R['e1_bound']:.1e} | {R['w_bound']:.1e} |")
        assert R["res_cg"] <= 2 * tol, (H, W)
        # the second run the bounds are made from really converges: below the oracle's cg_max_iter, true residual <= 10 x 1e-12
        assert R["o12"]["cg_iters"] == [R["cg_iters12"]] and R["cg_iters12"] < IO.DEFAULT_CONF["cg_max_iter"], (H, W)
        assert R["res_cg12"] <= 10 * 1e-12, (H, W, R["res_cg12"])
        # the arbiter: no residual left but what rounding z to fp64 puts there, |A| |z| 2^-53 per entry (x4 for the sum's own)
        floor = 4 * 2.0**-53 * np.linalg.norm(abs(R["A"]) @ np.abs(R["z_direct"])) / np.linalg.norm(R["b"])
        assert R["res_direct"] <= floor <= 0.1 * tol, (H, W, R["res_direct"], floor)
        # the three routes: PCG, LU, LU + refinement.  |e|_inf <= |e|_2 <= cond(A) (|r|_2 / |b|_2) |z|_2
        assert R["d_cg"] <= cond * R["res_cg"] * np.linalg.norm(R["z_direct"]), (H, W)
        assert R["d_refine"] <= 1e-9, (H, W)
        assert np.array_equal(R["o10"]["energies"][:1], R["o12"]["energies"][:1])  # no solve in the initial energy


@pytest.mark.parametrize("size", IC.SIZES, ids=IC.SIZE_IDS)
def test_reference_under_another_order_of_its_sums(size):
    """What a correct fp64 PCG may differ by: the oracle's PCG on the symmetrically permuted system (the same iterates in exact
    arithmetic, other rounding).  Every such run must meet every bound the GPU test sets: the reference passes its own test
    whatever the order of its sums.  (With `make_maps`' own focal length it does not at 2x300: integration_cases.FOCAL.)"""
    R = IC.step_reference(*size)
    n = size[0] * size[1]
    e_ref, wu_ref, wv_ref = IC.after_step(R["maps"], R["z_cg"])
    assert e_ref == pytest.approx(R["o10"]["energies"][1], rel=1e-13)
    rng = np.random.default_rng(7)
    perms = [np.arange(n)[::-1], np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)])] + [rng.permutation(n) for _ in range(22)]
    worst, its = np.zeros(3), []
    for perm in perms:
        z, it = IC.reordered_pcg(R, perm)
        its.append(it)
        e, wu, wv = IC.after_step(R["maps"], z)
        assert IC.true_residual(R["A"], R["b"], z) <= 2 * IC.STEP_CONF["cg_tol"]
        dz = float(np.max(np.abs(z - R["z_direct"])))
        assert dz <= R["z_bound"]
        worst = np.maximum(worst, [dz / R["z_bound"], abs(e - e_ref) / e_ref / R["e1_bound"],
                                   max(np.max(np.abs(wu - wu_ref)), np.max(np.abs(wv - wv_ref))) / R["w_bound"]])
    print(f"\n{size[0]}x{size[1]}: iterations {R['cg_iters']}, reordered {min(its)}..{max(its)}; worst z / E1 / w as a fraction of the "
          f"GPU bound: {worst[0]:.2f} {worst[1]:.2f} {worst[2]:.2f}")
    assert worst.max() <= 1.0


@pytest.mark.parametrize("k", [1, 15, 16, 17, 33])
def test_long_double_pcg_follows_scipy_iterate_by_iterate(k):
    """The plain long-double PCG stopped after k iterations against SciPy's fp64 iterate at maxiter = k (16x32)."""
    R = IC.step_reference(16, 32)
    zs, its = IC.scipy_pcg(R["A"], R["b"], R["z0"], R["diag"], 1e-300, maxiter=k)
    zl = IC.pcg_ld(R["A"], R["b"], R["z0"], R["diag"], k)
    d = float(np.max(np.abs(np.asarray(zl, np.float64) - zs)))
    print(f"\n16x32, {k} iterations: |z_ld - z_scipy|inf = {d:.2e}")
    assert its == k and d <= 1e-12
    # and it converges to the direct solution when left to run
    if k == 33:
        zl = IC.pcg_ld(R["A"], R["b"], R["z0"], R["diag"], 400)
        assert np.max(np.abs(np.asarray(zl, np.float64) - R["z_direct"])) <= 1e-12
