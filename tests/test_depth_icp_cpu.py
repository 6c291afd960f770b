"""CPU checks of the dense ICP's NumPy restatement (tests/numpy_depth_icp.py) and of the scenes the GPU tests pin the kernels to
(tests/depth_icp_scenes.py): the redraw condition, the fixed point and its bias, the rejection causes, the two failure endings
and the 6 x 6 step against NumPy's own solver."""

import numpy as np
import pytest

import depth_icp_scenes as S
import numpy_depth_icp as NDI


def _pose_error(T, R, t):
    return float(np.linalg.norm(T[:, :3] - R)), float(np.linalg.norm(T[:, 3] - t))


@pytest.mark.parametrize("name", list(S.LOOP_SCENES))
def test_loop_scene_is_found_within_the_redraws_and_its_starts_agree(name):
    s = S.loop_scene(name)  # raises when 8 draws do not give a scene without a fragile decision
    assert s["redraws"] < S.MAX_REDRAWS
    refs = s["refs"]
    assert [r["status"] for r in refs] == ["converged"] * 3
    assert refs[0]["iterations"] <= refs[1]["iterations"] <= refs[2]["iterations"] <= 6
    for r in refs[1:]:
        assert np.abs(r["tgt_from_src"] - refs[0]["tgt_from_src"]).max() < 1e-12
        assert r["num_pairs"] == refs[0]["num_pairs"] and r["rejected"] == refs[0]["rejected"]
    for r in refs:  # quadratic convergence: the last step is far below the one before
        steps = r["trace"][:, 2:].max(1)
        assert steps[-1] < S.LOOP_EPS and steps[-1] < 1e-3 * steps[-2]
        Rm = r["tgt_from_src"][:, :3]
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-14
        assert r["condition"] < 100.0


def test_edge_maps_are_found_within_the_redraws_and_sit_on_the_block_edges():
    counts = []
    for H, W, whole in S.EDGE_MAPS:
        s = S.edge_scene(H, W, whole)
        assert s["redraws"] < S.MAX_REDRAWS
        assert s["ref"]["num_pairs"] >= 100 and s["ref"]["iterations"] == 1
        counts.append((H - 2) * (W - 2))
    assert counts[:6] == [255, 256, 257, 1023, 1024, 1025] and counts[6] > 65536


def test_fixed_point_bias_is_the_recorded_one():
    """DESIGN.md section 4x records the distance of the fixed point from the truth on the 60 x 80 pair; the GPU end-to-end bound is
    twice S.FIXED_POINT_BIAS."""
    s = S.loop_scene("pair")
    dR, dt = _pose_error(s["refs"][0]["tgt_from_src"], s["R"], s["t"])
    print(f"fixed point of the 60 x 80 pair: |dR|_F = {dR:.4g}, |dt| = {dt:.4g}")
    assert 0.95 * S.FIXED_POINT_BIAS[0] < dR <= S.FIXED_POINT_BIAS[0]
    assert 0.95 * S.FIXED_POINT_BIAS[1] < dt <= S.FIXED_POINT_BIAS[1]
    # nearest-pixel association on a curved surface: the bias shrinks with the pixel
    big = S.loop_scene("large")
    bR, bt = _pose_error(big["refs"][0]["tgt_from_src"], big["R"], big["t"])
    assert bR < dR / 8.0 and bt < dt / 8.0


def test_every_rejection_cause_occurs():
    seen = np.zeros(4, int)
    for name in S.LOOP_SCENES:
        for r in S.loop_scene(name)["refs"]:
            seen += np.array(r["rejections"]).sum(0)
    assert (seen > 0).all(), dict(zip(NDI.REJECT_CAUSES, seen))
    tight = np.array(S.loop_scene("tight")["refs"][2]["rejections"])
    assert tight[0, 3] > 0 and tight[-1, 3] == 0  # the angle gate rejects while the pose is off, nothing at the fixed point


def test_fronto_parallel_plane_is_singular_and_keeps_the_pose():
    depth = np.full((20, 24), 2.5)
    intr = S.window_intr(20, 24)
    init = np.c_[np.eye(3), np.zeros(3)]
    r = NDI.icp(depth, intr, depth, intr, init)
    assert r["status"] == "singular" and r["iterations"] == 1 and r["num_pairs"] == 18 * 22
    assert np.array_equal(r["tgt_from_src"], init)
    assert r["info"][2, 2] == 0.0 and r["info"][3, 3] == 0.0 and r["info"][5, 5] == r["num_pairs"]
    assert r["trace"].tolist() == [[18 * 22, 0.0, 0.0, 0.0]]


def test_target_of_holes_has_too_few_pairs():
    s = S.loop_scene("pair")
    init = s["starts"][1]
    for hole in (0.0, -1.0, np.nan, np.inf):
        r = NDI.icp(s["depth0"], s["intr"], np.full_like(s["depth1"], hole), s["intr"], init)
        assert r["status"] == "too_few_pairs" and r["iterations"] == 1 and r["num_pairs"] == 0 and r["rmse"] == 0.0
        assert np.array_equal(r["tgt_from_src"], init)
        assert r["rejected"][1] > 4000 and r["rejected"][2] == r["rejected"][3] == 0


def test_normals_of_a_tilted_plane_and_their_validity():
    H, W = 9, 11
    intr = np.array([20.0, 21.0, 5.0, 4.0])
    n_true = np.array([0.3, -0.2, -1.0]) / np.linalg.norm([0.3, -0.2, -1.0])
    r, c = np.meshgrid(np.arange(H, dtype=float), np.arange(W, dtype=float), indexing="ij")
    rays = np.stack([(c - intr[2]) / intr[0], (r - intr[3]) / intr[1], np.ones_like(c)], -1)
    depth = (n_true @ np.array([0.0, 0.0, 2.0])) / (rays @ n_true)  # the plane through (0, 0, 2)
    depth[4, 5] = 0.0
    depth[2, 2] *= 1.2  # a depth edge
    normals, valid, _ = NDI.normal_map(depth, intr, 0.05)
    expect = np.zeros((H, W), bool)
    expect[1:-1, 1:-1] = True
    for rr, cc in ((4, 5), (2, 2)):
        for dr, dc in ((0, 0), (0, 1), (0, -1), (1, 0), (-1, 0)):
            expect[rr + dr, cc + dc] = False
    assert np.array_equal(valid, expect)
    assert np.abs(normals[valid] - n_true).max() < 1e-12
    assert not normals[~valid].any()
    small, ok, _ = NDI.normal_map(np.full((3, 3), 1.0), np.array([2.0, 2.0, 1.0, 1.0]), 0.05)
    assert ok.sum() == 1 and ok[1, 1] and np.array_equal(small[1, 1], [0.0, 0.0, -1.0])


def test_step_solves_the_system_and_refuses_rank_deficient_ones():
    rng = np.random.default_rng(5)
    for _ in range(200):
        J = rng.normal(size=(40, 6)) * 10.0 ** rng.uniform(-2, 2, 6)
        A, b = J.T @ J, rng.normal(size=6)
        xi, pivot = NDI.solve(A, b)
        assert pivot > NDI.MIN_PIVOT
        assert np.abs(xi - np.linalg.solve(A, b)).max() <= 1e-9 * np.abs(xi).max()
    J = rng.normal(size=(40, 6))
    J[:, 4] = J[:, 1] - 2.0 * J[:, 3]
    assert NDI.solve(J.T @ J, np.ones(6))[0] is None
    A = np.diag([1.0, 2.0, 0.0, 1.0, 1.0, 1.0])
    assert NDI.solve(A, np.ones(6)) == (None, None)


def test_pose_update_is_the_exponential_on_both_sides_of_the_small_angle():
    T = S.starts(_rot([0.3, -0.5, 0.8], 0.7), np.array([0.1, -0.2, 0.3]))[0]
    for ang in (0.3, 1e-5, 2e-12, 0.5e-12, 0.0):
        xi = np.r_[ang * np.array([0.6, 0.0, -0.8]), 0.01, -0.02, 0.03]
        out, nw, nv = NDI.apply(xi, T)
        E = _rot([0.6, 0.0, -0.8], ang)
        assert np.abs(out[:, :3] - E @ T[:, :3]).max() < 1e-15 and np.abs(out[:, 3] - (E @ T[:, 3] + xi[3:])).max() < 1e-15
        assert abs(nw - ang) <= 1e-15 * max(ang, 1.0) and abs(nv - np.linalg.norm(xi[3:])) < 1e-17


def _rot(axis, ang):
    return S._rodrigues(axis, ang)


def test_defaults_are_the_librarys():
    from mpsfm_amd import capi

    assert capi.ICP_DEFAULTS == NDI.DEFAULTS and capi.ICP_STATUS == NDI.STATUS
