"""GPU checks of the dense point-to-plane ICP (csrc/depth_icp.hip through capi.depth_normals, depth_pair_icp and
depth_pair_register_dense): the normal maps, one linearisation around every edge of the source partition against long-double
sums, the whole loop decision by decision against the NumPy restatement (tests/numpy_depth_icp.py), repeatability, the one-call
registration against its two halves and against the truth, the failure endings and the argument checks."""

import numpy as np
import pytest

import depth_icp_scenes as S
import numpy_depth_icp as NDI
from alignment_scenes import depth_pair_scene
from mpsfm_amd import capi
from mpsfm_amd.sfm.estimators import depth_to_normals, refine_depth_pair, register_depth_pair, register_depth_pair_dense
from mpsfm_amd.sfm.estimators.alignment import Sim3d

pytestmark = pytest.mark.gpu

LOOP_CASES = [(name, k) for name in S.LOOP_SCENES for k in range(3)]


def _icp(s, T, scale=1.0, depth1=None, **options):
    return capi.depth_pair_icp(s["depth0"], s["intr"], s["depth1"] if depth1 is None else depth1, s["intr"], T, scale=scale, **options)


def _same_bits(a, b):
    for k in ("status", "iterations", "num_pairs", "rejected", "rmse", "scale"):
        assert a[k] == b[k], k
    for k in ("tgt_from_src", "info", "rhs", "trace"):
        assert a[k].tobytes() == b[k].tobytes(), k


def _against_restatement(got, ref):
    """(c): decisions equal, the pose within 1e-9 (section 4w's model bound), trace rmse and step norms within 1e-9 absolute."""
    assert got["status"] == ref["status"] and got["iterations"] == ref["iterations"]
    assert got["trace"].shape == ref["trace"].shape
    assert got["trace"][:, 0].tolist() == [float(c) for c in ref["counts"]]
    assert got["num_pairs"] == ref["num_pairs"] and got["rejected"] == ref["rejected"]
    print("pose", np.abs(got["tgt_from_src"] - ref["tgt_from_src"]).max(), "trace", np.abs(got["trace"][:, 1:] - ref["trace"][:, 1:]).max())
    assert np.abs(got["tgt_from_src"] - ref["tgt_from_src"]).max() < 1e-9
    assert np.abs(got["trace"][:, 1:] - ref["trace"][:, 1:]).max() < 1e-9
    assert abs(got["rmse"] - ref["rmse"]) < 1e-9 and got["scale"] == ref["scale"]


@pytest.mark.parametrize("which", ["pair", "occluder", "tiny"])
def test_normal_maps_match_restatement(which):
    if which == "tiny":
        maps, intr = [np.array([[1.0, 1.1, 1.0], [1.2, 1.15, 1.1], [1.0, 1.2, 1.3]])], np.array([2.0, 2.5, 1.0, 1.0])
    else:
        s = S.loop_scene(which)
        maps, intr = [s["depth0"], s["depth1"]], s["intr"]
    for depth in maps:
        want, want_valid, fragile = NDI.normal_map(depth, intr, 0.05)
        assert not fragile
        got, got_valid = capi.depth_normals(depth, intr)
        assert got.shape == depth.shape + (3,) and got_valid.dtype == bool
        assert np.array_equal(got_valid, want_valid) and got_valid.any() and not got_valid.all()
        assert np.abs(got - want).max() < 1e-12
        assert not got[~got_valid].any()
        assert np.abs(np.linalg.norm(got[got_valid], axis=-1) - 1.0).max() < 1e-15
    nf, vf = depth_to_normals(maps[0].astype(np.float32), intr)  # float32 maps are widened on the host
    nd, vd = capi.depth_normals(maps[0].astype(np.float32).astype(np.float64), intr)
    assert nf.tobytes() == nd.tobytes() and np.array_equal(vf, vd)


@pytest.mark.parametrize("H,W,whole", S.EDGE_MAPS)
def test_one_linearisation_at_block_edges(H, W, whole):
    s = S.edge_scene(H, W, whole)
    ref = s["ref"]
    got = _icp(s, s["start"], **s["options"])
    assert got["iterations"] == 1 and got["trace"].shape == (1, 4)
    assert got["num_pairs"] == ref["num_pairs"] and got["rejected"] == ref["rejected"]
    top = np.abs(ref["info"]).max()
    print((H, W), "info", np.abs(got["info"] - ref["info"]).max() / top, "rhs", np.abs(got["rhs"] - ref["rhs"]).max() / top)
    assert np.abs(got["info"] - ref["info"]).max() <= 1e-12 * top
    assert np.abs(got["rhs"] - ref["rhs"]).max() <= 1e-12 * top
    assert np.array_equal(got["info"], got["info"].T)
    assert abs(got["rmse"] - ref["rmse"]) <= 1e-12 and got["trace"][0, 0] == ref["num_pairs"] and got["trace"][0, 1] == got["rmse"]


@pytest.mark.parametrize("name,k", LOOP_CASES)
def test_loop_matches_restatement(name, k):
    s = S.loop_scene(name)
    _against_restatement(_icp(s, s["starts"][k], **s["options"]), s["refs"][k])


def test_two_calls_are_bitwise_identical():
    s = S.loop_scene("large")
    a, b = _icp(s, s["starts"][2], **s["options"]), _icp(s, s["starts"][2], **s["options"])
    _same_bits(a, b)
    s = S.loop_scene("occluder")
    _same_bits(_icp(s, s["starts"][1], stride=3), _icp(s, s["starts"][1], stride=3))


def _pose_error(T, R, t):
    return float(np.linalg.norm(T[:, :3] - R)), float(np.linalg.norm(T[:, 3] - t))


def _point_rmse(T, R, t, depth, intr):
    """How far a pose carries the surface from where the true pose carries it: the RMS over the valid vertices of the map."""
    V, ok = NDI.vertex_map(depth, intr)
    X = V[ok]
    return float(np.sqrt((np.linalg.norm(X @ (T[:, :3] - R).T + (T[:, 3] - t), axis=1) ** 2).mean()))


def test_register_dense_is_the_composition_and_lands_at_the_fixed_point():
    """(e).  The distance of a pose from the truth is measured where it matters for a registration, on the surface: the RMS
    displacement of map 0's vertices between the pose and the true pose; the components |dR|_F and |dt| are held to twice the
    restatement's fixed-point bias.  Measured on an MI355X with seed 2: refined 9.65e-5 / 2.11e-4 (|dR|_F / |dt|)
    and 1.03e-4 on the surface; RANSAC 1.29e-4 / 1.51e-4 and 1.18e-4 on the surface.  The refined pose is closer in rotation and on the
    surface, not in |dt|: both poses sit at the level of the nearest-pixel bias."""
    P = depth_pair_scene()
    args = (P["depth0"], P["intr"], P["depth1"], P["intr"], P["kps0"], P["kps1"], P["matches"])
    got = capi.depth_pair_register_dense(*args, seed=2, icp=dict(eps_rotation=S.LOOP_EPS, eps_translation=S.LOOP_EPS))
    first = capi.depth_pair_register(*args, seed=2)
    for k in ("success", "num_trials", "num_inliers", "lo_rounds", "num_batches", "num_models", "scale"):
        assert got[k] == first[k], k
    for k in ("tgt_from_src", "inlier_mask", "valid", "lifted0", "lifted1"):
        assert got[k].tobytes() == first[k].tobytes(), k
    assert got["success"]
    second = capi.depth_pair_icp(P["depth0"], P["intr"], P["depth1"], P["intr"], first["tgt_from_src"], scale=first["scale"],
                                 eps_rotation=S.LOOP_EPS, eps_translation=S.LOOP_EPS)
    _same_bits(got["refined"], second)
    refined, ransac = got["refined"]["tgt_from_src"], first["tgt_from_src"]
    assert got["refined"]["status"] == "converged" and got["refined"]["iterations"] <= 6
    dR, dt = _pose_error(refined, P["R"], P["t"])
    rR, rt = _pose_error(ransac, P["R"], P["t"])
    e_icp, e_ransac = (_point_rmse(T, P["R"], P["t"], P["depth0"], P["intr"]) for T in (refined, ransac))
    print(f"refined |dR| {dR:.4g} |dt| {dt:.4g} surface {e_icp:.4g}; RANSAC |dR| {rR:.4g} |dt| {rt:.4g} surface {e_ransac:.4g}")
    assert dR <= 2.0 * S.FIXED_POINT_BIAS[0] and dt <= 2.0 * S.FIXED_POINT_BIAS[1]
    assert e_icp < e_ransac
    # the restatement from the same RANSAC pose ends at the same pose (a step more or less moves it by less than the last step)
    ref = NDI.icp(P["depth0"], P["intr"], P["depth1"], P["intr"], ransac, eps_rotation=S.LOOP_EPS, eps_translation=S.LOOP_EPS)
    assert np.abs(refined - ref["tgt_from_src"]).max() < 1e-9 and got["refined"]["num_pairs"] == ref["num_pairs"]
    # the estimators' interface: a Sim3d in, a Sim3d out
    res = register_depth_pair_dense(P["kps0"], P["kps1"], P["matches"], P["depth0"], P["depth1"], P["intr"], P["intr"], random_seed=2,
                                    icp=dict(eps_rotation=S.LOOP_EPS, eps_translation=S.LOOP_EPS))
    plain = register_depth_pair(P["kps0"], P["kps1"], P["matches"], P["depth0"], P["depth1"], P["intr"], P["intr"], random_seed=2)
    assert np.array_equal(res["tgt_from_src"].matrix(), plain["tgt_from_src"].matrix()) and np.array_equal(res["inlier_mask"], plain["inlier_mask"])
    again = refine_depth_pair(P["depth0"], P["depth1"], P["intr"], P["intr"], plain["tgt_from_src"], eps_rotation=S.LOOP_EPS,
                              eps_translation=S.LOOP_EPS)
    assert isinstance(res["refined"]["tgt_from_src"], Sim3d) and res["refined"]["status"] == again["status"] == "converged"
    assert np.abs(again["tgt_from_src"].matrix() - refined).max() < 1e-9 and np.abs(res["refined"]["tgt_from_src"].matrix() - refined).max() < 1e-9
    assert again["information"].shape == (6, 6) and again["trace"].shape == (again["iterations"], 4) and again["num_pairs"] == got["refined"]["num_pairs"]
    # no model: the ICP result is empty
    few = P["matches"][:2]
    none = capi.depth_pair_register_dense(P["depth0"], P["intr"], P["depth1"], P["intr"], P["kps0"], P["kps1"], few)
    assert none["success"] is False and none["refined"] is None
    assert register_depth_pair_dense(P["kps0"], P["kps1"], few, P["depth0"], P["depth1"], P["intr"], P["intr"]) is None


def test_singular_and_too_few_pairs_keep_the_pose():
    depth, intr, init = np.full((20, 24), 2.5), S.window_intr(20, 24), np.c_[np.eye(3), np.zeros(3)]
    got = capi.depth_pair_icp(depth, intr, depth, intr, init)
    ref = NDI.icp(depth, intr, depth, intr, init)
    assert ref["status"] == "singular" and not ref["fragile"]
    _against_restatement(got, ref)
    assert np.array_equal(got["tgt_from_src"], init) and np.abs(got["info"] - ref["info"]).max() <= 1e-12 * np.abs(ref["info"]).max()
    assert got["info"][2, 2] == 0.0  # a sum of exact zeros: the diagonal entry that makes the system singular
    s = S.loop_scene("pair")
    for hole in (0.0, np.nan):
        holes = np.full_like(s["depth1"], hole)
        got = _icp(s, s["starts"][1], depth1=holes)
        assert got["status"] == "too_few_pairs" and got["iterations"] == 1 and got["num_pairs"] == 0 and got["rmse"] == 0.0
        assert np.array_equal(got["tgt_from_src"], s["starts"][1]) and not got["info"].any()
        assert got["rejected"] == NDI.icp(s["depth0"], s["intr"], holes, s["intr"], s["starts"][1])["rejected"]
    # min_pairs above what the first linearisation finds
    ref = s["refs"][2]
    got = _icp(s, s["starts"][2], min_pairs=ref["counts"][0] + 50, **s["options"])
    want = NDI.icp(s["depth0"], s["intr"], s["depth1"], s["intr"], s["starts"][2], min_pairs=ref["counts"][0] + 50, max_iterations=1, **s["options"])
    assert want["status"] == "too_few_pairs" and got["status"] == "too_few_pairs" and got["num_pairs"] == ref["counts"][0]
    assert np.array_equal(got["tgt_from_src"], s["starts"][2])


def test_iteration_limits():
    s = S.loop_scene("pair")
    one = _icp(s, s["starts"][2], max_iterations=1)
    ref = NDI.icp(s["depth0"], s["intr"], s["depth1"], s["intr"], s["starts"][2], max_iterations=1)
    assert ref["status"] == "max_iterations" and not ref["fragile"]
    _against_restatement(one, ref)
    # eps = 0: no step is ever small enough; all 64 rounds run and stay at the fixed point
    full = _icp(s, s["starts"][1], max_iterations=64, eps_rotation=0.0, eps_translation=0.0)
    assert full["status"] == "max_iterations" and full["iterations"] == 64 and full["trace"].shape == (64, 4)
    assert set(full["trace"][2:, 0]) == {float(s["refs"][1]["num_pairs"])}
    assert np.abs(full["tgt_from_src"] - s["refs"][1]["tgt_from_src"]).max() < 1e-9
    assert full["trace"][8:, 2:].max() < 1e-12


def test_scaled_target_with_fixed_scale():
    s = S.loop_scene("pair")
    T = s["starts"][1].copy()
    T[:, 3] *= 1.7
    options = dict(s["options"], max_distance=0.17)
    ref = NDI.icp(s["depth0"], s["intr"], s["depth1"] * 1.7, s["intr"], T, scale=1.7, **options)
    assert not ref["fragile"] and ref["status"] == "converged"
    got = _icp(s, T, scale=1.7, depth1=s["depth1"] * 1.7, **options)
    _against_restatement(got, ref)
    plain = s["refs"][1]["tgt_from_src"]
    assert np.abs(got["tgt_from_src"][:, :3] - plain[:, :3]).max() < 1e-9 and np.abs(got["tgt_from_src"][:, 3] / 1.7 - plain[:, 3]).max() < 1e-9
    sim = refine_depth_pair(s["depth0"], s["depth1"] * 1.7, s["intr"], s["intr"], Sim3d(1.7, [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0]), **options)
    assert sim["tgt_from_src"].scale == 1.7 and sim["report"]["scale"] == 1.7


def test_argument_errors():
    s = S.loop_scene("pair")
    d0, d1, K, T = s["depth0"], s["depth1"], s["intr"], s["starts"][0]
    bad_T = T.copy()
    bad_T[1, 2] = np.nan
    calls = [
        lambda: capi.depth_pair_icp(d0[:2], K, d1, K, T), lambda: capi.depth_pair_icp(d0, K, d1[:, :2], K, T),
        lambda: capi.depth_pair_icp(d0, [0.0, 68.0, 1.0, 1.0], d1, K, T), lambda: capi.depth_pair_icp(d0, K, d1, [70.0, np.inf, 1.0, 1.0], T),
        lambda: capi.depth_pair_icp(d0, K, d1, K, bad_T), lambda: capi.depth_pair_icp(d0, K, d1, K, T, scale=0.0),
        lambda: capi.depth_pair_icp(d0, K, d1, K, T, scale=np.nan), lambda: capi.depth_pair_icp(d0, K, d1, K, T, scale=-1.0),
        lambda: capi.depth_pair_icp(d0, K, d1, K, T, max_iterations=0), lambda: capi.depth_pair_icp(d0, K, d1, K, T, max_iterations=65),
        lambda: capi.depth_pair_icp(d0, K, d1, K, T, min_pairs=5), lambda: capi.depth_pair_icp(d0, K, d1, K, T, stride=0),
        lambda: capi.depth_pair_icp(d0, K, d1, K, T, max_distance=0.0), lambda: capi.depth_pair_icp(d0, K, d1, K, T, max_angle_deg=181.0),
        lambda: capi.depth_pair_icp(d0, K, d1, K, T, edge_ratio=-0.1), lambda: capi.depth_pair_icp(d0, K, d1, K, T, eps_rotation=np.nan),
        lambda: capi.depth_pair_icp(d0, K, d1, K, T, eps_translation=-1.0), lambda: capi.depth_normals(d0, [70.0, 0.0, 1.0, 1.0]),
        lambda: capi.depth_normals(d0, K, edge_ratio=np.nan),
        lambda: capi.depth_pair_register_dense(d0, K, d1, K, np.zeros((4, 2)), np.zeros((4, 2)), [[0, 1]], icp=dict(stride=0)),
        lambda: capi.depth_pair_register_dense(d0[:2], K, d1, K, np.zeros((4, 2)), np.zeros((4, 2)), [[0, 1]]),
        lambda: capi.depth_pair_register_dense(d0, K, d1, K, np.zeros((4, 2)), np.zeros((4, 2)), [[0, 4]]),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(capi.MpsfmHipError) as e:
            call()
        assert e.value.code == -1, i  # MPSFM_EINVAL
    with pytest.raises(KeyError):
        capi.depth_pair_icp(d0, K, d1, K, T, pyramid=3)
    lib = capi.lib()
    Kc = np.ascontiguousarray(K)
    res, opt = capi.CIcpResult(), capi._icp_options({})
    import ctypes as C
    assert lib.mpsfm_depth_pair_icp(60, 80, None, Kc.ctypes.data, 60, 80, d1.ctypes.data, Kc.ctypes.data, T.ctypes.data, 1.0, C.byref(opt), 0, None,
                                    C.byref(res)) == -1
    assert lib.mpsfm_depth_pair_icp(60, 80, d0.ctypes.data, Kc.ctypes.data, 60, 80, d1.ctypes.data, Kc.ctypes.data, T.ctypes.data, 1.0, None, 0, None,
                                    C.byref(res)) == -1
    # data, not errors: a 1 x 1 normal map, a map of holes, a NULL trace
    n, v = capi.depth_normals(np.ones((1, 1)), K)
    assert n.shape == (1, 1, 3) and not n.any() and not v.any()
    Tc = np.ascontiguousarray(T)
    assert lib.mpsfm_depth_pair_icp(60, 80, d0.ctypes.data, Kc.ctypes.data, 60, 80, d1.ctypes.data, Kc.ctypes.data, Tc.ctypes.data, 1.0, C.byref(opt), 0,
                                    None, C.byref(res)) == 0
    assert res.status == 0 and 2 <= res.iterations <= s["refs"][0]["iterations"]
