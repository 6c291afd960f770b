"""GPU checks of the absolute-pose estimator (csrc/abs_pose.hip through capi.abs_pose_estimate and the drop-in
AbsolutePose): exact agreement with the NumPy restatement, refinement against the CPU oracle, failure cases, run-to-run
identity and one end-to-end registration on a synthetic scene."""

import numpy as np
import pytest

import numpy_absolute_pose as NA
from mpsfm_amd import capi
from mpsfm_amd.sfm.estimators import AbsolutePose

pytestmark = pytest.mark.gpu

SCENES = [(50, 0.2, 0), (50, 0.5, 1), (120, 0.7, 2), (300, 0.2, 3), (300, 0.5, 4), (1000, 0.7, 5), (2000, 0.2, 6), (2000, 0.5, 7),
          (5000, 0.7, 8), (12000, 0.5, 9), (30000, 0.2, 10), (30000, 0.7, 11), (800, 0.5, 12), (4000, 0.2, 13)]


class _Cam:
    def __init__(self, params, model="PINHOLE"):
        self.model, self.params = model, np.asarray(params, np.float64)


def _robust_scene(n, outliers, seed, noise_px=0.3):
    """a scene on which the restatement reports no fragile decision (the seed is redrawn otherwise)"""
    for k in range(8):
        p2, X, K, R, t, inl = NA.synthetic_problem(n, outliers, seed=1000 * seed + k, noise_px=noise_px)
        ref = NA.estimate(p2, X, K, seed=seed + k)
        if not ref["fragile"]:
            return p2, X, K, R, t, inl, ref, seed + k
    raise AssertionError(f"no robust scene for {(n, outliers, seed)}")


@pytest.mark.parametrize("n,outliers,seed", SCENES)
def test_hip_matches_restatement(n, outliers, seed):
    p2, X, K, R, t, inl, ref, s = _robust_scene(n, outliers, seed)
    got = capi.abs_pose_estimate(p2, X, K, seed=s)
    assert got["success"] == ref["success"]
    assert got["num_trials"] == ref["num_trials"]
    assert got["max_num_trials"] == ref["max_num_trials"] == 2194
    assert got["num_inliers"] == ref["num_inliers"]
    assert np.array_equal(got["inlier_mask"], ref["inlier_mask"])
    # lo_rounds is not compared: EPnP on a 4- or 5-point inlier set is ill-conditioned, and the two implementations may take
    # a different number of rounds to the same final inlier set
    assert np.abs(got["cam_from_world"] - ref["cam_from_world"]).max() < 1e-9
    assert np.abs(got["cam_from_world"] - np.c_[R, t]).max() < 1e-2


@pytest.mark.parametrize("batch", [1, 7, 100, 4096])
def test_batch_size_does_not_change_the_result(batch):
    p2, X, K, R, t, inl, ref, s = _robust_scene(3000, 0.6, 21)
    base = capi.abs_pose_estimate(p2, X, K, seed=s)
    got = capi.abs_pose_estimate(p2, X, K, seed=s, batch_trials=batch)
    for k in ("success", "num_trials", "num_inliers", "lo_rounds"):
        assert got[k] == base[k] == ref[k]
    assert np.array_equal(got["inlier_mask"], base["inlier_mask"])
    assert np.array_equal(got["cam_from_world"], base["cam_from_world"])


def test_refined_pose_matches_cpu_oracle():
    from oracle import cpu_oracle as O

    p2, X, K, R, t, inl = NA.synthetic_problem(1500, 0.4, seed=77, noise_px=0.5)
    ap = AbsolutePose()
    res = ap(p2, X, _Cam(K))
    assert res is not None
    est, hip = ap.last_estimate, ap.last_refinement
    prob = ap.refinement_problem(est["cam_from_world"], p2[est["inlier_mask"]], X[est["inlier_mask"]], K)
    ora = O.solve(prob, O.default_options(max_num_iterations=100, gradient_tolerance=1.0))
    q = res["cam_from_world"].rotation.quat
    q = q if np.dot(q, prob.cam_quat[0]) >= 0 else -q
    assert np.abs(q - prob.cam_quat[0]).max() < 1e-8
    assert np.abs(res["cam_from_world"].translation - prob.cam_t[0]).max() < 1e-8
    assert hip["num_iterations"] == ora["num_iterations"]
    assert hip["termination"] == ora["termination"]
    assert abs(hip["final_cost"] - ora["final_cost"]) <= 1e-8 * ora["final_cost"]
    assert res["num_inliers"] == est["num_inliers"] and np.array_equal(res["inlier_mask"], est["inlier_mask"])
    assert hip["final_cost"] <= hip["initial_cost"]
    assert np.abs(res["cam_from_world"].matrix() - np.c_[R, t]).max() < 1e-2


def test_failures_match_restatement():
    ap = AbsolutePose()
    rng = np.random.default_rng(3)
    K = np.array([820.0, 790.0, 640.0, 480.0])
    # collinear world points: every minimal sample is degenerate
    X = np.outer(rng.uniform(-1, 1, 200), [1.0, 2.0, -0.5]) + [0.3, 0.1, 6.0]
    p2 = rng.uniform(0, 1000, (200, 2))
    assert NA.estimate(p2, X, K)["success"] is False
    assert capi.abs_pose_estimate(p2, X, K)["success"] is False
    assert ap(p2, X, _Cam(K)) is None
    # N = 3 with a degenerate triangle (two coincident points)
    X3 = np.array([[0.0, 0.0, 5.0], [0.0, 0.0, 5.0], [1.0, 0.5, 6.0]])
    p3 = np.array([[640.0, 480.0], [640.0, 480.0], [800.0, 550.0]])
    assert NA.estimate(p3, X3, K)["success"] is False
    assert ap(p3, X3, _Cam(K)) is None
    # every point behind the camera in every hypothesis is impossible for P3P, but all coincident points give no model
    Xc = np.tile([[0.2, 0.1, 4.0]], (50, 1))
    assert ap(rng.uniform(0, 1000, (50, 2)), Xc, _Cam(K)) is None
    # all pairs outliers (random pixels): a minimal sample explains itself, so LORANSAC "succeeds" with a handful of inliers
    # and runs its whole trial budget.  Which of the samples that fit only themselves wins is rounding noise: the mask is
    # compared only when the restatement reports no such tie.
    Xr = rng.uniform(-2, 2, (400, 3)) + [0, 0, 8]
    pr = rng.uniform(0, 1280, (400, 2))
    for s in range(3):
        ref = NA.estimate(pr, Xr, K, seed=s)
        got = capi.abs_pose_estimate(pr, Xr, K, seed=s)
        assert got["success"] == ref["success"] and got["num_inliers"] == ref["num_inliers"]
        assert got["num_trials"] == ref["num_trials"] == 2194
        assert ref["num_inliers"] < 20
        if not ref["fragile"]:
            assert np.array_equal(got["inlier_mask"], ref["inlier_mask"])


def test_two_calls_are_bitwise_identical():
    p2, X, K, R, t, inl = NA.synthetic_problem(20000, 0.5, seed=31, noise_px=0.5)
    a = capi.abs_pose_estimate(p2, X, K, seed=3)
    b = capi.abs_pose_estimate(p2, X, K, seed=3)
    assert a["cam_from_world"].tobytes() == b["cam_from_world"].tobytes()
    assert np.array_equal(a["inlier_mask"], b["inlier_mask"])
    assert (a["num_trials"], a["num_inliers"], a["lo_rounds"]) == (b["num_trials"], b["num_inliers"], b["lo_rounds"])
    ap = AbsolutePose()
    r1, r2 = ap(p2, X, _Cam(K)), ap(p2, X, _Cam(K))
    assert r1["cam_from_world"].matrix().tobytes() == r2["cam_from_world"].matrix().tobytes()


def test_end_to_end_registration_of_a_scene_image():
    from mpsfm_amd.synthetic import R_from_quat, make_scene
    from numpy_scene import NumpyImage, Rigid3d

    prob, truth = make_scene(6, 3000, False, seed=4, outlier_frac=0.1)
    c = 3
    sel = prob.obs_cam == c
    p2, p3 = prob.obs_xy[sel], truth["pts"][prob.obs_pt[sel]]
    K = prob.cam_intr[0]
    # depth-lifted keypoints: pixels of the image unprojected with the true pose at a depth with 0.5 % noise
    rng = np.random.default_rng(9)
    R, t = R_from_quat(truth["cam_quat"][c])[0], truth["cam_t"][c]
    kp = np.c_[rng.uniform(0, 2 * K[2], 4000), rng.uniform(0, 2 * K[3], 4000)]
    d = rng.uniform(4.0, 9.0, 4000)
    Xc = np.c_[(kp[:, 0] - K[2]) / K[0], (kp[:, 1] - K[3]) / K[1], np.ones(4000)] * (d * (1 + 0.005 * rng.normal(size=4000)))[:, None]
    lifted = (Xc - t) @ R
    img = NumpyImage(c, 1, Rigid3d(prob.cam_quat[c], prob.cam_t[c]), np.r_[p2, kp])
    res = AbsolutePose()(np.r_[p2, kp], np.r_[p3, lifted], _Cam(K))
    assert res is not None and res["num_inliers"] > 0.8 * (len(p2) + 4000) * 0.9
    img.cam_from_world = res["cam_from_world"]
    M = img.cam_from_world.matrix()
    assert np.abs(M[:, :3] - R).max() < 1e-3
    assert np.abs(M[:, 3] - t).max() < 1e-2 * max(1.0, np.linalg.norm(t))
    assert img.cam_from_world.rotation.quat.shape == (4,)


def test_refinement_takes_the_single_launch_solver():
    import ctypes as C

    p2, X, K, R, t, inl = NA.synthetic_problem(2000, 0.0, seed=41, noise_px=0.5)
    ap = AbsolutePose()
    prob = ap.refinement_problem(np.c_[R, t], p2, X, K)
    L = capi.lib()
    with capi.BAHandle(prob, ap.solver_options()) as h:
        s = h.solve()
        clk = (C.c_int64 * 12)()
        assert L.mpsfm_debug_local_clocks(h._h, clk) == 1
        assert int(clk[6]) == s["num_iterations"] >= 1
