"""GPU checks of the relative-pose estimator (csrc/rel_pose.hip through capi.rel_pose_estimate and the drop-in
RelativePose): exact agreement with the NumPy restatement, batch-size independence, run-to-run identity, failure cases
and one end-to-end relative pose of two cameras of a synthetic scene."""

import numpy as np
import pytest

import numpy_relative_pose as NR
from mpsfm_amd import capi
from mpsfm_amd.sfm.estimators import RelativePose

pytestmark = pytest.mark.gpu

# (n, outliers, seed, noise_px, planar); 80 % outliers would need ~86 000 trials: those scenes cap max_num_trials
SCENES = [(50, 0.2, 0, 0.0, False), (50, 0.5, 1, 0.5, False), (120, 0.8, 2, 0.5, False), (300, 0.2, 3, 0.5, False),
          (300, 0.5, 4, 0.0, False), (1000, 0.8, 5, 0.5, False), (2000, 0.2, 6, 0.5, False), (2000, 0.5, 7, 0.0, False),
          (5000, 0.5, 8, 0.5, False), (20000, 0.2, 9, 0.5, False), (50000, 0.5, 10, 0.5, False), (800, 0.5, 11, 0.5, True)]


class _Cam:
    def __init__(self, params, model="PINHOLE"):
        self.model, self.params = model, np.asarray(params, np.float64)


def _opts(outliers):
    return dict(max_num_trials=1500) if outliers >= 0.8 else {}


def _robust_scene(n, outliers, seed, noise_px=0.5, planar=False, **opts):
    """a scene on which the restatement reports no fragile decision (the seed is redrawn otherwise)"""
    for k in range(6):
        p1, p2, K1, K2, R, t, inl = NR.synthetic_problem(n, outliers, seed=1000 * seed + k, noise_px=noise_px, planar=planar)
        ref = NR.estimate(p1, p2, K1, K2, seed=seed + k, **opts)
        if not ref["fragile"]:
            return p1, p2, K1, K2, R, t, inl, ref, seed + k
    raise AssertionError(f"no robust scene for {(n, outliers, seed)}")


@pytest.mark.parametrize("n,outliers,seed,noise,planar", SCENES)
def test_hip_matches_restatement(n, outliers, seed, noise, planar):
    o = _opts(outliers)
    p1, p2, K1, K2, R, t, inl, ref, s = _robust_scene(n, outliers, seed, noise, planar, **o)
    got = capi.rel_pose_estimate(p1, p2, K1, K2, seed=s, **o)
    assert got["success"] == ref["success"] is True
    assert got["num_trials"] == ref["num_trials"]
    assert got["max_num_trials"] == ref["max_num_trials"]
    assert got["num_inliers"] == ref["num_inliers"]
    assert np.array_equal(got["inlier_mask"], ref["inlier_mask"])
    assert got["num_cheirality_points"] == ref["num_cheirality_points"]
    assert np.abs(got["E"] - ref["E"]).max() < 1e-9
    assert np.abs(got["cam2_from_cam1"] - ref["cam2_from_cam1"]).max() < 1e-9
    if not planar and outliers < 0.8:  # the 80 % scenes stop at a capped budget, with whatever model it found
        assert np.abs(got["cam2_from_cam1"] - np.c_[R, t]).max() < 5e-2


@pytest.mark.parametrize("batch", [1, 7, 256, 4096])
def test_batch_size_does_not_change_the_result(batch):
    p1, p2, K1, K2, R, t, inl = NR.synthetic_problem(3000, 0.6, seed=21, noise_px=0.5)
    base = capi.rel_pose_estimate(p1, p2, K1, K2, seed=5)
    got = capi.rel_pose_estimate(p1, p2, K1, K2, seed=5, batch_trials=batch)
    for k in ("success", "num_trials", "num_inliers", "lo_rounds", "num_cheirality_points"):
        assert got[k] == base[k]
    assert np.array_equal(got["inlier_mask"], base["inlier_mask"])
    assert got["E"].tobytes() == base["E"].tobytes()
    assert got["cam2_from_cam1"].tobytes() == base["cam2_from_cam1"].tobytes()


def test_two_calls_are_bitwise_identical():
    p1, p2, K1, K2, R, t, inl = NR.synthetic_problem(20000, 0.5, seed=31, noise_px=0.5)
    a = capi.rel_pose_estimate(p1, p2, K1, K2, seed=3)
    b = capi.rel_pose_estimate(p1, p2, K1, K2, seed=3)
    assert a["E"].tobytes() == b["E"].tobytes()
    assert a["cam2_from_cam1"].tobytes() == b["cam2_from_cam1"].tobytes()
    assert np.array_equal(a["inlier_mask"], b["inlier_mask"])
    assert (a["num_trials"], a["num_inliers"], a["lo_rounds"]) == (b["num_trials"], b["num_inliers"], b["lo_rounds"])


def test_failures_match_restatement():
    rp = RelativePose()
    K1, K2 = np.array(NR.INTR1), np.array(NR.INTR2)
    # every match the same pixel pair: every sample's Q has rank 1, no model
    p1 = np.tile([[400.0, 300.0]], (40, 1))
    p2 = np.tile([[350.0, 320.0]], (40, 1))
    assert NR.estimate(p1, p2, K1, K2, max_num_trials=200)["success"] is False
    got = capi.rel_pose_estimate(p1, p2, K1, K2, max_num_trials=200, min_num_trials=100)
    assert got["success"] is False and got["num_trials"] == 200 and not got["inlier_mask"].any()
    assert rp(p1, p2, _Cam(K1), _Cam(K2)) is None
    # five matches, two of them coincident
    q1 = np.array([[100.0, 100.0], [100.0, 100.0], [500.0, 120.0], [300.0, 700.0], [900.0, 400.0]])
    q2 = np.array([[110.0, 90.0], [110.0, 90.0], [520.0, 130.0], [280.0, 690.0], [870.0, 420.0]])
    assert NR.estimate(q1, q2, K1, K2)["success"] is False
    assert rp(q1, q2, _Cam(K1), _Cam(K2)) is None
    # all matches random: a minimal sample explains itself, so LORANSAC "succeeds" with a handful of inliers and runs its
    # whole (capped) budget.  The mask is compared when the restatement reports no fragile decision.
    rng = np.random.default_rng(3)
    r1 = np.c_[rng.uniform(0, 1280, 400), rng.uniform(0, 960, 400)]
    r2 = np.c_[rng.uniform(0, 1200, 400), rng.uniform(0, 1000, 400)]
    for s in range(2):
        ref = NR.estimate(r1, r2, K1, K2, seed=s, max_num_trials=1500)
        got = capi.rel_pose_estimate(r1, r2, K1, K2, seed=s, max_num_trials=1500)
        assert got["success"] == ref["success"]
        assert got["num_trials"] == ref["num_trials"] == 1500
        assert ref["num_inliers"] < 40
        if not ref["fragile"]:
            assert got["num_inliers"] == ref["num_inliers"]
            assert np.array_equal(got["inlier_mask"], ref["inlier_mask"])


def test_end_to_end_relative_pose_of_two_scene_cameras():
    """Two cameras of a synthetic scene: the exact projections of their common landmarks, 10 % of the second view's moved by
    up to 80 px.  RANSAC's pose is not refined (neither is pycolmap's), so the inliers carry no noise here."""
    from mpsfm_amd.synthetic import R_from_quat, make_scene

    prob, truth = make_scene(6, 3000, False, seed=4, outlier_frac=0.1)
    c1, c2 = 1, 2
    K = prob.cam_intr[prob.cam_intr_idx[c1]]
    R1, R2 = R_from_quat(truth["cam_quat"][c1])[0], R_from_quat(truth["cam_quat"][c2])[0]
    t1, t2 = truth["cam_t"][c1], truth["cam_t"][c2]
    common = sorted(set(prob.obs_pt[prob.obs_cam == c1].tolist()) & set(prob.obs_pt[prob.obs_cam == c2].tolist()))
    assert len(common) > 500
    X = truth["pts"][np.array(common)]

    def project(R, t):
        Y = X @ R.T + t
        return np.c_[K[0] * Y[:, 0] / Y[:, 2] + K[2], K[1] * Y[:, 1] / Y[:, 2] + K[3]]

    rng = np.random.default_rng(7)
    a, b = project(R1, t1), project(R2, t2)
    out = rng.random(len(common)) < 0.1
    b[out] += rng.uniform(-80, 80, (int(out.sum()), 2))
    res = RelativePose()(a, b, _Cam(K), _Cam(K))
    assert res is not None and res["num_inliers"] >= 0.85 * len(common)
    Rr = R2 @ R1.T
    tr = t2 - Rr @ t1
    tr = tr / np.linalg.norm(tr)
    M = res["cam2_from_cam1"].matrix()
    assert np.abs(M[:, :3] - Rr).max() < 1e-3
    assert np.arccos(np.clip(M[:, 3] @ tr, -1, 1)) < 1e-2
    q = res["cam2_from_cam1"].rotation.quat
    assert q.shape == (4,) and abs(np.linalg.norm(q) - 1) < 1e-12
    assert np.abs(res["cam2_from_cam1"].translation - M[:, 3]).max() == 0
    assert res["E"].shape == (3, 3) and res["inlier_mask"].shape == (len(common),)
