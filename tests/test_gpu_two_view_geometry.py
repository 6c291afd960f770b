"""GPU checks of the two-view geometry estimator (csrc/two_view.hip through capi.two_view_geometry and the drop-ins): exact
agreement with the NumPy restatement on every configuration of the decision table, batch-size independence, run-to-run
identity, two concurrent host threads, failure cases and geometric verification of three camera pairs of a synthetic scene.

Bounds.  Integers, configs, masks and counters: exact.  E, F, H (canonical form), the pose and tri_angle (radians): 1e-9,
the project's bound for two routes to the same constant-size algebra (DESIGN.md sections 4g, 4h).  GRAM_BOUND is the wider
bound the issue allows for F and H where the local estimator takes the eigenvector of the 9 x 9 Gram matrix instead of the
SVD of the design matrix: 10 x the largest difference between the restatement's own two routes (SVD of the design matrix,
eigh of its Gram matrix) over the scenes below, measured on the CPU and recorded in DESIGN.md section 4j; it is not fitted to
HIP's output."""

import threading

import numpy as np
import pytest

import numpy_two_view_geometry as TV
from mpsfm_amd import capi
from mpsfm_amd.sfm.scene.correspondences import geometric_verification

pytestmark = pytest.mark.gpu

TOL = 1e-9
# restatement, SVD route against Gram route over SCENES (every decision the same): largest |dF| 3.4e-14, largest |dH| 4.1e-14
# (DESIGN.md section 4j); 10 x that is 4.1e-13, below TOL, so nothing is widened: F and H are held to TOL as well
GRAM_BOUND = max(TOL, 10 * 4.1e-14)

CAP = dict(max_num_trials=1500)  # where the restatement's runtime requires it (70 % outliers, large N), as section 4h's 80 % scenes
# (kind, n, outliers, noise_px, seed, options); every config of the decision table appears: general 2, wrong_intrinsics 3,
# planar 4, rotation 5, watermark 7 and weak 1 (10 planar inliers among 60 matches: no leg reaches min_num_inliers; with
# purely random matches the H leg ends on a tie of exact four-point fits, which rounding decides and the restatement
# reports as fragile on every draw)
SCENES = [("general", 50, 0.2, 0.0, 0, {}), ("general", 300, 0.5, 0.5, 1, {}), ("general", 2000, 0.7, 0.5, 2, CAP),
          ("general", 50000, 0.2, 0.5, 3, dict(max_num_trials=600)), ("wrong_intrinsics", 500, 0.2, 0.5, 4, {}),
          ("planar", 1000, 0.5, 0.5, 5, {}), ("planar", 5000, 0.2, 0.0, 6, {}), ("rotation", 800, 0.5, 0.5, 7, {}),
          ("rotation", 20000, 0.2, 0.5, 8, dict(max_num_trials=600)), ("watermark", 400, 0.2, 0.5, 9, {}),
          ("weak", 60, 0.83, 0.5, 10, dict(max_num_trials=600)), ("general", 5000, 0.5, 0.0, 11, CAP),
          ("wrong_intrinsics", 3000, 0.5, 0.0, 12, CAP), ("planar", 300, 0.7, 0.5, 14, CAP)]


def _args(s):
    return s["points1"], s["points2"], s["intr1"], s["intr2"], s["size1"], s["size2"]


def _robust_scene(kind, n, outliers, noise, seed, **opts):
    """a scene on which the restatement reports no fragile decision (the seed is redrawn otherwise, at most 6 draws)"""
    for k in range(6):
        s = TV.synthetic_pair(kind, n, outliers, 1000 * seed + k, noise)
        ref = TV.estimate(*_args(s), compute_relative_pose=True, seed=seed + k, **opts)
        if not ref["fragile"]:
            return s, ref, seed + k
    raise AssertionError(f"no robust scene for {(kind, n, outliers, noise, seed)}")


def _assert_matches(got, ref):
    assert got["config"] == ref["config"] and got["success"] == ref["success"]
    for k in "EFHT":
        if ref["legs"][k] is None:
            assert got["legs"][k]["num_trials"] == 0
            continue
        for f in ("success", "num_trials", "max_num_trials", "num_inliers"):
            assert got["legs"][k][f] == ref["legs"][k][f], (k, f, got["legs"][k], ref["legs"][k][f])
    assert np.array_equal(got["inlier_mask"], ref["inlier_mask"]) and got["num_inliers"] == ref["num_inliers"]
    assert got["num_cheirality_points"] == ref["num_cheirality_points"] and got["watermark"] == ref["watermark"]
    for k, tol in (("E", TOL), ("F", GRAM_BOUND), ("H", GRAM_BOUND)):
        if ref[k] is None:
            assert not got[k].any()
        else:
            d = np.abs(got[k] - ref[k]).max()
            print(f"|d{k}| = {d:.3e}")
            assert d < tol, (k, d)
    dP, dA = np.abs(got["cam2_from_cam1"] - ref["cam2_from_cam1"]).max(), abs(got["tri_angle"] - ref["tri_angle"])
    print(f"|dP| = {dP:.3e} |dtri| = {dA:.3e}")
    assert dP < TOL and dA < TOL


@pytest.mark.parametrize("kind,n,outliers,noise,seed,opts", SCENES)
def test_hip_matches_restatement(kind, n, outliers, noise, seed, opts):
    s, ref, sd = _robust_scene(kind, n, outliers, noise, seed, **opts)
    got = capi.two_view_geometry(*_args(s), compute_relative_pose=True, seed=sd, **opts)
    assert ref["config"] == s["expect"]
    _assert_matches(got, ref)
    if kind == "general" and outliers < 0.7:
        assert np.abs(got["cam2_from_cam1"][:, :3] - s["R"]).max() < 5e-2 and got["tri_angle"] > 0


def _same(a, b):
    assert a["config"] == b["config"]
    for k in a["legs"]:  # everything but the number of batches, which is what the batch size changes
        assert {f: v for f, v in a["legs"][k].items() if f != "num_batches"} == {f: v for f, v in b["legs"][k].items() if f != "num_batches"}
    assert np.array_equal(a["inlier_mask"], b["inlier_mask"])
    for k in ("E", "F", "H", "cam2_from_cam1"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (a["tri_angle"], a["num_cheirality_points"], a["num_inliers"], a["watermark"]) == \
        (b["tri_angle"], b["num_cheirality_points"], b["num_inliers"], b["watermark"])


@pytest.mark.parametrize("batch", [1, 7, 256])
@pytest.mark.parametrize("kind", ["general", "planar", "watermark"])
def test_batch_size_does_not_change_the_result(kind, batch):
    s = TV.synthetic_pair(kind, 3000, 0.5, seed=21, noise_px=0.5)
    o = dict(compute_relative_pose=True, seed=5, max_num_trials=700)
    _same(capi.two_view_geometry(*_args(s), **o), capi.two_view_geometry(*_args(s), batch_trials=batch, **o))


def test_two_calls_are_bitwise_identical():
    s = TV.synthetic_pair("general", 20000, 0.5, seed=31, noise_px=0.5)
    a = capi.two_view_geometry(*_args(s), compute_relative_pose=True, seed=3)
    b = capi.two_view_geometry(*_args(s), compute_relative_pose=True, seed=3)
    _same(a, b)
    assert a["legs"] == b["legs"] and a["config"] == 2


def test_two_host_threads_agree_with_the_serial_result():
    scenes = [TV.synthetic_pair(kind, 4000, 0.4, seed=41 + i, noise_px=0.5) for i, kind in enumerate(("general", "planar"))]
    o = dict(compute_relative_pose=True, seed=2)
    serial = [capi.two_view_geometry(*_args(s), **o) for s in scenes]
    out, err = [None, None], []

    def work(i):
        try:
            for _ in range(3):
                out[i] = capi.two_view_geometry(*_args(scenes[i]), **o)
        except Exception as e:  # noqa: BLE001
            err.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not err, err
    for a, b in zip(serial, out):
        _same(a, b)
        assert a["legs"] == b["legs"]


def test_failures_match_restatement():
    K1, K2 = np.array(TV.NR.INTR1), np.array(TV.NR.INTR2)
    sizes = (TV.SIZE1, TV.SIZE2)
    # every match the same pixel pair: no sample of any leg has a model
    p1 = np.tile([[400.0, 300.0]], (40, 1))
    p2 = np.tile([[350.0, 320.0]], (40, 1))
    ref = TV.estimate(p1, p2, K1, K2, *sizes, max_num_trials=200, compute_relative_pose=True)
    got = capi.two_view_geometry(p1, p2, K1, K2, *sizes, max_num_trials=200, compute_relative_pose=True)
    assert ref["config"] == got["config"] == 1 and not got["success"] and not got["inlier_mask"].any()
    for k in "EFH":
        assert got["legs"][k]["num_trials"] == ref["legs"][k]["num_trials"] == 200 and not got["legs"][k]["success"]
        assert got["legs"][k]["num_inliers"] == 0 and not got[k].any()
    assert np.array_equal(got["cam2_from_cam1"], np.eye(3, 4)) and got["tri_angle"] == 0.0
    # 14 matches: below min_num_inliers, nothing runs
    s = TV.synthetic_pair("general", 14, 0.0, seed=2)
    got = capi.two_view_geometry(*_args(s), compute_relative_pose=True)
    assert got["config"] == TV.estimate(*_args(s))["config"] == 1 and not got["inlier_mask"].any() and len(got["inlier_mask"]) == 14
    assert all(v["num_trials"] == 0 for v in got["legs"].values())
    # random matches: every leg "succeeds" with a handful of inliers and runs its whole (capped) budget
    for sd in range(2):
        s = TV.synthetic_pair("random", 60, 0.0, seed=50 + sd)
        ref = TV.estimate(*_args(s), seed=sd, max_num_trials=600, compute_relative_pose=True)
        got = capi.two_view_geometry(*_args(s), seed=sd, max_num_trials=600, compute_relative_pose=True)
        for k in "EFH":
            assert got["legs"][k]["num_trials"] == ref["legs"][k]["num_trials"] == 600
        assert max(ref["legs"][k]["num_inliers"] for k in "EFH") < 15
        if not ref["fragile"]:
            assert got["config"] == ref["config"] == 1
            for k in "EFH":
                assert got["legs"][k]["num_inliers"] == ref["legs"][k]["num_inliers"]
            assert np.array_equal(got["inlier_mask"], ref["inlier_mask"])


class _Cam:
    def __init__(self, params, size):
        self.model, self.params, self.width, self.height = "PINHOLE", np.asarray(params, np.float64), size[0], size[1]


class _Image:
    def __init__(self, name, image_id, camera_id):
        self.name, self.image_id, self.camera_id = name, image_id, camera_id


class _Reconstruction:
    def __init__(self):
        self.images, self.cameras = {}, {}


def test_end_to_end_geometric_verification_of_three_scene_pairs():
    """Three camera pairs of a synthetic scene: the exact projections of their common landmarks as keypoints, 10 % of the
    second view's moved by up to 80 px and at least 40 px off their epipolar line."""
    from mpsfm_amd.synthetic import R_from_quat, make_scene

    prob, truth = make_scene(6, 3000, False, seed=4, outlier_frac=0.1)
    rng = np.random.default_rng(7)
    rec, kps, matches, want = _Reconstruction(), {}, {}, {}
    pairs = [(0, 1), (1, 2), (2, 3)]
    for a, b in pairs:
        K = prob.cam_intr[prob.cam_intr_idx[a]]
        size = (int(round(2 * K[2])), int(round(2 * K[3])))
        common = sorted(set(prob.obs_pt[prob.obs_cam == a].tolist()) & set(prob.obs_pt[prob.obs_cam == b].tolist()))
        assert len(common) > 500
        X = truth["pts"][np.array(common)]
        Ra, Rb = R_from_quat(truth["cam_quat"][a])[0], R_from_quat(truth["cam_quat"][b])[0]
        ta, tb = truth["cam_t"][a], truth["cam_t"][b]

        def project(R, t, K=K, X=X):
            Y = X @ R.T + t
            return np.c_[K[0] * Y[:, 0] / Y[:, 2] + K[2], K[1] * Y[:, 1] / Y[:, 2] + K[3]]

        pa, pb = project(Ra, ta), project(Rb, tb)
        Rr = Rb @ Ra.T
        tr = tb - Rr @ ta
        # a displaced match must be an outlier: more than 10 max_error from its epipolar line, as numpy_relative_pose's
        # synthetic problems place theirs (one that stays within max_error is an inlier with up to 4 px of error, and the bounds
        # below are those of exact inliers)
        Ki = np.linalg.inv(TV.Kmat(K))
        F = Ki.T @ np.array([[0, -tr[2], tr[1]], [tr[2], 0, -tr[0]], [-tr[1], tr[0], 0]]) @ Rr @ Ki
        for i in np.nonzero(rng.random(len(common)) < 0.1)[0]:
            line = F @ np.r_[pa[i], 1.0]
            while True:
                q = pb[i] + rng.uniform(-80, 80, 2)
                if abs(line @ np.r_[q, 1.0]) > 40.0 * np.hypot(line[0], line[1]):
                    break
            pb[i] = q
        names = (f"im{a}_{b}_0.jpg", f"im{a}_{b}_1.jpg")
        for j, (name, kp) in enumerate(zip(names, (pa, pb))):
            iid = 10 * a + j + 1
            rec.images[iid] = _Image(name, iid, iid)
            rec.cameras[iid] = _Cam(K, size)
            kps[name] = kp
        perm = rng.permutation(len(common))
        matches[names] = np.c_[perm, perm].astype(np.int32)
        Xa = X @ Ra.T + ta
        ang = TV.triangulation_angle(np.zeros(3), -Rr.T @ tr, Xa)
        want[names] = (Rr, tr / np.linalg.norm(tr), float(np.median(ang)), len(common))
    masks, cache = geometric_verification(rec, list(want), max_error=4.0, keypoints=kps, matches=matches)
    for names, (Rr, tr, ang, n) in want.items():
        tvg = cache[names]
        assert tvg.config == 2
        assert masks[names].sum() >= 0.85 * n and len(tvg.inlier_matches) == masks[names].sum()
        M = tvg.cam2_from_cam1.matrix()
        assert np.abs(M[:, :3] - Rr).max() < 1e-3
        assert np.arccos(np.clip(M[:, 3] @ tr / np.linalg.norm(M[:, 3]), -1, 1)) < 1e-2
        print("tri_angle", tvg.tri_angle, "truth", ang)
        assert abs(tvg.tri_angle - ang) <= 0.1 * ang
