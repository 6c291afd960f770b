"""mpsfm_registration_pairs / mpsfm_init_pair_candidates (csrc/registration.hip) on the device: against the reference's
own results (tests/golden/reference_registration.npz), against the NumPy restatement at size, the two-view triangulation
against mpsfm_tri_estimate_batch bit for bit, the drop-in MpsfmRegistration end to end on a NumPy scene, run to run and
from two host threads.  Bounds as in test_registration_cpu.py (derived there).  Every device step runs under a time limit
of its own (a worker thread that is given up on when it does not come back)."""

import threading

import numpy as np
import pytest

import numpy_registration as NR
from mpsfm_amd import capi
from mpsfm_amd.sfm.mapper import MpsfmRegistration
from mpsfm_amd.synthetic import R_from_quat, make_scene
from test_registration_cpu import (COLMAP_OPTIONS, EPS, angle_bound_deg, ap_answers, assert_lift_close, check_init_candidates,
                                   spec_of)

pytestmark = pytest.mark.gpu

FRAGILE_CAP = 0.001  # at most 0.1 % of the matches of a case may be left out of the exact comparisons


@pytest.fixture(scope="module")
def Z():
    import os

    from test_registration_cpu import ROOT

    return np.load(os.path.join(ROOT, "tests", "golden", "reference_registration.npz"))


def limited(fn, seconds=120):
    """runs one device step in a worker thread; the test fails when it is not back in time"""
    box = {}

    def work():
        try:
            box["out"] = fn()
        except BaseException as e:  # noqa: BLE001 - handed to the test thread
            box["err"] = e

    t = threading.Thread(target=work, daemon=True)
    t.start()
    t.join(seconds)
    assert not t.is_alive(), f"device step still running after {seconds} s"
    if "err" in box:
        raise box["err"]
    return box["out"]


class HipBackend:
    """capi under a time limit, with the restatement's error scales beside every registration_pairs call"""

    def __init__(self):
        self.pairs = []

    def registration_pairs(self, refs, match_ref, ref_xy, match_pt, pts, pt_risky=None, lifted_registration=True, device=0):
        r = NR.registration_pairs(refs, match_ref, ref_xy, match_pt, pts, pt_risky, lifted_registration)
        xyz, kind = limited(lambda: capi.registration_pairs(refs, match_ref, ref_xy, match_pt, pts, pt_risky=pt_risky,
                                                            lifted_registration=lifted_registration, device=device))
        assert np.array_equal(kind, r["kind"])
        self.pairs.append(r)
        return xyz, kind

    @staticmethod
    def init_pair_candidates(*a, **k):
        return limited(lambda: capi.init_pair_candidates(*a, **k))


# ---- the reference's own results --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["next_lifted", "next_plain", "next_resample_taken"])
def test_hip_pairs_equal_the_reference_fixture(Z, tag):
    min_inliers, half, best, lifted, resample = (int(v) for v in Z[f"{tag}_conf"])
    scene, corr = NR.registration_scene(spec_of(Z, "next"), risky_ids=Z["next_risky"])
    scene.best_next_ref_imid = best
    backend = HipBackend()
    reg = MpsfmRegistration({"lifted_registration": bool(lifted), "resample_bunlde": bool(resample), "verbose": -1,
                             "colmap_options": dict(COLMAP_OPTIONS, abs_pose_min_num_inliers=min_inliers)}, scene, corr, None, backend=backend)
    reg.absolute_pose_estimator = NR.ReplayEstimator(ap_answers(Z, tag))
    assert reg.register_next_image(6) == bool(Z[f"{tag}_return"])
    calls = reg.absolute_pose_estimator.calls
    assert len(calls) == int(Z[f"{tag}_ap_calls"])
    for i, (p2, p3, _) in enumerate(calls):
        assert np.array_equal(p2, Z[f"{tag}_ap{i}_points2D"])
        want, r = Z[f"{tag}_ap{i}_points3D"], backend.pairs[i]
        n_tri = len(np.unique(Z[f"{tag}_pass{i}_ids3d"]))
        assert np.array_equal(p3[:n_tri], want[:n_tri])
        assert_lift_close(p3[n_tri:], want[n_tri:], r["scale"][r["kind"] == NR.LIFTED])
    assert np.array_equal(np.concatenate(list(scene.last_ap_inlier_masks.values())), Z[f"{tag}_mask_values"])
    for r in scene.images[6].ignore_matches_AP:
        assert np.array_equal(scene.images[6].ignore_matches_AP[r], Z[f"{tag}_ignore_ref{r}"])


@pytest.mark.parametrize("kind", ["high", "low", "none"])
def test_hip_init_candidates_equal_the_reference_fixture(Z, kind):
    check_init_candidates(Z, kind, HipBackend.init_pair_candidates)


# ---- at size against the restatement ----------------------------------------------------------------------------------------
def big_pairs(seed, n_refs=6, n=50000, n_pts=20000, H=290, W=387):
    rng = np.random.default_rng(seed)
    refs = []
    for r in range(n_refs):
        q = np.array([0.0, 0.0, 0.0, 1.0]) if r == 0 else np.r_[rng.normal(0, 0.3, 3), 1.0]
        q /= np.linalg.norm(q)
        f = rng.uniform(500, 700)
        refs.append(dict(depth_map=rng.uniform(0.5, 9.0, (H, W)), sx=W / 774.0, sy=H / 580.0, intr=[f, f * 1.01, 387 + rng.normal(0, 3), 290 + rng.normal(0, 3)],
                         quat_xyzw=q, t=np.zeros(3) if r == 0 else rng.normal(0, 2, 3)))  # reference 0 at the identity: xyz.z IS the sample
    match_ref = rng.integers(0, n_refs, n).astype(np.int32)
    ref_xy = np.stack([rng.uniform(-15, 789, n), rng.uniform(-15, 595, n)], 1)  # some outside the maps: zero padding
    match_pt = np.where(rng.uniform(size=n) < 0.4, rng.integers(0, n_pts, n), -1).astype(np.int32)
    return dict(refs=refs, match_ref=match_ref, ref_xy=ref_xy, match_pt=match_pt, pts=rng.normal(0, 4, (n_pts, 3)),
                pt_risky=rng.uniform(size=n_pts) < 0.2)


@pytest.mark.parametrize("lifted", [True, False])
def test_hip_pairs_equal_the_restatement_at_size(lifted):
    a = big_pairs(20261016)
    want = NR.registration_pairs(lifted_registration=lifted, **a)
    xyz, kind, ms = limited(lambda: capi.registration_pairs(lifted_registration=lifted, return_ms=True, **a))
    assert np.array_equal(kind, want["kind"])
    assert set(np.unique(kind)) == ({1, 2} if lifted else {0, 1})
    tri, lift = kind == NR.TRIANGULATED, kind == NR.LIFTED
    assert np.array_equal(xyz[tri], want["xyz"][tri]) and not xyz[kind == NR.DROPPED].any()
    assert_lift_close(xyz[lift], want["xyz"][lift], want["scale"][lift])
    if lifted:
        at_identity = lift & (a["match_ref"] == 0)
        assert at_identity.sum() > 3000
        assert np.array_equal(xyz[at_identity, 2], want["d"][at_identity])  # the sampled depth, bit for bit
        assert (want["d"][lift] == 0).any()  # keypoints beyond the border
    assert 0 < ms < 50


def big_init(seed, n=50000, H=290, W=387):
    rng = np.random.default_rng(seed)
    K1, K2 = [600.0, 605.0, 390.0, 288.0], [590.0, 600.0, 380.0, 295.0]
    q = np.r_[rng.normal(0, 0.03, 3), 1.0]
    R2 = R_from_quat(q / np.linalg.norm(q))[0]
    P2 = np.c_[R2, -R2 @ np.array([1.0, 0.05, -0.03])]
    xy1 = np.stack([rng.uniform(-10, 784, n), rng.uniform(-10, 590, n)], 1)
    z = rng.uniform(3.0, 40.0, n)
    X = np.stack([(xy1[:, 0] - K1[2]) / K1[0] * z, (xy1[:, 1] - K1[3]) / K1[1] * z, z], 1)
    Xc = X @ P2[:, :3].T + P2[:, 3]
    xy2 = np.stack([K2[0] * Xc[:, 0] / Xc[:, 2] + K2[2], K2[1] * Xc[:, 1] / Xc[:, 2] + K2[3]], 1) + rng.normal(0, 0.5, (n, 2))
    wrong = rng.uniform(size=n) < 0.1
    xy2[wrong] = rng.uniform(0, 700, (int(wrong.sum()), 2))
    prior = rng.uniform(0.5, 20.0, (H, W))
    prior[:40, :60] = -1.0  # behind the camera once lifted
    valid = rng.uniform(size=(H, W)) > 0.05
    return dict(xy1=xy1, xy2=xy2, intr1=K1, intr2=K2, cam2_from_cam1=P2, prior_map=prior, valid_map=valid, sx=W / 774.0, sy=H / 580.0)


def tri_batch(a, **kw):
    """the same candidates through mpsfm_tri_estimate_batch"""
    n = len(a["xy1"])
    P = np.zeros((2 * n, 12))
    P[0::2], P[1::2] = np.eye(3, 4).reshape(12), np.asarray(a["cam2_from_cam1"]).reshape(12)
    K = np.zeros((2 * n, 4))
    K[0::2], K[1::2] = a["intr1"], a["intr2"]
    xy = np.zeros((2 * n, 2))
    xy[0::2], xy[1::2] = a["xy1"], a["xy2"]
    return capi.tri_estimate_batch(np.arange(0, 2 * n + 1, 2), P, K, xy, **kw)


@pytest.mark.parametrize("rescale", [1.0, 0.437])
def test_hip_init_candidates_equal_the_restatement_at_size(rescale):
    a = big_init(20261017)
    n = len(a["xy1"])
    want = NR.init_pair_candidates(rescale=rescale, **a)
    got = limited(lambda: capi.init_pair_candidates(rescale=rescale, **a))
    fragile = NR.fragile_init(want)
    print("fragile matches:", int(fragile.sum()), "of", n)
    assert fragile.sum() <= FRAGILE_CAP * n
    ok = ~fragile
    # the sampler is the restatement's arithmetic bit for bit: no match is left out here
    assert np.array_equal(got["d_prior"], want["d_prior"]) and np.array_equal(got["valid"], want["valid"])
    assert 0.5 < want["valid"].mean() < 0.97 and (want["d_prior"] < 0).any()
    for k in ("tri_ok", "lift_posdepth1", "lift_posdepth2"):
        assert np.array_equal(got[k][ok], want[k][ok]), k
    assert 0.8 < want["tri_ok"].mean() < 0.95 and not want["lift_posdepth1"].all()
    scale = np.sqrt((want["lift_xyz"] ** 2).sum(1))
    assert_lift_close(got["lift_xyz"], want["lift_xyz"], scale)
    finite = np.isfinite(want["lift_angle_deg"])
    assert np.array_equal(np.isnan(got["lift_angle_deg"]), np.isnan(want["lift_angle_deg"]))
    assert np.all(np.abs(got["lift_angle_deg"] - want["lift_angle_deg"])[finite & ok] <= angle_bound_deg(want["lift_c"])[finite & ok])
    # the triangulated candidate: angle and cheirality of the restatement on the device's own point
    t = got["tri_ok"]
    m = NR.candidate_measures(a["cam2_from_cam1"], got["tri_xyz"][t])
    edge = np.zeros(n, bool)
    edge[t] = (1.0 - np.abs(m["c"]) < 1e-12) | (np.abs(m["z2"] - EPS) <= 1e-9 * np.abs(m["z2"]))
    assert edge.sum() + fragile.sum() <= FRAGILE_CAP * n
    keep = ~edge[t]
    assert np.all(np.abs(got["tri_angle_deg"][t] - m["angle"])[keep] <= angle_bound_deg(m["c"])[keep])
    assert np.array_equal(got["tri_posdepth1"][t][keep], m["posdepth1"][keep]) and np.array_equal(got["tri_posdepth2"][t][keep], m["posdepth2"][keep])
    assert got["tri_posdepth1"][t].all() and got["tri_posdepth2"][t].all()  # the estimator's own cheirality test
    assert not got["tri_xyz"][~t].any() and not got["tri_angle_deg"][~t].any()
    both = t & want["tri_ok"]
    assert np.allclose(got["tri_xyz"][both], want["tri_xyz"][both], rtol=1e-9, atol=0)
    # the reference's angle, not the geometric one: far larger on this pair
    assert np.nanmedian(got["tri_angle_deg"][t]) > 2 * np.rad2deg(1.0 / 20.0)
    assert 0 < got["ms"] < 50


def test_two_view_triangulation_equals_tri_estimate_batch_bit_for_bit():
    a = big_init(20261018, n=30000)
    got = limited(lambda: capi.init_pair_candidates(what=capi.INIT_TRIANGULATE, **a))
    xyz, ok, inl = limited(lambda: tri_batch(a, min_tri_angle=0.0, max_error=capi.INIT_TRI_MAX_ERROR))
    assert np.array_equal(got["tri_ok"], ok) and 0.8 < ok.mean() < 0.95
    assert np.array_equal(got["tri_xyz"], xyz)
    assert np.array_equal(inl.reshape(-1, 2).all(1), ok)
    # other options reach the device functions the same way
    got = limited(lambda: capi.init_pair_candidates(what=capi.INIT_TRIANGULATE, tri_min_angle=np.deg2rad(1.5), tri_max_error=np.deg2rad(0.02), **a))
    xyz, ok, _ = limited(lambda: tri_batch(a, min_tri_angle=np.deg2rad(1.5), max_error=np.deg2rad(0.02)))
    assert np.array_equal(got["tri_ok"], ok) and np.array_equal(got["tri_xyz"], xyz) and 0.05 < ok.mean() < 0.8
    assert not got["lift_xyz"].any() and not got["valid"].any()  # not asked for


# ---- run to run, thread to thread -------------------------------------------------------------------------------------------
def _same(x, y):
    if isinstance(x, dict):
        return all(np.array_equal(x[k], y[k], equal_nan=True) for k in x if k != "ms")
    return all(np.array_equal(u, v) for u, v in zip(x, y))


def test_results_are_identical_run_to_run_and_from_two_threads():
    a, b = big_pairs(5, n=20000), big_init(6, n=20000)
    calls = (lambda: capi.registration_pairs(**a), lambda: capi.init_pair_candidates(rescale=0.8, **b))
    serial = [limited(c) for c in calls]
    assert all(_same(limited(c), s) for c, s in zip(calls, serial))
    out = [[None] * 4, [None] * 4]

    def worker(k):
        for i in range(4):
            out[k][i] = calls[(k + i) % 2]()

    def both():
        ts = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()

    limited(both, 240)
    for k in range(2):
        for i in range(4):
            assert _same(out[k][i], serial[(k + i) % 2]), (k, i)


# ---- the drop-in end to end ---------------------------------------------------------------------------------------------------
def _run_mapper(backend):
    """init pair, then every other image by register_and_triangulate_next_image, on a synthetic scene"""
    from mpsfm_amd.sfm.mapper.triangulator import MpsfmTriangulator
    from numpy_scene import correspondences_from_problem, scene_from_problem

    prob, truth = make_scene(6, 3000, True, seed=97, perturb=False, outlier_frac=0.10)
    sc = scene_from_problem(prob, truth, map_size=(129, 97), seed=97, with_points=False)
    cg = correspondences_from_problem(sc, prob, false_matches=150, seed=97)
    order = []
    for imid, im in sc.images.items():
        im.has_pose, im.imid, im.ignore_matches_AP = False, imid, {}

    def register(imid):
        sc.images[imid].has_pose = True
        order.append(imid)

    sc.register_image = sc.rec.register_image = register
    sc.camera = lambda imid: sc.rec.cameras[sc.images[imid].camera_id]
    sc.best_next_ref_imid = None
    tri = MpsfmTriangulator({"colmap_options": {"min_angle": 0.001, "ignore_two_view_tracks": False}, "lift_low_parallax": False}, sc, cg)
    # the estimators' samplers are counter-based: both runs see the same RANSAC
    reg = MpsfmRegistration({"colmap_options": COLMAP_OPTIONS, "verbose": -1}, sc, NR.Matches(cg), tri, backend=backend)
    ids = sorted(sc.images)
    log = [("init", reg.register_and_triangulate_init_pair(ids[0], ids[1]), len(sc.points3D))]
    # the init pair fixes the scale (unit baseline); the mapper's post-init refinement brings the depth maps to it
    C = [-R_from_quat(truth["cam_quat"][k])[0].T @ truth["cam_t"][k] for k in (0, 1)]
    s = 1.0 / np.linalg.norm(C[1] - C[0])
    for im in sc.images.values():
        im.depth.data = im.depth.data_prior * s
    for imid in ids[2:]:
        log.append((imid, reg.register_and_triangulate_next_image(imid), len(sc.points3D)))
        masks = sc.last_ap_inlier_masks
        log.append(tuple((r, m.tobytes()) for r, m in masks.items()) if masks else None)
    tracks = {pid: tuple((e.image_id, e.point2D_idx) for e in p.track.elements) for pid, p in sc.points3D.items()}
    xyz = np.array([sc.points3D[p].xyz for p in sorted(sc.points3D)])
    poses = np.array([sc.images[i].cam_from_world.matrix() for i in ids])
    return log, order, tracks, xyz, poses


def test_drop_in_end_to_end_equals_the_restatement_behind_the_same_shim():
    hip = limited(lambda: _run_mapper(HipBackend()), 600)
    ref = limited(lambda: _run_mapper(NR.NumpyBackend()), 600)
    assert hip[0] == ref[0] and hip[1] == ref[1] and hip[2] == ref[2]
    print("end to end:", [e[:3] for e in hip[0] if e and isinstance(e[1], bool)], "registered", hip[1], "points", len(hip[2]))
    assert hip[0][0][1] is True and len(hip[1]) >= 4  # the init pair and at least two more images
    assert len(hip[2]) > 1000
    assert np.allclose(hip[3], ref[3], rtol=1e-9, atol=1e-9) and np.allclose(hip[4], ref[4], rtol=1e-9, atol=1e-9)
