"""Fixture for image registration (tests/golden/reference_registration.npz), computed BY THE REFERENCE'S OWN CODE:

  by file path      mpsfm/utils/geometry.py                         calculate_triangulation_angle, has_point_positive_depth
                    mpsfm/sfm/scene/image/mixins/priorutils.py      PriorUtils (the depth objects of the scene)
  by AST extraction mpsfm/sfm/mapper/registration.py                MpsfmRegistration._candidate_points3D_for_init,
                    _find_2D3D_pairs, _collect_pairs, _lift_points_to_3d, _lift_points_for_init, _process_2D3D_pairs,
                    _candidate_lift_for_init, _init_pair_points_and_pose, register_next_image,
                    register_and_triangulate_init_pair
  (the module imports pycolmap and mpsfm.baseclass, absent here, hence the extraction)

They run on the stand-in scene of tests/numpy_registration.py (depth objects swapped for the reference's PriorUtils) with
  * a stand-in `pycolmap` namespace written here: Rigid3d, Track, and estimate_triangulation ANSWERED BY THIS REPOSITORY'S
    OWN CPU RESTATEMENT of COLMAP's estimator (oracle.track_graph_oracle.loransac_estimate): that one function stays
    "restated, parity unpinned";
  * recorded AbsolutePose / RelativePose answers (poses and inlier masks drawn here and stored in the fixture): the
    estimators are stubs that return them, so nothing depends on RANSAC.

Cases.  `next`: a registration against 5 reference images (two map sizes; one has no matches) with risky points,
ignore_matches_AP entries, 3-D ids shared between references, keypoints outside the maps; run with lifted_registration on
and off, with the resample branch taken once, with too few inliers, and with forced registration.  `init_*`: init pairs in
the high- and the low-parallax branch, with AP_info None, with invalid-mask keypoints, keypoints matched twice and matches
whose keypoints already carry points.  Keypoints lie on a quarter-pixel grid, maps hold float32 values.  An init case in
which a decision lies within 1e-9 (relative) of its boundary (an angle against 1.5 / 16, a depth against eps, a residual of
the triangulation against 2 degrees, a sampled mask against 1, the neighbours of the median's middle pair) is drawn again.
The file holds inputs and outputs only.

Run in the build container:  python tests/golden/make_golden_registration.py
"""
import os
import sys
import types
from collections import defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_reference import REF, ROOT, extract_functions, load_by_path  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy_registration as NR  # noqa: E402
from mpsfm_amd.synthetic import R_from_quat  # noqa: E402
from oracle import track_graph_oracle as TGO  # noqa: E402

METHODS = ("_candidate_points3D_for_init", "_find_2D3D_pairs", "_collect_pairs", "_lift_points_to_3d", "_lift_points_for_init",
           "_process_2D3D_pairs", "_candidate_lift_for_init", "_init_pair_points_and_pose", "register_next_image",
           "register_and_triangulate_init_pair")
IMAGE_SIZE = (512.0, 384.0)
MAP_SIZES = {1: (48, 64), 2: (24, 32), 3: (48, 64), 4: (24, 32), 5: (48, 64), 6: (3, 4)}  # (H, W) per image id of `next`
KEYS = ("pt2d_id_1", "pt2d_id_2", "tri_angle", "posdepth1", "posdepth2", "xyz")


# ---- the stand-in pycolmap namespace -------------------------------------------------------------------------------------
class Rot:
    def __init__(self, R):
        self.R = np.asarray(R, np.float64)

    def inverse(self):
        return Rot(self.R.T)

    def matrix(self):
        return self.R.copy()

    def __mul__(self, v):
        return self.R @ np.asarray(v, np.float64)


class Rig:
    """pycolmap.Rigid3d as the reference uses it; Rig() is the identity"""

    def __init__(self, quat=None, t=None):
        self.quat = np.array([0.0, 0.0, 0.0, 1.0]) if quat is None else np.asarray(quat, np.float64)
        self.rotation = Rot(np.eye(3) if quat is None else R_from_quat(self.quat)[0])
        self.translation = np.zeros(3) if t is None else np.asarray(t, np.float64)

    def matrix(self):
        return np.concatenate([self.rotation.R, self.translation[:, None]], 1)

    def inverse(self):
        out = Rig()
        out.rotation = Rot(self.rotation.R.T)
        out.translation = -self.rotation.R.T @ self.translation
        return out

    def __mul__(self, pts):
        return np.asarray(pts, np.float64) @ self.rotation.R.T + self.translation


def estimate_triangulation(pointdata, cams_from_world, cameras):
    """RESTATED, parity unpinned: COLMAP's EstimateTriangulation by oracle.track_graph_oracle.loransac_estimate with the
    defaults of pycolmap 3.11 as recalled (min_tri_angle 0, angular residual, max_error 2 degrees)"""
    views = []
    for xy, pose, cam in zip(pointdata, cams_from_world, cameras):
        K = np.asarray(cam.params, np.float64)
        P = pose.matrix()
        views.append(TGO.View(xy=np.asarray(xy, np.float64), xn=(xy - K[2:4]) / K[0:2], P=P, C=-P[:, :3].T @ P[:, 3], K=K))
    rep = TGO.loransac_estimate(views, TGO.RansacOptions(max_error=float(np.deg2rad(2.0)), min_tri_angle=0.0))
    return {"xyz": np.asarray(rep.model, np.float64)} if rep.success else None


def reference_class():
    geom = load_by_path("ref_geometry", "mpsfm/utils/geometry.py")
    ns = extract_functions("mpsfm/sfm/mapper/registration.py", cls="MpsfmRegistration", method_names=METHODS)
    from numpy_scene import Track

    ns.update(defaultdict=defaultdict, calculate_triangulation_angle=geom.calculate_triangulation_angle,
              has_point_positive_depth=geom.has_point_positive_depth,
              pycolmap=types.SimpleNamespace(Rigid3d=Rig, Track=Track, estimate_triangulation=estimate_triangulation))

    class Conf(dict):
        __getattr__ = dict.__getitem__

    class Reg(ns["MpsfmRegistration"]):
        """the extracted methods plus a recorder of the intermediate candidate lists"""

        def __init__(self, scene, correspondences, rel, ab, **conf):
            c = dict(lifted_registration=True, reduce_min_inliers_at_failure=6, parallax_thresh=1.5, combined_triangle_thresh=1.5,
                     robust_triangles=1, resample_bunlde=False, verbose=0,
                     colmap_options=Conf(init_min_tri_angle=16.0, abs_pose_min_num_inliers=30))
            c.update(conf)
            self.conf = Conf(c)
            self.mpsfm_rec, self.correspondences = scene, correspondences
            self.relative_pose_estimator, self.absolute_pose_estimator = rel, ab
            self.half_ap_min_inliers, self.registration_cache = 0, defaultdict(dict)
            self.recorded = []

        def _candidate_points3D_for_init(self, *a, **k):
            out = ns["MpsfmRegistration"]._candidate_points3D_for_init(*a, **k)
            self.recorded.append(("tri", out, a[1].matrix()))
            return out

        def _candidate_lift_for_init(self, *a, **k):
            out = ns["MpsfmRegistration"]._candidate_lift_for_init(self, *a, **k)
            self.recorded.append(("lift", out, a[1].matrix()))
            return out

        def _process_2D3D_pairs(self, pair2D3D):
            out = ns["MpsfmRegistration"]._process_2D3D_pairs(self, pair2D3D)
            self.recorded.append(("pairs", out))
            return out

    return Reg


def reference_scene(spec, risky_ids):
    P = load_by_path("ref_priorutils", "mpsfm/sfm/scene/image/mixins/priorutils.py").PriorUtils

    def depth(data, data_prior, valid, camera):
        o = P.init_empty()
        o.data, o.data_prior, o.valid, o.camera = data, data_prior, valid, camera
        return o

    return NR.registration_scene(spec, depth_factory=depth, pose_factory=Rig, risky_ids=risky_ids)


# ---- drawing ------------------------------------------------------------------------------------------------------------------
def quarter(v):
    return np.round(np.asarray(v) * 4.0) / 4.0


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def unit_quat(rng, scale=0.3):
    q = np.concatenate([rng.normal(0, scale, 3), [1.0]])
    return q / np.linalg.norm(q)


def image_entry(spec, k, kps, intr, data, prior, valid, quat, t, registered, kp_point3D):
    spec[f"im{k}_kps"], spec[f"im{k}_intr"], spec[f"im{k}_size"] = kps, np.asarray(intr, np.float64), np.array(IMAGE_SIZE)
    spec[f"im{k}_data"], spec[f"im{k}_valid"] = data, valid
    if prior is not None:  # absent: the scene takes `data` (registration against references never reads the prior)
        spec[f"im{k}_data_prior"] = prior
    spec[f"im{k}_quat"], spec[f"im{k}_t"], spec[f"im{k}_registered"] = quat, np.asarray(t, np.float64), np.array(registered)
    spec[f"im{k}_kp_point3D"] = np.asarray(kp_point3D, np.int64)


def draw_next(rng):
    """references 1..5 (5 without matches), query 6; the geometry is arbitrary: the estimator answers are recorded"""
    spec = {"image_ids": np.arange(1, 7)}
    n_kp, n_pts = 300, 160
    point_ids = np.arange(1, n_pts + 1) * 3  # ids are not indices
    spec["point_ids"], spec["point_xyz"] = point_ids, rng.normal(0, 3, (n_pts, 3))
    for k in range(1, 7):
        H, W = MAP_SIZES[k]
        kps = quarter(np.stack([rng.uniform(-20, IMAGE_SIZE[0] + 20, n_kp), rng.uniform(-20, IMAGE_SIZE[1] + 20, n_kp)], 1))
        kps[:6] = [[0, 0], [IMAGE_SIZE[0] - 8, 0], [0, IMAGE_SIZE[1] - 8], [-7.75, 100], [IMAGE_SIZE[0] - 4, 50], [200, IMAGE_SIZE[1] + 9]]
        f = rng.uniform(400, 520)
        intr = [f, f * rng.uniform(0.97, 1.03), IMAGE_SIZE[0] / 2 + rng.normal(0, 4), IMAGE_SIZE[1] / 2 + rng.normal(0, 4)]
        data = f32(rng.uniform(0.5, 9.0, (H, W)))
        if k <= 5:
            data[2:4, 5:9] = 0.0
            data[10, 3:6] = -1.25
        if k == 6:  # the query: its first 60 keypoints left of x = 100 (reference 1 matches only those), the others right of it
            kps[:, 0] = quarter(np.where(np.arange(n_kp) < 60, rng.uniform(-20, 99, n_kp), rng.uniform(101, IMAGE_SIZE[0] + 20, n_kp)))
        kp3 = np.full(n_kp, -1, np.int64)
        if k <= 5:  # every reference sees a random half of the points: ids shared between references
            seen = rng.permutation(n_pts)[: n_pts // 2]
            kp3[rng.permutation(n_kp)[: len(seen)]] = point_ids[seen]
        image_entry(spec, k, kps, intr, data, None, rng.uniform(size=(H, W)) > 0.1, unit_quat(rng),
                    rng.normal(0, 2, 3), k <= 5, kp3)
    pairs = []
    for j, ref in enumerate((1, 2, 3, 4)):
        m = 140
        a = rng.integers(0, n_kp, m)
        a[:6] = np.arange(6)  # the keypoints on and beyond the map border
        b = rng.integers(0, 60, m) if ref == 1 else rng.integers(60, n_kp, m)
        pairs.append((ref, 6))
        spec[f"pair{j}_matches"] = np.stack([a, b], 1)
    spec["pairs"] = np.array(pairs)
    spec["ignore"] = np.array([(6, 2), (6, 4)])
    spec["ignore0_mask"] = rng.uniform(size=140) < 0.2
    spec["ignore1_mask"] = rng.uniform(size=140) < 0.5
    risky = point_ids[rng.uniform(size=n_pts) < 0.25]
    return spec, risky


def draw_init(rng, kind):
    """image 1 at the identity, image 2 a baseline to the side; points in front of both; the prior of image 1 is the true
    depth times ~0.5 (so the median rescale matters) with noise"""
    n_kp, n_match = 420, 330
    spec = {"image_ids": np.array([1, 2])}
    H, W = 48, 64
    f = 460.0
    intr1 = [f, f * 1.01, IMAGE_SIZE[0] / 2 + 3.0, IMAGE_SIZE[1] / 2 - 2.0]
    intr2 = [f * 0.98, f, IMAGE_SIZE[0] / 2 - 4.0, IMAGE_SIZE[1] / 2 + 1.0]
    # the reference's angle grows like sqrt(baseline / depth): the low-parallax pair needs a tiny baseline to straddle 1.5 degrees
    base = {"high": 1.2, "low": 0.002, "none": 0.6}[kind]
    q2 = unit_quat(rng, 0.03)
    R2 = R_from_quat(q2)[0]
    C2 = np.array([base, 0.05 * base, -0.02 * base])
    t2 = -R2 @ C2
    kps1 = quarter(np.stack([rng.uniform(-6, IMAGE_SIZE[0] + 6, n_kp), rng.uniform(-6, IMAGE_SIZE[1] + 6, n_kp)], 1))
    z = rng.uniform(2.0, 9.0, n_kp)
    X = np.stack([(kps1[:, 0] - intr1[2]) / intr1[0] * z, (kps1[:, 1] - intr1[3]) / intr1[1] * z, z], 1)
    Xc = X @ R2.T + t2
    proj = np.stack([intr2[0] * Xc[:, 0] / Xc[:, 2] + intr2[2], intr2[1] * Xc[:, 1] / Xc[:, 2] + intr2[3]], 1)
    noise, grid = (0.002, 256.0) if kind == "low" else (0.4, 4.0)  # sub-pixel disparities need fine keypoints in image 2
    kps2 = np.round(np.concatenate([proj + rng.normal(0, noise, proj.shape), rng.uniform(0, 380, (40, 2))]) * grid) / grid
    m1 = rng.permutation(n_kp)[:n_match]
    m2 = m1.copy()
    wrong = rng.uniform(size=n_match) < 0.12  # false matches
    m2[wrong] = rng.integers(0, len(kps2), wrong.sum())
    m1[-8:] = m1[:8]  # keypoints of image 1 matched twice
    matches = np.stack([m1, m2], 1)
    # prior: nearest keypoint's depth, scaled
    gy, gx = np.mgrid[0:H, 0:W]
    sx, sy = W / IMAGE_SIZE[0], H / IMAGE_SIZE[1]
    d2 = (gx.ravel()[:, None] - kps1[:, 0] * sx) ** 2 + (gy.ravel()[:, None] - kps1[:, 1] * sy) ** 2
    prior = f32((z[np.argmin(d2, 1)] * 0.5 * np.exp(rng.normal(0, 0.03, H * W))).reshape(H, W))
    valid = rng.uniform(size=(H, W)) > 0.08
    valid[30:36, 40:52] = False
    kp3_1, kp3_2 = np.full(n_kp, -1, np.int64), np.full(len(kps2), -1, np.int64)
    point_ids = np.array([7, 11])  # two points already in the scene, on matched keypoints
    kp3_1[m1[20]], kp3_2[m2[33]] = 7, 11
    spec["point_ids"], spec["point_xyz"] = point_ids, rng.normal(0, 1, (2, 3)) + [0, 0, 5]
    image_entry(spec, 1, kps1, intr1, prior.copy(), prior, valid, unit_quat(rng), rng.normal(0, 1, 3), False, kp3_1)
    image_entry(spec, 2, kps2, intr2, f32(rng.uniform(1, 8, (3, 4))), None, np.ones((3, 4), bool), unit_quat(rng),  # maps of image 2: never read
                rng.normal(0, 1, 3), False, kp3_2)
    spec["pairs"], spec["pair0_matches"] = np.array([(1, 2)]), matches
    spec["ignore"] = np.zeros((0, 2), np.int64)
    # recorded answers: the relative pose (true, unit baseline) with a mask, the absolute pose (true scale of the prior) with one
    scale = np.linalg.norm(t2)
    answers = dict(E_quat=q2, E_t=t2 / scale, E_mask=(~wrong) & (rng.uniform(size=n_match) < (0.45 if kind == "low" else 0.93)),
                   AP_quat=q2, AP_t=t2 * 0.5, AP_seed=int(rng.integers(1 << 30)),
                   AP_none=np.array(kind == "none"), AP_inlier_fraction=np.array({"high": 0.05, "low": 0.9, "none": 0.0}[kind]))
    return spec, answers


# ---- running the reference ------------------------------------------------------------------------------------------------------
def ap_answer(p2, quat, t, fraction, seed):
    """fraction < 0: no inlier among the rows whose query keypoint lies left of x = 100 (the rows of reference 1 in `next`)"""
    mask = np.random.default_rng(seed).uniform(size=len(p2)) < abs(fraction)
    if fraction < 0:
        mask &= np.asarray(p2)[:, 0] >= 100.0
    return {"cam_from_world": (quat, t), "num_inliers": int(mask.sum()), "inlier_mask": mask}


class RecordingAP:
    """AbsolutePose stub: draws its answer (a fixed pose and a random mask of the right length) and records call and answer"""

    def __init__(self, answers, pose_cls):
        self.answers, self.pose_cls, self.calls = list(answers), pose_cls, []

    def __call__(self, p2, p3, camera):
        a = self.answers[len(self.calls)]
        out = None
        if a is not None:
            r = ap_answer(p2, *a)
            out = dict(r, cam_from_world=self.pose_cls(*r["cam_from_world"]))
        self.calls.append((np.array(p2, np.float64).reshape(-1, 2), np.array(p3, np.float64).reshape(-1, 3),
                           None if out is None else out["inlier_mask"], None if a is None else np.concatenate([a[0], a[1]])))
        return out


def store_ap_calls(out, tag, ap, points=True):
    out[f"{tag}_ap_calls"] = np.array(len(ap.calls))
    for i, (p2, p3, mask, pose) in enumerate(ap.calls):
        if points:
            out[f"{tag}_ap{i}_points2D"], out[f"{tag}_ap{i}_points3D"] = p2, p3
        out[f"{tag}_ap{i}_pose"] = np.zeros(7) if pose is None else pose  # quat xyzw, t
        out[f"{tag}_ap{i}_mask"] = np.zeros(0, bool) if mask is None else mask
        out[f"{tag}_ap{i}_none"] = np.array(mask is None)


def run_next(Reg, spec, risky, out, tag, answers, min_inliers=30, half=0, best=1, points=True, **conf):
    """points=False: the estimator's inputs are those of `next_lifted` and are not stored again"""
    scene, corr = reference_scene(spec, risky)
    scene.best_next_ref_imid = best
    ap = RecordingAP(answers, Rig)
    reg = Reg(scene, corr, None, ap, **conf)
    reg.conf.colmap_options["abs_pose_min_num_inliers"] = min_inliers
    reg.half_ap_min_inliers = half
    ok = reg.register_next_image(6)
    out[f"{tag}_return"] = np.array(bool(ok))
    out[f"{tag}_conf"] = np.array([min_inliers, half, best, int(conf.get("lifted_registration", True)), int(conf.get("resample_bunlde", False))])
    store_ap_calls(out, tag, ap, points)
    pairs = [r[1] for r in reg.recorded if r[0] == "pairs"]
    out[f"{tag}_passes"] = np.array(len(pairs))
    for i, (p2, p3, order, lifted, ids3d) in enumerate(pairs if points else []):
        out[f"{tag}_pass{i}_points2D"], out[f"{tag}_pass{i}_points3D"] = p2, p3
        out[f"{tag}_pass{i}_order"], out[f"{tag}_pass{i}_lifted"], out[f"{tag}_pass{i}_ids3d"] = np.array(order), lifted, np.asarray(ids3d, np.int64)
    masks = scene.last_ap_inlier_masks
    out[f"{tag}_has_masks"] = np.array(masks is not None)
    if masks is not None:
        out[f"{tag}_mask_refs"] = np.array(list(masks), np.int64)
        out[f"{tag}_mask_sizes"] = np.array([len(m) for m in masks.values()], np.int64)
        out[f"{tag}_mask_values"] = np.concatenate([np.asarray(m, bool) for m in masks.values()])
    ign = scene.images[6].ignore_matches_AP
    out[f"{tag}_ignore_refs"] = np.array(sorted(ign), np.int64)
    for r in sorted(ign):
        out[f"{tag}_ignore_ref{r}"] = np.asarray(ign[r], bool)
    out[f"{tag}_registered"] = np.array(scene.registration_order, np.int64)
    if ok:
        out[f"{tag}_pose"] = scene.images[6].cam_from_world.matrix()
    print(f"{tag}: return {ok}, {len(ap.calls)} AP call(s), rows {[len(p[0]) for p in pairs]}, lifted {[int(p[3].sum()) for p in pairs]}, "
          f"triangulated ids {[len(p[4]) for p in pairs]} (unique {[len(np.unique(p[4])) for p in pairs]}), risky calls {scene.risky_calls}")


def init_margins(spec, answers, reg, cand):
    """number of decisions of an init case within 1e-9 of their boundary"""
    bad = 0
    kps1, kps2 = spec["im1_kps"], spec["im2_kps"]
    m = spec["pair0_matches"]
    cam_maps = dict(prior_map=spec["im1_data_prior"], valid_map=spec["im1_valid"], sx=64 / IMAGE_SIZE[0], sy=48 / IMAGE_SIZE[1])
    for kind, lists, P2 in reg.recorded:
        ang = np.asarray(lists["tri_angle"], np.float64)
        for th in (1.5, 16.0):
            bad += int((np.abs(ang - th) <= NR.NEAR * th).sum())
        if len(ang):
            mm = NR.candidate_measures(P2, np.vstack(lists["xyz"]))
            for z in (mm["z1"], mm["z2"]):
                bad += int((np.abs(z - NR.EPS) <= NR.NEAR * np.maximum(np.abs(z), NR.EPS)).sum())
            bad += int((1.0 - np.abs(mm["c"]) < 1e-12).sum())
        if kind == "tri":  # every match the estimator saw: the residual and cheirality margins of the restatement
            o = NR.init_pair_candidates(kps1[m[:, 0]], kps2[m[:, 1]], spec["im1_intr"], spec["im2_intr"], P2, what=1)
            bad += int((o["tri_margin"] < NR.NEAR).sum())
    o = NR.init_pair_candidates(kps1, kps1, spec["im1_intr"], spec["im2_intr"], np.eye(3, 4), what=2, **cam_maps)
    bad += int(NR.near_valid(o).sum())
    tri = [r for r in reg.recorded if r[0] == "tri"]
    if tri and len(tri[0][1]["xyz"]) > 2:
        ids = np.asarray(tri[0][1]["pt2d_id_1"], np.int64)
        ratio = np.sort(np.vstack(tri[0][1]["xyz"])[:, 2] / o["d_prior"][ids])
        mid = len(ratio) // 2
        near = ratio[max(mid - 2, 0): mid + 2]
        bad += int((np.diff(near) <= NR.NEAR * np.abs(near[1:])).sum())
    return bad


def run_init(Reg, spec, answers, out, tag):
    scene, corr = reference_scene(spec, None)
    rel = NR.ReplayEstimator([{"cam2_from_cam1": Rig(answers["E_quat"], answers["E_t"]), "inlier_mask": answers["E_mask"]}])
    ap = RecordingAP([None if answers["AP_none"] else (answers["AP_quat"], answers["AP_t"], float(answers["AP_inlier_fraction"]), int(answers["AP_seed"]))], Rig)
    reg = Reg(scene, corr, rel, ap)
    kw = dict(imid1=1, imid2=2, matches=corr.matches(1, 2), kps1=scene.keypoints(1), kps2=scene.keypoints(2), camera1=scene.camera(1),
              camera2=scene.camera(2))
    cand, pose = reg._init_pair_points_and_pose(**kw)
    bad = init_margins(spec, answers, reg, cand)
    if bad:
        return bad
    for k in KEYS:
        out[f"{tag}_cand_{k}"] = np.array(cand[k]) if len(cand[k]) else np.zeros((0, 3) if k == "xyz" else 0)
    out[f"{tag}_cand_pose"] = pose.matrix()
    for i, (kind, lists, P2) in enumerate(reg.recorded):
        out[f"{tag}_rec{i}_kind"] = np.array(kind)
        for k in KEYS:
            out[f"{tag}_rec{i}_{k}"] = np.array(lists[k]) if len(lists[k]) else np.zeros((0, 3) if k == "xyz" else 0)
    out[f"{tag}_recorded"] = np.array(len(reg.recorded))
    store_ap_calls(out, tag + "_pp", ap)
    # the whole method on a fresh scene
    scene, corr = reference_scene(spec, None)
    rel.calls, ap.calls = [], []
    reg = Reg(scene, corr, rel, ap)
    n_before = len(scene.points3D)
    ok = reg.register_and_triangulate_init_pair(1, 2)
    out[f"{tag}_return"] = np.array(bool(ok))
    new = sorted(p for p in scene.points3D if p not in (7, 11))
    out[f"{tag}_added_xyz"] = np.array([scene.points3D[p].xyz for p in new]).reshape(-1, 3)
    out[f"{tag}_added_tracks"] = np.array([[e.point2D_idx for e in scene.points3D[p].track.elements] for p in new], np.int64).reshape(-1, 2)
    out[f"{tag}_registered"] = np.array(scene.registration_order, np.int64)
    out[f"{tag}_pose1"], out[f"{tag}_pose2"] = scene.images[1].cam_from_world.matrix(), scene.images[2].cam_from_world.matrix()
    for k, v in answers.items():
        out[f"{tag}_answer_{k}"] = np.asarray(v)
    print(f"{tag}: return {ok}, candidates {len(cand['xyz'])}, recorded {[(r[0], len(r[1]['xyz'])) for r in reg.recorded]}, "
          f"points {n_before} -> {len(scene.points3D)}, AP {'None' if answers['AP_none'] else ap.calls[0][2].sum()}")
    return 0


def store_spec(out, tag, spec):
    for k, v in spec.items():
        v = np.asarray(v)
        if k.endswith(("_data", "_data_prior")):
            assert np.array_equal(v, v.astype(np.float32).astype(np.float64))
            v = v.astype(np.float32)
        out[f"{tag}_spec_{k}"] = v


def generate():
    rng = np.random.default_rng(20261016)
    Reg = reference_class()
    out = {}
    spec, risky = draw_next(rng)
    store_spec(out, "next", spec)
    out["next_risky"] = risky
    q, t = unit_quat(rng), rng.normal(0, 2, 3)
    full = (q, t, 0.6, 11)
    run_next(Reg, spec, risky, out, "next_lifted", [full])
    run_next(Reg, spec, risky, out, "next_plain", [full], lifted_registration=False)
    # the resample branch: the first answer leaves the best reference (1) almost without inliers, the second ends the loop
    run_next(Reg, spec, risky, out, "next_resample", [(q, t, 0.0, 5), full], points=False, resample_bunlde=True, min_inliers=0, best=1)
    run_next(Reg, spec, risky, out, "next_resample_taken", [(q, t, -0.5, 5), (q, t, 0.5, 6)], resample_bunlde=True, min_inliers=0, best=1)
    run_next(Reg, spec, risky, out, "next_few", [(q, t, 0.02, 3)], points=False, min_inliers=30, half=2)
    run_next(Reg, spec, risky, out, "next_forced", [(q, t, 0.02, 3)], points=False, min_inliers=30, half=6)
    run_next(Reg, spec, risky, out, "next_none", [None], points=False)
    for kind in ("high", "low", "none"):
        for attempt in range(60):
            spec, answers = draw_init(rng, kind)
            case = {}
            bad = run_init(Reg, spec, answers, case, f"init_{kind}")
            if bad == 0:
                break
            print(f"init_{kind}: redraw, {bad} decision(s) near a boundary")
        else:
            raise RuntimeError("no clean init case in 60 draws")
        store_spec(out, f"init_{kind}", spec)
        out.update(case)
    return out


if __name__ == "__main__":
    assert os.path.isdir(REF), REF
    out = generate()
    path = os.path.join(HERE, "reference_registration.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")
