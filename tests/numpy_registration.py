"""Vectorised NumPy restatement of the per-match arithmetic of registration (csrc/registration.hip; reference
mpsfm/sfm/mapper/registration.py :38-66, :341-391, :419-441 and mpsfm/utils/geometry.py :54-75), pinned by
tests/golden/reference_registration.npz.  `NumpyBackend` has the two calls of mpsfm_amd.capi that MpsfmRegistration makes,
so the drop-in's host logic runs without a device.

Every product and sum is written out element by element (no matmul / BLAS, whose fused multiply-adds differ between
machines): the sampled depths and the lifts are then the kernels' bit for bit where the kernels round every operation.
Beside each result the functions return what the tests' error bounds and fragility rules need."""

from __future__ import annotations

import numpy as np

from mpsfm_amd.sfm.scene.priorutils import bilinear_at_kps

EPS = 2.0**-52
DROPPED, TRIANGULATED, LIFTED = 0, 1, 2
NEAR = 1e-9  # a decision within this relative distance of its boundary is fragile


def quat_to_R(q):
    """common.h quat_to_R: Eigen (x, y, z, w), not normalised"""
    x, y, z, w = (float(v) for v in q)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def _len3(v):
    return np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])


def registration_pairs(refs, match_ref, ref_xy, match_pt, pts, pt_risky=None, lifted_registration=True):
    """Returns dict(xyz [n,3], kind [n], d [n] sampled depth of the lifted rows, scale [n] = |ray d| + |t| of the lifted
    rows: the size the lift's rounding errors are relative to)."""
    match_ref = np.asarray(match_ref, np.int64).reshape(-1)
    match_pt = np.asarray(match_pt, np.int64).reshape(-1)
    ref_xy = np.asarray(ref_xy, np.float64).reshape(-1, 2)
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    n = len(match_ref)
    xyz, kind, dd, scale = np.zeros((n, 3)), np.zeros(n, np.uint8), np.zeros(n), np.zeros(n)
    has = match_pt >= 0
    use3d = has.copy()
    if pt_risky is not None and len(pts):
        use3d[has] &= ~np.asarray(pt_risky, bool)[match_pt[has]]
    xyz[use3d] = pts[match_pt[use3d]]
    kind[use3d] = TRIANGULATED
    if lifted_registration:
        for r, ref in enumerate(refs):
            sel = np.flatnonzero(~use3d & (match_ref == r))
            if len(sel) == 0:
                continue
            xy = ref_xy[sel]
            d = bilinear_at_kps(ref["depth_map"], xy, ref["sx"], ref["sy"])
            fx, fy, cx, cy = (float(v) for v in ref["intr"])
            R, t = quat_to_R(ref["quat_xyzw"]), np.asarray(ref["t"], np.float64)
            p = np.stack([(xy[:, 0] - cx) / fx * d, (xy[:, 1] - cy) / fy * d, d], 1)
            q = p - t
            for k in range(3):
                xyz[sel, k] = R[0, k] * q[:, 0] + R[1, k] * q[:, 1] + R[2, k] * q[:, 2]
            kind[sel] = LIFTED
            dd[sel] = d
            scale[sel] = _len3(p) + _len3(t)
    return dict(xyz=xyz, kind=kind, d=dd, scale=scale)


def reference_angle_deg(C1, C2, X):
    """calculate_triangulation_angle (geometry.py:54-65) in degrees, on PLAIN lengths as the reference computes it.
    Returns (angle [n], c [n] the argument of acos)."""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    b = _len3(np.asarray(C1, np.float64) - np.asarray(C2, np.float64))
    r1, r2 = _len3(X - C1), _len3(X - C2)
    den = 2.0 * np.sqrt(r1 * r2)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = (r1 + r2 - b) / den
        a = np.abs(np.arccos(c))
    f = np.pi - a
    a = np.where(f < a, f, a)  # Python's min(a, pi - a): NaN stays NaN
    a = np.where(den == 0.0, 0.0, a)
    return a * (180.0 / np.pi), np.where(den == 0.0, 0.0, c)


def positive_depth(P, X):
    """has_point_positive_depth (geometry.py:68-75).  Returns (flag [n], depth [n])."""
    P = np.asarray(P, np.float64).reshape(3, 4)
    X = np.asarray(X, np.float64).reshape(-1, 3)
    z = P[2, 0] * X[:, 0] + P[2, 1] * X[:, 1] + P[2, 2] * X[:, 2] + P[2, 3]
    return z >= EPS, z


def projection_centre(P):
    P = np.asarray(P, np.float64).reshape(3, 4)
    R, t = P[:, :3], P[:, 3]
    return np.array([-(R[0, k] * t[0] + R[1, k] * t[1] + R[2, k] * t[2]) for k in range(3)])


def two_view_triangulation(xy1, xy2, intr1, intr2, P2, min_tri_angle=0.0, max_error=np.deg2rad(2.0)):
    """EstimateTriangulation of two views (COLMAP 3.11 as recalled, as oracle.track_graph_oracle.loransac_estimate runs it):
    DLT by the null vector of the 4 x 4 system, cheirality in both views, the true triangulation angle >= min_tri_angle,
    both angular residuals <= max_error.  Returns (ok [n], xyz [n,3] (0 where not ok), margin [n]: smallest relative distance
    of a decision to its boundary)."""
    xy1, xy2 = np.asarray(xy1, np.float64).reshape(-1, 2), np.asarray(xy2, np.float64).reshape(-1, 2)
    n = len(xy1)
    if n == 0:
        return np.zeros(0, bool), np.zeros((0, 3)), np.zeros(0)
    K1, K2 = np.asarray(intr1, np.float64), np.asarray(intr2, np.float64)
    P1 = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    P2 = np.asarray(P2, np.float64).reshape(3, 4)
    a = (xy1 - K1[2:4]) / K1[0:2]
    b = (xy2 - K2[2:4]) / K2[0:2]
    A = np.stack([a[:, 0, None] * P1[2] - P1[0], a[:, 1, None] * P1[2] - P1[1], b[:, 0, None] * P2[2] - P2[0],
                  b[:, 1, None] * P2[2] - P2[1]], 1)
    v = np.linalg.svd(A)[2][:, 3]
    with np.errstate(invalid="ignore", divide="ignore"):
        X = v[:, :3] / v[:, 3:4]
    X = np.where(np.isfinite(X), X, 0.0)
    f1, z1 = positive_depth(P1, X)
    f2, z2 = positive_depth(P2, X)
    C1, C2 = np.zeros(3), projection_centre(P2)
    bb, r1, r2 = ((C1 - C2) ** 2).sum(), ((X - C1) ** 2).sum(1), ((X - C2) ** 2).sum(1)
    den = 2.0 * np.sqrt(r1 * r2)
    with np.errstate(invalid="ignore", divide="ignore"):
        ang = np.abs(np.arccos(np.clip((r1 + r2 - bb) / den, -1.0, 1.0)))
    ang = np.where(den == 0.0, 0.0, np.minimum(ang, np.pi - ang))

    def angular(xn, P):
        ray = np.concatenate([xn, np.ones((n, 1))], 1)
        cam = X @ P[:, :3].T + P[:, 3]
        with np.errstate(invalid="ignore", divide="ignore"):
            c = (ray * cam).sum(1) / (_len3(ray) * _len3(cam))
        return np.arccos(np.clip(c, -1.0, 1.0))

    e1, e2 = angular(a, P1), angular(b, P2)
    ok = f1 & f2 & (ang >= min_tri_angle) & (e1 <= max_error) & (e2 <= max_error) & (v[:, 3] != 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        margin = np.minimum.reduce([np.abs(z1 - EPS) / np.maximum(np.abs(z1), EPS), np.abs(z2 - EPS) / np.maximum(np.abs(z2), EPS),
                                    np.abs(e1 - max_error) / max_error, np.abs(e2 - max_error) / max_error])
        if min_tri_angle > 0:
            margin = np.minimum(margin, np.abs(ang - min_tri_angle) / min_tri_angle)
    return ok, np.where(ok[:, None], X, 0.0), margin


def candidate_measures(P2, X):
    """angle (degrees, the reference's), its acos argument and the positive-depth flags / depths of candidates X [n,3] of a
    pair with image 1 at the identity"""
    P1 = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    ang, c = reference_angle_deg(np.zeros(3), projection_centre(P2), X)
    (f1, z1), (f2, z2) = positive_depth(P1, X), positive_depth(P2, X)
    return dict(angle=ang, c=c, posdepth1=f1, posdepth2=f2, z1=z1, z2=z2)


def init_pair_candidates(xy1, xy2, intr1, intr2, cam2_from_cam1, prior_map=None, valid_map=None, sx=1.0, sy=1.0, rescale=1.0,
                         select=None, what=3, tri_min_angle=0.0, tri_max_error=np.deg2rad(2.0), device=0):
    """The restatement of mpsfm_init_pair_candidates with the keys of capi.init_pair_candidates, plus tri_c / lift_c (acos
    arguments), tri_margin and lift_z1 / lift_z2 (camera depths of the lifted candidate) for the tests' bounds."""
    xy1, xy2 = np.asarray(xy1, np.float64).reshape(-1, 2), np.asarray(xy2, np.float64).reshape(-1, 2)
    n = len(xy1)
    P2 = np.asarray(cam2_from_cam1, np.float64).reshape(3, 4)
    keep = np.ones(n, bool) if select is None else np.asarray(select).astype(bool)
    o = dict(tri_ok=np.zeros(n, bool), tri_xyz=np.zeros((n, 3)), tri_angle_deg=np.zeros(n), tri_posdepth1=np.zeros(n, bool),
             tri_posdepth2=np.zeros(n, bool), lift_xyz=np.zeros((n, 3)), lift_angle_deg=np.zeros(n), lift_posdepth1=np.zeros(n, bool),
             lift_posdepth2=np.zeros(n, bool), d_prior=np.zeros(n), valid=np.zeros(n, bool), ms=0.0, tri_c=np.zeros(n),
             lift_c=np.zeros(n), tri_margin=np.full(n, np.inf), lift_z1=np.ones(n), lift_z2=np.ones(n), valid_sample=np.zeros(n))
    idx = np.flatnonzero(keep)
    if what & 1 and len(idx):
        ok, X, margin = two_view_triangulation(xy1[idx], xy2[idx], intr1, intr2, P2, tri_min_angle, tri_max_error)
        m = candidate_measures(P2, X)
        o["tri_ok"][idx], o["tri_xyz"][idx], o["tri_margin"][idx] = ok, X, margin
        o["tri_angle_deg"][idx] = np.where(ok, m["angle"], 0.0)
        o["tri_c"][idx] = np.where(ok, m["c"], 0.0)
        o["tri_posdepth1"][idx], o["tri_posdepth2"][idx] = ok & m["posdepth1"], ok & m["posdepth2"]
    if what & 2 and len(idx):
        fx, fy, cx, cy = (float(v) for v in np.asarray(intr1, np.float64).reshape(4))
        xy = xy1[idx]
        d = bilinear_at_kps(prior_map, xy, sx, sy)
        vs = bilinear_at_kps(np.asarray(valid_map, np.float64), xy, sx, sy)
        ds = d * float(rescale)
        X = np.stack([(xy[:, 0] - cx) / fx * ds, (xy[:, 1] - cy) / fy * ds, ds], 1)
        m = candidate_measures(P2, X)
        o["d_prior"][idx], o["valid"][idx], o["valid_sample"][idx], o["lift_xyz"][idx] = d, vs == 1, vs, X
        o["lift_angle_deg"][idx], o["lift_c"][idx] = m["angle"], m["c"]
        o["lift_posdepth1"][idx], o["lift_posdepth2"][idx] = m["posdepth1"], m["posdepth2"]
        o["lift_z1"][idx], o["lift_z2"][idx] = m["z1"], m["z2"]
    return o


def fragile_init(o, thresholds=(1.5, 16.0)):
    """matches of an init_pair_candidates result with a decision within NEAR (relative) of its boundary, or whose acos
    argument is within 1e-12 of +-1.  The validity decision (sampled mask == 1) is not among them: the sampler is the same
    arithmetic bit for bit on every side, so a sample one ulp below 1 is invalid everywhere (see near_valid)."""
    f = np.zeros(len(o["valid"]), bool)
    f |= o["tri_margin"] < NEAR
    for z in (o["lift_z1"], o["lift_z2"]):
        f |= np.abs(z - EPS) <= NEAR * np.maximum(np.abs(z), EPS)
    for c in (o["tri_c"], o["lift_c"]):
        f |= 1.0 - np.abs(c) < 1e-12
    for a in (o["tri_angle_deg"], o["lift_angle_deg"]):
        for th in thresholds:
            f |= np.abs(a - th) <= NEAR * th
    return f


def near_valid(o):
    """matches whose sampled mask is within NEAR of 1 without being 1 (the fixture generator draws such cases again)"""
    return (np.abs(o["valid_sample"] - 1.0) <= NEAR) & (o["valid_sample"] != 1.0)


class NumpyBackend:
    """the two calls MpsfmRegistration makes on mpsfm_amd.capi, answered by the restatement"""

    @staticmethod
    def registration_pairs(refs, match_ref, ref_xy, match_pt, pts, pt_risky=None, lifted_registration=True, device=0):
        r = registration_pairs(refs, match_ref, ref_xy, match_pt, pts, pt_risky, lifted_registration)
        return r["xyz"], r["kind"]

    @staticmethod
    def init_pair_candidates(*a, **k):
        return init_pair_candidates(*a, **k)


# ---- stand-in scene for MpsfmRegistration (the accessors the reference's class uses on mpsfm_rec / correspondences) ----------
class Matches:
    """`correspondences.matches(imid1, imid2)` [m, 2] (keypoint of imid1, keypoint of imid2) over a correspondence graph"""

    def __init__(self, graph):
        self.graph = graph

    def matches(self, imid1, imid2):
        return np.asarray(self.graph.find_correspondences_between_images(imid1, imid2), np.int64).reshape(-1, 2)


def registration_scene(spec, depth_factory=None, pose_factory=None, risky_ids=None):
    """A NumpyReconstruction with what registration needs on top (register_image, camera, best_next_ref_imid,
    last_ap_inlier_masks, images[*].imid / ignore_matches_AP) from a dict of arrays `spec`:
      image_ids [I], and per image id k: im{k}_kps, im{k}_intr, im{k}_size (w, h), im{k}_data, im{k}_data_prior (absent: data), im{k}_valid,
      im{k}_quat, im{k}_t, im{k}_registered, im{k}_kp_point3D (-1: none); point_ids [P], point_xyz [P,3];
      pairs [M,2] with pair{j}_matches [m,2]; ignore [G,2] = (image, reference) with ignore{j}_mask.
    `risky_ids`: the answer of find_points3D_with_small_triangulation_angle (None: the scene's own, which needs a device).
    `depth_factory(data, data_prior, valid, camera)` / `pose_factory(quat, t)`: other depth / pose classes (the fixture
    generator passes the reference's)."""
    from numpy_scene import INVALID_POINT3D, NumpyCamera, NumpyCorrespondenceGraph, NumpyDepth, NumpyImage, NumpyReconstruction, Rigid3d, Track

    class Scene(NumpyReconstruction):
        best_next_ref_imid = None
        last_ap_inlier_masks = None

        def camera(self, imid):
            return self.rec.cameras[self.images[imid].camera_id]

        def register_image(self, imid):
            self.images[imid].has_pose = True
            self.registration_order.append(int(imid))

        def find_points3D_with_small_triangulation_angle(self, min_angle, point3D_ids):
            if self.risky_ids is None:
                return super().find_points3D_with_small_triangulation_angle(min_angle, point3D_ids)
            self.risky_calls += 1
            return np.array([int(p) in self.risky_ids for p in point3D_ids], bool)

    def default_depth(data, data_prior, valid, camera):
        d = NumpyDepth.__new__(NumpyDepth)
        d.data, d.data_prior, d.valid, d.camera = data, data_prior, valid, camera
        return d

    depth_factory, pose_factory = depth_factory or default_depth, pose_factory or Rigid3d
    scene = Scene()
    scene.registration_order, scene.risky_calls = [], 0
    scene.risky_ids = None if risky_ids is None else {int(p) for p in risky_ids}
    scene.rec.register_image = scene.register_image
    graph = NumpyCorrespondenceGraph()
    for k in (int(v) for v in spec["image_ids"]):
        kps = np.asarray(spec[f"im{k}_kps"], np.float64)
        w, h = (float(v) for v in spec[f"im{k}_size"])
        data = np.asarray(spec[f"im{k}_data"], np.float64)
        cam = NumpyCamera(k, spec[f"im{k}_intr"], w, h, data.shape[1], data.shape[0])
        scene.rec.cameras[k] = cam
        depth = depth_factory(data.copy(), np.asarray(spec[f"im{k}_data_prior"] if f"im{k}_data_prior" in spec else data, np.float64).copy(),
                              np.asarray(spec[f"im{k}_valid"]).astype(bool), cam)
        img = NumpyImage(k, k, pose_factory(spec[f"im{k}_quat"], spec[f"im{k}_t"]), kps, 1.0, depth)
        img.imid, img.ignore_matches_AP, img.has_pose = k, {}, bool(spec[f"im{k}_registered"])
        scene.images[k] = img
        graph.add_image(k, len(kps))
    # points keep their ids: tracks are rebuilt from the keypoints that carry them
    ids = [int(p) for p in spec["point_ids"]]
    els = {p: Track() for p in ids}
    for k in (int(v) for v in spec["image_ids"]):
        for i, p in enumerate(np.asarray(spec[f"im{k}_kp_point3D"], np.int64)):
            if p >= 0:
                els[int(p)].add_element(k, i)
    for p, xyz in zip(ids, np.asarray(spec["point_xyz"], np.float64).reshape(-1, 3)):
        scene._next_point3D_id = p
        assert scene.obs.add_point3D(xyz, els[p]) == p
    scene._next_point3D_id = max(ids, default=0) + 1
    for j, (a, b) in enumerate(np.asarray(spec["pairs"], np.int64).reshape(-1, 2)):
        graph.add_correspondences(int(a), int(b), spec[f"pair{j}_matches"])
    for j, (im, ref) in enumerate(np.asarray(spec["ignore"], np.int64).reshape(-1, 2)):
        scene.images[int(im)].ignore_matches_AP[int(ref)] = np.asarray(spec[f"ignore{j}_mask"]).astype(bool).copy()
    assert INVALID_POINT3D
    return scene, Matches(graph)


class ReplayEstimator:
    """An estimator stub that answers its calls from a recorded list (None entries included) and keeps what it was asked"""

    def __init__(self, answers):
        self.answers, self.calls = list(answers), []

    def __call__(self, *args):
        self.calls.append(args)
        return self.answers[len(self.calls) - 1]
