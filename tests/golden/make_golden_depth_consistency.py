"""Fixture for the depth-consistency check (tests/golden/reference_depth_consistency.npz), computed BY THE REFERENCE'S
OWN CODE:

  by file path      mpsfm/sfm/scene/reconstruction/mixins/depth_utils.py     DepthUtils.reproject_depth
                    mpsfm/sfm/scene/reconstruction/mixins/points3D_utils.py  Points3DUtils.lifted_pointcovs_cam, rotate_covs*
  by AST extraction mpsfm/sfm/mapper/depthconsistency.py                      DepthConsistencyChecker.find_min_buffer,
                                                                              check_depth_consistency,
                                                                              check_bundle_depth_concistency
  (the module imports mpsfm.baseclass, which needs omegaconf: absent here, hence the extraction)

These run on a minimal stand-in scene (images with .depth / .cam_from_world / .camera_id / .name, PINHOLE cameras with
sx / sy).  Four images, maps of 40x56 and 36x48: the query (image 0) against a partially overlapping reference, a
reference pulled back (many query pixels share one target pixel) and a rotated one; some depths <= 0 (clamped to 0.1 in
place by the reference), some zero variances.  A scene in which any pixel lies within 1e-9 (relative) of a decision
boundary (integer crossings of the projection, the +0.5 canvas edges, depth = 0, t = +-s) is drawn again.
The file holds inputs and outputs only (masks packed with np.packbits).

Run in the build container:  python tests/golden/make_golden_depth_consistency.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_reference import REF, ROOT, extract_functions, load_by_path  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy_depth_consistency as NDC  # noqa: E402

SIZES = [(40, 56), (36, 48), (40, 56), (36, 48)]  # (H, W) of the maps of images 0..3
IMAGE_SIZE = (560.0, 400.0)  # (width, height) of the camera


def rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def draw_scene(rng):
    """cam_from_world, intrinsics and depth / variance maps of four images looking at a bumpy surface near z = 6."""
    centres = [np.array([0.0, 0.0, 0.0]), np.array([1.2, 0.1, 0.2]), np.array([0.1, -0.2, -7.0]), np.array([-0.4, 0.3, 0.5])]
    angles = [(0, 0, 0), (0.02, -0.15, 0.01), (0.01, 0.0, 0.02), (0.25, 0.1, 0.3)]
    images = []
    for k, ((H, W), C, ang) in enumerate(zip(SIZES, centres, angles)):
        R = rot(*(np.array(ang) + rng.normal(0, 0.01, 3)))
        C = C + rng.normal(0, 0.05, 3)
        t = -R @ C
        f = rng.uniform(480, 560)
        intr = np.array([f, f * rng.uniform(0.98, 1.02), IMAGE_SIZE[0] / 2 + rng.normal(0, 3), IMAGE_SIZE[1] / 2 + rng.normal(0, 3)])
        sx, sy = W / IMAGE_SIZE[0], H / IMAGE_SIZE[1]
        Ks = np.array([[intr[0] * sx, 0, intr[2] * sx], [0, intr[1] * sy, intr[3] * sy], [0, 0, 1.0]])
        y, x = np.mgrid[0:H, 0:W]
        rays = R.T @ (np.linalg.inv(Ks) @ np.stack([x.ravel(), y.ravel(), np.ones(H * W)]))
        lam = (6.0 - C[2]) / rays[2]  # plane z = 6 in the world
        pts = C[:, None] + lam * rays
        bump = 1.5 * np.exp(-((pts[0] - 0.3) ** 2 + (pts[1] + 0.2) ** 2) / 0.5)  # a bump only this image "sees" at random
        depth = lam * (1 + rng.normal(0, 0.01, H * W)) - (bump if k in (1, 3) else 0.0)
        depth = depth.reshape(H, W)
        if k == 0:
            depth[3:6, 10:14] = 0.0
            depth[20, 30:33] = -1.5
        if k == 2:
            depth[0, :4] = -0.2
        var = (rng.uniform(0.002, 0.02, (H, W)) * depth) ** 2
        if k == 1:
            var[30:, :8] = 0.0
        # float32-representable values: the fixture stores the maps in half the bytes
        depth, var = depth.astype(np.float32).astype(np.float64), var.astype(np.float32).astype(np.float64)
        images.append(dict(depth=depth, variance=var, prior_std_multiplier=float(rng.choice([1.0, 2.0, 1.5])), intr=intr,
                           sx=sx, sy=sy, R=R, t=t))
    return images


class _Conf(dict):
    __getattr__ = dict.__getitem__


def reference_objects(images):
    """Stand-in scene with the reference's DepthUtils / Points3DUtils mixins and the extracted checker."""
    DU = load_by_path("ref_depth_utils", "mpsfm/sfm/scene/reconstruction/mixins/depth_utils.py").DepthUtils
    PU = load_by_path("ref_points3d_utils", "mpsfm/sfm/scene/reconstruction/mixins/points3D_utils.py").Points3DUtils
    ns = extract_functions("mpsfm/sfm/mapper/depthconsistency.py", cls="DepthConsistencyChecker",
                           method_names=("find_min_buffer", "check_depth_consistency", "check_bundle_depth_concistency"))

    class Cam:
        def __init__(self, d):
            self.focal_length_x, self.focal_length_y, self.principal_point_x, self.principal_point_y = (float(v) for v in d["intr"])
            self.sx, self.sy = d["sx"], d["sy"]

        def calibration_matrix(self):
            return np.array([[self.focal_length_x, 0, self.principal_point_x], [0, self.focal_length_y, self.principal_point_y],
                             [0, 0, 1.0]])

    class Pose:
        def __init__(self, R, t):
            self.rotation = types.SimpleNamespace(matrix=lambda: R.copy())
            self._M = np.concatenate([R, t[:, None]], 1)

        def matrix(self):
            return self._M.copy()

    class Rec(DU, PU):
        pass

    rec = Rec()
    rec.images, rec.cameras = {}, {}
    for k, d in enumerate(images):
        rec.cameras[k] = Cam(d)
        depth = types.SimpleNamespace(data=d["depth"].copy(), data_prior=d["depth"].copy(), uncertainty=d["variance"].copy(),
                                      conf=types.SimpleNamespace(prior_std_multiplier=d["prior_std_multiplier"]))
        rec.images[k] = types.SimpleNamespace(depth=depth, camera_id=k, cam_from_world=Pose(d["R"], d["t"]), name=f"image{k}.jpg")
    rec.camera = lambda imid: rec.cameras[rec.images[imid].camera_id]

    class Checker(ns["DepthConsistencyChecker"]):
        def __init__(self, rec):
            self.mpsfm_rec = rec
            self.conf = _Conf(depth_cons_valid_thresh=0.6)

        def log(self, *a, **k):
            pass

    return rec, Checker(rec)


def as_entry(d):
    return dict(depth=d["depth"].copy(), variance=d["variance"], prior_std_multiplier=d["prior_std_multiplier"],
                intr_scaled=(d["intr"][0] * d["sx"], d["intr"][1] * d["sy"], d["intr"][2] * d["sx"], d["intr"][3] * d["sy"]),
                intr=d["intr"], cam_from_world=np.concatenate([d["R"], d["t"][:, None]], 1))


PAIRS = [(0, 1), (0, 2), (0, 3), (2, 3)]
THRESHOLDS = (0.6, 0.8)


def near_boundary(images):
    """Pixels within 1e-9 of a decision boundary, by the reference's own reprojection and by the restatement's t."""
    rec, _ = reference_objects(images)
    n = 0
    for a, b in PAIRS:
        for s_, d_ in ((a, b), (b, a)):
            out = rec.reproject_depth(s_, d_)
            p, z = out["p2D12"].reshape(-1, 2), out["depth12"].ravel()
            H, W = images[d_]["depth"].shape
            for v, edge in ((p[:, 0], W - 0.5), (p[:, 1], H - 0.5)):
                n += np.count_nonzero(np.abs(v - np.round(v)) <= 1e-9 * np.maximum(1, np.abs(v)))
                n += np.count_nonzero(np.abs(v - edge) <= 1e-9 * edge)
            n += np.count_nonzero(np.abs(z) <= 1e-9 * np.maximum(1, np.abs(out["depth1"].ravel())))
        ents = [as_entry(d) for d in images]
        for s in THRESHOLDS:
            l12, l21 = NDC.pair(ents, a, b, s=s)
            n += int(l12["near"].sum() + l21["near"].sum())
    return n


def generate():
    rng = np.random.default_rng(20261016)
    for attempt in range(50):
        images = draw_scene(rng)
        if near_boundary(images) == 0:
            break
        print("redraw: pixels near a decision boundary")
    else:
        raise RuntimeError("no clean scene in 50 draws")
    out = {"n_images": len(images), "pairs": np.array(PAIRS, np.int32), "thresholds": np.array(THRESHOLDS)}
    for k, d in enumerate(images):
        out[f"im{k}_depth"] = d["depth"].astype(np.float32)  # exact: the maps are float32 values
        out[f"im{k}_variance"] = d["variance"].astype(np.float32)
        out[f"im{k}_psm"] = d["prior_std_multiplier"]
        out[f"im{k}_intr"] = d["intr"]
        out[f"im{k}_sxsy"] = np.array([d["sx"], d["sy"]])
        out[f"im{k}_cam_from_world"] = np.concatenate([d["R"], d["t"][:, None]], 1)
    for si, s in enumerate(THRESHOLDS):
        for pi, (a, b) in enumerate(PAIRS):
            rec, chk = reference_objects(images)
            res = chk.check_depth_consistency(a, b, score_thresh=s)
            for key in NDC.MASK_KEYS:
                out[f"s{si}_pair{pi}_{key}"] = np.packbits(res[key].ravel())
            if si == 0 and pi == 0:
                changed = np.flatnonzero(rec.images[0].depth.data.ravel() != images[0]["depth"].ravel())
                out["clamped0_index"] = changed.astype(np.int32)  # pixels of image 0 the reference clamped in place
                out["clamped0_value"] = rec.images[0].depth.data.ravel()[changed]
        rec, chk = reference_objects(images)
        score, sums = chk.check_bundle_depth_concistency(0, {"optim_ids": {0, 1, 2, 3}}, score_thresh=s)
        out[f"s{si}_bundle_score"] = float(score)
        out[f"s{si}_bundle_sums"] = np.array(sums, np.int64)
        print(f"score_thresh {s}: bundle score {score:.6f}, in-canvas sums {sums}")
    # how many query pixels share a target in the pulled-back reference (collision-heavy pair (0, 2))
    l02, _ = NDC.pair([as_entry(d) for d in images], 0, 2)
    tg = l02["target"][l02["target"] >= 0]
    print("pair (0, 2): query pixels in canvas", tg.size, "distinct targets", np.unique(tg).size)
    for pi, (a, b) in enumerate(PAIRS):
        l12, l21 = NDC.pair([as_entry(d) for d in images], a, b)
        print(f"pair {(a, b)} counts (in, surface, occl, invalid):", NDC.counts_of(l12["code"]), NDC.counts_of(l21["code"]))
    return out


if __name__ == "__main__":
    assert os.path.isdir(REF), REF
    out = generate()
    path = os.path.join(HERE, "reference_depth_consistency.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")
