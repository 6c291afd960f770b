"""3D-3D alignment over libmpsfm_hip: ``estimate_rigid3d`` / ``estimate_sim3d``, their ``_robust`` forms and
``register_depth_pair``; dense point-to-plane ICP of an RGB-D pair behind it: ``depth_to_normals``, ``refine_depth_pair``,
``register_depth_pair_dense`` (``csrc/depth_icp.hip``).

The reference has no estimator of this kind under ``mpsfm/``; its fork adds ``icp/main.py``, which registers an RGB-D pair
with 5000 Python iterations of 3-point rigid alignment (``rigid_transform_3D``, :149-175) over depth-lifted keypoint matches.
``register_depth_pair`` replaces lines 105-193 of that script; the four ``estimate_*`` functions are the same arithmetic on
point sets the caller already holds.  Their names and return values are pycolmap's (``pycolmap.estimate_rigid3d`` ...,
COLMAP 3.11's EstimateRigid3d(Robust) / EstimateSim3d(Robust)) as recalled: parity with pycolmap is unpinned.  Everything runs
in ``csrc/align3d.hip`` (``mpsfm_align3d_fit``, ``mpsfm_align3d_estimate``, ``mpsfm_depth_pair_register``).

Deviations, documented in DESIGN.md section 4w: the sampler is counter-based, so every call is deterministic
(``random_seed < 0`` maps to seed 0); collinear samples and point sets on a line give no model; the defaults of the robust forms
are the fork's where it sets a value (``max_error`` 0.1, 5000 trials).
"""

from __future__ import annotations

import numpy as np

from ... import capi
from ...synthetic import quat_from_R
from .absolute_pose import _Rotation3d

RANSAC_DEFAULTS = {k: v for k, v in capi.ALIGN3D_DEFAULTS.items() if k not in ("seed", "batch_trials")}
RANSAC_DEFAULTS["random_seed"] = -1
ICP_DEFAULTS = dict(capi.ICP_DEFAULTS)


class Sim3d:
    """tgt_from_src: x_tgt = scale * R x_src + t, with the attributes of pycolmap.Sim3d (and, at scale 1, Rigid3d) that callers
    read: ``scale``, ``rotation.matrix()``, ``rotation.quat`` (xyzw), ``translation``, ``matrix()`` = [scale R | t]."""

    def __init__(self, scale, quat_xyzw, translation):
        self.scale = float(scale)
        self.rotation = _Rotation3d(quat_xyzw)
        self.translation = np.asarray(translation, np.float64)

    def matrix(self):
        return np.concatenate([self.scale * self.rotation.matrix(), self.translation[:, None]], axis=1)


def _transform(res) -> Sim3d:
    M = res["tgt_from_src"]
    return Sim3d(res["scale"], quat_from_R(M[:, :3])[0], M[:, 3].copy())


def _ransac_kwargs(ransac_options) -> dict:
    o = dict(RANSAC_DEFAULTS)
    given = dict(ransac_options or {})
    unknown = set(given) - set(o)
    if unknown:
        raise KeyError(f"unknown RANSAC option(s) {sorted(unknown)}")
    o.update(given)
    seed = int(o.pop("random_seed"))
    return dict(o, seed=seed if seed >= 0 else 0)


def _fit(src, tgt, with_scale, device):
    if len(np.asarray(src).reshape(-1, 3)) < 3:
        return None
    res = capi.align3d_fit(src, tgt, with_scale=with_scale, device=device)
    return _transform(res) if res["success"] else None


def _robust(src, tgt, with_scale, ransac_options, device):
    if len(np.asarray(src).reshape(-1, 3)) < 3:
        return None
    res = capi.align3d_estimate(src, tgt, with_scale=with_scale, device=device, **_ransac_kwargs(ransac_options))
    if not res["success"]:
        return None
    return {"tgt_from_src": _transform(res), "num_inliers": res["num_inliers"], "inlier_mask": res["inlier_mask"], "report": res}


def estimate_rigid3d(src, tgt, device=0):
    """The least-squares rigid transform tgt ~ R src + t of [n, 3] point pairs, or None (fewer than 3 points, points on a line).
    Name and return value are pycolmap.estimate_rigid3d's as recalled: parity with pycolmap unpinned."""
    return _fit(src, tgt, False, device)


def estimate_sim3d(src, tgt, device=0):
    """The least-squares similarity tgt ~ s R src + t of [n, 3] point pairs, or None.  pycolmap.estimate_sim3d's name and
    return value as recalled: parity with pycolmap unpinned."""
    return _fit(src, tgt, True, device)


def estimate_rigid3d_robust(src, tgt, ransac_options=None, device=0):
    """LO-RANSAC of tgt ~ R src + t.  ``ransac_options``: keys of RANSAC_DEFAULTS.  Returns None when no model is found, else
    ``{"tgt_from_src", "num_inliers", "inlier_mask", "report"}``; ``report`` is capi.align3d_estimate's dict.
    pycolmap.estimate_rigid3d_robust's name and return value as recalled: parity with pycolmap unpinned."""
    return _robust(src, tgt, False, ransac_options, device)


def estimate_sim3d_robust(src, tgt, ransac_options=None, device=0):
    """LO-RANSAC of tgt ~ s R src + t; see estimate_rigid3d_robust.  pycolmap.estimate_sim3d_robust's name and return value as
    recalled: parity with pycolmap unpinned."""
    return _robust(src, tgt, True, ransac_options, device)


def register_depth_pair(kps0, kps1, matches, depth0, depth1, intr0, intr1, with_scale=False, device=0, **ransac):
    """icp/main.py:105-193 in one call: the matched keypoints of both images are lifted through their depth maps (float32 or
    float64 [H, W]; float32 is widened exactly; PINHOLE intr = fx, fy, cx, cy) and image 0's points are aligned to image 1's.
    ``matches`` [m, 2] holds (keypoint of image 0, keypoint of image 1); ``ransac``: keys of RANSAC_DEFAULTS.  Returns None when no
    model is found, else ``{"tgt_from_src" (cam1_from_cam0), "num_inliers", "inlier_mask" [m], "valid" [m], "lifted0", "lifted1",
    "report"}``.  A match with an end on the border, outside the map or over a depth hole is not valid and takes no part."""
    res = capi.depth_pair_register(depth0, intr0, depth1, intr1, kps0, kps1, matches, with_scale=with_scale, device=device,
                                   **_ransac_kwargs(ransac))
    if not res["success"]:
        return None
    return {"tgt_from_src": _transform(res), "num_inliers": res["num_inliers"], "inlier_mask": res["inlier_mask"], "valid": res["valid"],
            "lifted0": res["lifted0"], "lifted1": res["lifted1"], "report": res}


def depth_to_normals(depth, intr, edge_ratio=ICP_DEFAULTS["edge_ratio"], device=0):
    """The camera-facing normal map of a depth map (float32 or float64 [H, W]; PINHOLE intr = fx, fy, cx, cy) as the ICP forms
    it: central differences of the vertex map, no normal on the border, over a hole or across a depth edge (a neighbour's depth
    differs by more than ``edge_ratio`` of the pixel's).  Returns (normals [H, W, 3], valid bool [H, W])."""
    return capi.depth_normals(depth, intr, edge_ratio=edge_ratio, device=device)


def _pose_and_scale(tgt_from_src, scale):
    if isinstance(tgt_from_src, Sim3d):
        return np.concatenate([tgt_from_src.rotation.matrix(), tgt_from_src.translation[:, None]], axis=1), tgt_from_src.scale
    return np.asarray(tgt_from_src, np.float64).reshape(3, 4), 1.0 if scale is None else float(scale)


def _refined(res) -> dict:
    return {"tgt_from_src": _transform(res), "status": res["status"], "iterations": res["iterations"], "num_pairs": res["num_pairs"],
            "rmse": res["rmse"], "information": res["info"], "trace": res["trace"], "report": res}


def refine_depth_pair(depth0, depth1, intr0, intr1, tgt_from_src, scale=None, device=0, **icp):
    """Dense projective point-to-plane ICP of depth map 0 onto depth map 1 from ``tgt_from_src``: a ``Sim3d`` (its scale is kept),
    or a 3 x 4 array [R | t] with ``scale`` (default 1).  The scale is held constant; R and t are refined.  ``icp``: keys of
    ICP_DEFAULTS.  Returns ``{"tgt_from_src" (Sim3d), "status" ("converged", "max_iterations", "too_few_pairs", "singular"),
    "iterations", "num_pairs", "rmse", "information" [6, 6] (order rotation, translation), "trace" [iterations, 4], "report"}``;
    ``report`` is capi.depth_pair_icp's dict."""
    T, s = _pose_and_scale(tgt_from_src, scale)
    return _refined(capi.depth_pair_icp(depth0, intr0, depth1, intr1, T, scale=s, device=device, **icp))


def register_depth_pair_dense(kps0, kps1, matches, depth0, depth1, intr0, intr1, with_scale=False, device=0, icp=None, **ransac):
    """``register_depth_pair`` followed by ``refine_depth_pair`` from its model, in one call that uploads the maps once.  ``icp``: a
    dict with keys of ICP_DEFAULTS; ``ransac``: keys of RANSAC_DEFAULTS.  Returns None when the RANSAC finds no model, else
    ``register_depth_pair``'s dict plus ``"refined"``: ``refine_depth_pair``'s dict."""
    res = capi.depth_pair_register_dense(depth0, intr0, depth1, intr1, kps0, kps1, matches, with_scale=with_scale, device=device, icp=icp,
                                         **_ransac_kwargs(ransac))
    if not res["success"]:
        return None
    return {"tgt_from_src": _transform(res), "num_inliers": res["num_inliers"], "inlier_mask": res["inlier_mask"], "valid": res["valid"],
            "lifted0": res["lifted0"], "lifted1": res["lifted1"], "report": res, "refined": _refined(res["refined"])}
