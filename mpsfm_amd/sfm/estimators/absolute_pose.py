"""Drop-in ``AbsolutePose`` over libmpsfm_hip.

Mirror of reference ``mpsfm/sfm/estimators/absolute_pose.py`` (class AbsolutePose, :6-25), which calls
``pycolmap.estimate_and_refine_absolute_pose``.  The estimation (COLMAP's LO-RANSAC with P3P samples and EPnP local
optimisation) runs in ``csrc/abs_pose.hip`` through ``mpsfm_abs_pose_estimate``; the refinement (COLMAP's
RefineAbsolutePose: Ceres LM on the pose alone, Cauchy loss on the inlier reprojection errors, intrinsics constant) is one
``mpsfm_ba_solve`` of a one-camera problem whose landmarks are the constant inlier points.  Returns None where pycolmap
would (no model), else ``{"cam_from_world", "num_inliers", "inlier_mask"}`` with RANSAC's mask and the refined pose.

Deviations, all documented in DESIGN.md section 4g: the sampler is counter-based, so ``random_seed < 0`` (pycolmap: seeded
from the clock) maps to the fixed seed 0 and every call is deterministic; focal-length estimation and refinement and the
refinement of extra parameters are refused (NotImplementedError); cameras other than (SIMPLE_)PINHOLE are refused.
"""

from __future__ import annotations

import copy

import numpy as np

from ... import capi
from ...baseclass import BaseClass, to_conf
from ...problem import LOSS_CAUCHY, BAProblem
from ...synthetic import quat_from_R
from ..mapper.bundle_adjustment import pinhole_params

# pycolmap 3.11 defaults as recalled (AbsolutePoseEstimationOptions / RANSACOptions / AbsolutePoseRefinementOptions)
ESTIMATION_DEFAULTS = {
    "estimate_focal_length": False,
    "ransac": {
        "max_error": 12.0,
        "min_inlier_ratio": 0.25,  # the reference's override of pycolmap's 0.1
        "confidence": 0.99999,
        "dyn_num_trials_multiplier": 3.0,
        "min_num_trials": 100,
        "max_num_trials": 10000,
        "random_seed": -1,
    },
}
REFINEMENT_DEFAULTS = {
    "gradient_tolerance": 1.0,
    "max_num_iterations": 100,
    "loss_function_scale": 1.0,
    "refine_focal_length": False,
    "refine_extra_params": False,
    "print_summary": False,
}


def _fill(defaults: dict, given, path: str) -> dict:
    """defaults with the given (possibly partial, possibly nested) values; unknown keys are an error"""
    out = copy.deepcopy(defaults)
    for k, v in (given or {}).items():
        if k not in defaults:
            raise KeyError(f"unknown configuration key {path}{k!r} for AbsolutePose")
        out[k] = _fill(defaults[k], v, f"{path}{k}.") if isinstance(defaults[k], dict) else v
    return out


class _Rotation3d:
    def __init__(self, quat_xyzw):
        self.quat = np.asarray(quat_xyzw, np.float64)

    def matrix(self):
        x, y, z, w = self.quat
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


class _Rigid3d:
    """cam_from_world when pycolmap is absent: x_cam = R x_world + t, the attributes of pycolmap.Rigid3d the mapper reads."""

    def __init__(self, quat_xyzw, translation):
        self.rotation = _Rotation3d(quat_xyzw)
        self.translation = np.asarray(translation, np.float64)

    def matrix(self):
        return np.concatenate([self.rotation.matrix(), self.translation[:, None]], axis=1)


def make_rigid3d(quat_xyzw, translation):
    try:
        import pycolmap
    except ImportError:
        return _Rigid3d(quat_xyzw, translation)
    return pycolmap.Rigid3d(pycolmap.Rotation3d(np.asarray(quat_xyzw, np.float64)), np.asarray(translation, np.float64))


class AbsolutePose(BaseClass):
    """Absolute pose estimation (LO-RANSAC + refinement) on the GPU."""

    default_conf = {
        "colmap_estimation_options": ESTIMATION_DEFAULTS,
        "colmap_refinement_options": REFINEMENT_DEFAULTS,
        "verbose": 0,
    }

    @classmethod
    def _merged_conf(cls, conf):
        given = to_conf(conf)
        merged = super()._merged_conf(
            {k: v for k, v in given.items() if k not in ("colmap_estimation_options", "colmap_refinement_options")})
        merged["colmap_estimation_options"] = to_conf(_fill(ESTIMATION_DEFAULTS, given.get("colmap_estimation_options"), ""))
        merged["colmap_refinement_options"] = to_conf(_fill(REFINEMENT_DEFAULTS, given.get("colmap_refinement_options"), ""))
        return merged

    def _assert_configs(self):
        e, r = self.conf.colmap_estimation_options, self.conf.colmap_refinement_options
        for name, on in (("estimate_focal_length", e.estimate_focal_length), ("refine_focal_length", r.refine_focal_length),
                         ("refine_extra_params", r.refine_extra_params)):
            if on:
                raise NotImplementedError(f"AbsolutePose: {name}=True is not implemented by the HIP path")

    def _init(self, device: int = 0):
        self.device = device

    def __call__(self, points2D, points3D, camera):
        intr = pinhole_params(camera)
        p2 = np.ascontiguousarray(points2D, np.float64).reshape(-1, 2)
        p3 = np.ascontiguousarray(points3D, np.float64).reshape(-1, 3)
        if len(p2) != len(p3):
            raise ValueError("points2D and points3D differ in length")
        if len(p2) < 3:
            return None
        ro = self.conf.colmap_estimation_options.ransac
        seed = int(ro.random_seed)
        est = capi.abs_pose_estimate(p2, p3, intr, device=self.device, max_error=float(ro.max_error),
                                     min_inlier_ratio=float(ro.min_inlier_ratio), confidence=float(ro.confidence),
                                     dyn_num_trials_multiplier=float(ro.dyn_num_trials_multiplier),
                                     min_num_trials=int(ro.min_num_trials), max_num_trials=int(ro.max_num_trials),
                                     seed=seed if seed >= 0 else 0)
        if not est["success"]:
            return None
        mask = est["inlier_mask"]
        q, t, summary = self.refine(est["cam_from_world"], p2[mask], p3[mask], intr)
        self.last_estimate, self.last_refinement = est, summary
        self.log(f"absolute pose: {est['num_inliers']} inliers after {est['num_trials']} trials, refinement "
                 f"{summary['num_iterations']} iterations ({summary['termination']})", level=1)
        return {"cam_from_world": make_rigid3d(q, t), "num_inliers": est["num_inliers"], "inlier_mask": mask}

    def refinement_problem(self, cam_from_world, points2D, points3D, intr) -> BAProblem:
        """RefineAbsolutePose as a bundle-adjustment problem: one variable camera, every inlier a constant landmark with one
        observation, Cauchy loss of scale loss_function_scale on the pixel reprojection error, no gauge fixing."""
        P = np.asarray(cam_from_world, np.float64).reshape(3, 4)
        m = len(points3D)
        return BAProblem(
            cam_quat=quat_from_R(P[:, :3])[0], cam_t=P[:, 3].copy(), pts=np.asarray(points3D, np.float64).reshape(-1, 3).copy(),
            cam_intr=np.asarray(intr, np.float64).reshape(1, 4), cam_intr_idx=np.zeros(1, np.int32), pose_const=np.zeros(1, np.uint8),
            pt_const=np.ones(m, np.uint8), obs_cam=np.zeros(m, np.int32), obs_pt=np.arange(m, dtype=np.int32),
            obs_xy=np.asarray(points2D, np.float64).reshape(-1, 2), gauge_axis_cam=-1, reproj_loss_type=LOSS_CAUCHY,
            reproj_loss_scale=float(self.conf.colmap_refinement_options.loss_function_scale), reproj_loss_magnitude=1.0)

    def solver_options(self):
        r = self.conf.colmap_refinement_options
        return capi.default_options(max_num_iterations=int(r.max_num_iterations), gradient_tolerance=float(r.gradient_tolerance),
                                    device=int(self.device))

    def refine(self, cam_from_world, points2D, points3D, intr):
        prob = self.refinement_problem(cam_from_world, points2D, points3D, intr)
        summary = capi.ba_solve(prob, self.solver_options())
        return prob.cam_quat[0].copy(), prob.cam_t[0].copy(), summary
