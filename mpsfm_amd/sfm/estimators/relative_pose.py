"""Drop-in ``RelativePose`` over libmpsfm_hip.

Mirror of reference ``mpsfm/sfm/estimators/relative_pose.py`` (class RelativePose, :7-17), which calls
``pycolmap.essential_matrix_estimation``.  The estimation (COLMAP's LO-RANSAC with five-point samples and five-point local
optimisation on the Sampson error) and the pose of the best essential matrix (decomposition, cheirality test on the inliers)
run in ``csrc/rel_pose.hip`` through ``mpsfm_rel_pose_estimate``.  Returns None where pycolmap would (no model), else
``{"E", "cam2_from_cam1", "num_inliers", "inlier_mask"}`` with RANSAC's mask; pycolmap refines nothing after RANSAC, and
neither does this.

Deviations, all documented in DESIGN.md section 4h: the sampler is counter-based, so ``random_seed < 0`` (pycolmap: seeded
from the clock) maps to the fixed seed 0 and every call is deterministic; the models of a trial are canonical and in
lexicographic order; cameras other than (SIMPLE_)PINHOLE are refused.
"""

from __future__ import annotations

import numpy as np

from ... import capi
from ...baseclass import BaseClass, to_conf
from ...synthetic import quat_from_R
from ..mapper.bundle_adjustment import pinhole_params
from .absolute_pose import _fill, make_rigid3d

# pycolmap 3.11 RANSACOptions() as recalled (the binding's overrides of COLMAP's struct defaults)
RANSAC_DEFAULTS = {
    "max_error": 4.0,
    "min_inlier_ratio": 0.01,
    "confidence": 0.9999,
    "dyn_num_trials_multiplier": 3.0,
    "min_num_trials": 1000,
    "max_num_trials": 100000,
    "random_seed": -1,
}


class RelativePose(BaseClass):
    """Relative pose estimation (five-point LO-RANSAC + pose from E) on the GPU."""

    default_conf = {
        "colmap_options": RANSAC_DEFAULTS,
        "verbose": 0,
    }

    @classmethod
    def _merged_conf(cls, conf):
        given = to_conf(conf)
        merged = super()._merged_conf({k: v for k, v in given.items() if k != "colmap_options"})
        merged["colmap_options"] = to_conf(_fill(RANSAC_DEFAULTS, given.get("colmap_options"), "colmap_options."))
        return merged

    def _init(self, device: int = 0):
        self.device = device

    def __call__(self, points1, points2, camera1, camera2):
        intr1, intr2 = pinhole_params(camera1), pinhole_params(camera2)
        p1 = np.ascontiguousarray(points1, np.float64).reshape(-1, 2)
        p2 = np.ascontiguousarray(points2, np.float64).reshape(-1, 2)
        if len(p1) != len(p2):
            raise ValueError("points1 and points2 differ in length")
        if len(p1) < 5:
            return None
        ro = self.conf.colmap_options
        seed = int(ro.random_seed)
        est = capi.rel_pose_estimate(p1, p2, intr1, intr2, device=self.device, max_error=float(ro.max_error),
                                     min_inlier_ratio=float(ro.min_inlier_ratio), confidence=float(ro.confidence),
                                     dyn_num_trials_multiplier=float(ro.dyn_num_trials_multiplier),
                                     min_num_trials=int(ro.min_num_trials), max_num_trials=int(ro.max_num_trials),
                                     seed=seed if seed >= 0 else 0)
        self.last_estimate = est
        if not est["success"]:
            return None
        P = est["cam2_from_cam1"]
        self.log(f"relative pose: {est['num_inliers']} inliers after {est['num_trials']} trials, "
                 f"{est['num_cheirality_points']} in front of both cameras", level=1)
        return {"E": est["E"], "cam2_from_cam1": make_rigid3d(quat_from_R(P[:, :3])[0], P[:, 3]),
                "num_inliers": est["num_inliers"], "inlier_mask": est["inlier_mask"]}
