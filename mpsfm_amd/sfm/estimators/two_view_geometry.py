"""Drop-in ``estimate_calibrated_two_view_geometry`` over libmpsfm_hip.

Mirror of ``pycolmap.estimate_calibrated_two_view_geometry`` as the reference calls it
(``mpsfm/sfm/scene/correspondences/utils.py:13-32``): the E, F and H LO-RANSACs of one image pair, COLMAP's decision between
them, the watermark test and the relative pose run in ``csrc/two_view.hip`` through ``mpsfm_two_view_geometry``.  The result
carries what the reference reads: ``config`` (compares equal to the plain ints of ``find_init_pairs``), ``inlier_matches``,
``cam2_from_cam1`` and ``tri_angle``, plus ``E``, ``F``, ``H`` and ``invert()``.

Deviations, all documented in DESIGN.md section 4j: the sampler is counter-based, so ``random_seed < 0`` maps to the fixed
seed 0 and every call is deterministic; models are canonical and a trial's models are in lexicographic order; cameras other
than (SIMPLE_)PINHOLE are refused; ``multiple_models`` / ``force_H_use`` are not provided.
``estimate_calibrated_two_view_geometry_batch`` takes many pairs in one call (``mpsfm_two_view_geometry_batch``, section 4k).
"""

from __future__ import annotations

from enum import IntEnum

import numpy as np

from ... import capi
from ...synthetic import quat_from_R
from ..mapper.bundle_adjustment import pinhole_params
from .absolute_pose import make_rigid3d


class TwoViewGeometryConfig(IntEnum):
    """COLMAP's TwoViewGeometry::ConfigurationType."""

    UNDEFINED = 0
    DEGENERATE = 1
    CALIBRATED = 2
    UNCALIBRATED = 3
    PLANAR = 4
    PANORAMIC = 5
    PLANAR_OR_PANORAMIC = 6
    WATERMARK = 7
    MULTIPLE = 8


# COLMAP 3.11 TwoViewGeometryOptions as recalled; "ransac" nests pycolmap's RANSACOptions keys
OPTION_DEFAULTS = {
    "min_num_inliers": 15,
    "min_E_F_inlier_ratio": 0.95,
    "max_H_inlier_ratio": 0.8,
    "watermark_min_inlier_ratio": 0.7,
    "watermark_border_size": 0.1,
    "detect_watermark": True,
    "compute_relative_pose": False,
    "ransac": {
        "max_error": 4.0,
        "min_inlier_ratio": 0.25,
        "confidence": 0.999,
        "dyn_num_trials_multiplier": 3.0,
        "min_num_trials": 100,
        "max_num_trials": 10000,
        "random_seed": -1,
    },
}
UNSUPPORTED_OPTIONS = ("multiple_models", "force_H_use", "multiple_ignore_watermark")


def _identity_pose():
    return make_rigid3d(np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3))


def _pose_matrix(pose) -> np.ndarray:
    M = pose.matrix()
    return np.asarray(M() if callable(M) else M, np.float64)[:3, :4]


class TwoViewGeometry:
    """What pycolmap.TwoViewGeometry holds: config, E, F, H, cam2_from_cam1, inlier_matches [(k, 2) int], tri_angle."""

    def __init__(self, config=TwoViewGeometryConfig.UNDEFINED, E=None, F=None, H=None, cam2_from_cam1=None, inlier_matches=None,
                 tri_angle=0.0):
        self.config = TwoViewGeometryConfig(int(config))
        self.E = np.zeros((3, 3)) if E is None else np.asarray(E, np.float64)
        self.F = np.zeros((3, 3)) if F is None else np.asarray(F, np.float64)
        self.H = np.zeros((3, 3)) if H is None else np.asarray(H, np.float64)
        self.cam2_from_cam1 = _identity_pose() if cam2_from_cam1 is None else cam2_from_cam1
        self.inlier_matches = np.zeros((0, 2), np.uint32) if inlier_matches is None else np.asarray(inlier_matches)
        self.tri_angle = float(tri_angle)

    def invert(self):
        """COLMAP's TwoViewGeometry::Invert, in place: E and F transposed, H inverted, the pose inverted, match columns
        swapped."""
        self.E = self.E.T.copy()
        self.F = self.F.T.copy()
        self.H = np.linalg.inv(self.H) if np.any(self.H) else self.H.copy()
        M = _pose_matrix(self.cam2_from_cam1)
        R, t = M[:, :3].T, -M[:, :3].T @ M[:, 3]
        self.cam2_from_cam1 = make_rigid3d(quat_from_R(R)[0], t)
        self.inlier_matches = np.ascontiguousarray(self.inlier_matches[:, ::-1])

    def __repr__(self):
        return f"TwoViewGeometry(config={self.config.name}, num_inliers={len(self.inlier_matches)}, tri_angle={self.tri_angle:.6g})"


def _merge_options(options) -> dict:
    o = {k: (dict(v) if isinstance(v, dict) else v) for k, v in OPTION_DEFAULTS.items()}
    given = {} if options is None else dict(options)
    for k, v in given.items():
        if k in UNSUPPORTED_OPTIONS:
            if v:
                raise NotImplementedError(f"two-view geometry option {k} is not provided (DESIGN.md section 4j)")
            continue
        if k not in o:
            raise KeyError(f"unknown two-view geometry option {k}")
        if k == "ransac":
            for rk, rv in dict(v).items():
                if rk not in o["ransac"]:
                    raise KeyError(f"unknown option ransac.{rk}")
                o["ransac"][rk] = rv
        else:
            o[k] = v
    return o


def _image_size(camera, intr) -> tuple[int, int]:
    w, h = getattr(camera, "width", None), getattr(camera, "height", None)
    if w is None or h is None or int(w) <= 0 or int(h) <= 0:  # a camera without a size: the principal point at the centre
        return max(int(round(2 * intr[2])), 1), max(int(round(2 * intr[3])), 1)
    return int(w), int(h)


def _prepare(cam0, kps0, cam1, kps1, matches, what="a match"):
    """One pair as the backend takes it: (positional arguments of two_view_geometry, the match rows)."""
    intr0, intr1 = pinhole_params(cam0), pinhole_params(cam1)
    m = np.asarray(matches)
    if m.size == 0:
        m = m.reshape(0, 2)
    if m.ndim != 2 or m.shape[1] != 2:
        raise ValueError("matches must be [m, 2]")
    k0 = np.asarray(kps0, np.float64).reshape(-1, 2)
    k1 = np.asarray(kps1, np.float64).reshape(-1, 2)
    idx = m.astype(np.int64)
    if len(idx) and (idx.min() < 0 or idx[:, 0].max() >= len(k0) or idx[:, 1].max() >= len(k1)):
        raise IndexError(f"{what} indexes past the keypoints")
    return (k0[idx[:, 0]], k1[idx[:, 1]], intr0, intr1, _image_size(cam0, intr0), _image_size(cam1, intr1)), m


def _backend_options(options) -> dict:
    """The nested option dict as the keyword arguments of the backend."""
    o = _merge_options(options)
    ro = o.pop("ransac")
    seed = int(ro.pop("random_seed"))
    return dict(seed=seed if seed >= 0 else 0, **ro, **o)


def _result(est, m, compute_relative_pose) -> TwoViewGeometry:
    P = np.asarray(est["cam2_from_cam1"], np.float64)
    pose = make_rigid3d(quat_from_R(P[:, :3])[0], P[:, 3]) if est["config"] in (2, 3, 4, 5) and compute_relative_pose else None
    tvg = TwoViewGeometry(est["config"], est["E"], est["F"], est["H"], pose, m[np.asarray(est["inlier_mask"], bool)], est["tri_angle"])
    tvg.estimate = est
    return tvg


def estimate_calibrated_two_view_geometry(cam0, kps0, cam1, kps1, matches, options=None, device: int = 0, backend=None) -> TwoViewGeometry:
    """The two-view geometry of one pair: keypoints [n, 2] pixels of both images, matches [(m, 2) int] into them, and the
    nested option dict the reference passes ({"ransac": {...}, "compute_relative_pose": True}).  `backend`: an object with
    capi's ``two_view_geometry`` (tests inject the NumPy restatement); None: libmpsfm_hip."""
    kw = _backend_options(options)
    args, m = _prepare(cam0, kps0, cam1, kps1, matches)
    est = (backend or capi).two_view_geometry(*args, device=device, **kw)
    return _result(est, m, kw["compute_relative_pose"])


def estimate_calibrated_two_view_geometry_batch(items, options=None, device: int = 0, backend=None) -> list:
    """The two-view geometries of many pairs in one call of ``mpsfm_two_view_geometry_batch``: `items` is a sequence of
    (cam0, kps0, cam1, kps1, matches), `options` serve every pair; the list of TwoViewGeometry in input order, each what
    estimate_calibrated_two_view_geometry returns for that pair.  A `backend` without ``two_view_geometry_batch`` is called
    pair by pair."""
    kw = _backend_options(options)
    prepared = [_prepare(*item, what=f"pair {k}: a match") for k, item in enumerate(items)]
    be = backend or capi
    if hasattr(be, "two_view_geometry_batch"):
        ests = be.two_view_geometry_batch([args for args, _ in prepared], device=device, **kw)
    else:
        ests = [be.two_view_geometry(*args, device=device, **kw) for args, _ in prepared]
    return [_result(est, m, kw["compute_relative_pose"]) for est, (_, m) in zip(ests, prepared)]
