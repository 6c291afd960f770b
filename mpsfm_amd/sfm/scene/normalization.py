"""Normalisation of a scene: ``MpsfmReconstruction.normalize`` (reference mpsfm/sfm/scene/reconstruction/base.py:116-121),
which calls COLMAP 3.11's ``Reconstruction::Normalize`` through pycolmap and then scales the depth maps.

``normalize`` restates COLMAP's rule (parity with pycolmap itself is not pinned by a fixture):
the coordinates — the point positions, or with ``use_images`` the projection centres of the posed images — are cast to
float32 and sorted per axis; with n of them, P0 = int(min_percentile (n - 1)) and P1 = int(max_percentile (n - 1)) when
n > 3, else 0 and n - 1; the box is the per-axis [P0] and [P1], the centroid the per-axis mean of the sorted entries
P0..P1 accumulated in float64; scale = extent / |max - min| unless ``fixed_scale`` or the box is smaller than
DBL_EPSILON.  Every point becomes scale (X - c); every posed image keeps its rotation R and gets t' = scale (t + R c),
so that every camera-frame coordinate, depths included, is multiplied by scale and every reprojection stays.
Plain NumPy on the host: a few thousand coordinates, once per global-refinement iteration.
"""

from __future__ import annotations

import numpy as np


def _coordinates(scene, use_images):
    if use_images:
        out = []
        for image in scene.images.values():
            if image.has_pose:
                R = image.cam_from_world.rotation.matrix()
                out.append(-R.T @ np.asarray(image.cam_from_world.translation, np.float64))
        return np.array(out, np.float64).reshape(-1, 3)
    ids = list(scene.points3D.keys())
    if hasattr(scene, "point3D_coordinates"):
        return np.asarray(scene.point3D_coordinates(ids), np.float64).reshape(-1, 3)
    return np.array([scene.points3D[i].xyz for i in ids], np.float64).reshape(-1, 3)


def bounding_box_and_centroid(coords, min_percentile, max_percentile):
    """(box min [3], box max [3], centroid [3]) of [n, 3] coordinates by the rule above; n >= 1."""
    srt = np.sort(np.asarray(coords, np.float64).astype(np.float32), axis=0)
    n = len(srt)
    p0 = int(min_percentile * (n - 1)) if n > 3 else 0
    p1 = int(max_percentile * (n - 1)) if n > 3 else n - 1
    lo, hi = srt[p0].astype(np.float64), srt[p1].astype(np.float64)
    centroid = srt[p0:p1 + 1].astype(np.float64).sum(axis=0) / (p1 - p0 + 1)
    return lo, hi, centroid


def normalize(scene, fixed_scale=False, extent=5, min_percentile=0.2, max_percentile=0.8, use_images=False):
    """Normalises the scene in place; returns (scale, translation) of the applied similarity X' = scale X + translation."""
    coords = _coordinates(scene, use_images)
    if len(coords) < 2:
        return 1.0, np.zeros(3)
    lo, hi, c = bounding_box_and_centroid(coords, min_percentile, max_percentile)
    old_extent = float(np.linalg.norm(hi - lo))
    scale = 1.0 if fixed_scale or old_extent < np.finfo(np.float64).eps else float(extent) / old_extent
    ids = list(scene.points3D.keys())
    if ids:
        if hasattr(scene, "point3D_coordinates") and hasattr(scene, "set_point3D_coordinates"):
            scene.set_point3D_coordinates(ids, scale * (np.asarray(scene.point3D_coordinates(ids), np.float64).reshape(-1, 3) - c))
        else:
            for i in ids:
                scene.points3D[i].xyz = scale * (np.asarray(scene.points3D[i].xyz, np.float64) - c)
    for image in scene.images.values():
        if image.has_pose:
            pose = image.cam_from_world
            pose.translation[:] = scale * (np.asarray(pose.translation, np.float64) + pose.rotation.matrix() @ c)
    return scale, -scale * c


def normalize_scene(scene):
    """MpsfmReconstruction.normalize (reference reconstruction/base.py:116-121): the similarity, then the depth maps."""
    scale, _ = normalize(scene, False, 5, 0.2, 0.8, False)
    scene.normalize_depths(scale)
    return True
