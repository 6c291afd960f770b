"""Geometric verification of image pairs over libmpsfm_hip.

Mirror of reference ``mpsfm/sfm/scene/correspondences/utils.py`` (``process_pair`` :13-32, ``geometric_verification``
:51-77) with the reference's signatures and options (max_num_trials 20000, min_inlier_ratio 0.1, compute_relative_pose).
By default each pair is one stateless call of ``mpsfm_two_view_geometry`` in a plain loop over the pairs in this process;
``batched=True`` gathers all pairs and makes one call of ``mpsfm_two_view_geometry_batch`` in place of the reference's process
pool, with the same result for every pair.
``Correspondences.populate``, the HDF5 gathering and the correspondence graph stay with the reference.
"""

from __future__ import annotations

import numpy as np

from ..estimators.two_view_geometry import estimate_calibrated_two_view_geometry, estimate_calibrated_two_view_geometry_batch


def pair_options(max_error) -> dict:
    """The options the reference passes for every pair."""
    return {
        "ransac": {"max_num_trials": 20000, "min_inlier_ratio": 0.1, "max_error": max_error},
        "compute_relative_pose": True,
    }


def process_pair(data, max_error, backend=None):
    """Estimates the two-view geometry of one gathered pair: (tvg, matches, name0, name1)."""
    tvg = estimate_calibrated_two_view_geometry(
        data["cam0"], data["kps0"], data["cam1"], data["kps1"], data["matches"], pair_options(max_error), backend=backend
    )
    return (tvg, data["matches"], data["name0"], data["name1"])


def gather_data(name0, name1, rec_name_to_id, reference, keypoints_cache, matches_cache):
    """The cameras, keypoints and matches of one pair."""
    out = {"name0": name0, "name1": name1}
    for k, name in (("0", name0), ("1", name1)):
        image = reference.images[rec_name_to_id[name]]
        cam = reference.cameras[image.camera_id]
        out["cam" + k] = cam.as_colmap() if hasattr(cam, "as_colmap") else cam
        out["kps" + k] = keypoints_cache[name]
    out["matches"] = matches_cache[name0, name1]
    return out


def geometric_verification(reference, pairs, max_error: float = 4.0, keypoints=None, matches=None, backend=None, batched: bool = False):
    """Geometric verification of `pairs` [(name0, name1)]: (inlier_masks, tvg_cache), both keyed (name0, name1).  `batched`: all
    pairs in one call of the batched estimator instead of one call per pair; the results are the same."""
    tvg_cache = {}
    inlier_masks = {}
    rec_name_to_id = {im.name: im.image_id for im in reference.images.values()}
    gathered = (gather_data(name0, name1, rec_name_to_id, reference, keypoints, matches) for name0, name1 in pairs)
    if batched:
        gathered = list(gathered)
        tvgs = estimate_calibrated_two_view_geometry_batch(
            [(d["cam0"], d["kps0"], d["cam1"], d["kps1"], d["matches"]) for d in gathered], pair_options(max_error), backend=backend
        )
        done = ((tvg, d["matches"], d["name0"], d["name1"]) for tvg, d in zip(tvgs, gathered))
    else:
        done = (process_pair(data, max_error, backend=backend) for data in gathered)
    for tvg, matches_, name0, name1 in done:
        tvg_cache[name0, name1] = tvg
        # the reference's expression: a match row is an inlier when an equal row is among the inlier matches, so every copy of
        # a duplicated row shares one answer
        mask = np.isin(
            matches_.view([("", matches_.dtype)] * 2), tvg.inlier_matches.view([("", tvg.inlier_matches.dtype)] * 2)
        )
        inlier_masks[(name0, name1)] = mask[:, 0]
    return inlier_masks, tvg_cache
