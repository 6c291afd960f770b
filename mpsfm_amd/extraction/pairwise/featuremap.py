"""The sparse leg of a dense-feature matcher with the reference's name and signature (mpsfm/extraction/pairwise/models/
utils/featuremap.py ``NNs_sparse``): descriptor and confidence maps sampled bilinearly at both images' keypoints, mutual
nearest neighbours of the samples, a score threshold, and ``sqrt(conf0 conf1)`` as the match score, in one call into
libmpsfm_hip (csrc/descriptor_matches.hip).  Maps that are device tensors stay on the device."""

from __future__ import annotations

from ... import capi


def NNs_sparse(pts1, pts2, scores1, scores2, kps1, kps2, scores_thresh=0.85, **matcher_kw):
    """pts ``[H, W, C]`` descriptor maps, scores ``[H, W]`` confidence maps, kps ``[n, 2]`` (x, y).  Returns ``matches0``
    int64 ``[n1]`` and ``matching_scores0`` float64 ``[n1]`` as NumPy arrays.  Unlike the reference it is defined for a single
    keypoint.  ``matcher_kw`` is accepted and IGNORED, as in the reference, whose only caller passes ``subsample_or_initxy1``,
    ``ret_xy``, ``dist``, ``block_size`` or ``workers`` there: the matcher is always the mutual nearest neighbour without ratio
    or distance test (``capi.match_map_descriptors`` takes those options).  ``scores_thresh=None`` switches the threshold off."""
    if hasattr(kps1, "detach"):
        kps1 = kps1.detach().cpu().numpy()
    if hasattr(kps2, "detach"):
        kps2 = kps2.detach().cpu().numpy()
    return capi.match_map_descriptors(pts1, scores1, pts2, scores2, kps1, kps2, score_threshold=scores_thresh)
