"""The dense leg of the MASt3R matcher with the reference's names and signatures (mpsfm/extraction/pairwise/models/mast3r.py
``merge_corres``, ``extract_correspondences``, ``map_keypoints_to_original_after_crop``, and MASt3R's ``fast_reciprocal_NNs``
as that file calls it): reciprocal nearest-neighbour descents from a grid of seeds between two descriptor maps, the merge of
the four searches of a pair and the confidence product, in one call into libmpsfm_hip (csrc/reciprocal_matches.hip, DESIGN.md
section 4p).  Maps that are device tensors stay on the device."""

from __future__ import annotations

import numpy as np

from ... import capi

MAX_ITER = 10  # fixed inside fast_reciprocal_NNs


def fast_reciprocal_NNs(pts1, pts2, subsample_or_initxy1=8, ret_xy=True, pixel_tol=0, ret_basin=False, dist="dot", **kw):
    """pts1 ``[H1, W1, C]``, pts2 ``[H2, W2, C]`` descriptor maps.  Returns the converged reciprocal pairs, unique and sorted: int32
    linear indices ``(idx1, idx2)`` with ``ret_xy=False``, else int64 ``[n, 2]`` (x, y) arrays.  Only the form the reference uses is
    built: an int subsample, ``pixel_tol=0``, no basin, dot-product similarity; ``device``, ``block_size`` and ``workers`` are
    accepted and ignored."""
    if not isinstance(subsample_or_initxy1, (int, np.integer)) or isinstance(subsample_or_initxy1, bool):
        raise NotImplementedError("explicit seed arrays are not supported: pass an int subsample")
    if pixel_tol:
        raise NotImplementedError("pixel_tol > 0 is not supported")
    if ret_basin:
        raise NotImplementedError("ret_basin is not supported")
    if dist != "dot":
        raise NotImplementedError(f"dist={dist!r} is not supported: only 'dot'")
    unknown = set(kw) - {"device", "block_size", "workers"}
    if unknown:
        raise TypeError(f"unexpected keyword arguments {sorted(unknown)}")
    idx1, idx2 = capi.reciprocal_nns(pts1, pts2, int(subsample_or_initxy1), MAX_ITER)
    if not ret_xy:
        return idx1, idx2
    W1, W2 = int(pts1.shape[1]), int(pts2.shape[1])
    i1, i2 = idx1.astype(np.int64), idx2.astype(np.int64)
    return np.stack([i1 % W1, i1 // W1], 1), np.stack([i2 % W2, i2 // W2], 1)


def merge_corres(idx1, idx2, shape1=None, shape2=None, ret_xy=True, ret_index=False):
    """Rows unique by (idx1 major, idx2 minor) ascending; with ``ret_index`` also the index of every kept row's first occurrence.
    ``ret_xy``: int64 ``[n, 2]`` (x, y) arrays (``"y_x"``: the (y, x) tuples of ``np.unravel_index``), else the int32 indices."""
    idx1, idx2 = np.asarray(idx1), np.asarray(idx2)
    assert idx1.dtype == idx2.dtype == np.int32
    key, indices = np.unique(idx1.astype(np.int64) << 32 | idx2.astype(np.int64), return_index=True)
    xy1, xy2 = (key >> 32).astype(np.int32), (key & 0xFFFFFFFF).astype(np.int32)
    if ret_xy:
        assert shape1 and shape2
        xy1, xy2 = np.unravel_index(xy1, shape1), np.unravel_index(xy2, shape2)
        if ret_xy != "y_x":
            xy1, xy2 = np.stack(xy1[::-1], 1).astype(np.int64), np.stack(xy2[::-1], 1).astype(np.int64)
    return (xy1, xy2, indices) if ret_index else (xy1, xy2)


def extract_correspondences(feats, qonfs, subsample=8, ptmap_key="pred_desc"):
    """feats ``(feat11, feat21, feat22, feat12)`` descriptor maps, qonfs their confidence maps in the same order.  Returns ``xy1``,
    ``xy2`` int64 ``[n, 2]`` (x, y) and the float32 scores ``sqrt(qonf1 qonf2)`` of every pair's first occurrence."""
    if "3d" in ptmap_key:
        raise NotImplementedError("the pts3d variant (nearest neighbours by distance) is not supported")
    return capi.dense_correspondences(feats, qonfs, subsample, MAX_ITER)


def map_keypoints_to_original_after_crop(keypoints_crop, cx, cy, halfw, halfh):
    return keypoints_crop + np.array([cx - halfw, cy - halfh])
