"""The neighbour geometry between a dense matcher's raw output and the match lists two-view verification consumes, with the
reference's names and signatures (mpsfm/extraction/pairwise/models/utils/generic.py ``sparse_nms``, .../warp.py
``assign_keypoints``, and the ``dense`` leg of match_dense_2view.py:127-161 as ``thin_dense_matches``).

The reference does these with a SciPy KD-tree on the host; here each is one call into libmpsfm_hip (csrc/dense_matches.hip).
Inputs may be NumPy arrays or torch tensors of float32 or float64; the arithmetic is fp64 whatever comes in, as the
KD-tree's is, and the radius decisions (``<=`` for the suppression, ``<`` for the assignment) are exact.

Ties.  The reference orders the points with ``torch.argsort(scores, descending=True)``, which is not a stable sort: the
order among equal scores (the matched sparse keypoints all carry 100) is an accident of the torch build.  Here equal scores
go in index order, lower index first; pass ``order=`` (a permutation, highest priority first) to impose another.
"""

from __future__ import annotations

import numpy as np

from ... import capi


def _np(a):
    if a is None:
        return None
    if hasattr(a, "detach"):  # torch tensor
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def sparse_nms(points, scores, nms_radius: float, order=None):
    """Greedy radius suppression: the points are visited by descending score and a visited point that is still alive
    suppresses every point within ``nms_radius`` (inclusive).  Returns the kept indices, sorted, as the reference does."""
    points, scores = _np(points), _np(scores)
    assert points.shape[0] == scores.shape[0]
    if points.shape[0] == 0:
        return np.zeros(0, np.int64)
    keep = capi.radius_nms(points, scores, nms_radius, order=_np(order))
    return np.flatnonzero(keep).astype(np.int64)


def assign_keypoints(kpts, other_cpts, max_error):
    """For every row of ``kpts`` the index of the nearest row of ``other_cpts`` strictly closer than ``max_error``, else -1."""
    kpts, other_cpts = _np(kpts), _np(other_cpts)
    if len(other_cpts) == 0 or len(kpts) == 0:
        return np.full(len(kpts), -1)
    return capi.assign_keypoints_ids(kpts, other_cpts, max_error)


def thin_dense_matches(dkpts0, dkpts1, dscores, skpts0_matched=None, skpts1_matched=None, nms_radius=6, reference_slice=True):
    """The ``dense`` leg of match_dense: suppression over image 0, then over the survivors in image 1; with matched sparse
    keypoints given (``sparse+dense``) they are prepended with score 100 in both passes, so dense matches only fill the
    regions the sparse ones leave.  Returns ``(dkpts0, dkpts1, dscores)`` thinned, as NumPy arrays: what the reference writes
    to HDF5.

    ``reference_slice``.  The reference selects a pass's survivors as ``sparse_nms(comb, ...)[n_sparse:] - n_sparse``,
    which presumes every sparse point survives.  When matched sparse keypoints lie within the radius of each other only
    ``k < n_sparse`` do, and the expression then also drops the first ``n_sparse - k`` surviving dense matches.  True
    (default) reproduces the reference; False keeps every surviving dense match."""
    dkpts0, dkpts1, dscores = _np(dkpts0), _np(dkpts1), _np(dscores)
    if (skpts0_matched is None) != (skpts1_matched is None):
        raise ValueError("give both skpts0_matched and skpts1_matched or neither")
    if len(dkpts0) == 0:
        return dkpts0, dkpts1, dscores
    keep = capi.thin_dense_matches_mask(dkpts0, dkpts1, dscores, _np(skpts0_matched), _np(skpts1_matched), radius=nms_radius,
                                        reference_slice=reference_slice)
    return dkpts0[keep], dkpts1[keep], dscores[keep]
