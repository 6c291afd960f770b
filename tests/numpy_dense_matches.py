"""NumPy restatement of the dense-match thinning (csrc/dense_matches.hip): brute force, fp64, one rounding per operation.

sparse_nms        the reference's greedy radius suppression (mpsfm/extraction/pairwise/models/utils/generic.py) with a
                  defined order: score descending, equal scores by lower index (a stable sort), or the given ``order``.
reference_slice   the reference's expression for "the dense survivors of a pass", written once.
thin_dense_mask   the two passes of match_dense_2view.py:127-161 over one pair.
assign_keypoints  nearest keypoint strictly closer than max_error, lowest index among equidistant ones, else -1.
"""

import numpy as np


def d2_to(points, p):
    """Squared distances of all `points` to `p`: dx*dx + dy*dy in fp64."""
    dx = points[:, 0] - p[0]
    dy = points[:, 1] - p[1]
    return dx * dx + dy * dy


def priority_order(scores):
    s = np.asarray(scores, np.float64) + 0.0  # -0.0 + 0.0 = +0.0
    return np.argsort(-s, kind="stable")


def sparse_nms(points, scores, nms_radius, order=None, alive=None):
    """Sorted kept indices.  `alive` (bool [n], optional): points that take part; the others neither keep nor suppress."""
    points = np.asarray(points, np.float64).reshape(-1, 2)
    n = len(points)
    order = priority_order(scores) if order is None else np.asarray(order, np.int64)
    assert sorted(order.tolist()) == list(range(n))
    r2 = np.float64(nms_radius) * np.float64(nms_radius)
    live = np.ones(n, bool) if alive is None else np.asarray(alive, bool).copy()
    keep = np.zeros(n, bool)
    for i in order:
        if not live[i]:
            continue
        keep[i] = True
        live[d2_to(points, points[i]) <= r2] = False
    return np.flatnonzero(keep)


def reference_slice(kept_sorted, n_sparse):
    """match_dense_2view.py:136-137: sparse_nms(comb, ...)[n_sparse:] - n_sparse."""
    return kept_sorted[n_sparse:] - n_sparse


def dense_survivors(kept_sorted, n_sparse, use_reference_slice):
    if use_reference_slice:
        return reference_slice(kept_sorted, n_sparse)
    return kept_sorted[kept_sorted >= n_sparse] - n_sparse


def thin_dense_mask(dense0, dense1, dscores, sparse0=None, sparse1=None, radius=6.0, use_reference_slice=True, sparse_nms_fn=None):
    """Indices (sorted) of the dense matches that survive both passes, computed as the reference does: on compacted arrays."""
    nms = sparse_nms if sparse_nms_fn is None else sparse_nms_fn
    dense0, dense1 = np.asarray(dense0, np.float64).reshape(-1, 2), np.asarray(dense1, np.float64).reshape(-1, 2)
    dscores = np.asarray(dscores, np.float64)
    sparse0 = np.zeros((0, 2)) if sparse0 is None else np.asarray(sparse0, np.float64).reshape(-1, 2)
    sparse1 = np.zeros((0, 2)) if sparse1 is None else np.asarray(sparse1, np.float64).reshape(-1, 2)
    ns = len(sparse0)
    idx = np.arange(len(dense0))
    for sp, de in ((sparse0, dense0), (sparse1, dense1)):
        comb = np.concatenate([sp, de[idx]])
        sc = np.concatenate([np.ones(ns) * 100, dscores[idx]])
        idx = idx[dense_survivors(nms(comb, sc, radius), ns, use_reference_slice)]
    return idx


def assign_keypoints(kpts, other_cpts, max_error):
    kpts = np.asarray(kpts, np.float64).reshape(-1, 2)
    other = np.asarray(other_cpts, np.float64).reshape(-1, 2)
    out = np.full(len(kpts), -1, np.int64)
    if len(other) == 0:
        return out
    e2 = np.float64(max_error) * np.float64(max_error)
    for lo in range(0, len(kpts), 2048):
        q = kpts[lo:lo + 2048]
        dx = q[:, None, 0] - other[None, :, 0]
        dy = q[:, None, 1] - other[None, :, 1]
        d2 = dx * dx + dy * dy
        j = np.argmin(d2, axis=1)  # the first minimum: the lowest index
        ok = d2[np.arange(len(q)), j] < e2
        out[lo:lo + 2048] = np.where(ok, j, -1)
    return out
