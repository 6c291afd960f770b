"""NumPy restatement of the warp-to-matches contracts (csrc/warp_matches.hip), independent of the device
code and of torch.

simple_nms            the reference's models/utils/warp.py simple_nms: a sliding maximum with -inf padding, comparisons on
                      the float32 values themselves.
unique_rows           get_unique_matches with a defined winner: per group the highest score, equal scores (-0.0 as +0.0) to
                      the lowest row, by a stable lexsort.
kpids_to_matches0     the rows to matches0 / scores0 of the reference's length (1 + the largest matched id0).
to_pixel_coordinates  W / 2 * (x + 1) in np.float32, step by step.
warp_to_matches       both legs of Roma._forward after the network; the lookup is numpy_dense_matches.assign_keypoints.
"""

import numpy as np

import numpy_dense_matches as ND


def max_pool(x, r):
    """out[i, j] = max of x over |di| <= r, |dj| <= r inside the map (outside counts as -inf)"""
    H, W = x.shape
    p = np.full((H + 2 * r, W + 2 * r), -np.inf, np.float32)
    p[r:r + H, r:r + W] = x
    rows = p[:, 0:W].copy()
    for d in range(1, 2 * r + 1):
        rows = np.maximum(rows, p[:, d:d + W])
    out = rows[0:H].copy()
    for d in range(1, 2 * r + 1):
        out = np.maximum(out, rows[d:d + H])
    return out


def simple_nms(scores, r):
    s = np.asarray(scores, np.float32)
    assert s.ndim == 2 and r >= 0
    zeros = np.zeros_like(s)
    mask = s == max_pool(s, r)
    for _ in range(2):
        supp = max_pool(mask.astype(np.float32), r) > 0
        ss = np.where(supp, zeros, s)
        mask = mask | ((ss == max_pool(ss, r)) & ~supp)
    return np.where(mask, s, zeros)


def group_winners(ids, scores, rows):
    """of the given rows, per value of ids[rows] the one with the highest score, the lowest row among equal scores"""
    s = scores[rows].astype(np.float64) + 0.0  # -0.0 + 0.0 = +0.0
    order = np.lexsort((rows, -s, ids[rows]))  # by id, then score descending, then row ascending
    srt = rows[order]
    first = np.ones(len(srt), bool)
    first[1:] = ids[srt][1:] != ids[srt][:-1]
    return srt[first]


def unique_rows(ids0, ids1, scores):
    ids0, ids1, scores = np.asarray(ids0, np.int64), np.asarray(ids1, np.int64), np.asarray(scores, np.float32)
    valid = np.flatnonzero((ids0 >= 0) & (ids1 >= 0))
    if len(valid) == 0:
        return valid
    return np.intersect1d(group_winners(ids0, scores, valid), group_winners(ids1, scores, valid))


def kpids_to_matches0(ids0, ids1, scores):
    """matches0 int32, scores0 float32 (the wrapper's float16 is a cast of it), kept rows"""
    ids0, ids1, scores = np.asarray(ids0, np.int64), np.asarray(ids1, np.int64), np.asarray(scores, np.float32)
    keep = unique_rows(ids0, ids1, scores)
    if len(keep) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.float32), keep
    n = int(ids0[keep].max()) + 1
    m, s = np.full(n, -1, np.int32), np.zeros(n, np.float32)
    m[ids0[keep]] = ids1[keep]
    s[ids0[keep]] = scores[keep]
    return m, s, keep


def to_pixel_coordinates(warp, H_A, W_A, H_B, W_B):
    w = np.asarray(warp, np.float32).reshape(-1, 4)
    one = np.float32(1.0)
    out = []
    for half_w, half_h, c in ((np.float32(W_A / 2), np.float32(H_A / 2), 0), (np.float32(W_B / 2), np.float32(H_B / 2), 2)):
        t0 = (w[:, c] + one).astype(np.float32)
        t1 = (w[:, c + 1] + one).astype(np.float32)
        out.append(np.stack([(half_w * t0).astype(np.float32), (half_h * t1).astype(np.float32)], 1))
    return out


def warp_to_matches(warp, certainty, sizes, dense=True, sparse=True, skpts0=None, skpts1=None, scale0=(1, 1), scale1=(1, 1), nms_radius=8,
                    sample_thresh=0.1, max_error=2):
    c = np.asarray(certainty, np.float32)
    k0, k1 = to_pixel_coordinates(warp, *sizes)
    out = {}
    if dense:
        nms = simple_nms(c, nms_radius).reshape(-1)
        sel = nms > np.float32(sample_thresh)
        out.update(dkeypoints0=k0[sel], dkeypoints1=k1[sel], dscores=nms[sel])
    if sparse:
        s0, s1 = np.asarray(skpts0, np.float64).reshape(-1, 2), np.asarray(skpts1, np.float64).reshape(-1, 2)
        if len(s0) == 0 or len(s1) == 0:
            out.update(smatches0=np.zeros(0, np.int32), smatching_scores0=np.zeros(0, np.float32))
        else:
            ids0 = ND.assign_keypoints(k0.astype(np.float64) * np.asarray(scale0, np.float64), s0, max_error)
            ids1 = ND.assign_keypoints(k1.astype(np.float64) * np.asarray(scale1, np.float64), s1, max_error)
            m, s, _ = kpids_to_matches0(ids0, ids1, c.reshape(-1))
            out.update(smatches0=m, smatching_scores0=s, ids0=ids0, ids1=ids1)
    return out
