"""The in-memory half of the reference's sparse matching stage (mpsfm/extraction/pairwise/match_sparse.py, adapted from hloc):
which pairs to match, and the match lists of all of them from ONE call into libmpsfm_hip (mpsfm_match_descriptors_batch,
csrc/descriptor_matches_batch.hip) instead of one call per pair.  Reading features from and writing matches to
HDF5 stays with the reference.
"""

from __future__ import annotations

import numpy as np

from ... import capi
from .nearest_neighbor import NearestNeighbor, _is_float64, _is_torch


def names_to_pair(name0, name1, separator="/"):
    """The key of a pair in a match file: '/' inside a name becomes '-'."""
    return separator.join((name0.replace("/", "-"), name1.replace("/", "-")))


def names_to_pair_old(name0, name1):
    return names_to_pair(name0, name1, separator="_")


def find_unique_new_pairs(pairs_all, existing=None):
    """The pairs still to be matched: (i, j) is dropped when (j, i) was already taken (and a repeated (i, j) is taken once), and
    when `existing` holds the pair under any of its four keys (`names_to_pair` / `names_to_pair_old`, either order).  `existing` is
    anything that answers `in` for such keys: an open HDF5 match file, a set, a dict.

    The result is in order of first appearance.  The reference returns `list(set)`, whose order is arbitrary and changes from run
    to run with string hashing; the set of pairs is the same."""
    taken, pairs = set(), []
    for i, j in pairs_all:
        if (j, i) not in taken and (i, j) not in taken:
            taken.add((i, j))
            pairs.append((i, j))
    if existing is None:
        return pairs
    return [(i, j) for i, j in pairs
            if not (names_to_pair(i, j) in existing or names_to_pair(j, i) in existing or names_to_pair_old(i, j) in existing
                    or names_to_pair_old(j, i) in existing)]


def _n_by_dim(d):
    """[D, N] as the feature files store it -> [N, D] (a view)."""
    if getattr(d, "ndim", None) != 2:
        raise ValueError("descriptors must be [D, N]")
    if _is_float64(d):
        raise TypeError("float64 descriptors are not supported: float16 and float32 are widened exactly")
    return d.transpose(0, 1) if _is_torch(d) else d.T


def match_pairs(conf, pairs, features_q, features_ref=None, batched=True):
    """What the loop of `match_from_paths` computes, for all pairs at once.  `pairs`: (name0, name1) tuples, name0 looked up in
    `features_q` and name1 in `features_ref` (default: `features_q`); both map an image name to {"descriptors": [D, N]} (float16 /
    float32; NumPy, host tensors or device tensors).  `conf`: the keys of `NearestNeighbor.default_conf`.

    Returns {names_to_pair(name0, name1): {"matches0": int64 [1, N0], "matching_scores0": float64 [1, N0]}}, each entry what
    `NearestNeighbor(conf)` returns for that pair: torch tensors on the descriptors' device for torch input, NumPy otherwise.
    `batched=False` is that loop itself, one call per pair; the results are equal.  The same name in `features_q` and in a
    different `features_ref` is two images."""
    conf = {**NearestNeighbor.default_conf, **dict(conf or {})}
    pairs = [(a, b) for a, b in pairs]
    same = features_ref is None or features_ref is features_q
    if same:
        features_ref = features_q
    if not batched:
        nn = NearestNeighbor(conf)
        out = {}
        for a, b in pairs:
            d0, d1 = features_q[a]["descriptors"], features_ref[b]["descriptors"]
            _n_by_dim(d0), _n_by_dim(d1)
            out[names_to_pair(a, b)] = nn({"descriptors0": d0[None], "descriptors1": d1[None]})
        return out
    index, descs, idx_pairs = {}, [], []  # (side, name) -> image number; side 0 serves both sides when there is one feature set

    def image(side, features, name):
        key = (0 if same else side, name)
        if key not in index:
            index[key] = len(descs)
            descs.append(_n_by_dim(features[name]["descriptors"]))
        return index[key]

    for a, b in pairs:
        idx_pairs.append((image(0, features_q, a), image(1, features_ref, b)))
    if not pairs:
        return {}
    matches, scores = capi.match_descriptors_batch(descs, idx_pairs, conf["ratio_threshold"], conf["distance_threshold"], conf["do_mutual_check"])
    out = {}
    for (a, b), (i, _), m, s in zip(pairs, idx_pairs, matches, scores):
        m, s = m[None], s[None]
        if _is_torch(descs[i]):
            import torch

            m, s = torch.from_numpy(np.ascontiguousarray(m)).to(descs[i].device), torch.from_numpy(np.ascontiguousarray(s)).to(descs[i].device)
        out[names_to_pair(a, b)] = {"matches0": m, "matching_scores0": s}
    return out
