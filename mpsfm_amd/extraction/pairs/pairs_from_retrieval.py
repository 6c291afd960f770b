"""Pairs by retrieval (reference: mpsfm/extraction/pairs/hloc/pairs_from_retrieval.py, adapted from hloc): for every query image
the `num_matched` db images whose global descriptors are most similar.  The similarities and the selection run in ONE call into
libmpsfm_hip (mpsfm_retrieve_topk, csrc/retrieval.hip): no Nq x Nd matrix, fp64 decisions, equal
similarities to the lowest index.  A feature "file" is a mapping name -> {"global_descriptor": [D]}.

The reference's quirk, kept: the list length is min(num_matched, number of QUERY images), not of db images."""

from __future__ import annotations

from collections.abc import Iterable, Mapping
from pathlib import Path

import numpy as np

from ... import capi
from ...utils.parsers import parse_image_lists
from .base import write_pairs


def parse_names(prefix, names, names_all):
    """The names a side works on: those of `names_all` that start with `prefix` (a string or several), else `names` (a list file or
    an iterable), else all of them."""
    if prefix is not None:
        prefix = prefix if isinstance(prefix, str) else tuple(prefix)
        names = [n for n in names_all if n.startswith(prefix)]
        if not names:
            raise ValueError(f"Could not find any image with the prefix `{prefix}`.")
        return names
    if names is None:
        return names_all
    if isinstance(names, (str, Path)):
        return parse_image_lists(names)
    if isinstance(names, Iterable):
        return list(names)
    raise ValueError(f"Unknown type of image list: {names}. Provide either a list or a path to a list file.")


def _select_length(num_select, n_query, n_db):
    """min(num_select, number of query rows), as the reference clips it, and the two cases it cannot serve."""
    k = min(int(num_select), int(n_query))
    if n_query > 0 and k > n_db:
        raise ValueError(f"{k} = min(num_matched, number of query images) exceeds the {n_db} db images: the reference clips the "
                         "list length by the number of QUERY images, and torch.topk raises there")
    if k > capi.MAX_NUM_SELECT:
        raise ValueError(f"num_matched {k} (after clipping to the number of query images) exceeds the cap of {capi.MAX_NUM_SELECT}")
    return k


def pairs_from_descriptors(query_desc, db_desc, num_select, min_score=0, query_ids=None, db_ids=None):
    """[(i, j)] in row-major order of the valid entries, query ascending, then rank: what the reference's
    `pairs_from_score_matrix(einsum(query, db), ids equal, num_select, min_score)` lists, on the device.  Descriptors [n, D], float16
    / float32; NumPy, host tensors or device tensors."""
    k = _select_length(num_select, query_desc.shape[0], db_desc.shape[0])
    if k < 1:
        return []
    indices, _, counts = capi.retrieve_topk(query_desc, db_desc, k, min_score, query_ids, db_ids)
    return [(i, int(j)) for i in range(len(counts)) for j in indices[i, :counts[i]]]


def pairs_from_score_matrix(scores, invalid, num_select, min_score=None):
    """The reference's selection from a given score matrix, on the host in NumPy: per row the first min(num_select, rows) entries
    that are neither `invalid` nor below `min_score`, under (score descending, index ascending).  Returns [(i, j)], row-major.
    Unlike the reference, which fills `scores` in place, the arguments are left as they are."""
    if type(scores).__module__.startswith("torch"):
        scores = scores.detach().cpu().numpy()
    scores, invalid = np.asarray(scores), np.asarray(invalid, bool)
    assert scores.shape == invalid.shape
    k = min(int(num_select), scores.shape[0])
    if scores.shape[0] > 0 and k > scores.shape[1]:
        raise ValueError(f"{k} = min(num_select, rows) exceeds the {scores.shape[1]} columns: torch.topk raises in the reference")
    out = invalid.copy()
    if min_score is not None:
        out |= scores < min_score
    pairs = []
    cols = np.arange(scores.shape[1])
    for i in range(scores.shape[0]):
        keep = ~out[i] & np.isfinite(scores[i])
        order = np.lexsort((cols[keep], -scores[i][keep].astype(np.float64)))[:k]
        pairs += [(i, int(j)) for j in cols[keep][order]]
    return pairs


def _named(features):
    """name -> (mapping that holds it); where a name appears in several mappings the last one wins"""
    if isinstance(features, Mapping):
        features = [features]
    return {name: f for f in features for name in f.keys()}


def _stack(names, where):
    return np.stack([np.asarray(_host(where[n][n]["global_descriptor"])) for n in names], 0)


def _host(x):
    return x.detach().cpu().numpy() if type(x).__module__.startswith("torch") else x


def main(descriptors, output, num_matched, query_prefix=None, query_list=None, db_prefix=None, db_list=None, db_descriptors=None, verbose=0):
    """The reference's `main` on mappings: `descriptors` name -> {"global_descriptor": [D]} holds the query images, `db_descriptors`
    (one mapping or a list of them; default: `descriptors`) the db images.  An image never pairs with its own name.  Returns
    [(query_name, db_name)] and writes it to `output` unless that is None."""
    name2db = _named(descriptors if db_descriptors is None else db_descriptors)
    db_names = parse_names(db_prefix, db_list, list(name2db.keys()))
    if len(db_names) == 0:
        raise ValueError("Could not find any database image.")
    query_names = parse_names(query_prefix, query_list, list(descriptors.keys()))
    db_desc = _stack(db_names, name2db)
    query_desc = _stack(query_names, {n: descriptors for n in query_names})
    ids = {}  # identity ids from names
    query_ids = np.array([ids.setdefault(n, len(ids)) for n in query_names], np.int32)
    db_ids = np.array([ids.setdefault(n, len(ids)) for n in db_names], np.int32)
    pairs = pairs_from_descriptors(query_desc, db_desc, num_matched, 0, query_ids, db_ids)
    pairs = [(query_names[i], db_names[j]) for i, j in pairs]
    if verbose > 0:
        print(f"Found {len(pairs)} pairs.")
    write_pairs(output, pairs)
    return pairs
