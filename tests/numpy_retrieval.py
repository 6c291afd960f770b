"""fp64 NumPy restatement of retrieval (mpsfm_retrieve_topk, csrc/retrieval.hip; reference: pairs_from_retrieval.py: einsum,
masked_fill, torch.topk).

Similarities come from numpy_descriptor_matches.similarities: an explicit loop over k, one rounded product and one rounded sum per
step, the same sequence for every element, so identical descriptors tie bitwise.  Candidates of a row: every column but those with
query_ids[i] == db_ids[j] and, with the score test on, those with sim < min_score.  Result: the first k candidates under
np.lexsort((index, -value)): value descending, index ascending.

Besides lists and counts every function returns each row's DECISION MARGIN, the smallest of
  the gaps between consecutive values among the first min(k + 1, n_valid) sorted candidates   (who is listed, and in which order)
  |sim - min_score|, with the score test on: over those same values when n_valid >= k + 1, and over all columns the identity test
  leaves otherwise, because there the score test alone decides membership.
Two correct evaluations whose similarities differ by less than e agree on every row whose margin exceeds 4 e (the rule of
numpy_descriptor_matches.py: a gap moves by at most 2 e)."""

import numpy as np

from numpy_descriptor_matches import TAU32_EPS, TAU64_EPS, similarities, tau  # noqa: F401 - the tests read them from here


def topk_similarities(sim, k, min_score=0.0, query_ids=None, db_ids=None):
    """sim [nq, nd] -> indices int64 [nq, k] (-1 beyond the count), scores [nq, k] (0 beyond it), counts int64 [nq], margin [nq]."""
    sim = np.asarray(sim, np.float64)
    nq, nd = sim.shape
    indices, scores = np.full((nq, k), -1, np.int64), np.zeros((nq, k))
    counts, margin = np.zeros(nq, np.int64), np.full(nq, np.inf)
    cols = np.arange(nd)
    for i in range(nq):
        allowed = np.ones(nd, bool) if query_ids is None else np.asarray(db_ids) != np.asarray(query_ids)[i]
        valid = allowed if min_score is None else allowed & ~(sim[i] < min_score)
        c, v = cols[valid], sim[i][valid]
        order = np.lexsort((c, -v))
        c, v = c[order], v[order]
        n = min(k, len(c))
        indices[i, :n], scores[i, :n], counts[i] = c[:n], v[:n], n
        head = v[:min(k + 1, len(v))]
        if len(head) > 1:
            margin[i] = np.min(head[:-1] - head[1:])
        if min_score is not None:
            near = head if len(v) >= k + 1 else sim[i][allowed]
            if len(near):
                margin[i] = min(margin[i], np.min(np.abs(near - min_score)))
    return indices, scores, counts, margin


def retrieve_topk(query, db, k, min_score=0.0, query_ids=None, db_ids=None):
    """query [nq, D], db [nd, D] -> indices, scores, counts, margin as topk_similarities."""
    q, d = np.asarray(query, np.float64), np.asarray(db, np.float64)
    if len(q) == 0 or len(d) == 0:
        return np.full((len(q), k), -1, np.int64), np.zeros((len(q), k)), np.zeros(len(q), np.int64), np.full(len(q), np.inf)
    return topk_similarities(similarities(q, d), k, min_score, query_ids, db_ids)


def pairs_of(indices, counts):
    """[(i, j)] in row-major order of the valid entries."""
    return [(i, int(j)) for i in range(len(counts)) for j in indices[i, :counts[i]]]


def name_ids(query_names, db_names):
    ids = {}
    q = np.array([ids.setdefault(n, len(ids)) for n in query_names], np.int32)
    return q, np.array([ids.setdefault(n, len(ids)) for n in db_names], np.int32)
