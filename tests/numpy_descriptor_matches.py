"""fp64 NumPy restatement of the descriptor matcher (mpsfm_match_descriptors / mpsfm_match_map_descriptors,
csrc/descriptor_matches.hip; reference: NearestNeighbor / find_nn / mutual_check and NNs_sparse).

Similarities are accumulated with an explicit loop over k, one rounded product and one rounded sum per step, the same
sequence for every element: identical descriptors tie bitwise.  Nearest neighbour: the maximum, equal values going to the
lowest index; second nearest: the maximum over the remaining columns.

Besides the result every function returns each row's DECISION MARGIN: the smallest of
  top1 - top2                      (which column is the nearest)
  |dist0 - ratio^2 dist1|          (ratio test, when on)
  |dist0 - distance^2|             (distance test, when on)
  |score - score_threshold|        (score threshold, when on)
and, with the mutual check on, of the same quantity of the chosen column in the other direction.  Two evaluations whose
similarities differ by less than e agree on every row whose margin exceeds 4 e: the gap moves by at most 2 e, dist by 2 e,
dist0 - ratio^2 dist1 by at most 4 e for ratio <= 1."""

import numpy as np


def tau(dim, eps):
    """4 dim eps: the margin below which two correct evaluations with unit roundoff eps may disagree (|descriptor| <= 1)."""
    return 4.0 * dim * eps


TAU32_EPS = 2.0 ** -24
TAU64_EPS = 2.0 ** -53


def similarities(d0, d1):
    """[n0, n1] fp64, sum over k ascending of d0[i, k] * d1[j, k]."""
    a, b = np.asarray(d0, np.float64), np.asarray(d1, np.float64)
    sim = np.zeros((a.shape[0], b.shape[0]))
    for k in range(a.shape[1]):
        sim = sim + a[:, k:k + 1] * b[None, :, k]
    return sim


def top2(sim):
    """(v1, i1, v2): lowest index among equal maxima; v2 = -inf with a single column."""
    n = sim.shape[0]
    rows = np.arange(n)
    i1 = sim.argmax(1)
    v1 = sim[rows, i1]
    rest = sim.copy()
    rest[rows, i1] = -np.inf
    v2 = rest.max(1)
    return v1, i1.astype(np.int64), v2


def find_nn(sim, ratio2, dist2):
    """find_nn in fp64: matches, scores, margin and the nearest column of every row.  ratio2 / dist2: squared thresholds or None."""
    v1, i1, v2 = top2(sim)
    d0, d1 = 2.0 * (1.0 - v1), 2.0 * (1.0 - v2)
    ok = np.ones(len(v1), bool)
    margin = v1 - v2
    if ratio2 is not None:
        rhs = ratio2 * d1
        ok &= d0 <= rhs
        margin = np.minimum(margin, np.abs(d0 - rhs))
    if dist2 is not None:
        ok &= d0 <= dist2
        margin = np.minimum(margin, np.abs(d0 - dist2))
    return np.where(ok, i1, -1), np.where(ok, (v1 + 1.0) / 2.0, 0.0), margin, i1


def match_similarities(sim, ratio_threshold=None, distance_threshold=None, do_mutual_check=True, score_threshold=None):
    n0, n1 = sim.shape
    if n0 == 0 or n1 == 0:
        return np.full(n0, -1, np.int64), np.zeros(n0), np.full(n0, np.inf)
    ratio2 = float(ratio_threshold) * float(ratio_threshold) if ratio_threshold and ratio_threshold > 0 and n0 > 1 and n1 > 1 else None
    dist2 = float(distance_threshold) * float(distance_threshold) if distance_threshold and distance_threshold > 0 else None
    m0, s0, margin, i1 = find_nn(sim, ratio2, dist2)
    if do_mutual_check:
        m1, _, margin1, _ = find_nn(sim.T, ratio2, dist2)
        loop = m1[np.where(m0 > -1, m0, 0)]
        m0 = np.where((m0 > -1) & (loop == np.arange(n0)), m0, -1)
        margin = np.minimum(margin, margin1[i1])
    if score_threshold and score_threshold > 0:
        m0 = np.where(s0 < score_threshold, -1, m0)
        margin = np.minimum(margin, np.abs((sim.max(1) + 1.0) / 2.0 - score_threshold))
    return m0.astype(np.int64), s0, margin


def match_descriptors(d0, d1, ratio_threshold=None, distance_threshold=None, do_mutual_check=True, score_threshold=None):
    """d0 [n0, dim], d1 [n1, dim] -> matches0 int64 [n0], scores0 [n0], margin [n0]."""
    d0, d1 = np.asarray(d0, np.float64), np.asarray(d1, np.float64)
    if len(d0) == 0 or len(d1) == 0:
        return np.full(len(d0), -1, np.int64), np.zeros(len(d0)), np.full(len(d0), np.inf)
    return match_similarities(similarities(d0, d1), ratio_threshold, distance_threshold, do_mutual_check, score_threshold)


def sample_map(m, kps):
    """Bilinear samples of m [H, W, C] (or [H, W]) at kps [n, 2] (x, y): align_corners, zero padding, the keypoints rounded to
    float32 first and taken as pixel coordinates, then fp64 with every operation rounded on its own."""
    m = np.asarray(m, np.float64)
    flat = m.ndim == 2
    if flat:
        m = m[:, :, None]
    H, W, C = m.shape
    k = np.asarray(kps, np.float64).reshape(-1, 2).astype(np.float32).astype(np.float64)
    x, y = k[:, 0], k[:, 1]
    x0f, y0f = np.floor(x), np.floor(y)
    wx1, wy1 = x - x0f, y - y0f
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    fin = (x0f > -2.0) & (x0f < W + 1.0) & (y0f > -2.0) & (y0f < H + 1.0)
    x0, y0 = np.where(fin, x0f, 0).astype(np.int64), np.where(fin, y0f, 0).astype(np.int64)
    w = [wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1]
    out = np.zeros((len(k), C))
    for c in range(4):
        xi, yi = x0 + (c & 1), y0 + (c >> 1)
        inside = fin & (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        term = w[c][:, None] * m[np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1)]
        out = np.where(inside[:, None], out + term, out)
    return out[:, 0] if flat else out


def nns_sparse(map0, map1, conf0, conf1, kps0, kps1, scores_thresh=0.85, **kw):
    """NNs_sparse: matches0 int64 [n0], scores0 = sqrt(conf0 conf1) of the matched rows, margin [n0]."""
    d0, d1 = sample_map(map0, kps0), sample_map(map1, kps1)
    c0, c1 = sample_map(conf0, kps0), sample_map(conf1, kps1)
    m0, _, margin = match_descriptors(d0, d1, score_threshold=scores_thresh, **kw)
    scores = np.where(m0 > -1, np.sqrt(c0 * c1[np.where(m0 > -1, m0, 0)]) if len(c1) else 0.0, 0.0)
    return m0, scores, margin
