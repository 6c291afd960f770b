"""fp64 NumPy restatement of the dense reciprocal matcher (mpsfm_reciprocal_nns / mpsfm_dense_correspondences,
csrc/reciprocal_matches.hip; reference: mast3r.py merge_corres / extract_correspondences with MASt3R's
fast_reciprocal_NNs, whose descent rule is inferred and frozen here).

Nearest neighbours use the similarities of tests/numpy_descriptor_matches.py (k ascending, one operation sequence for every
element) and give equal similarities to the lowest index.  For every query the GAP between the best and the second-best
similarity is kept: a seed is DECIDED when every query on its trajectory has a gap above tau64 = 4 C 2^-53 (|value| <= 1); two
correct fp64 evaluations agree on every decided seed.

The module also builds the inputs the tests share, from integer hashes and correctly rounded IEEE operations only (no libm, no
library random stream), so that every machine builds the same bits: `scene_maps` (the fixture's maps, whose digests the fixture
stores), `random_maps` and `planted` cases."""

import hashlib

import numpy as np

import numpy_descriptor_matches as NM


def tau64(C):
    return NM.tau(C, NM.TAU64_EPS)


def tau32(C):
    return NM.tau(C, NM.TAU32_EPS)


def seed_pixels(H, W, S):
    ys, xs = np.arange(S // 2, H, S), np.arange(S // 2, W, S)
    return (ys[:, None] * W + xs[None, :]).ravel().astype(np.int32)


def nearest(Q, M, block=1 << 19):
    """(index, gap) of the rows of Q [n, C] among the rows of M [m, C]: fp64 similarities summed with k ascending, the lowest index
    among equal maxima, gap = best - second best (inf with a single row of M).  M is walked in blocks of columns that stay in
    cache; channels in which every query is zero are skipped, which leaves every sum as it is (x + 0 * y == x for finite y)."""
    n, m = len(Q), len(M)
    bv, bi, sv = np.full(n, -np.inf), np.zeros(n, np.int64), np.full(n, -np.inf)
    ks = np.flatnonzero((Q != 0).any(0))
    step = max(1, block // max(n, 1))
    for c0 in range(0, m, step):
        Mb = M[c0:c0 + step]
        sim = np.zeros((n, len(Mb)))
        for k in ks:
            sim = sim + Q[:, k:k + 1] * Mb[None, :, k]
        v1, i1, v2 = NM.top2(sim)
        better = v1 > bv  # an equal maximum in a later block loses to the earlier, lower index
        sv = np.where(better, np.maximum(bv, v2), np.maximum(sv, v1))
        bi = np.where(better, i1 + c0, bi)
        bv = np.where(better, v1, bv)
    return bi, bv - sv


def fast_reciprocal_nns(A, B, subsample=8, max_iter=10):
    """One search.  Returns dict(idx1, idx2: the converged pairs, unique and sorted by (idx1, idx2), int32; seeds_xy1, seeds_xy2,
    converged: per seed; gap: per seed, the smallest gap of its trajectory; n_seeds, n_converged, iterations, nn_queries;
    iters_of_seed: iterations in which the seed was active)."""
    A, B = np.asarray(A), np.asarray(B)
    (H1, W1, C), (H2, W2, C2) = A.shape, B.shape
    assert C == C2
    fa, fb = A.reshape(-1, C).astype(np.float64), B.reshape(-1, C).astype(np.float64)
    xy1 = seed_pixels(H1, W1, subsample).astype(np.int64)
    n = len(xy1)
    xy2 = np.full(n, -1, np.int64)
    old1, old2 = xy1.copy(), xy2.copy()
    active = np.ones(n, bool)
    gap, its = np.full(n, np.inf), np.zeros(n, np.int64)
    iterations = queries = 0
    while active.any():
        its[active] += 1
        a = np.flatnonzero(active)
        xy2[a], g = nearest(fa[xy1[a]], fb)
        gap[a] = np.minimum(gap[a], g)
        queries += len(a)
        active[a] = xy2[a] != old2[a]
        a = np.flatnonzero(active)
        xy1[a], g = nearest(fb[xy2[a]], fa)
        gap[a] = np.minimum(gap[a], g)
        queries += len(a)
        active[a] = xy1[a] != old1[a]
        iterations += 1
        if iterations >= max_iter:
            break
        old1, old2 = xy1.copy(), xy2.copy()
    conv = ~active
    pairs = np.unique(np.stack([xy1[conv], xy2[conv]], 1), axis=0) if conv.any() else np.zeros((0, 2), np.int64)
    return dict(idx1=pairs[:, 0].astype(np.int32), idx2=pairs[:, 1].astype(np.int32), seeds_xy1=xy1, seeds_xy2=xy2, converged=conv, gap=gap,
                n_seeds=n, n_converged=int(conv.sum()), iterations=iterations, nn_queries=queries, iters_of_seed=its)


def merge_corres(idx1, idx2, shape1, shape2):
    """Unique (idx1 major, idx2 minor) ascending; (xy1 [n, 2] int64 x, y; xy2; index of the first occurrence of every kept row)."""
    idx1, idx2 = np.asarray(idx1, np.int64), np.asarray(idx2, np.int64)
    key = idx1 * (1 << 32) + idx2
    key, first = np.unique(key, return_index=True)
    i1, i2 = key >> 32, key & 0xFFFFFFFF
    xy1 = np.stack([i1 % shape1[1], i1 // shape1[1]], 1)
    xy2 = np.stack([i2 % shape2[1], i2 // shape2[1]], 1)
    return xy1, xy2, first


def extract_correspondences(feats, qonfs, subsample=8, max_iter=10, return_runs=False):
    """extract_correspondences: xy1, xy2 int64 [n, 2], scores float32 [n][, the four searches' dicts]."""
    feat11, feat21, feat22, feat12 = [np.asarray(f) for f in feats]
    qonf11, qonf21, qonf22, qonf12 = [np.asarray(q, np.float32) for q in qonfs]
    idx1, idx2, q1, q2, runs = [], [], [], [], []
    for A, B, QA, QB in ((feat11, feat21, qonf11, qonf21), (feat12, feat22, qonf12, qonf22)):
        f = fast_reciprocal_nns(A, B, subsample, max_iter)
        b = fast_reciprocal_nns(B, A, subsample, max_iter)
        runs += [f, b]
        idx1.append(np.r_[f["idx1"], b["idx2"]])
        idx2.append(np.r_[f["idx2"], b["idx1"]])
        q1.append(QA.ravel()[idx1[-1]])
        q2.append(QB.ravel()[idx2[-1]])
    xy1, xy2, first = merge_corres(np.concatenate(idx1), np.concatenate(idx2), feat11.shape[:2], feat22.shape[:2])
    scores = np.sqrt(np.concatenate(q1)[first] * np.concatenate(q2)[first])
    assert scores.dtype == np.float32
    return (xy1, xy2, scores, runs) if return_runs else (xy1, xy2, scores)


# ---- inputs that every machine builds bitwise alike ------------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def hash_u64(seed, idx):
    """splitmix64 of (seed, idx): uint64, the shape of idx."""
    z = np.asarray(idx).astype(np.uint64) + np.uint64((int(seed) * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & _M64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def random_maps(seed, H, W, C):
    """[H, W, C] float32, uniform multiples of 2^-23 in [-1, 1)."""
    h = hash_u64(seed, np.arange(H * W * C).reshape(H, W, C))
    return ((h >> np.uint64(40)).astype(np.int64) - (1 << 23)).astype(np.float32) / np.float32(1 << 23)


def _grid_field(seed, qx, qy, C, cell, lo, hi):
    """Bilinear interpolation (integer weights, exact) at the quarter-pixel positions qx, qy [H, W] of a grid of hashed integers in
    [lo, hi] with `cell` quarter pixels between nodes: int64 [H, W, C], in units of 1 / cell^2."""
    gx, gy = qx // cell, qy // cell
    fx, fy = (qx - gx * cell)[..., None], (qy - gy * cell)[..., None]

    def node(ix, iy):
        k = ((iy[..., None] + 4096) * 8192 + (ix[..., None] + 4096)) * 1024 + np.arange(C)
        return (hash_u64(seed, k) % np.uint64(hi - lo + 1)).astype(np.int64) + lo

    return ((cell - fx) * (cell - fy) * node(gx, gy) + fx * (cell - fy) * node(gx + 1, gy) + (cell - fx) * fy * node(gx, gy + 1)
            + fx * fy * node(gx + 1, gy + 1))


def scene_maps(seed, H, W, C, shift_q=(0, 0), noise=6, noise_seed=0, cell=24):
    """One view of a scene: (map [H, W, C] float32 with rows of norm < 1, confidence [H, W] float32 in [0.3, 0.9]).  Pixel (x, y)
    sees the scene point (x, y) + shift_q / 4.  The field is piecewise bilinear between hashed integer nodes `cell` / 4 pixels
    apart, plus hashed integer noise of amplitude `noise` / 64 of the field's; the row is divided by its exact integer norm."""
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    qx, qy = 4 * x + int(shift_q[0]), 4 * y + int(shift_q[1])
    f = _grid_field(seed, qx, qy, C, cell, -64, 64) * 64
    n = (hash_u64(1000003 * (noise_seed + 1) + seed, np.arange(H * W * C).reshape(H, W, C)) % np.uint64(2 * noise + 1)).astype(np.int64) - noise
    f = f + n * cell * cell
    norm = np.sqrt((f * f).sum(2).astype(np.float64))  # the sum is an exact integer below 2^53
    m = (f.astype(np.float64) / np.maximum(norm, 1.0)[..., None] * (1.0 - 2.0 ** -20)).astype(np.float32)
    c = _grid_field(seed + 77 + noise_seed, qx, qy, 1, cell * 2, 0, 64)[..., 0].astype(np.float64) / (64.0 * 4 * cell * cell)
    return m, (0.3 + 0.6 * c).astype(np.float32)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.shape, a.dtype.str)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


# the fixture's cases: name -> (seed, (H1, W1), (H2, W2), C, S, shift of image 2 in quarter pixels)
FIXTURE_CASES = {"small": (11, (37, 45), (40, 48), 24, 2, (38, -25)), "large": (12, (72, 80), (72, 80), 24, 8, (38, -25))}


def fixture_inputs(name):
    """feats (feat11, feat21, feat22, feat12) and qonfs (qonf11, qonf21, qonf22, qonf12) of a fixture case: the two decoder passes
    see the same scene with different noise and different confidences."""
    seed, s1, s2, C, S, shift = FIXTURE_CASES[name]
    f11, q11 = scene_maps(seed, *s1, C, (0, 0), noise_seed=0)
    f21, q21 = scene_maps(seed, *s2, C, shift, noise_seed=1)
    f22, q22 = scene_maps(seed, *s2, C, shift, noise_seed=2)
    f12, q12 = scene_maps(seed, *s1, C, (0, 0), noise_seed=3)
    return (f11, f21, f22, f12), (q11, q21, q22, q12), S


def planted(H1, W1, H2, W2, C, links, background=True):
    """Maps of zeros with planted exact descriptors.  `links` is a list of (pixel of A, pixel of B, channel, value of A, value
    of B): A[pa][ch] = va and B[pb][ch] = vb, small dyadic values, so every similarity is an exact product or an exact sum of
    few.  background: pixel 0 of each map gets 2^-6 in the last channel, which gives the all-zero pixels a defined trajectory
    (every one of them ties at similarity 0 and goes to pixel 0, then stays)."""
    A, B = np.zeros((H1 * W1, C), np.float32), np.zeros((H2 * W2, C), np.float32)
    for pa, pb, ch, va, vb in links:
        if pa is not None:
            A[pa, ch] = va
        if pb is not None:
            B[pb, ch] = vb
    if background:
        A[0, C - 1] = B[0, C - 1] = 2.0 ** -6
    return A.reshape(H1, W1, C), B.reshape(H2, W2, C)


def chain_links(pixels_a, pixels_b, first_channel=0, exp0=-24):
    """The links of a descent chain a1 -> b1 -> a2 -> ... -> an <-> bn (n = len(pixels_a) = len(pixels_b)): link k couples its two
    pixels through a channel of its own with the value 2^(exp0 + k) on both sides, so the products 4^(exp0 + k) increase strictly
    along the chain and every pixel's best neighbour is the next one.  A seed at a1 needs n iterations."""
    links, k = [], 0
    for i in range(len(pixels_a)):
        if i > 0:
            links.append((pixels_a[i], pixels_b[i - 1], first_channel + k, 2.0 ** (exp0 + k), 2.0 ** (exp0 + k)))
            k += 1
        links.append((pixels_a[i], pixels_b[i], first_channel + k, 2.0 ** (exp0 + k), 2.0 ** (exp0 + k)))
        k += 1
    return links


# random cases of the GPU test: name -> (seed, (H1, W1), (H2, W2), C, S, max_iter).  tests/test_reciprocal_matches_cpu.py asserts that
# every seed of every case is decided, which is what allows the GPU test to ask for equality on all of them.
SWEEP_CASES = {
    "seeds1": (21, (5, 5), (37, 45), 24, 4, 10), "seeds63": (22, (21, 27), (37, 45), 24, 3, 10), "seeds64": (23, (24, 24), (37, 45), 24, 3, 10),
    "seeds65": (24, (15, 39), (37, 45), 24, 3, 10), "seeds90": (25, (27, 30), (37, 45), 24, 3, 10),
    "C1": (31, (12, 13), (19, 21), 1, 2, 10), "C3": (32, (12, 13), (19, 21), 3, 2, 10), "C4": (33, (12, 13), (19, 21), 4, 2, 10),
    "C5": (34, (12, 13), (19, 21), 5, 2, 10), "C33": (35, (12, 13), (19, 21), 33, 2, 10),
    "S1": (41, (12, 13), (9, 17), 24, 1, 10), "S8": (42, (20, 33), (37, 45), 24, 8, 10), "S_beyond": (43, (6, 7), (9, 17), 24, 16, 10),
    "iter1": (51, (12, 13), (19, 21), 24, 1, 1), "iter2": (51, (12, 13), (19, 21), 24, 1, 2),
}


def sweep_inputs(name):
    seed, s1, s2, C, S, max_iter = SWEEP_CASES[name]
    return random_maps(seed, *s1, C), random_maps(seed + 500, *s2, C), S, max_iter
