"""Fixture for the dense-match thinning (tests/golden/reference_dense_matches.npz), computed BY THE REFERENCE'S OWN CODE,
imported by file path:

  mpsfm/extraction/pairwise/models/utils/generic.py   sparse_nms        (torch.argsort + SciPy KDTree.query_ball_point)
  mpsfm/extraction/pairwise/models/utils/warp.py      assign_keypoints  (SciPy KDTree.query with distance_upper_bound)

Cases (every condition a case rests on is asserted here, so the reference alone satisfies it):
  float_distinct      3 000 float32 points in 512 x 384, distinct scores, radius 6.  The reference's sort order is recorded;
                      with distinct scores it is THE descending order, and the restatement without `order` equals the reference.
  int_distinct        integer pixel coordinates in 160 x 120, distinct scores: distances of exactly 6 occur between points
                      (asserted), the inclusive boundary of the suppression.
  ties                scores quantised to 1/8: many equal scores.  `order` is what the reference's own sort expression
                      (torch.argsort(torch.tensor(scores), descending=True)) gave here; with it the restatement equals
                      the reference.
  combined_separated  the two-pass `sparse+dense` leg of match_dense_2view.py:127-151 with 250 matched sparse keypoints
                      pairwise farther apart than the radius in BOTH images (asserted): all of them survive, the slice
                      [n_sparse:] is exact and their order among themselves (all score 100) cannot matter.
  assign              20 000 queries x 1 000 keypoints, max_error 8: nearest and second-nearest distance differ for every
                      query (asserted), so the answer does not depend on a tie rule.
The file holds inputs and outputs only.

Run in the build container:  python tests/golden/make_golden_dense_matches.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_reference import ROOT, load_by_path  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy_dense_matches as ND  # noqa: E402

generic = load_by_path("ref_generic", "mpsfm/extraction/pairwise/models/utils/generic.py")
warp = load_by_path("ref_warp", "mpsfm/extraction/pairwise/models/utils/warp.py")
RADIUS = 6.0


def reference_order(scores):
    return torch.argsort(torch.tensor(scores), descending=True).numpy().astype(np.int64)


def distinct_scores(rng, n):
    s = rng.permutation(n).astype(np.float32) / np.float32(n)
    assert len(np.unique(s)) == n
    return s


def min_pair_distance2(p):
    p = p.astype(np.float64)
    best = np.inf
    for i in range(len(p) - 1):
        best = min(best, ND.d2_to(p[i + 1:], p[i]).min())
    return best


def main():
    rng = np.random.default_rng(20240917)
    out = {}

    pts = (rng.random((3000, 2)) * [512, 384]).astype(np.float32)
    sc = distinct_scores(rng, 3000)
    ref = generic.sparse_nms(pts, sc, RADIUS)
    order = reference_order(sc)
    assert np.array_equal(ND.sparse_nms(pts, sc, RADIUS), ref) and np.array_equal(ND.sparse_nms(pts, sc, RADIUS, order=order), ref)
    out.update(float_distinct_points=pts, float_distinct_scores=sc, float_distinct_order=order, float_distinct_kept=ref.astype(np.int64))

    pts = np.stack([rng.integers(0, 160, 3000), rng.integers(0, 120, 3000)], 1).astype(np.float32)
    sc = distinct_scores(rng, 3000)
    ref = generic.sparse_nms(pts, sc, RADIUS)
    n_exact = sum(int((ND.d2_to(pts.astype(np.float64), p) == 36.0).sum()) for p in pts.astype(np.float64))
    assert n_exact > 100, n_exact
    # the boundary decides: with an exclusive comparison the result differs
    r_in = np.nextafter(RADIUS, 0.0)
    assert not np.array_equal(ND.sparse_nms(pts, sc, r_in), ref)
    assert np.array_equal(ND.sparse_nms(pts, sc, RADIUS), ref)
    out.update(int_distinct_points=pts, int_distinct_scores=sc, int_distinct_kept=ref.astype(np.int64))

    pts = (rng.random((3000, 2)) * [512, 384]).astype(np.float32)
    sc = (np.round(rng.random(3000) * 8) / 8).astype(np.float32)
    assert len(np.unique(sc)) <= 9
    ref = generic.sparse_nms(pts, sc, RADIUS)
    order = reference_order(sc)
    assert np.array_equal(ND.sparse_nms(pts, sc, RADIUS, order=order), ref)
    out.update(ties_points=pts, ties_scores=sc, ties_order=order, ties_kept=ref.astype(np.int64),
               ties_order_is_stable=np.array(np.array_equal(order, ND.priority_order(sc))))

    # matched sparse keypoints, separated in both images: candidates thinned by the restatement in image 0, then in image 1
    def warp01(p):
        return (p * [0.9, 0.95] + [20.0, 7.0] + 3.0 * np.sin(p[:, ::-1] / 40.0)).astype(np.float32)

    cand0 = (rng.random((4000, 2)) * [512, 384]).astype(np.float32)
    cand1 = warp01(cand0.astype(np.float64))
    k = ND.sparse_nms(cand0, np.arange(4000)[::-1], 2 * RADIUS)
    k = k[ND.sparse_nms(cand1[k], np.arange(len(k))[::-1], 2 * RADIUS)][:250]
    s0, s1 = cand0[k], cand1[k]
    assert len(s0) == 250 and min_pair_distance2(s0) > RADIUS * RADIUS and min_pair_distance2(s1) > RADIUS * RADIUS
    d0 = (rng.random((3000, 2)) * [512, 384]).astype(np.float32)
    d1 = (warp01(d0.astype(np.float64)) + rng.normal(0, 0.5, (3000, 2))).astype(np.float32)
    dsc = distinct_scores(rng, 3000)
    ns = len(s0)
    # match_dense_2view.py:133-151 with the reference's sparse_nms
    dk0, dk1, ds, idx = d0, d1, dsc, np.arange(3000)
    for sp, which in ((s0, 0), (s1, 1)):
        comb = np.concatenate([sp, (dk0, dk1)[which]])
        scores_comb = np.concatenate([np.ones(ns) * 100, ds], axis=0)
        kept = generic.sparse_nms(comb, scores_comb, RADIUS)
        assert np.array_equal(kept[:ns], np.arange(ns))  # every sparse point survived
        mask = kept[ns:] - ns
        dk0, dk1, ds, idx = dk0[mask], dk1[mask], ds[mask], idx[mask]
    for flag in (True, False):
        assert np.array_equal(ND.thin_dense_mask(d0, d1, dsc, s0, s1, RADIUS, flag), idx)
    assert 0 < len(idx) < 3000
    out.update(combined_separated_sparse0=s0, combined_separated_sparse1=s1, combined_separated_dense0=d0, combined_separated_dense1=d1,
               combined_separated_dscores=dsc, combined_separated_kept=idx.astype(np.int64))

    kps = (rng.random((1000, 2)) * [512, 384]).astype(np.float32)
    q = (rng.random((20000, 2)) * [540, 400] - [14, 8]).astype(np.float32)
    ref = np.asarray(warp.assign_keypoints(q, kps, 8.0), np.int64)
    q64, k64 = q.astype(np.float64), kps.astype(np.float64)
    for i in range(len(q)):
        d2 = np.sort(ND.d2_to(k64, q64[i]))
        assert d2[0] != d2[1]
    assert np.array_equal(ND.assign_keypoints(q, kps, 8.0), ref) and (ref >= 0).sum() > 1000 and (ref < 0).sum() > 1000
    out.update(assign_query=q, assign_kps=kps, assign_max_error=np.array(8.0), assign_ids=ref)

    out["radius"] = np.array(RADIUS)
    path = os.path.join(HERE, "reference_dense_matches.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: (v.shape, str(v.dtype)) for k, v in out.items()})


if __name__ == "__main__":
    main()
