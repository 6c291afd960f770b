"""mpsfm_radius_nms / mpsfm_thin_dense_matches / mpsfm_assign_keypoints (csrc/dense_matches.hip) on the device: exact
equality with the fixture computed by the reference's own code and with the NumPy restatement (tests/numpy_dense_matches.py).
Every comparison is an equality of index sets: the decisions are fp64 comparisons of dx*dx + dy*dy, bit-exact by design."""

import functools
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import numpy_dense_matches as ND
from mpsfm_amd import capi
from mpsfm_amd.extraction.pairwise import utils as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "reference_dense_matches.npz"))
RADIUS = float(GOLD["radius"])


def kept(points, scores, radius, order=None, info=False):
    r = capi.radius_nms(points, scores, radius, order=order, return_info=info)
    return (np.flatnonzero(r[0]), r[1]) if info else np.flatnonzero(r)


def check(points, scores, radius, order=None):
    got = kept(points, scores, radius, order)
    want = ND.sparse_nms(points, scores, radius, order=order)
    assert np.array_equal(got, want), (len(got), len(want))
    return got


# ---- fixtures -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["float_distinct", "int_distinct"])
def test_nms_equals_the_reference(case):
    pts, sc, want = GOLD[f"{case}_points"], GOLD[f"{case}_scores"], GOLD[f"{case}_kept"]
    got = U.sparse_nms(pts, sc, RADIUS)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    if case == "float_distinct":
        assert np.array_equal(U.sparse_nms(pts, sc, RADIUS, order=GOLD["float_distinct_order"]), want)
        import torch

        assert np.array_equal(U.sparse_nms(torch.from_numpy(pts), torch.from_numpy(sc), RADIUS), want)
        assert np.array_equal(U.sparse_nms(pts.astype(np.float64), sc.astype(np.float64), RADIUS), want)


def test_nms_ties_with_the_recorded_order_and_with_the_stable_rule():
    pts, sc = GOLD["ties_points"], GOLD["ties_scores"]
    assert np.array_equal(U.sparse_nms(pts, sc, RADIUS, order=GOLD["ties_order"]), GOLD["ties_kept"])  # the reference's result
    assert np.array_equal(U.sparse_nms(pts, sc, RADIUS), ND.sparse_nms(pts, sc, RADIUS))  # lower index first
    z = np.where(np.arange(len(sc)) % 2 == 0, -0.0, 0.0)  # -0.0 ties with +0.0
    assert np.array_equal(U.sparse_nms(pts, z, RADIUS), ND.sparse_nms(pts, np.zeros(len(sc)), RADIUS))


def test_two_pass_leg_equals_the_reference():
    g = {k: GOLD[f"combined_separated_{k}"] for k in ("sparse0", "sparse1", "dense0", "dense1", "dscores", "kept")}
    for flag in (True, False):
        d0, d1, ds = U.thin_dense_matches(g["dense0"], g["dense1"], g["dscores"], g["sparse0"], g["sparse1"], RADIUS, reference_slice=flag)
        k = g["kept"]
        assert np.array_equal(d0, g["dense0"][k]) and np.array_equal(d1, g["dense1"][k]) and np.array_equal(ds, g["dscores"][k])
        assert d0.dtype == np.float32


def test_assignment_equals_the_reference():
    got = U.assign_keypoints(GOLD["assign_query"], GOLD["assign_kps"], float(GOLD["assign_max_error"]))
    assert got.dtype == np.int64 and np.array_equal(got, GOLD["assign_ids"])


# ---- boundary -----------------------------------------------------------------------------------------------------------
def test_nms_radius_is_inclusive_to_the_ulp():
    sc = np.array([2.0, 1.0])
    assert kept(np.array([[0.0, 0.0], [3.0, 4.0]]), sc, 5.0).tolist() == [0]  # d2 == 25 exactly: suppressed
    for out in ([np.nextafter(3.0, 4.0), 4.0], [3.0, np.nextafter(4.0, 5.0)]):
        assert kept(np.array([[0.0, 0.0], out]), sc, 5.0).tolist() == [0, 1]
    for ins in ([np.nextafter(3.0, 0.0), 4.0], [3.0, np.nextafter(4.0, 0.0)]):
        assert kept(np.array([[0.0, 0.0], ins]), sc, 5.0).tolist() == [0]
    assert kept(np.array([[-3.0, -4.0], [0.0, 0.0]]), sc, 5.0).tolist() == [0]


def test_assignment_radius_is_exclusive_to_the_ulp():
    q = np.array([[0.0, 0.0]])
    assert capi.assign_keypoints_ids(q, np.array([[3.0, 4.0]]), 5.0).tolist() == [-1]  # exactly max_error: none
    assert capi.assign_keypoints_ids(q, np.array([[3.0, np.nextafter(4.0, 0.0)]]), 5.0).tolist() == [0]
    assert capi.assign_keypoints_ids(q, np.array([[3.0, 4.0]]), np.nextafter(5.0, 6.0)).tolist() == [0]
    assert capi.assign_keypoints_ids(q, np.array([[0.0, 0.0]]), 0.0).tolist() == [-1]
    # equidistant nearest keypoints: the lowest index, wherever it sits in the array
    k = np.array([[9.0, 9.0], [0.0, 2.0], [2.0, 0.0], [0.0, -2.0], [-2.0, 0.0], [0.0, 2.0]])
    assert capi.assign_keypoints_ids(q, k, 3.0).tolist() == [1]
    assert capi.assign_keypoints_ids(q, k[::-1].copy(), 3.0).tolist() == [0]


# ---- grid ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [(0.0, 0.0), (-1000.5, -2000.25)])
def test_neighbours_in_all_eight_adjacent_cells(shift):
    """The cells are 6 (1 + 2^-20) wide from the minimum corner (the anchor): the centre lies in cell (1, 1) and each
    neighbour in another adjacent cell.  One call per neighbour, so a missed cell cannot hide behind another suppressor."""
    c = 6.0 * (1.0 + 2.0 ** -20)
    centre = np.array([9.1, 9.1])
    cells = set()
    for off in [(-5, 0), (5, 0), (0, -5), (0, 5), (-4, -4), (-4, 4), (4, -4), (4, 4)]:
        nb = centre + off
        cells.add(tuple(np.floor(nb / c).astype(int) - np.floor(centre / c).astype(int)))
        pts = np.array([[0.0, 0.0], centre, nb, [30.0, 30.0]]) + shift
        assert check(pts, np.array([0.0, 3.0, 2.0, 1.0]), 6.0).tolist() == [0, 1, 3]
        assert capi.assign_keypoints_ids(pts[1:2], pts[[0, 2, 3]], 6.0).tolist() == [1]
    assert len(cells) == 8 and (0, 0) not in cells


def test_points_on_cell_edges_and_lattices():
    rng = np.random.default_rng(2)
    gx, gy = np.meshgrid(np.arange(20.0), np.arange(20.0))
    for step, all_kept in ((6.0, False), (6.0 * (1.0 + 2.0 ** -30), True), (6.0 * (1.0 + 2.0 ** -20), True)):
        pts = np.stack([gx.ravel(), gy.ravel()], 1) * step - 17 * step  # negative and positive, on the cell edges for the last step
        got = check(pts, rng.permutation(400).astype(np.float64), 6.0)
        assert (len(got) == 400) == all_kept
    q = rng.random((2000, 2)) * 130 - 108
    assert np.array_equal(capi.assign_keypoints_ids(q, pts, 6.0), ND.assign_keypoints(q, pts, 6.0))


def test_far_outlier_does_not_blow_up_the_cell_table():
    rng = np.random.default_rng(3)
    pts = np.concatenate([rng.random((500, 2)) * [512, 384], [[1e7, 1e7]]])
    sc = rng.permutation(501).astype(np.float64)
    got, info = kept(pts, sc, 6.0, info=True)
    assert np.array_equal(got, ND.sparse_nms(pts, sc, 6.0)) and 500 in got
    assert info["cells"] <= 501 and info["max_cell_points"] >= 250  # the cells widened to extent / 4096
    q = np.concatenate([rng.random((500, 2)) * [512, 384], [[1e7 + 1, 1e7], [-1e9, 5.0], [1e12, 1e12]]])
    assert np.array_equal(capi.assign_keypoints_ids(q, pts, 6.0), ND.assign_keypoints(q, pts, 6.0))


def test_radius_zero_suppresses_only_coincident_points():
    rng = np.random.default_rng(4)
    pts = rng.integers(0, 12, (600, 2)).astype(np.float64)
    sc = np.round(rng.random(600) * 4)
    got = check(pts, sc, 0.0)
    assert len(got) == len(np.unique(pts, axis=0)) < 600
    same = np.zeros((300, 2)) + 7.25  # all coincident: extent 0 and radius 0
    assert kept(same, np.arange(300.0), 0.0).tolist() == [299]


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_sizes_around_the_tile(n):
    rng = np.random.default_rng(100 + n)
    pts = rng.random((n, 2)) * 90
    sc = np.round(rng.random(n) * 10)  # ties: the index rule decides
    got = check(pts, sc, 6.0)
    assert np.array_equal(U.sparse_nms(pts.astype(np.float32), sc.astype(np.float32), 6.0),
                          ND.sparse_nms(pts.astype(np.float32), sc.astype(np.float32), 6.0))
    order = rng.permutation(n)
    check(pts, sc, 6.0, order=order)
    if n:
        kps = pts[got]
        assert np.array_equal(capi.assign_keypoints_ids(pts, kps, 6.0), ND.assign_keypoints(pts, kps, 6.0))


# ---- progress -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", [1, -1])
def test_chain_of_2048_needs_every_round(direction):
    """Collinear points 4 apart, radius 6, strictly monotone scores: every point waits for its neighbour's decision, the
    dependency chain is as long as the input.  A round cap, or a loop that stops before the undecided count is zero, fails."""
    n = 2048
    x = np.arange(n) * 4.0
    sc = (np.arange(n)[::-1] if direction == 1 else np.arange(n)).astype(np.float64)
    perm = np.random.default_rng(6).permutation(n)  # the caller's index order is not the spatial one
    pts = np.stack([x, np.full(n, 3.0)], 1)[perm]
    got, info = kept(pts, sc[perm], 6.0, info=True)
    want = np.sort(np.flatnonzero(perm % 2 == (0 if direction == 1 else 1)))
    assert np.array_equal(got, want) and len(got) == n // 2
    assert info["launches"] > 1 and 1 <= info["rounds"] <= info["launches"]


def test_dense_cell_of_5000_points():
    rng = np.random.default_rng(7)
    cluster = 100.0 + rng.random((5000, 2)) * 2.0
    cluster[1000:4000] = [101.0, 101.0]  # thousands of coincident points
    pts = np.concatenate([cluster, rng.random((100, 2)) * [512, 384]])
    sc = rng.permutation(5100).astype(np.float64)
    shuffle = rng.permutation(5100)
    pts, sc = pts[shuffle], sc[shuffle]
    got, info = kept(pts, sc, 6.0, info=True)
    assert np.array_equal(got, ND.sparse_nms(pts, sc, 6.0))
    in_cluster = np.flatnonzero(shuffle < 5000)
    survivors = np.intersect1d(got, in_cluster)
    assert survivors.tolist() == [in_cluster[np.argmax(sc[in_cluster])]]
    assert info["max_cell_points"] >= 3000


# ---- the two-pass leg against the restatement --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def crowded():
    """Matched sparse keypoints that have NOT been thinned: some lie within the radius of each other."""
    rng = np.random.default_rng(8)
    s0 = (rng.random((300, 2)) * [256, 192]).astype(np.float32)
    s1 = (s0 * 0.9 + 11 + rng.normal(0, 1, s0.shape)).astype(np.float32)
    d0 = (rng.random((1500, 2)) * [256, 192]).astype(np.float32)
    d1 = (d0 * 0.9 + 11 + rng.normal(0, 1, d0.shape)).astype(np.float32)
    ds = np.round(rng.random(1500) * 50).astype(np.float32) / 50
    want = {flag: ND.thin_dense_mask(d0, d1, ds, s0, s1, 6.0, flag) for flag in (True, False)}
    return s0, s1, d0, d1, ds, want


def test_two_pass_leg_dense_only():
    _, _, d0, d1, ds, _ = crowded()
    got = np.flatnonzero(capi.thin_dense_matches_mask(d0, d1, ds, radius=6.0))
    assert np.array_equal(got, ND.thin_dense_mask(d0, d1, ds, radius=6.0)) and 0 < len(got) < len(d0)
    a, b, c = U.thin_dense_matches(d0, d1, ds, nms_radius=6)
    assert np.array_equal(a, d0[got]) and np.array_equal(b, d1[got]) and np.array_equal(c, ds[got])


def test_two_pass_leg_with_the_reference_slice():
    s0, s1, d0, d1, ds, want = crowded()
    got, info = capi.thin_dense_matches_mask(d0, d1, ds, s0, s1, 6.0, reference_slice=True, return_info=True)
    assert np.array_equal(np.flatnonzero(got), want[True])
    assert not np.array_equal(want[True], want[False])  # the slice drops surviving dense matches here
    assert info["rounds"] >= 2 and info["launches"] >= info["rounds"] and info["ms"] > 0
    a, _, _ = U.thin_dense_matches(d0, d1, ds, s0, s1)  # the wrapper's default is the reference's behaviour
    assert np.array_equal(a, d0[want[True]])


def test_two_pass_leg_without_the_reference_slice():
    s0, s1, d0, d1, ds, want = crowded()
    got = np.flatnonzero(capi.thin_dense_matches_mask(d0, d1, ds, s0, s1, 6.0, reference_slice=False))
    assert np.array_equal(got, want[False]) and len(want[False]) > len(want[True])


def test_two_pass_leg_with_an_empty_dense_set():
    s0, s1, _, _, _, _ = crowded()
    e2, e1 = np.zeros((0, 2), np.float32), np.zeros(0, np.float32)
    a, b, c = U.thin_dense_matches(e2, e2, e1, s0, s1)
    assert a.shape == (0, 2) and b.shape == (0, 2) and c.shape == (0,)
    assert capi.thin_dense_matches_mask(e2, e2, e1, s0, s1).tolist() == []


# ---- determinism ----------------------------------------------------------------------------------------------------------
def test_results_are_identical_run_to_run_and_across_host_threads():
    s0, s1, d0, d1, ds, want = crowded()
    pts, sc = GOLD["ties_points"], GOLD["ties_scores"]
    q, kps = GOLD["assign_query"][:5000], GOLD["assign_kps"]

    def work():
        return (capi.radius_nms(pts, sc, RADIUS), capi.thin_dense_matches_mask(d0, d1, ds, s0, s1, 6.0),
                capi.assign_keypoints_ids(q, kps, 8.0))

    first = work()
    again = work()
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    out = [None, None]

    def run(slot):
        out[slot] = [work() for _ in range(3)]

    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for res in out:
        assert res is not None
        for r in res:
            assert all(np.array_equal(a, b) for a, b in zip(first, r))


def test_results_do_not_depend_on_what_the_device_blocks_held():
    env = dict(os.environ, MPSFM_POISON="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_dense_matches_worker.py")], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
