"""GPU checks of the 3D-3D alignment (csrc/align3d.hip through capi.align3d_estimate, align3d_fit, lift_keypoints and
depth_pair_register): exact agreement with the NumPy restatement, independence of the batch size, the reductions around every
block edge against long-double sums, the reference's own closed form and lifting (tests/golden/alignment.npz), the validity rule
of the lift, failure cases, and the RGB-D pair registration end to end."""

import os

import numpy as np
import pytest

import numpy_alignment as NAL
from alignment_scenes import OPTIONS, SCENES, depth_pair_scene, robust_scene
from mpsfm_amd import capi
from mpsfm_amd.sfm.estimators import estimate_rigid3d, estimate_sim3d, estimate_sim3d_robust, register_depth_pair

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "alignment.npz"))
# what a call reports apart from its device time; num_batches and num_models count the batches themselves
DECISIONS = ("success", "num_trials", "max_num_trials", "num_inliers", "lo_rounds")
EDGES = [3, 4, 255, 256, 257, 1023, 1024, 1025, 65535, 65536, 65537]


def _same_result(a, b, counters=DECISIONS):
    for k in counters:
        assert a[k] == b[k], k
    assert np.array_equal(a["inlier_mask"], b["inlier_mask"])
    assert a["tgt_from_src"].tobytes() == b["tgt_from_src"].tobytes() and a["scale"] == b["scale"]


@pytest.mark.parametrize("with_scale", [False, True])
@pytest.mark.parametrize("n,outliers,seed", SCENES)
def test_hip_matches_restatement(n, outliers, seed, with_scale):
    src, tgt, R, t, s, inl, ref, sampler_seed, _ = robust_scene(n, outliers, seed, with_scale)
    got = capi.align3d_estimate(src, tgt, with_scale, seed=sampler_seed, **OPTIONS)
    for k in DECISIONS:  # lo_rounds too: the local fit is well conditioned here
        assert got[k] == ref[k], k
    assert np.array_equal(got["inlier_mask"], ref["inlier_mask"])
    assert np.abs(got["tgt_from_src"] - ref["tgt_from_src"]).max() < 1e-9
    assert abs(got["scale"] - ref["scale"]) < 1e-9
    assert with_scale or got["scale"] == 1.0
    Rg = got["tgt_from_src"][:, :3]
    assert np.abs(Rg @ Rg.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(Rg) - 1.0) < 1e-14


@pytest.mark.parametrize("batch", [1, 7, 100, 4096])
def test_batch_size_does_not_change_the_result(batch):
    for with_scale in (False, True):
        src, tgt, *_, ref, sampler_seed, _ = robust_scene(1000, 0.7, 5, with_scale)
        base = capi.align3d_estimate(src, tgt, with_scale, seed=sampler_seed, **OPTIONS)
        got = capi.align3d_estimate(src, tgt, with_scale, seed=sampler_seed, batch_trials=batch, **OPTIONS)
        _same_result(got, base)
        assert got["num_trials"] == ref["num_trials"] and got["num_models"] >= got["num_batches"] >= 1


def test_two_calls_are_bitwise_identical():
    src, tgt, *_ = NAL.synthetic_problem(20000, 0.5, 31, True)
    a = capi.align3d_estimate(src, tgt, True, seed=3)
    b = capi.align3d_estimate(src, tgt, True, seed=3)
    _same_result(a, b, DECISIONS + ("num_batches", "num_models"))
    keep = np.arange(20000) % 3 == 0
    f1, f2 = capi.align3d_fit(src, tgt, keep, True), capi.align3d_fit(src, tgt, keep, True)
    assert f1["tgt_from_src"].tobytes() == f2["tgt_from_src"].tobytes() and f1["scale"] == f2["scale"]


def _fit_long_double(src, tgt, keep, with_scale):
    """The closed form from sums accumulated in long double: (M, s), or None below 3 points."""
    P, Q = src[keep].astype(np.longdouble), tgt[keep].astype(np.longdouble)
    if len(P) < 3:
        return None
    mp, mq = P.sum(0) / len(P), Q.sum(0) / len(Q)
    Pc, Qc = P - mp, Q - mq
    S = (Qc[:, :, None] * Pc[:, None, :]).sum(0)
    U, _, Vt = np.linalg.svd(S.astype(np.float64))
    R = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt
    s = float((S * R.astype(np.longdouble)).sum() / (Pc * Pc).sum()) if with_scale else 1.0
    return np.c_[R, (mq - s * (R.astype(np.longdouble) @ mp)).astype(np.float64)], s


@pytest.fixture(scope="module")
def edge_points():
    """{with_scale: (src, tgt without outliers, tgt with 30 % outliers, designed inliers)} of the largest edge size; a test takes the
    first n"""
    out = {}
    for with_scale in (False, True):
        src, clean, *_ = NAL.synthetic_problem(EDGES[-1], 0.0, 17, with_scale)
        same_src, tgt, R, t, s, inl = NAL.synthetic_problem(EDGES[-1], 0.3, 17, with_scale)
        assert np.array_equal(src, same_src)
        for a in (src, clean, tgt, inl):
            a.setflags(write=False)
        out[with_scale] = (src, clean, tgt, inl)
    return out


@pytest.mark.parametrize("n", EDGES)
def test_fit_reductions_at_block_edges(n, edge_points):
    """n around a workgroup (256), around one scoring block's 1024 observations and around the 64-block cap (65536), where the
    grid-stride loops start; no mask, every third point, three points."""
    src, tgt = edge_points[True][0][:n], edge_points[True][1][:n]  # a rigid fit of scaled points is a fit all the same
    three = np.zeros(n, bool)
    three[[0, n // 2, n - 1]] = True
    for mask in (None, np.arange(n) % 3 == 0, three):
        keep = np.ones(n, bool) if mask is None else mask
        for with_scale in (False, True):
            want = _fit_long_double(src, tgt, keep, with_scale)
            got = capi.align3d_fit(src, tgt, mask, with_scale=with_scale)
            assert got["num_inliers"] == keep.sum()
            assert got["success"] == (want is not None)
            if want is not None:
                assert np.abs(got["tgt_from_src"] - want[0]).max() < 1e-12
                assert abs(got["scale"] - want[1]) < 1e-12
                assert with_scale or got["scale"] == 1.0


@pytest.mark.parametrize("n", EDGES)
def test_estimate_mask_and_count_at_block_edges(n, edge_points):
    for with_scale in (False, True):
        src, clean, tgt, inl = (a[:n] for a in edge_points[with_scale])
        if n < 255:  # three or four pairs with an outlier among them have no model to speak of
            tgt, inl = clean, np.ones(n, bool)
        got = capi.align3d_estimate(src, tgt, with_scale, seed=n)
        assert got["success"] and got["max_num_trials"] == 5000
        res = NAL.residuals(got["tgt_from_src"], got["scale"], src, tgt)
        assert not (np.abs(res - 0.01) <= 1e-7 * 0.01).any()  # no residual at the threshold: the mask is decided
        assert np.array_equal(got["inlier_mask"], res <= 0.01)
        assert got["num_inliers"] == got["inlier_mask"].sum() >= 3
        if n >= 255:
            assert got["inlier_mask"][inl].all() and got["num_inliers"] <= inl.sum() + 0.02 * n


@pytest.mark.parametrize("tag", ["a", "b"])
def test_lift_is_the_references_bit_for_bit(tag):
    xyz, valid = capi.lift_keypoints(GOLDEN[f"lift_{tag}_depth"], GOLDEN[f"lift_{tag}_intr"], GOLDEN[f"lift_{tag}_xy"])
    assert valid.all()
    assert np.array_equal(xyz, GOLDEN[f"lift_{tag}_xyz"])
    xyz32, valid32 = capi.lift_keypoints(GOLDEN[f"lift_{tag}_depth"].astype(np.float32), GOLDEN[f"lift_{tag}_intr"], GOLDEN[f"lift_{tag}_xy"])
    want32, _ = NAL.lift(GOLDEN[f"lift_{tag}_depth"].astype(np.float32).astype(np.float64), GOLDEN[f"lift_{tag}_intr"], GOLDEN[f"lift_{tag}_xy"])
    assert valid32.all() and np.array_equal(xyz32, want32)  # a float32 map is widened exactly


def test_fit_is_the_references_closed_form():
    for tag in ("4", "10", "100", "1000", "mirrored"):
        got = capi.align3d_fit(GOLDEN[f"fit_{tag}_src"], GOLDEN[f"fit_{tag}_tgt"])
        assert got["success"] and got["scale"] == 1.0 and got["num_inliers"] == len(GOLDEN[f"fit_{tag}_src"])
        assert np.abs(got["tgt_from_src"][:, :3] - GOLDEN[f"fit_{tag}_R"]).max() < 1e-12, tag
        assert np.abs(got["tgt_from_src"][:, 3] - GOLDEN[f"fit_{tag}_t"]).max() < 1e-12, tag
        assert abs(np.linalg.det(got["tgt_from_src"][:, :3]) - 1.0) < 1e-12
    for P, Q, R, t in zip(*(GOLDEN[f"fit_triples_{k}"] for k in ("src", "tgt", "R", "t"))):
        got = capi.align3d_fit(P, Q)
        assert got["success"] and got["num_inliers"] == 3
        assert np.abs(got["tgt_from_src"][:, :3] - R).max() < 1e-12 and np.abs(got["tgt_from_src"][:, 3] - t).max() < 1e-12
    T = estimate_rigid3d(GOLDEN["fit_100_src"], GOLDEN["fit_100_tgt"])
    assert T.scale == 1.0 and np.abs(T.rotation.matrix() - GOLDEN["fit_100_R"]).max() < 1e-12
    assert np.abs(T.translation - GOLDEN["fit_100_t"]).max() < 1e-12 and T.rotation.quat.shape == (4,)
    exact = 1.7 * (GOLDEN["fit_100_src"] @ GOLDEN["fit_100_R"].T + GOLDEN["fit_100_t"])
    assert abs(estimate_sim3d(GOLDEN["fit_100_src"], exact).scale - 1.7) < 1e-12


def test_validity_of_the_lift():
    H, W = 5, 4
    rng = np.random.default_rng(5)
    depth = rng.uniform(0.5, 9.0, (H, W))
    K = np.array([3.6, 3.4, 1.7, 2.7])
    xy = np.array([[W - 1.0, 1.5], [W - 1 - 1e-12, 1.5], [-1e-9, 1.5], [1.5, H - 1.0], [1.5, H - 1 - 1e-12], [0.0, 0.0], [1.5, -1e-9],
                   [np.nan, 1.0], [1.0, np.inf], [1e300, 1.0], [-np.inf, 1.0], [2.25, 3.75]])
    want_valid = np.array([0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 1], bool)
    xyz, valid = capi.lift_keypoints(depth, K, xy)
    want_xyz, restated_valid = NAL.lift(depth, K, xy)
    assert np.array_equal(restated_valid, want_valid) and np.array_equal(valid, want_valid)
    assert np.array_equal(xyz, want_xyz) and not xyz[~want_valid].any() and xyz[want_valid].all()
    at = np.array([[2.5, 1.5], [0.5, 3.5]])  # the first keypoint's cell is rows 1-2, columns 2-3; the second's is untouched
    for hole in (0.0, -1.0, np.nan, np.inf):
        for r, c in ((1, 2), (1, 3), (2, 2), (2, 3)):
            d = depth.copy()
            d[r, c] = hole
            xyz, valid = capi.lift_keypoints(d, K, at)
            assert list(valid) == [False, True] and not xyz[0].any()
            assert np.array_equal(xyz, NAL.lift(d, K, at)[0])


def _line(rng, n=200):
    return np.outer(rng.uniform(-1, 1, n), [1.0, 2.0, -0.5]) + [0.3, 0.1, 2.0]


@pytest.mark.parametrize("case", ["source on a line", "target on a line", "target coincident"])
def test_degenerate_sets_give_no_model(case):
    src, tgt, *_ = NAL.synthetic_problem(200, 0.0, 4)
    rng = np.random.default_rng(3)
    a, b = {"source on a line": (_line(rng), tgt), "target on a line": (src, _line(rng)),
            "target coincident": (src, np.tile([[0.2, 0.1, 4.0]], (200, 1)))}[case]
    ref = NAL.estimate(a, b, max_num_trials=1000)  # every minimal sample is degenerate: the whole budget runs
    got = capi.align3d_estimate(a, b, max_num_trials=1000)
    assert ref["success"] is False and got["success"] is False
    assert got["num_inliers"] == 0 and not got["inlier_mask"].any()
    assert got["num_trials"] == ref["num_trials"] == ref["max_num_trials"] == got["max_num_trials"] == 1000
    assert capi.align3d_fit(a, b)["success"] is False and NAL.fit(a, b)[0] is None
    assert estimate_sim3d_robust(a, b) is None and estimate_rigid3d(a, b) is None


def test_three_points():
    src, tgt, *_ = NAL.synthetic_problem(200, 0.0, 4)
    # a degenerate triangle (two coincident points)
    P3 = np.array([[0.0, 0.0, 5.0], [0.0, 0.0, 5.0], [1.0, 0.5, 6.0]])
    for a, b in ((P3, tgt[:3]), (src[:3], P3)):
        ref, got = NAL.estimate(a, b), capi.align3d_estimate(a, b)
        assert ref["success"] is False and got["success"] is False and got["num_trials"] == ref["num_trials"] == 5000
        assert capi.align3d_fit(a, b)["success"] is False
    # a proper triangle: the sample is the model
    for with_scale in (False, True):
        ref = NAL.estimate(src[:3], tgt[:3], with_scale)
        got = capi.align3d_estimate(src[:3], tgt[:3], with_scale)
        fit = capi.align3d_fit(src[:3], tgt[:3], with_scale=with_scale)
        assert got["success"] and ref["success"] and got["num_inliers"] == ref["num_inliers"] == 3 and got["inlier_mask"].all()
        assert got["num_trials"] == ref["num_trials"] and got["lo_rounds"] == ref["lo_rounds"] == 0
        assert fit["success"] and fit["num_inliers"] == 3
        assert np.abs(got["tgt_from_src"] - fit["tgt_from_src"]).max() < 1e-9 and abs(got["scale"] - fit["scale"]) < 1e-9
        assert np.abs(got["tgt_from_src"] - ref["tgt_from_src"]).max() < 1e-9


@pytest.mark.parametrize("with_scale", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_all_pairs_outliers_match_restatement(seed, with_scale):
    """Unrelated point sets: unlike a P3P sample, three pairs do not explain themselves (the triangles are not congruent, nor
    similar), so the best support is a handful of chance inliers, or none, and the whole budget runs.  The counts are equal; the
    mask is compared when the restatement reports no fragile decision."""
    rng = np.random.default_rng(3)
    Pr, Qr = rng.uniform(-2, 2, (400, 3)), rng.uniform(-4, 4, (400, 3))
    ref = NAL.estimate(Pr, Qr, with_scale, seed=seed, max_num_trials=1500)
    got = capi.align3d_estimate(Pr, Qr, with_scale, seed=seed, max_num_trials=1500)
    print(f"seed {seed} with_scale {with_scale}: {ref['num_inliers']} inliers, fragile {ref['fragile']}")
    assert got["success"] == ref["success"] and got["num_inliers"] == ref["num_inliers"] < 20
    assert got["num_trials"] == ref["num_trials"] == 1500 and got["lo_rounds"] == ref["lo_rounds"]
    if not ref["fragile"]:
        assert np.array_equal(got["inlier_mask"], ref["inlier_mask"])


def test_argument_errors():
    src, tgt, *_ = NAL.synthetic_problem(20, 0.0, 4)
    bad = src.copy()
    bad[5, 1] = np.nan
    for call in (lambda: capi.align3d_estimate(src[:2], tgt[:2]), lambda: capi.align3d_estimate(bad, tgt), lambda: capi.align3d_estimate(src, bad),
                 lambda: capi.align3d_estimate(src, tgt, max_error=0.0), lambda: capi.align3d_fit(src[:2], tgt[:2]), lambda: capi.align3d_fit(bad, tgt)):
        with pytest.raises(capi.MpsfmHipError) as e:
            call()
        assert e.value.code == -1  # MPSFM_EINVAL


def _composition(S, depth1, with_scale, **options):
    """depth_pair_register from the single calls: two lifts, a host compaction, the estimate, the mask scattered back."""
    m = S["matches"]
    l0, v0 = capi.lift_keypoints(S["depth0"], S["intr"], S["kps0"][m[:, 0]])
    l1, v1 = capi.lift_keypoints(depth1, S["intr"], S["kps1"][m[:, 1]])
    valid = v0 & v1
    est = capi.align3d_estimate(l0[valid], l1[valid], with_scale, **options)
    mask = np.zeros(len(m), bool)
    mask[valid] = est["inlier_mask"]
    return dict(est, inlier_mask=mask), valid, l0, l1


@pytest.mark.parametrize("scale", [1.0, 1.7])
def test_depth_pair_register_end_to_end(scale):
    S = depth_pair_scene()
    m, with_scale = S["matches"], scale != 1.0
    depth1 = S["depth1"] * scale
    got = capi.depth_pair_register(S["depth0"], S["intr"], depth1, S["intr"], S["kps0"], S["kps1"], m, with_scale, seed=2)
    want, valid, l0, l1 = _composition(S, depth1, with_scale, seed=2)
    _same_result(got, want, DECISIONS + ("num_batches", "num_models"))
    assert np.array_equal(got["valid"], valid)
    assert got["lifted0"].tobytes() == l0.tobytes() and got["lifted1"].tobytes() == l1.tobytes()
    r0, rv0 = NAL.lift(S["depth0"], S["intr"], S["kps0"][m[:, 0]])
    r1, rv1 = NAL.lift(depth1, S["intr"], S["kps1"][m[:, 1]])
    assert np.array_equal(got["valid"], rv0 & rv1) and not got["valid"][S["touched"]].any() and got["valid"].sum() >= 270
    assert np.array_equal(got["lifted0"], r0) and np.array_equal(got["lifted1"], r1)
    assert not got["inlier_mask"][~got["valid"]].any() and not got["inlier_mask"][S["wrong"]].any()
    assert got["success"] and got["num_inliers"] == got["inlier_mask"].sum() >= 180
    assert np.abs(got["tgt_from_src"] - np.c_[S["R"], scale * S["t"]]).max() < 2e-2
    assert abs(got["scale"] - scale) < 1e-2 and (with_scale or got["scale"] == 1.0)
    # float32 maps through the estimator's interface
    res = register_depth_pair(S["kps0"], S["kps1"], m, S["depth0"].astype(np.float32), depth1.astype(np.float32), S["intr"], S["intr"],
                              with_scale=with_scale, random_seed=2)
    assert res is not None and np.abs(res["tgt_from_src"].matrix() - np.c_[scale * S["R"], scale * S["t"]]).max() < 2e-2
    assert res["inlier_mask"].shape == (300,) and res["num_inliers"] >= 180
    # fewer than 3 valid matches: no model
    few = np.r_[m[S["touched"]], m[~S["touched"] & got["valid"]][:2]]
    none = capi.depth_pair_register(S["depth0"], S["intr"], depth1, S["intr"], S["kps0"], S["kps1"], few, with_scale)
    assert none["success"] is False and none["valid"].sum() == 2 and not none["inlier_mask"].any() and none["num_trials"] == 0
    assert register_depth_pair(S["kps0"], S["kps1"], few, S["depth0"], depth1, S["intr"], S["intr"], with_scale=with_scale) is None
