"""mpsfm_depth_consistency (csrc/depth_consistency.hip) on the device: against the reference's own results
(tests/golden/reference_depth_consistency.npz), against the NumPy restatement on seeded 290x387 bundles, through the
drop-in DepthConsistencyChecker on a NumPy scene, and run to run."""

import os

import numpy as np
import pytest

import numpy_depth_consistency as NDC
from mpsfm_amd import capi
from mpsfm_amd.sfm.mapper import DepthConsistencyChecker
from test_depth_consistency_cpu import GOLDEN, fixture_images, unpack

pytestmark = pytest.mark.gpu


def _masks_from_codes(c1, c2):
    return NDC.masks({"code": c1}, {"code": c2})


@pytest.mark.parametrize("si", [0, 1])
def test_hip_equals_reference_fixture(si):
    z = np.load(GOLDEN)
    s = float(z["thresholds"][si])
    pairs = [(int(a), int(b)) for a, b in z["pairs"]]
    ims = fixture_images(z)
    counts, summary, codes = capi.depth_consistency(ims, pairs, score_thresh=s, return_codes=True)
    assert summary["n_legs"] == 2 * len(pairs)
    for pi, (a, b) in enumerate(pairs):
        got = _masks_from_codes(*codes[pi])
        for key in NDC.MASK_KEYS:
            want = unpack(z[f"s{si}_pair{pi}_{key}"], got[key].shape)
            np.testing.assert_array_equal(got[key], want, err_msg=f"pair {(a, b)} {key}")
        for leg in range(2):
            np.testing.assert_array_equal(counts[pi, leg], NDC.counts_of(codes[pi][leg]))
    # the clamp landed in the caller's map
    idx = z["clamped0_index"]
    np.testing.assert_array_equal(ims[0]["depth"].ravel()[idx], z["clamped0_value"])
    # bundle of image 0 with references 1, 2, 3 in ONE call, counts only
    ims = fixture_images(z)
    counts, _ = capi.depth_consistency(ims, [(0, 1), (0, 2), (0, 3)], score_thresh=s)
    score, sums = NDC.bundle_score(counts)
    assert abs(score - float(z[f"s{si}_bundle_score"])) <= 1e-12
    assert tuple(sums) == tuple(int(v) for v in z[f"s{si}_bundle_sums"])


def _rot(rng, scale):
    a = rng.normal(0, scale, 3)
    th = np.linalg.norm(a)
    if th == 0:
        return np.eye(3)
    k = a / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def big_bundle(seed):
    """A query and 5 references at 290x387 and 240x320: a partially overlapping one, one pulled back (collisions), one with
    the query's exact rotation and zero variances (zero denominators: +-inf and NaN test values), two rotated ones."""
    rng = np.random.default_rng(seed)
    sizes = [(290, 387), (290, 387), (240, 320), (290, 387), (240, 320), (290, 387)]
    R0 = np.eye(3)  # exact: the query and reference 3 share it, m = (0, 0, 1) without rounding
    centres = [np.zeros(3), np.array([1.5, 0.2, 0.3]), np.array([0.2, -0.1, -9.0]), np.array([0.4, 0.0, 0.0]),
               np.array([-0.8, 0.5, 0.6]), np.array([0.3, 0.9, -0.4])]
    ims = []
    for k, ((H, W), C) in enumerate(zip(sizes, centres)):
        R = R0 if k in (0, 3) else _rot(rng, 0.15) @ R0
        C = C + (rng.normal(0, 0.05, 3) if k not in (0, 3) else 0.0)
        f = rng.uniform(450, 600)
        intr = np.array([f, f * rng.uniform(0.98, 1.02), 770 / 2 + rng.normal(0, 4), 580 / 2 + rng.normal(0, 4)])
        sx, sy = W / 770.0, H / 580.0
        Ks = np.array([[intr[0] * sx, 0, intr[2] * sx], [0, intr[1] * sy, intr[3] * sy], [0, 0, 1.0]])
        y, x = np.mgrid[0:H, 0:W]
        rays = R.T @ (np.linalg.inv(Ks) @ np.stack([x.ravel(), y.ravel(), np.ones(H * W)]))
        lam = (7.0 - C[2]) / rays[2]
        pts = C[:, None] + lam * rays
        bump = 2.0 * np.exp(-((pts[0] + 0.5) ** 2 + (pts[1] - 0.3) ** 2) / 0.8) * (k % 2)
        depth = (lam * (1 + rng.normal(0, 0.01, H * W)) - bump).reshape(H, W)
        depth[rng.uniform(size=(H, W)) < 0.002] = 0.0
        var = (rng.uniform(0.002, 0.02, (H, W)) * depth) ** 2
        if k in (0, 3):
            # same rotation, a pure x shift, zero variances: std_bar = std = 0 -> t = +-inf, and NaN where the depths are equal
            var[: H // 3] = 0.0
            depth[: H // 6] = 7.0
        if k == 4:
            var[:, : W // 4] = 0.0
        ims.append(dict(depth=depth, variance=var, prior_std_multiplier=float(rng.choice([1.0, 2.0])),
                        intr_scaled=(intr[0] * sx, intr[1] * sy, intr[2] * sx, intr[3] * sy), intr=intr,
                        cam_from_world=np.concatenate([R, (-R @ C)[:, None]], 1)))
    return ims


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_hip_equals_restatement_at_290x387(seed):
    ims = big_bundle(seed)
    pairs = [(0, r) for r in range(1, 6)]
    ref_ims = [dict(im, depth=im["depth"].copy()) for im in ims]
    counts, summary, codes = capi.depth_consistency(ims, pairs, return_codes=True)
    score_np, sums_np, counts_np, legs = NDC.bundle(ref_ims, 0, list(range(1, 6)))
    for k in range(6):
        np.testing.assert_array_equal(ims[k]["depth"], ref_ims[k]["depth"])  # the same clamp
    n_near, n_bad = 0, 0
    nonfinite, nan = 0, 0
    for p, (l12, l21) in enumerate(legs):
        for leg, L in enumerate((l12, l21)):
            diff = codes[p][leg] != L["code"]
            assert not (diff & ~L["near"]).any(), f"pair {p} leg {leg}: {np.count_nonzero(diff & ~L['near'])} pixels differ away from a boundary"
            n_bad += np.count_nonzero(diff)
            n_near += np.count_nonzero(L["near"])
            nonfinite += np.count_nonzero(L["in_canvas"] & np.isinf(L["t"]))
            nan += np.count_nonzero(L["in_canvas"] & np.isnan(L["t"]))
            if not L["near"].any():
                np.testing.assert_array_equal(counts[p, leg], counts_np[p, leg])
    total = sum(L["code"].size for l12, l21 in legs for L in (l12, l21))
    assert n_near <= 1e-4 * total, n_near
    assert nonfinite > 0 and nan > 0  # the zero-denominator cases are exercised
    assert counts[:, :, 2].sum() > 0 and counts[:, :, 3].sum() > 0
    t02 = legs[1][0]["target"]
    assert np.unique(t02[t02 >= 0]).size < 0.5 * np.count_nonzero(t02 >= 0)  # collisions in the pulled-back reference
    score, sums = NDC.bundle_score(counts)
    if n_near == 0:
        assert abs(score - score_np) <= 1e-9 and tuple(sums) == tuple(sums_np)
    print(f"seed {seed}: score {score:.6f}, near-boundary pixels {n_near}, differing {n_bad}, device {summary['ms']:.3f} ms")


def test_identical_calls_are_bit_identical():
    ims = big_bundle(7)
    pairs = [(0, r) for r in range(1, 6)]
    c1, _, k1 = capi.depth_consistency(ims, pairs, return_codes=True)
    c2, _, k2 = capi.depth_consistency(ims, pairs, return_codes=True)
    np.testing.assert_array_equal(c1, c2)
    for a, b in zip(k1, k2):
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])


# -- the drop-in checker on the NumPy scene --------------------------------------------------------------------------
def _scene():
    import types

    from mpsfm_amd.synthetic import make_scene
    from numpy_scene import scene_from_problem

    prob, truth = make_scene(6, 800, True, seed=3)
    sc = scene_from_problem(prob, truth, map_size=(129, 97), seed=3)
    psm = {imid: 1.0 + 0.5 * (k % 2) for k, imid in enumerate(sorted(sc.images))}
    for imid, im in sc.images.items():
        im.name = f"image{imid:03d}.jpg"
        im.depth.conf = types.SimpleNamespace(prior_std_multiplier=psm[imid])
    sc.camera = lambda imid: sc.rec.cameras[sc.images[imid].camera_id]
    return sc


def _entries(sc, ids):
    out = []
    for imid in ids:
        im, cam = sc.images[imid], sc.camera(imid)
        fx, fy, cx, cy = cam.params
        out.append(dict(depth=im.depth.data.copy(), variance=im.depth.uncertainty, prior_std_multiplier=im.depth.conf.prior_std_multiplier,
                        intr_scaled=(fx * cam.sx, fy * cam.sy, cx * cam.sx, cy * cam.sy), intr=cam.params,
                        cam_from_world=im.cam_from_world.matrix()))
    return out


def test_drop_in_checker_on_a_numpy_scene():
    sc = _scene()
    ids = sorted(sc.images)
    q, refs = ids[0], ids[1:]
    sc.images[q].depth.data[5:8, 10:20] = -0.5  # the clamp must land in the caller's map
    sc.images[refs[0]].depth.data[0, 0] = 0.0
    ents = _entries(sc, [q] + refs)
    score_np, sums_np, counts_np, legs = NDC.bundle(ents, 0, list(range(1, len(ids))))
    assert not any(L["near"].any() for l in legs for L in l)

    chk = DepthConsistencyChecker({}, sc, None)
    score, sums = chk.check_bundle_depth_concistency(q, {"optim_ids": set(ids)})
    assert abs(score - score_np) <= 1e-12 and tuple(sums) == tuple(sums_np)
    assert np.all(sc.images[q].depth.data[5:8, 10:20] == 0.1) and sc.images[refs[0]].depth.data[0, 0] == 0.1
    np.testing.assert_array_equal(sc.images[q].depth.data, ents[0]["depth"])

    m = chk.check_depth_consistency(q, refs[1])
    want = NDC.masks(*legs[1])
    assert list(m) == NDC.MASK_KEYS
    for key in NDC.MASK_KEYS:
        np.testing.assert_array_equal(m[key], want[key], err_msg=key)

    # check_image: the decision and the counters follow the score against depth_cons_thresh
    chk.depth_cons_thresh = score_np * 0.5 if score_np > 0 else -1.0
    assert chk.check_image(q, {"optim_ids": set(ids)}) is False
    assert chk.reg_batch_dc_times_failed == 1 and sc.images[q].failed_dc_check is True
    chk.depth_cons_thresh = score_np * 2 + 1e-3
    assert chk.check_image(q, {"optim_ids": set(ids)}) is True
    assert chk.reg_batch_dc_times_failed == 1
    chk.relax_thresholds()
    assert chk.reg_batch_dc_times_failed == 0 and chk.cons_thresh_times_increased == 1
    # init_pair: score of the pair (query = first of the set) at init_valid_thresh against init_depth_cons_thresh
    pair = [q, refs[0]]
    first = list(set(pair))[0]
    other = pair[1] if first == pair[0] else pair[0]
    ents3 = _entries(sc, [first, other])
    s3, _, _, _ = NDC.bundle(ents3, 0, [1], s=chk.conf.init_valid_thresh)
    assert chk.init_pair(set(pair)) == (s3 <= chk.conf.init_depth_cons_thresh)
