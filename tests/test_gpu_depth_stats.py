"""mpsfm_depth_stats on the device: the selection alone (bitwise against np.partition on the call's own per-observation outputs),
the arithmetic against the NumPy restatement (tests/numpy_depth_stats.py), Optimizer(stats="device") against stats="host" end to
end, the refusals, and the wall time of both paths."""

import ctypes as C
import time

import numpy as np
import pytest

import numpy_depth_stats as N
from mpsfm_amd import capi
from mpsfm_amd.capi import SEL_FIT, SEL_SIGMA, SEL_VALID, STATS_EMPTY, STATS_EMPTY_METRIC, STATS_FIT, STATS_SIGMA
from mpsfm_amd.sfm.mapper.bundle_adjustment import Optimizer
from mpsfm_amd.sfm.scene.prior_gather import gather_bundle
from mpsfm_amd.synthetic import make_scene
from numpy_scene import scene_from_problem

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 3, 255, 256, 257, 2048, 2049]  # around the workgroup size and the LDS capacity of the per-image select
KINDS = ["runs", "lowbyte", "mixed", "zeros"]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b, zero_sign_open=False):
    """Bitwise equal (NaN equals NaN).  zero_sign_open: a zero may differ in sign — among zeros of both signs, which compare equal,
    np.partition leaves open which of them lands on a rank."""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    return bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b)) | (zero_sign_open & (a == 0) & (b == 0))))


def both_zeros(values):
    zero = values[values == 0]
    return bool(len(zero) and np.signbit(zero).any() and not np.signbit(zero).all())


def content(kind, n, rng):
    """(z, var, keep) of n observations.  With the one-pixel-exact maps below d = 1, so r = max(z, 1e-6) and
    w = -log(z) / max(sqrt(var), 1e-6): z = 0 / inf / a negative number / NaN give w = +inf / -inf / NaN / NaN, var = inf gives a
    signed zero; keep = 0 puts the keypoint on the invalid pixel."""
    var, keep = np.full(n, 0.25), np.ones(n, bool)
    if n == 0:
        return np.zeros(0), var, keep
    if kind == "runs":  # runs of equal values that straddle the middle, neighbours one ulp apart on either side
        z = rng.choice([0.5, 2.0, 3.0, np.nextafter(3.0, 4.0), np.nextafter(3.0, 2.0), 7.0], n, p=[0.1, 0.15, 0.4, 0.1, 0.1, 0.15])
    elif kind == "lowbyte":  # values that differ only in the lowest byte
        z = (np.float64(3.0).view(np.uint64) + rng.integers(0, 256, n).astype(np.uint64)).view(np.float64)
        var[:] = 1.0
    elif kind == "mixed":
        z = np.exp(rng.normal(0, 1.5, n))  # w of both signs
        for k, special in enumerate([0.0, np.inf, -2.0, np.nan, 1.0, 1e-9, 1e300]):
            z[rng.integers(0, n, max(n // 40, 1 if n > 2 * k else 0))] = special
        keep = rng.uniform(size=n) > 0.1
    else:  # "zeros": a run of w = +0 (z = 1) across the middle between negative and positive w; in the longer segments also
        z = rng.choice([0.25, 1.0, 4.0], n, p=[0.3, 0.4, 0.3])  # a few -0 (z = 4, var = inf) and +0 from a division by infinity
        if n > 16:
            var[np.flatnonzero(z == 4.0)[:2]] = np.inf
            var[np.flatnonzero(z == 0.25)[:3]] = np.inf
    return z, var, keep


def run_segments(segments, what=STATS_FIT | STATS_SIGMA, filt=0):
    """One call over images whose observations are the given (z, var, keep): maps of ones, validity 0 at pixel (3, 3), identity
    poses, so that d = 1 and the camera-frame depth is the point's own z.  5x5 maps at scale 1: grid_sample's coordinate arithmetic
    is exact for the keypoints (1, 1) and (3, 3), so v is exactly 1 or exactly 0."""
    n_img = len(segments)
    valid = np.ones((5, 5))
    valid[3, 3] = 0
    z = np.concatenate([s[0] for s in segments]) if segments else np.zeros(0)
    var = np.concatenate([s[1] for s in segments]) if segments else np.zeros(0)
    keep = np.concatenate([s[2] for s in segments]) if segments else np.zeros(0, bool)
    n = len(z)
    xy = np.where(keep[:, None], 1.0, 3.0) * np.ones((n, 2))
    pts = np.stack([np.zeros(n), np.zeros(n), z], 1)
    kw = dict(depth_maps=[np.ones((5, 5))] * n_img, valid_maps=[valid] * n_img, sx=np.ones(n_img), sy=np.ones(n_img),
              cam_quat=np.tile([0, 0, 0, 1.0], (n_img, 1)), cam_t=np.zeros((n_img, 3)),
              obs_img=np.repeat(np.arange(n_img), [len(s[0]) for s in segments]).astype(np.int32), obs_xy=xy, obs_var=var,
              obs_pt=np.arange(n, dtype=np.int32), pts=pts, what=what, filter=np.full(n_img, filt, np.uint8), per_obs=True)
    return kw, capi.depth_stats(**kw)


def check_selection(kw, out):
    """Every order statistic and count of `out` against np.partition on the call's own ratio / whitened / selected."""
    obs_img, sel = kw["obs_img"], out["selected"]
    if kw["what"] & STATS_FIT:
        for k in range(len(kw["depth_maps"])):
            seg = obs_img == k
            r = out["ratio"][seg][(sel[seg] & SEL_FIT) != 0]
            ranked = r[~np.isnan(r)]
            assert out["n_valid"][k] == ((sel[seg] & SEL_VALID) != 0).sum() and out["n_sel"][k] == len(r), k
            assert out["n_nan"][k] == len(r) - len(ranked), k
            empty = len(r) == 0 and ("mode" not in kw or kw["mode"][k] == 1)  # a skipped image has no flags
            assert out["flags"][k] == (STATS_EMPTY | (STATS_EMPTY_METRIC if kw["filter"][k] == 2 else 0) if empty else 0), k
            lo, hi = N.two_middle(ranked) if len(ranked) else (np.nan, np.nan)
            assert same_bits(out["ratio_lo"][k], lo) and same_bits(out["ratio_hi"][k], hi), (k, seg.sum(), out["ratio_lo"][k], lo, out["ratio_hi"][k], hi)
    if kw["what"] & STATS_SIGMA:
        w = out["whitened"][(sel & SEL_SIGMA) != 0]
        ranked = w[~np.isnan(w)]
        assert out["sigma_n_sel"] == len(w) and out["sigma_n_nan"] == len(w) - len(ranked)
        mu = mad = np.nan
        if len(ranked):
            with np.errstate(invalid="ignore"):
                mu = 0.5 * np.add(*N.two_middle(ranked))
                dev = np.abs(ranked - mu)
                mad = np.nan if np.isnan(dev).any() else 0.5 * np.add(*N.two_middle(dev))
        assert same_bits(out["mu"], mu, both_zeros(ranked)) and same_bits(out["mad"], mad), (len(ranked), out["mu"], mu, out["mad"], mad)
        return mu, mad


def same_bytes(a, b):
    assert a.keys() == b.keys()
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


# ---- selection alone --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_per_image_medians_are_bitwise_np_partition_at_every_segment_length(kind):
    rng = np.random.default_rng(KINDS.index(kind))
    segments = [content(kind, n, rng) for n in LENGTHS for _ in range(2)]
    kw, out = run_segments(segments)
    check_selection(kw, out)
    assert same_bytes(out, capi.depth_stats(**kw))  # two calls, identical bytes
    w = out["whitened"][(out["selected"] & SEL_SIGMA) != 0]
    if kind == "runs":  # the middle of a long segment lies inside a run, and the run has neighbours one ulp away
        k = 2 * LENGTHS.index(2049)
        assert out["ratio_lo"][k] == out["ratio_hi"][k] == 3.0 and np.nextafter(3.0, 4.0) in out["ratio"]
    if kind == "lowbyte":
        assert len(np.unique(bits(out["ratio"]) >> np.uint64(8))) == 1 and len(np.unique(bits(w) >> np.uint64(8))) < len(np.unique(bits(w))) // 4
    if kind == "mixed":
        assert np.isposinf(w).any() and np.isneginf(w).any() and np.isnan(w).any() and (w < 0).any() and (w > 0).any()
        assert out["n_nan"].sum() > 0 and (out["n_sel"] < out["n_valid"]).sum() == 0 and (out["n_valid"] < np.array([len(s[0]) for s in segments]))[8:].all()
        assert (out["ratio"] == 1e-6).sum() > 10  # z <= 0 is clipped: a run at the lower end
    if kind == "zeros":
        assert (bits(w) == bits(np.array([-0.0]))[0]).sum() >= 10 and (bits(w) == 0).sum() > 100 and out["mu"] == 0.0


@pytest.mark.parametrize("kind, n", [("mixed", 70001), ("runs", 70000), ("lowbyte", 69999), ("zeros", 70002)])
def test_whole_scene_medians_over_many_workgroups_are_bitwise_np_partition(kind, n):
    """One segment of about 70 000 observations: 35 workgroups of k_ds_scene_hist share it, and the per-image select reads it from
    memory, not from LDS."""
    rng = np.random.default_rng(100 + n)
    kw, out = run_segments([content(kind, n, rng)])
    mu, mad = check_selection(kw, out)
    assert same_bytes(out, capi.depth_stats(**kw))
    assert out["sigma_n_sel"] > 60000 and np.isfinite(mu) and np.isfinite(mad)
    if kind == "mixed":
        assert out["sigma_n_nan"] > 1000 and mad > 0 and (out["whitened"] < 0).sum() > 20000
    # several images share the scene segment too, and FIT / SIGMA alone give what both together give
    parts = [content(kind, m, rng) for m in (30000, 0, 25000, 17)]
    kw, both = run_segments(parts)
    check_selection(kw, both)
    for what in (STATS_FIT, STATS_SIGMA):
        kw1, one = run_segments(parts, what=what)
        check_selection(kw1, one)
        assert all(np.asarray(one[k]).tobytes() == np.asarray(both[k]).tobytes() for k in one if k not in ("ratio", "whitened", "selected"))


def test_small_empty_and_degenerate_scene_segments():
    rng = np.random.default_rng(5)
    for zs in ([2.0], [2.0, 5.0], [7.0, 2.0, 5.0], [2.0, 2.0, 2.0, 2.0], [0.5, 2.0, np.nan, 3.0]):
        kw, out = run_segments([(np.array(zs), np.full(len(zs), 0.25), np.ones(len(zs), bool))])
        check_selection(kw, out)
    # nothing selected: counts 0, NaN medians, the EMPTY flags (with and without the metric filter)
    for filt in (0, 2):
        near_one = (rng.choice([0.9, 1.1, 1.2], 300), np.full(300, 0.25), np.ones(300, bool))  # passes the metric filter at scales of 1
        kw, out = run_segments([(np.array([2.0, 3.0]), np.full(2, 0.25), np.zeros(2, bool)), near_one], filt=filt)
        check_selection(kw, out)
        assert out["n_sel"][0] == 0 and out["flags"][0] == (STATS_EMPTY | (STATS_EMPTY_METRIC if filt == 2 else 0)) and out["flags"][1] == 0
        assert np.isnan(out["ratio_lo"][0]) and out["n_sel"][1] == 300
    kw, out = run_segments([(np.array([2.0, 3.0]), np.full(2, 0.25), np.zeros(2, bool))])
    assert out["sigma_n_sel"] == 0 and np.isnan(out["mu"]) and np.isnan(out["mad"])
    # a median at infinity: |w - mu| holds NaNs, and np.median answers NaN
    z = np.array([0.0] * 5 + [2.0, 3.0])
    kw, out = run_segments([(z, np.full(7, 0.25), np.ones(7, bool))])
    mu, mad = check_selection(kw, out)
    assert np.isposinf(mu) and np.isnan(mad) and out["sigma_n_nan"] == 0
    # mode 0: the image is skipped
    kw, _ = run_segments([content("runs", 100, rng), content("runs", 100, rng)])
    out = capi.depth_stats(**{**kw, "mode": [0, 1]})
    assert out["n_valid"][0] == out["n_sel"][0] == 0 and out["flags"][0] == 0 and np.isnan(out["ratio_lo"][0]) and out["n_sel"][1] == 100
    assert not (out["selected"][:100] & (SEL_VALID | SEL_FIT)).any() and (out["selected"][:100] & SEL_SIGMA).all()


# ---- arithmetic ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def modified_scene():
    """The scene of test_gather_kernel_matches_numpy_restatement (tests/test_gpu_prior.py): maps of unequal size, non-positive depths,
    keypoints off the map — in the prior and in the integrated map alike — and priors at scales of their own."""
    prob, truth = make_scene(9, 2500, True, seed=61)
    sc = scene_from_problem(prob, truth, seed=6)
    rng = np.random.default_rng(1)
    ids = sorted(sc.images)
    d = sc.images[ids[2]].depth
    d.data, d.data_prior, d.valid = d.data[:-7, :-5].copy(), d.data_prior[:-7, :-5].copy(), d.valid[:-7, :-5].copy()
    sc.images[ids[3]].depth.data[::6, ::4] = -1.0
    sc.images[ids[3]].depth.data_prior[::6, ::4] = -1.0
    sc.images[ids[4]].kps[::9] += rng.uniform(-900, 900, sc.images[ids[4]].kps[::9].shape)
    for k, imid in enumerate(ids):
        s = 1.0 + 0.01 * k
        d = sc.images[imid].depth
        d.data_prior, d.scale = d.data_prior / s, 1.0 / s
    return sc, ids, prob


def test_kernel_matches_the_numpy_restatement(modified_scene):
    sc, ids, prob = modified_scene
    results = {}
    for depth_type, what in (("prior", STATS_FIT), ("update", STATS_SIGMA), ("update", STATS_FIT | STATS_SIGMA)):
        g = gather_bundle(sc, ids, depth_type)
        assert g["obs_img"].max() == len(ids) - 1 and len(g["obs_img"]) == prob.n_obs and np.all(np.diff(g["obs_img"]) >= 0)
        scales = np.array([sc.images[i].depth.scale for i in ids])
        map_scale = np.array([np.mean(np.delete(scales, k)) for k in range(len(ids))])
        map_scale[7] *= 40.0  # the metric filter empties this image ...
        map_scale[[2, 4]] *= 1.52  # ... and has something to decide in these: div lies around its upper bound 1.5
        kw = dict(depth_maps=g["depth_maps"], valid_maps=g["valid_maps"], sx=g["sx"], sy=g["sy"], cam_quat=g["cam_quat"], cam_t=g["cam_t"],
                  obs_img=g["obs_img"], obs_xy=g["obs_xy"], obs_var=g["obs_var"], obs_pt=g["obs_pt"], pts=sc.point3D_coordinates(g["point_ids"]),
                  what=what, mode=[1, 1, 1, 1, 1, 0, 1, 1, 1], filter=[0, 1, 2, 1, 2, 1, 0, 2, 1], im_scale=scales, map_scale=map_scale,
                  scale_filter_factor=1.07, per_obs=True)
        margins = []
        hip, ref = capi.depth_stats(**kw), N.depth_stats(margins=margins, **kw)
        # the condition of the exact comparisons, on the restatement itself: no filtered div within 1e-9 of a threshold
        if what & STATS_FIT:
            assert len(margins) > 1000 and min(margins) > 1e-9
        np.testing.assert_array_equal(hip["selected"], ref["selected"])
        assert len(np.unique(hip["selected"])) >= {STATS_FIT: 3, STATS_SIGMA: 2, STATS_FIT | STATS_SIGMA: 5}[what]
        if what & STATS_FIT:
            for k in ("n_valid", "n_sel", "n_nan", "flags"):
                np.testing.assert_array_equal(hip[k], ref[k], err_msg=k)
            assert hip["flags"][7] == STATS_EMPTY | STATS_EMPTY_METRIC and hip["flags"][5] == 0 and hip["n_valid"][5] == 0
            fitted = hip["n_sel"] > 0
            cut = hip["n_sel"] < hip["n_valid"]
            assert fitted.sum() == 7 and cut[[1, 3, 8]].any() and cut[[2, 4]].any() and not cut[[0, 6]].any()  # each filter decides
            print("per image n_valid / n_sel:", hip["n_valid"].tolist(), hip["n_sel"].tolist())
            for k in ("ratio_lo", "ratio_hi"):
                print(k, "max relative difference", np.max(np.abs(hip[k][fitted] / ref[k][fitted] - 1)))
                np.testing.assert_allclose(hip[k][fitted], ref[k][fitted], rtol=1e-12)
                assert np.isnan(hip[k][~fitted]).all()
            on = (hip["selected"] & SEL_FIT) != 0
            np.testing.assert_allclose(hip["ratio"][on], ref["ratio"][on], rtol=1e-12)
        if what & STATS_SIGMA:
            assert hip["sigma_n_sel"] == ref["sigma_n_sel"] > 10000 and hip["sigma_n_nan"] == ref["sigma_n_nan"]
            print(f"mu {hip['mu']!r} against {ref['mu']!r}, mad {hip['mad']!r} against {ref['mad']!r}")
            assert hip["mu"] == pytest.approx(ref["mu"], rel=1e-12) and hip["mad"] == pytest.approx(ref["mad"], rel=1e-12)
            results[what] = (hip["mu"], hip["mad"])
        check_selection(kw, hip)
    assert results[STATS_SIGMA] == results[STATS_FIT | STATS_SIGMA]


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_optimizer_with_device_stats_equals_host_stats(modified_scene):
    sc, ids, _ = modified_scene
    glob, loc = {"optim_ids": ids}, {"optim_ids": ids[:5], "ref_id": ids[1]}
    cases = [({}, glob, {}), ({}, glob, {"allow_scale_filter": True}), ({"scale_filter_factor": 1.05}, glob, {"allow_scale_filter": True}),
             ({}, loc, {}), ({}, loc, {"allow_metric_scale_filter": True}), ({"single_rescale": False}, loc, {"allow_metric_scale_filter": True}),
             ({"single_rescale": False}, loc, {"allow_scale_filter": True}), ({"metric_scale_filter": False}, loc, {"allow_scale_filter": True})]
    for conf, bundle, kw in cases:
        host, dev = Optimizer(conf, sc, None), Optimizer(conf, sc, None, stats="device")
        want, ok_w = host.optimize_prior_shiftscale(bundle, **kw)
        got, ok_g = dev.optimize_prior_shiftscale(bundle, **kw)
        assert ok_w and ok_g and list(got) == list(want) and len(want) >= 1, (conf, kw)
        for imid in want:
            assert got[imid][0] == want[imid][0] == 0.0 and got[imid][1] == pytest.approx(want[imid][1], rel=1e-12), (conf, kw, imid)
    # the early return: the metric filter empties the third image of the walk
    d = sc.images[ids[2]].depth
    keep = d.data_prior
    d.data_prior = keep * 40.0
    try:
        conf, bundle = {"single_rescale": False}, {"optim_ids": ids[:5], "ref_id": ids[2]}
        want, _ = Optimizer(conf, sc, None).optimize_prior_shiftscale(bundle, allow_metric_scale_filter=True)
        got, _ = Optimizer(conf, sc, None, stats="device").optimize_prior_shiftscale(bundle, allow_metric_scale_filter=True)
        assert list(want) == ids[:3] == list(got)
        for imid in want:
            assert got[imid][1] == pytest.approx(want[imid][1], rel=1e-12)
    finally:
        d.data_prior = keep
    host, dev = Optimizer({}, sc, None), Optimizer({}, sc, None, stats="device")
    host.update_truncation_multiplier(ids)
    dev.update_truncation_multiplier(ids)
    print(f"truncation multiplier: host {host.truncation_multiplier!r}, device {dev.truncation_multiplier!r}")
    assert dev.truncation_multiplier == pytest.approx(host.truncation_multiplier, rel=1e-12)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_empty_call():
    rng = np.random.default_rng(9)
    kw, _ = run_segments([content("runs", 40, rng), content("runs", 40, rng)])
    swapped = kw["obs_img"].copy()
    swapped[[39, 40]] = swapped[[40, 39]]
    with pytest.raises(capi.MpsfmHipError) as e:
        capi.depth_stats(**{**kw, "obs_img": swapped})
    assert e.value.code == -1 and "obs_img" in str(e.value)  # MPSFM_EINVAL
    with pytest.raises(capi.MpsfmHipError) as e:
        capi.depth_stats(**{**kw, "what": 0})
    assert e.value.code == -1
    # NULL outputs, through the C entry point itself
    G, _keep, n_img, n = capi._depth_gather(*[kw[k] for k in ("depth_maps", "valid_maps", "sx", "sy", "cam_quat", "cam_t", "obs_img", "obs_xy",
                                                               "obs_var", "obs_pt", "pts")], 1.5, 1.0)
    mode, filt, one = np.ones(n_img, np.uint8), np.zeros(n_img, np.uint8), np.ones(n_img)
    counts, ratio, flags, sc, ss = np.zeros((n_img, 3), np.int64), np.zeros((n_img, 2)), np.zeros(n_img, np.uint32), np.zeros(2, np.int64), np.zeros(2)
    outs = [counts.ctypes.data, ratio.ctypes.data, flags.ctypes.data, sc.ctypes.data, ss.ctypes.data]
    call = lambda what, o: capi.lib().mpsfm_depth_stats(C.byref(G), what, mode.ctypes.data, filt.ctypes.data, one.ctypes.data,  # noqa: E731
                                                        one.ctypes.data, 0, *o, None, None, None)
    assert call(3, outs) == 0 and counts[:, 1].tolist() == [40, 40]
    for k in range(5):
        assert call(3, outs[:k] + [None] + outs[k + 1:]) == -1, k
    assert call(STATS_SIGMA, [None, None, None] + outs[3:]) == 0 and call(STATS_FIT, outs[:3] + [None, None]) == 0  # the other part's are not needed
    # no observation: 0, with empty results
    kw0, out = run_segments([(np.zeros(0), np.zeros(0), np.zeros(0, bool))] * 2)
    assert out["n_valid"].tolist() == out["n_sel"].tolist() == [0, 0] and out["flags"].tolist() == [STATS_EMPTY] * 2
    assert np.isnan(out["ratio_lo"]).all() and out["sigma_n_sel"] == 0 and np.isnan(out["mu"]) and np.isnan(out["mad"]) and len(out["ratio"]) == 0


# ---- wall time ----------------------------------------------------------------------------------------------------------------------
def test_wall_time_of_both_paths_on_40_cameras_and_30k_landmarks():
    """No pass mark: prints the wall time of optimize_prior_shiftscale and update_truncation_multiplier with stats="host" and
    stats="device" (DESIGN.md section 4y records the numbers)."""
    prob, truth = make_scene(40, 30000, True, seed=5)
    sc = scene_from_problem(prob, truth, seed=1)
    ids = sorted(sc.images)
    bundle = {"optim_ids": set(ids), "pts3D": set(sc.points3D), "constpoints": set()}
    res = {}
    for stats in ("host", "device"):
        opt = Optimizer({}, sc, None, stats=stats)
        for name, fn in (("optimize_prior_shiftscale", lambda: opt.optimize_prior_shiftscale(bundle, allow_scale_filter=True)),
                         ("update_truncation_multiplier", lambda: opt.update_truncation_multiplier(ids))):
            fn()  # warm-up (allocator cache, code objects)
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                r = fn()
                ts.append(1e3 * (time.perf_counter() - t0))
            res[(stats, name)] = (min(ts), r[0] if r is not None else opt.truncation_multiplier)
            print(f"{name} stats={stats}: {min(ts):.2f} ms wall ({prob.n_obs} observations, 40 cameras / 30 k landmarks)")
    a, b = res[("host", "optimize_prior_shiftscale")][1], res[("device", "optimize_prior_shiftscale")][1]
    assert list(a) == list(b) and all(b[i][1] == pytest.approx(a[i][1], rel=1e-12) for i in a)
    assert res[("device", "update_truncation_multiplier")][1] == pytest.approx(res[("host", "update_truncation_multiplier")][1], rel=1e-12)
