"""CPU tests around mpsfm_depth_stats: its NumPy restatement (tests/numpy_depth_stats.py) against the Optimizer's host paths,
the host logic of Optimizer(stats="device") over that restatement, the scene bookkeeping of the package (depth_utils,
normalization) and a replay of one global-refinement iteration (reference mapper/base.py:476-514) with package code only."""

import copy

import numpy as np
import pytest

import numpy_depth_stats as N
from backends import OracleBackend
from mapper_replay import MapperReplay
from mpsfm_amd.sfm.mapper.bundle_adjustment import Optimizer
from mpsfm_amd.sfm.scene.depth_utils import DepthUtils
from mpsfm_amd.sfm.scene.normalization import bounding_box_and_centroid, normalize, normalize_scene
from mpsfm_amd.sfm.scene.observations import HipObservationManager
from mpsfm_amd.synthetic import make_scene
from numpy_scene import NumpyReconstruction, ObservationManager, scene_from_problem
from oracle import cpu_oracle as O


class StatsOracleBackend(OracleBackend):
    """The oracle backend with the restatement of mpsfm_depth_stats."""

    def __init__(self):
        self.stats_calls = 0

    def depth_stats(self, **kw):
        self.stats_calls += 1
        self.last_kw, self.last = kw, N.depth_stats(**kw)
        return self.last


class PackageScene(DepthUtils, NumpyReconstruction):
    """The NumPy scene with the package's depth bookkeeping in front of the stand-in's."""


def _scene(seed=21, n_cams=7, n_pts=350, scales=True):
    prob, truth = make_scene(n_cams, n_pts, True, seed=seed)
    sc = scene_from_problem(prob, truth, map_size=(64, 48), seed=seed + 1)
    if scales:  # priors at scales of their own: the metric-scale filter has something to decide
        for k, imid in enumerate(sorted(sc.images)):
            s = 1.0 + 0.07 * k
            d = sc.images[imid].depth
            d.data_prior, d.data, d.scale = d.data_prior / s, d.data / s, 1.0 / s
        sc.images[sorted(sc.images)[1]].depth.scale *= 0.62  # the proposed scales of this image lie around the filter's bound
    return sc


def _bundles(sc):
    ids = sorted(sc.images)
    return {"global": {"optim_ids": set(ids)}, "local": {"optim_ids": set(ids[:4]), "ref_id": ids[1]}}


def _assert_same_shiftscale(got, want, rel=1e-12):
    assert list(got) == list(want)
    for imid in want:
        assert got[imid][0] == want[imid][0] == 0.0
        assert got[imid][1] == pytest.approx(want[imid][1], rel=rel, nan_ok=True)


CASES = [  # conf, which bundle, keyword arguments, the filter of the fitted images (0 none, 1 scale, 2 metric scale)
    ({}, "global", {}, 0),
    ({}, "global", {"allow_scale_filter": True}, 1),
    ({"scale_filter_factor": 1.02}, "global", {"allow_scale_filter": True}, 1),
    ({}, "local", {}, 0),
    ({}, "local", {"allow_metric_scale_filter": True}, 2),
    ({}, "local", {"allow_scale_filter": True, "allow_metric_scale_filter": True}, 2),
    ({"single_rescale": False}, "local", {"allow_metric_scale_filter": True}, 2),
    ({"single_rescale": False}, "local", {"allow_scale_filter": True}, 1),
    ({"metric_scale_filter": False}, "local", {"allow_metric_scale_filter": True, "allow_scale_filter": True}, 0),
    ({"scale_filter": False}, "global", {"allow_scale_filter": True}, 0),
]


@pytest.mark.parametrize("conf, which, kw, filt", CASES)
def test_restatement_and_device_logic_equal_the_host_path(conf, which, kw, filt):
    sc = _scene()
    bundle = _bundles(sc)[which]
    host = Optimizer(conf, sc, None, backend=OracleBackend())
    want, ok = host._build_shiftscale_problem(bundle, **kw)
    assert ok and len(want) >= 1
    got, ok = N.shiftscale(sc, host.conf, bundle, **kw)
    assert ok
    _assert_same_shiftscale(got, want, rel=0)  # the same operations on the same arrays
    backend = StatsOracleBackend()
    dev = Optimizer(conf, sc, None, backend=backend, stats="device")
    got, ok = dev._build_shiftscale_problem(bundle, **kw)
    assert ok and backend.stats_calls == 1
    _assert_same_shiftscale(got, want)
    assert set(backend.last_kw["filter"]) == {filt} and len(backend.last_kw["filter"]) == len(want)
    n_valid, n_sel = backend.last["n_valid"], backend.last["n_sel"]
    if filt:  # the filter decides: some image loses observations to it, none loses all
        assert (n_sel < n_valid).any() and (n_sel > 0).all(), (n_valid, n_sel)
    else:
        np.testing.assert_array_equal(n_sel, n_valid)
    a, _ = host.optimize_prior_shiftscale(bundle, **kw)
    b, _ = dev.optimize_prior_shiftscale(bundle, **kw)
    assert list(a) == list(b) and all(b[i][1] == pytest.approx(a[i][1], rel=1e-12) for i in a)


def test_the_metric_filter_that_empties_an_image_returns_early_with_the_map_scale():
    sc = _scene()
    ids = sorted(sc.images)
    bundle = {"optim_ids": ids[:5], "ref_id": ids[2]}  # a list: the walk has an order to stop in
    conf = {"single_rescale": False}
    d = sc.images[ids[2]].depth
    d.data_prior = d.data_prior * 40.0  # every proposed scale of the third image is off by 40
    host = Optimizer(conf, sc, None, backend=OracleBackend())
    want, _ = host._build_shiftscale_problem(bundle, allow_metric_scale_filter=True)
    assert list(want) == ids[:3]  # the entries so far plus the emptied image
    map_scale = np.mean([sc.images[i].depth.scale for i in ids[:5] if i != ids[2]])
    assert want[ids[2]][1] == np.log(map_scale / d.scale)
    got, _ = N.shiftscale(sc, host.conf, bundle, allow_metric_scale_filter=True)
    _assert_same_shiftscale(got, want, rel=0)
    dev = Optimizer(conf, sc, None, backend=StatsOracleBackend(), stats="device")
    got, _ = dev._build_shiftscale_problem(bundle, allow_metric_scale_filter=True)
    _assert_same_shiftscale(got, want)
    assert got[ids[2]][1] == want[ids[2]][1]


def test_an_image_without_observations_or_activation_is_fitted_like_on_the_host():
    sc = _scene()
    ids = sorted(sc.images)
    sc.images[ids[1]].depth.reset()  # not activated: post_registration_refinement fits such an image
    sc.images[ids[1]].depth.data = None
    sc.images[ids[3]].kp_point3D[:] = np.iinfo(np.uint64).max  # no observation: np.median of nothing
    bundle = {"optim_ids": ids}
    with np.errstate(all="ignore"), pytest.warns(RuntimeWarning):
        want, _ = Optimizer({}, sc, None, backend=OracleBackend())._build_shiftscale_problem(bundle, allow_scale_filter=True)
    got, _ = Optimizer({}, sc, None, backend=StatsOracleBackend(), stats="device")._build_shiftscale_problem(bundle, allow_scale_filter=True)
    assert np.isnan(want[ids[3]][1]) and np.isfinite(want[ids[1]][1])
    _assert_same_shiftscale(got, want)


def test_truncation_sigma_restatement_and_device_logic_equal_the_host_path():
    sc = _scene(seed=23, scales=False)
    ids = sorted(sc.images)
    sc.images[ids[2]].depth.data[::5, ::3] = -1.0
    host = Optimizer({}, sc, None, backend=OracleBackend())
    host.update_truncation_multiplier(ids)
    assert N.truncation_sigma(sc, ids) == pytest.approx(host.truncation_multiplier, rel=1e-12)
    backend = StatsOracleBackend()
    dev = Optimizer({}, sc, None, backend=backend, stats="device")
    dev.update_truncation_multiplier(ids)
    assert backend.stats_calls == 1 and dev.truncation_multiplier == pytest.approx(host.truncation_multiplier, rel=1e-12)
    floor = Optimizer({"min_truncation_mult": 50.0}, sc, None, backend=StatsOracleBackend(), stats="device")
    floor.update_truncation_multiplier(ids)
    assert floor.truncation_multiplier == 50.0
    with pytest.raises(ValueError):
        Optimizer({}, sc, None, backend=OracleBackend(), stats="gpu")


def test_restatement_counts_nans_apart_and_refuses_a_decreasing_obs_img():
    maps, valid = [np.full((4, 4), 2.0)], [np.ones((4, 4))]
    kw = dict(depth_maps=maps, valid_maps=valid, sx=[1.0], sy=[1.0], cam_quat=[[0, 0, 0, 1.0]], cam_t=[[0, 0, 0.0]],
              obs_img=np.zeros(5, np.int32), obs_xy=np.ones((5, 2)), obs_var=np.full(5, 0.01), obs_pt=np.arange(5), per_obs=True,
              pts=np.array([[0, 0, 4.0], [0, 0, 8.0], [0, 0, np.nan], [0, 0, -1.0], [0, 0, 16.0]]))
    out = N.depth_stats(**kw)
    assert (out["n_valid"][0], out["n_sel"][0], out["n_nan"][0]) == (5, 5, 1)
    assert (out["ratio_lo"][0], out["ratio_hi"][0]) == (2.0, 4.0)  # of 1e-6, 2, 4, 8
    assert out["sigma_n_sel"] == 5 and out["sigma_n_nan"] == 2  # log of a NaN and of -1
    with pytest.raises(ValueError):
        N.depth_stats(**{**kw, "depth_maps": maps * 2, "valid_maps": valid * 2, "sx": [1, 1], "sy": [1, 1], "cam_quat": [[0, 0, 0, 1.0]] * 2,
                         "cam_t": [[0, 0, 0.0]] * 2, "obs_img": [0, 1, 0, 1, 1]})


def test_the_entry_point_refuses_bad_arguments_before_it_looks_for_a_device():
    from mpsfm_amd import capi

    kw = dict(depth_maps=[np.ones((5, 5))] * 2, valid_maps=[np.ones((5, 5))] * 2, sx=[1.0, 1.0], sy=[1.0, 1.0], cam_quat=[[0, 0, 0, 1.0]] * 2,
              cam_t=np.zeros((2, 3)), obs_img=[0, 1, 0], obs_xy=np.ones((3, 2)), obs_var=np.ones(3), obs_pt=[0, 0, 0], pts=[[0, 0, 2.0]])
    for bad in ({}, {"obs_img": [0, 0, 1], "what": 0}, {"obs_img": [0, 0, 1], "what": 4}, {"obs_img": [0, 0, 2]}, {"obs_img": [0, 0, 1], "mode": [2, 1]},
                {"obs_img": [0, 0, 1], "filter": [0, 3]}, {"obs_img": [0, 0, 1], "scale_filter_factor": 0.0}):
        with pytest.raises(capi.MpsfmHipError) as e:
            capi.depth_stats(**{**kw, **bad})
        assert e.value.code == -1, (bad, str(e.value))  # MPSFM_EINVAL, not MPSFM_ENODEVICE
    with pytest.raises(capi.MpsfmHipError) as e:
        capi.depth_stats(**kw)
    assert "obs_img must not decrease" in str(e.value)
    # no observation: answered on the host, with empty results
    out = capi.depth_stats(**{**kw, "obs_img": [], "obs_xy": np.zeros((0, 2)), "obs_var": [], "obs_pt": [], "filter": [0, 2], "mode": [1, 1]})
    assert out["n_sel"].tolist() == [0, 0] and out["flags"].tolist() == [capi.STATS_EMPTY, capi.STATS_EMPTY | capi.STATS_EMPTY_METRIC]
    assert np.isnan(out["ratio_lo"]).all() and out["sigma_n_sel"] == 0 and np.isnan(out["mu"]) and np.isnan(out["mad"])


# ---- depth bookkeeping ---------------------------------------------------------------------------------------------------------
def _depth_state(sc):
    return {i: {k: copy.deepcopy(getattr(im.depth, k)) for k in ("data", "data_prior", "uncertainty", "uncertainty_update", "scale", "shift", "activated")}
            for i, im in sc.images.items()}


def _assert_same_depths(a, b):
    for i in a:
        for k, v in a[i].items():
            if v is None or b[i][k] is None:
                assert v is None and b[i][k] is None, (i, k)
            else:
                np.testing.assert_array_equal(v, b[i][k], err_msg=f"image {i} {k}")


def test_depth_utils_equal_the_stand_in_and_keep_the_references_quirk():
    a = _scene(seed=25)
    b = copy.deepcopy(a)
    b.__class__ = PackageScene
    ids = sorted(a.images)
    for sc in (a, b):
        sc.images[ids[0]].depth.reset()
        sc.images[ids[4]].depth.reset()
    shift_scales = {ids[0]: (0.0, 1.3), ids[2]: (0.25, 0.8), ids[5]: (0.0, 1.0)}
    for sc in (a, b):
        sc.rescale_all(shift_scales)
        sc.activate_depths([ids[0], ids[2]])
    assert type(b).rescale_all is DepthUtils.rescale_all and type(a).rescale_all is NumpyReconstruction.rescale_all
    _assert_same_depths(_depth_state(a), _depth_state(b))
    assert b.images[ids[0]].depth.activated and not b.images[ids[4]].depth.activated
    # rescale_depths alone: the update variances scale, the integrated map keeps its values
    before = _depth_state(b)
    b.rescale_depths({ids[2]: (0.5, 2.0)})
    after = _depth_state(b)
    np.testing.assert_array_equal(after[ids[2]]["data"], before[ids[2]]["data"])
    np.testing.assert_array_equal(after[ids[2]]["uncertainty_update"], before[ids[2]]["uncertainty_update"] * 4.0)
    np.testing.assert_array_equal(after[ids[2]]["data_prior"], before[ids[2]]["data_prior"])
    # normalize_depths: priors of every image, and the integrated map of the activated ones
    b.normalize_depths(0.5)
    last = _depth_state(b)
    for i in ids:
        np.testing.assert_array_equal(last[i]["data_prior"], after[i]["data_prior"] * 0.5)
        np.testing.assert_array_equal(last[i]["uncertainty"], after[i]["uncertainty"] * 0.25)
        np.testing.assert_array_equal(last[i]["uncertainty_update"], after[i]["uncertainty_update"] * 0.25)
        assert last[i]["scale"] == after[i]["scale"] * 0.5
        if after[i]["activated"]:
            np.testing.assert_array_equal(last[i]["data"], after[i]["data"] * 0.5)
        else:
            assert last[i]["data"] is None


# ---- normalisation ---------------------------------------------------------------------------------------------------------------
def _point_scene(xyz, n_cams=3, seed=0):
    """A PackageScene with the given points (each observed by every camera) and cameras on a ring that look at the origin."""
    from numpy_scene import NumpyCamera, NumpyDepth, NumpyImage, Rigid3d, Track
    from mpsfm_amd.synthetic import quat_from_R

    rng = np.random.default_rng(seed)
    sc = PackageScene()
    sc.rec.cameras[0] = NumpyCamera(0, [900.0, 950.0, 800.0, 600.0], 1600.0, 1200.0, 16, 12)
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    for c in range(n_cams):
        ang = 0.4 * c + 0.1
        Ry = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        t = np.array([0.1 * c, -0.2, 40.0 + c])
        kps = rng.uniform(0, 1000, (len(xyz), 2))
        depth = NumpyDepth(np.full((12, 16), 2.0 + c), np.full((12, 16), 0.1), np.ones((12, 16)), sc.rec.cameras[0], kps)
        sc.images[c + 1] = NumpyImage(c + 1, 0, Rigid3d(quat_from_R(Ry[None])[0], t), kps, 1.0, depth)
    for p, X in enumerate(xyz):
        tr = Track()
        for c in range(n_cams):
            tr.add_element(c + 1, p)
        sc.obs.add_point3D(X, tr)
    return sc


def _project(sc):
    """{(image, point): (u, v, depth)}"""
    out = {}
    ids = sorted(sc.points3D)
    X = sc.point3D_coordinates(ids)
    for i, im in sc.images.items():
        Xc = im.cam_from_world * X
        fx, fy, cx, cy = sc.rec.cameras[im.camera_id].params
        out[i] = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy, Xc[:, 2]], 1)
    return out


def _hand_sets():
    rng = np.random.default_rng(7)
    ties = np.array([[0.0, 5, 1], [1, 5, 1], [1, 5, 2], [1, 6, 3], [2, 7, 4], [3, 8, 5], [4, 9, 6], [4, 9, 7], [4, 9, 7], [5, 9, 8], [9, 9, 9]])
    return {1: rng.normal(0, 3, (1, 3)), 2: rng.normal(0, 3, (2, 3)), 3: rng.normal(0, 3, (3, 3)), 4: rng.normal(0, 3, (4, 3)),
            11: rng.normal(0, 3, (11, 3)), "ties": ties}


@pytest.mark.parametrize("name", [1, 2, 3, 4, 11, "ties"])
def test_normalize_puts_the_box_where_the_rule_says_and_keeps_every_reprojection(name):
    xyz = _hand_sets()[name]
    n = len(xyz)
    sc = _point_scene(xyz)
    before = _project(sc)
    poses = {i: (im.cam_from_world.rotation.quat.copy(), im.cam_from_world.translation.copy()) for i, im in sc.images.items()}
    scale, translation = normalize(sc)
    after = _project(sc)
    if n < 2:
        assert scale == 1.0 and np.all(translation == 0)
        np.testing.assert_array_equal(sc.point3D_coordinates(sorted(sc.points3D)), xyz)
        for i, im in sc.images.items():
            np.testing.assert_array_equal(im.cam_from_world.translation, poses[i][1])
        return
    # the rule by hand: sorted float32 per axis, the percentile indices, the mean between them
    srt = np.sort(xyz.astype(np.float32), axis=0).astype(np.float64)
    p0, p1 = (int(0.2 * (n - 1)), int(0.8 * (n - 1))) if n > 3 else (0, n - 1)
    assert (p0, p1) == {2: (0, 1), 3: (0, 2), 4: (0, 2), 11: (2, 8)}[n]
    lo, hi = srt[p0], srt[p1]
    c = np.array([sum(srt[p0:p1 + 1, a].tolist()) / (p1 - p0 + 1) for a in range(3)])
    blo, bhi, bc = bounding_box_and_centroid(xyz, 0.2, 0.8)
    np.testing.assert_array_equal(blo, lo), np.testing.assert_array_equal(bhi, hi)
    np.testing.assert_allclose(bc, c, rtol=1e-15)
    if name == "ties":
        np.testing.assert_array_equal(lo, [1, 5, 2]), np.testing.assert_array_equal(hi, [4, 9, 7])
    assert scale == pytest.approx(5.0 / np.linalg.norm(hi - lo), rel=1e-15)
    np.testing.assert_allclose(translation, -scale * c, rtol=1e-15)
    # the box corners land at scale (corner - c): the new box has extent 5 around the centroid's image, the origin
    np.testing.assert_allclose(np.linalg.norm(scale * (hi - c) - scale * (lo - c)), 5.0, rtol=1e-14)
    np.testing.assert_allclose(sc.point3D_coordinates(sorted(sc.points3D)), scale * (xyz - c), rtol=1e-14, atol=1e-14)
    for i in before:
        np.testing.assert_array_equal(sc.images[i].cam_from_world.rotation.quat, poses[i][0])
        np.testing.assert_allclose(after[i][:, :2], before[i][:, :2], rtol=1e-12)  # every reprojection stays
        np.testing.assert_allclose(after[i][:, 2], scale * before[i][:, 2], rtol=1e-12)  # every depth scales


def test_normalize_options_and_the_depth_maps():
    xyz = _hand_sets()[11]
    sc = _point_scene(xyz)
    scale, tr = normalize(sc, fixed_scale=True)
    assert scale == 1.0 and np.any(tr != 0)
    sc = _point_scene(xyz, n_cams=5)
    centres = np.array([-im.cam_from_world.rotation.matrix().T @ im.cam_from_world.translation for im in sc.images.values()])
    lo, hi, c = bounding_box_and_centroid(centres, 0.0, 1.0)
    scale, tr = normalize(sc, extent=10, min_percentile=0.0, max_percentile=1.0, use_images=True)
    assert scale == pytest.approx(10.0 / np.linalg.norm(hi - lo), rel=1e-15)
    np.testing.assert_allclose(tr, -scale * c, rtol=1e-15)
    sc = _point_scene(np.ones((5, 3)))  # no extent: the scale stays, the centroid moves to the origin
    scale, tr = normalize(sc)
    assert scale == 1.0
    np.testing.assert_array_equal(sc.point3D_coordinates(sorted(sc.points3D)), np.zeros((5, 3)))
    # MpsfmReconstruction.normalize: the similarity's scale reaches the depth maps
    sc = _point_scene(xyz)
    prior = {i: im.depth.data_prior.copy() for i, im in sc.images.items()}
    want, _ = normalize(copy.deepcopy(sc))
    assert normalize_scene(sc) is True
    for i, im in sc.images.items():
        np.testing.assert_array_equal(im.depth.data_prior, prior[i] * want)
        np.testing.assert_array_equal(im.depth.data, prior[i] * want)
        assert im.depth.scale == want


# ---- one iteration of the global refinement ---------------------------------------------------------------------------------------
def oracle_numerics(tracks, xyz, device):
    return O.filter_tracks(tracks, xyz)


class GlobalRefinementReplay(MapperReplay):
    """base.py:476-514 for one iteration (no triangulator: the track engine is outside this test), every step package code:
    calculate_point_covs -> optimize_prior_shiftscale -> rescale_all -> _refinement(global) -> normalize."""

    def global_refinement_iteration(self):
        self.first_refinement = True
        bundle = self.find_global_bundle()
        self.calls.append(("calculate_point_covs",))
        self.optimizer.calculate_point_covs(bundle)
        self.calls.append(("optimize_prior_shiftscale",))
        shift_scale, success = self.optimizer.optimize_prior_shiftscale(bundle)
        self.mpsfm_rec.rescale_all(shift_scale)
        changed, success = self._refinement(bundle, int_covs=False, mode="global", allow_scale_filter=True)
        self.calls.append(("normalize",))
        normalize_scene(self.mpsfm_rec)
        return shift_scale, changed, success


def _replay_scene(stats):
    prob, truth = make_scene(6, 300, True, seed=33)
    sc = scene_from_problem(prob, truth, map_size=(64, 48), seed=34)
    sc.__class__ = PackageScene
    sc.obs = HipObservationManager(sc, ObservationManager(sc), numerics=oracle_numerics)
    for k, imid in enumerate(sorted(sc.images)):  # priors that the fit has to bring back
        d = sc.images[imid].depth
        d.data_prior, d.data = d.data_prior * (1.0 + 0.1 * k), d.data * (1.0 + 0.1 * k)
    return sc, GlobalRefinementReplay(sc, Optimizer({}, sc, None, backend=StatsOracleBackend(), stats=stats), None, integrate=False)


def test_one_global_refinement_iteration_replays_with_package_code():
    (a, ma), (b, mb) = _replay_scene("host"), _replay_scene("device")
    ra, rb = ma.global_refinement_iteration(), mb.global_refinement_iteration()
    assert ma.calls == mb.calls
    assert [c[0] for c in ma.calls] == ["calculate_point_covs", "optimize_prior_shiftscale", "update_truncation_multiplier", "ba",
                                        "filter_bundle", "normalize"]
    assert mb.optimizer.backend.stats_calls == 2 and ma.optimizer.backend.stats_calls == 0
    assert ra[2] and rb[2] and ra[1] == rb[1]
    for imid, (shift, scale) in ra[0].items():
        assert shift == 0.0 and scale == pytest.approx(rb[0][imid][1], rel=1e-12)
        assert scale == pytest.approx(1.0 / (1.0 + 0.1 * sorted(a.images).index(imid)), rel=0.05)  # the fit undoes the scaling
    assert mb.optimizer.truncation_multiplier == pytest.approx(ma.optimizer.truncation_multiplier, rel=1e-9)
    # after normalize: the 20 % .. 80 % box of the points has extent 5 and its centroid is the origin, in both scenes
    for sc in (a, b):
        lo, hi, c = bounding_box_and_centroid(sc.point3D_coordinates(sorted(sc.points3D)), 0.2, 0.8)
        assert np.linalg.norm(hi - lo) == pytest.approx(5.0, rel=1e-6) and np.abs(c).max() < 1e-6
    assert set(a.points3D) == set(b.points3D)
    np.testing.assert_allclose(a.point3D_coordinates(sorted(a.points3D)), b.point3D_coordinates(sorted(b.points3D)), atol=1e-6)
    for i in a.images:
        np.testing.assert_allclose(a.images[i].depth.data_prior, b.images[i].depth.data_prior, rtol=1e-9)
        assert a.images[i].depth.scale == pytest.approx(b.images[i].depth.scale, rel=1e-9)
