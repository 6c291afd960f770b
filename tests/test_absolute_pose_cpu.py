"""CPU checks of the absolute-pose estimator: the NumPy restatement on noise-free scenes, the trial budget, the sampler,
argument validation of mpsfm_abs_pose_estimate before any device is touched, and the configuration of the drop-in
AbsolutePose (reference mpsfm/sfm/estimators/absolute_pose.py)."""

import ctypes as C

import numpy as np
import pytest

import numpy_absolute_pose as NA
from mpsfm_amd import capi
from mpsfm_amd.sfm.estimators import AbsolutePose
from mpsfm_amd.sfm.estimators.absolute_pose import ESTIMATION_DEFAULTS, REFINEMENT_DEFAULTS


@pytest.mark.parametrize("outliers", [0.0, 0.4, 0.7])
def test_restatement_recovers_noise_free_pose(outliers):
    for seed in range(3):
        p2, X, K, R, t, inl = NA.synthetic_problem(300, outliers, seed=100 + seed)
        r = NA.estimate(p2, X, K, seed=seed)
        assert r["success"]
        assert np.abs(r["cam_from_world"] - np.c_[R, t]).max() < 1e-9
        assert np.array_equal(r["inlier_mask"], inl)
        assert r["num_inliers"] == inl.sum()
        assert r["num_trials"] <= r["max_num_trials"]


def test_trial_cap_and_bounds():
    assert NA.num_trials(int(0.25 * 100000), 100000, 0.99999, 3.0) == 2194
    assert NA.num_trials(0, 100, 0.99999, 3.0) == float("inf")
    assert NA.num_trials(100, 100, 0.99999, 3.0) == 1
    # all inliers: the dynamic bound is 1 at once, so min_num_trials decides where the loop stops.  LORANSAC's report
    # counts two trials past the one that set the abort flag (the loop's increment, then `num_trials += 1; break`)
    p2, X, K, R, t, inl = NA.synthetic_problem(100, 0.0, seed=5)
    for m in (0, 7, 100):
        r = NA.estimate(p2, X, K, min_num_trials=m)
        assert r["num_trials"] == max(m, 1) + 2
    r = NA.estimate(p2, X, K, min_num_trials=5, max_num_trials=5)
    assert r["num_trials"] == 5
    # 70 % outliers: the dynamic bound of the true inlier ratio, below the 2194 cap
    p2, X, K, R, t, inl = NA.synthetic_problem(400, 0.7, seed=6)
    r = NA.estimate(p2, X, K)
    dyn = NA.num_trials(int(inl.sum()), 400, 0.99999, 3.0)
    assert r["max_num_trials"] == 2194 and dyn < 2194
    assert dyn + 2 <= r["num_trials"] <= dyn + 5


def test_sampler_draws_distinct_indices_in_range():
    for n in (3, 4, 5, 17, 1000, 2**31 - 1):
        for t in range(200):
            idx = NA.sample(12345, t, n)
            assert len(set(idx)) == 3 and all(0 <= i < n for i in idx)
    assert NA.sample(0, 0, 1000) != NA.sample(1, 0, 1000)
    assert NA.sample(0, 0, 1000) != NA.sample(0, 1, 1000)


def _call(n, p2, p3, K, o=None, mask=True, res=True):
    L = capi.lib()
    if o is None:
        o = capi.CAbsPoseOptions(12.0, 0.25, 0.99999, 3.0, 100, 10000, 0, 0, 0)
    m = np.zeros(max(n, 1), np.uint8)
    r = capi.CAbsPoseResult()
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    return L.mpsfm_abs_pose_estimate(n, ptr(p2), ptr(p3), ptr(K), C.byref(o) if o is not False else None, 0,
                                     m.ctypes.data if mask else None, C.byref(r) if res else None)


def test_entry_point_validates_arguments_first():
    p2, X, K, *_ = NA.synthetic_problem(20, 0.0, seed=1)
    p2, X, K = np.ascontiguousarray(p2), np.ascontiguousarray(X), np.ascontiguousarray(K)
    assert _call(20, None, X, K) == capi_einval()
    assert _call(20, p2, None, K) == capi_einval()
    assert _call(20, p2, X, None) == capi_einval()
    assert _call(20, p2, X, K, o=False) == capi_einval()
    assert _call(20, p2, X, K, mask=False) == capi_einval()
    assert _call(20, p2, X, K, res=False) == capi_einval()
    assert _call(2, p2, X, K) == capi_einval()
    assert _call(-1, p2, X, K) == capi_einval()
    assert _call(2**31, p2, X, K) == capi_einval()
    for arr, k in ((p2, 0), (X, 0), (K, 0), (p2, 7), (X, 11)):
        bad = arr.copy()
        bad.reshape(-1)[k] = np.nan
        args = [p2, X, K]
        args[[p2 is arr, X is arr, K is arr].index(True)] = bad
        assert _call(20, *args) == capi_einval()
    bad = X.copy()
    bad[3, 1] = np.inf
    assert _call(20, p2, bad, K) == capi_einval()
    zero_f = K.copy()
    zero_f[0] = 0.0
    assert _call(20, p2, X, zero_f) == capi_einval()
    for field, value in (("max_error", 0.0), ("min_inlier_ratio", 0.0), ("confidence", 1.5), ("min_num_trials", -1),
                         ("batch_trials", -3)):
        o = capi.CAbsPoseOptions(12.0, 0.25, 0.99999, 3.0, 100, 10000, 0, 0, 0)
        setattr(o, field, value)
        assert _call(20, p2, X, K, o=o) == capi_einval()
    with pytest.raises(capi.MpsfmHipError) as e:
        capi.abs_pose_estimate(p2[:2], X[:2], K)
    assert e.value.code == -1


def capi_einval():
    return -1


def test_entry_point_without_device_fails_loudly():
    if capi.device_count() > 0:
        pytest.skip("a gfx950 device is visible")
    p2, X, K, *_ = NA.synthetic_problem(20, 0.0, seed=1)
    with pytest.raises(capi.MpsfmHipError) as e:
        capi.abs_pose_estimate(p2, X, K)
    assert e.value.code == -2


class _Cam:
    def __init__(self, model, params):
        self.model, self.params = model, np.asarray(params, np.float64)


def test_shim_merges_nested_options():
    a = AbsolutePose({"colmap_estimation_options": {"ransac": {"max_error": 8}}, "colmap_refinement_options": {"max_num_iterations": 7}})
    r = a.conf.colmap_estimation_options.ransac
    assert r.max_error == 8
    for k, v in ESTIMATION_DEFAULTS["ransac"].items():
        if k != "max_error":
            assert r[k] == v
    assert a.conf.colmap_estimation_options.estimate_focal_length is False
    assert a.conf.colmap_refinement_options.max_num_iterations == 7
    assert a.conf.colmap_refinement_options.gradient_tolerance == REFINEMENT_DEFAULTS["gradient_tolerance"]
    assert AbsolutePose().conf.colmap_estimation_options.ransac.min_inlier_ratio == 0.25
    assert ESTIMATION_DEFAULTS["ransac"]["max_error"] == 12.0  # the defaults are not mutated by a merge
    with pytest.raises(KeyError):
        AbsolutePose({"colmap_estimation_options": {"ransac": {"max_eror": 8}}})
    with pytest.raises(KeyError):
        AbsolutePose({"no_such_key": 1})


@pytest.mark.parametrize("conf", [
    {"colmap_estimation_options": {"estimate_focal_length": True}},
    {"colmap_refinement_options": {"refine_focal_length": True}},
    {"colmap_refinement_options": {"refine_extra_params": True}},
])
def test_shim_refuses_unimplemented_options(conf):
    with pytest.raises(NotImplementedError):
        AbsolutePose(conf)


def test_shim_refuses_other_cameras_and_returns_none_below_three_points():
    a = AbsolutePose()
    p2, X, K, *_ = NA.synthetic_problem(10, 0.0, seed=2)
    with pytest.raises(NotImplementedError):
        a(p2, X, _Cam("SIMPLE_RADIAL", [800, 640, 480, 0.01]))
    cam = _Cam("PINHOLE", K)
    assert a(p2[:2], X[:2], cam) is None
    assert a(np.zeros((0, 2)), np.zeros((0, 3)), cam) is None


def test_refinement_problem_is_one_variable_camera_with_constant_landmarks():
    from oracle import cpu_oracle as O

    p2, X, K, R, t, inl = NA.synthetic_problem(200, 0.0, seed=3, noise_px=0.5)
    a = AbsolutePose()
    prob = a.refinement_problem(np.c_[R, t], p2, X, K)
    assert prob.n_cams == 1 and prob.pose_const[0] == 0 and prob.gauge_axis_cam == -1
    assert prob.pt_const.all() and prob.n_obs == 200 and prob.n_dobs == 0
    o = O.default_options(max_num_iterations=100, gradient_tolerance=1.0)
    s = O.solve(prob, o)
    assert s["final_cost"] <= s["initial_cost"]
    assert np.array_equal(prob.pts, X)  # landmarks stay constant
