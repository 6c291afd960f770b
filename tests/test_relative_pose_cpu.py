"""CPU checks of the relative-pose estimator: the NumPy restatement on noise-free scenes (general, planar, forward motion),
the trial budget for sample size 5, the five-index sampler, the decomposition's candidate choice, argument validation of
mpsfm_rel_pose_estimate before any device is touched, and the configuration of the drop-in RelativePose (reference
mpsfm/sfm/estimators/relative_pose.py)."""

import ctypes as C

import numpy as np
import pytest

import numpy_relative_pose as NR
from mpsfm_amd import capi
from mpsfm_amd.sfm.estimators import RelativePose
from mpsfm_amd.sfm.estimators.relative_pose import RANSAC_DEFAULTS


def _angle(R):
    return float(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))


@pytest.mark.parametrize("kind", ["general", "planar", "forward"])
def test_restatement_recovers_noise_free_relative_pose(kind):
    p1, p2, K1, K2, R, t, inl = NR.synthetic_problem(150, 0.4, seed=11, planar=kind == "planar", forward=kind == "forward")
    r = NR.estimate(p1, p2, K1, K2, seed=2, max_error=1.0, min_num_trials=200)
    assert r["success"]
    P = r["cam2_from_cam1"]
    assert np.abs(P[:, :3] - R).max() < 1e-8
    assert np.abs(P[:, 3] - t).max() < 1e-8
    assert np.array_equal(r["inlier_mask"], inl) and r["num_inliers"] == inl.sum()
    assert r["num_cheirality_points"] == inl.sum()
    E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
    assert np.abs(r["E"] - NR.canonical(E)).max() < 1e-8


def test_five_point_solutions_contain_the_truth_and_are_ordered():
    p1, p2, K1, K2, R, t, inl = NR.synthetic_problem(5, 0.0, seed=4)
    x1, x2 = NR.normalise(p1, K1), NR.normalise(p2, K2)
    E = NR.canonical(np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R)
    models = NR.five_point(x1, x2)
    assert 1 <= len(models) <= 10
    assert min(np.abs(m - E).max() for m in models) < 1e-10
    keys = [tuple(m.reshape(-1)) for m in models]
    assert keys == sorted(keys)
    for m in models:
        assert abs(np.linalg.norm(m) - 1) < 1e-12 and m.reshape(-1)[np.argmax(np.abs(m))] > 0
        assert np.abs(NR.sampson(m, x1, x2)).max() < 1e-18
    # coincident points: the nullspace is larger than 4, no model
    assert NR.five_point(np.tile(x1[:1], (5, 1)), np.tile(x2[:1], (5, 1))) == []


def test_trial_cap_and_bounds():
    assert NR.num_trials(int(0.01 * 100000), 100000, 0.9999, 3.0) > 100000  # the cap leaves max_num_trials = 100 000
    assert NR.num_trials(int(0.25 * 100000), 100000, 0.9999, 3.0) == 28281  # ceil(log(1e-4) / log(1 - 0.25^5) 3)
    assert NR.num_trials(50, 100, 0.9999, 3.0) == 871
    assert NR.num_trials(0, 100, 0.9999, 3.0) == float("inf")
    assert NR.num_trials(100, 100, 0.9999, 3.0) == 1
    p1, p2, K1, K2, R, t, inl = NR.synthetic_problem(60, 0.0, seed=5)
    r = NR.estimate(p1, p2, K1, K2, min_num_trials=7)
    assert r["max_num_trials"] == 100000 and r["num_trials"] == 9  # two past the trial that set the abort flag
    r = NR.estimate(p1, p2, K1, K2, min_num_trials=5, max_num_trials=5)
    assert r["num_trials"] == 5


def test_sampler_draws_five_distinct_indices_in_range():
    for n in (5, 6, 17, 1000, 2**31 - 1):
        for t in range(200):
            idx = NR.sample(12345, t, n)
            assert len(idx) == 5 and len(set(idx)) == 5 and all(0 <= i < n for i in idx)
    assert NR.sample(0, 0, 1000) != NR.sample(1, 0, 1000)
    assert NR.sample(0, 0, 1000)[:3] == __import__("numpy_absolute_pose").sample(0, 0, 1000)  # the same recipe, two more draws


def test_decomposition_picks_the_physical_candidate():
    R = NR._rot([0.3, -1.0, 0.2], 0.4)
    t = np.array([0.6, -0.2, 0.3])
    t /= np.linalg.norm(t)
    rng = np.random.default_rng(8)
    X = np.c_[rng.uniform(-2, 2, (40, 2)), rng.uniform(4, 9, 40)]
    X2 = X @ R.T + t
    x1, x2 = X[:, :2] / X[:, 2:], X2[:, :2] / X2[:, 2:]
    E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
    for s in (1.0, -1.0):  # E and -E: the same pose
        P, npts, counts = NR.pose_from_essential(NR.canonical(s * E), x1, x2)
        assert np.abs(P[:, :3] - R).max() < 1e-10 and np.abs(P[:, 3] - t).max() < 1e-10
        assert npts == 40 and sorted(counts)[-2] < 40
    R1, R2, tt = NR.decompose(E)
    assert abs(np.linalg.det(R1) - 1) < 1e-12 and abs(np.linalg.det(R2) - 1) < 1e-12
    assert tt[np.argmax(np.abs(tt))] > 0


def _call(n, p1, p2, K1, K2, o=None, mask=True, res=True):
    L = capi.lib()
    if o is None:
        o = capi.CRelPoseOptions(4.0, 0.01, 0.9999, 3.0, 1000, 100000, 0, 0, 0)
    m = np.zeros(max(n, 1), np.uint8)
    r = capi.CRelPoseResult()
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    return L.mpsfm_rel_pose_estimate(n, ptr(p1), ptr(p2), ptr(K1), ptr(K2), C.byref(o) if o is not False else None, 0,
                                     m.ctypes.data if mask else None, C.byref(r) if res else None)


def test_entry_point_validates_arguments_first():
    p1, p2, K1, K2, *_ = NR.synthetic_problem(20, 0.0, seed=1)
    p1, p2, K1, K2 = (np.ascontiguousarray(a) for a in (p1, p2, K1, K2))
    einval = -1
    assert _call(20, None, p2, K1, K2) == einval
    assert _call(20, p1, None, K1, K2) == einval
    assert _call(20, p1, p2, None, K2) == einval
    assert _call(20, p1, p2, K1, None) == einval
    assert _call(20, p1, p2, K1, K2, o=False) == einval
    assert _call(20, p1, p2, K1, K2, mask=False) == einval
    assert _call(20, p1, p2, K1, K2, res=False) == einval
    for n in (4, 0, -1, 2**31):
        assert _call(n, p1, p2, K1, K2) == einval
    for which, k in ((0, 0), (0, 7), (1, 3), (1, 39)):
        args = [p1.copy(), p2.copy()]
        args[which].reshape(-1)[k] = np.nan if k % 2 else np.inf
        assert _call(20, *args, K1, K2) == einval
    for which in (0, 1):
        Ks = [K1.copy(), K2.copy()]
        Ks[which][which] = 0.0
        assert _call(20, p1, p2, *Ks) == einval
        Ks = [K1.copy(), K2.copy()]
        Ks[which][2] = np.nan
        assert _call(20, p1, p2, *Ks) == einval
    for field, value in (("max_error", 0.0), ("min_inlier_ratio", 0.0), ("min_inlier_ratio", 1.5), ("confidence", 1.5),
                         ("dyn_num_trials_multiplier", 0.0), ("min_num_trials", -1), ("max_num_trials", 10), ("batch_trials", -3),
                         ("batch_trials", 1 << 20)):
        o = capi.CRelPoseOptions(4.0, 0.01, 0.9999, 3.0, 1000, 100000, 0, 0, 0)
        setattr(o, field, value)
        assert _call(20, p1, p2, K1, K2, o=o) == einval
    with pytest.raises(capi.MpsfmHipError) as e:
        capi.rel_pose_estimate(p1[:4], p2[:4], K1, K2)
    assert e.value.code == -1
    with pytest.raises(KeyError):
        capi.rel_pose_estimate(p1, p2, K1, K2, max_eror=3.0)


def test_entry_point_without_device_fails_loudly():
    if capi.device_count() > 0:
        pytest.skip("a gfx950 device is visible")
    p1, p2, K1, K2, *_ = NR.synthetic_problem(20, 0.0, seed=1)
    with pytest.raises(capi.MpsfmHipError) as e:
        capi.rel_pose_estimate(p1, p2, K1, K2)
    assert e.value.code == -2


class _Cam:
    def __init__(self, model, params):
        self.model, self.params = model, np.asarray(params, np.float64)


def test_shim_merges_options_and_refuses_unknown_keys():
    r = RelativePose({"colmap_options": {"max_error": 2.5, "min_num_trials": 50}})
    o = r.conf.colmap_options
    assert o.max_error == 2.5 and o.min_num_trials == 50
    for k, v in RANSAC_DEFAULTS.items():
        if k not in ("max_error", "min_num_trials"):
            assert o[k] == v
    assert RelativePose().conf.colmap_options.max_num_trials == 100000
    assert RANSAC_DEFAULTS["max_error"] == 4.0  # the defaults are not mutated by a merge
    with pytest.raises(KeyError):
        RelativePose({"colmap_options": {"max_eror": 8}})
    with pytest.raises(KeyError):
        RelativePose({"no_such_key": 1})


def test_shim_refuses_other_cameras_and_returns_none_below_five_matches():
    r = RelativePose()
    p1, p2, K1, K2, *_ = NR.synthetic_problem(10, 0.0, seed=2)
    with pytest.raises(NotImplementedError):
        r(p1, p2, _Cam("SIMPLE_RADIAL", [800, 640, 480, 0.01]), _Cam("PINHOLE", K2))
    with pytest.raises(NotImplementedError):
        r(p1, p2, _Cam("PINHOLE", K1), _Cam("OPENCV", [800, 800, 640, 480, 0, 0, 0, 0]))
    assert r(p1[:4], p2[:4], _Cam("PINHOLE", K1), _Cam("SIMPLE_PINHOLE", [700, 600, 500])) is None
    assert r(np.zeros((0, 2)), np.zeros((0, 2)), _Cam("PINHOLE", K1), _Cam("PINHOLE", K2)) is None
