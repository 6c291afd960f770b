"""Prior construction without a GPU: the NumPy restatement (tests/numpy_mono_priors.py) against the reference's own
results (tests/golden/reference_mono_priors.npz), the ctypes structs against the header, the classes' settings against
the reference's, and the mask-resize rule against the bilinear resize."""

import ctypes as C
import json
import os

import numpy as np
import pytest

import numpy_mono_priors as NMP
from mpsfm_amd import capi
from mpsfm_amd.sfm.scene.integration import resize_linear

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_mono_priors.npz"))


def exact_case(meta, item, key="depth"):
    """equal sizes or exact factor 2 on even sizes: the resize is a copy or a 2x2 mean"""
    h, w = item[key].shape[:2]
    H, W = meta["size"]
    return (h, w) == (H, W) or (h == 2 * H and w == 2 * W)


def test_fixture_holds_every_case_and_a_small_redraw_share(ref):
    meta = json.loads(str(ref["cases"]))
    names = {c["name"] for c in meta["depth"]}
    for need in ("a_default", "b_flip_prior", "b_flip_only", "c_fixed", "c_variance_only", "d_half", "d_odd", "d_up", "e_masks",
                 "f_a_default_f32", "g_threshold_f64", "g_threshold_f32", "k_1x1", "k_1x5", "k_5x1"):
        assert need in names
    assert {"i_equal", "i_odd", "j_flip_equal", "j_flip_odd"} <= {c["name"] for c in meta["normals"]}
    assert 0.0 <= float(ref["redraw_share"]) < 0.2
    e = dict((c["name"], c) for c in meta["depth"])["e_masks"]
    assert e["conf"]["depth_lim"] is not None and e["conf"]["max_std"] is not None


def test_restatement_equals_the_reference_depth(ref):
    for meta, item, want in NMP.fixture_cases(ref, "depth"):
        got = NMP.depth_priors(item, meta["conf"])
        for k in ("valid", "continuity_mask"):
            assert np.array_equal(got[k], want[k]), (meta["name"], k)
        if meta["masks_only"]:
            continue
        rel = 1e-15 if exact_case(meta, item) else 1e-13
        for k in ("data_prior", "uncertainty"):
            NMP.assert_values(got[k], want[k], rel, f"{meta['name']}.{k}")
        # a sample is measured against the uncertainties around it, not against a 1e6 fill elsewhere in the list
        NMP.assert_values(got["uncertainty_update"], want["uncertainty_update"], rel, f"{meta['name']}.uncertainty_update",
                          scale=NMP.kps_local_scale(want["uncertainty"], item["kps"], item["sx"], item["sy"]))


def test_restatement_equals_the_reference_normals(ref):
    for meta, item, want in NMP.fixture_cases(ref, "normals"):
        got = NMP.normal_priors(item, meta["conf"])
        rel = 1e-15 if exact_case(meta, item, "normals") else 1e-13
        for k in NMP.NORMALS_OUT:
            NMP.assert_values(got[k], want[k], rel, f"{meta['name']}.{k}")


def test_half_size_is_pythons_floor_division_on_both_sides_of_the_abi():
    """`int(W // f)` for a non-integer factor is not floor(W / f) (77 // 1.1 == 69, floor(77 / 1.1) == 70): the library
    computes it like Python and refuses a problem whose half size, for which the caller allocated, is another one.  The
    check comes before the device is opened, so it runs here."""
    assert int(77 // 1.1) == 69 and int(np.floor(77 / 1.1)) == 70 and int(11 // 1.1) == 9
    L = capi.lib()
    n, v = np.zeros((4, 4, 3)) + [0.0, 0.0, -1.0], np.full((4, 4), 0.01)

    def call(H, W, f, Hd, Wd):
        out = [np.zeros((H, W, 3)), np.zeros((H, W, 3, 3)), np.zeros((max(Hd, 1), max(Wd, 1), 3)), np.zeros((max(Hd, 1), max(Wd, 1), 3, 3))]
        P, O, cf = capi.CNormalPriorProblem(), capi.CNormalPriorOutput(), capi.CNormalPriorConf()
        P.height, P.width, P.int_height, P.int_width, P.half_height, P.half_width = 4, 4, H, W, Hd, Wd
        P.normals, P.normals_variance = n.ctypes.data, v.ctypes.data
        O.data, O.uncertainty, O.data_downscaled, O.uncertainty_downscaled = (a.ctypes.data for a in out)
        cf.inherent_polar_noise, cf.std_multiplier, cf.lc_std_multiplier, cf.prior_std_multiplier, cf.downscale_factor = 0.017, 1, 1, 1, f
        return L.mpsfm_normal_priors(1, C.addressof(P), C.addressof(cf), 0, C.addressof(O), None)

    accepted = (0, -2)  # computed, or no device here: the sizes passed the check
    assert call(11, 77, 1.1, 9, 69) in accepted
    assert call(11, 77, 1.1, 10, 70) == -1 and call(11, 77, 1.1, 9, 70) == -1 and call(11, 77, 1.1, 10, 69) == -1
    assert "half_height" in (L.mpsfm_last_error() or b"").decode()
    rng = np.random.default_rng(11)
    factors = [2, 3, 1.1, 1.5, 2.5, 0.7, 1.3, 1.7, 2.2, 3.3, 0.1 * 3] + list(rng.uniform(1.0, 4.0, 40))
    for f in factors:
        for H, W in ((11, 77), (58, 77), (290, 387), (33, 21), (7, 99)):
            Hd, Wd = int(H // f), int(W // f)
            if Hd >= 1 and Wd >= 1 and Hd * Wd <= 4096:
                assert call(H, W, f, Hd, Wd) in accepted, (H, W, f)
    assert call(2, 2, 2.0, 1, 1) in accepted and call(1, 1, 2.0, 0, 0) == -1


def test_near_threshold_cases_decide_differently_in_the_two_precisions(ref):
    cases = {m["name"]: (m, i, w) for m, i, w in NMP.fixture_cases(ref, "depth")}
    c64, c32 = cases["g_threshold_f64"][2]["continuity_mask"], cases["g_threshold_f32"][2]["continuity_mask"]
    assert 0 < c64.sum() < c64.size and 0 < c32.sum() < c32.size
    assert not np.array_equal(c64, c32)  # the same values: the precision of the test decides
    assert cases["g_threshold_f32"][1]["depth"].dtype == np.float32 and cases["g_threshold_f64"][1]["depth"].dtype == np.float64


def test_resize_rules_equal_the_packages_resize_linear(ref):
    rng = np.random.default_rng(5)
    sizes = {(tuple(i["depth"].shape), tuple(m["size"])) for m, i, _ in NMP.fixture_cases(ref, "depth")}
    sizes |= {(tuple(i["normals"].shape[:2]), tuple(m["size"])) for m, i, _ in NMP.fixture_cases(ref, "normals")}
    sizes |= {((96, 128), (58, 77)), ((58, 77), (29, 38)), ((518, 692), (290, 387))}
    assert any(a != b for a, b in sizes)
    for src, dst in sorted(sizes):
        img = rng.uniform(0.5, 4.0, src)
        want = resize_linear(img, (dst[1], dst[0]))
        got = NMP.resize_linear(img, dst)
        assert np.abs(got - want).max() <= 1e-15 * 4.0 * 4, (src, dst)
        if src == dst:
            assert np.array_equal(got, img)
        for p in (0.5, 0.9, 1.0):
            mask = rng.uniform(size=src) < p
            assert np.array_equal(NMP.resize_mask(mask, dst), resize_linear(mask.astype(np.float64), (dst[1], dst[0])) == 1), (src, dst, p)
    m = np.arange(12).reshape(3, 4)
    assert np.array_equal(NMP.resize_nearest(m, (6, 8)), m[np.arange(6) // 2][:, np.arange(8) // 2])
    assert np.array_equal(NMP.resize_nearest(m, (2, 3)), m[[0, 1]][:, [0, 1, 2]])
    assert np.array_equal(NMP.resize_linear(np.arange(16.0).reshape(4, 4), (2, 2)), np.array([[2.5, 4.5], [10.5, 12.5]]))  # 2x2 means


def test_default_conf_equals_the_reference(ref):
    from mpsfm_amd.sfm.scene.image import Depth, Normals

    assert Depth.default_conf == json.loads(str(ref["depth_default_conf"])) == NMP.DEPTH_CONF
    assert Normals.default_conf == json.loads(str(ref["normals_default_conf"])) == NMP.NORMALS_CONF
    assert list(Depth.default_conf) == list(json.loads(str(ref["depth_default_conf"])))


def test_argument_errors_come_before_the_device():
    """MPSFM_EINVAL for what the reference asserts, an empty batch is a no-op, and without a device a valid call fails
    loudly (MPSFM_ENODEVICE)."""
    assert capi.depth_priors([], NMP.DEPTH_CONF) == [] and capi.normal_priors([], NMP.NORMALS_CONF) == []
    d = np.full((4, 5), 2.0)
    n = np.zeros((4, 5, 3)) + [0.0, 0.0, -1.0]
    base = dict(depth=d, depth_variance=d * 0.01, size=(4, 5), kps=np.zeros((0, 2)), sx=1.0, sy=1.0)
    nbase = dict(normals=n, normals_variance=d * 0.01, size=(4, 5))

    def code(fn, *a):
        with pytest.raises(capi.MpsfmHipError) as e:
            fn(*a)
        return e.value.code

    assert code(capi.depth_priors, [base], dict(NMP.DEPTH_CONF, flip_consistency=True)) == -1  # no depth2
    assert code(capi.depth_priors, [dict(base, depth_variance=None)], NMP.DEPTH_CONF) == -1
    assert code(capi.depth_priors, [dict(base, size=(0, 5))], NMP.DEPTH_CONF) == -1
    assert code(capi.depth_priors, [dict(base, depth_variance=None)], dict(NMP.DEPTH_CONF, prior_uncertainty=False, depth_uncertainty=None)) == -1
    assert code(capi.normal_priors, [nbase], dict(NMP.NORMALS_CONF, flip_consistency=True)) == -1  # no normals2
    assert "needs normals2" in (capi.lib().mpsfm_last_error() or b"").decode()
    assert code(capi.normal_priors, [dict(nbase, normals_variance=None)], NMP.NORMALS_CONF) == -1
    assert code(capi.normal_priors, [nbase], dict(NMP.NORMALS_CONF, std_multiplier=2, lc_std_multiplier=3)) == -1
    assert code(capi.normal_priors, [dict(nbase, size=(1, 1))], NMP.NORMALS_CONF) == -1  # no half-size map
    if capi.device_count() == 0:
        assert code(capi.depth_priors, [base], NMP.DEPTH_CONF) == -2
        assert code(capi.normal_priors, [nbase], NMP.NORMALS_CONF) == -2
