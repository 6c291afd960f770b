"""GPU parity of the prior construction (csrc/mono_priors.hip): mpsfm_depth_priors / mpsfm_normal_priors against the
reference's own results (tests/golden/reference_mono_priors.npz), batched against single calls, the Python classes, and
one medium batch against the NumPy restatement (tests/numpy_mono_priors.py).

Bounds: masks exact; fp64 values to 1e-13 of the array's largest magnitude (fills excluded and compared exactly); the
flip_consistency covariances to 1e-11 of each pixel's largest entry (the arccos there is conditioned up to ~71 by the
fixture's redraw guard, and the device's acos / sin / cos differ from the host's libm by a few ulps)."""

import os

import numpy as np
import pytest

import numpy_mono_priors as NMP
from conftest import GOLDEN
from mpsfm_amd import capi
from numpy_scene import NumpyCamera

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "reference_mono_priors.npz"))


@pytest.fixture(scope="module")
def depth_cases(ref):
    return NMP.fixture_cases(ref, "depth")


@pytest.fixture(scope="module")
def normal_cases(ref):
    return NMP.fixture_cases(ref, "normals")


def _conf(base, meta):
    return dict(base, **meta["conf"])


def _check_depth(name, got, want, item, masks_only=False):
    """`item` gives the keypoints: a sample is measured against the uncertainties around it (NMP.kps_local_scale), so one
    among ordinary variances is not excused by a 1e6 fill elsewhere in the list"""
    for k in ("valid", "continuity_mask"):
        assert got[k].dtype == np.bool_ and np.array_equal(got[k], want[k]), (name, k)
    if masks_only:
        return
    for k in ("data_prior", "uncertainty", "uncertainty_update"):
        assert got[k].dtype == np.float64
    for k in ("data_prior", "uncertainty"):
        NMP.assert_values(got[k], want[k], 1e-13, f"{name}.{k}")
    NMP.assert_values(got["uncertainty_update"], want["uncertainty_update"], 1e-13, f"{name}.uncertainty_update",
                      scale=NMP.kps_local_scale(want["uncertainty"], item["kps"], item["sx"], item["sy"]))


def _check_normals(name, got, want, flip):
    for k in ("data", "data_downscaled"):
        NMP.assert_values(got[k], want[k], 1e-13, f"{name}.{k}")
    for k in ("uncertainty", "uncertainty_downscaled"):
        if flip:
            NMP.assert_values(got[k], want[k], 1e-11, f"{name}.{k}", per_pixel=2)
        else:
            NMP.assert_values(got[k], want[k], 1e-13, f"{name}.{k}")


def test_depth_cases_equal_the_reference(depth_cases):
    for meta, item, want in depth_cases:
        got = capi.depth_priors([item], _conf(NMP.DEPTH_CONF, meta))[0]
        _check_depth(meta["name"], got, want, item, meta["masks_only"])


def test_normal_cases_equal_the_reference(normal_cases):
    for meta, item, want in normal_cases:
        got = capi.normal_priors([item], _conf(NMP.NORMALS_CONF, meta))[0]
        _check_normals(meta["name"], got, want, bool(meta["conf"].get("flip_consistency")))
    nan = dict((m["name"], w) for m, _, w in normal_cases)["i_equal"]["uncertainty"]
    assert np.isnan(nan).any()  # the zero-length normal


def test_float32_values_equal_the_float64_fixture(depth_cases, normal_cases):
    """the library upcasts on load: float32 inputs of the same (float32-representable) values give the fp64 results"""
    for meta, item, want in depth_cases:
        if meta["masks_only"] or meta["name"].startswith("g_"):  # (g): the continuity test is precision dependent by design
            continue
        item32 = {k: (v.astype(np.float32) if isinstance(v, np.ndarray) and v.dtype == np.float64 and k.startswith("depth") else v)
                  for k, v in item.items()}
        got = capi.depth_priors([item32], _conf(NMP.DEPTH_CONF, meta))[0]
        _check_depth("f32 " + meta["name"], dict(got, continuity_mask=want["continuity_mask"]), want, item)  # continuity: cases (f), (g)
    for meta, item, want in normal_cases:
        item32 = {k: (v.astype(np.float32) if k.startswith("normals") else v) for k, v in item.items()}
        got = capi.normal_priors([item32], _conf(NMP.NORMALS_CONF, meta))[0]
        _check_normals("f32 " + meta["name"], got, want, bool(meta["conf"].get("flip_consistency")))


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f") for k in a)


def test_one_batched_call_equals_the_single_calls_bit_for_bit(depth_cases, normal_cases):
    """all fixture images of one configuration in one call: mixed sizes, precisions and optional inputs"""
    for base, cases, fn in ((NMP.DEPTH_CONF, depth_cases, capi.depth_priors), (NMP.NORMALS_CONF, normal_cases, capi.normal_priors)):
        groups = {}
        for meta, item, _ in cases:
            groups.setdefault(tuple(sorted(meta["conf"].items())), []).append(item)
        assert max(len(g) for g in groups.values()) >= 3
        for key, items in groups.items():
            conf = dict(base, **dict(key))
            singles = [fn([it], conf)[0] for it in items]
            batch, summary = fn(items, conf, return_summary=True)
            again = fn(items, conf)
            assert summary["n_images"] == len(items) and summary["ms"] > 0
            for s, b, a in zip(singles, batch, again):
                assert _same(s, b) and _same(b, a)
    default = [it for m, it, _ in depth_cases if not m["conf"]]
    assert len({it["depth"].shape for it in default}) > 3 and len({it["depth"].dtype for it in default}) == 2


def test_empty_batch_and_refused_inputs(normal_cases, depth_cases):
    assert capi.depth_priors([], NMP.DEPTH_CONF) == [] and capi.normal_priors([], NMP.NORMALS_CONF) == []
    L = capi.lib()
    assert L.mpsfm_depth_priors(0, None, None, 0, None, None) == 0 and L.mpsfm_normal_priors(0, None, None, 0, None, None) == 0
    item = dict(normal_cases[0][1])
    item.pop("normals2", None)
    with pytest.raises(capi.MpsfmHipError) as e:
        capi.normal_priors([item], dict(NMP.NORMALS_CONF, flip_consistency=True))
    assert e.value.code == -1 and "needs normals2" in str(e.value)
    with pytest.raises(capi.MpsfmHipError) as e:
        capi.depth_priors([dict(depth_cases[0][1], size=(0, 4))], NMP.DEPTH_CONF)
    assert e.value.code == -1
    # the call after a refused one works
    meta, item, want = depth_cases[0]
    _check_depth(meta["name"], capi.depth_priors([item], _conf(NMP.DEPTH_CONF, meta))[0], want, item)


def _camera(size, image=(200.0, 280.0)):
    cam = NumpyCamera(1, [300.0, 300.0, image[1] / 2, image[0] / 2], image[1], image[0], size[1], size[0])
    cam.int_height, cam.int_width = size
    return cam


def test_classes_and_prepare_mono_priors(depth_cases, normal_cases):
    from mpsfm_amd.sfm.scene.image import Depth, Normals, prepare_mono_priors

    dc = {m["name"]: (m, i, w) for m, i, w in depth_cases}
    nc = {m["name"]: (m, i, w) for m, i, w in normal_cases}
    meta, item, want = dc["e_masks"]
    cam = _camera(item["size"])
    assert (cam.sx, cam.sy) == (item["sx"], item["sy"])
    ddict = {k: item[k] for k in ("depth", "depth_variance", "valid")}
    before = {k: v.copy() for k, v in ddict.items()}
    d = Depth(meta["conf"], depth_dict=ddict, camera=cam, kps=item["kps"], mask=item["mask"])
    assert all(np.array_equal(before[k], ddict[k], equal_nan=True) for k in before)  # the caller's dict is untouched
    _check_depth("Depth(e_masks)", dict((k, getattr(d, k)) for k in NMP.DEPTH_OUT), want, item)
    assert (d.scale, d.shift, d.activated, d.data) == (1, 0, False, None) and d.camera is cam and d.kps is item["kps"]
    assert np.array_equal(d.uncertainty_update, d.uncertainty_at_kps(item["kps"]))  # the package's own sampler, bit for bit
    prior, unc = d.data_prior.copy(), d.uncertainty.copy()
    d.scale, d.shift, d.activated, d.data = 2.0, 0.5, True, prior * 2
    d.data_prior *= 2.0
    d.uncertainty *= 4.0
    d.reset()
    assert np.array_equal(d.data_prior, prior, equal_nan=True) and np.array_equal(d.uncertainty, unc)
    assert (d.scale, d.shift, d.activated, d.data) == (1, 0, False, None)
    NMP.assert_values(d.uncertainty_update, want["uncertainty_update"], 1e-13, "Depth.reset().uncertainty_update",
                      scale=NMP.kps_local_scale(want["uncertainty"], item["kps"], item["sx"], item["sy"]))
    assert Depth(dict(use_continuity=False), depth_dict=ddict, camera=cam, kps=item["kps"]).continuity_mask is None

    meta, item, want = nc["j_flip_equal"]
    ncam = _camera(item["size"])
    ndict = {k: item[k] for k in ("normals", "normals2", "normals_variance", "normals2_variance")}
    before = {k: v.copy() for k, v in ndict.items()}
    n = Normals(meta["conf"], normals_dict=ndict, camera=ncam, mask=item["mask"], continuity_mask=item["continuity_mask"])
    assert all(np.array_equal(before[k], ndict[k]) for k in before)  # the variances are not scaled in place
    _check_normals("Normals(j_flip_equal)", dict((k, getattr(n, k)) for k in NMP.NORMALS_OUT), want, True)
    assert n.data.dtype == n.uncertainty.dtype == np.float64 and n.uncertainty.shape == item["size"] + (3, 3)

    # many images, one call of each entry point; the normals take the depth's continuity mask
    rng = np.random.default_rng(3)
    items = []
    for shape in ((20, 28), (35, 49), (12, 16)):
        m = NMP.normal_maps(rng, shape, np.full(shape, 0.1))
        dm = NMP.depth_maps(rng, shape, second=False)
        items.append(dict(depth_dict=dm, normals_dict={k: m[k] for k in ("normals", "normals_variance")}, camera=_camera((20, 28)),
                          kps=rng.uniform(0, 270, (15, 2)), mask=rng.uniform(size=(9, 9)) > 0.1))
    built = prepare_mono_priors(items)
    assert len(built) == 3
    for it, (dep, nor) in zip(items, built):
        one = Depth(None, depth_dict=it["depth_dict"], camera=it["camera"], kps=it["kps"], mask=it["mask"])
        assert isinstance(dep, Depth) and isinstance(nor, Normals)
        assert all(np.array_equal(getattr(dep, k), getattr(one, k)) for k in NMP.DEPTH_OUT)
        none = Normals(None, normals_dict=it["normals_dict"], camera=it["camera"], mask=it["mask"], continuity_mask=dep.continuity_mask)
        assert all(np.array_equal(getattr(nor, k), getattr(none, k), equal_nan=True) for k in NMP.NORMALS_OUT)
        assert np.all(nor.uncertainty[~dep.continuity_mask] == 1e6) and (~dep.continuity_mask).any()
        flat = dict(it["depth_dict"], size=(20, 28), kps=it["kps"], mask=it["mask"], sx=it["camera"].sx, sy=it["camera"].sy)
        _check_depth("prepare_mono_priors", dict((k, getattr(dep, k)) for k in NMP.DEPTH_OUT), NMP.depth_priors(flat, {}), flat)


def test_depth_object_feeds_the_integration():
    """`Depth` objects built from the maps of the 24x32 integration case, fed to integrate_depth.
    1. Built from the case's prior and variance alone, the object's maps are the hand-built ones bit for bit, and with the
       case's validity mask the solve returns the case's stored result, to the bounds of test_gpu_integration.test_golden_case
       (depth rtol 2e-4, energies rtol 1e-6).
    2. Built with the case's validity map as well, the object differs from the hand-built maps in ONE documented way: the
       reference's `uncertainty[~valid] = 1e6` (depth.py:121), which the hand-built case does not apply and which enters the
       solve (the data term reads the variance at every pixel).  That solve is checked against the CPU oracle on hand-built
       maps with the same rule, to the bounds test_gpu_integration uses between HIP and oracle (energies rtol 1e-6, depth
       rtol 2e-4); how far it moves from the stored result is printed (DESIGN.md 4o records it)."""
    from mpsfm_amd.sfm.scene.image import Depth
    from oracle import integration_oracle as IO

    z = np.load(os.path.join(GOLDEN, "integration_case_24x32.npz"))
    cam = _camera((24, 32), image=(240.0, 320.0))
    valid = z["valid"].astype(bool)
    assert (~valid).any()
    nu = z["normals_uncertainty"]
    nvar = np.stack([nu[..., 0, 0], nu[..., 1, 1], nu[..., 2, 2]], -1)
    rest = (z["normals"], nvar, z["depth_init"], tuple(z["K"]), z["kps"], z["depth3d"], z["zvars3d"])
    conf = dict(depth_uncertainty=None)  # the variance map as it is (clipped at inherent_noise^2, below every entry here)

    d = Depth(conf, depth_dict=dict(depth=z["depth_prior"], depth_variance=z["depth_uncertainty"]), camera=cam, kps=z["kps"] / cam.sx)
    assert np.array_equal(d.data_prior, z["depth_prior"]) and np.array_equal(d.uncertainty, z["depth_uncertainty"]) and d.valid.all()
    got, s, *_ = capi.integrate_depth(d.data_prior, d.uncertainty, d.valid & valid, *rest)
    assert got is not None
    np.testing.assert_allclose(got, z["out_depth"], rtol=2e-4)
    np.testing.assert_allclose(s["energies"], z["energies"], rtol=1e-6)

    dv = Depth(conf, depth_dict=dict(depth=z["depth_prior"], depth_variance=z["depth_uncertainty"], valid=valid), camera=cam, kps=z["kps"] / cam.sx)
    assert np.array_equal(dv.data_prior, z["depth_prior"]) and np.array_equal(dv.valid, valid)
    assert np.array_equal(dv.uncertainty[valid], z["depth_uncertainty"][valid]) and np.all(dv.uncertainty[~valid] == 1e6)
    got_v, s_v, *_ = capi.integrate_depth(dv.data_prior, dv.uncertainty, dv.valid, *rest)
    hand = IO.IntInputs(depth_prior=z["depth_prior"], depth_uncertainty=np.where(valid, z["depth_uncertainty"], 1e6), valid=valid,
                        normals=z["normals"], normals_uncertainty=nu, depth_init=z["depth_init"], K=tuple(z["K"]), kps=z["kps"],
                        depth3d=z["depth3d"], zvars3d=z["zvars3d"])
    want_v, changed, _, info = IO.integrate(hand)
    assert changed and got_v is not None and len(s_v["energies"]) == len(info["energies"])
    np.testing.assert_allclose(s_v["energies"], info["energies"], rtol=1e-6)
    np.testing.assert_allclose(got_v, want_v, rtol=2e-4)
    print("1e6 at invalid pixels moves the integrated depth by at most", float(np.max(np.abs(got_v / got - 1))), "(relative);",
          "at valid pixels by", float(np.max(np.abs(got_v / got - 1)[valid])))


def test_non_integer_downscale_factor():
    """`int(W // f)` with f = 1.1: 77 // 1.1 is 69, not floor(77 / 1.1) = 70.  The half-size maps have Python's shape and
    equal the restatement."""
    rng = np.random.default_rng(8)
    m = NMP.normal_maps(rng, (9, 40), np.full((9, 40), 0.1))
    item = dict(normals=m["normals"], normals_variance=m["normals_variance"], size=(11, 77))
    conf = dict(NMP.NORMALS_CONF, downscale_factor=1.1)
    got = capi.normal_priors([item], conf)[0]
    assert got["data_downscaled"].shape == (9, 69, 3) and got["uncertainty_downscaled"].shape == (9, 69, 3, 3)
    _check_normals("downscale_factor 1.1", got, NMP.normal_priors(item, conf), False)


def test_medium_batch_against_the_restatement():
    """7 images of 96x128 -> 58x77 in one call of each entry point, flip_consistency with predicted variances"""
    rng = np.random.default_rng(20261019)
    src, dst, n = (96, 128), (58, 77), 7
    cam = _camera(dst, image=(580.0, 770.0))
    stats = [0, 0]
    ditems, nitems = [], []
    for k in range(n):
        dm = NMP.depth_maps(rng, src)
        if k % 2:
            dm["valid"] = rng.uniform(size=src) > 0.05
        if k % 3 == 0:
            dm["depth"][rng.uniform(size=src) < 0.01] = 0.0
        ditems.append(dict(dm, size=dst, kps=rng.uniform(-20, 790, (50, 2)), sx=cam.sx, sy=cam.sy, mask=(rng.uniform(size=(40, 40)) > 0.1) if k % 2 == 0 else None))
        nm = NMP.guarded_normals(rng, src, dst, 2, stats)
        nitems.append(dict(nm, size=dst, mask=ditems[-1]["mask"]))
    assert stats[0] / stats[1] < 0.2
    dconf = dict(NMP.DEPTH_CONF, flip_consistency=True, depth_lim=6.5)
    nconf = dict(NMP.NORMALS_CONF, flip_consistency=True, prior_std_multiplier=1.5, lc_std_multiplier=2)
    dgot = capi.depth_priors(ditems, dconf)
    for it, g in zip(nitems, dgot):
        it["continuity_mask"] = g["continuity_mask"]
    ngot = capi.normal_priors(nitems, nconf)
    for k in range(n):
        _check_depth(f"medium depth {k}", dgot[k], NMP.depth_priors(ditems[k], dconf), ditems[k])
        _check_normals(f"medium normals {k}", ngot[k], NMP.normal_priors(nitems[k], nconf), True)
    plain = [dict(normals=it["normals"], normals_variance=it["normals_variance"], size=dst) for it in nitems]
    for k, g in enumerate(capi.normal_priors(plain, NMP.NORMALS_CONF)):
        _check_normals(f"medium normals (no flip) {k}", g, NMP.normal_priors(plain[k], NMP.NORMALS_CONF), False)
