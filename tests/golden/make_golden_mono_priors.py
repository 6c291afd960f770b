"""Fixture for the prior construction (tests/golden/reference_mono_priors.npz), computed BY THE REFERENCE'S OWN CODE:

  by file path   mpsfm/sfm/scene/image/depth.py     Depth._init (with image/utils.py get_continuity_mask and
                                                    image/mixins/priorutils.py PriorUtils.uncertainty_at_kps)
                 mpsfm/sfm/scene/image/normals.py   Normals._init and the module functions it calls

The two modules import `mpsfm.baseclass` (needs omegaconf) and `cv2`; neither is available, so both are replaced by stub
modules before the import: a BaseClass that merges `default_conf` with the passed settings and calls `_init`, and a cv2
whose `resize` follows the rule of DESIGN.md 4o (bilinear: mpsfm_amd.sfm.scene.integration.resize_linear per channel, a
copy at equal sizes; a map that holds a NaN - the normalised normals of the zero-length case on their way to half size -
goes through the two-tap form tests/numpy_mono_priors.resize_linear, because the matrix product would spread the NaN
over its row and column; INTER_NEAREST: source index min(floor(i n_src / n_dst), n_src - 1)).  The package `mpsfm.sfm.scene.image` is entered as a bare namespace: its
__init__ imports the whole image stack.

The file holds settings, inputs and outputs only (masks packed with np.packbits).  Value maps are float32-representable;
they are stored as float32 and fed as float64, so the reference computes in fp64, except in the float32 cases (f), (g),
of which only the masks are kept.  Maps that are resized hold no NaN.

For the flip_consistency cases of the normals, pixels are redrawn until numpy_mono_priors.flip_guard holds at full and at
half size (arccos arguments at least 1e-4 from +-1, |n_y| >= 1e-6, no angle difference within 1e-9 of +-pi); the share
of redrawn source pixels is stored as `redraw_share` and must stay under 20 %.

Run in the build container:  python tests/golden/make_golden_mono_priors.py
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_reference import REF, ROOT, load_by_path  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy_mono_priors as NMP  # noqa: E402
from mpsfm_amd.sfm.scene.integration import resize_linear as package_resize_linear  # noqa: E402

TARGET = (20, 28)          # (int_height, int_width) of every resized case
NORMALS_TARGET = (14, 20)  # the 3x3 covariances are nine doubles a pixel
IMAGE = (200.0, 280.0)     # (height, width) of the camera: sx = sy = 0.1 at TARGET


# ---- stubs -----------------------------------------------------------------------------------------------------------
class _Conf(dict):
    __getattr__ = dict.__getitem__


def install_stubs():
    cv2 = types.ModuleType("cv2")
    cv2.INTER_NEAREST = 0
    cv2.INTER_LINEAR = 1

    def resize(img, dsize, interpolation=1):
        size = (int(dsize[1]), int(dsize[0]))
        if interpolation == cv2.INTER_NEAREST:
            return NMP.resize_nearest(img, size)
        img = np.asarray(img, np.float64)
        if img.shape[:2] == size:
            return img.copy()
        if not np.isfinite(img).all():  # the matrix product would spread a NaN over its row and column: two taps, like OpenCV
            return NMP.resize_linear(img, size)
        if img.ndim == 2:
            return package_resize_linear(img, dsize)
        return np.stack([package_resize_linear(img[..., c], dsize) for c in range(img.shape[2])], -1)

    cv2.resize = resize
    sys.modules["cv2"] = cv2

    base = types.ModuleType("mpsfm.baseclass")

    class BaseClass:
        default_conf = {}

        def __init__(self, conf=None, *args, **kwargs):
            self.conf = _Conf(dict(self.default_conf), **dict(conf or {}))
            self._init(*args, **kwargs)

    base.BaseClass = BaseClass
    sys.modules["mpsfm.baseclass"] = base
    pkg = types.ModuleType("mpsfm.sfm.scene.image")
    pkg.__path__ = [os.path.join(REF, "mpsfm", "sfm", "scene", "image")]
    sys.modules["mpsfm.sfm.scene.image"] = pkg


def camera(size, image=IMAGE):
    return types.SimpleNamespace(int_height=size[0], int_width=size[1], sx=size[1] / image[1], sy=size[0] / image[0])


f32, depth_maps, normal_maps, guarded_normals = NMP.f32, NMP.depth_maps, NMP.normal_maps, NMP.guarded_normals


def keypoints(rng, size, sx, sy, n=40):
    H, W = size
    kps = np.stack([rng.uniform(0, W - 1, n) / sx, rng.uniform(0, H - 1, n) / sy], 1)
    kps[:8] = np.array([[0, 0], [(W - 1) / sx, 0], [0, (H - 1) / sy], [(W - 1) / sx, (H - 1) / sy], [3 / sx, 2 / sy],
                        [-0.4 / sx, 1 / sy], [(W - 0.5) / sx, (H - 0.5) / sy], [(W + 3) / sx, -5 / sy]])
    return kps


def threshold_map(rng, shape=(16, 24)):
    """neighbour ratios at 1.015 (1 +- 1e-7) along the rows, in float32-representable values"""
    H, W = shape
    d = np.empty(shape)
    d[:, 0] = 2.0
    for j in range(1, W):  # every row takes the same steps (the vertical ratios stay at 1 +- 1e-6), each with its own offset
        r = 1.015 * (1 + rng.choice([-1e-7, 1e-7, -3e-8, 3e-8, 0.0], H))
        up = rng.uniform() < 0.5 if 1.5 < d[0, j - 1] < 3.0 else d[0, j - 1] <= 1.5
        d[:, j] = d[:, j - 1] * r if up else d[:, j - 1] / r
    return f32(d)


# ---- cases -----------------------------------------------------------------------------------------------------------
def depth_cases(rng):
    T = TARGET
    sx, sy = camera(T).sx, camera(T).sy
    cases = []

    def add(name, maps, conf, size=T, kps=None, mask=None, keep=None, masks_only=False):
        cases.append(dict(name=name, maps=maps, conf=conf, size=size, kps=np.zeros((0, 2)) if kps is None else kps, mask=mask,
                          masks_only=masks_only))

    a = depth_maps(rng, T)
    both = dict(flip_consistency=True)
    add("a_default", {k: a[k] for k in ("depth", "depth_variance")}, {}, kps=keypoints(rng, T, sx, sy))          # (a), (h)
    add("b_flip_prior", a, both, kps=keypoints(rng, T, sx, sy))                                                     # (b)
    add("b_flip_only", {k: a[k] for k in ("depth", "depth2")}, dict(flip_consistency=True, prior_uncertainty=False))
    add("b_flip_only_no_du", {k: a[k] for k in ("depth", "depth2")}, dict(flip_consistency=True, prior_uncertainty=False, depth_uncertainty=None))
    add("b_flip_prior_no_du", a, dict(flip_consistency=True, depth_uncertainty=None))
    add("c_fixed", {"depth": a["depth"]}, dict(fixed_uncertainty=True, depth_uncertainty=None, prior_uncertainty=False, std_multiplier=2))  # (c), (h) empty
    add("c_variance_only", {k: a[k] for k in ("depth", "depth_variance")}, dict(depth_uncertainty=None))
    add("c_no_prior_unc", {"depth": a["depth"]}, dict(prior_uncertainty=False, std_multiplier=1.5))
    for tag, shape in (("d_half", (40, 56)), ("d_odd", (35, 49)), ("d_up", (12, 16))):                              # (d)
        m = depth_maps(rng, shape)
        m["valid"] = rng.uniform(size=shape) > 0.05
        m["valid2"] = rng.uniform(size=shape) > 0.05
        m["depth"][rng.uniform(size=shape) < 0.02] = 0.0
        add(tag, m, both if tag != "d_half" else {}, kps=keypoints(rng, T, sx, sy, 20),
            mask=(rng.uniform(size=(9, 11)) > 0.1) if tag == "d_odd" else None)
    e = depth_maps(rng, T)                                                                                           # (e)
    e["valid"] = rng.uniform(size=T) > 0.1
    e["depth"][2:4, 5:9] = 0.0
    e["depth"][10, 3:6] = -1.25
    e["depth"][15, 20] = np.nan
    add("e_masks", {k: e[k] for k in ("depth", "depth_variance", "valid")}, dict(depth_lim=5.5, max_std=0.3), kps=keypoints(rng, T, sx, sy, 20),
        mask=rng.uniform(size=(11, 13)) > 0.15)
    for src in ("a_default", "d_odd"):                                                                               # (f)
        c = next(c for c in cases if c["name"] == src)
        m32 = {k: (v.astype(np.float32) if v.dtype == np.float64 else v) for k, v in c["maps"].items()}
        add("f_" + src + "_f32", m32, c["conf"], mask=c["mask"], masks_only=True)
    g = threshold_map(rng)                                                                                           # (g)
    gv = f32(rng.uniform(0.001, 0.01, g.shape))
    add("g_threshold_f64", dict(depth=g, depth_variance=gv, depth2=np.ascontiguousarray(g[::-1])), {}, size=g.shape)
    add("g_threshold_f32", dict(depth=g.astype(np.float32), depth_variance=gv.astype(np.float32),
                                depth2=np.ascontiguousarray(g[::-1]).astype(np.float32)), {}, size=g.shape, masks_only=True)
    add("g_threshold_resized_f32", dict(depth=g.astype(np.float32), depth_variance=gv.astype(np.float32)), {}, size=(11, 17), masks_only=True)
    for shape in ((1, 1), (1, 5), (5, 1)):                                                                           # (k)
        m = depth_maps(rng, shape, second=False)
        if shape != (1, 1):
            m["depth"].ravel()[2] = f32(m["depth"].ravel()[2] * 1.2)
        add(f"k_{shape[0]}x{shape[1]}", m, {}, size=shape)
        add(f"k_{shape[0]}x{shape[1]}_f32", {k: v.astype(np.float32) for k, v in m.items()}, {}, size=shape, masks_only=True)
    add("k_1x5_to_3x7", depth_maps(rng, (1, 5), second=False), {}, size=(3, 7))
    return cases


def normal_cases(rng, stats):
    T = NORMALS_TARGET
    cases = []

    def add(name, maps, conf, size=T, mask=None, cont=None):
        cases.append(dict(name=name, maps=maps, conf=conf, size=size, mask=mask, continuity_mask=cont))

    plain = ("normals", "normals_variance")
    m = normal_maps(rng, T, np.full(T, 0.1))                                                                         # (i)
    m["normals"][4, 6] = 0.0  # a zero-length normal: NaN
    add("i_equal", {k: m[k] for k in plain}, {})
    m = normal_maps(rng, (25, 35), np.full((25, 35), 0.1))
    add("i_odd", {k: m[k] for k in plain}, dict(std_multiplier=2), mask=rng.uniform(size=T) > 0.1)
    m = normal_maps(rng, (28, 40), np.full((28, 40), 0.1))
    add("i_half", {k: m[k] for k in plain}, {})
    add("j_flip_equal", guarded_normals(rng, T, T, 2, stats), dict(flip_consistency=True, prior_std_multiplier=1.5, lc_std_multiplier=2),   # (j)
        mask=rng.uniform(size=(11, 13)) > 0.1, cont=rng.uniform(size=T) > 0.1)
    add("j_flip_odd", guarded_normals(rng, (25, 35), T, 2, stats), dict(flip_consistency=True, std_multiplier=2), cont=rng.uniform(size=T) > 0.1)
    add("j_flip_up", guarded_normals(rng, (8, 12), (15, 21), 3, stats), dict(flip_consistency=True, downscale_factor=3, lc_std_multiplier=0.5),
        size=(15, 21))
    add("k_2x2", {k: normal_maps(rng, (2, 2), np.full((2, 2), 0.1))[k] for k in plain}, {}, size=(2, 2))           # (k): smallest with a half size
    add("k_1x5_to_2x6", {k: normal_maps(rng, (1, 5), np.full((1, 5), 0.1))[k] for k in plain}, {}, size=(2, 6))
    return cases


DEPTH_OUT = ("data_prior", "uncertainty", "valid", "continuity_mask", "uncertainty_update")
NORMAL_OUT = ("data", "uncertainty", "data_downscaled", "uncertainty_downscaled")


def store(out, key, a):
    a = np.asarray(a)
    if a.dtype == np.bool_:
        out[key + "__bits"] = np.packbits(a.ravel())
        out[key + "__shape"] = np.array(a.shape, np.int32)
    else:
        out[key] = a


def generate():
    install_stubs()
    Depth = load_by_path("ref_depth", "mpsfm/sfm/scene/image/depth.py").Depth
    Normals = load_by_path("ref_normals", "mpsfm/sfm/scene/image/normals.py").Normals
    rng = np.random.default_rng(20261019)
    out = {"depth_default_conf": json.dumps(dict(Depth.default_conf)), "normals_default_conf": json.dumps(dict(Normals.default_conf))}
    meta = {"depth": [], "normals": []}
    for c in depth_cases(rng):
        name = "depth_" + c["name"]
        cam = camera(c["size"], IMAGE if c["size"] == TARGET else (c["size"][0] * 10.0, c["size"][1] * 10.0))
        maps = {k: v.copy() for k, v in c["maps"].items()}
        with np.errstate(all="ignore"):
            d = Depth(c["conf"], depth_dict=maps, camera=cam, kps=c["kps"], mask=None if c["mask"] is None else c["mask"].copy())
        if not hasattr(d, "continuity_mask"):  # unset without a resize (depth.py:105-112): taken from the same functions
            U = sys.modules["mpsfm.sfm.scene.image.utils"]
            d.continuity_mask = U.get_continuity_mask(c["maps"]["depth"])
            if "depth2" in c["maps"]:
                d.continuity_mask = d.continuity_mask & U.get_continuity_mask(c["maps"]["depth2"])
        for k, v in c["maps"].items():
            store(out, f"{name}_in_{k}", v.astype(np.float32) if v.dtype == np.float64 else v)  # exact: float32 values
        if c["mask"] is not None:
            store(out, f"{name}_in_mask", c["mask"])
        out[f"{name}_in_kps"] = c["kps"]
        out[f"{name}_in_sxsy"] = np.array([cam.sx, cam.sy])
        for k in DEPTH_OUT:
            if c["masks_only"] and k not in ("valid", "continuity_mask"):
                continue
            store(out, f"{name}_out_{k}", np.asarray(getattr(d, k)))
        meta["depth"].append(dict(name=c["name"], conf=c["conf"], size=list(c["size"]), masks_only=c["masks_only"],
                                  float32=bool(c["maps"]["depth"].dtype == np.float32)))
        print(f"{name}: valid {int(np.sum(d.valid))}/{d.valid.size}, continuous {int(np.sum(d.continuity_mask))}")
    stats = [0, 0]
    for c in normal_cases(rng, stats):
        name = "normals_" + c["name"]
        cam = camera(c["size"])
        maps = {k: v.copy() for k, v in c["maps"].items()}
        with np.errstate(all="ignore"):
            nobj = Normals(c["conf"], normals_dict=maps, camera=cam, mask=None if c["mask"] is None else c["mask"].copy(),
                           continuity_mask=None if c["continuity_mask"] is None else c["continuity_mask"].copy())
        for k, v in c["maps"].items():
            store(out, f"{name}_in_{k}", v.astype(np.float32))
        for k in ("mask", "continuity_mask"):
            if c[k] is not None:
                store(out, f"{name}_in_{k}", c[k])
        for k in NORMAL_OUT:
            store(out, f"{name}_out_{k}", np.asarray(getattr(nobj, k), np.float64))
        meta["normals"].append(dict(name=c["name"], conf=c["conf"], size=list(c["size"])))
        print(f"{name}: NaN entries {int(np.isnan(nobj.uncertainty).sum())}, 1e6 pixels {int(np.sum(nobj.uncertainty[..., 0, 0] == 1e6))}")
    share = stats[0] / max(stats[1], 1)
    print(f"flip cases: {stats[0]} of {stats[1]} source pixels redrawn ({100 * share:.2f} %)")
    assert share < 0.2, share
    out["redraw_share"] = share
    out["cases"] = json.dumps(meta)
    return out


if __name__ == "__main__":
    assert os.path.isdir(REF), REF
    out = generate()
    path = os.path.join(HERE, "reference_mono_priors.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")
