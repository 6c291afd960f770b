"""NumPy restatement of the prior construction: the depth prior, its uncertainty, validity and continuity
masks, and the normal prior with its 3x3 covariances at full and half size.  Test scaffolding, written from the rules in
DESIGN.md; the reference's own results are in tests/golden/reference_mono_priors.npz.

Resizing is tap based (two taps per axis, a tap of zero weight is not read), so a NaN stays local; on finite maps it
equals `mpsfm_amd.sfm.scene.integration.resize_linear`.
"""

from __future__ import annotations

import numpy as np

from mpsfm_amd.sfm.scene.priorutils import bilinear_at_kps

DEPTH_CONF = dict(inherent_noise=0.02, std_multiplier=1, lc_std_multiplier=10, prior_std_multiplier=3.33, max_std=None,
                  use_continuity=True, depth_lim=None, fixed_uncertainty_val=0.03, fixed_uncertainty=False, fill=True,
                  prior_uncertainty=True, flip_consistency=False, depth_uncertainty=0.0263, verbose=0)
NORMALS_CONF = dict(inherent_polar_noise=np.pi / 180, std_multiplier=1, lc_std_multiplier=1, prior_std_multiplier=1,
                    downscale_factor=2, prior_uncertainty=True, flip_consistency=False, verbose=0)
LARGE = 1e6


# ---- resize rules ---------------------------------------------------------------------------------------------------
def linear_taps(n_src, n_dst):
    """(lo, hi, frac) per destination index: sample position (i + 0.5) (n_src / n_dst) - 0.5, replicated border,
    fraction rounded to float32"""
    pos = (np.arange(n_dst) + 0.5) * (1.0 / (n_dst / n_src)) - 0.5
    lo = np.floor(pos).astype(int)
    frac = (pos - lo).astype(np.float32).astype(np.float64)
    frac[(lo < 0) | (lo >= n_src - 1)] = 0.0
    lo = np.clip(lo, 0, n_src - 1)
    return lo, np.minimum(lo + 1, n_src - 1), frac


def _blend(a, b, f):
    """(1 - f) a + f b, with b unread where f == 0"""
    with np.errstate(invalid="ignore"):
        return np.where(f == 0.0, a, (1.0 - f) * a + f * np.where(f == 0.0, 0.0, b))


def resize_linear(img, size):
    """size = (H, W); [h, w] or [h, w, c] -> [H, W(, c)], rows first, then columns; equal sizes copy"""
    img = np.asarray(img, np.float64)
    if img.shape[:2] == tuple(size):
        return img.copy()
    ylo, yhi, fy = linear_taps(img.shape[0], size[0])
    xlo, xhi, fx = linear_taps(img.shape[1], size[1])
    ex = (slice(None),) + (None,) * (img.ndim - 1)
    rows = _blend(img[ylo], img[yhi], fy[ex])
    ex = (None, slice(None)) + (None,) * (img.ndim - 2)
    return _blend(rows[:, xlo], rows[:, xhi], fx[ex])


def resize_mask(mask, size):
    """`resize(mask.astype(float)) == 1`: true iff every tap of non-zero weight is true"""
    mask = np.asarray(mask, bool)
    if mask.shape == tuple(size):
        return mask.copy()
    ylo, yhi, fy = linear_taps(mask.shape[0], size[0])
    xlo, xhi, fx = linear_taps(mask.shape[1], size[1])
    rows = mask[ylo] & (mask[yhi] | (fy == 0.0)[:, None])
    return rows[:, xlo] & (rows[:, xhi] | (fx == 0.0)[None])


def resize_nearest(mask, size):
    """source index min(floor(i n_src / n_dst), n_src - 1)"""
    mask = np.asarray(mask)
    if mask.shape == tuple(size):
        return mask.copy()
    ys = np.minimum(np.arange(size[0]) * mask.shape[0] // size[0], mask.shape[0] - 1)
    xs = np.minimum(np.arange(size[1]) * mask.shape[1] // size[1], mask.shape[1] - 1)
    return mask[ys][:, xs]


# ---- depth -----------------------------------------------------------------------------------------------------------
def continuity_mask(depth):
    """in the map's own precision: float32 division and the float32 value of 1.015 for a float32 map"""
    depth = np.asarray(depth)
    T = depth.dtype.type
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = T(1) / np.where(depth < T(1e-6), T(1e-6), depth)
        thr = T(1.015)
        cont = np.ones(depth.shape, bool)
        h = ~((inv[:, 1:] / inv[:, :-1] > thr) | (inv[:, :-1] / inv[:, 1:] > thr))
        v = ~((inv[1:, :] / inv[:-1, :] > thr) | (inv[:-1, :] / inv[1:, :] > thr))
    cont[:, 1:] &= h
    cont[:, :-1] &= h
    cont[1:, :] &= v
    cont[:-1, :] &= v
    return cont


def depth_priors(item, conf):
    """item: depth, [depth2, depth_variance, depth_variance2, valid, valid2, mask], size (H, W), kps, sx, sy"""
    c = dict(DEPTH_CONF, **conf)
    raw = {k: np.asarray(item[k]) for k in ("depth", "depth2", "depth_variance", "depth_variance2") if item.get(k) is not None}
    f = {k: v.astype(np.float64) for k, v in raw.items()}
    flip, pu = c["flip_consistency"], c["prior_uncertainty"]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if flip and not pu:
            mews, vs = [(f["depth2"] + f["depth"]) / 2], [(f["depth"] - f["depth2"]) ** 2]
        elif flip:
            mews, vs = [f["depth"], f["depth2"]], [f["depth_variance"], f["depth_variance2"]]
        elif pu:
            mews, vs = [f["depth"]], [f["depth_variance"]]
        else:
            mews, vs = [f["depth"]], []
        isum = lambda terms: sum(terms[1:], 0 + terms[0])  # noqa: E731  left to right, like sum()
        prior = isum([m / (v + 1e-6) for m, v in zip(mews, vs)]) / (isum([1 / (v + 1e-6) for v in vs]) + 1e-6) if len(mews) > 1 else mews[0]
        du, psm2 = c["depth_uncertainty"], c["prior_std_multiplier"] ** 2
        if du is not None:
            if pu:
                nv = [np.maximum(v * psm2, (m * du) ** 2) for m, v in zip(mews, vs)]
                unc = 1 / (isum([1 / (v + 1e-6) for v in nv]) + 1e-6) if len(nv) > 1 else nv[0]
            else:
                unc = (prior * du) ** 2
        elif flip:
            unc = (1 / (isum([1 / (v + 1e-6) for v in vs]) + 1e-6)) * psm2
        elif c["fixed_uncertainty"]:
            unc = np.ones_like(mews[0]) * c["fixed_uncertainty_val"] * c["std_multiplier"] ** 2
        else:
            assert len(vs) == 1
            unc = vs[0]
        unc = np.maximum(unc, c["inherent_noise"] ** 2)
        if c["max_std"] is not None:
            unc = np.minimum(unc, c["max_std"] ** 2)
        unc = unc * c["std_multiplier"] ** 2
        valid = raw["depth"] > 0
    for k in ("valid", "valid2"):
        if item.get(k) is not None:
            valid = valid & np.asarray(item[k], bool)
    cont = np.ones(valid.shape, bool)
    if c["use_continuity"]:
        cont = continuity_mask(raw["depth"])
        if "depth2" in raw:
            cont &= continuity_mask(raw["depth2"])
    size = tuple(int(x) for x in item["size"])
    prior, unc = resize_linear(prior, size), resize_linear(unc, size)
    valid, cont = resize_mask(valid, size), resize_mask(cont, size)
    if item.get("mask") is not None:
        valid = valid & resize_nearest(np.asarray(item["mask"]) != 0, size)
    unc[~valid] = LARGE
    zero = prior == 0
    prior[zero] = 0.1
    valid[zero] = False
    if c["depth_lim"] is not None:
        with np.errstate(invalid="ignore"):
            valid[prior > c["depth_lim"]] = False
    kps = np.asarray(item.get("kps", np.zeros((0, 2))), np.float64).reshape(-1, 2)
    upd = bilinear_at_kps(unc, kps, item["sx"], item["sy"]) if len(kps) else np.zeros(0)
    return dict(data_prior=prior, uncertainty=unc, valid=valid, continuity_mask=cont, uncertainty_update=upd)


# ---- normals ---------------------------------------------------------------------------------------------------------
def _unit(n):
    with np.errstate(divide="ignore", invalid="ignore"):
        return n / np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])[..., None]


def _jacobian(theta, phi):
    ct, cp, st, sp = np.cos(theta), np.cos(phi), np.sin(theta), np.sin(phi)
    J = np.zeros(theta.shape + (3, 2))
    J[..., 0, 0], J[..., 0, 1] = ct * cp, -st * sp
    J[..., 1, 0], J[..., 1, 1] = ct * sp, st * cp
    J[..., 2, 0] = -st
    return J


def _jcjt(J, a, b, c):
    """(J C) J^T with C = [[a, b], [b, c]], written out so that NaN / inf entries behave as in the element formulas"""
    M = np.stack([J[..., 0] * a[..., None] + J[..., 1] * b[..., None], J[..., 0] * b[..., None] + J[..., 1] * c[..., None]], -1)
    return M[..., :, None, 0] * J[..., None, :, 0] + M[..., :, None, 1] * J[..., None, :, 1]


def _spherical(n):
    n = _unit(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([np.arccos(n[..., 2]), np.sign(n[..., 1]) * np.arccos(n[..., 0] / (1e-6 + np.sqrt(n[..., 0] ** 2 + n[..., 1] ** 2)))], -1)


def _diff_angle(a, b):
    d = np.abs(a - b)
    return np.minimum(d, 2 * np.pi - d)


def flip_guard(n1, n2):
    """True where the two-view covariance of unit normals n1, n2 is well conditioned: both arccos arguments at least
    1e-4 from +-1, |n_y| >= 1e-6, no angle difference within 1e-9 of +-pi (the fixtures redraw the other pixels)."""
    ok = np.ones(n1.shape[:-1], bool)
    sph = []
    for n in (_unit(n1), _unit(n2)):
        arg = n[..., 0] / (1e-6 + np.sqrt(n[..., 0] ** 2 + n[..., 1] ** 2))
        ok &= (1 - np.abs(n[..., 2]) >= 1e-4) & (1 - np.abs(arg) >= 1e-4) & (np.abs(n[..., 1]) >= 1e-6)
        sph.append(_spherical(n))
    diff = sph[1] - sph[0]
    return ok & np.all(np.abs(np.abs(diff) - np.pi) > 1e-9, -1)


def normal_cov(c, n1, n2, v1, v2):
    """mean normal and covariance before std_multiplier^2 and the fills"""
    if not c["flip_consistency"]:
        v = v1.astype(np.float32).astype(np.float64)
        return n1, _jcjt(_jacobian(n1[..., 0], n1[..., 1]), v, np.zeros_like(v), v)
    data = _unit((n2 + n1) / 2)
    s1, s2 = _spherical(n1), _spherical(n2)
    diff = s2 - s1
    s2 = np.where(diff > np.pi, s2 - 2 * np.pi, s2)
    s2 = np.where(diff < -np.pi, s2 + 2 * np.pi, s2)
    mean = (s1 + s2) / 2
    d1, d2 = _diff_angle(s1, mean), _diff_angle(s2, mean)
    diag = np.maximum(d1 ** 2 + d2 ** 2, 0)
    a, cc = diag[..., 0], diag[..., 1]
    b = d1[..., 0] * d1[..., 1] + d2[..., 0] * d2[..., 1]
    # closed-form symmetric 2x2 eigen-decomposition, eigenvalues clamped at the (unsquared) noise
    hm, hd = (a + cc) / 2, (a - cc) / 2
    r = np.sqrt(hd * hd + b * b)
    l1, l2 = np.maximum(hm + r, c["inherent_polar_noise"]), np.maximum(hm - r, c["inherent_polar_noise"])
    t = 0.5 * np.arctan2(2 * b, a - cc)
    ce, se = np.cos(t), np.sin(t)
    a, cc, b = l1 * ce * ce + l2 * se * se, l1 * se * se + l2 * ce * ce, (l1 - l2) * ce * se
    lc2, psm2 = c["lc_std_multiplier"] ** 2, c["prior_std_multiplier"] ** 2
    a, b, cc = a * lc2, b * lc2, cc * lc2
    for v in (v1, v2):
        a, cc = np.maximum(a, v * psm2), np.maximum(cc, v * psm2)
    U = _jcjt(_jacobian(mean[..., 0], mean[..., 1]), a, b, cc)
    for k in range(3):
        U[..., k, k] = np.maximum(U[..., k, k], 0)
    return data, U


def normal_priors(item, conf):
    """item: normals [h,w,3], normals_variance, [normals2, normals2_variance, mask, continuity_mask], size (H, W)"""
    c = dict(NORMALS_CONF, **conf)
    flip = c["flip_consistency"]
    H, W = (int(x) for x in item["size"])
    half = (int(H // c["downscale_factor"]), int(W // c["downscale_factor"]))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        n1 = _unit(resize_linear(item["normals"], (H, W)))
        v1 = resize_linear(item["normals_variance"], (H, W))
        d1, dv1 = _unit(resize_linear(n1, half)), resize_linear(v1, half)
        n2 = v2 = d2 = dv2 = None
        if flip:
            n2 = _unit(resize_linear(item["normals2"], (H, W)))
            v2 = resize_linear(item["normals2_variance"], (H, W))
            d2, dv2 = _unit(resize_linear(n2, half)), resize_linear(v2, half)
        data, U = normal_cov(c, n1, n2, v1, v2)
        data_d, U_d = normal_cov(c, d1, d2, dv1, dv2)
        U, U_d = U * c["std_multiplier"] ** 2, U_d * c["std_multiplier"] ** 2
    if item.get("mask") is not None:
        U[~resize_nearest(np.asarray(item["mask"]) != 0, (H, W))] = LARGE
    if item.get("continuity_mask") is not None:
        U[~np.asarray(item["continuity_mask"], bool)] = LARGE
    return dict(data=data, uncertainty=U, data_downscaled=data_d, uncertainty_downscaled=U_d)


# ---- the reference fixture (tests/golden/reference_mono_priors.npz) -------------------------------------------------
DEPTH_IN = ("depth", "depth2", "depth_variance", "depth_variance2", "valid", "valid2", "mask")
NORMALS_IN = ("normals", "normals2", "normals_variance", "normals2_variance", "mask", "continuity_mask")
DEPTH_OUT = ("data_prior", "uncertainty", "valid", "continuity_mask", "uncertainty_update")
NORMALS_OUT = ("data", "uncertainty", "data_downscaled", "uncertainty_downscaled")


def _fetch(z, key):
    if key + "__bits" in z:
        shape = tuple(z[key + "__shape"])
        return np.unpackbits(z[key + "__bits"])[: int(np.prod(shape))].astype(bool).reshape(shape)
    return z[key] if key in z else None


def fixture_cases(z, kind):
    """[(meta, item, expected)] of the 'depth' or 'normals' cases; value maps come back as float64 unless the case is a
    float32 one"""
    import json

    out = []
    for meta in json.loads(str(z["cases"]))[kind]:
        pre = f"{kind}_{meta['name']}"
        item = {}
        for k in DEPTH_IN if kind == "depth" else NORMALS_IN:
            a = _fetch(z, f"{pre}_in_{k}")
            if a is not None:
                item[k] = a if a.dtype == bool or meta.get("float32") else a.astype(np.float64)
        item["size"] = tuple(meta["size"])
        if kind == "depth":
            item["kps"] = z[f"{pre}_in_kps"]
            item["sx"], item["sy"] = (float(v) for v in z[f"{pre}_in_sxsy"])
        want = {k: _fetch(z, f"{pre}_out_{k}") for k in (DEPTH_OUT if kind == "depth" else NORMALS_OUT)}
        out.append((meta, item, {k: v for k, v in want.items() if v is not None}))
    return out


def kps_local_scale(unc, kps, sx, sy):
    """Per keypoint the largest |uncertainty| among the pixels around its sample position (3 x 3 around the rounded
    position, which holds the four bilinear taps): the scale a sample's rounding error goes with.  A sample next to a 1e6
    fill is conditioned by 1e6, one among ordinary variances by those; 0 for a keypoint outside the map."""
    unc = np.abs(np.asarray(unc, np.float64))
    H, W = unc.shape
    pad = np.zeros((H + 4, W + 4))
    pad[2:-2, 2:-2] = np.where(np.isnan(unc), 0.0, unc)
    kps = np.asarray(kps, np.float64).reshape(-1, 2)
    x = np.clip(np.round(kps[:, 0] * sx), -2, W + 1).astype(int) + 2
    y = np.clip(np.round(kps[:, 1] * sy), -2, H + 1).astype(int) + 2
    out = np.zeros(len(kps))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            out = np.maximum(out, pad[np.clip(y + dy, 0, H + 3), np.clip(x + dx, 0, W + 3)])
    return out


def assert_values(got, want, rel, what, per_pixel=0, scale=None):
    """NaN where the reference has NaN, the 1e6 / 0.1 fills exact, everything else within rel of the largest magnitude
    of the array's other entries (per_pixel = n: of each pixel's, the last n axes being one pixel; scale: an explicit
    per-element scale, for samples whose conditioning differs from element to element)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern differs"
    fill = (want == LARGE) | (want == 0.1)
    assert np.array_equal(got[fill], want[fill]), f"{what}: fills differ"
    rest = ~fill & ~np.isnan(want)
    if not rest.any():
        return 0.0
    mag = np.where(rest, np.abs(want), 0.0)
    if scale is not None:
        scale = np.broadcast_to(np.asarray(scale, np.float64), want.shape)
    elif per_pixel:
        axes = tuple(range(want.ndim - per_pixel, want.ndim))
        scale = np.broadcast_to(mag.max(axis=axes, keepdims=True), want.shape)
    else:
        scale = np.full(want.shape, mag.max())
    err = np.abs(got - want)[rest] / np.maximum(scale[rest], np.finfo(float).tiny)
    worst = float(err.max())
    print(f"{what}: worst relative error {worst:.3e} (bound {rel:.0e})")
    assert worst <= rel, f"{what}: {worst:.3e} > {rel:.0e}"
    return worst


# ---- seeded inputs (shared by the fixture maker and the GPU tests) ---------------------------------------------------
def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def depth_maps(rng, shape, second=True):
    """a slanted surface with a step (so the continuity mask is not trivial), its flipped estimate and variances"""
    H, W = shape
    y, x = np.mgrid[0:H, 0:W]
    d = 4.0 + 0.03 * x + 0.02 * y + rng.normal(0, 0.004, shape)
    d[:, W // 2:] *= 1.3
    d = d * np.where(rng.uniform(size=shape) < 0.03, 1.1, 1.0)  # isolated spikes
    out = dict(depth=f32(d), depth_variance=f32((rng.uniform(0.005, 0.08, shape) * d) ** 2))
    if second:
        out["depth2"] = f32(d * (1 + rng.normal(0, 0.002, shape)))
        out["depth_variance2"] = f32((rng.uniform(0.005, 0.08, shape) * d) ** 2)
    return out


def normal_maps(rng, shape, spread):
    H, W = shape
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([0.6 * np.sin(x / 7.0) + 0.2, 0.5 * np.cos(y / 5.0) + 0.25, -np.ones(shape)], -1)
    n1 = base + rng.normal(0, 0.15, shape + (3,))
    n2 = n1 + rng.normal(0, 1.0, shape + (3,)) * spread[..., None]
    scale = rng.uniform(0.8, 1.2, shape + (1,))  # the maps arrive unnormalised
    return dict(normals=f32(n1 * scale), normals2=f32(n2 * scale), normals_variance=f32(rng.uniform(1e-4, 0.05, shape)),
                normals2_variance=f32(rng.uniform(1e-4, 0.05, shape)))


def source_pixels_of(bad, n_src_shape):
    """source pixels a set of destination pixels is sampled from"""
    out = np.zeros(n_src_shape, bool)
    if bad.shape == n_src_shape:
        return bad.copy()
    ylo, yhi, _ = linear_taps(n_src_shape[0], bad.shape[0])
    xlo, xhi, _ = linear_taps(n_src_shape[1], bad.shape[1])
    ys, xs = np.nonzero(bad)
    for ya in (ylo, yhi):
        for xa in (xlo, xhi):
            out[ya[ys], xa[xs]] = True
    return out


def guarded_normals(rng, shape, size, factor, stats):
    """normal maps whose resized, normalised versions pass the flip guard at full and at half size"""
    spread = np.where(rng.uniform(size=shape) < 0.5, 0.03, 0.35)
    m = normal_maps(rng, shape, spread)
    redrawn = np.zeros(shape, bool)
    half = (int(size[0] // factor), int(size[1] // factor))
    for _ in range(100):
        n1, n2 = (_unit(resize_linear(m[k], size)) for k in ("normals", "normals2"))
        d1, d2 = (_unit(resize_linear(n, half)) for n in (n1, n2))
        bad_full = ~flip_guard(n1, n2) | source_pixels_of(~flip_guard(d1, d2), size)
        bad = source_pixels_of(bad_full, shape)
        if not bad.any():
            break
        fresh = normal_maps(rng, shape, spread)
        for k in ("normals", "normals2"):
            m[k][bad] = fresh[k][bad]
        redrawn |= bad
    else:
        raise RuntimeError("the flip guard still fails after 100 redraws")
    stats[0] += int(redrawn.sum())
    stats[1] += redrawn.size
    return m
