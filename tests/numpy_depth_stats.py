"""NumPy restatement of the prior scale fit and of the truncation sigma — TEST INFRASTRUCTURE, not product code.

Two levels.  ``shiftscale`` and ``truncation_sigma`` follow the reference's loops over a scene
(mpsfm/sfm/mapper/bundle_adjustment.py:187-242 with its early return, :295-333 with fit_robust_gaussian_mad :10-15)
through the scene's own accessors: the map sampling of PriorUtils (mpsfm_amd.sfm.scene.priorutils.bilinear_at_kps, pinned
by tests/test_reference_fixtures_cpu.py against vectors of the reference's PriorUtils) and the scene's pose product.
``depth_stats`` takes the arguments of mpsfm_amd.capi.depth_stats and answers with the same dict: the checker of
mpsfm_depth_stats, and what an oracle backend hands to Optimizer(stats="device").
"""

from __future__ import annotations

import numpy as np

from mpsfm_amd.sfm.scene.priorutils import bilinear_at_kps
from mpsfm_amd.synthetic import R_from_quat

STATS_FIT, STATS_SIGMA = 1, 2
STATS_EMPTY, STATS_EMPTY_METRIC = 1, 2
SEL_VALID, SEL_FIT, SEL_SIGMA = 1, 2, 4


def two_middle(values):
    """(lo, hi): the order statistics of rank (n - 1) // 2 and n // 2 of a non-empty array without NaNs."""
    n = len(values)
    part = np.partition(values, sorted({(n - 1) // 2, n // 2}))
    return part[(n - 1) // 2], part[n // 2]


# ---- scene level: the reference's loops --------------------------------------------------------------------------------------
def shiftscale(scene, conf, bundle, allow_scale_filter=False, allow_metric_scale_filter=False):
    """{imid: [0, median log ratio]} as __build_shiftscale_problem returns it (conf: scale_filter, scale_filter_factor,
    metric_scale_filter, single_rescale)."""
    shift_scale = {}
    for imid in bundle["optim_ids"]:
        image = scene.images[imid]
        p2d = image.get_observation_point2D_idxs()
        kps = image.keypoint_coordinates(p2d)
        p3dids = image.point3D_ids(p2d)
        obsdepths = image.depth.data_prior_at_kps(kps)
        valid = np.array(image.depth.valid_at_kps(kps), dtype=bool)
        z = (image.cam_from_world * scene.point3D_coordinates(p3dids))[:, -1]  # also the reference's projdepths (geometry.project3D)
        if (conf["scale_filter_factor"] or conf["metric_scale_filter"]) and (
                "ref_id" in bundle and imid != bundle["ref_id"] and conf["single_rescale"]):
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            if allow_metric_scale_filter and conf["metric_scale_filter"] and ((imid == bundle["ref_id"]) or (not conf["single_rescale"])):
                scale = z / obsdepths.clip(1e-6, None)
                im_scale = image.depth.scale
                proposed_scale = scale * im_scale
                map_scale = np.mean([scene.images[i].depth.scale for i in bundle["optim_ids"] if i != imid])
                div = map_scale / proposed_scale
                valid = valid * ((div < 1.5) * (div > (1 / 1.5)))
                if valid.sum() == 0:
                    shift_scale[imid] = np.array([0.0, np.log(map_scale / im_scale)])
                    return shift_scale, True
            if allow_scale_filter and conf["scale_filter"] and not allow_metric_scale_filter:
                div = obsdepths / z
                valid = valid * ((div < conf["scale_filter_factor"]) * (div > (1 / conf["scale_filter_factor"])))
            ratio = (z[valid] / obsdepths[valid]).clip(1e-6, None)
            proposed = np.median(np.log(ratio)) if len(ratio) else np.nan
        shift_scale[imid] = np.array([0.0, proposed])
    return shift_scale, True


def truncation_sigma(scene, imids):
    """sigma of update_truncation_multiplier: the per-image loop, then 1.4826 MAD of the whitened log-depth errors."""
    D, D3d, dstds = [], [], []
    for imid in imids:
        image = scene.images[imid]
        if not image.depth.activated:  # what gather_bundle leaves out: the reference's mapper passes registered, activated images
            continue
        p2Ds = np.array(image.get_observation_point2D_idxs())
        kps = image.keypoint_coordinates(p2Ds)
        valid = image.depth.valid_at_kps(kps)
        kps, p2Ds = kps[valid], p2Ds[valid]
        depths = image.depth.data_at_kps(kps)
        mask = depths > 0
        p3Ds = np.array(image.point3D_ids(p2Ds))[mask]
        depth3d = (image.cam_from_world * scene.point3D_coordinates(p3Ds))[:, -1]
        D.append(depths[mask])
        D3d.append(depth3d)
        dstds.append(np.asarray(image.depth.uncertainty_update, np.float64)[p2Ds[mask]] ** 0.5)
    depths, depth3ds, dstds = np.concatenate(D), np.concatenate(D3d), np.concatenate(dstds)
    with np.errstate(divide="ignore", invalid="ignore"):
        whitened = (np.log(depths) - np.log(depth3ds)) / np.clip(dstds / depths, 1e-6, None)
    mu = np.median(whitened)
    return 1.4826 * np.median(np.abs(whitened - mu))


# ---- array level: the entry point ----------------------------------------------------------------------------------------------
def depth_stats(depth_maps, valid_maps, sx, sy, cam_quat, cam_t, obs_img, obs_xy, obs_var, obs_pt, pts, what=STATS_FIT | STATS_SIGMA,
                mode=None, filter=None, im_scale=None, map_scale=None, scale_filter_factor=1.5, per_obs=False, margins=None):
    """Same arguments and outputs as mpsfm_amd.capi.depth_stats (no device).  `margins`: a list that receives, per filtered
    observation, the relative distance of its `div` to the nearer threshold (the condition of the exact comparisons)."""
    n_img, n = len(depth_maps), len(obs_img)
    obs_img, obs_pt = np.asarray(obs_img), np.asarray(obs_pt)
    if np.any(np.diff(obs_img) < 0):
        raise ValueError("obs_img must not decrease")
    mode = np.ones(n_img, np.uint8) if mode is None else np.asarray(mode, np.uint8)
    filt = np.zeros(n_img, np.uint8) if filter is None else np.asarray(filter, np.uint8)
    im_scale = np.ones(n_img) if im_scale is None else np.asarray(im_scale, np.float64)
    map_scale = np.ones(n_img) if map_scale is None else np.asarray(map_scale, np.float64)
    R = R_from_quat(np.asarray(cam_quat, np.float64).reshape(-1, 4))
    t = np.asarray(cam_t, np.float64).reshape(-1, 3)
    obs_xy, pts, obs_var = np.asarray(obs_xy, np.float64).reshape(-1, 2), np.asarray(pts, np.float64).reshape(-1, 3), np.asarray(obs_var, np.float64)
    ratio, whitened, selected = np.zeros(n), np.zeros(n), np.zeros(n, np.uint8)
    out = {}
    if what & STATS_FIT:
        out.update(n_valid=np.zeros(n_img, np.int64), n_sel=np.zeros(n_img, np.int64), n_nan=np.zeros(n_img, np.int64),
                   ratio_lo=np.full(n_img, np.nan), ratio_hi=np.full(n_img, np.nan), flags=np.zeros(n_img, np.uint32))
    f = float(scale_filter_factor)
    for k in range(n_img):
        sel = np.flatnonzero(obs_img == k)
        v = bilinear_at_kps(np.asarray(valid_maps[k]), obs_xy[sel], sx[k], sy[k])
        d = bilinear_at_kps(depth_maps[k], obs_xy[sel], sx[k], sy[k])
        X = pts[obs_pt[sel]]
        z = (np.concatenate([R[k], t[k][:, None]], 1) @ np.concatenate([X, np.ones((len(X), 1))], 1).T).T[:, 2]
        base = v == 1
        with np.errstate(divide="ignore", invalid="ignore"):
            if (what & STATS_FIT) and mode[k] == 1:
                keep = base.copy()
                if filt[k] == 1:
                    div = d / z
                    keep &= (div < f) & (div > 1 / f)
                    if margins is not None:
                        margins.extend(np.minimum(np.abs(div / f - 1), np.abs(div * f - 1))[base].tolist())
                elif filt[k] == 2:
                    div = map_scale[k] / ((z / d.clip(1e-6, None)) * im_scale[k])
                    keep &= (div < 1.5) & (div > 1 / 1.5)
                    if margins is not None:
                        margins.extend(np.minimum(np.abs(div / 1.5 - 1), np.abs(div * 1.5 - 1))[base].tolist())
                r = (z / d).clip(1e-6, None)
                ratio[sel] = r
                selected[sel] |= base.astype(np.uint8) * SEL_VALID | keep.astype(np.uint8) * SEL_FIT
                ranked = r[keep & ~np.isnan(r)]
                out["n_valid"][k], out["n_sel"][k], out["n_nan"][k] = base.sum(), keep.sum(), np.isnan(r[keep]).sum()
                if len(ranked):
                    out["ratio_lo"][k], out["ratio_hi"][k] = two_middle(ranked)
                if keep.sum() == 0:
                    out["flags"][k] = STATS_EMPTY | (STATS_EMPTY_METRIC if filt[k] == 2 else 0)
            if what & STATS_SIGMA:
                whitened[sel] = (np.log(d) - np.log(z)) / np.clip(obs_var[sel] ** 0.5 / d, 1e-6, None)
                selected[sel] |= (base & (d > 0)).astype(np.uint8) * SEL_SIGMA
    if what & STATS_SIGMA:
        w = whitened[(selected & SEL_SIGMA) != 0]
        ranked = w[~np.isnan(w)]
        mu = mad = np.nan
        if len(ranked):
            with np.errstate(invalid="ignore"):
                mu = 0.5 * np.add(*two_middle(ranked))
                dev = np.abs(ranked - mu)
                mad = np.nan if np.isnan(dev).any() else 0.5 * np.add(*two_middle(dev))
        out.update(sigma_n_sel=len(w), sigma_n_nan=int(np.isnan(w).sum()), mu=float(mu), mad=float(mad))
    if per_obs:
        out.update(ratio=ratio, whitened=whitened, selected=selected)
    return out
