"""Vectorised NumPy restatement of the reference's depth-consistency check (mpsfm/sfm/mapper/depthconsistency.py:62-159
and :224-246, reconstruction/mixins/depth_utils.py:9-48), with the lifted covariance rotated in closed form.

The projection follows the reference's own arithmetic (unproject through inv(K_scaled) and inv([cam_from_world; 0 0 0 1]),
project through cam_from_world and K_scaled); the z-buffer keeps the last writer in raster order per target pixel (what
the reference's `find_min_buffer` does, its mask against an all-inf buffer being all true), computed here with
np.maximum.at over source indices.  std_bar^2 = var (m . u)^2 + m0^2 a^2 + m1^2 b^2 with m = row 2 of R_t^T R_s.

Every function takes plain arrays (an image is a dict with depth, variance, prior_std_multiplier, intr_scaled, intr and
cam_from_world, as capi.depth_consistency takes them) and reports, per source pixel, whether it lies within `eps`
(relative) of a decision boundary, so that a device result can be compared exactly everywhere else.
"""

from __future__ import annotations

import numpy as np

IN, SURFACE, OCCL, INVALID = 1, 2, 4, 8


def _K(f):
    return np.array([[f[0], 0.0, f[2]], [0.0, f[1], f[3]], [0.0, 0.0, 1.0]])


def clamp_depth(im):
    """The reference's in-place `depth[depth <= 0] = 0.1`."""
    im["depth"][im["depth"] <= 0] = 0.1


def leg(src, dst, c=15.0, s=0.6, eps=1e-9):
    """One direction src -> dst of check_depth_consistency.  Both maps must already be clamped.
    Returns dict(code uint8 [Hs,Ws], near bool [Hs,Ws], t float [Hs,Ws] (NaN outside the canvas), in_canvas, target)."""
    d1 = np.asarray(src["depth"], np.float64)
    Hs, Ws = d1.shape
    Hd, Wd = np.asarray(dst["depth"]).shape
    y, x = np.mgrid[0:Hs, 0:Ws]
    x, y, dd = x.ravel().astype(np.float64), y.ravel().astype(np.float64), d1.ravel()
    H1 = np.vstack([np.asarray(src["cam_from_world"], np.float64).reshape(3, 4), [0, 0, 0, 1.0]])
    H2 = np.vstack([np.asarray(dst["cam_from_world"], np.float64).reshape(3, 4), [0, 0, 0, 1.0]])
    pc = np.linalg.inv(_K(src["intr_scaled"])) @ np.vstack([x * dd, y * dd, dd])
    pw = (np.linalg.inv(H1) @ np.vstack([pc, np.ones(len(dd))]))[:3]
    pcam = (H2 @ np.vstack([pw, np.ones(len(dd))]))[:3]
    z = pcam[2].copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        pp = (_K(dst["intr_scaled"]) @ (pcam / z[None]))[:2]
    px, py = pp
    inc = (px >= 0) & (px + 0.5 < Wd) & (py >= 0) & (py + 0.5 < Hd) & (z > 0)
    n = Hs * Ws
    idx = np.arange(n)
    tgt = np.full(n, -1, np.int64)
    tgt[inc] = py[inc].astype(np.int64) * Wd + px[inc].astype(np.int64)
    win = np.full(Hd * Wd, -1, np.int64)
    np.maximum.at(win, tgt[inc], idx[inc])

    # closed-form std_bar of the source pixel (lifted covariance with unscaled intrinsics at map coordinates)
    R1 = H1[:3, :3]
    R2 = H2[:3, :3]
    m = (R2.T @ R1)[2]
    fx, fy, cx, cy = (float(v) for v in src["intr"])
    v1 = np.asarray(src["variance"], np.float64).ravel() / src["prior_std_multiplier"] ** 2
    ux, uy = (x - cx) * (1.0 / fx), (y - cy) * (1.0 / fy)
    a, b = np.clip(dd * (1.0 / fx), -1e6, 1e6), np.clip(dd * (1.0 / fy), -1e6, 1e6)
    s1sq = v1 * (m[0] * ux + m[1] * uy + m[2]) ** 2 + m[0] ** 2 * a**2 + m[1] ** 2 * b**2
    d2 = np.asarray(dst["depth"], np.float64).ravel()
    std2 = np.sqrt(np.asarray(dst["variance"], np.float64).ravel() / dst["prior_std_multiplier"] ** 2)

    ti = tgt[inc]
    buf = z[win[ti]]
    num = buf - d2[ti]
    den = np.sqrt((np.sqrt(s1sq[inc]) * c) ** 2 + (std2[ti] * c) ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        tv = num / den
    code = np.zeros(n, np.uint8)
    code[inc] = IN | np.where(np.abs(tv) < s, SURFACE, 0) | np.where(tv > s, OCCL, 0) | np.where(tv < -s, INVALID, 0)
    t_full = np.full(n, np.nan)
    t_full[inc] = tv

    # pixels within eps of a decision boundary: canvas edges, integer crossings of p, depth = 0, |num| = s den
    def near(v, b_):
        return np.abs(v - b_) <= eps * np.maximum(1.0, np.abs(b_))

    with np.errstate(invalid="ignore"):
        near_p = (near(px, np.round(px)) | near(px, Wd - 0.5) | near(py, np.round(py)) | near(py, Hd - 0.5)
                  | (np.abs(z) <= eps * np.maximum(1.0, dd)))
    near_p &= np.isfinite(px) & np.isfinite(py)
    # a pixel near a projection boundary may move the winner of the targets it could land on: those targets are unstable
    unstable = np.zeros(Hd * Wd, bool)
    for dx in (-1e-6, 1e-6):
        for dy in (-1e-6, 1e-6):
            qx, qy = px[near_p] + dx * np.maximum(1, np.abs(px[near_p])), py[near_p] + dy * np.maximum(1, np.abs(py[near_p]))
            ok = (qx >= 0) & (qx < Wd) & (qy >= 0) & (qy < Hd)
            unstable[qy[ok].astype(np.int64) * Wd + qx[ok].astype(np.int64)] = True
    nearv = near_p.copy()
    nt = np.zeros(inc.sum(), bool)
    with np.errstate(invalid="ignore"):
        nt = np.abs(np.abs(num) - s * den) <= eps * np.maximum.reduce([np.abs(buf), np.abs(d2[ti]), s * den])
    # 0 / 0 comes from bit-identical inputs (the same rotation, zero variances, equal depths), computed exactly on both sides
    nt &= ~((num == 0) & (den == 0))
    nt |= unstable[ti]
    nearv[np.flatnonzero(inc)[nt]] = True
    return dict(code=code.reshape(Hs, Ws), near=nearv.reshape(Hs, Ws), t=t_full.reshape(Hs, Ws), in_canvas=inc.reshape(Hs, Ws),
                target=tgt.reshape(Hs, Ws))


def counts_of(code):
    return np.array([np.count_nonzero(code & k) for k in (IN, SURFACE, OCCL, INVALID)], np.int64)


def pair(images, a, b, c=15.0, s=0.6, eps=1e-9):
    """Both legs of pair (a, b); clamps both maps in place first, as reproject_depth does."""
    clamp_depth(images[a])
    clamp_depth(images[b])
    return leg(images[a], images[b], c, s, eps), leg(images[b], images[a], c, s, eps)


def masks(l12, l21):
    """The reference check_depth_consistency dict rebuilt from the two legs' codes."""
    out = {}
    for tag, code in (("1", l12["code"]), ("2", l21["code"])):
        out["valid" + tag] = (code & (SURFACE | OCCL)) != 0
        out["occl" + tag] = (code & OCCL) != 0
        out["invalid" + tag] = (code & INVALID) != 0
        out["surface" + tag] = (code & SURFACE) != 0
        out[f"valid{tag}_mask"] = (code & IN) != 0
    return out


MASK_KEYS = ["valid1", "valid2", "occl1", "occl2", "invalid1", "invalid2", "surface1", "surface2", "valid1_mask", "valid2_mask"]


def bundle_score(counts):
    """check_bundle_depth_concistency from per-pair counts [n_pairs, 2, 4] (leg 0 query -> ref, leg 1 ref -> query)."""
    counts = np.asarray(counts, np.int64).reshape(-1, 2, 4)
    tot = counts.sum(axis=0)
    q_in, q_surf, q_occl = (int(v) for v in tot[0, :3])
    r_in, r_surf, r_occl = (int(v) for v in tot[1, :3])
    ref = (r_in - r_surf - r_occl) / max(r_in - r_occl, 0.1)
    qry = (q_in - q_surf - q_occl) / max(q_in - q_occl, 0.1)
    return max(ref, qry), (q_in, r_in)


def bundle(images, query, refs, c=15.0, s=0.6, eps=1e-9):
    """All pairs (query, ref): returns (score, (in-canvas sums), counts [n,2,4], legs [(l12, l21)])."""
    legs = [pair(images, query, r, c, s, eps) for r in refs]
    counts = np.array([[counts_of(l12["code"]), counts_of(l21["code"])] for l12, l21 in legs], np.int64).reshape(-1, 2, 4)
    score, sums = bundle_score(counts) if len(refs) else (0.0, (0, 0))
    return score, sums, counts, legs
