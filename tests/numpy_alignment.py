"""numpy_alignment.py — TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Independent NumPy restatement of the 3D-3D alignment of csrc/align3d.hip (include/mpsfm_hip.h, mpsfm_align3d_estimate and
its siblings): LO-RANSAC of ``tgt ~ s R src + t`` with a 3-point closed form and the same closed form as local estimator,
modelled on COLMAP 3.11's EstimateRigid3dRobust / EstimateSim3dRobust as recalled (**parity with pycolmap unpinned**), the
least-squares fit on its own, and the lifting of keypoints through a depth map as the reference's ``icp/depth_to_3d.py`` +
``icp/interpolate.py`` do it.

It shares no code with csrc/align3d_math.h: the rotation is an SVD (Kabsch, with the reflection fix) where the HIP path uses
Horn's quaternion and Jacobi sweeps, the degeneracy rule reads ``np.linalg.eigvalsh``, the sums are NumPy's.  The sampler,
``ComputeNumTrials`` and the support measure are numpy_loransac.py's.

``estimate`` also reports FRAGILE decisions, which rounding may decide differently in another implementation: a residual within
1e-7 (relative) of the threshold in a model whose support decided something, equal inlier counts whose residual sums are within
1e-9 (relative) or both at rounding level (when that count is the final one), and a sample whose collinearity measure is
within a factor of 100 of the 1e-20 bound.  Tests redraw such scenes.
"""

from __future__ import annotations

import numpy as np

from numpy_loransac import MASK64, _better, _support, num_trials, sample

DBL_MAX = np.finfo(np.float64).max
COLLINEAR_SIN2 = 1e-20
LINE_EIG_RATIO = 1e-12


def residuals(M: np.ndarray, s: float, src: np.ndarray, tgt: np.ndarray) -> np.ndarray:
    """|q - (s R p + t)|^2 per pair, M = [R | t]."""
    d = [tgt[:, r] - (s * (M[r, 0] * src[:, 0] + M[r, 1] * src[:, 1] + M[r, 2] * src[:, 2]) + M[r, 3]) for r in range(3)]
    return d[0] * d[0] + d[1] * d[1] + d[2] * d[2]


def _closed_form(P: np.ndarray, Q: np.ndarray, with_scale: bool):
    """(M [3,4], s) minimising sum |q - (s R p + t)|^2, R a proper rotation; None when the scale is not finite and positive."""
    mp, mq = P.sum(0) / len(P), Q.sum(0) / len(Q)
    Pc, Qc = P - mp, Q - mq
    U, _, Vt = np.linalg.svd(Qc.T @ Pc)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0])
    R = U @ D @ Vt
    s = 1.0
    if with_scale:
        with np.errstate(all="ignore"):
            s = float(np.sum(Qc * (Pc @ R.T)) / np.sum(Pc * Pc))
        if not (np.isfinite(s) and s > 0):
            return None
    return np.c_[R, mq - s * (R @ mp)], s


def _sin2(X: np.ndarray) -> float:
    """sin^2 of the angle at the first of three points (0 for coincident points)."""
    e1, e2 = X[1] - X[0], X[2] - X[0]
    den = (e1 @ e1) * (e2 @ e2)
    cr = np.cross(e1, e2)
    return float(cr @ cr / den) if den > 0 else 0.0


def minimal(P: np.ndarray, Q: np.ndarray, with_scale: bool, fragile: list | None = None):
    """The 3-point solver: None when the source or the target triangle is degenerate."""
    s2 = min(_sin2(P), _sin2(Q))
    if fragile is not None and COLLINEAR_SIN2 / 100 <= s2 <= COLLINEAR_SIN2 * 100:
        fragile.append(("collinear", s2))
    if s2 <= COLLINEAR_SIN2:
        return None
    return _closed_form(P, Q, with_scale)


def _is_line(X: np.ndarray) -> bool:
    Xc = X - X.sum(0) / len(X)
    w = np.linalg.eigvalsh(Xc.T @ Xc)
    return not w[1] > LINE_EIG_RATIO * w[2]


def fit(src, tgt, mask=None, with_scale: bool = False):
    """The least-squares fit over the pairs `mask` keeps: (M [3,4], s, points used), M None when there is no model (fewer than 3
    points, or source or target points on a line)."""
    P = np.asarray(src, np.float64).reshape(-1, 3)
    Q = np.asarray(tgt, np.float64).reshape(-1, 3)
    if mask is not None:
        keep = np.asarray(mask).reshape(-1) != 0
        P, Q = P[keep], Q[keep]
    if len(P) < 3 or _is_line(P) or _is_line(Q):
        return None, 1.0, len(P)
    got = _closed_form(P, Q, with_scale)
    return (None, 1.0, len(P)) if got is None else (got[0], got[1], len(P))


DEFAULT_OPTIONS = dict(max_error=0.1, min_inlier_ratio=0.1, confidence=0.99, dyn_num_trials_multiplier=3.0, min_num_trials=100,
                       max_num_trials=5000, seed=0)


def estimate(src, tgt, with_scale: bool = False, **opts) -> dict:
    """LO-RANSAC of tgt ~ s R src + t.  Returns dict(success, tgt_from_src [3,4] or None, scale, num_inliers, inlier_mask,
    num_trials, max_num_trials, lo_rounds, fragile)."""
    o = dict(DEFAULT_OPTIONS)
    o.update(opts)
    P = np.asarray(src, np.float64).reshape(-1, 3)
    Q = np.asarray(tgt, np.float64).reshape(-1, 3)
    n = len(P)
    thr2 = o["max_error"] * o["max_error"]
    fragile: list = []
    out = dict(success=False, tgt_from_src=None, scale=0.0, num_inliers=0, inlier_mask=np.zeros(n, bool), num_trials=0, lo_rounds=0,
               fragile=fragile)
    if n < 3:
        return out
    max_trials = min(o["max_num_trials"], num_trials(int(o["min_inlier_ratio"] * 100000), 100000, o["confidence"],
                                                     o["dyn_num_trials_multiplier"], 3))
    out["max_num_trials"] = max_trials
    seed = int(o["seed"]) & MASK64
    tie_counts: set = set()

    def scored(model, best):
        res = residuals(model[0], model[1], P, Q)
        sup = _support(res, thr2)
        near = int(np.sum(np.abs(res - thr2) <= 1e-7 * thr2))
        better = _better(sup, best)
        if near and (better or abs(sup[0] - best[0]) <= near):
            fragile.append(("threshold", near, sup[0], best[0]))
        if sup[0] == best[0] and sup[0] > 0:
            floor = 1e-10 * thr2 * sup[0]
            if sup[1] <= floor and best[1] <= floor:
                tie_counts.add(sup[0])  # models that fit their points to rounding level: which one wins is noise
            elif abs(sup[1] - best[1]) <= 1e-9 * max(abs(sup[1]), abs(best[1]), 1e-300):
                fragile.append(("tie", sup, best))
        return res, sup, better

    best, best_model = (0, DBL_MAX), None
    dyn = max_trials
    abort = False
    trials = 0
    lo_rounds = 0
    while trials < max_trials:
        if abort:
            trials += 1
            break
        idx = sample(seed, trials, n, 3)
        model = minimal(P[idx], Q[idx], with_scale, fragile)
        if model is not None:
            res, sup, better = scored(model, best)
            if better:
                best, best_model = sup, model
                if sup[0] > 3:
                    for _ in range(10):
                        inl = res <= thr2
                        prev = best[0]
                        lo_rounds += 1
                        M, s, _ = fit(P[inl], Q[inl], None, with_scale)
                        if M is not None:
                            lres, lsup, lbetter = scored((M, s), best)
                            if lbetter:
                                best, best_model, res = lsup, (M, s), lres
                        if best[0] <= prev:
                            break
                dyn = num_trials(best[0], n, o["confidence"], o["dyn_num_trials_multiplier"], 3)
            if trials >= dyn and trials >= o["min_num_trials"]:
                abort = True
        trials += 1
    out.update(num_trials=trials, lo_rounds=lo_rounds)
    if best[0] < 3:
        return out
    if best[0] in tie_counts:
        fragile.append(("noise_tie", best[0]))
    res = residuals(best_model[0], best_model[1], P, Q)
    out.update(success=True, tgt_from_src=best_model[0], scale=best_model[1], num_inliers=best[0], inlier_mask=res <= thr2)
    return out


def lift(depth, intr, xy):
    """Keypoints [n, 2] through the point map of depth [H, W], PINHOLE intr = (fx, fy, cx, cy): (xyz [n, 3], valid [n]), in the
    reference's order of operations; validity by the rule of include/mpsfm_hip.h; invalid keypoints are zeros."""
    depth = np.asarray(depth, np.float64)
    H, W = depth.shape
    fx, fy, cx, cy = (np.float64(v) for v in intr)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    xyz, valid = np.zeros((len(xy), 3)), np.zeros(len(xy), bool)

    def point(r, c):
        z = depth[r, c]
        return np.array([(c - cx) * z / fx, (r - cy) * z / fy, z])

    for i, (x, y) in enumerate(xy):
        if not (x >= 0 and y >= 0):
            continue
        if not (np.trunc(x) + 1 <= W - 1 and np.trunc(y) + 1 <= H - 1):
            continue
        c, r = int(x), int(y)
        z = depth[r:r + 2, c:c + 2]
        if not (np.isfinite(z).all() and (z > 0).all()):
            continue
        ax, ay = x - c, y - r
        with np.errstate(all="ignore"):
            v = point(r, c) * (1 - ax) * (1 - ay) + point(r, c + 1) * ax * (1 - ay) + point(r + 1, c) * (1 - ax) * ay + point(r + 1, c + 1) * ax * ay
        if np.isfinite(v).all():
            xyz[i], valid[i] = v, True
    return xyz, valid


def synthetic_problem(n: int, outliers: float, seed: int, with_scale: bool = False):
    """n point pairs under a random transform: (src, tgt, R, t, s, designed inlier mask).  Rotation about a random axis by
    U(0.1, 3.0) rad, t ~ N(0, 1), src uniform in [-2,2] x [-1.5,1.5] x [0.5,6], tgt = s R src + t + N(0, 0.01) with s = 1.7 for a
    similarity, round(outliers n) targets replaced by uniform points in [-4,4]^2 x [0,8]."""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=3)
    ang = rng.uniform(0.1, 3.0)
    k = a / np.linalg.norm(a)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    t = rng.normal(size=3)
    s = 1.7 if with_scale else 1.0
    src = rng.uniform([-2.0, -1.5, 0.5], [2.0, 1.5, 6.0], (n, 3))
    tgt = s * src @ R.T + t + rng.normal(size=(n, 3)) * 0.01
    inl = np.ones(n, bool)
    n_out = int(round(outliers * n))
    bad = rng.choice(n, n_out, replace=False)
    tgt[bad] = rng.uniform([-4.0, -4.0, 0.0], [4.0, 4.0, 8.0], (n_out, 3))
    inl[bad] = False
    return src, tgt, R, t, s, inl
