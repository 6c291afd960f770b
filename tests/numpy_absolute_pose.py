"""numpy_absolute_pose.py — TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Independent NumPy restatement of the estimation half of ``pycolmap.estimate_and_refine_absolute_pose`` (reference
mpsfm/sfm/estimators/absolute_pose.py:6-25): COLMAP 3.11 ``EstimateAbsolutePose`` =
``LORANSAC<P3PEstimator, EPNPEstimator, InlierSupportMeasurer>`` on CamFromImg-normalised points, restated from the
upstream sources as recalled (src/colmap/estimators/pose.cc, absolute_pose.cc, optim/loransac.h, optim/ransac.h,
optim/support_measurement.cc).  The reference's COLMAP fork is not in its tree: **parity unpinned**.

It shares no code with csrc/abs_pose_math.h / csrc/abs_pose.hip: P3P roots come from ``np.roots`` (companion matrix) plus a
Newton polish where the HIP path runs an Aberth iteration; the absolute orientation is an SVD (Kabsch) where the HIP path
uses Horn's quaternion; EPnP uses ``np.linalg.eigh`` / ``lstsq`` / ``svd`` where the HIP path runs Jacobi sweeps, a
Householder QR and device reductions.  The sampler is the documented counter-based recipe (include/mpsfm_hip.h), computed
with Python ints.

``estimate`` also reports FRAGILE decisions, which rounding may decide differently in another implementation: a residual
within 1e-7 (relative) of the threshold in a model whose support decided something, equal inlier counts whose residual
sums are within 1e-9 (relative) or both at rounding level (when that count is the final one), a P3P root whose imaginary part is within a factor of 10 of the 1e-10 cut-off, P3P roots
closer than 1e-7 (relative: their order sets the order of the models), a final P3P model whose root is ill-conditioned
(clustered roots of Grunert's quartic) and an EPnP choice between beta solutions whose reprojection sums are within 1e-9
(relative).  Tests redraw such scenes.
"""

from __future__ import annotations

import math

import numpy as np

from numpy_loransac import MASK64, PHI, _better, _mix, _support  # noqa: F401  (names the tests use)
from numpy_loransac import num_trials as _num_trials
from numpy_loransac import sample as _sample

DBL_MAX = np.finfo(np.float64).max
DBL_EPS = np.finfo(np.float64).eps
MAX_ROOT_IMAG = 1e-10


def sample(seed: int, t: int, n: int) -> list[int]:
    """The three distinct indices of trial t."""
    return _sample(seed, t, n, 3)


def num_trials(num_inliers: int, n: int, confidence: float, multiplier: float) -> float:
    """RANSAC::ComputeNumTrials with kMinNumSamples = 3 (math.inf for size_t max)."""
    return _num_trials(num_inliers, n, confidence, multiplier, 3)


def residuals(P: np.ndarray, x: np.ndarray, X: np.ndarray) -> np.ndarray:
    """ComputeSquaredReprojectionError: normalised plane, DBL_MAX at depth <= DBL_EPSILON."""
    R, t = P[:, :3], P[:, 3]
    Xc = X @ R.T + t
    z = Xc[:, 2]
    out = np.full(len(X), DBL_MAX)
    ok = z > DBL_EPS
    d = Xc[ok, :2] / z[ok, None] - x[ok]
    out[ok] = d[:, 0] ** 2 + d[:, 1] ** 2
    return out


def _kabsch(W: np.ndarray, Cm: np.ndarray):
    """R, t with Cm ~ R W + t (rows are points)."""
    w0, c0 = W.mean(0), Cm.mean(0)
    U, _, Vt = np.linalg.svd((Cm - c0).T @ (W - w0))
    R = U @ Vt
    if np.linalg.det(R) < 0:
        V = Vt.T.copy()
        V[:, 2] = -V[:, 2]
        R = U @ V.T
    return R, c0 - R @ w0


def p3p(x: np.ndarray, X: np.ndarray, fragile: list | None = None, conds: list | None = None) -> list[np.ndarray]:
    """P3PEstimator::Estimate: Grunert's quartic in s3 / s1, real roots (|imag| <= 1e-10) with positive lengths.  `conds`
    receives per model the relative error that one rounding of the coefficients can cause in its root (clustered roots of
    Grunert's quartic make it large: such a pose is only known to ~1e-8 in any implementation)."""
    e1, e2 = X[1] - X[0], X[2] - X[0]
    cr = np.cross(e1, e2)
    if cr @ cr <= 1e-20 * (e1 @ e1) * (e2 @ e2):
        return []
    f = np.c_[x, np.ones(3)]
    f = f / np.linalg.norm(f, axis=1)[:, None]
    a2, b2, c2 = np.sum((X[1] - X[2]) ** 2), np.sum((X[0] - X[2]) ** 2), np.sum((X[0] - X[1]) ** 2)
    ca, cb, cg = f[1] @ f[2], f[0] @ f[2], f[0] @ f[1]
    amc, apc = (a2 - c2) / b2, (a2 + c2) / b2
    coef = np.array([
        (amc - 1) ** 2 - 4 * c2 / b2 * ca * ca,
        4 * (amc * (1 - amc) * cb - (1 - apc) * ca * cg + 2 * c2 / b2 * ca * ca * cb),
        2 * (amc ** 2 - 1 + 2 * amc ** 2 * cb * cb + 2 * (b2 - c2) / b2 * ca * ca - 4 * apc * ca * cb * cg + 2 * (b2 - a2) / b2 * cg * cg),
        4 * (-amc * (1 + amc) * cb + 2 * a2 / b2 * cg * cg * cb - (1 - apc) * ca * cg),
        (1 + amc) ** 2 - 4 * a2 / b2 * cg * cg,
    ])
    if coef[0] == 0 or not np.isfinite(coef[0]):
        return []
    roots = np.roots(coef).astype(complex)
    dcoef = np.polyder(coef)
    for _ in range(2):  # Newton polish
        d = np.polyval(dcoef, roots)
        ok = d != 0
        roots[ok] = roots[ok] - np.polyval(coef, roots[ok]) / d[ok]
    if fragile is not None:
        fragile.extend(("p3p_root_imag", abs(r.imag)) for r in roots if 1e-11 <= abs(r.imag) <= 1e-9)
    real = np.sort([r.real for r in roots if abs(r.imag) <= MAX_ROOT_IMAG])  # models in ascending order of the root
    if fragile is not None and len(real) > 1 and np.min(np.diff(real)) <= 1e-7 * np.max(np.abs(real)):
        fragile.append(("p3p_root_order", real))
    models = []
    for v in real:
        v = float(v)
        if v < 0:
            continue
        den = 2 * (cg - v * ca)
        if den == 0:
            continue
        u = ((-1 + amc) * v * v - 2 * amc * cb * v + 1 + amc) / den
        if u < 0:
            continue
        s1 = math.sqrt(b2 / (1 + v * v - 2 * v * cb))
        Y = np.array([s1, u * s1, v * s1])[:, None] * f
        R, t = _kabsch(X, Y)
        models.append(np.c_[R, t])
        if conds is not None:
            scale = float(np.sum(np.abs(coef) * np.abs(v) ** np.arange(4, -1, -1)))
            conds.append(DBL_EPS * scale / max(abs(np.polyval(dcoef, v)) * abs(v), 1e-300))
    return models


def epnp(x: np.ndarray, X: np.ndarray, fragile: list | None = None):
    """EPNPEstimator::ComputePose (returns the 3x4 model or None)."""
    n = len(X)
    c0 = X.sum(0) / n
    PW0 = X - c0
    D, U = np.linalg.eigh(PW0.T @ PW0)
    D, U = D[::-1], U[:, ::-1]
    U = U * np.sign(U[np.argmax(np.abs(U), axis=0), np.arange(3)])  # each axis: largest-magnitude component positive
    k = np.sqrt(np.maximum(D, 0) / n)
    if not k[2] > 6.66e-16 * k[0]:
        return None
    cws = np.vstack([c0, c0 + k[:, None] * U.T])
    CC = (cws[1:] - c0).T
    a = np.linalg.solve(CC, PW0.T).T
    alphas = np.c_[1 - a.sum(1), a]
    M = np.zeros((2 * n, 12))
    for j in range(4):
        M[0::2, 3 * j] = alphas[:, j]
        M[0::2, 3 * j + 2] = -alphas[:, j] * x[:, 0]
        M[1::2, 3 * j + 1] = alphas[:, j]
        M[1::2, 3 * j + 2] = -alphas[:, j] * x[:, 1]
    _, V = np.linalg.eigh(M.T @ M)
    vs = [V[:, i] for i in range(4)]  # eigenvectors of the 4 smallest eigenvalues
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    dv = [[vs[i].reshape(4, 3)[a_] - vs[i].reshape(4, 3)[b_] for a_, b_ in pairs] for i in range(4)]
    L = np.zeros((6, 10))
    for r in range(6):
        d0, d1, d2, d3 = dv[0][r], dv[1][r], dv[2][r], dv[3][r]
        L[r] = [d0 @ d0, 2 * d0 @ d1, d1 @ d1, 2 * d0 @ d2, 2 * d1 @ d2, d2 @ d2, 2 * d0 @ d3, 2 * d1 @ d3, 2 * d2 @ d3, d3 @ d3]
    rho = np.array([np.sum((cws[a_] - cws[b_]) ** 2) for a_, b_ in pairs])
    lstsq = lambda A, b: np.linalg.lstsq(A, b, rcond=None)[0]  # noqa: E731
    betas = []
    b4 = lstsq(L[:, [0, 1, 3, 6]], rho)
    be = np.sqrt(-b4[0]) if b4[0] < 0 else np.sqrt(b4[0])
    betas.append(np.array([be, *(-b4[1:] / be if b4[0] < 0 else b4[1:] / be)]))
    b3 = lstsq(L[:, :3], rho)
    if b3[0] < 0:
        bb = [math.sqrt(-b3[0]), math.sqrt(-b3[2]) if b3[2] < 0 else 0.0]
    else:
        bb = [math.sqrt(b3[0]), math.sqrt(b3[2]) if b3[2] > 0 else 0.0]
    if b3[1] < 0:
        bb[0] = -bb[0]
    betas.append(np.array([bb[0], bb[1], 0.0, 0.0]))
    b5 = lstsq(L[:, :5], rho)
    if b5[0] < 0:
        bb = [math.sqrt(-b5[0]), math.sqrt(-b5[2]) if b5[2] < 0 else 0.0]
    else:
        bb = [math.sqrt(b5[0]), math.sqrt(b5[2]) if b5[2] > 0 else 0.0]
    if b5[1] < 0:
        bb[0] = -bb[0]
    betas.append(np.array([bb[0], bb[1], b5[3] / bb[0], 0.0]))
    models, errs = [], []
    for be in betas:
        be = be.copy()
        for _ in range(5):  # RunGaussNewton
            A = np.c_[2 * L[:, 0] * be[0] + L[:, 1] * be[1] + L[:, 3] * be[2] + L[:, 6] * be[3],
                      L[:, 1] * be[0] + 2 * L[:, 2] * be[1] + L[:, 4] * be[2] + L[:, 7] * be[3],
                      L[:, 3] * be[0] + L[:, 4] * be[1] + 2 * L[:, 5] * be[2] + L[:, 8] * be[3],
                      L[:, 6] * be[0] + L[:, 7] * be[1] + L[:, 8] * be[2] + 2 * L[:, 9] * be[3]]
            B = np.array([be[0] ** 2, be[0] * be[1], be[1] ** 2, be[0] * be[2], be[1] * be[2], be[2] ** 2, be[0] * be[3], be[1] * be[3],
                          be[2] * be[3], be[3] ** 2])
            be = be + lstsq(A, rho - L @ B)
        ccs = sum(be[i] * vs[i].reshape(4, 3) for i in range(4))
        pcs = alphas @ ccs
        if pcs[0, 2] < 0:  # SolveForSign
            pcs = -pcs
        R, t = _kabsch(X, pcs)
        P = np.c_[R, t]
        models.append(P)
        errs.append(float(np.sum(np.sqrt(residuals(P, x, X)))))
    best = 0
    if errs[1] < errs[0]:
        best = 1
    if errs[2] < errs[best]:
        best = 2
    if fragile is not None:
        for i in range(3):
            if (i != best and abs(errs[i] - errs[best]) <= 1e-9 * max(abs(errs[best]), 1e-300)
                    and np.abs(models[i] - models[best]).max() > 1e-10):
                fragile.append(("epnp_choice", errs[i], errs[best]))
    return models[best]


DEFAULT_OPTIONS = dict(max_error=12.0, min_inlier_ratio=0.25, confidence=0.99999, dyn_num_trials_multiplier=3.0, min_num_trials=100,
                       max_num_trials=10000, seed=0)


def estimate(points2D, points3D, intr, **opts) -> dict:
    """EstimateAbsolutePose on PINHOLE intr = (fx, fy, cx, cy).  Returns dict(success, cam_from_world [3,4] or None,
    num_inliers, inlier_mask, num_trials, max_num_trials, lo_rounds, fragile)."""
    o = dict(DEFAULT_OPTIONS)
    o.update(opts)
    p2 = np.asarray(points2D, np.float64).reshape(-1, 2)
    X = np.asarray(points3D, np.float64).reshape(-1, 3)
    fx, fy, cx, cy = (float(v) for v in intr)
    n = len(X)
    x = np.c_[(p2[:, 0] - cx) / fx, (p2[:, 1] - cy) / fy]
    thr = o["max_error"] / ((fx + fy) / 2.0)
    thr2 = thr * thr
    fragile: list = []
    out = dict(success=False, cam_from_world=None, num_inliers=0, inlier_mask=np.zeros(n, bool), num_trials=0, lo_rounds=0,
               fragile=fragile)
    if n < 3:
        return out
    max_trials = min(o["max_num_trials"], num_trials(int(o["min_inlier_ratio"] * 100000), 100000, o["confidence"],
                                                     o["dyn_num_trials_multiplier"]))
    out["max_num_trials"] = max_trials
    seed = int(o["seed"]) & MASK64

    def scored(P, best):
        res = residuals(P, x, X)
        sup = _support(res, thr2)
        near = int(np.sum(np.abs(res - thr2) <= 1e-7 * thr2))
        better = _better(sup, best)
        if near and (better or abs(sup[0] - best[0]) <= near):
            fragile.append(("threshold", near, sup[0], best[0]))
        if sup[0] == best[0] and sup[0] > 0:
            floor = 1e-10 * thr2 * sup[0]
            if sup[1] <= floor and best[1] <= floor:
                # models that fit their points to rounding level (a minimal sample explaining only itself): which one wins is
                # noise; it matters only if no model with more inliers comes later
                tie_counts.add(sup[0])
            elif abs(sup[1] - best[1]) <= 1e-9 * max(abs(sup[1]), abs(best[1]), 1e-300):
                fragile.append(("tie", sup, best))
        return res, sup, better

    best, best_model, best_cond = (0, DBL_MAX), None, 0.0
    tie_counts: set = set()
    dyn = max_trials
    abort = False
    trials = 0
    lo_rounds = 0
    while trials < max_trials:
        if abort:
            trials += 1
            break
        idx = sample(seed, trials, n)
        conds: list = []
        for model, cond in zip(p3p(x[idx], X[idx], fragile, conds), conds):
            res, sup, better = scored(model, best)
            if better:
                best, best_model, best_cond = sup, model, cond
                if sup[0] > 3 and sup[0] >= 4:
                    for _ in range(10):
                        inl = res <= thr2
                        prev = best[0]
                        lo_rounds += 1
                        lm = epnp(x[inl], X[inl], fragile)
                        if lm is not None:
                            lres, lsup, lbetter = scored(lm, best)
                            if lbetter:
                                best, best_model, res, best_cond = lsup, lm, lres, 0.0
                        if best[0] <= prev:
                            break
                dyn = num_trials(best[0], n, o["confidence"], o["dyn_num_trials_multiplier"])
            if trials >= dyn and trials >= o["min_num_trials"]:
                abort = True
                break
        trials += 1
    out.update(num_trials=trials, lo_rounds=lo_rounds)
    if best[0] < 3:
        return out
    if best[0] in tie_counts:
        fragile.append(("noise_tie", best[0]))
    if best_cond > 1e-13:
        fragile.append(("p3p_root_condition", best_cond))
    res = residuals(best_model, x, X)
    out.update(success=True, cam_from_world=best_model, num_inliers=best[0], inlier_mask=res <= thr2)
    return out


def synthetic_problem(n: int, outlier_ratio: float, seed: int, noise_px: float = 0.0, max_error: float = 12.0,
                      intr=(820.0, 790.0, 640.0, 480.0), size=(1280, 960)):
    """n 2D-3D pairs seen by a random camera: (points2D, points3D, intr, R, t, designed inlier mask).  Outliers get a random
    pixel more than 3 max_error away from their true projection."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = intr
    W, H = size
    a = rng.normal(size=3)
    ang = rng.uniform(0.1, 3.0)
    k = a / np.linalg.norm(a)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    t = rng.normal(size=3) * 2.0
    px = np.c_[rng.uniform(0, W, n), rng.uniform(0, H, n)]
    depth = rng.uniform(2.0, 12.0, n)
    Xc = np.c_[(px[:, 0] - cx) / fx * depth, (px[:, 1] - cy) / fy * depth, depth]
    X = (Xc - t) @ R
    p2 = px + rng.normal(size=(n, 2)) * noise_px
    inl = np.ones(n, bool)
    n_out = int(round(outlier_ratio * n))
    for i in rng.choice(n, n_out, replace=False):
        while True:
            q = np.array([rng.uniform(0, W), rng.uniform(0, H)])
            if np.linalg.norm(q - px[i]) > 3 * max_error:
                break
        p2[i] = q
        inl[i] = False
    return p2, X, np.array(intr), R, t, inl
