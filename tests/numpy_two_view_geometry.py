"""numpy_two_view_geometry.py — TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Independent NumPy restatement of ``pycolmap.estimate_calibrated_two_view_geometry`` (reference
mpsfm/sfm/scene/correspondences/utils.py:13-32): COLMAP 3.11 ``EstimateCalibratedTwoViewGeometry`` (three LO-RANSACs: E on
normalised points, F = seven-point + eight-point and H = normalised DLT on pixels, then the decision between them),
``DetectWatermark`` and ``EstimateTwoViewGeometryPose``, restated from the upstream sources as recalled.  The reference's
COLMAP fork is not in its tree: **parity unpinned**.

It shares no code with csrc/two_view_math.h / csrc/two_view.hip.  The nullspaces come from SVDs (HIP: Householder QR of the
sample, Jacobi sweeps of a 9 x 9 Gram matrix for the local estimators), the cubic's coefficients from four determinants
(HIP: expansion over permutations), its roots from ``np.roots`` plus a Newton polish (HIP: closed form plus deflation), the
local estimators from SVDs of the full n x 9 and 2n x 9 design matrices with two-pass Hartley normalisation (HIP: moments and
a centred Gram matrix reduced on the device), rank 2 and the homography decomposition from ``np.linalg.svd`` (HIP: Jacobi on
the 3 x 3 normal matrices) and the median from ``np.median``.  The sampler and the E leg are numpy_loransac's and
numpy_relative_pose's.

``estimate`` also reports FRAGILE decisions, which rounding may decide differently in another implementation: those of
numpy_relative_pose for every leg (threshold, tie, root_imag, double_root, lex_order, rank, cheirality), a cubic whose
leading coefficient nearly vanishes or whose root is huge, a nearly collinear triple of a four-point sample, inlier ratios
within one match of min_E_F_inlier_ratio / max_H_inlier_ratio / watermark_min_inlier_ratio, counts within one of
min_num_inliers, and max |Hn^T Hn - I| within 10 % of 1e-3.  Tests redraw such scenes.
"""

from __future__ import annotations

import math

import numpy as np

import numpy_relative_pose as NR
from numpy_loransac import MASK64, _better, _support
from numpy_loransac import num_trials as _num_trials
from numpy_loransac import sample as _sample

DBL_MAX = np.finfo(np.float64).max
DBL_EPS = np.finfo(np.float64).eps
RANK_TOL = 1e-12
COLLINEAR_TOL = 1e-10
MAX_ROOT_IMAG = NR.MAX_ROOT_IMAG

UNDEFINED, DEGENERATE, CALIBRATED, UNCALIBRATED, PLANAR, PANORAMIC, PLANAR_OR_PANORAMIC, WATERMARK, MULTIPLE = range(9)

# COLMAP 3.11 TwoViewGeometryOptions as recalled
DEFAULT_OPTIONS = dict(max_error=4.0, min_inlier_ratio=0.25, confidence=0.999, dyn_num_trials_multiplier=3.0, min_num_trials=100,
                       max_num_trials=10000, seed=0, min_num_inliers=15, min_E_F_inlier_ratio=0.95, max_H_inlier_ratio=0.8,
                       watermark_min_inlier_ratio=0.7, watermark_border_size=0.1, detect_watermark=True, compute_relative_pose=False)

canonical = NR.canonical
sampson = NR.sampson


def _q_rows(x1, x2):
    return np.c_[x2[:, :1] * x1[:, :1], x2[:, :1] * x1[:, 1:], x2[:, :1], x2[:, 1:] * x1[:, :1], x2[:, 1:] * x1[:, 1:], x2[:, 1:],
                 x1[:, :1], x1[:, 1:], np.ones((len(x1), 1))]


def _lex_sorted(models, fragile):
    models.sort(key=lambda M: tuple(M.reshape(-1)))
    if fragile is not None:
        for a in range(len(models) - 1):
            x, y = models[a].reshape(-1), models[a + 1].reshape(-1)
            nz = np.nonzero(y - x)[0]
            # relative to the entry: the leading entries of a unit-norm F or H in pixel units are many orders below 1, and so
            # are their rounding errors (numpy_relative_pose's absolute 1e-9 suits essential matrices, whose entries are O(1))
            if len(nz) and abs(y[nz[0]] - x[nz[0]]) <= 1e-7 * max(abs(x[nz[0]]), abs(y[nz[0]])):
                fragile.append(("lex_order", y[nz[0]] - x[nz[0]]))
    return models


# ---- F: seven-point and eight-point -------------------------------------------------------------------------------------
def seven_point(x1, x2, fragile: list | None = None):
    """FundamentalMatrixSevenPointEstimator::Estimate on 7 pixel matches: up to 3 canonical F in lexicographic order."""
    Q = _q_rows(x1, x2)
    _, s, Vt = np.linalg.svd(Q, full_matrices=True)
    if not s[6] > RANK_TOL * s[0]:
        if fragile is not None and s[6] > 1e-2 * RANK_TOL * s[0]:
            fragile.append(("rank", s[6] / s[0]))
        return []
    if fragile is not None and s[6] <= 1e2 * RANK_TOL * s[0]:
        fragile.append(("rank", s[6] / s[0]))
    F1, F2 = Vt[7].reshape(3, 3), Vt[8].reshape(3, 3)
    # det(F2 + l (F1 - F2)) = c3 l^3 + c2 l^2 + c1 l + c0 from its values at l = 0, 1, -1 and its leading term
    det = np.linalg.det
    c0, c3, p1, m1 = det(F2), det(F1 - F2), det(F1), det(2 * F2 - F1)
    c2 = 0.5 * (p1 + m1) - c0
    c1 = 0.5 * (p1 - m1) - c3
    coef = np.array([c3, c2, c1, c0])
    if not np.all(np.isfinite(coef)) or c3 == 0:
        return []
    if fragile is not None and abs(c3) <= 1e-9 * np.abs(coef).max():
        fragile.append(("cubic_lead", c3))
    roots = np.roots(coef).astype(complex)
    d1 = np.polyder(coef)
    for _ in range(2):
        dv = np.polyval(d1, roots)
        ok = dv != 0
        roots[ok] = roots[ok] - np.polyval(coef, roots[ok]) / dv[ok]
    scale = 1.0 + np.abs(roots)
    if fragile is not None:
        for r, sc in zip(roots, scale):
            if 0.1 * MAX_ROOT_IMAG * sc <= abs(r.imag) <= 10 * MAX_ROOT_IMAG * sc:
                fragile.append(("root_imag", r))
            if abs(r) > 1e6:
                fragile.append(("cubic_lead", r))
        for a in range(3):
            for b in range(a + 1, 3):
                if abs(roots[a] - roots[b]) <= 1e-7 * max(scale[a], scale[b]) and abs(roots[a].imag) <= 1e-6 * scale[a]:
                    fragile.append(("double_root", roots[a], roots[b]))
    models = []
    for r, sc in zip(roots, scale):
        if abs(r.imag) <= MAX_ROOT_IMAG * sc:
            F = canonical(r.real * F1 + (1 - r.real) * F2)
            if F is not None:
                models.append(F)
    return _lex_sorted(models, fragile)


def hartley(x):
    """CenterAndNormalizeImagePoints: (normalised points, T) with the centroid at 0 and RMS distance sqrt(2); None when the
    points coincide."""
    c = x.mean(axis=0)
    rms = math.sqrt(float(np.sum((x - c) ** 2)) / len(x))
    if not (rms > 0 and math.isfinite(rms)):
        return None
    s = math.sqrt(2.0) / rms
    return (x - c) * s, np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])


def _null_vector(A, route, fragile):
    """The right singular vector of the smallest singular value of A [m, 9] (rank >= 8 required), by SVD of A or by eigh of
    AᵀA."""
    if route == "svd":
        _, s, Vt = np.linalg.svd(A, full_matrices=A.shape[0] < 9)  # Vt is 9 x 9 either way; a full U would be m x m
        s = np.r_[s, np.zeros(9 - len(s))]
        ratio = s[7] / s[0] if s[0] > 0 else 0.0
        v = Vt[8]
    else:
        w, V = np.linalg.eigh(A.T @ A)
        ratio = math.sqrt(max(w[1], 0.0) / w[8]) if w[8] > 0 else 0.0
        v = V[:, 0]
    if not ratio > RANK_TOL:
        if fragile is not None and ratio > 1e-2 * RANK_TOL:
            fragile.append(("rank", ratio))
        return None
    if fragile is not None and ratio <= 1e2 * RANK_TOL:
        fragile.append(("rank", ratio))
    return v


def eight_point(x1, x2, fragile: list | None = None, route: str = "svd"):
    """FundamentalMatrixEightPointEstimator::Estimate on n >= 8 pixel matches: [F] or []."""
    if len(x1) < 8:
        return []
    h1, h2 = hartley(x1), hartley(x2)
    if h1 is None or h2 is None:
        return []
    (n1, T1), (n2, T2) = h1, h2
    v = _null_vector(_q_rows(n1, n2), route, fragile)
    if v is None:
        return []
    U, s, Vt = np.linalg.svd(v.reshape(3, 3))
    Fh = U @ np.diag([s[0], s[1], 0.0]) @ Vt
    F = canonical(T2.T @ Fh @ T1)
    return [] if F is None else [F]


# ---- H: normalised DLT --------------------------------------------------------------------------------------------------
def h_residual(H, x1, x2):
    """Squared forward transfer error; DBL_MAX where the third homogeneous coordinate is 0."""
    y = np.c_[x1, np.ones(len(x1))] @ H.T
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (x2[:, 0] - y[:, 0] / y[:, 2]) ** 2 + (x2[:, 1] - y[:, 1] / y[:, 2]) ** 2
    return np.where(y[:, 2] == 0, DBL_MAX, r)


def _collinear4(x, fragile):
    for a, b, c in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
        u, v = x[b] - x[a], x[c] - x[a]
        cr, den = abs(u[0] * v[1] - u[1] * v[0]), math.sqrt(float(u @ u) * float(v @ v))
        if fragile is not None and 1e-2 * COLLINEAR_TOL * den < cr <= 1e2 * COLLINEAR_TOL * den:
            fragile.append(("collinear", cr / den))
        if not cr > COLLINEAR_TOL * den:
            return True
    return False


def homography_dlt(x1, x2, fragile: list | None = None, route: str = "svd"):
    """HomographyMatrixEstimator::Estimate on n >= 4 pixel matches: [H] or [].  A four-point sample with a collinear triple
    in either image gives no model."""
    if len(x1) < 4:
        return []
    if len(x1) == 4 and (_collinear4(x1, fragile) or _collinear4(x2, fragile)):
        return []
    h1, h2 = hartley(x1), hartley(x2)
    if h1 is None or h2 is None:
        return []
    (n1, T1), (n2, T2) = h1, h2
    m = len(x1)
    A = np.zeros((2 * m, 9))
    A[0::2, 0:2], A[0::2, 2] = -n1, -1.0
    A[0::2, 6:8], A[0::2, 8] = n2[:, :1] * n1, n2[:, 0]
    A[1::2, 3:5], A[1::2, 5] = -n1, -1.0
    A[1::2, 6:8], A[1::2, 8] = n2[:, 1:] * n1, n2[:, 1]
    v = _null_vector(A, route, fragile)
    if v is None:
        return []
    H = canonical(np.linalg.inv(T2) @ v.reshape(3, 3) @ T1)
    return [] if H is None else [H]


# ---- LO-RANSAC ----------------------------------------------------------------------------------------------------------
def loransac(n, sample_size, minimal, local, residuals, thr2, o, fragile):
    """LORANSAC as csrc/lo_ransac.h replays it.  minimal(idx, fragile list of the trial) -> models, local(inlier mask) ->
    models, residuals(model) -> [n].  The order of two nearly equal models of a trial only matters when one of them
    becomes the best model (otherwise the loop's state does not change): a trial's lex_order entries count only then.  Returns dict(success, model, num_inliers, inlier_mask, num_trials, max_num_trials, lo_rounds)."""
    max_trials = min(o["max_num_trials"], _num_trials(int(o["min_inlier_ratio"] * 100000), 100000, o["confidence"],
                                                      o["dyn_num_trials_multiplier"], sample_size))
    seed = int(o["seed"]) & MASK64
    out = dict(success=False, model=None, num_inliers=0, inlier_mask=np.zeros(n, bool), num_trials=0, max_num_trials=max_trials, lo_rounds=0)
    if n < sample_size:
        out["max_num_trials"] = 0
        return out

    best, best_model = (0, DBL_MAX), None
    exact_ties: list = []

    def scored(model, best):
        res = residuals(model)
        sup = _support(res, thr2)
        near = int(np.sum(np.abs(res - thr2) <= 1e-7 * thr2))
        better = _better(sup, best)
        if near and (better or abs(sup[0] - best[0]) <= near):
            fragile.append(("threshold", near, sup[0], best[0]))
        if sup[0] == best[0] and sup[0] > 0:
            if abs(sup[1] - best[1]) <= 1e-9 * max(abs(sup[1]), abs(best[1]), 1e-300):
                fragile.append(("tie", sup, best))
            # two exact fits (a minimal sample that explains only itself, noise-free inliers): both residual sums are rounding
            # noise (below 1e-12 of the threshold per inlier), so rounding picks the winner; that matters unless the two are
            # the same model
            # anyway, or a model with more inliers supersedes both (checked when the loop ends)
            elif max(sup[1], best[1]) <= 1e-12 * thr2 * sup[0] and np.abs(np.asarray(model) - np.asarray(best_model)).max() > 1e-10:
                exact_ties.append(sup[0])
        return res, sup, better

    dyn, abort, trials, lo_rounds = max_trials, False, 0, 0
    while trials < max_trials:
        if abort:
            trials += 1
            break
        trial_fragile: list = []
        updated = False
        for model in minimal(_sample(seed, trials, n, sample_size), trial_fragile):
            res, sup, better = scored(model, best)
            if better:
                updated = True
                best, best_model = sup, model
                if sup[0] > sample_size:
                    for _ in range(10):
                        prev = best[0]
                        lo_rounds += 1
                        for lm in local(res <= thr2):
                            lres, lsup, lbetter = scored(lm, best)
                            if lbetter:
                                best, best_model, res = lsup, lm, lres  # noqa: F841 (scored reads best_model)
                        if best[0] <= prev:
                            break
                dyn = _num_trials(best[0], n, o["confidence"], o["dyn_num_trials_multiplier"], sample_size)
            if trials >= dyn and trials >= o["min_num_trials"]:
                abort = True
                break
        fragile.extend(f for f in trial_fragile if updated or f[0] != "lex_order")
        trials += 1
    if best[0] in exact_ties and best[1] <= 1e-12 * thr2 * best[0]:
        fragile.append(("tie", best, exact_ties.count(best[0])))
    out.update(num_trials=trials, lo_rounds=lo_rounds, num_inliers=best[0])
    if best[0] < sample_size:
        return out
    out.update(success=True, model=best_model, inlier_mask=residuals(best_model) <= thr2)
    return out


def _ransac_opts(o):
    return {k: o[k] for k in ("max_error", "min_inlier_ratio", "confidence", "dyn_num_trials_multiplier", "min_num_trials", "max_num_trials",
                              "seed")}


def f_leg(p1, p2, o, fragile, route="svd"):
    return loransac(len(p1), 7, lambda idx, fr: seven_point(p1[idx], p2[idx], fr), lambda inl: eight_point(p1[inl], p2[inl], fragile, route),
                    lambda F: sampson(F, p1, p2), o["max_error"] ** 2, o, fragile)


def h_leg(p1, p2, o, fragile, route="svd"):
    return loransac(len(p1), 4, lambda idx, fr: homography_dlt(p1[idx], p2[idx], fr),
                    lambda inl: homography_dlt(p1[inl], p2[inl], fragile, route), lambda H: h_residual(H, p1, p2), o["max_error"] ** 2, o,
                    fragile)


def _five_point(x1, x2, fragile):
    """numpy_relative_pose.five_point with a thin SVD for many matches (its full U would be n x n)."""
    if len(x1) < 9:
        return NR.five_point(x1, x2, fragile)
    _, s, Vt = np.linalg.svd(_q_rows(x1, x2), full_matrices=False)
    if not s[4] > NR.RANK_TOL * s[0]:
        if s[4] > 1e-2 * NR.RANK_TOL * s[0]:
            fragile.append(("rank", s[4] / s[0]))
        return []
    if s[4] <= 1e2 * NR.RANK_TOL * s[0]:
        fragile.append(("rank", s[4] / s[0]))
    return NR.models_from_nullspace(Vt[5:9], fragile)


def e_leg(p1, p2, K1, K2, o, fragile):
    """The estimator of numpy_relative_pose.estimate (five-point samples and local estimator, Sampson error on normalised
    points, threshold 0.5 (max_error / f1 + max_error / f2)) without its pose."""
    x1, x2 = NR.normalise(p1, K1), NR.normalise(p2, K2)
    thr = 0.5 * (o["max_error"] / ((K1[0] + K1[1]) / 2.0) + o["max_error"] / ((K2[0] + K2[1]) / 2.0))
    return loransac(len(x1), 5, lambda idx, fr: NR.five_point(x1[idx], x2[idx], fr), lambda inl: _five_point(x1[inl], x2[inl], fragile),
                    lambda E: sampson(E, x1, x2), thr * thr, o, fragile)


def translation_leg(p1, p2, o, fragile):
    d = p2 - p1
    return loransac(len(d), 1, lambda idx, fr: [d[idx].mean(axis=0)], lambda inl: [d[inl].mean(axis=0)] if inl.any() else [],
                    lambda t: np.sum((d - t) ** 2, axis=1), o["max_error"] ** 2, o, fragile)


# ---- pose -----------------------------------------------------------------------------------------------------------------
def triangulation_angle(C1, C2, X):
    """CalculateTriangulationAngle for points X [m, 3]: the geometric angle at X, folded to [0, pi / 2]."""
    b2 = float(np.sum((C1 - C2) ** 2))
    r1 = np.sum((X - C1) ** 2, axis=1)
    r2 = np.sum((X - C2) ** 2, axis=1)
    den = 2.0 * np.sqrt(r1 * r2)
    with np.errstate(divide="ignore", invalid="ignore"):
        ang = np.abs(np.arccos(np.clip((r1 + r2 - b2) / den, -1.0, 1.0)))
    ang = np.minimum(ang, np.pi - ang)
    return np.where(den == 0, 0.0, ang)


def cheirality_points(R, t, x1, x2):
    """CheckCheirality: (mask of the matches whose two-view DLT point has both depths in (eps, 1000 |t|), the points, the
    number of uncertain matches)."""
    m = len(x1)
    P2 = np.c_[R, t]
    A = np.zeros((m, 4, 4))
    A[:, 0] = x1[:, :1] * np.array([0, 0, 1, 0.0]) - np.array([1, 0, 0, 0.0])
    A[:, 1] = x1[:, 1:] * np.array([0, 0, 1, 0.0]) - np.array([0, 1, 0, 0.0])
    A[:, 2] = x2[:, :1] * P2[2] - P2[0]
    A[:, 3] = x2[:, 1:] * P2[2] - P2[1]
    Xh = np.linalg.svd(A)[2][:, 3, :] if m else np.zeros((0, 4))
    with np.errstate(divide="ignore", invalid="ignore"):
        X = Xh[:, :3] / Xh[:, 3:]
    d1 = X[:, 2]
    d2 = X @ R[2] + t[2]
    hi = 1000.0 * np.linalg.norm(t)
    with np.errstate(invalid="ignore"):
        ok = (d1 > DBL_EPS) & (d1 < hi) & (d2 > DBL_EPS) & (d2 < hi)
        far = np.abs(Xh[:, 3]) <= 1e-9 * np.linalg.norm(Xh, axis=1)
        near = lambda d: (np.abs(d - hi) <= 1e-9 * hi) | (np.abs(d) <= 1e-12)  # noqa: E731
        unsure = (far | near(d1) | near(d2)) if hi > 0 else np.zeros(m, bool)
    return ok, X, int(np.sum(unsure))


def pick_pose(cands, x1, x2, fragile):
    """The candidate with the most cheirality points, the later one on a tie: (P [3,4], count, counts, tri_angle)."""
    results = [cheirality_points(R, t, x1, x2) for R, t in cands]
    counts = [int(ok.sum()) for ok, _, _ in results]
    best, best_n = 0, -1
    for i, c in enumerate(counts):
        if c >= best_n:
            best, best_n = i, c
    if fragile is not None:
        for i, c in enumerate(counts):
            if i != best and best_n - c <= results[i][2] + results[best][2] and (best_n > 0 or results[i][2] + results[best][2] > 0):
                fragile.append(("cheirality", i, c, best_n))
    R, t = cands[best]
    ok, X, _ = results[best]
    ang = triangulation_angle(np.zeros(3), -R.T @ t, X[ok])
    return np.c_[R, t], best_n, counts, (float(np.median(ang)) if len(ang) else 0.0)


def Kmat(intr):
    fx, fy, cx, cy = (float(v) for v in intr)
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])


def decompose_homography(H, K1, K2, fragile: list | None = None):
    """DecomposeHomographyMatrix on Hn = K2^-1 H K1 / sigma_2 (det > 0): [(R, t)] in OUR order (module docstring of the
    product: include/mpsfm_hip.h); a single (Hn, 0) when max |HnᵀHn - I| < 1e-3."""
    Hn = np.linalg.inv(Kmat(K2)) @ H @ Kmat(K1)
    Hn = Hn / np.linalg.svd(Hn)[1][1]
    if np.linalg.det(Hn) < 0:
        Hn = -Hn
    dev = float(np.abs(Hn.T @ Hn - np.eye(3)).max())
    if fragile is not None and 0.9e-3 <= dev <= 1.1e-3:
        fragile.append(("near_rotation", dev))
    if dev < 1e-3:
        return [(Hn, np.zeros(3))]
    _, s, Vt = np.linalg.svd(Hn)
    v1, v2 = Vt[0], Vt[1]
    v3 = np.cross(v1, v2)
    l1, l3 = s[0] ** 2, s[2] ** 2
    a, b, den = math.sqrt(max(0.0, 1 - l3)), math.sqrt(max(0.0, l1 - 1)), math.sqrt(l1 - l3)
    sols = []
    for sb in (1.0, -1.0):
        u = (a * v1 + sb * b * v3) / den
        nrm = np.cross(v2, u)
        U = np.c_[v2, u, nrm]
        W = np.c_[Hn @ v2, Hn @ u, np.cross(Hn @ v2, Hn @ u)]
        R = W @ U.T
        t = (Hn - R) @ nrm
        if t[int(np.argmax(np.abs(t)))] < 0:
            t = -t
        sols.append((R, t))
    ka, kb = tuple(sols[0][0].reshape(-1)), tuple(sols[1][0].reshape(-1))
    if fragile is not None:
        d = np.array(kb) - np.array(ka)
        nz = np.nonzero(d)[0]
        if len(nz) and abs(d[nz[0]]) <= 1e-9:
            fragile.append(("lex_order", d[nz[0]]))
    if kb < ka:
        sols = sols[::-1]
    (Ra, ta), (Rb, tb) = sols
    return [(Ra, ta), (Rb, tb), (Ra, -ta), (Rb, -tb)]


def pose_candidates_from_E(E):
    R1, R2, t = NR.decompose(E)
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


# ---- the estimator ------------------------------------------------------------------------------------------------------
def _ratio(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


def _ratio_gt(a, b, thr, fragile, tag):
    """a / b > thr; fragile when one match more or less on either side changes the answer."""
    ans = _ratio(a, b) > thr
    for da, db in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        if a + da >= 0 and b + db >= 0 and (_ratio(a + da, b + db) > thr) != ans:
            fragile.append((tag, a, b))
            break
    return ans


def _ratio_ge(a, b, thr, fragile, tag):
    """a / b >= thr; fragile when one match more or less in the numerator changes the answer."""
    ans = _ratio(a, b) >= thr
    if (_ratio(a + 1, b) >= thr) != ans or (_ratio(a - 1, b) >= thr) != ans:
        fragile.append((tag, a, b))
    return ans


def _at_least(a, m, fragile, tag):
    if abs(a - m) <= 1:
        fragile.append((tag, a, m))
    return a >= m


def estimate(points1, points2, intr1, intr2, size1, size2, route="svd", **opts) -> dict:
    """estimate_calibrated_two_view_geometry on PINHOLE intr = (fx, fy, cx, cy) and sizes (width, height).  Returns
    dict(config, success, E, F, H ([3,3] or None), cam2_from_cam1 [3,4], tri_angle, inlier_mask, num_inliers, legs (dict E /
    F / H / T -> report or None), num_cheirality_points, watermark, fragile)."""
    o = dict(DEFAULT_OPTIONS)
    unknown = set(opts) - set(o)
    if unknown:
        raise KeyError(f"unknown option(s) {sorted(unknown)}")
    o.update(opts)
    p1 = np.asarray(points1, np.float64).reshape(-1, 2)
    p2 = np.asarray(points2, np.float64).reshape(-1, 2)
    n = len(p1)
    fragile: list = []
    out = dict(config=DEGENERATE, success=False, E=None, F=None, H=None, cam2_from_cam1=np.eye(3, 4), tri_angle=0.0,
               inlier_mask=np.zeros(n, bool), num_inliers=0, legs=dict(E=None, F=None, H=None, T=None), num_cheirality_points=0,
               watermark=False, fragile=fragile)
    minI = int(o["min_num_inliers"])
    if n < minI or n < 4:
        return out
    rE = e_leg(p1, p2, intr1, intr2, o, fragile)
    rF = f_leg(p1, p2, o, fragile, route)
    rH = h_leg(p1, p2, o, fragile, route)
    out["legs"].update(E=rE, F=rF, H=rH)
    out.update(E=rE["model"], F=rF["model"], H=rH["model"])
    nE, nF, nH = rE["num_inliers"], rF["num_inliers"], rH["num_inliers"]

    config, chosen = DEGENERATE, None
    if not (rE["success"] or rF["success"] or rH["success"]) or (nE < minI and nF < minI and nH < minI):
        for c in (nE, nF, nH):
            _at_least(c, minI, fragile, "min_inliers")
    elif rE["success"] and _ratio_gt(nE, nF, o["min_E_F_inlier_ratio"], fragile, "E_F_ratio") and _at_least(nE, minI, fragile, "min_inliers"):
        chosen = rE if nE >= nF else rF
        if _ratio_gt(nH, nE, o["max_H_inlier_ratio"], fragile, "H_E_ratio"):
            config = PLANAR_OR_PANORAMIC
            if nH > max(nE, nF):
                chosen = rH
        else:
            config = CALIBRATED
    elif rF["success"] and _at_least(nF, minI, fragile, "min_inliers"):
        chosen = rF
        if _ratio_gt(nH, nF, o["max_H_inlier_ratio"], fragile, "H_F_ratio"):
            config = PLANAR_OR_PANORAMIC
            if nH > nF:
                chosen = rH
        else:
            config = UNCALIBRATED
    elif rH["success"] and _at_least(nH, minI, fragile, "min_inliers"):
        chosen, config = rH, PLANAR_OR_PANORAMIC
    out["config"] = config
    if chosen is None:
        return out
    mask = chosen["inlier_mask"]
    nsel = int(mask.sum())
    out.update(inlier_mask=mask, num_inliers=nsel, success=True)

    if o["detect_watermark"]:
        def outside(p, size):
            b = o["watermark_border_size"] * math.hypot(size[0], size[1])
            return ~((p[:, 0] >= b) & (p[:, 0] <= size[0] - b) & (p[:, 1] >= b) & (p[:, 1] <= size[1] - b))

        border = mask & outside(p1, size1) & outside(p2, size2)
        m = int(border.sum())
        wr = o["watermark_min_inlier_ratio"]
        if m > 0 and _ratio_ge(m, nsel, wr, fragile, "border_ratio"):
            rT = translation_leg(p1[border], p2[border], dict(o, min_inlier_ratio=wr), fragile)
            out["legs"]["T"] = rT
            if _ratio_ge(rT["num_inliers"], nsel, wr, fragile, "watermark_ratio"):
                config = WATERMARK
                out["watermark"] = True
    out["config"] = config

    if o["compute_relative_pose"] and config in (CALIBRATED, UNCALIBRATED, PLANAR_OR_PANORAMIC):
        x1, x2 = NR.normalise(p1, intr1)[mask], NR.normalise(p2, intr2)[mask]
        if config == CALIBRATED:
            cands = pose_candidates_from_E(rE["model"])
        elif config == UNCALIBRATED:
            cands = pose_candidates_from_E(canonical(Kmat(intr2).T @ rF["model"] @ Kmat(intr1)))
        else:
            cands = decompose_homography(rH["model"], intr1, intr2, fragile)
        P, npts, counts, ang = pick_pose(cands, x1, x2, fragile)
        out.update(cam2_from_cam1=P, num_cheirality_points=npts, cheirality_counts=counts, tri_angle=ang)
        if config == PLANAR_OR_PANORAMIC:
            config = PANORAMIC if not np.any(P[:, 3]) else PLANAR
            if config == PANORAMIC:
                out["tri_angle"] = 0.0
        out["config"] = config
    return out


# ---- synthetic pairs ------------------------------------------------------------------------------------------------------
SIZE1 = (int(2 * NR.INTR1[2]), int(2 * NR.INTR1[3]))
SIZE2 = (int(2 * NR.INTR2[2]), int(2 * NR.INTR2[3]))
KINDS = ("general", "wrong_intrinsics", "planar", "rotation", "random", "watermark", "weak")


def synthetic_pair(kind: str, n: int, outlier_ratio: float, seed: int, noise_px: float = 0.0):
    """n matches of one kind: dict(points1, points2, intr1, intr2 (what the estimator is given), size1, size2, R, t (truth, None
    where there is none), expect (the config the decision table should give with compute_relative_pose))."""
    rng = np.random.default_rng(seed + 77)
    K1, K2 = np.array(NR.INTR1), np.array(NR.INTR2)
    base = dict(intr1=K1, intr2=K2, size1=SIZE1, size2=SIZE2, R=None, t=None)
    if kind in ("general", "planar", "wrong_intrinsics", "weak"):
        # "weak": a planar scene whose caller leaves fewer than min_num_inliers designed inliers among the outliers
        p1, p2, _, _, R, t, inl = NR.synthetic_problem(n, outlier_ratio, seed, noise_px, planar=kind in ("planar", "weak"))
        base.update(points1=p1, points2=p2, R=R, t=t, inliers=inl,
                    expect=PLANAR if kind == "planar" else DEGENERATE if kind == "weak" else CALIBRATED)
        if kind == "wrong_intrinsics":  # the estimator is told focal lengths and principal points far from the truth
            base.update(intr1=K1 * np.array([0.45, 0.5, 0.6, 1.3]), intr2=K2 * np.array([1.9, 1.7, 1.4, 0.7]), expect=UNCALIBRATED)
        return base
    if kind == "rotation":
        R = NR._rot(rng.normal(size=3), rng.uniform(0.05, 0.2))
        p1 = np.zeros((0, 2))
        p2 = np.zeros((0, 2))
        while len(p1) < n:
            m = 2 * (n - len(p1)) + 16
            a = np.c_[rng.uniform(0, SIZE1[0], m), rng.uniform(0, SIZE1[1], m)]
            ray = np.c_[(a[:, 0] - K1[2]) / K1[0], (a[:, 1] - K1[3]) / K1[1], np.ones(m)] @ R.T
            b = np.c_[K2[0] * ray[:, 0] / ray[:, 2] + K2[2], K2[1] * ray[:, 1] / ray[:, 2] + K2[3]]
            ok = (ray[:, 2] > 0.1) & (b[:, 0] >= 0) & (b[:, 0] < SIZE2[0]) & (b[:, 1] >= 0) & (b[:, 1] < SIZE2[1])
            p1, p2 = np.r_[p1, a[ok]][:n], np.r_[p2, b[ok]][:n]
        p1 = p1 + rng.normal(size=p1.shape) * noise_px
        p2 = p2 + rng.normal(size=p2.shape) * noise_px
        inl = np.ones(n, bool)
        for i in rng.choice(n, int(round(outlier_ratio * n)), replace=False):
            while True:
                q = np.array([rng.uniform(0, SIZE2[0]), rng.uniform(0, SIZE2[1])])
                if np.linalg.norm(q - p2[i]) > 40:
                    break
            p2[i], inl[i] = q, False
        base.update(points1=p1, points2=p2, R=R, t=np.zeros(3), inliers=inl, expect=PANORAMIC)
        return base
    if kind == "random":
        base.update(points1=np.c_[rng.uniform(0, SIZE1[0], n), rng.uniform(0, SIZE1[1], n)],
                    points2=np.c_[rng.uniform(0, SIZE2[0], n), rng.uniform(0, SIZE2[1], n)], inliers=np.zeros(n, bool), expect=DEGENERATE)
        return base
    if kind == "watermark":
        shift = np.array([9.0, -6.0])
        b1, b2 = 0.1 * math.hypot(*SIZE1), 0.1 * math.hypot(*SIZE2)
        pts = np.zeros((0, 2))
        while len(pts) < n:
            a = np.c_[rng.uniform(0, SIZE1[0], 4 * n), rng.uniform(0, SIZE1[1], 4 * n)]
            b = a + shift
            out1 = ~((a[:, 0] >= b1) & (a[:, 0] <= SIZE1[0] - b1) & (a[:, 1] >= b1) & (a[:, 1] <= SIZE1[1] - b1))
            out2 = ~((b[:, 0] >= b2) & (b[:, 0] <= SIZE2[0] - b2) & (b[:, 1] >= b2) & (b[:, 1] <= SIZE2[1] - b2))
            inside = (b[:, 0] >= 0) & (b[:, 0] < SIZE2[0]) & (b[:, 1] >= 0) & (b[:, 1] < SIZE2[1])
            pts = np.r_[pts, a[out1 & out2 & inside]][:n]
        p1 = pts + rng.normal(size=pts.shape) * noise_px
        p2 = pts + shift + rng.normal(size=pts.shape) * noise_px
        inl = np.ones(n, bool)
        for i in rng.choice(n, int(round(outlier_ratio * n)), replace=False):
            while True:
                q = np.array([rng.uniform(0, SIZE2[0]), rng.uniform(0, SIZE2[1])])
                if np.linalg.norm(q - p2[i]) > 40:
                    break
            p2[i], inl[i] = q, False
        base.update(points1=p1, points2=p2, inliers=inl, expect=WATERMARK)
        return base
    raise KeyError(kind)
