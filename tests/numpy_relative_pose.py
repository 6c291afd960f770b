"""numpy_relative_pose.py — TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Independent NumPy restatement of ``pycolmap.essential_matrix_estimation`` (reference
mpsfm/sfm/estimators/relative_pose.py:7-17): COLMAP 3.11 ``EstimateEssentialMatrix`` =
``LORANSAC<EssentialMatrixFivePointEstimator, EssentialMatrixFivePointEstimator, InlierSupportMeasurer>`` on
CamFromImg-normalised points, then ``PoseFromEssentialMatrix`` on the inliers, restated from the upstream sources as recalled.
The reference's COLMAP fork is not in its tree: **parity unpinned**.

It shares no code with csrc/rel_pose_math.h / csrc/rel_pose.hip: the nullspace comes from an SVD of the epipolar matrix Q
(the HIP path: Householder QR of the 5 x 9 sample, Jacobi sweeps of the 9 x 9 QᵀQ for the local estimator), the cubic
constraints are built by einsum over monomial incidence tensors, the elimination is ``np.linalg.solve``, the degree-10 roots come from
``np.roots`` (companion matrix) plus a Newton polish (HIP: Aberth iteration), the (x, y) of a root is the SVD null vector of
the 3 x 3 B(z) (HIP: a cross product of two rows), the essential-matrix decomposition is ``np.linalg.svd`` (HIP: Jacobi on EᵀE)
and the triangulation is a batched 4 x 4 SVD.  The sampler is the documented counter-based recipe computed with Python ints.

``estimate`` also reports FRAGILE decisions, which rounding may decide differently in another implementation: a residual
within 1e-7 (relative) of the threshold in a model whose support decided something, equal inlier counts whose residual sums
are within 1e-9 (relative), a root whose imaginary part is within a factor of 10 of the cut-off, roots closer than 1e-7
(relative), two models of one trial whose lexicographic keys first differ by less than 1e-9, a sample whose fifth singular value
is within a factor of 100 of the rank cut-off, and cheirality counts whose winner is within the number of near-infinite or
boundary-depth points of another candidate.  Tests redraw such scenes.
"""

from __future__ import annotations

import math

import numpy as np

from numpy_loransac import MASK64, PHI, _better, _mix, _support  # noqa: F401  (names the tests use)
from numpy_loransac import num_trials as _num_trials
from numpy_loransac import sample as _sample

DBL_MAX = np.finfo(np.float64).max
DBL_EPS = np.finfo(np.float64).eps
MAX_ROOT_IMAG = 1e-10  # relative to 1 + |z|
RANK_TOL = 1e-12       # fifth singular value / largest: below it the nullspace is larger than 4
SAMPLE_SIZE = 5


def sample(seed: int, t: int, n: int, k: int = SAMPLE_SIZE) -> list[int]:
    """The k distinct indices of trial t."""
    return _sample(seed, t, n, k)


def num_trials(num_inliers: int, n: int, confidence: float, multiplier: float, sample_size: int = SAMPLE_SIZE) -> float:
    """RANSAC::ComputeNumTrials with kMinNumSamples = sample_size (math.inf for size_t max)."""
    return _num_trials(num_inliers, n, confidence, multiplier, sample_size)


def sampson(E: np.ndarray, x1: np.ndarray, x2: np.ndarray) -> np.ndarray:
    """ComputeSquaredSampsonError of x2ᵀ E x1 on normalised points [n, 2]."""
    X1, X2 = np.c_[x1, np.ones(len(x1))], np.c_[x2, np.ones(len(x2))]
    Ex1 = X1 @ E.T
    Etx2 = X2 @ E
    num = np.sum(X2 * Ex1, axis=1) ** 2
    den = Ex1[:, 0] ** 2 + Ex1[:, 1] ** 2 + Etx2[:, 0] ** 2 + Etx2[:, 1] ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        return num / den


# ---- five-point solver ----------------------------------------------------------------------------------------------
# polynomials in (x, y, z) as coefficient vectors over monomial bases; products through 0/1 incidence tensors
# monomial order of the 10 x 20 system: the 10 eliminated, then xz², xz, x, yz², yz, y, z³, z², z, 1
MONOMIALS = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
             (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]
_LIN = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
_QUAD = sorted({tuple(a + b for a, b in zip(p, q)) for p in _LIN for q in _LIN})


def _incidence(left, right, out):
    T = np.zeros((len(left), len(right), len(out)))
    for i, p in enumerate(left):
        for j, q in enumerate(right):
            T[i, j, out.index(tuple(a + b for a, b in zip(p, q)))] = 1.0
    return T


_T2 = _incidence(_LIN, _LIN, _QUAD)
_T3 = _incidence(_QUAD, _LIN, MONOMIALS)
_EPS = np.zeros((3, 3, 3))
for _a, _b, _c in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
    _EPS[_a, _b, _c], _EPS[_a, _c, _b] = 1.0, -1.0


def constraint_matrix(N: np.ndarray) -> np.ndarray:
    """The 10 x 20 coefficients of det(E) = 0 and 2 E Eᵀ E - tr(E Eᵀ) E = 0 for E = x N0 + y N1 + z N2 + N3."""
    El = N.T.reshape(3, 3, 4)  # El[i, j] = coefficients of E_ij in (x, y, z, 1)
    q12 = np.einsum("bx,cy,xyq->bcq", El[1], El[2], _T2)
    det = np.einsum("abc,ax,bcq,qxm->m", _EPS, El[0], q12, _T3)
    EEt = np.einsum("ika,jkb,abq->ijq", El, El, _T2)
    M = 2.0 * EEt - np.eye(3)[:, :, None] * (EEt[0, 0] + EEt[1, 1] + EEt[2, 2])[None, None, :]
    C = np.einsum("ikq,kja,qam->ijm", M, El, _T3)
    return np.vstack([det[None], C.reshape(9, 20)])


def models_from_nullspace(N: np.ndarray, fragile: list | None = None) -> list[np.ndarray]:
    """The canonical essential matrices of the 4-D nullspace N [4, 9], in lexicographic order."""
    A = constraint_matrix(N)
    try:
        AA = np.linalg.solve(A[:, :10], A[:, 10:])
    except np.linalg.LinAlgError:
        return []
    if not np.all(np.isfinite(AA)):
        return []

    def rows(e, f):  # x, y and 1 coefficients of e - z f as polynomials in z (highest power first, padded to degree 4)
        return [[0.0, -f[0], e[0] - f[1], e[1] - f[2], e[2]], [0.0, -f[3], e[3] - f[4], e[4] - f[5], e[5]],
                [-f[6], e[6] - f[7], e[7] - f[8], e[8] - f[9], e[9]]]

    Bp = np.array([rows(AA[4], AA[5]), rows(AA[6], AA[7]), rows(AA[8], AA[9])])  # [3, 3, 5]
    cv = np.convolve
    det = np.zeros(13)
    for a, b, c, s in ((0, 1, 2, 1), (0, 2, 1, -1), (1, 0, 2, -1), (1, 2, 0, 1), (2, 0, 1, 1), (2, 1, 0, -1)):
        det += s * cv(Bp[0, a], cv(Bp[1, b], Bp[2, c]))
    det = det[2:]  # degree 10
    if not np.all(np.isfinite(det)) or det[0] == 0:
        return []
    roots = np.roots(det).astype(complex)
    d1 = np.polyder(det)
    for _ in range(2):  # Newton polish
        dv = np.polyval(d1, roots)
        ok = dv != 0
        roots[ok] = roots[ok] - np.polyval(det, roots[ok]) / dv[ok]
    scale = 1.0 + np.abs(roots)
    if fragile is not None:
        for r, s in zip(roots, scale):
            if 0.1 * MAX_ROOT_IMAG * s <= abs(r.imag) <= 10 * MAX_ROOT_IMAG * s:
                fragile.append(("root_imag", r))
    real = [r.real for r, s in zip(roots, scale) if abs(r.imag) <= MAX_ROOT_IMAG * s]
    if fragile is not None:
        for a in range(len(roots)):
            for b in range(a + 1, len(roots)):
                if abs(roots[a] - roots[b]) <= 1e-7 * max(scale[a], scale[b]) and (abs(roots[a].imag) <= 1e-6 * scale[a]):
                    fragile.append(("double_root", roots[a], roots[b]))
    models = []
    for z in real:
        B = Bp[..., 0]
        for c in range(1, 5):
            B = B * z + Bp[..., c]
        v = np.linalg.svd(B)[2][2]
        if v[2] == 0:
            continue
        E = canonical(polish(N, np.array([v[0] / v[2], v[1] / v[2], z])))
        if E is not None:
            models.append(E)
    models.sort(key=lambda E: tuple(E.reshape(-1)))
    if fragile is not None:
        for a in range(len(models) - 1):
            d = models[a + 1].reshape(-1) - models[a].reshape(-1)
            nz = np.nonzero(d)[0]
            if len(nz) and abs(d[nz[0]]) <= 1e-9:
                fragile.append(("lex_order", d[nz[0]]))
    return models


def _constraints(N, p):
    """The ten constraints at E(p) = x N0 + y N1 + z N2 + N3 and their Jacobian in (x, y, z)."""
    E = (p[0] * N[0] + p[1] * N[1] + p[2] * N[2] + N[3]).reshape(3, 3)
    e0, e1, e2 = E
    cof = np.array([[e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]],
                    [e2[1] * e0[2] - e2[2] * e0[1], e2[2] * e0[0] - e2[0] * e0[2], e2[0] * e0[1] - e2[1] * e0[0]],
                    [e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]]])  # d det / dE
    EEt = E @ E.T
    tr = np.trace(EEt)
    f = np.r_[np.sum(e0 * cof[0]), (2 * EEt @ E - tr * E).reshape(-1)]
    D = N[:3].reshape(3, 3, 3)
    dG = 2 * (D @ E.T @ E + E @ D.transpose(0, 2, 1) @ E + EEt @ D) - 2 * np.sum(E * D, axis=(1, 2))[:, None, None] * E - tr * D
    J = np.c_[np.sum(cof * D, axis=(1, 2)), dG.reshape(3, 9)].T
    return f, J


def polish(N, p):
    """Three Gauss-Newton steps of (x, y, z) on the ten constraints (least squares by lstsq); E(p)."""
    p = p.astype(np.float64).copy()
    for _ in range(3):
        f, J = _constraints(N, p)
        d = np.linalg.lstsq(J, -f, rcond=None)[0]
        if not np.all(np.isfinite(d)):
            break
        p = p + d
    return (p[0] * N[0] + p[1] * N[1] + p[2] * N[2] + N[3]).reshape(3, 3)


def canonical(E: np.ndarray):
    """Unit Frobenius norm, largest-magnitude entry positive (the first in row-major order on ties)."""
    nrm = math.sqrt(float(np.sum(E * E)))
    if not (nrm > 0 and math.isfinite(nrm)):
        return None
    E = E / nrm
    i = int(np.argmax(np.abs(E.reshape(-1))))
    return -E if E.reshape(-1)[i] < 0 else E


def five_point(x1: np.ndarray, x2: np.ndarray, fragile: list | None = None) -> list[np.ndarray]:
    """EssentialMatrixFivePointEstimator::Estimate on n >= 5 normalised correspondences."""
    Q = np.c_[x2[:, :1] * x1[:, :1], x2[:, :1] * x1[:, 1:], x2[:, :1], x2[:, 1:] * x1[:, :1], x2[:, 1:] * x1[:, 1:], x2[:, 1:],
              x1[:, :1], x1[:, 1:], np.ones((len(x1), 1))]
    _, s, Vt = np.linalg.svd(Q, full_matrices=True)
    if len(s) < 5 or not s[4] > RANK_TOL * s[0]:
        if fragile is not None and len(s) >= 5 and s[4] > 1e-2 * RANK_TOL * s[0]:
            fragile.append(("rank", s[4] / s[0]))
        return []
    if fragile is not None and s[4] <= 1e2 * RANK_TOL * s[0]:
        fragile.append(("rank", s[4] / s[0]))
    return models_from_nullspace(Vt[5:9], fragile)


# ---- pose from E --------------------------------------------------------------------------------------------------
W_MAT = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def decompose(E: np.ndarray):
    """DecomposeEssentialMatrix: (R1, R2, t) with E = U diag(s) Vᵀ, det U = det V = +1 (the third column flipped where
    needed, which leaves E unchanged) and t = U[:, 2] with its largest-magnitude component positive.  Both are our choices:
    they fix the order of the four candidates, which only matters on a tie."""
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U[:, 2] = -U[:, 2]
    if np.linalg.det(Vt) < 0:
        Vt[2] = -Vt[2]
    t = U[:, 2]
    if t[int(np.argmax(np.abs(t)))] < 0:
        D = np.diag([-1.0, 1.0, -1.0])
        U, Vt = U @ D, D @ Vt
    return U @ W_MAT @ Vt, U @ W_MAT.T @ Vt, U[:, 2] / np.linalg.norm(U[:, 2])


def cheirality(R, t, x1, x2):
    """CheckCheirality: (count, number of uncertain points) of the two-view DLT points with both depths in (eps, 1000 |t|)."""
    m = len(x1)
    P2 = np.c_[R, t]
    A = np.zeros((m, 4, 4))
    A[:, 0] = x1[:, :1] * np.array([0, 0, 1, 0.0]) - np.array([1, 0, 0, 0.0])
    A[:, 1] = x1[:, 1:] * np.array([0, 0, 1, 0.0]) - np.array([0, 1, 0, 0.0])
    A[:, 2] = x2[:, :1] * P2[2] - P2[0]
    A[:, 3] = x2[:, 1:] * P2[2] - P2[1]
    Xh = np.linalg.svd(A)[2][:, 3, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        X = Xh[:, :3] / Xh[:, 3:]
    d1 = X[:, 2]
    d2 = X @ R[2] + t[2]
    hi = 1000.0 * np.linalg.norm(t)
    ok = (d1 > DBL_EPS) & (d1 < hi) & (d2 > DBL_EPS) & (d2 < hi)
    far = np.abs(Xh[:, 3]) <= 1e-9 * np.linalg.norm(Xh, axis=1)
    near = lambda d: (np.abs(d - hi) <= 1e-9 * hi) | (np.abs(d) <= 1e-12)  # noqa: E731
    unsure = far | near(d1) | near(d2)
    return int(np.sum(ok)), int(np.sum(unsure))


def pose_from_essential(E, x1, x2, fragile: list | None = None):
    """PoseFromEssentialMatrix: the candidate with the most points in front of both cameras, the later one on a tie."""
    R1, R2, t = decompose(E)
    cands = [(R1, t), (R2, t), (R1, -t), (R2, -t)]
    counts = [cheirality(R, tt, x1, x2) for R, tt in cands]
    best, best_n = 0, -1
    for i, (c, _) in enumerate(counts):
        if c >= best_n:
            best, best_n = i, c
    if fragile is not None:
        for i, (c, u) in enumerate(counts):
            if i != best and best_n - c <= u + counts[best][1]:
                fragile.append(("cheirality", i, c, best_n))
    R, tt = cands[best]
    return np.c_[R, tt], best_n, [c for c, _ in counts]


# ---- LORANSAC -----------------------------------------------------------------------------------------------------
# pycolmap 3.11 RANSACOptions() as recalled
DEFAULT_OPTIONS = dict(max_error=4.0, min_inlier_ratio=0.01, confidence=0.9999, dyn_num_trials_multiplier=3.0, min_num_trials=1000,
                       max_num_trials=100000, seed=0)


def normalise(points, intr):
    fx, fy, cx, cy = (float(v) for v in intr)
    p = np.asarray(points, np.float64).reshape(-1, 2)
    return np.c_[(p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy]


def estimate(points1, points2, intr1, intr2, **opts) -> dict:
    """essential_matrix_estimation on PINHOLE intr = (fx, fy, cx, cy).  Returns dict(success, E [3,3] or None,
    cam2_from_cam1 [3,4] or None, num_inliers, inlier_mask, num_trials, max_num_trials, lo_rounds, cheirality_counts,
    fragile)."""
    o = dict(DEFAULT_OPTIONS)
    o.update(opts)
    x1, x2 = normalise(points1, intr1), normalise(points2, intr2)
    n = len(x1)
    f1, f2 = (intr1[0] + intr1[1]) / 2.0, (intr2[0] + intr2[1]) / 2.0
    thr = 0.5 * (o["max_error"] / f1 + o["max_error"] / f2)
    thr2 = thr * thr
    fragile: list = []
    out = dict(success=False, E=None, cam2_from_cam1=None, num_inliers=0, inlier_mask=np.zeros(n, bool), num_trials=0, lo_rounds=0,
               max_num_trials=0, fragile=fragile)
    if n < SAMPLE_SIZE:
        return out
    max_trials = min(o["max_num_trials"], num_trials(int(o["min_inlier_ratio"] * 100000), 100000, o["confidence"],
                                                     o["dyn_num_trials_multiplier"]))
    out["max_num_trials"] = max_trials
    seed = int(o["seed"]) & MASK64

    X1, X2 = np.c_[x1, np.ones(n)], np.c_[x2, np.ones(n)]

    def sampson_all(models):  # the squared Sampson errors of several models at once [k, n]
        Es = np.asarray(models)
        Ex1 = np.einsum("kij,nj->kni", Es, X1)
        Etx2 = np.einsum("kji,nj->kni", Es, X2)
        num = np.einsum("kni,ni->kn", Ex1, X2) ** 2
        den = Ex1[..., 0] ** 2 + Ex1[..., 1] ** 2 + Etx2[..., 0] ** 2 + Etx2[..., 1] ** 2
        with np.errstate(divide="ignore", invalid="ignore"):
            return num / den

    def scored(E, best, res=None):
        res = sampson(E, x1, x2) if res is None else res
        sup = _support(res, thr2)
        near = int(np.sum(np.abs(res - thr2) <= 1e-7 * thr2))
        better = _better(sup, best)
        if near and (better or abs(sup[0] - best[0]) <= near):
            fragile.append(("threshold", near, sup[0], best[0]))
        if sup[0] == best[0] and sup[0] > 0 and abs(sup[1] - best[1]) <= 1e-9 * max(abs(sup[1]), abs(best[1]), 1e-300):
            fragile.append(("tie", sup, best))
        return res, sup, better

    best, best_model = (0, DBL_MAX), None
    dyn = max_trials
    abort = False
    trials = lo_rounds = 0
    while trials < max_trials:
        if abort:
            trials += 1
            break
        idx = sample(seed, trials, n)
        models = five_point(x1[idx], x2[idx], fragile)
        all_res = sampson_all(models) if models else None
        for mi, model in enumerate(models):
            res, sup, better = scored(model, best, all_res[mi])
            if better:
                best, best_model = sup, model
                if sup[0] > SAMPLE_SIZE and sup[0] >= SAMPLE_SIZE:
                    for _ in range(10):
                        inl = res <= thr2
                        prev = best[0]
                        lo_rounds += 1
                        for lm in five_point(x1[inl], x2[inl], fragile):
                            lres, lsup, lbetter = scored(lm, best)
                            if lbetter:
                                best, best_model, res = lsup, lm, lres
                        if best[0] <= prev:
                            break
                dyn = num_trials(best[0], n, o["confidence"], o["dyn_num_trials_multiplier"])
            if trials >= dyn and trials >= o["min_num_trials"]:
                abort = True
                break
        trials += 1
    out.update(num_trials=trials, lo_rounds=lo_rounds)
    if best[0] < SAMPLE_SIZE:
        return out
    mask = sampson(best_model, x1, x2) <= thr2
    P, npts, counts = pose_from_essential(best_model, x1[mask], x2[mask], fragile)
    out.update(success=True, E=best_model, cam2_from_cam1=P, num_inliers=best[0], inlier_mask=mask, num_cheirality_points=npts,
               cheirality_counts=counts)
    return out


# ---- synthetic two-view problems ------------------------------------------------------------------------------------
INTR1 = (820.0, 790.0, 640.0, 480.0)
INTR2 = (700.0, 710.0, 600.0, 500.0)


def _rot(axis, ang):
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def synthetic_problem(n: int, outlier_ratio: float, seed: int, noise_px: float = 0.0, planar: bool = False, forward: bool = False,
                      max_error: float = 4.0):
    """n matches between two PINHOLE cameras (INTR1, INTR2): (points1, points2, intr1, intr2, R, t, designed inlier mask) with
    cam2_from_cam1 = [R | t], |t| = 1.  Points lie in front of both cameras (on a plane when `planar`); `forward` moves the
    camera along its axis.  Outliers move points2 to a random pixel more than 10 max_error from its epipolar line."""
    rng = np.random.default_rng(seed)
    W2, H2 = 2 * INTR2[2], 2 * INTR2[3]
    R = _rot(rng.normal(size=3), rng.uniform(0.05, 0.3))
    t = np.array([0.0, 0.0, 1.0]) + 0.05 * rng.normal(size=3) if forward else rng.normal(size=3)
    t = t / np.linalg.norm(t)
    if planar:
        nrm = np.array([0.0, 0.0, 1.0]) + 0.3 * rng.normal(size=3)
        nrm /= np.linalg.norm(nrm)
    X = np.zeros((0, 3))
    while len(X) < n:
        m = 2 * (n - len(X)) + 16
        px = np.c_[rng.uniform(0, 2 * INTR1[2], m), rng.uniform(0, 2 * INTR1[3], m)]
        ray = np.c_[(px[:, 0] - INTR1[2]) / INTR1[0], (px[:, 1] - INTR1[3]) / INTR1[1], np.ones(m)]
        d = (8.0 / (ray @ nrm)) if planar else rng.uniform(4.0, 16.0, m)
        P = ray * d[:, None]
        P2 = P @ R.T + t
        u = INTR2[0] * P2[:, 0] / P2[:, 2] + INTR2[2]
        v = INTR2[1] * P2[:, 1] / P2[:, 2] + INTR2[3]
        ok = (d > 1.0) & (d < 40.0) & (P2[:, 2] > 1.0) & (u >= 0) & (u < W2) & (v >= 0) & (v < H2)
        X = np.r_[X, P[ok]][:n]
    X2 = X @ R.T + t
    p1 = np.c_[INTR1[0] * X[:, 0] / X[:, 2] + INTR1[2], INTR1[1] * X[:, 1] / X[:, 2] + INTR1[3]]
    p2 = np.c_[INTR2[0] * X2[:, 0] / X2[:, 2] + INTR2[2], INTR2[1] * X2[:, 1] / X2[:, 2] + INTR2[3]]
    p1 = p1 + rng.normal(size=p1.shape) * noise_px
    p2 = p2 + rng.normal(size=p2.shape) * noise_px
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    K1 = np.array([[INTR1[0], 0, INTR1[2]], [0, INTR1[1], INTR1[3]], [0, 0, 1]])
    K2 = np.array([[INTR2[0], 0, INTR2[2]], [0, INTR2[1], INTR2[3]], [0, 0, 1]])
    F = np.linalg.inv(K2).T @ tx @ R @ np.linalg.inv(K1)
    inl = np.ones(n, bool)
    for i in rng.choice(n, int(round(outlier_ratio * n)), replace=False):
        line = F @ np.r_[p1[i], 1.0]
        while True:
            q = np.array([rng.uniform(0, W2), rng.uniform(0, H2)])
            if abs(line @ np.r_[q, 1.0]) > 10 * max_error * np.hypot(line[0], line[1]):
                break
        p2[i] = q
        inl[i] = False
    return p1, p2, np.array(INTR1), np.array(INTR2), R, t, inl
