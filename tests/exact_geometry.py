"""Exact reference for the stateless track entry points and the consumers of csrc/tri_math.h — TEST INFRASTRUCTURE.

    mpsfm_triangulate_tracks   xyz[t] = dehomogenised smallest eigenvector of A = sum (P - x x^T P)^T (P - x x^T P)
    mpsfm_filter_tracks        max pairwise triangulation angle, squared reprojection error, cheirality
    mpsfm_point_covs           cov[j] = (sum magnitude * Jp^T Jp)^-1
    mpsfm_tri_estimate_batch   EstimateTriangulation per candidate: exact_loransac walks the loop of tri_ransac_scratch
    mpsfm_init_pair_candidates the two-view candidate (the same walk), the reference's angle, depth flags and the lift

Everything in the first half of this module is plain mpmath at 60 digits, written from the definitions in
include/mpsfm_hip.h and COLMAP's published formulas (TriangulateMultiViewPoint, CalculateTriangulationAngle,
CalculateSquaredReprojectionError, HasPointPositiveDepth): `mp.eigsy` and a plain matrix inverse, no Jacobi, no
Cholesky, no NumPy arithmetic.  The fp64 arrays of a `Tracks` / `BAProblem` are taken as exact numbers.

Conventions: quaternions are (x, y, z, w); R(q) is the usual quadratic form of q (no normalisation, as Eigen's
toRotationMatrix); cam_from_world is Xc = R X + t; the projection centre is C = -R^T t; intrinsics are fx fy cx cy.

The second half holds what the CPU and the GPU tests share: the comparison functions (one per criterion, each returns
the ratio "error / (eps * form)" so that a constant can be measured as well as asserted), the independent fp64 NumPy
evaluation the constants are measured with, and the deterministic case sets.
"""

from __future__ import annotations

import functools
import math

import mpmath as mp
import numpy as np

from mpsfm_amd.problem import BAProblem, Tracks
from mpsfm_amd.sfm.scene.priorutils import bilinear_at_kps

DPS = 60
EPS = 2.0 ** -52
mpf = mp.mpf


def _hp(fn):
    @functools.wraps(fn)
    def wrapped(*a, **kw):
        with mp.workdps(DPS):
            return fn(*a, **kw)

    return wrapped


# ============================================================================================================
# the exact reference
# ============================================================================================================
def _vec(a):
    return [mpf(float(v)) for v in a]


def rotation(q):
    """R(q) for q = (x, y, z, w) as a 3x3 list of mpf."""
    x, y, z, w = _vec(q)
    return [
        [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
        [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
        [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)],
    ]


def centre(R, t):
    return [-(R[0][k] * t[0] + R[1][k] * t[1] + R[2][k] * t[2]) for k in range(3)]


def to_camera(R, t, X):
    return [R[i][0] * X[0] + R[i][1] * X[1] + R[i][2] * X[2] + t[i] for i in range(3)]


def _norm(v):
    return mp.sqrt(sum(a * a for a in v))


def _fro(A):
    return mp.sqrt(sum(A[i, j] ** 2 for i in range(A.rows) for j in range(A.cols)))


class _Cams:
    """mpf views of the camera arrays, made on first use."""

    def __init__(self, quat, t, intr, intr_idx):
        self.quat, self.t, self.intr, self.intr_idx = quat, t, intr, intr_idx
        self._c = {}

    def __call__(self, c):
        c = int(c)
        if c not in self._c:
            R = rotation(self.quat[c])
            t = _vec(self.t[c])
            self._c[c] = (R, t, centre(R, t), _vec(self.intr[int(self.intr_idx[c])]))
        return self._c[c]


def _cams_of(tr):
    if getattr(tr, "_exact_cams", None) is None:
        tr._exact_cams = _Cams(tr.cam_quat, tr.cam_t, tr.cam_intr, tr.cam_intr_idx)
    return tr._exact_cams


def _elements(tr: Tracks, k: int):
    return range(int(tr.track_start[k]), int(tr.track_start[k + 1]))


@_hp
def triangulation_matrix(tr: Tracks, k: int):
    """The exact 4x4 A = sum_i (P_i - x_i x_i^T P_i)^T (P_i - x_i x_i^T P_i) of track k; x_i the unit viewing ray."""
    cams = _cams_of(tr)
    A = mp.zeros(4)
    for e in _elements(tr, k):
        R, t, _, K = cams(tr.el_cam[e])
        u, v = _vec(tr.el_xy[e])
        x = [(u - K[2]) / K[0], (v - K[3]) / K[1], mpf(1)]
        n = _norm(x)
        x = [a / n for a in x]
        P = mp.matrix([[R[i][0], R[i][1], R[i][2], t[i]] for i in range(3)])
        xm = mp.matrix(x)
        M = P - xm * (xm.T * P)
        A += M.T * M
    return A


@_hp
def eig(A):
    """Eigenvalues ascending and the matching unit eigenvectors (list of 4-lists) of a symmetric matrix."""
    E, Q = mp.eigsy(A)
    order = sorted(range(A.rows), key=lambda i: E[i])
    return [E[i] for i in order], [[Q[r, i] for r in range(A.rows)] for i in order]


@_hp
def angle_pair(C1, C2, X):
    """(angle folded to [0, pi/2], kappa) of one camera pair; see the docstring of tests/test_gpu_exact_geometry.py for
    kappa.  The angle is 0 where a ray has zero length."""
    d1 = [X[k] - C1[k] for k in range(3)]
    d2 = [X[k] - C2[k] for k in range(3)]
    b = [C1[k] - C2[k] for k in range(3)]
    n1, n2, nb = _norm(d1), _norm(d2), _norm(b)
    if n1 == 0 or n2 == 0:
        return mpf(0), mpf(1)
    dot = sum(d1[k] * d2[k] for k in range(3))
    cross = [d1[1] * d2[2] - d1[2] * d2[1], d1[2] * d2[0] - d1[0] * d2[2], d1[0] * d2[1] - d1[1] * d2[0]]
    ang = mp.atan2(_norm(cross), dot)  # exact 0 and pi for parallel rays, unlike acos of a rounded cosine
    cs = dot / (n1 * n2)
    r1, r2, b2 = n1 * n1, n2 * n2, nb * nb
    den = 2 * n1 * n2
    g1 = (_norm(X) + _norm(C1)) / n1
    g2 = (_norm(X) + _norm(C2)) / n2
    gb = (_norm(C1) + _norm(C2)) / nb if nb != 0 else mpf(0)
    dcs = (2 * g1 * r1 + 2 * g2 * r2 + 2 * gb * b2 + r1 + r2 + b2) / den + abs(cs) * (g1 + g2 + 2)
    kappa = dcs / max(mp.sin(ang), mp.sqrt(mpf(EPS)))
    return min(ang, mp.pi - ang), kappa


@_hp
def filter_numbers(tr: Tracks, k: int, X):
    """Exact numbers of track k at the fp64 point X: dict(angle, pairs [(angle, kappa)], zc [n], err [n],
    err_scale [n], front [n]).  err is None where zc == 0."""
    cams = _cams_of(tr)
    X = _vec(X)
    els = list(_elements(tr, k))
    zc, err, scale, front, cen = [], [], [], [], []
    for e in els:
        R, t, C, K = cams(tr.el_cam[e])
        cen.append(C)
        xc, yc, z = to_camera(R, t, X)
        zc.append(z)
        front.append(z >= mpf(EPS))
        if z == 0:
            err.append(None)
            scale.append(None)
            continue
        u, v = _vec(tr.el_xy[e])
        du, dv = K[0] * xc / z + K[2] - u, K[1] * yc / z + K[3] - v
        err.append(du * du + dv * dv)
        mag = [sum(abs(R[i][j] * X[j]) for j in range(3)) + abs(t[i]) for i in range(3)]  # the terms that cancel in R X + t
        mu = K[0] / abs(z) * (mag[0] + abs(xc / z) * mag[2]) + abs(K[2]) + abs(u)
        mv = K[1] / abs(z) * (mag[1] + abs(yc / z) * mag[2]) + abs(K[3]) + abs(v)
        scale.append(mu * mu + mv * mv)
    pairs = [angle_pair(cen[i], cen[j], X) for i in range(len(els)) for j in range(i + 1, len(els))]
    return dict(angle=max([p[0] for p in pairs], default=mpf(0)), pairs=pairs, zc=zc, err=err, err_scale=scale, front=front)


@_hp
def point_hessians(prob: BAProblem):
    """Per point: dict(n_obs, H, inv, cond).  H = sum magnitude * Jp^T Jp (3x3), inv its plain inverse and cond its 2-norm
    condition number; inv is None and cond is inf where H has no inverse worth the name (fewer than two observations)."""
    cams = _Cams(prob.cam_quat, prob.cam_t, prob.cam_intr, prob.cam_intr_idx)
    mag = mpf(float(prob.reproj_loss_magnitude))
    H = [mp.zeros(3) for _ in range(prob.n_pts)]
    n = [0] * prob.n_pts
    block = {}  # J^T J of a (camera, point) pair: repeated observations of one pair share it
    for c, p in zip(prob.obs_cam.tolist(), prob.obs_pt.tolist()):
        if (c, p) not in block:
            R, t, _, K = cams(c)
            xc, yc, z = to_camera(R, t, _vec(prob.pts[p]))
            J = mp.matrix(2, 3)
            for j in range(3):
                J[0, j] = K[0] * (R[0][j] * z - xc * R[2][j]) / (z * z)
                J[1, j] = K[1] * (R[1][j] * z - yc * R[2][j]) / (z * z)
            block[c, p] = mag * (J.T * J)
        H[p] += block[c, p]
        n[p] += 1
    out = []
    for p in range(prob.n_pts):
        if n[p] < 2:
            out.append(dict(n_obs=n[p], H=H[p], inv=None, cond=mp.inf))
            continue
        lam, _ = eig(H[p])
        if lam[0] <= lam[2] * mpf(10) ** -40:
            out.append(dict(n_obs=n[p], H=H[p], inv=None, cond=mp.inf))
        else:
            out.append(dict(n_obs=n[p], H=H[p], inv=H[p] ** -1, cond=lam[2] / lam[0]))
    return out


# ============================================================================================================
# deterministic scene builder
# ============================================================================================================
def _quat_R_float(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([
        [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
        [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
        [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)],
    ])


def quat_mul(p, q):
    px, py, pz, pw = p
    qx, qy, qz, qw = q
    return (pw * qx + px * qw + py * qz - pz * qy, pw * qy - px * qz + py * qw + pz * qx,
            pw * qz + px * qy - py * qx + pz * qw, pw * qw - px * qx - py * qy - pz * qz)


def axis_quat(axis, deg):
    a = math.radians(deg) / 2
    s = math.sin(a) / math.sqrt(sum(v * v for v in axis))
    return (axis[0] * s, axis[1] * s, axis[2] * s, math.cos(a))


class SceneBuilder:
    """Cameras given as quaternion and centre, points, tracks.  The quaternion is normalised and t = -R C is formed in
    mpmath from the rounded quaternion; projections are made in mpmath from the rounded q, t, K and rounded to fp64;
    pixel noise (a fixed stream per builder) is added afterwards on request."""

    def __init__(self, intr, seed=0):
        self.intr = np.asarray(intr, np.float64).reshape(-1, 4)
        self.quat, self.t, self.intr_idx = [], [], []
        self.start, self.el_cam, self.el_xy, self.labels, self.truth = [0], [], [], [], []
        self.rng = np.random.default_rng(seed)

    @_hp
    def add_camera(self, quat, centre_, intr_idx=0) -> int:
        q = _vec(quat)
        n = _norm(q)
        q = [float(a / n) for a in q]
        R = rotation(q)
        C = _vec(centre_)
        self.quat.append(q)
        self.t.append([float(-(R[i][0] * C[0] + R[i][1] * C[1] + R[i][2] * C[2])) for i in range(3)])
        self.intr_idx.append(int(intr_idx))
        return len(self.quat) - 1

    def add_camera_seeing(self, quat, target, cam_xyz, intr_idx=0) -> int:
        """A camera with rotation `quat` placed so that `target` has the camera coordinates `cam_xyz`."""
        q = np.asarray(quat, np.float64)
        R = _quat_R_float(q / np.linalg.norm(q))
        return self.add_camera(quat, np.asarray(target, np.float64) - R.T @ np.asarray(cam_xyz, np.float64), intr_idx)

    @_hp
    def project(self, cam, X):
        R, t, K = rotation(self.quat[cam]), _vec(self.t[cam]), _vec(self.intr[self.intr_idx[cam]])
        xc, yc, z = to_camera(R, t, _vec(X))
        return [float(K[0] * xc / z + K[2]), float(K[1] * yc / z + K[3])]

    def add_track(self, label, X, cams, noise_px=0.0, xy=None) -> int:
        """One track of the point X over `cams`; `xy` overrides the projections.  Returns the track index."""
        for i, c in enumerate(cams):
            p = list(xy[i]) if xy is not None else self.project(c, X)
            if noise_px:
                p = [p[0] + noise_px * float(self.rng.standard_normal()), p[1] + noise_px * float(self.rng.standard_normal())]
            self.el_cam.append(int(c))
            self.el_xy.append(p)
        self.start.append(len(self.el_cam))
        self.labels.append(label)
        self.truth.append(None if X is None else [float(v) for v in X])
        return len(self.labels) - 1

    def tracks(self, n_tracks=None) -> Tracks:
        n = len(self.labels) if n_tracks is None else n_tracks
        ne = self.start[n]
        tr = Tracks(np.array(self.quat).reshape(-1, 4), np.array(self.t).reshape(-1, 3), self.intr, np.array(self.intr_idx, np.int32),
                    np.array(self.start[: n + 1], np.int64), np.array(self.el_cam[:ne], np.int32),
                    np.array(self.el_xy[:ne], np.float64).reshape(-1, 2))
        tr.labels = self.labels[:n]
        return tr


# ============================================================================================================
# comparison functions: every one returns ratios, error / (eps * form of the criterion)
# ============================================================================================================
@_hp
def triangulation_reference(tr: Tracks):
    """Per track: dict(A, fro, lam, X, gap, fwd_unit) — fwd_unit is the forward bound per unit of C_t * eps."""
    out = []
    for k in range(tr.n_tracks):
        if tr.track_start[k + 1] - tr.track_start[k] < 2:
            out.append(None)
            continue
        A = triangulation_matrix(tr, k)
        lam, vec = eig(A)
        v = vec[0]
        fro = _fro(A)
        X = [v[i] / v[3] for i in range(3)] if v[3] != 0 else None
        gap = lam[1] - lam[0]
        unit = None
        if X is not None and gap > 0:
            nx = _norm(X)
            unit = fro / gap * (1 + nx) * mp.sqrt(1 + nx * nx)
        out.append(dict(A=A, fro=fro, lam=lam, X=X, gap=gap, fwd_unit=unit))
    return out


@_hp
def triangulation_informative(ref, C_t):
    """The forward bound of a track is worth asserting: C_t * eps * fwd_unit <= 1e-6 * (1 + |X_ref|)."""
    if ref is None or ref["fwd_unit"] is None:
        return False
    return C_t * mpf(EPS) * ref["fwd_unit"] <= mpf(10) ** -6 * (1 + _norm(ref["X"]))


@_hp
def triangulation_ratios(ref, xyz):
    """Per track (backward, forward) ratios of the output xyz [T,3]: backward = max(|A v - (v'Av) v|, v'Av - lambda_min)
    / (eps |A|_F) with v = (X, 1) / |(X, 1)|; forward = |X - X_ref| / (eps * fwd_unit).  A track of fewer than two
    elements gives (0, None) for an all-NaN output and (inf, None) otherwise; a non-finite output of a longer track
    gives (None, None): nothing to assert."""
    res = []
    for k, r in enumerate(ref):
        x = [float(a) for a in xyz[k]]
        if r is None:
            res.append((0.0 if all(math.isnan(a) for a in x) else math.inf, None))
            continue
        if not all(math.isfinite(a) for a in x):
            res.append((None, None))
            continue
        v = _vec(x) + [mpf(1)]
        n = _norm(v)
        v = mp.matrix([a / n for a in v])
        Av = r["A"] * v
        ray = (v.T * Av)[0]
        back = max(_norm([Av[i] - ray * v[i] for i in range(4)]), ray - r["lam"][0]) / (mpf(EPS) * r["fro"])
        fwd = None
        if r["fwd_unit"] is not None:
            fwd = float(_norm([mpf(x[i]) - r["X"][i] for i in range(3)]) / (mpf(EPS) * r["fwd_unit"]))
        res.append((float(back), fwd))
    return res


@_hp
def filter_reference(tr: Tracks, xyz):
    return [filter_numbers(tr, k, xyz[k]) for k in range(tr.n_tracks)]


@_hp
def angle_ratio(ref, ang):
    """Smallest C_a with which the kernel's maximum `ang` fits the per-pair criterion |a_i - ref_i| <= C_a eps kappa_i:
    a maximum of such a_i lies in [max_i (ref_i - C eps kappa_i), max_i (ref_i + C eps kappa_i)].  A track without a
    pair, and pairs with a zero-length ray, must give exactly 0."""
    ang = mpf(float(ang))
    if not ref["pairs"]:
        return 0.0 if ang == 0 else math.inf
    if ref["angle"] == 0 and all(k == 1 for _, k in ref["pairs"]):  # every pair has a zero-length ray
        return 0.0 if ang == 0 else math.inf
    lo = max((a - ang) / (mpf(EPS) * k) for a, k in ref["pairs"])
    hi = min((ang - a) / (mpf(EPS) * k) for a, k in ref["pairs"])
    return float(max(lo, hi, 0))


@_hp
def sq_err_ratios(ref, err):
    """Per element |e - e_ref| / (eps (e_ref + s)); for zc == 0 the output must be inf or NaN (ratio 0, else inf)."""
    out = []
    for e_ref, s, e in zip(ref["err"], ref["err_scale"], err):
        e = float(e)
        if e_ref is None:
            out.append(0.0 if not math.isfinite(e) else math.inf)
        elif not math.isfinite(e):
            out.append(math.inf)
        else:
            out.append(float(abs(mpf(e) - e_ref) / (mpf(EPS) * (e_ref + s))))
    return out


@_hp
def cov_ratios(ref, covs):
    """Per point the smallest C_p that accepts the output: |cov - ref|_F / (eps cond |ref|_F), or 1 / (eps cond) for a NaN
    output (accepted only where C_p eps cond >= 1).  Fewer than two observations: 0 for all-NaN, inf otherwise."""
    out = []
    for r, c in zip(ref, covs):
        c = np.asarray(c, np.float64)
        if r["n_obs"] < 2:
            out.append(0.0 if np.isnan(c).all() else math.inf)
        elif r["inv"] is None:
            out.append(0.0)
        elif not np.isfinite(c).all():
            out.append(float(1 / (mpf(EPS) * r["cond"])))
        else:
            d = mp.sqrt(sum((mpf(float(c[i, j])) - r["inv"][i, j]) ** 2 for i in range(3) for j in range(3)))
            out.append(float(d / (mpf(EPS) * r["cond"] * _fro(r["inv"]))))
    return out


# ============================================================================================================
# the independent fp64 evaluation the constants are measured with (NumPy, eigh / inv; not the C oracle's Jacobi)
# ============================================================================================================
def numpy_triangulate(tr: Tracks) -> np.ndarray:
    out = np.full((tr.n_tracks, 3), np.nan)
    for k in range(tr.n_tracks):
        e0, e1 = int(tr.track_start[k]), int(tr.track_start[k + 1])
        if e1 - e0 < 2:
            continue
        A = np.zeros((4, 4))
        for e in range(e0, e1):
            c = tr.el_cam[e]
            K = tr.cam_intr[tr.cam_intr_idx[c]]
            P = np.concatenate([_quat_R_float(tr.cam_quat[c]), tr.cam_t[c][:, None]], 1)
            x = np.array([(tr.el_xy[e, 0] - K[2]) / K[0], (tr.el_xy[e, 1] - K[3]) / K[1], 1.0])
            x /= np.linalg.norm(x)
            M = P - np.outer(x, x @ P)
            A += M.T @ M
        _, Q = np.linalg.eigh(A)
        with np.errstate(all="ignore"):
            out[k] = Q[:3, 0] / Q[3, 0]
    return out


def numpy_filter(tr: Tracks, xyz):
    ang, err, front = np.zeros(tr.n_tracks), np.zeros(tr.n_el), np.zeros(tr.n_el, bool)
    R = np.stack([_quat_R_float(q) for q in tr.cam_quat])
    C = -np.einsum("nji,nj->ni", R, tr.cam_t)
    with np.errstate(all="ignore"):
        for k in range(tr.n_tracks):
            X = np.asarray(xyz[k], np.float64)
            e0, e1 = int(tr.track_start[k]), int(tr.track_start[k + 1])
            for e in range(e0, e1):
                c = tr.el_cam[e]
                K = tr.cam_intr[tr.cam_intr_idx[c]]
                Xc = R[c] @ X + tr.cam_t[c]
                front[e] = Xc[2] >= EPS
                d = K[:2] * Xc[:2] / Xc[2] + K[2:] - tr.el_xy[e]
                err[e] = d @ d
                for f in range(e + 1, e1):
                    c2 = tr.el_cam[f]
                    b2, r1, r2 = np.sum((C[c] - C[c2]) ** 2), np.sum((X - C[c]) ** 2), np.sum((X - C[c2]) ** 2)
                    den = 2 * np.sqrt(r1 * r2)
                    if den == 0:
                        continue
                    a = np.arccos(np.clip((r1 + r2 - b2) / den, -1.0, 1.0))
                    ang[k] = max(ang[k], min(a, np.pi - a))
    return ang, err, front


def numpy_point_covs(prob: BAProblem) -> np.ndarray:
    H = np.zeros((prob.n_pts, 3, 3))
    n = np.bincount(prob.obs_pt, minlength=prob.n_pts)
    for c, p in zip(prob.obs_cam, prob.obs_pt):
        R, K = _quat_R_float(prob.cam_quat[c]), prob.cam_intr[prob.cam_intr_idx[c]]
        Xc = R @ prob.pts[p] + prob.cam_t[c]
        J = np.array([[K[0] / Xc[2], 0, -K[0] * Xc[0] / Xc[2] ** 2], [0, K[1] / Xc[2], -K[1] * Xc[1] / Xc[2] ** 2]]) @ R
        H[p] += prob.reproj_loss_magnitude * (J.T @ J)
    out = np.full((prob.n_pts, 3, 3), np.nan)
    for p in range(prob.n_pts):
        if n[p] >= 2:
            try:
                out[p] = np.linalg.inv(H[p])
            except np.linalg.LinAlgError:
                pass
    return out


# ============================================================================================================
# case sets
# ============================================================================================================
INTR = [[1000.0, 1010.0, 640.0, 480.0], [700.0, 650.0, 500.0, 380.0]]  # two rows that differ in all four numbers
N_RIG = 200
BLOCK_EDGES = (1, 127, 128, 129, 257)  # n_tracks around the 128 threads of a triangulation / filter block


def _rig(b: SceneBuilder, n, shift=(0.0, 0.0, 0.0), scale=1.0):
    """n friendly cameras: on an arc of +-60 degrees around `shift`, 10 `scale` away, looking at it with a small roll and
    tilt; intrinsics rows alternate in a pattern that is not the identity."""
    cams = []
    for i in range(n):
        yaw = -60.0 + 120.0 * ((i * 37) % n) / max(n - 1, 1)
        q = quat_mul(axis_quat((0, 0, 1), 3.0 * ((i % 5) - 2)), quat_mul(axis_quat((1, 0, 0), 4.0 * ((i % 3) - 1)), axis_quat((0, 1, 0), yaw)))
        cam_xyz = np.array([0.3 * ((i % 4) - 1.5), 0.2 * ((i % 3) - 1), 10.0 + 0.5 * (i % 7)]) * scale
        cams.append(b.add_camera_seeing(q, shift, cam_xyz, intr_idx=1 if i % 3 == 0 else 0))
    return cams


def _friendly_points(rng, n, shift=(0.0, 0.0, 0.0), scale=1.0):
    return np.asarray(shift) + scale * rng.uniform(-1.0, 1.0, (n, 3))


@functools.lru_cache(maxsize=None)
def triangulation_cases():
    """(builder, groups): groups maps a group name to its track indices; `forward` lists the groups whose every track
    must be informative (the forward bound is asserted there)."""
    b = SceneBuilder(INTR, seed=11)
    rng = np.random.default_rng(5)
    rig = _rig(b, N_RIG)
    g = {}

    def group(name, idx):
        g.setdefault(name, []).extend(idx)

    # friendly tracks first: prefixes of this list are the block-edge launches (n_tracks 1, 127, 128, 129, 257)
    pts = _friendly_points(rng, BLOCK_EDGES[-1])
    for i, X in enumerate(pts):
        nv = (2, 3, 5)[i % 3]
        cams = [rig[(7 * i + 13 * j) % N_RIG] for j in range(nv)]
        group("friendly", [b.add_track(f"friendly{nv}", X, cams, noise_px=0.5 if i % 2 else 0.0)])
    for nv in (64, 200):
        group("friendly", [b.add_track(f"views{nv}", pts[nv % 7], rig[:nv], noise_px=0.5)])
        group("friendly", [b.add_track(f"views{nv}_exact", pts[nv % 5], rig[:nv])])
    group("friendly", [b.add_track("shuffled_cams", pts[3], [rig[17], rig[3], rig[11], rig[5], rig[8]], noise_px=0.5)])
    # low parallax: two cameras `base` apart, the point 2 away
    for ratio in (1e-2, 1e-3, 1e-4):
        c0 = b.add_camera((0, 0, 0, 1), (-ratio, 0, 0), 0)
        c1 = b.add_camera(axis_quat((0, 1, 0), 0.5), (ratio, 0, 0), 1)
        name = f"parallax{ratio:g}"
        group(name, [b.add_track(name, (0.03, -0.02, 2.0), [c0, c1])])
        if ratio == 1e-2:
            group(name, [b.add_track(name + "_noise", (0.03, -0.02, 2.0), [c0, c1], noise_px=0.5)])
        if ratio == 1e-2:  # depth 1e6 baselines: v[3] tiny
            group("far_point", [b.add_track("far_point", (1e3, -2e3, 2e4), [c0, c1])])
    # the whole scene translated and scaled
    for name, shift, scale in (("shift1e3", (1e3, -1e3, 1e3), 1.0), ("shift1e4", (1e4, 1e4, -1e4), 1.0),
                               ("scale1e-3", (0, 0, 0), 1e-3), ("scale1e3", (0, 0, 0), 1e3)):
        cams = _rig(b, 6, shift, scale)
        for i, X in enumerate(_friendly_points(rng, 4, shift, scale)):
            group(name, [b.add_track(name, X, cams[: (2, 3, 5, 6)[i]], noise_px=0.5 if i % 2 else 0.0)])
    # large rotations: 180 degrees about each axis (w = 0), a negative w, a 90 degree roll
    target = (0.2, -0.1, 0.3)
    big = [b.add_camera_seeing((1, 0, 0, 0), target, (3.0, 1.0, 9.0), 0), b.add_camera_seeing((0, 1, 0, 0), target, (-2.0, 2.5, 11.0), 1),
           b.add_camera_seeing((0, 0, 1, 0), target, (1.0, -3.0, 10.0), 0),
           b.add_camera_seeing(tuple(-v for v in axis_quat((0.2, 1, 0.1), 50.0)), target, (0.5, 0.5, 12.0), 1),
           b.add_camera_seeing(axis_quat((0, 0, 1), 90.0), target, (-1.0, 2.0, 8.0), 0)]
    X = (0.5, 0.1, -0.2)
    group("rotations", [b.add_track("rot_all", X, big, noise_px=0.5), b.add_track("rot_xy", X, big[:2]), b.add_track("rot_yz", X, big[1:3]),
                        b.add_track("rot_xz", X, [big[0], big[2]]), b.add_track("rot_negw_roll", X, big[3:], noise_px=0.5),
                        b.add_track("rot_x_roll_rig", X, [big[0], big[4], rig[0]])])
    # rank-deficient or unusual but legal tracks: backward criterion only
    p0, p1 = b.project(rig[0], pts[0]), b.project(rig[1], pts[0])
    group("same_cam_twice", [b.add_track("same_cam_two_pixels", None, [rig[0], rig[0]], xy=[p0, [p0[0] + 40.0, p0[1] - 25.0]]),
                             b.add_track("same_cam_twice_plus_one", None, [rig[0], rig[0], rig[1]], xy=[p0, [p0[0] + 0.7, p0[1] - 0.4], p1])])
    group("rank_deficient", [b.add_track("same_cam_same_pixel", None, [rig[0], rig[0]], xy=[p0, p0])])
    centre0 = np.asarray(rig_centre(b, rig[0]))
    twin = b.add_camera(axis_quat((0.1, 1, 0), -20.0), centre0, 1)
    group("rank_deficient", [b.add_track("pure_rotation", pts[0], [rig[0], twin])])
    group("pure_rotation_noise", [b.add_track("pure_rotation_noise", pts[0], [rig[0], twin], noise_px=0.5)])
    # fewer than two elements: NaN by contract
    group("short", [b.add_track("empty", None, []), b.add_track("one_view", pts[1], [rig[2]])])
    return b, g


TRI_FORWARD_GROUPS = ("friendly", "rotations", "parallax0.01")  # every track of these must be informative


def rig_centre(b: SceneBuilder, cam):
    with mp.workdps(DPS):
        return [float(v) for v in centre(rotation(b.quat[cam]), _vec(b.t[cam]))]


def _ident_cam(b, C, intr_idx=0):
    return b.add_camera((0, 0, 0, 1), C, intr_idx)


@functools.lru_cache(maxsize=None)
def filter_cases(shift=0.0):
    """(Tracks, xyz [T,3]) of the filter cases, the whole set translated by `shift` along (1, -1, 1)."""
    T = np.array([shift, -shift, shift])
    b = SceneBuilder(INTR, seed=3)
    xyz = []

    def track(label, X, cams, **kw):
        xyz.append(np.asarray(X, np.float64))
        if label.startswith("angle_"):  # the pixels play no part in the angle, and some of these cameras have zc == 0
            kw["xy"] = [[100.0, 200.0]] * len(cams)
        return b.add_track(label, X, cams, **kw)

    with mp.workdps(DPS):
        X0 = T + np.array([0.0, 0.0, 5.0])
        near = _ident_cam(b, T + np.array([0.0, 0.0, -5.0]))  # 10 from X0 along z
        for name, deg in (("1e-7", math.degrees(1e-7)), ("1e-5", math.degrees(1e-5)), ("1e-3", math.degrees(1e-3)), ("1.5deg", 1.5),
                          ("45deg", 45.0), ("120deg", 120.0), ("179deg", 179.0)):
            a = mp.radians(mpf(deg))
            c = _ident_cam(b, X0 + np.array([float(-13 * mp.sin(a)), 0.0, float(-13 * mp.cos(a))]), 1)
            track("angle_" + name, X0, [near, c])
        # 90 degrees from a 3-4-5 triangle, and one ulp of 4 to either side of it
        c3 = _ident_cam(b, X0 + np.array([3.0, 0.0, 0.0]))
        ulp = math.nextafter(4.0, math.inf) - 4.0
        for name, dx in (("90deg", 0.0), ("90deg_below", ulp), ("90deg_above", -ulp)):
            track("angle_" + name, X0, [c3, _ident_cam(b, X0 + np.array([dx, 4.0, 0.0]), 1)])
        track("angle_180deg", X0, [near, _ident_cam(b, X0 + np.array([0.0, 0.0, 13.0]))])
        # zero-length rays and coincident centres: exactly 0
        cx = _ident_cam(b, X0)
        track("point_at_centre", X0, [cx, near], xy=[[0.0, 0.0], [640.0, 480.0]])
        track("identical_centres", X0, [near, _ident_cam(b, T + np.array([0.0, 0.0, -5.0]), 1)])  # same t, bit for bit
        twin = b.add_camera(axis_quat((0, 1, 0), 10.0), T + np.array([0.0, 0.0, -5.0]), 1)
        track("rotated_twin_centre", X0, [near, twin])  # one centre up to the rounding of t = -R C: general criterion
        track("same_camera_twice", X0, [near, near])
        track("empty", X0, [])
        track("one_element", X0, [near])
        # 40 views: 38 in a tight cluster, two 30 degrees to either side; the maximum is the pair of the two
        cluster = [b.add_camera_seeing(axis_quat((0, 1, 0), 0.01 * i), X0, (0.0, 0.0, 10.0 + 0.01 * i), i % 2) for i in range(38)]
        wide = [b.add_camera_seeing(axis_quat((0, 1, 0), s * 30.0), X0, (0.0, 0.0, 9.0), 1) for s in (-1, 1)]
        track("max_is_last_pair", X0, cluster + wide)
        track("max_is_first_pair", X0, wide + cluster)
        # front: identity rotation and t = 0, so zc is X[2] exactly.  Only meaningful without the shift.
        if shift == 0.0:
            origin = _ident_cam(b, (0.0, 0.0, 0.0))
            e = 2.0 ** -52
            for z in (e, math.nextafter(e, 0.0), math.nextafter(e, 1.0), 0.0, -0.0, -1.0, 1e-300, 1e300):
                track(f"front_z={z!r}", (0.0, 0.0, z), [origin], xy=[[640.0, 480.0]])
            track("err_zc_zero_off_axis", (0.5, -0.25, 0.0), [origin], xy=[[640.0, 480.0]])
        # squared error: exact projections, offsets of 0.5 and 1e4 px, a point 0.01 in front, a point behind
        rig = _rig(b, 5, T + np.array([0.0, 0.0, 5.0]))
        Xe = X0 + np.array([0.3, -0.2, 0.4])
        exact = [b.project(c, Xe) for c in rig]
        track("err_exact", Xe, rig)
        track("err_half_px", Xe, rig, xy=[[u + 0.5, v] for u, v in exact])
        track("err_1e4_px", Xe, rig, xy=[[u - 6e3, v + 8e3] for u, v in exact])
        close = b.add_camera_seeing(axis_quat((1, 1, 0), 25.0), Xe, (0.004, -0.003, 0.01), 1)
        track("err_zc_0.01", Xe, [close, rig[0]])
        behind = b.add_camera_seeing(axis_quat((0, 1, 0), 5.0), Xe, (0.5, 0.4, -3.0), 0)
        track("err_behind", Xe, [behind, rig[1]], xy=[b.project(behind, Xe), exact[1]])
    return b.tracks(), np.array(xyz).reshape(-1, 3)


def _problem(b: SceneBuilder, pts, obs, magnitude):
    obs = np.asarray(obs, np.int64).reshape(-1, 2)
    nc = len(b.quat)
    return BAProblem(cam_quat=np.array(b.quat), cam_t=np.array(b.t), pts=np.asarray(pts, np.float64).reshape(-1, 3), cam_intr=b.intr,
                     cam_intr_idx=np.array(b.intr_idx, np.int32), pose_const=np.ones(nc, np.uint8), pt_const=np.zeros(len(pts), np.uint8),
                     obs_cam=obs[:, 0].astype(np.int32), obs_pt=obs[:, 1].astype(np.int32), obs_xy=np.zeros((len(obs), 2)),
                     reproj_loss_magnitude=float(magnitude))


@functools.lru_cache(maxsize=None)
def friendly_cov_problem(magnitude=1.0, n_obs=None):
    """64 friendly landmarks with 2..7 observations each over 12 cameras with both intrinsics rows;
    `n_obs` keeps the first observations only, 257 by default (255 / 256 / 257 around the 256 threads of an accumulation block)."""
    b = SceneBuilder(INTR)
    rig = _rig(b, 12)
    pts = _friendly_points(np.random.default_rng(8), 64)
    obs = [(rig[(5 * p + 7 * j) % 12], p) for j in range(7) for p in range(64) if j < 2 + (p * 3 + 1) % 6]
    order = np.random.default_rng(9).permutation(len(obs))  # observations of one landmark spread over the list
    obs = [obs[i] for i in order]
    assert len(obs) >= 257
    return _problem(b, pts, obs[: (n_obs or 257)], magnitude)


@functools.lru_cache(maxsize=None)
def hard_cov_problem():
    """(problem, labels): the 5000-observation landmark beside two-observation ones, low-parallax pairs, a landmark
    0.01 in front of a camera, landmarks with 0 and 1 observation between ordinary ones."""
    b = SceneBuilder(INTR)
    rig = _rig(b, 50)
    rng = np.random.default_rng(12)
    pts, obs, labels = [], [], []

    def landmark(label, X, cams):
        pts.append(np.asarray(X, np.float64))
        labels.append(label)
        obs.extend((c, len(pts) - 1) for c in cams)

    fr = _friendly_points(rng, 8)
    landmark("two_obs_a", fr[0], [rig[1], rig[30]])
    landmark("obs5000", fr[1], [rig[i % 50] for i in range(5000)])
    landmark("two_obs_b", fr[2], [rig[7], rig[44]])
    landmark("no_obs", fr[3], [])
    landmark("ordinary_a", fr[4], rig[:4])
    landmark("one_obs", fr[5], [rig[9]])
    landmark("ordinary_b", fr[6], rig[10:15])
    for ratio in (1e-2, 1e-3, 1e-4):
        c0 = b.add_camera((0, 0, 0, 1), (-ratio, 0, 0), 0)
        c1 = b.add_camera(axis_quat((0, 1, 0), 0.5), (ratio, 0, 0), 1)
        landmark(f"parallax{ratio:g}", (0.03, -0.02, 2.0), [c0, c1])
    close = b.add_camera_seeing(axis_quat((1, 1, 0), 25.0), fr[7], (0.004, -0.003, 0.01), 1)
    landmark("zc_0.01", fr[7], [close, rig[0], rig[20]])
    landmark("ordinary_c", fr[0] + 0.1, rig[40:43])
    order = np.random.default_rng(13).permutation(len(obs))
    return _problem(b, pts, [obs[i] for i in order], 1.0), labels


# ============================================================================================================
# the criteria, applied: each function takes the implementation under test and returns the list of failures
# ============================================================================================================
# 8 x the largest ratio of the NumPy evaluation over the cases above, rounded up to a power of two (the table is in
# tests/test_gpu_exact_geometry.py; `PYTHONPATH=. python tests/exact_geometry.py` prints it again)
C_T, C_A, C_E, C_P = 16.0, 1.0, 2.0, 128.0
ANGLE_EXACTLY_ZERO = ("point_at_centre", "identical_centres", "same_camera_twice", "empty", "one_element")


@functools.lru_cache(maxsize=None)
def triangulation_case_reference():
    return triangulation_reference(triangulation_cases()[0].tracks())


def triangulation_failures(triangulate, n_tracks=None, stats=None):
    """`triangulate(Tracks) -> xyz`.  n_tracks: only the first tracks (the friendly ones), for the block-edge launches."""
    b, groups = triangulation_cases()
    tr = b.tracks(n_tracks)
    ref = triangulation_case_reference()[: tr.n_tracks]
    group_of = {k: name for name, idx in groups.items() for k in idx}
    xyz = np.asarray(triangulate(tr), np.float64)
    fails = []
    for k, (back, fwd) in enumerate(triangulation_ratios(ref, xyz)):
        what = f"track {k} {tr.labels[k]} ({group_of[k]}) xyz={xyz[k]}"
        if back is None:
            if group_of[k] != "rank_deficient":
                fails.append(f"{what}: not finite")
            continue
        if stats is not None:
            stats.append((group_of[k], "backward", back))
        if not back <= C_T:
            fails.append(f"{what}: backward ratio {back:.3g} > {C_T}")
        if ref[k] is not None and triangulation_informative(ref[k], C_T):
            if stats is not None:
                stats.append((group_of[k], "forward", fwd))
            if not fwd <= C_T:
                fails.append(f"{what}: forward ratio {fwd:.3g} > {C_T}")
    return fails


@functools.lru_cache(maxsize=None)
def filter_case_reference(shift=0.0):
    tr, xyz = filter_cases(shift)
    return filter_reference(tr, xyz)


def filter_failures(filter_tracks, shift=0.0, stats=None):
    """`filter_tracks(Tracks, xyz) -> (max_angle [T], sq_err [E], front [E])`."""
    tr, xyz = filter_cases(shift)
    ref = filter_case_reference(shift)
    ang, err, front = filter_tracks(tr, xyz)
    fails = []
    for k, r in enumerate(ref):
        lab, e0, e1 = tr.labels[k], int(tr.track_start[k]), int(tr.track_start[k + 1])
        ra = angle_ratio(r, ang[k])
        re = sq_err_ratios(r, err[e0:e1])
        if stats is not None:
            stats.append((lab, "angle", ra))
            stats.extend((lab, "sq_err", v) for v in re)
        if not ra <= C_A:
            fails.append(f"{lab}: angle {ang[k]!r} vs {float(r['angle'])!r}, ratio {ra:.3g} > {C_A}")
        if lab in ANGLE_EXACTLY_ZERO and not ang[k] == 0.0:
            fails.append(f"{lab}: angle {ang[k]!r} is not exactly 0")
        for i, v in enumerate(re):
            if not v <= C_E:
                fails.append(f"{lab}[{i}]: sq_err {err[e0 + i]!r} vs {r['err'][i] if r['err'][i] is None else float(r['err'][i])!r}, ratio {v:.3g} > {C_E}")
        for i, f in enumerate(r["front"]):
            if bool(front[e0 + i]) != bool(f):
                fails.append(f"{lab}[{i}]: front {bool(front[e0 + i])} vs {bool(f)} at zc = {float(r['zc'][i])!r}")
    return fails


@functools.lru_cache(maxsize=None)
def _cov_reference(which, *args):
    return point_hessians(which(*args)[0] if which is hard_cov_problem else which(*args))


def cov_failures(point_covs, which, *args, stats=None):
    """`point_covs(BAProblem) -> [N,3,3]` on `which(*args)`, one of the two problem makers above."""
    prob = which(*args)
    labels = [f"landmark {p}" for p in range(prob.n_pts)] if which is not hard_cov_problem else prob[1]
    prob = prob[0] if which is hard_cov_problem else prob
    ref = _cov_reference(which, *args)
    covs = np.asarray(point_covs(prob), np.float64)
    fails = []
    for lab, r, ratio, c in zip(labels, ref, cov_ratios(ref, covs), covs):
        if stats is not None and r["inv"] is not None:
            stats.append((lab, "cov", ratio))
        if not ratio <= C_P:
            fails.append(f"{lab} ({r['n_obs']} obs, cond {float(r['cond']):.3g}): ratio {ratio:.3g} > {C_P}, cov {c.ravel()}")
    return fails


def all_failures(triangulate, filter_tracks, point_covs, stats=None):
    """Every case of the GPU tests through one implementation: {check name: failures}."""
    out = {}
    for n in BLOCK_EDGES + (None,):
        out[f"triangulation n_tracks={n}"] = triangulation_failures(triangulate, n, stats if n is None else None)
    for shift in (0.0, 1e4):
        out[f"filters shift={shift:g}"] = filter_failures(filter_tracks, shift, stats)
    for mag in (0.25, 4.0, 1e-6):
        out[f"covs magnitude={mag:g}"] = cov_failures(point_covs, friendly_cov_problem, mag, stats=stats)
    for n in (255, 256, 257):
        out[f"covs n_obs={n}"] = cov_failures(point_covs, friendly_cov_problem, 1.0, n, stats=stats)
    out["covs hard"] = cov_failures(point_covs, hard_cov_problem, stats=stats)
    return out


# ============================================================================================================
# candidate tracks (mpsfm_tri_estimate_batch) and init-pair points (mpsfm_init_pair_candidates): the exact reference
# ============================================================================================================
ANGULAR, REPROJECTION = 0, 1
# 8 x the largest NumPy ratio over the candidate and init-pair cases, rounded up to a power of two (same table)
C_Z, C_R, C_S, C_RA, C_L = 4.0, 8.0, 4.0, 2.0, 16.0


class ExactView:
    """One observation read exactly: P [3][4] cam_from_world, C = -R^T t, xn = (xy - c) / f, K, xy; all mpf."""

    @_hp
    def __init__(self, P, K, xy):
        P = np.asarray(P, np.float64).reshape(3, 4)
        self.P = [[mpf(float(P[i, j])) for j in range(4)] for i in range(3)]
        self.R = [r[:3] for r in self.P]
        self.t = [r[3] for r in self.P]
        self.K, self.xy = _vec(K), _vec(xy)
        self.xn = [(self.xy[0] - self.K[2]) / self.K[0], (self.xy[1] - self.K[3]) / self.K[1]]
        self.C = centre(self.R, self.t)
        self._term = None

    def term(self):
        """(P - x x^T P)^T (P - x x^T P), x the unit viewing ray: this view's share of the multi-view matrix."""
        if self._term is None:
            x = [self.xn[0], self.xn[1], mpf(1)]
            n = _norm(x)
            xm = mp.matrix([a / n for a in x])
            P = mp.matrix(self.P)
            M = P - xm * (xm.T * P)
            self._term = M.T * M
        return self._term


def exact_views(P, K, xy):
    return [ExactView(p, k, x) for p, k, x in zip(np.asarray(P).reshape(-1, 12), np.asarray(K).reshape(-1, 4), np.asarray(xy).reshape(-1, 2))]


@_hp
def two_view_matrix(a: ExactView, b: ExactView):
    """A2 = sum row^T row over the four rows x * P_2 - P_0, y * P_2 - P_1 of tri_two_view (unnormalised)."""
    A = mp.zeros(4)
    for v in (a, b):
        for c in range(2):
            row = mp.matrix([[v.xn[c] * v.P[2][k] - v.P[c][k] for k in range(4)]])
            A += row.T * row
    return A


@_hp
def multi_view_matrix(views, idx):
    A = mp.zeros(4)
    for i in idx:
        A += views[i].term()
    return A


@_hp
def solve_model(A):
    """dict(A, fro, lam, X, gap, fwd_unit, dirs) of the smallest eigenvector of A, or None where it has no finite point.
    dirs: three 3-vectors, the first-order bound of the device's error in X resolved by eigendirection.  A computed v
    that meets the backward criterion is an eigenvector of A + E with |E| <= C_t eps |A|_F, so to first order
    dv = sum_k c_k v_k with |c_k| <= C_t eps |A|_F / (lambda_k - lambda_1), and X = v[:3] / v[3] moves by
    c_k (v_k[:3] - X v_k[3]) / v[3] per direction; the norm bound fwd_unit of triangulation_reference is its coarse form.
    dirs is None (nothing can be decided from this model) where the gap is not above 4 C_t eps |A|_F."""
    lam, vec = eig(A)
    v = vec[0]
    if v[3] == 0:
        return None
    X = [v[i] / v[3] for i in range(3)]
    fro, gap = _fro(A), lam[1] - lam[0]
    nx = _norm(X)
    dirs = None
    if gap > 4 * C_T * mpf(EPS) * fro:
        dirs = [[C_T * mpf(EPS) * fro / (lam[k] - lam[0]) * (vec[k][i] - X[i] * vec[k][3]) / v[3] for i in range(3)] for k in (1, 2, 3)]
    return dict(A=A, fro=fro, lam=lam, X=X, gap=gap, fwd_unit=fro / gap * (1 + nx) * mp.sqrt(1 + nx * nx) if gap > 0 else None, dirs=dirs)


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def _prop(grad, dirs):
    """first-order effect of the model's forward error on a quantity with gradient `grad` in X"""
    return mp.inf if dirs is None else sum(abs(_dot(grad, d)) for d in dirs)


def _prop_norm(scale, dirs):
    """the same from a bound `scale` on the gradient's length (where the gradient itself has no direction)"""
    return mp.inf if dirs is None else scale * sum(_norm(d) for d in dirs)


def _ratio(dist, bound):
    if bound == 0:
        return mp.inf if dist > 0 else mpf(0)
    return mp.inf if bound == mp.inf and dist == mp.inf else dist / bound


@_hp
def depth_numbers(v: ExactView, X):
    """(zc, mag, gradient): mag = sum |P_2j X_j| + |t_2|, the terms that cancel in the depth."""
    z = _dot(v.R[2], X) + v.t[2]
    return z, sum(abs(v.R[2][j] * X[j]) for j in range(3)) + abs(v.t[2]), v.R[2]


@_hp
def angular_numbers(v: ExactView, X):
    """(e, form, gradient of e in X or None, 1 / |b|) of the angular residual e = angle((xn, 1), P X); see the docstring of
    tests/test_gpu_exact_geometry.py for the form.  e is None where P X = 0."""
    a = [v.xn[0], v.xn[1], mpf(1)]
    b = to_camera(v.R, v.t, X)
    mag = [sum(abs(v.R[i][j] * X[j]) for j in range(3)) + abs(v.t[i]) for i in range(3)]
    na, nb = _norm(a), _norm(b)
    if nb == 0:
        return None, None, None, None
    dot = _dot(a, b)
    cr = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    e = mp.atan2(_norm(cr), dot)
    cs, sn = dot / (na * nb), mp.sin(e)
    dcs = sn * _norm(mag) / nb + sum(abs(a[k] * b[k]) for k in range(3)) / (na * nb) + 2 * abs(cs)
    form = dcs / max(sn, mp.sqrt(mpf(EPS)))
    grad = None
    if sn > mpf(10) ** -40:
        gb = [-(a[k] / na - cs * b[k] / nb) / (nb * sn) for k in range(3)]
        grad = [sum(v.R[i][j] * gb[i] for i in range(3)) for j in range(3)]
    return e, form, grad, 1 / nb


@_hp
def reprojection_numbers(v: ExactView, X):
    """(err, scale s, gradient of err in X, (|grad du|, |grad dv|)) at zc != 0; the forms are those of filter_numbers."""
    xc, yc, z = to_camera(v.R, v.t, X)
    K = v.K
    du, dv = K[0] * xc / z + K[2] - v.xy[0], K[1] * yc / z + K[3] - v.xy[1]
    mag = [sum(abs(v.R[i][j] * X[j]) for j in range(3)) + abs(v.t[i]) for i in range(3)]
    mu = K[0] / abs(z) * (mag[0] + abs(xc / z) * mag[2]) + abs(K[2]) + abs(v.xy[0])
    mv = K[1] / abs(z) * (mag[1] + abs(yc / z) * mag[2]) + abs(K[3]) + abs(v.xy[1])
    gu = [K[0] * (v.R[0][j] * z - xc * v.R[2][j]) / (z * z) for j in range(3)]
    gv = [K[1] * (v.R[1][j] * z - yc * v.R[2][j]) / (z * z) for j in range(3)]
    return du * du + dv * dv, mu * mu + mv * mv, [2 * du * gu[j] + 2 * dv * gv[j] for j in range(3)], (gu, gv)


@_hp
def tri_angle_numbers(C1, C2, X):
    """(angle, kappa, gradient of the angle in X or None, 1/|d1| + 1/|d2|) of tri_angle; angle and kappa from angle_pair."""
    ang, kappa = angle_pair(C1, C2, X)
    d1, d2 = [X[k] - C1[k] for k in range(3)], [X[k] - C2[k] for k in range(3)]
    n1, n2 = _norm(d1), _norm(d2)
    if n1 == 0 or n2 == 0:
        return ang, kappa, None, mp.inf
    cr = [d1[1] * d2[2] - d1[2] * d2[1], d1[2] * d2[0] - d1[0] * d2[2], d1[0] * d2[1] - d1[1] * d2[0]]
    sn, cs = _norm(cr) / (n1 * n2), _dot(d1, d2) / (n1 * n2)
    grad = None
    if sn > mpf(10) ** -40:
        grad = [-(d2[k] / n2 - cs * d1[k] / n1) / (n1 * sn) - (d1[k] / n1 - cs * d2[k] / n2) / (n2 * sn) for k in range(3)]
    return ang, kappa, grad, 1 / n1 + 1 / n2


@_hp
def ref_angle_numbers(C1, C2, X):
    """The reference's calculate_triangulation_angle on PLAIN lengths, exactly: (angle in degrees or NaN, c, dc, slope).
    c = (r1 + r2 - b) / (2 sqrt(r1 r2)) with r1 = |X - C1|, r2 = |X - C2|, b = |C1 - C2|; angle 0 where the denominator
    is 0, NaN where c exceeds 1 in magnitude.  dc is the rounding form of c and slope = 1 / max(sin acos c, sqrt(eps))."""
    d1, d2 = [X[k] - C1[k] for k in range(3)], [X[k] - C2[k] for k in range(3)]
    r1, r2, b = _norm(d1), _norm(d2), _norm([C1[k] - C2[k] for k in range(3)])
    den = 2 * mp.sqrt(r1 * r2)
    if den == 0:
        return mpf(0), mpf(0), mpf(0), mpf(1)
    c = (r1 + r2 - b) / den
    g1, g2 = (_norm(X) + _norm(C1)) / r1, (_norm(X) + _norm(C2)) / r2
    gb = (_norm(C1) + _norm(C2)) / b if b != 0 else mpf(0)
    dc = ((g1 + 2) * r1 + (g2 + 2) * r2 + (gb + 2) * b) / den + abs(c) * ((g1 + g2) / 2 + 5)
    if abs(c) > 1:
        return mp.nan, c, dc, 1 / mp.sqrt(mpf(EPS))
    a = mp.acos(c)
    return min(a, mp.pi - a) * 180 / mp.pi, c, dc, 1 / max(mp.sin(a), mp.sqrt(mpf(EPS)))


@_hp
def num_trials_numbers(k, n, confidence=0.9999):
    """(dyn_max, margin) of tri_num_trials: ceil(3 log(1 - confidence) / log(1 - (k / n)^2)) with its special cases; the
    margin is the distance of the real value from the nearest integer over C_s eps times its rounding form."""
    if 1 - mpf(float(confidence)) <= 0 or k == 0:
        return 2 ** 63 - 1, mp.inf
    if k == n:
        return 1, mp.inf
    v, form = _num_trials_value(k, n, confidence)
    return int(mp.ceil(v)), _ratio(min(v - mp.floor(v), mp.ceil(v) - v), C_S * mpf(EPS) * form)


@_hp
def _num_trials_value(k, n, confidence):
    """(v, form) of v = 3 log(1 - confidence) / log(1 - (k / n)^2) for 0 < k < n.  1 - confidence is exact in fp64; the ratio,
    its square and the difference carry eps (1 + 3 r^2 / denom) relative to denom, which the logarithm divides by
    |log denom|; the two logarithms, the division and the product add a few eps."""
    nom = 1 - mpf(float(confidence))
    r = mpf(k) / n
    denom = 1 - r * r
    v = 3 * mp.log(nom) / mp.log(denom)
    return v, abs(v) * (3 + (1 + 3 * r * r / denom) / abs(mp.log(denom)) + 1 / abs(mp.log(nom)))


class _Support:
    def __init__(self, count, total, bound, inl, margin):
        self.count, self.total, self.bound, self.inl, self.margin = count, total, bound, inl, margin


class ExactCandidate:
    """The views of one candidate with the exact models and supports made so far (shared by both residual types)."""

    def __init__(self, P, K, xy):
        self.views = exact_views(P, K, xy)
        self.n = len(self.views)
        self._models, self._estimates, self._supports = {}, {}, {}

    def model(self, idx):
        idx = tuple(idx)
        if idx not in self._models:
            A = two_view_matrix(self.views[idx[0]], self.views[idx[1]]) if len(idx) == 2 else multi_view_matrix(self.views, idx)
            m = solve_model(A)
            if m is not None:
                m["idx"] = idx
            self._models[idx] = m
        return self._models[idx]

    @_hp
    def estimate(self, idx, min_tri_angle):
        """tri_estimate: (ok, model, margin).  ok needs every depth >= 2^-52 and one pair's angle >= min_tri_angle: a true
        outcome is as firm as its weakest test, a false one as its firmest failing test."""
        key = (tuple(idx), float(min_tri_angle))
        if key in self._estimates:
            return self._estimates[key]
        m = self.model(idx)
        if m is None:
            out = (False, None, mpf(0))
        else:
            X, dirs = m["X"], m["dirs"]
            passing, failing = [], []
            for i in idx:
                z, mag, g = depth_numbers(self.views[i], X)
                (passing if z >= mpf(EPS) else failing).append(_ratio(abs(z - mpf(EPS)), C_Z * mpf(EPS) * mag + _prop(g, dirs)))
            thr = mpf(float(min_tri_angle))
            if thr > 0:  # the device's angle is never negative: a threshold of 0 always passes
                ok_pairs, all_pairs = [], []
                for a in range(len(idx)):
                    for b in range(a):
                        ang, kappa, g, gn = tri_angle_numbers(self.views[idx[a]].C, self.views[idx[b]].C, X)
                        mg = _ratio(abs(ang - thr), C_A * mpf(EPS) * kappa + (_prop(g, dirs) if g is not None else _prop_norm(gn, dirs)))
                        all_pairs.append(mg)
                        if ang >= thr:
                            ok_pairs.append(mg)
                            if mg > 1:
                                break
                    if ok_pairs and ok_pairs[-1] > 1:
                        break
                if ok_pairs:
                    passing.append(max(ok_pairs))
                else:
                    failing.append(min(all_pairs))
            out = (False, m, max(failing)) if failing else (True, m, min(passing))
        self._estimates[key] = out
        return out

    @_hp
    def support(self, m, max_error, rt):
        key = (m["idx"], float(max_error), rt)
        if key in self._supports:
            return self._supports[key]
        thr = mpf(float(max_error)) ** 2
        X, dirs = m["X"], m["dirs"]
        count, total, bound, inl, margin = 0, mpf(0), mpf(0), [], mp.inf
        for v in self.views:
            if rt == REPROJECTION:
                z, mag, g = depth_numbers(v, X)
                mz = _ratio(abs(z - mpf(EPS)), C_Z * mpf(EPS) * mag + _prop(g, dirs))
                if z < mpf(EPS):
                    r, rb, mg = mp.inf, mpf(0), mz  # DBL_MAX
                else:
                    r, s, g, (gu, gv) = reprojection_numbers(v, X)
                    rb = C_E * mpf(EPS) * (r + s) + _prop(g, dirs) + _prop(gu, dirs) ** 2 + _prop(gv, dirs) ** 2 + mpf(EPS) * thr
                    mg = min(mz, _ratio(abs(r - thr), rb))
            else:
                e, form, g, gn = angular_numbers(v, X)
                if e is None:
                    r, rb, mg = mp.inf, mpf(0), mpf(0)
                else:
                    de = C_R * mpf(EPS) * form + (_prop(g, dirs) if g is not None else _prop_norm(gn, dirs))
                    r, rb = e * e, 2 * e * de + de * de + mpf(EPS) * thr
                    mg = _ratio(abs(r - thr), rb)
            margin = min(margin, mg)
            inl.append(bool(r <= thr))
            if inl[-1]:
                count, total, bound = count + 1, total + r, bound + rb
        out = _Support(count, total, bound + self.n * mpf(EPS) * total, inl, margin)
        self._supports[key] = out
        return out


def _better(l: _Support, r):
    """tri_better and its margin; r is None for the initial (0, DBL_MAX)."""
    if r is None:
        return True, mp.inf
    if l.count != r.count:
        return l.count > r.count, mp.inf
    return l.total < r.total, _ratio(abs(l.total - r.total), l.bound + r.bound) if l.total != r.total or l.bound + r.bound > 0 else mp.inf


def default_min_num_trials(n):
    return n * (n - 1) // 2 if n <= 15 else 0


@_hp
def exact_loransac(cand: ExactCandidate, min_tri_angle, max_error, rt, min_num_trials=None, confidence=0.9999, max_num_trials=10000):
    """tri_ransac_scratch walked with exact arithmetic.  Returns dict(ok, mask [n] bool, model (solve_model's dict with idx,
    None on failure), margin, trials, lo_rounds): every comparison on the path adds its margin (distance from the threshold
    over the error bound of the compared quantity); the candidate is decided when margin > 1."""
    n = cand.n
    fail = dict(ok=False, mask=[False] * n, model=None, margin=mp.inf, trials=0, lo_rounds=0)
    if n < 2:
        return fail
    if min_num_trials is None:
        min_num_trials = default_min_num_trials(n)
    margin = [mp.inf]

    def note(m):
        margin[0] = min(margin[0], m)

    best, best_model = None, None
    max_trials = min(max_num_trials, n * (n - 1) // 2)
    dyn_max, trials, a, b, abort, lo_rounds = max_trials, 0, 0, 1, False, 0
    while trials < max_trials:
        if abort:
            trials += 1
            break
        pair = (a, b)
        b += 1
        if b == n:
            a += 1
            b = a + 1
        ok, m, mg = cand.estimate(pair, min_tri_angle)
        note(mg)
        if ok:
            sup = cand.support(m, max_error, rt)
            note(sup.margin)
            bt, mg = _better(sup, best)
            note(mg)
            if bt:
                best, best_model, res = sup, m, sup
                if sup.count > 2:
                    for _ in range(10):
                        idx = [i for i in range(n) if res.inl[i]]
                        prev = best.count
                        ok2, lm, mg = cand.estimate(idx, min_tri_angle)
                        note(mg)
                        if ok2:
                            ls = cand.support(lm, max_error, rt)
                            note(ls.margin)
                            bt2, mg = _better(ls, best)
                            note(mg)
                            if bt2:
                                best, best_model, res = ls, lm, ls
                                lo_rounds += 1
                        if best.count <= prev:
                            break
                dyn_max, mg = num_trials_numbers(best.count, n, confidence)
                note(mg)
            if trials >= dyn_max and trials >= min_num_trials:
                abort = True
        trials += 1
    if best is None or best.count < 2:
        fail.update(margin=margin[0], trials=trials)
        return fail
    return dict(ok=True, mask=list(best.inl), model=best_model, margin=margin[0], trials=trials, lo_rounds=lo_rounds)


# ---- plain NumPy float64 evaluations of the same quantities: the constants are measured with these -------------------
def numpy_model(P, K, xy, idx):
    """The point of the views idx: eigh of the two-view normal matrix (two views) or of the multi-view matrix."""
    P, K, xy = np.asarray(P).reshape(-1, 3, 4), np.asarray(K).reshape(-1, 4), np.asarray(xy).reshape(-1, 2)
    xn = (xy - K[:, 2:]) / K[:, :2]
    A = np.zeros((4, 4))
    if len(idx) == 2:
        rows = np.array([xn[i, c] * P[i, 2] - P[i, c] for i in idx for c in range(2)])
        A = rows.T @ rows
    else:
        for i in idx:
            x = np.array([xn[i, 0], xn[i, 1], 1.0])
            x /= np.linalg.norm(x)
            M = P[i] - np.outer(x, x @ P[i])
            A += M.T @ M
    _, Q = np.linalg.eigh(A)
    with np.errstate(all="ignore"):
        return Q[:3, 0] / Q[3, 0]


def numpy_depth(P, X):
    P = np.asarray(P).reshape(3, 4)
    return P[2, :3] @ X + P[2, 3]


def numpy_angular(P, K, xy, X):
    P = np.asarray(P).reshape(3, 4)
    a = np.array([(xy[0] - K[2]) / K[0], (xy[1] - K[3]) / K[1], 1.0])
    b = P[:, :3] @ X + P[:, 3]
    return np.arccos(np.clip(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)), -1.0, 1.0))


def numpy_reprojection(P, K, xy, X):
    P = np.asarray(P).reshape(3, 4)
    pc = P[:, :3] @ X + P[:, 3]
    d = K[:2] * pc[:2] / pc[2] + K[2:] - xy
    return d @ d


def numpy_num_trials(k, n, confidence=0.9999):
    return np.log(1.0 - confidence) / np.log(1.0 - (k / n) ** 2) * 3.0


def numpy_ref_angle_deg(C1, C2, X):
    r1, r2, b = np.linalg.norm(X - C1), np.linalg.norm(X - C2), np.linalg.norm(C1 - C2)
    den = 2.0 * np.sqrt(r1 * r2)
    if den == 0.0:
        return 0.0
    with np.errstate(invalid="ignore"):
        a = abs(np.arccos((r1 + r2 - b) / den))
    return min(a, np.pi - a) * (180.0 / np.pi) if a == a else np.nan


# ---- comparison of an output with the exact numbers ------------------------------------------------------------------
@_hp
def ref_angle_ratio(C1, C2, X, got):
    """Smallest C with which `got` (degrees, possibly NaN) is a legal value of the reference's angle at the fp64 point X.
    In exact arithmetic |c| <= 1 always ((sqrt r1 - sqrt r2)^2 <= |r1 - r2| <= b <= r1 + r2), so a NaN is rounding: it is
    legal where 1 - |c| is within the bound of c, and only there; a finite value must lie within C eps dc slope of the exact
    angle (in radians)."""
    ang, c, dc, slope = ref_angle_numbers(C1, C2, _vec(X))
    got = float(got)
    if math.isnan(got):
        return float(_ratio(1 - abs(c), mpf(EPS) * dc))
    if mp.isnan(ang):
        return float(_ratio(abs(c) - 1, mpf(EPS) * dc))
    return float(_ratio(abs(mpf(got) - ang) * mp.pi / 180, mpf(EPS) * (dc * slope + ang * mp.pi / 180)))


@_hp
def lift_ratio(xy, K, d, rescale, got):
    """max_k |got_k - L_k| / (eps |L_k|) for the exact L = ((x - cx) / fx ds, (y - cy) / fy ds, ds), ds = d rescale."""
    x, y = _vec(xy)
    K = _vec(K)
    ds = mpf(float(d)) * mpf(float(rescale))
    L = [(x - K[2]) / K[0] * ds, (y - K[3]) / K[1] * ds, ds]
    return float(max(_ratio(abs(mpf(float(g)) - l), mpf(EPS) * abs(l)) for g, l in zip(got, L)))


# ---- candidate case set ----------------------------------------------------------------------------------------------
CAND_MIN_ANGLE = math.radians(0.5)  # Create's min_angle as the existing parity test uses it
CAND_MAX_ERROR = {ANGULAR: math.radians(2.0), REPROJECTION: 4.0}  # Create 2 degrees, CompleteImage 4 px
CAND_BLOCK_EDGES = (63, 64, 65, 129)  # candidate counts around the 64 threads of a k_tri_ransac block
CAND_GOLDEN = "exact_candidates.npz"
OUTLIER_PX = ((150.0, -220.0), (-310.0, 180.0), (95.0, 260.0))  # far beyond 2 degrees (35 px at f = 1000) and 4 px
N_RANDOM = 200


class CandidateSet:
    """Named candidates: label, group, [n,12] P, [n,4] K, [n,2] xy, min_num_trials (-1: the n <= 15 rule)."""

    def __init__(self, seed=21):
        self.b = SceneBuilder(INTR, seed=seed)
        self.labels, self.groups, self.P, self.K, self.xy, self.mnt = [], [], [], [], [], []

    @_hp
    def _P(self, cam):
        R = rotation(self.b.quat[cam])
        return [float(R[i][j]) if j < 3 else float(self.b.t[cam][i]) for i in range(3) for j in range(4)]

    def add(self, label, group, X, cams, noise_px=0.5, offsets=None, min_num_trials=-1, rng=None):
        """`X`: one point, or one per view; offsets {view: (du, dv)} make outliers; rng: a noise stream of its own."""
        b = self.b
        rng = b.rng if rng is None else rng
        Xs = [X] * len(cams) if np.ndim(X) == 1 else list(X)
        xy = []
        for i, c in enumerate(cams):
            p = b.project(c, Xs[i])
            n = noise_px[i] if np.ndim(noise_px) else noise_px
            if n:
                p = [p[0] + n * float(rng.standard_normal()), p[1] + n * float(rng.standard_normal())]
            if offsets and i in offsets:
                p = [p[0] + offsets[i][0], p[1] + offsets[i][1]]
            xy.append(p)
        self.labels.append(label)
        self.groups.append(group)
        self.P.append(np.array([self._P(c) for c in cams]).reshape(-1, 12))
        self.K.append(self.b.intr[[self.b.intr_idx[c] for c in cams]].reshape(-1, 4))
        self.xy.append(np.array(xy, np.float64).reshape(-1, 2))
        self.mnt.append(int(min_num_trials))

    def arrays(self, order=None):
        order = range(len(self.labels)) if order is None else order
        cs = np.concatenate([[0], np.cumsum([len(self.P[i]) for i in order])]).astype(np.int64)
        return dict(cand_start=cs, P=np.concatenate([self.P[i] for i in order]), K=np.concatenate([self.K[i] for i in order]),
                    xy=np.concatenate([self.xy[i] for i in order]), min_num_trials=np.array([self.mnt[i] for i in order], np.int64),
                    labels=np.array([self.labels[i] for i in order]), groups=np.array([self.groups[i] for i in order]))


CAND_FRIENDLY_VIEWS = (2, 3, 5, 15, 16, 63, 64)


@functools.lru_cache(maxsize=None)
def candidate_cases() -> CandidateSet:
    """The named candidates and the seeded random set; groups: friendly, outliers, geometry, contract, threshold, random."""
    s = CandidateSet()
    b = s.b
    X0 = np.array([0.2, -0.1, 0.3])
    up = np.array([0.0, 1.5, 0.0])  # across the epipolar planes of the rig (cameras on a horizontal arc): 8 degrees at depth 10
    for n in CAND_FRIENDLY_VIEWS:
        s.add(f"friendly{n}", "friendly", X0 + 0.01 * n, _rig(b, n))
    for n in (3, 5, 15, 64):
        for where, v in (("first", 0), ("middle", n // 2), ("last", n - 1)):
            s.add(f"outlier{n}_{where}", "outliers", X0, _rig(b, n), offsets={v: OUTLIER_PX[v % 3]})
    # one true view and four views displaced across the epipolar planes by amounts that differ pairwise by > 100 px
    s.add("majority_outliers5", "outliers", X0, _rig(b, 5), offsets={1: (0.0, 120.0), 2: (0.0, -150.0), 3: (0.0, 300.0), 4: (0.0, -280.0)})
    s.add("clean20", "outliers", X0, _rig(b, 20))
    s.add("exhaustive_matters16", "outliers", X0, _rig(b, 16), noise_px=1.2, rng=np.random.default_rng(108))  # see trials_noisy16
    s.add("first_pairs_outliers20", "outliers", X0, _rig(b, 20), offsets={0: OUTLIER_PX[0], 1: OUTLIER_PX[1], 2: OUTLIER_PX[2]})
    # twenty noisy views (1.5 px) whose first two are neighbours on the arc: the first sample has a poor depth and few
    # inliers, and the local optimisation needs more than one round to collect the rest before the stop rule ends the loop
    rig20 = _rig(b, 20)
    near = [0, 13]  # yaw slots 0 and 1 of the rig
    s.add("lo_two_rounds20", "outliers", X0, [rig20[i] for i in near] + [rig20[i] for i in range(20) if i not in near], noise_px=1.5,
          rng=np.random.default_rng(201))
    # two structures: equal counts, the residual sum decides (views 2, 3 are exact, views 0, 1 carry 1 px of noise)
    s.add("two_pairs_tie", "outliers", [X0, X0, X0 + up, X0 + up], _rig(b, 4), noise_px=[1.0, 1.0, 0.0, 0.0])
    # ten views of one point, then ten of another: the stop rule ends the loop before a pair of the second ten is drawn
    s.add("two_structures20", "outliers", [X0] * 10 + [X0 + up] * 10, _rig(b, 20))
    # geometry: two cameras 2 h apart, the point 2 away on the bisector: the angle is 2 atan(h / 2)
    for name, ang in (("parallax_above", CAND_MIN_ANGLE * (1 + 1e-3)), ("parallax_below", CAND_MIN_ANGLE * (1 - 1e-3)),
                      ("parallax1e-2", 1e-2), ("parallax1e-4", 1e-4), ("parallax1e-6", 1e-6)):
        h = 2.0 * math.tan(ang / 2)
        c0 = b.add_camera((0, 0, 0, 1), (-h, 0, 0), 0)
        c1 = b.add_camera(axis_quat((0, 1, 0), 0.5), (h, 0, 0), 1)
        s.add(name, "geometry", (0.0, 0.0, 2.0), [c0, c1], noise_px=0.0)
    rig = _rig(b, 3)
    away = b.add_camera_seeing(axis_quat((0, 1, 0), 10.0), X0, (0.5, 0.4, -6.0), 0)  # X0 is 6 behind this camera
    away2 = b.add_camera_seeing(axis_quat((0, 1, 0), -25.0), X0, (-0.7, 0.2, -8.0), 1)
    away3 = b.add_camera_seeing(axis_quat((1, 0, 0), 15.0), X0, (0.1, -0.6, -7.0), 0)
    s.add("behind_one", "geometry", X0, [rig[0], rig[1], away], noise_px=0.0)
    # the point behind the second of three views, and the only pair in front of which it lies 0.11 degrees apart (below
    # min_tri_angle): the homogeneous two-view solve does not see the sign of a depth, so the pairs with the middle view
    # give the true point, and only the depth test of the sample's second view keeps them from becoming the result
    front = [b.add_camera((0, 0, 0, 1), (-0.01, 0, 0), 0), b.add_camera((0, 0, 0, 1), (0.5, 0.3, 20.0), 1), b.add_camera((0, 0, 0, 1), (0.01, 0, 0), 0)]
    s.add("behind_second_low_parallax", "geometry", (0.2, -0.1, 10.0), front, noise_px=0.3, rng=np.random.default_rng(34))
    s.add("behind_all2", "geometry", X0, [away, away2], noise_px=0.0)
    s.add("behind_all3", "geometry", X0, [away, away2, away3], noise_px=0.0)
    close = b.add_camera_seeing(axis_quat((1, 1, 0), 25.0), X0, (0.004, -0.003, 0.01), 1)
    s.add("depth0.01", "geometry", X0, [close, rig[0], rig[2]])
    # translated by 1e4, |A|_F is 1e9 and the forward bound C_t eps |A|_F / gap |(X, 1)| lets the point move by several 1e-2:
    # at the rig's own size no comparison of residual sums can be decided from it (five views translated by 1e3 can).  Two
    # views (no sums to compare) of a scene ten times the size, and three views of one three hundred times the size, can.
    for name, shift, scale, n in (("shift1e3", (1e3, 1e3, -1e3), 1.0, 5), ("shift1e4", (1e4, 1e4, -1e4), 10.0, 2),
                                  ("shift1e4_three", (1e4, 1e4, -1e4), 300.0, 3), ("scale1e-3", (0, 0, 0), 1e-3, 5), ("scale1e3", (0, 0, 0), 1e3, 5)):
        s.add(name, "geometry", np.asarray(shift) + scale * X0, _rig(b, n, shift, scale), rng=np.random.default_rng(33))
    big = [b.add_camera_seeing((1, 0, 0, 0), X0, (3.0, 1.0, 9.0), 0), b.add_camera_seeing((0, 1, 0, 0), X0, (-2.0, 2.5, 11.0), 1),
           b.add_camera_seeing((0, 0, 1, 0), X0, (1.0, -3.0, 10.0), 0)]
    s.add("rot180_pair", "geometry", X0, big[:2])
    s.add("rot180_three", "geometry", X0, big)
    # contract: 0 and 1 views between ordinary candidates, and a caller's min_num_trials
    s.add("empty", "contract", X0, [])
    s.add("contract_friendly3", "contract", X0, _rig(b, 3))
    s.add("one_view", "contract", X0, [rig[1]])
    # (noise stream 108 was found with the float64 restatement: a later two-view sample has the lower residual sum there,
    # so drawing all pairs and stopping early end at different points; the exact walk agrees, see lo / trials in the file)
    for lab, n, seed in (("trials_friendly", 5, 31), ("trials_noisy15", 15, 32), ("trials_noisy16", 16, 108)):
        cams = _rig(b, n)
        for mnt in (0, 1, n * (n - 1) // 2):  # the same pixels for the three settings
            s.add(f"{lab}_mnt{mnt}", "contract", X0, cams, noise_px=0.5 if n == 5 else 1.2, min_num_trials=mnt, rng=np.random.default_rng(seed))
    # threshold: a third view displaced by the residual bound itself (4 px; a ray at exactly max_error), and a pair whose
    # parallax is min_tri_angle to the last bit
    cams = _rig(b, 3)
    s.add("threshold_px", "threshold", X0, cams, noise_px=0.0, offsets={2: (0.0, 4.0)})
    with mp.workdps(DPS):  # the third pixel moved so that its ray makes exactly max_error with the ray of the point
        p, Kc = b.project(cams[2], X0), _vec(b.intr[b.intr_idx[cams[2]]])
        a0 = [(mpf(p[0]) - Kc[2]) / Kc[0], (mpf(p[1]) - Kc[3]) / Kc[1], mpf(1)]
        w = [-a0[1], a0[0], mpf(0)]
        th = mpf(CAND_MAX_ERROR[ANGULAR])
        a = [a0[k] / _norm(a0) * mp.cos(th) + w[k] / _norm(w) * mp.sin(th) for k in range(3)]
        off = (float(a[0] / a[2] * Kc[0] + Kc[2] - mpf(p[0])), float(a[1] / a[2] * Kc[1] + Kc[3] - mpf(p[1])))
    s.add("threshold_angle", "threshold", X0, cams, noise_px=0.0, offsets={2: off})
    h = 2.0 * math.tan(CAND_MIN_ANGLE / 2)
    s.add("threshold_parallax", "threshold", (0.0, 0.0, 2.0), [b.add_camera((0, 0, 0, 1), (-h, 0, 0), 0), b.add_camera((0, 0, 0, 1), (h, 0, 0), 1)], noise_px=0.0)
    # seeded random: 2..12 views, noise, outliers with probability 0.15, every fifth a false match, every seventh narrow
    rng = np.random.default_rng(77)
    for k in range(N_RANDOM):
        n = int(rng.integers(2, 13))
        cams = [b.add_camera_seeing(quat_mul(axis_quat((0, 0, 1), float(rng.uniform(-10, 10))), axis_quat((0, 1, 0), float(y))), X0,
                                    (float(rng.uniform(-1, 1)), float(rng.uniform(-1, 1)), float(rng.uniform(6, 14))), int(rng.integers(0, 2)))
                for y in rng.uniform(-50, 50, n) * (0.004 if k % 7 == 6 else 1.0)]
        X = [X0 + rng.uniform(-1, 1, 3) for _ in range(n)] if k % 5 == 4 else X0 + rng.uniform(-1, 1, 3)
        off = {i: (float(rng.uniform(40, 300)) * (-1) ** i, float(rng.uniform(40, 300))) for i in range(n) if rng.uniform() < 0.15}
        s.add(f"random{k}", "random", X, cams, noise_px=0.7, offsets=off)
    return s


def _split(a):
    """an mpf as two float64 (106 bits): what the golden file stores"""
    hi = float(a)
    return hi, float(a - mpf(hi))


@_hp
def walk_candidates(arr, which=None):
    """The exact walk of the candidates `which` (all by default) of `arr` (CandidateSet.arrays or the golden file) for both
    residual types.  Returns the arrays of the golden file."""
    cs = arr["cand_start"]
    which = range(len(cs) - 1) if which is None else which
    out = {f"{k}{rt}": [] for rt in (0, 1) for k in ("ok", "mask", "idx", "X", "A", "lam", "margin", "trials", "lo_rounds")}
    for c in which:
        sl = slice(int(cs[c]), int(cs[c + 1]))
        cand = ExactCandidate(arr["P"][sl], arr["K"][sl], arr["xy"][sl])
        mnt = int(arr["min_num_trials"][c])
        for rt in (0, 1):
            r = exact_loransac(cand, CAND_MIN_ANGLE, CAND_MAX_ERROR[rt], rt, None if mnt < 0 else mnt)
            m = r["model"]
            out[f"ok{rt}"].append(r["ok"])
            out[f"mask{rt}"].append(sum(1 << i for i, f in enumerate(r["mask"]) if f))
            out[f"idx{rt}"].append(sum(1 << i for i in m["idx"]) if m else 0)
            out[f"X{rt}"].append([_split(v) for v in m["X"]] if m else [(0.0, 0.0)] * 3)
            out[f"A{rt}"].append([_split(m["A"][i, j]) for i in range(4) for j in range(4)] if m else [(0.0, 0.0)] * 16)
            out[f"lam{rt}"].append([_split(v) for v in m["lam"]] if m else [(0.0, 0.0)] * 4)
            out[f"margin{rt}"].append(min(float(r["margin"]), 1e300))
            out[f"trials{rt}"].append(r["trials"])
            out[f"lo_rounds{rt}"].append(r["lo_rounds"])
    dt = dict(ok=bool, mask=np.uint64, idx=np.uint64, trials=np.int64, lo_rounds=np.int64)
    return {k: np.array(v, dt.get(k[:-1], np.float64)) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def candidate_golden():
    import pathlib

    with np.load(pathlib.Path(__file__).parent / "golden" / CAND_GOLDEN) as z:
        return {k: z[k] for k in z.files}


@_hp
def _golden_ref(g, rt, c):
    """triangulation_ratios' reference dict of candidate c from the golden arrays"""
    j = lambda a: mpf(float(a[0])) + mpf(float(a[1]))
    A = mp.matrix(4, 4)
    for i in range(16):
        A[i // 4, i % 4] = j(g[f"A{rt}"][c][i])
    lam = [j(v) for v in g[f"lam{rt}"][c]]
    X = [j(v) for v in g[f"X{rt}"][c]]
    fro, gap, nx = _fro(A), lam[1] - lam[0], _norm(X)
    return dict(A=A, fro=fro, lam=lam, X=X, gap=gap, fwd_unit=fro / gap * (1 + nx) * mp.sqrt(1 + nx * nx) if gap > 0 else None)


def candidate_launch(which):
    """The arrays of one launch over the golden candidates `which` (indices, repeats allowed)."""
    g = candidate_golden()
    cs = g["cand_start"]
    rows = np.concatenate([np.arange(cs[c], cs[c + 1]) for c in which] + [np.zeros(0, np.int64)]).astype(np.int64)
    start = np.concatenate([[0], np.cumsum([cs[c + 1] - cs[c] for c in which])]).astype(np.int64)
    return start, g["P"][rows], g["K"][rows], g["xy"][rows], g["min_num_trials"][list(which)]


def candidate_failures(batch, rt, which=None, stats=None, explicit_trials=False):
    """`batch(cand_start, P, K, xy, min_tri_angle, max_error, residual_type, min_num_trials) -> (xyz, ok, inlier)` on the
    golden candidates `which`.  Decided candidates: ok and the mask exact, the point within the backward criterion on the
    matrix of the exact index set and, where informative, the forward criterion; failed: zeros.  Open candidates (margin
    <= 1: the threshold group): ok = 0 with zeros, or ok = 1 with at least two inliers and a finite point.
    Returns (failures, open labels).  min_num_trials is passed as NULL unless a candidate of the launch sets one."""
    g = candidate_golden()
    which = list(range(len(g["labels"]))) if which is None else list(which)
    start, P, K, xy, mnt = candidate_launch(which)
    if (mnt >= 0).any() and (mnt < 0).any() and not explicit_trials:  # the library's own rule is on trial too: NULL where no candidate sets a value
        parts = [candidate_failures(batch, rt, [c for c, m in zip(which, mnt) if (m >= 0) == explicit], stats) for explicit in (False, True)]
        return parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]
    n_views = np.diff(start)
    trials = None
    if explicit_trials or (mnt >= 0).any():
        trials = np.where(mnt >= 0, mnt, [default_min_num_trials(int(n)) for n in n_views])
    xyz, ok, inl = batch(start, P, K, xy, CAND_MIN_ANGLE, CAND_MAX_ERROR[rt], rt, trials)
    fails, open_ = [], []
    for k, c in enumerate(which):
        lab, got = str(g["labels"][c]), inl[start[k]:start[k + 1]]
        what = f"{lab} (rt {rt}, launch slot {k})"
        if not ok[k] and (np.any(xyz[k] != 0) or got.any()):
            fails.append(f"{what}: failed but xyz {xyz[k]} / inliers {got.astype(int)} are not zeros")
        if ok[k] and not (got.sum() >= 2 and np.isfinite(xyz[k]).all()):
            fails.append(f"{what}: ok with {int(got.sum())} inliers, xyz {xyz[k]}")
        if not g[f"margin{rt}"][c] > 1.0:
            open_.append(lab)
            continue
        want = np.array([(int(g[f"mask{rt}"][c]) >> i) & 1 for i in range(int(n_views[k]))], bool)
        if bool(ok[k]) != bool(g[f"ok{rt}"][c]):
            fails.append(f"{what}: ok {bool(ok[k])}, exact {bool(g[f'ok{rt}'][c])} with margin {g[f'margin{rt}'][c]:.3g}")
            continue
        if not ok[k]:
            continue
        if not np.array_equal(got, want):
            fails.append(f"{what}: inliers {got.astype(int)} vs exact {want.astype(int)}")
        ref = _golden_ref(g, rt, c)
        (back, fwd), = triangulation_ratios([ref], xyz[k:k + 1])
        if stats is not None:
            stats.append((lab, "cand backward", back))
        if not back <= C_T:
            fails.append(f"{what}: backward ratio {back:.3g} > {C_T} on the exact index set {int(g[f'idx{rt}'][c]):#x}, xyz {xyz[k]}")
        if triangulation_informative(ref, C_T):
            if stats is not None:
                stats.append((lab, "cand forward", fwd))
            if not fwd <= C_T:
                fails.append(f"{what}: forward ratio {fwd:.3g} > {C_T}")
    return fails, open_


def restatement_batch(cand_start, P, K, xy, min_tri_angle, max_error, rt, min_num_trials=None, rule_n=15, reverse=False, drop_bit63=False):
    """oracle.track_graph_oracle.loransac_estimate with the signature of capi.tri_estimate_batch.  rule_n, reverse and
    drop_bit63 are the mutations that live in the caller: the n <= 15 rule moved, the pairs drawn in the reverse order,
    bit 63 of the mask lost."""
    from oracle import track_graph_oracle as TG

    nc = len(cand_start) - 1
    xyz, ok, inl = np.zeros((nc, 3)), np.zeros(nc, bool), np.zeros(len(P), bool)
    for c in range(nc):
        e0, e1 = int(cand_start[c]), int(cand_start[c + 1])
        views = []
        for e in range(e0, e1):
            Pm = np.asarray(P[e], np.float64).reshape(3, 4)
            views.append(TG.View(xy=xy[e], xn=(xy[e] - K[e, 2:]) / K[e, :2], P=Pm, C=-Pm[:, :3].T @ Pm[:, 3], K=K[e]))
        n = e1 - e0
        mnt = int(min_num_trials[c]) if min_num_trials is not None else (n * (n - 1) // 2 if n <= rule_n else 0)
        rep = TG.loransac_estimate(views[::-1] if reverse else views, TG.RansacOptions(max_error=max_error, min_tri_angle=min_tri_angle, residual_type=rt, min_num_trials=mnt))
        if rep.success:
            ok[c], xyz[c] = True, rep.model
            inl[e0:e1] = rep.inlier_mask[::-1] if reverse else rep.inlier_mask
            if drop_bit63 and n > 63:
                inl[e0 + 63] = False
    return xyz, ok, inl


# ---- init-pair case set and checks -----------------------------------------------------------------------------------
INIT_BLOCK_EDGES = (255, 256, 257)  # n_matches around the 256 threads of a k_init_candidates block
INIT_MAX_ERROR = math.radians(2.0)
INIT_TRIANGULATE, INIT_LIFT = 1, 2


@functools.lru_cache(maxsize=None)
def init_pair_cases():
    """One pair of cameras (image 1 at the identity) and its matches: dict(xy1, xy2, intr1, intr2, P2, prior_map, valid_map,
    sx, sy, select, groups).  The friendly matches come first: prefixes are the block-edge launches."""
    s = CandidateSet(seed=41)
    b = s.b
    c1 = b.add_camera((0, 0, 0, 1), (0, 0, 0), 0)
    c2 = b.add_camera(quat_mul(axis_quat((0, 0, 1), 2.0), axis_quat((0, 1, 0), -6.0)), (1.0, 0.05, 0.6), 1)
    rng = np.random.default_rng(42)
    xy1, xy2, groups = [], [], {}

    def match(group, X, noise=0.5, at=None):
        p1 = b.project(c1, X) if at is None else list(at)
        p2 = b.project(c2, X)
        groups.setdefault(group, []).append(len(xy1))
        xy1.append([p1[0] + noise * float(rng.standard_normal()), p1[1] + noise * float(rng.standard_normal())] if at is None else p1)
        xy2.append([p2[0] + noise * float(rng.standard_normal()), p2[1] + noise * float(rng.standard_normal())])

    for _ in range(INIT_BLOCK_EDGES[-1] + 3):
        z = float(rng.uniform(4, 12))
        match("friendly", [z * float(rng.uniform(-0.35, 0.35)), z * float(rng.uniform(-0.3, 0.3)), z])
    for z in (1e3, 1e5, 1e7, 1e9):  # low parallax: the acos argument of the reference's angle is 1 - 0.6 / z
        for k in range(3):
            match("low_parallax", [z * 0.1 * (k - 1), z * 0.07, z], noise=0.0)
    # image 1 pixels over the corner of the prior map that holds 3e15 .. 3e16: 1 - c = 0.6 / d is about eps there, and the
    # float64 evaluation of c lands on 1, below it or above it (NaN).  Four pixels of each kind, chosen by that evaluation.
    H, W = 24, 32
    yy, xx = np.mgrid[0:H, 0:W]
    prior = 7.0 + 2.0 * np.sin(0.37 * xx) + 1.5 * np.cos(0.29 * yy)
    prior[:5, :5] = 10.0 ** (15.5 + (xx[:5, :5] + yy[:5, :5]) / 8.0)
    prior[19:, 27:] = 0.3
    sx, sy = W / 1280.0, H / 960.0
    P2 = np.array(s._P(c2)).reshape(3, 4)
    at = np.array([(5.0 + 3.7 * i, 5.0 + 5.3 * j) for i in range(30) for j in range(20)])
    d = bilinear_at_kps(prior, at, sx, sy)
    K1 = b.intr[0]
    L = np.stack([(at[:, 0] - K1[2]) / K1[0] * d, (at[:, 1] - K1[3]) / K1[1] * d, d], 1)
    ang = np.array([numpy_ref_angle_deg(np.zeros(3), -P2[:, :3].T @ P2[:, 3], x) for x in L])
    for k in np.concatenate([np.flatnonzero(np.isnan(ang))[:4], np.flatnonzero(ang == 0)[:4], np.flatnonzero(ang > 0)[:4]]):
        match("lift_huge", [0.3 * (k % 7) - 1.0, 0.5, 8.0], at=at[k])
    for k in range(5):  # and over the corner that holds 0.3: in front of camera 1, behind camera 2 (its centre is at z = 0.6)
        match("lift_behind2", [0.1 * k, 0.1, 6.0], at=(1150.0 + 19.0 * k, 830.0 + 13.0 * k))
    for k in range(4):  # matches whose rays diverge: the triangulated point is behind the cameras
        X = [0.4 * k - 0.5, 0.3, -5.0 - k]
        match("tri_behind", X, noise=0.0)
    n = len(xy1)
    valid = np.ones((H, W), np.uint8)
    valid[10:13, 14:18] = 0
    select = np.ones(n, np.uint8)
    select[5::7] = 0
    return dict(xy1=np.array(xy1), xy2=np.array(xy2), intr1=b.intr[0], intr2=b.intr[1], P2=P2, prior_map=prior,
                valid_map=valid, sx=sx, sy=sy, select=select, groups=groups)


@functools.lru_cache(maxsize=None)
def _init_exact_tri(i, tri_min_angle):
    Z = init_pair_cases()
    P = np.stack([np.eye(3, 4), Z["P2"]]).reshape(2, 12)
    cand = ExactCandidate(P, np.stack([Z["intr1"], Z["intr2"]]), np.stack([Z["xy1"][i], Z["xy2"][i]]))
    return cand, exact_loransac(cand, tri_min_angle, INIT_MAX_ERROR, ANGULAR)


@_hp
def init_pair_failures(call, what, rescale=1.0, tri_min_angle=0.0, n_matches=None, use_select=False, stats=None):
    """`call(**kw) -> dict` with the keys of capi.init_pair_candidates.  The triangulated point against the exact two-view
    walk (flags exact where decided, the point by the candidates' rule); both angles, the four depth flags and the lift
    from the exact numbers at the kernel's own points and its own d_prior.  Returns (failures, open match indices)."""
    Z = init_pair_cases()
    n = len(Z["xy1"]) if n_matches is None else n_matches
    sel = Z["select"][:n] if use_select else None
    o = call(xy1=Z["xy1"][:n], xy2=Z["xy2"][:n], intr1=Z["intr1"], intr2=Z["intr2"], cam2_from_cam1=Z["P2"], prior_map=Z["prior_map"],
             valid_map=Z["valid_map"], sx=Z["sx"], sy=Z["sy"], rescale=rescale, select=sel, what=what, tri_min_angle=tri_min_angle,
             tri_max_error=INIT_MAX_ERROR)
    group_of = {i: g for g, idx in Z["groups"].items() for i in idx}
    fails, open_ = [], []
    keys = ("tri_ok", "tri_posdepth1", "tri_posdepth2", "valid", "lift_posdepth1", "lift_posdepth2", "tri_xyz", "tri_angle_deg", "lift_xyz", "lift_angle_deg", "d_prior")

    def stat(i, kind, v):
        if stats is not None:
            stats.append((group_of[i], kind, v))

    def at_point(i, X, ang, f1, f2, name):
        """the reference's angle and the two depth flags at the fp64 point X"""
        cand = _init_exact_tri(i, 0.0)[0]
        r = ref_angle_ratio(cand.views[0].C, cand.views[1].C, X, ang)
        stat(i, "ref angle", r)
        if not r <= C_RA:
            fails.append(f"match {i} ({group_of[i]}) {name}_angle_deg {ang!r} at {X}: ratio {r:.3g} > {C_RA}")
        for v, f in zip(cand.views, (f1, f2)):
            z, mag, _ = depth_numbers(v, _vec(X))
            if _ratio(abs(z - mpf(EPS)), C_Z * mpf(EPS) * mag) > 1 and bool(f) != bool(z >= mpf(EPS)):
                fails.append(f"match {i} ({group_of[i]}) {name} depth flag {bool(f)} at zc = {float(z)!r}")

    for i in range(n):
        tri_zero = all(not np.any(o[k][i]) for k in keys[:3] + ("tri_xyz", "tri_angle_deg"))
        lift_zero = all(not np.any(o[k][i]) for k in keys[3:6] + ("lift_xyz", "lift_angle_deg", "d_prior"))
        if sel is not None and not sel[i]:
            if not (tri_zero and lift_zero):
                fails.append(f"match {i}: skipped but not all zeros")
            continue
        if not what & INIT_TRIANGULATE:
            if not tri_zero:
                fails.append(f"match {i}: triangulation not asked for but not zeros")
        else:
            _, r = _init_exact_tri(i, float(tri_min_angle))
            ok = bool(o["tri_ok"][i])
            if not ok and not tri_zero:
                fails.append(f"match {i} ({group_of[i]}): no triangulation but not zeros")
            if r["margin"] > 1 and ok != r["ok"]:
                fails.append(f"match {i} ({group_of[i]}): tri_ok {ok}, exact {r['ok']} with margin {float(r['margin']):.3g}")
            elif not r["margin"] > 1:
                open_.append(i)
            if ok:
                X = o["tri_xyz"][i]
                if r["ok"]:  # one pair, one model: the matrix is the same whatever the decision
                    (back, fwd), = triangulation_ratios([r["model"]], X[None])
                    stat(i, "init backward", back)
                    if not back <= C_T:
                        fails.append(f"match {i} ({group_of[i]}): tri_xyz {X} backward ratio {back:.3g} > {C_T}")
                    if triangulation_informative(r["model"], C_T):
                        stat(i, "init forward", fwd)
                        if not fwd <= C_T:
                            fails.append(f"match {i} ({group_of[i]}): tri_xyz {X} forward ratio {fwd:.3g} > {C_T}")
                at_point(i, X, o["tri_angle_deg"][i], o["tri_posdepth1"][i], o["tri_posdepth2"][i], "tri")
        if not what & INIT_LIFT:
            if not lift_zero:
                fails.append(f"match {i}: lift not asked for but not zeros")
        else:
            L = o["lift_xyz"][i]
            lr = lift_ratio(Z["xy1"][i], Z["intr1"], o["d_prior"][i], rescale, L)
            stat(i, "lift", lr)
            if not lr <= C_L:
                fails.append(f"match {i} ({group_of[i]}): lift_xyz {L} from d_prior {o['d_prior'][i]!r}: ratio {lr:.3g} > {C_L}")
            at_point(i, L, o["lift_angle_deg"][i], o["lift_posdepth1"][i], o["lift_posdepth2"][i], "lift")
    return fails, open_


# ---- the constants' table --------------------------------------------------------------------------------------------
@_hp
def candidate_numpy_ratios(restatement=False):
    """Ratios error / (eps x form) of plain NumPy float64 (or, for information, of the restatements in oracle/ and
    tests/numpy_registration.py) for the forms of the candidate and init-pair checks, over exactly their cases."""
    from oracle import track_graph_oracle as TG
    import numpy_registration as NR

    g = candidate_golden()
    st = []
    cs = g["cand_start"]
    for c in range(len(cs) - 1):
        sl = slice(int(cs[c]), int(cs[c + 1]))
        P, K, xy = g["P"][sl], g["K"][sl], g["xy"][sl]
        views = exact_views(P, K, xy)
        for rt in (0, 1):
            if not g[f"ok{rt}"][c]:
                continue
            idx = [i for i in range(len(views)) if int(g[f"idx{rt}"][c]) >> i & 1]
            Pm = P.reshape(-1, 3, 4)
            xn = (xy - K[:, 2:]) / K[:, :2]
            if restatement:
                X = TG.triangulate_point(Pm[idx[0]], Pm[idx[1]], xn[idx[0]], xn[idx[1]]) if len(idx) == 2 else TG.triangulate_multi_view_point(Pm[idx], xn[idx])
            else:
                X = numpy_model(P, K, xy, idx)
            ref = _golden_ref(g, rt, c)
            (back, fwd), = triangulation_ratios([ref], X[None])
            kind = "two-view" if len(idx) == 2 else "multi-view"
            st.append((c, f"{kind} backward", back))
            if triangulation_informative(ref, C_T):
                st.append((c, f"{kind} forward", fwd))
            if rt == 1:
                continue
            Xm = _vec(X)
            for i, v in enumerate(views):
                z, mag, _ = depth_numbers(v, Xm)
                st.append((c, "depth", float(abs(mpf(float(numpy_depth(P[i], X))) - z) / (mpf(EPS) * mag))))
                e, form, _, _ = angular_numbers(v, Xm)
                got = TG.calculate_normalized_angular_error(xn[i], X, Pm[i]) if restatement else numpy_angular(P[i], K[i], xy[i], X)
                st.append((c, "angular residual", float(abs(mpf(float(got)) - e) / (mpf(EPS) * form))))
                if z >= mpf(EPS):
                    err, s, _, _ = reprojection_numbers(v, Xm)
                    got = TG.calculate_squared_reprojection_error(xy[i], X, P[i].reshape(3, 4), K[i]) if restatement else numpy_reprojection(P[i], K[i], xy[i], X)
                    st.append((c, "sq reprojection", float(abs(mpf(float(got)) - err) / (mpf(EPS) * (err + s)))))
    for n in range(2, 65):
        for k in range(1, n):
            v, form = _num_trials_value(k, n, 0.9999)
            got = math.log(1.0 - 0.9999) / math.log(1.0 - (k / float(n)) ** 2) * 3.0 if restatement else numpy_num_trials(k, n)
            st.append((n, "stop rule", float(abs(mpf(float(got)) - v) / (mpf(EPS) * form))))
    Z = init_pair_cases()
    o = NR.init_pair_candidates(xy1=Z["xy1"], xy2=Z["xy2"], intr1=Z["intr1"], intr2=Z["intr2"], cam2_from_cam1=Z["P2"], prior_map=Z["prior_map"],
                                valid_map=Z["valid_map"], sx=Z["sx"], sy=Z["sy"], rescale=0.437, tri_max_error=INIT_MAX_ERROR)
    C1, C2 = np.zeros(3), -Z["P2"][:, :3].T @ Z["P2"][:, 3]
    K1 = Z["intr1"]
    for i in range(len(Z["xy1"])):
        for X in ([o["tri_xyz"][i]] if o["tri_ok"][i] else []) + [o["lift_xyz"][i]]:
            got = NR.reference_angle_deg(C1, C2, X)[0][0] if restatement else numpy_ref_angle_deg(C1, C2, X)
            st.append((i, "ref angle", ref_angle_ratio(_vec(C1), _vec(C2), X, got)))
        ds = o["d_prior"][i] * 0.437
        L = o["lift_xyz"][i] if restatement else np.array([(Z["xy1"][i, 0] - K1[2]) / K1[0] * ds, (Z["xy1"][i, 1] - K1[3]) / K1[1] * ds, ds])
        st.append((i, "lift", lift_ratio(Z["xy1"][i], K1, o["d_prior"][i], 0.437, L)))
    return st


def _largest(stats):
    top = {}
    for _, kind, v in stats:
        if v is not None and math.isfinite(v):
            top[kind] = max(top.get(kind, 0.0), v)
    return top


if __name__ == "__main__":  # the table of measured ratios: NumPy (sets the constants) and the C oracle (for information)
    from oracle import cpu_oracle as O

    rows = {}
    for name, impl in (("numpy", (numpy_triangulate, numpy_filter, numpy_point_covs)), ("oracle", (O.triangulate_tracks, O.filter_tracks, O.point_covs))):
        st = []
        bad = {k: v for k, v in all_failures(*impl, stats=st).items() if v}
        rows[name] = _largest(st)
        print(name, rows[name], "failures:", bad)
    for kind, top in rows["numpy"].items():
        print(f"{kind:9s} numpy {top:8.3g}  oracle {rows['oracle'][kind]:8.3g}  constant {2.0 ** math.ceil(math.log2(8 * top)):g}")
    # candidates and init pair: NumPy (sets the constants) and the restatements (for information)
    cand = {name: _largest(candidate_numpy_ratios(restatement=r)) for name, r in (("numpy", False), ("restatement", True))}
    for kind, top in cand["numpy"].items():
        print(f"{kind:20s} numpy {top:8.3g}  restatement {cand['restatement'].get(kind, float('nan')):8.3g}  constant {2.0 ** math.ceil(math.log2(8 * top)):g}")
