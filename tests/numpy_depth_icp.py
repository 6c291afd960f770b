"""numpy_depth_icp.py — TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The dense point-to-plane ICP of csrc/depth_icp.hip restated in NumPy, rule by rule as include/mpsfm_hip.h (mpsfm_depth_pair_icp)
states them: every per-pixel expression in float64 with the association of csrc/icp_math.h, but the sums over pixels in long
double, so they are the reference the device's fixed-order float64 reduction is measured against.  The 6 x 6 step runs in
Python floats on the rounded sums.  Every call reports the decisions that a rounding error could flip (`fragile`)."""

import math

import numpy as np

DEFAULTS = dict(max_distance=0.1, max_angle_deg=30.0, edge_ratio=0.05, eps_rotation=1e-6, eps_translation=1e-6, max_iterations=30,
                min_pairs=100, stride=1)
STATUS = ("converged", "max_iterations", "too_few_pairs", "singular")
MIN_PIVOT, SMALL_ANGLE = 1e-10, 1e-12
NEAR = 1e-9  # a decision closer than this to its threshold is fragile
REJECT_CAUSES = ("outside", "no_target_normal", "distance", "angle")


def vertex_map(depth, intr):
    """V [H, W, 3] = (((c - cx) z) / fx, ((r - cy) z) / fy, z) and ok [H, W]: z finite and > 0."""
    fx, fy, cx, cy = (float(v) for v in intr)
    z = np.asarray(depth, np.float64)
    H, W = z.shape
    r, c = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        V = np.stack([((c - cx) * z) / fx, ((r - cy) * z) / fy, z], -1)
        ok = np.isfinite(z) & (z > 0.0)
    return V, ok


def normal_map(depth, intr, edge_ratio):
    """(normals [H, W, 3], valid [H, W], fragile): camera-facing unit normals by central differences; zeros where invalid."""
    z = np.asarray(depth, np.float64)
    H, W = z.shape
    V, ok = vertex_map(z, intr)
    normals, valid, fragile = np.zeros((H, W, 3)), np.zeros((H, W), bool), []
    if H < 3 or W < 3:
        return normals, valid, fragile
    ctr = (slice(1, H - 1), slice(1, W - 1))
    nbs = [(slice(1, H - 1), slice(0, W - 2)), (slice(1, H - 1), slice(2, W)), (slice(0, H - 2), slice(1, W - 1)), (slice(2, H), slice(1, W - 1))]
    with np.errstate(all="ignore"):
        good = ok[ctr].copy()
        for nb in nbs:
            good &= ok[nb]
        edge = edge_ratio * z[ctr]
        for nb in nbs:
            gap = np.abs(z[nb] - z[ctr])
            if (good & (np.abs(gap - edge) < NEAR)).any():
                fragile.append("edge rule")
            good &= gap <= edge
        a, b = V[nbs[1]] - V[nbs[0]], V[nbs[3]] - V[nbs[2]]
        m = np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                      a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)
        mm = m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1] + m[..., 2] * m[..., 2]
        good &= np.isfinite(mm) & (mm > 0.0)
        u = m / np.sqrt(mm)[..., None]
        d = u[..., 0] * V[ctr][..., 0] + u[..., 1] * V[ctr][..., 1] + u[..., 2] * V[ctr][..., 2]
        if (good & (np.abs(d) < NEAR)).any():
            fragile.append("n.V")
        good &= (d < 0.0) | (d > 0.0)
        n = np.where((d > 0.0)[..., None], -1.0, 1.0) * u
    normals[ctr] = np.where(good[..., None], n, 0.0)
    valid[ctr] = good
    return normals, valid, fragile


class Maps:
    """Both maps of a pair with their vertex and normal maps, formed once."""

    def __init__(self, depth0, intr0, depth1, intr1, edge_ratio):
        self.intr1 = tuple(float(v) for v in intr1)
        self.V0, _ = vertex_map(depth0, intr0)
        self.V1, _ = vertex_map(depth1, intr1)
        self.n0, self.valid0, f0 = normal_map(depth0, intr0, edge_ratio)
        self.n1, self.valid1, f1 = normal_map(depth1, intr1, edge_ratio)
        self.fragile = f0 + f1
        self.H1, self.W1 = self.valid1.shape

    def source(self, stride):
        """(p [n, 3], n0 [n, 3]) of the source set in row-major pixel order."""
        H, W = self.valid0.shape
        sel = np.zeros((H, W), bool)
        sel[::stride, ::stride] = True
        sel &= self.valid0
        return self.V0[sel], self.n0[sel]


def linearise(maps, T, scale, stride, max_distance, min_cos):
    """One linearisation at T [3, 4]: dict(A [6, 6], b [6], rr, count, rejected [4], fragile); sums in long double, rounded once."""
    fx, fy, cx, cy = maps.intr1
    p, n0 = maps.source(stride)
    fragile = []
    rejected = [0, 0, 0, 0]
    with np.errstate(all="ignore"):
        x = np.stack([scale * (T[k, 0] * p[:, 0] + T[k, 1] * p[:, 1] + T[k, 2] * p[:, 2]) + T[k, 3] for k in range(3)], -1)
        if (np.abs(x[:, 2]) < NEAR).any():
            fragile.append("p'_z")
        front = x[:, 2] > 0.0
        u, v = (x[:, 0] / x[:, 2]) * fx + cx, (x[:, 1] / x[:, 2]) * fy + cy
        cf, rf = np.floor(u + 0.5), np.floor(v + 0.5)
        inside = front & (cf >= 0.0) & (cf <= maps.W1 - 1.0) & (rf >= 0.0) & (rf <= maps.H1 - 1.0)
        # a rounding on the fence between two pixels, for a pixel inside the map or within a pixel of it
        about = front & (cf >= -1.0) & (cf <= maps.W1) & (rf >= -1.0) & (rf <= maps.H1)
        if (about & ((np.abs(u + 0.5 - np.rint(u + 0.5)) < NEAR) | (np.abs(v + 0.5 - np.rint(v + 0.5)) < NEAR))).any():
            fragile.append("pixel rounding")
    rejected[0] = int((~inside).sum())
    x, n0 = x[inside], n0[inside]
    ri, ci = rf[inside].astype(np.int64), cf[inside].astype(np.int64)
    has = maps.valid1[ri, ci]
    rejected[1] = int((~has).sum())
    x, n0, ri, ci = x[has], n0[has], ri[has], ci[has]
    q, n1 = maps.V1[ri, ci], maps.n1[ri, ci]
    d = x - q
    d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    max_d2 = max_distance * max_distance
    if (np.abs(d2 - max_d2) < NEAR).any():
        fragile.append("distance gate")
    near = d2 <= max_d2
    rejected[2] = int((~near).sum())
    x, n0, n1, d = x[near], n0[near], n1[near], d[near]
    c = np.zeros(len(x))
    for k in range(3):
        c = c + (T[k, 0] * n0[:, 0] + T[k, 1] * n0[:, 1] + T[k, 2] * n0[:, 2]) * n1[:, k]
    if (np.abs(c - min_cos) < NEAR).any():
        fragile.append("angle gate")
    facing = c >= min_cos
    rejected[3] = int((~facing).sum())
    x, n1, d = x[facing], n1[facing], d[facing]
    res = n1[:, 0] * d[:, 0] + n1[:, 1] * d[:, 1] + n1[:, 2] * d[:, 2]
    J = np.stack([x[:, 1] * n1[:, 2] - x[:, 2] * n1[:, 1], x[:, 2] * n1[:, 0] - x[:, 0] * n1[:, 2], x[:, 0] * n1[:, 1] - x[:, 1] * n1[:, 0],
                  n1[:, 0], n1[:, 1], n1[:, 2]], -1)
    A, b = np.zeros((6, 6)), np.zeros(6)
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = float((J[:, i] * J[:, j]).astype(np.longdouble).sum())
        b[i] = -float((J[:, i] * res).astype(np.longdouble).sum())
    rr = float((res * res).astype(np.longdouble).sum())
    return dict(A=A, b=b, rr=rr, count=len(x), rejected=rejected, fragile=fragile)


def solve(A, b):
    """(xi or None, smallest pivot of the scaled matrix or None): Cholesky without pivoting of D^-1 A D^-1, D = sqrt(diag A)."""
    if not all(A[i, i] > 0.0 for i in range(6)):
        return None, None
    d = [math.sqrt(A[i, i]) for i in range(6)]
    L = [[0.0] * 6 for _ in range(6)]
    low = math.inf
    for j in range(6):
        s = A[j, j] / (d[j] * d[j])
        for k in range(j):
            s -= L[j][k] * L[j][k]
        low = min(low, s)
        if not s > MIN_PIVOT:
            return None, low
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, 6):
            e = A[i, j] / (d[i] * d[j])
            for k in range(j):
                e -= L[i][k] * L[j][k]
            L[i][j] = e / L[j][j]
    y, xi = [0.0] * 6, [0.0] * 6
    for i in range(6):
        s = b[i] / d[i]
        for k in range(i):
            s -= L[i][k] * y[k]
        y[i] = s / L[i][i]
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s -= L[k][i] * xi[k]
        xi[i] = s / L[i][i]
    return np.array([xi[i] / d[i] for i in range(6)]), low


def apply(xi, T):
    """(exp(xi) T, |w|, |v|): R <- exp(w) R, t <- exp(w) t + v."""
    w = [float(v) for v in xi[:3]]
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    th = math.sqrt(th2)
    Kx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    a, b = 1.0, 0.0
    if not th < SMALL_ANGLE:
        sh = math.sin(0.5 * th)
        a, b = math.sin(th) / th, (2.0 * (sh * sh)) / th2
    E = np.eye(3) + a * Kx + b * (np.outer(w, w) - th2 * np.eye(3))
    out = np.zeros((3, 4))
    for i in range(3):
        for j in range(4):
            out[i, j] = E[i, 0] * T[0, j] + E[i, 1] * T[1, j] + E[i, 2] * T[2, j]
        out[i, 3] += xi[3 + i]
    return out, th, math.sqrt(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5])


def icp(depth0, intr0, depth1, intr1, init, scale=1.0, **options):
    """The loop.  dict(tgt_from_src [3, 4], scale, status, iterations, num_pairs, rejected, rmse, info, rhs, trace [iterations, 4],
    counts, rejections (per iteration), condition (of the last scaled system solved), fragile)."""
    o = dict(DEFAULTS)
    assert not set(options) - set(o), options
    o.update(options)
    maps = Maps(depth0, intr0, depth1, intr1, o["edge_ratio"])
    min_cos = math.cos(o["max_angle_deg"] * (math.pi / 180.0))
    T = np.array(init, np.float64).reshape(3, 4)
    fragile, trace, counts, rejections = list(maps.fragile), [], [], []
    status, lin, condition = None, None, None
    for it in range(o["max_iterations"]):
        lin = linearise(maps, T, float(scale), o["stride"], o["max_distance"], min_cos)
        fragile += [f"{f} (iteration {it})" for f in lin["fragile"]]
        count = lin["count"]
        rmse = math.sqrt(lin["rr"] / count) if count > 0 else 0.0
        counts.append(count)
        rejections.append(list(lin["rejected"]))
        if abs(count - o["min_pairs"]) <= 2:
            fragile.append(f"pair count {count} (iteration {it})")
        if count < o["min_pairs"]:
            status = "too_few_pairs"
            trace.append([count, rmse, 0.0, 0.0])
            break
        xi, pivot = solve(lin["A"], lin["b"])
        if pivot is not None and MIN_PIVOT / 100.0 < pivot < MIN_PIVOT * 100.0:
            fragile.append(f"pivot {pivot:.3g} (iteration {it})")
        if xi is None:
            status = "singular"
            trace.append([count, rmse, 0.0, 0.0])
            break
        dd = np.sqrt(np.diag(lin["A"]))
        condition = float(np.linalg.cond(lin["A"] / np.outer(dd, dd)))
        T, nw, nv = apply(xi, T)
        trace.append([count, rmse, nw, nv])
        for norm, eps, what in ((nw, o["eps_rotation"], "|w|"), (nv, o["eps_translation"], "|v|")):
            if eps / 10.0 < norm < eps * 10.0:
                fragile.append(f"{what} = {norm:.3g} near its eps (iteration {it})")
        if nw <= o["eps_rotation"] and nv <= o["eps_translation"]:
            status = "converged"
            break
    if status is None:
        status = "max_iterations"
    count = lin["count"]
    return dict(tgt_from_src=T, scale=float(scale), status=status, iterations=len(trace), num_pairs=count, rejected=list(lin["rejected"]),
                rmse=math.sqrt(lin["rr"] / count) if count > 0 else 0.0, info=lin["A"], rhs=lin["b"], trace=np.array(trace).reshape(-1, 4),
                counts=counts, rejections=rejections, condition=condition, fragile=fragile)
