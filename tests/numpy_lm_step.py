"""One Levenberg-Marquardt step of the bundle adjustment behind a GIVEN camera step, restated in plain NumPy: the reference of
tests/test_gpu_update_once.py (the update sweep of csrc/sweep_update_body.h and csrc/ba_kernels.hip through
mpsfm_debug_update_once) and of tests/test_lm_step_cpu.py.  Written from the formulas, not from the kernels or oracle/ba_oracle.c:

  camera-frame point   P = R(q) X + t, Y = R(q) X;  q = (x, y, z, w)
  reprojection block   r = (fx Px / Pz + cx - u, fy Py / Pz + cy - v);  valid when finite
  log-depth block      r = log Pz - log(d exp(s) + b), (b, s) = shift_logscale of the camera (0, 0 without);  valid when Pz > 0
  Jacobians            dr/dP = a (one row per residual);  d/dX: a R;  d/dt: a;  d/dtheta: 2 (Y x a), for q [+] d = exp(d) * q with
                       exp(d) = (sin|d| d / |d|, cos|d|) (no factor 1/2: a rotation by 2 |d|)
  robust weight        w = sqrt(magnitude rho'(s)), s = |r|^2; r and both Jacobians are multiplied by w (rho'' <= 0 for all three
                       losses, so the corrector has no second-order term).  trivial: rho = s; soft-L1: rho = 2 a^2 (sqrt(1 + s / a^2) - 1) = 2 s / (sqrt(1 + s / a^2) + 1),
                       rho' = 1 / sqrt(1 + s / a^2); Cauchy: rho = a^2 log(1 + s / a^2), rho' = 1 / (1 + s / a^2); rho' >= DBL_MIN
  scaling              Jc .* cs (6 per camera, 0: a constant coordinate), Jp .* ps (3 per landmark, 0: a constant landmark)
  per variable landmark  V = sum Jp^T Jp, g = sum Jp^T (r + Jc yc), D = clamp(diag V, lo, hi) / radius, yp = -(V + D)^-1 g, X2 = X + ps .* yp
  model cost change    -sum m (r + m / 2), m = Jc yc + Jp yp, over the blocks valid at the linearisation point
  cost                 sum 1/2 magnitude rho(s) over the blocks of the reduced program (a block of a constant camera AND a constant
                       landmark is not part of it)

Every array is computed in `dtype`: np.longdouble for the reference, np.float64 for the yardstick that the bounds of the GPU test are
multiples of.  Sums run in block order (reprojection blocks, then depth blocks), one after the other."""

import numpy as np

LD = np.longdouble
DBL_MIN = np.finfo(np.float64).tiny
TRIVIAL, SOFT_L1, CAUCHY = 0, 1, 2


def loss(kind, a, s, dtype=LD):
    """rho(s) and rho'(s) of loss `kind` (scalar or array per element) with scale a."""
    a, s = np.asarray(a, dtype), np.asarray(s, dtype)
    kind = np.broadcast_to(np.asarray(kind), s.shape)
    with np.errstate(all="ignore"):
        z = s / (a * a)
        rho = np.where(kind == SOFT_L1, 2 * s / (np.sqrt(1 + z) + 1), np.where(kind == CAUCHY, a * a * np.log1p(z), s))
        rho1 = np.where(kind == SOFT_L1, 1 / np.sqrt(1 + z), np.where(kind == CAUCHY, 1 / (1 + z), np.ones_like(s)))
    return rho, np.maximum(rho1, dtype(DBL_MIN))


def rotation(q, dtype=LD):
    x, y, z, w = (np.asarray(q, dtype)[..., k] for k in range(4))
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def quat_plus(q, d, dtype=LD):
    """exp(d) * q (Hamilton product, xyzw), rows of q [n, 4] and d [n, 3]."""
    q, d = np.asarray(q, dtype), np.asarray(d, dtype)
    n = np.sqrt((d * d).sum(-1))
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(n == 0, dtype(1), np.sin(n) / n)
    px, py, pz, pw = s * d[..., 0], s * d[..., 1], s * d[..., 2], np.cos(n)
    qx, qy, qz, qw = (q[..., k] for k in range(4))
    out = np.stack([pw * qx + px * qw + py * qz - pz * qy, pw * qy - px * qz + py * qw + pz * qx,
                    pw * qz + px * qy - py * qx + pz * qw, pw * qw - px * qx - py * qy - pz * qz], -1)
    return np.where((n == 0)[..., None], q, out)


class Layout:
    """Which cameras and landmarks are variables, and the blocks of the reduced program: reprojection blocks first, then depth blocks."""

    def __init__(self, prob):
        nc, npt = prob.n_cams, prob.n_pts
        cam = np.concatenate([prob.obs_cam, prob.dobs_cam]).astype(np.int64)
        pt = np.concatenate([prob.obs_pt, prob.dobs_pt]).astype(np.int64)
        kind = np.concatenate([np.zeros(prob.n_obs, np.int64), np.ones(prob.n_dobs, np.int64)])
        src = np.concatenate([np.arange(prob.n_obs), np.arange(prob.n_dobs)])
        self.cam_var = (prob.pose_const == 0) & (np.bincount(cam, minlength=nc) > 0)
        fixed = ~self.cam_var[cam] & (prob.pt_const[pt] != 0)
        self.fixed = dict(cam=cam[fixed], pt=pt[fixed], kind=kind[fixed], src=src[fixed])
        self.cam, self.pt, self.kind, self.src = cam[~fixed], pt[~fixed], kind[~fixed], src[~fixed]
        self.pvar = (prob.pt_const == 0) & (np.bincount(self.pt, minlength=npt) > 0)
        self.n_blocks = int(self.cam.size)


def residual_rows(prob, blk, q, t, pts, dtype=LD):
    """The blocks `blk` (cam, pt, kind, src) at the state (q, t, pts), raw: r [nb, 2] (second row of a depth block zero), a = dr/dP
    [nb, 2, 3], Y = R X [nb, 3], R per block, valid [nb], rows [nb, 2] (which rows exist), and per block the loss type, scale and
    magnitude."""
    cam, pt, kind, src = blk["cam"], blk["pt"], blk["kind"], blk["src"]
    q, t, pts = np.asarray(q, dtype), np.asarray(t, dtype), np.asarray(pts, dtype)
    rep = kind == 0
    nb = cam.size
    Rb = rotation(q, dtype)[cam]
    Y = np.einsum("bij,bj->bi", Rb, pts[pt])
    P = Y + t[cam]
    K = np.asarray(prob.cam_intr, dtype)[prob.cam_intr_idx[cam]]
    uv, dep, a_d, m_d = np.zeros((nb, 2), dtype), np.ones(nb, dtype), np.ones(nb, dtype), np.zeros(nb, dtype)
    uv[rep] = np.asarray(prob.obs_xy, dtype)[src[rep]]
    sd, cd = src[~rep], cam[~rep]
    d_eff = np.asarray(prob.dobs_depth, dtype)[sd]
    if prob.shift_logscale is not None:
        sl = np.asarray(prob.shift_logscale, dtype)
        d_eff = d_eff * np.exp(sl[cd, 1]) + sl[cd, 0]
    dep[~rep] = d_eff
    a_d[~rep] = np.asarray(prob.dobs_param, dtype)[sd]
    m_d[~rep] = np.asarray(prob.dobs_magnitude, dtype)[sd]
    zero = np.zeros(nb, dtype)
    with np.errstate(all="ignore"):
        iz = 1 / P[:, 2]
        r_rep = np.stack([K[:, 0] * P[:, 0] * iz + K[:, 2] - uv[:, 0], K[:, 1] * P[:, 1] * iz + K[:, 3] - uv[:, 1]], -1)
        a_rep = np.stack([np.stack([K[:, 0] * iz, zero, -K[:, 0] * P[:, 0] * iz * iz], -1),
                          np.stack([zero, K[:, 1] * iz, -K[:, 1] * P[:, 1] * iz * iz], -1)], -2)
        r_dep = np.stack([np.log(P[:, 2]) - np.log(dep), zero], -1)
        a_dep = np.stack([np.stack([zero, zero, iz], -1), np.zeros((nb, 3), dtype)], -2)
    r = np.where(rep[:, None], r_rep, r_dep)
    a = np.where(rep[:, None, None], a_rep, a_dep)
    with np.errstate(all="ignore"):  # the terms a residual is the difference of: what its rounding is relative to
        t_rep = np.stack([np.abs(K[:, 0] * P[:, 0] * iz) + np.abs(K[:, 2]) + np.abs(uv[:, 0]), np.abs(K[:, 1] * P[:, 1] * iz) + np.abs(K[:, 3]) + np.abs(uv[:, 1])], -1)
        t_dep = np.stack([np.abs(np.log(P[:, 2])) + np.abs(np.log(dep)) + 1, zero], -1)
    r_terms = np.where(rep[:, None], t_rep, t_dep)
    valid = np.where(rep, np.isfinite(r_rep).all(-1), (P[:, 2] > 0) & (dep > 0) & np.isfinite(r_dep[:, 0]))
    rows = np.stack([np.ones(nb, bool), rep], -1) & valid[:, None]
    r = np.where(rows, r, 0)
    a = np.where(rows[:, :, None], a, 0)
    ltype = np.where(rep, prob.reproj_loss_type, prob.depth_loss_type)
    lscale = np.where(rep, dtype(prob.reproj_loss_scale), a_d)
    lmag = np.where(rep, dtype(prob.reproj_loss_magnitude), m_d)
    r_terms = np.where(rows, r_terms, 0)
    return dict(r=r, r_terms=r_terms, a=a, Y=Y, R=Rb, Z=P[:, 2], valid=valid, rows=rows, ltype=ltype, lscale=lscale, lmag=lmag)


def block_costs(prob, blk, q, t, pts, dtype=LD):
    """(cost of every block, valid): 1/2 magnitude rho(|r|^2), 0 where the block cannot be evaluated."""
    rr = residual_rows(prob, blk, q, t, pts, dtype)
    rho, _ = loss(rr["ltype"], rr["lscale"], (rr["r"] ** 2).sum(-1), dtype)
    return np.where(rr["valid"], rr["lmag"] * rho / 2, 0), rr["valid"]


def linearize(prob, L, q, t, pts, cs, ps, dtype=LD):
    """Robustified, scaled residual rows and Jacobians of the reduced program's blocks: r [nb, 2], Jc [nb, 2, 6], Jp [nb, 2, 3], the
    squared norms s, the weights w, cost per block and valid."""
    blk = dict(cam=L.cam, pt=L.pt, kind=L.kind, src=L.src)
    rr = residual_rows(prob, blk, q, t, pts, dtype)
    cs, ps = np.asarray(cs, dtype), np.asarray(ps, dtype)
    s = (rr["r"] ** 2).sum(-1)
    rho, rho1 = loss(rr["ltype"], rr["lscale"], s, dtype)
    w = np.sqrt(rr["lmag"] * rho1)
    a = rr["a"]
    Jc = np.concatenate([2 * np.cross(rr["Y"][:, None, :], a), a], -1) * w[:, None, None] * cs[L.cam][:, None, :]
    Jp = np.einsum("bri,bij->brj", a, rr["R"]) * w[:, None, None] * ps[L.pt][:, None, :]
    # the same products with every term in absolute value (|R| <= 1 entry by entry): what a rounding of the entries is relative to
    aa, Ya = np.abs(a), np.abs(rr["Y"])[:, None, :]
    cross = np.stack([Ya[..., 1] * aa[..., 2] + Ya[..., 2] * aa[..., 1], Ya[..., 2] * aa[..., 0] + Ya[..., 0] * aa[..., 2],
                      Ya[..., 0] * aa[..., 1] + Ya[..., 1] * aa[..., 0]], -1)
    Jc_abs = np.concatenate([2 * cross, aa], -1) * w[:, None, None] * cs[L.cam][:, None, :]
    Jp_abs = aa.sum(-1)[:, :, None] * np.ones(3, dtype) * w[:, None, None] * ps[L.pt][:, None, :]
    # relative change of the weight per unit relative rounding of the residual's terms: w = sqrt(mag rho'), rho' = (1 + z)^-1 (Cauchy)
    # or (1 + z)^-1/2 (soft-L1) with z = |r|^2 / a^2, so |dw / w| <= k sum |r_i| |dr_i| / (a^2 (1 + z)), k = 1 or 1/2
    with np.errstate(all="ignore"):
        k = np.where(rr["ltype"] == CAUCHY, 1.0, np.where(rr["ltype"] == SOFT_L1, 0.5, 0.0)).astype(dtype)
        w_sens = k * (np.abs(rr["r"]) * rr["r_terms"]).sum(-1) / (rr["lscale"] ** 2 + s)
    return dict(r=rr["r"] * w[:, None], Jc=Jc, Jp=Jp, Jc_abs=Jc_abs, Jp_abs=Jp_abs, w_sens=np.where(rr["valid"], w_sens, 0), s=s, w=w, rho1=rho1, lscale=rr["lscale"], cost=np.where(rr["valid"], rr["lmag"] * rho / 2, 0),
                valid=rr["valid"], rows=rr["rows"], Z=rr["Z"])


def solve_spd3(M, b, dtype=LD):
    """x = M^-1 b by an L L^T factorisation, per row of M [n, 3, 3], b [n, 3]; ok: every pivot positive."""
    one = dtype(1)
    with np.errstate(all="ignore"):
        l00 = np.sqrt(M[:, 0, 0])
        l10, l20 = M[:, 1, 0] / l00, M[:, 2, 0] / l00
        t11 = M[:, 1, 1] - l10 * l10
        l11 = np.sqrt(t11)
        l21 = (M[:, 2, 1] - l20 * l10) / l11
        t22 = M[:, 2, 2] - l20 * l20 - l21 * l21
        l22 = np.sqrt(t22)
        z0 = b[:, 0] / l00
        z1 = (b[:, 1] - l10 * z0) / l11
        z2 = (b[:, 2] - l20 * z0 - l21 * z1) / l22
        x2 = z2 / l22
        x1 = (z1 - l21 * x2) / l11
        x0 = (z0 - l10 * x1 - l20 * x2) / l00
    ok = (M[:, 0, 0] > 0) & (t11 > 0) & (t22 > 0)
    return np.where(ok[:, None], np.stack([x0, x1, x2], -1), 0 * one), ok


class LMStep:
    """One step at the state of `prob` with the column scales cs [n_cams, 6], ps [n_pts, 3], the camera step yc [6 variable cameras]
    (scaled coordinates, variable cameras in the problem's order) and the trust-region radius."""

    def __init__(self, prob, cs, ps, yc, radius, dtype=LD, min_diag=1e-6, max_diag=1e32):
        self.prob, self.dtype, self.radius = prob, dtype, radius
        L = self.L = Layout(prob)
        cs, ps = np.asarray(cs, dtype), np.asarray(ps, dtype) * L.pvar[:, None]
        self.cs, self.ps = cs, ps
        q, t, X = (np.asarray(v, dtype) for v in (prob.cam_quat, prob.cam_t, prob.pts))
        npt, nc = prob.n_pts, prob.n_cams
        lin = self.lin = linearize(prob, L, q, t, X, cs, ps, dtype)
        self.bad_lin = int((~lin["valid"]).sum())
        ycam = np.zeros((nc, 6), dtype)
        ycam[L.cam_var] = np.asarray(yc, dtype).reshape(-1, 6)
        self.ycam = ycam
        r, Jc, Jp = lin["r"], lin["Jc"], lin["Jp"]
        self.mc = np.einsum("brk,bk->br", Jc, ycam[L.cam])
        self.rr = r + self.mc
        V, g, gabs = np.zeros((npt, 3, 3), dtype), np.zeros((npt, 3), dtype), np.zeros((npt, 3), dtype)
        np.add.at(V, L.pt, np.einsum("bri,brj->bij", Jp, Jp))
        np.add.at(g, L.pt, np.einsum("bri,br->bi", Jp, self.rr))
        np.add.at(gabs, L.pt, np.einsum("bri,br->bi", np.abs(Jp), np.abs(self.rr)))
        dV = np.einsum("pii->pi", V)
        self.M = V.copy()
        np.einsum("pii->pi", self.M)[...] = dV + np.clip(dV, dtype(min_diag), dtype(max_diag)) / dtype(radius)
        self.V, self.g, self.gabs = V, g, gabs
        yp, ok = solve_spd3(self.M, -g, dtype)
        self.failed = L.pvar & ~ok                 # landmarks whose damped block is not positive definite
        self.yp = np.where((L.pvar & ok)[:, None], yp, 0)
        self.pts2 = np.where(L.pvar[:, None], X + ps * self.yp, X)
        d = cs * ycam
        self.q2 = np.where(L.cam_var[:, None], quat_plus(q, d[:, :3], dtype), q)
        self.t2 = np.where(L.cam_var[:, None], t + d[:, 3:], t)
        m = self.m_rows(self.yp)
        use = (lin["valid"] & ~self.failed[L.pt])[:, None]
        self.mcc = -(np.where(use, m * (r + m / 2), 0)).sum()
        self.mcc_scale = (np.where(use, np.abs(m) * (np.abs(r) + np.abs(m) / 2), 0)).sum()
        # camera gradient: g_c = sum Jc^T r (scaled), its absolute sum, and the maximum norm of the unscaled gradient
        gc, gc_abs, n_rows = np.zeros((nc, 6), dtype), np.zeros((nc, 6), dtype), np.zeros(nc)
        np.add.at(gc, L.cam, np.einsum("brk,br->bk", Jc, r))
        np.add.at(gc_abs, L.cam, np.einsum("brk,br->bk", np.abs(Jc), np.abs(r)))
        np.add.at(n_rows, L.cam, lin["rows"].sum(-1))
        self.gc, self.gc_abs, self.cam_rows = gc, gc_abs, n_rows
        self.pt_rows = np.zeros(npt)
        np.add.at(self.pt_rows, L.pt, lin["rows"].sum(-1))
        with np.errstate(all="ignore"):
            gu = np.where(cs > 0, -gc / cs, 0)
            self.gu_abs = np.where(cs > 0, gc_abs / cs, 0)
        qg = quat_plus(q, gu[:, :3], dtype)
        per_cam = np.maximum(np.abs(qg - q).max(-1), np.abs(gu[:, 3:]).max(-1))
        self.gmax = per_cam[L.cam_var].max() if L.cam_var.any() else dtype(0)

    def m_rows(self, yp):
        """m = Jc yc + Jp yp per row, for landmark steps yp [n_pts, 3] (scaled coordinates)"""
        return self.mc + np.einsum("bri,bi->br", self.lin["Jp"], np.asarray(yp, self.dtype)[self.L.pt])

    def eta_p(self, yp, slack=None):
        """Componentwise backward error of the landmark steps yp [n_pts, 3] in this step's systems (V + D) yp = -g, per landmark: max_k
        |(V + D) yp + g|_k / (|V + D| |yp| + sum |Jp|^T |r + Jc yc|)_k; 0 where numerator and denominator are both zero.  slack
        [n_pts, 3]: how far every entry of yp may be from the value it stands for (a step recovered from rounded candidates); the
        numerator is reduced by |V + D| slack."""
        yp = np.asarray(yp, self.dtype)
        num = np.abs(np.einsum("pij,pj->pi", self.M, yp) + self.g)
        if slack is not None:
            num = np.maximum(num - np.einsum("pij,pj->pi", np.abs(self.M), np.asarray(slack, self.dtype)), 0)
        den = np.einsum("pij,pj->pi", np.abs(self.M), np.abs(yp)) + self.gabs
        with np.errstate(all="ignore"):
            e = np.where(num == 0, 0, num / den)
        return e.max(-1)

    def scale_tolerances(self, ops=64, ops_r=16):
        """How far a float64 computation of the Jacobi scales 1 / (1 + sqrt(v)), v = sum J^2 over the rows of a column (unit scales), may
        be from this step's cs and ps, which are such a computation themselves: every entry of J within `ops` u of its terms in absolute
        value (linearize's Jc_abs, Jp_abs), the robust weight moved by the rounding of the residual it is a function of (every
        residual within `ops_r` u of its terms: rotation, translation, reciprocal, two products, two sums; w_sens), the sum of n squares
        in any order (n + 2) u, the root and the quotient 2 u; twice that, for the two sides.  (cs_tol [n_cams, 6], ps_tol [n_pts, 3]), absolute."""
        dt, L, lin = self.dtype, self.L, self.lin
        u = dt(2.0) ** -53

        def tol(scale, idx, J, J_abs, n_rows):
            sq, cross = np.zeros_like(scale), np.zeros_like(scale)
            np.add.at(sq, idx, (J * J).sum(1))
            np.add.at(cross, idx, (np.abs(J) * (ops * J_abs + ops_r * lin["w_sens"][:, None, None] * np.abs(J))).sum(1))
            dv = 2 * u * cross + (n_rows[:, None] + 2) * u * sq          # (both times scale^2)
            with np.errstate(all="ignore"):
                root = np.where(scale > 0, 1 / np.where(scale > 0, scale, 1) - 1, 0)   # sqrt(v)
                ds = np.where(root > 0, dv / (2 * np.where(root > 0, root, 1)), 0)     # |ds/dv| dv = s^2 dv / (2 sqrt v); dv holds the s^2
            return 2 * (ds + 2 * u * scale)

        return tol(self.cs, L.cam, lin["Jc"], lin["Jc_abs"], self.cam_rows), tol(self.ps, L.pt, lin["Jp"], lin["Jp_abs"], self.pt_rows)

    def candidate_tolerance(self, eta_bound):
        """How far the candidate landmarks of a step whose backward error eta_p is at most `eta_bound` may be from this step's, per
        entry [n_pts, 3]: ps |(V + D)^-1| (eta_bound (|V + D| |yp| + sum |Jp|^T |r + Jc yc|) + |V + D| u |X2| / ps) + u |X2| (the
        residual of the system may be that large, and the rounding of X2 on top), with this step's own yp and X2 in the bound."""
        dt = self.dtype
        u = dt(2.0) ** -53
        eye = np.eye(3, dtype=dt)
        cols = [solve_spd3(self.M, np.broadcast_to(eye[k], self.g.shape).copy(), dt)[0] for k in range(3)]
        Minv = np.abs(np.stack(cols, -1))
        with np.errstate(all="ignore"):
            slack = np.where(self.ps > 0, u * np.abs(self.pts2) / np.where(self.ps > 0, self.ps, 1), 0)
        den = np.einsum("pij,pj->pi", np.abs(self.M), np.abs(self.yp)) + self.gabs
        res = eta_bound * den + np.einsum("pij,pj->pi", np.abs(self.M), slack)
        return np.where(self.L.pvar[:, None], self.ps * np.einsum("pij,pj->pi", Minv, res) + u * np.abs(self.pts2), 0)

    def mcc_measure(self, mcc):
        return abs(self.dtype(mcc) - self.mcc) / self.mcc_scale if self.mcc_scale > 0 else abs(self.dtype(mcc) - self.mcc)

    def cost_at(self, q, t, pts):
        """(cost of the reduced program at the given state over the blocks that can be evaluated, number of blocks that cannot)"""
        L = self.L
        c, valid = block_costs(self.prob, dict(cam=L.cam, pt=L.pt, kind=L.kind, src=L.src), q, t, pts, self.dtype)
        return c.sum(), int((~valid).sum())

    def cost_gradient_at(self, q, t, pts):
        """|d cost / d X| per landmark [n_pts, 3] and |d cost / d (theta, t)| per camera [n_cams, 6] at the given state, summed in
        absolute value over the blocks (unit scales): what a small change of the state can change the cost by, to first order."""
        L, dt = self.L, self.dtype
        lin = linearize(self.prob, L, q, t, pts, np.ones((self.prob.n_cams, 6)), np.ones((self.prob.n_pts, 3)), dt)
        gp, gc = np.zeros((self.prob.n_pts, 3), dt), np.zeros((self.prob.n_cams, 6), dt)
        np.add.at(gp, L.pt, np.einsum("bri,br->bi", np.abs(lin["Jp"]), np.abs(lin["r"])))
        np.add.at(gc, L.cam, np.einsum("brk,br->bk", np.abs(lin["Jc"]), np.abs(lin["r"])))
        return gp, gc

    def norms(self, q2, t2, pts2):
        """(step_sq_pts, xn_sq_pts, step_sq_cams, xn_sq_cams) of a candidate state against this step's state, over the variables"""
        dt, L = self.dtype, self.L
        q, t, X = (np.asarray(v, dt) for v in (self.prob.cam_quat, self.prob.cam_t, self.prob.pts))
        q2, t2, pts2 = (np.asarray(v, dt) for v in (q2, t2, pts2))
        pv, cv = L.pvar & ~self.failed, L.cam_var
        return (((pts2 - X)[pv] ** 2).sum(), (pts2[pv] ** 2).sum(), ((q2 - q)[cv] ** 2).sum() + ((t2 - t)[cv] ** 2).sum(),
                (q2[cv] ** 2).sum() + (t2[cv] ** 2).sum())
