"""Block-edge maps for the depth-from-normals integration and the reference side of their linear system: shared by
tests/test_integration_system_cpu.py (the reference alone) and tests/test_gpu_integration_system.py (HIP against it).

The reference is oracle/integration_oracle.py (prepare, CamData, init_int_vars, calc_Wpm, calc_Amat, rhs, integrate with its
`record=` hook), SciPy's sparse direct solve and cg, and plain NumPy in long double.  No arithmetic of the package goes into it:
`make_maps` only draws the inputs."""

from __future__ import annotations

from functools import lru_cache

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.linalg import cg, splu

from mpsfm_amd.synthetic_maps import make_maps
from oracle import integration_oracle as IO

KEYS = ("depth_prior", "depth_uncertainty", "valid", "normals", "normals_uncertainty", "depth_init", "K", "kps", "depth3d", "zvars3d")

# The CG kernels run 256 threads per workgroup with one or two pixels per thread: 256 / 512 pixels per workgroup.
SIZES = (
    (2, 2),      # 4: every pixel a corner
    (2, 3),      # 6: two rows
    (3, 2),      # 6: two columns
    (15, 17),    # 255: one below the 256-pixel workgroup edge (one pixel per thread)
    (16, 16),    # 256: on that edge
    (2, 129),    # 258: one past it; the second pixel slot covers two pixels
    (129, 2),    # 258: the same count with the neighbours the other way
    (7, 73),     # 511: one below the 512-pixel edge (two pixels per thread)
    (16, 32),    # 512: on that edge
    (19, 27),    # 513: one past it
    (24, 32),    # 768: the second slot of the second workgroup is empty
    (22, 35),    # 770: that slot holds two pixels
    (2, 300),    # 600: a row longer than a workgroup, the down neighbour is in the next one
)
SIZE_IDS = [f"{h}x{w}" for h, w in SIZES]
VARIANCE_SIZES = ((2, 2), (2, 129), (129, 2), (7, 73), (16, 32), (19, 27), (2, 300))
PAD = 4  # the crop window lies PAD pixels inside the drawn map on every side
# Focal length of the draw in map widths.  The couplings of the system grow with f^2 against the depth prior's anchoring, and
# with `make_maps`' own 1.1 the 2x300 chain is beyond what the reference can pin: the oracle at cg_tol 1e-12 runs into its
# cg_max_iter of 5000 with a true residual of 3.9e-10, worse than its run at 1e-10, so a bound made from that pair means
# nothing, and reordered fp64 sums move the stop of the 1e-10 run by 130 iterations.  A tight pin needs a reference that
# converges at 1e-12 at every size; 0.3 (a wide-angle camera) gives that with room (2x300: 3256 iterations, cond 1.4e6), and
# tests/test_integration_system_cpu.py asserts it, together with the reference meeting its own bounds under reordered sums.
FOCAL = 0.3


def sparse_pixels(H, W):
    """(x, y) of the sparse set: the four corners, the middle of each border line that has one, the first corner again."""
    px = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    if W >= 3:
        px += [(W // 2, 0), (W // 2, H - 1)]
    if H >= 3:
        px += [(0, H // 2), (W - 1, H // 2)]
    return px + [(0, 0)]


def build_maps(H, W, seed=0, n_interior=0, sparse=True):
    """The centre H x W window of a (H + 2 PAD) x (W + 2 PAD) `make_maps` draw.  A centred window keeps u and v of every pixel, so
    the normals stay consistent with a principal point at the window's centre.  At least two pixels are invalid (one for 2x2).
    Sparse points: `sparse_pixels`, the repeated corner with a second depth 3 % off ("last write wins" in calc_Amat / rhs, both
    entries in the energy), then `n_interior` of the draw's own points that fall inside the window."""
    big = make_maps(H + 2 * PAD, W + 2 * PAD, seed=seed, n_sparse=max(60, 6 * n_interior), f=FOCAL * (W + 2 * PAD))
    win = (slice(PAD, PAD + H), slice(PAD, PAD + W))
    m = {k: np.ascontiguousarray(big[k][win]) for k in ("depth_true", "depth_prior", "depth_uncertainty", "valid", "normals",
                                                         "normals_uncertainty", "depth_init")}
    m["K"] = (big["K"][0], big["K"][1], (H - 1) / 2.0, (W - 1) / 2.0)
    valid = m["valid"].copy()
    valid.flat[(H * W) // 2] = False          # 2x2: the pixel (1, 0)
    if H * W > 4:
        valid[H - 1, W // 2] = False          # on the last row
        valid[H // 2, W - 1] = False          # on the last column
    m["valid"] = valid
    rng = np.random.default_rng(1000 + seed)
    if sparse:
        px = np.array(sparse_pixels(H, W))
        d3 = m["depth_true"][px[:, 1], px[:, 0]] * np.exp(rng.normal(0, 0.01, len(px)))
        d3[-1] = 1.03 * d3[0]
        inside = [(x - PAD, y - PAD) for x, y in big["kps"] if PAD + 1 <= x < PAD + W - 1 and PAD + 1 <= y < PAD + H - 1][:n_interior]
        if inside:
            ins = np.array(inside)
            px = np.concatenate([px, ins])
            d3 = np.concatenate([d3, m["depth_true"][ins[:, 1], ins[:, 0]] * np.exp(rng.normal(0, 0.01, len(ins)))])
        m["kps"], m["depth3d"] = px.astype(np.int64), d3
        m["zvars3d"] = (0.01 * d3) ** 2 * rng.uniform(0.5, 2.0, len(d3))
    else:
        m["kps"], m["depth3d"], m["zvars3d"] = np.zeros((0, 2), np.int64), np.zeros(0), np.zeros(0)
    return m


def conf_of(**conf):
    c = dict(IO.DEFAULT_CONF)
    c.update(conf)
    return c


def inputs(maps, conf=None):
    return IO.IntInputs(**{k: maps[k] for k in KEYS}, conf=conf_of(**(conf or {})))


def normals_var(maps):
    nu = maps["normals_uncertainty"]
    return np.stack([nu[..., 0, 0], nu[..., 1, 1], nu[..., 2, 2]], -1)


# ---- the linear system of IRLS step 0, from the oracle's own pieces -----------------------------------------------------------

def system(maps, conf=None):
    """(A csr, b, diag, z0) of the first IRLS step: the matrix of calc_Amat, the right-hand side of rhs, the diagonal the
    preconditioner is made from and the start vector log(depth_init)."""
    inp = inputs(maps, conf)
    c = inp.conf
    P = IO.prepare(inp)
    H, W = P["shape"]
    cam = IO.CamData(H, W)
    state = IO.IntState()
    Nz, Nu_p, Nv_p, _, _ = IO.init_int_vars(cam, P["z"], inp.K, P["nx"], P["ny"], P["nz"], P["Vnx"], P["Vny"], P["Vnz"], c, state)
    W4 = IO.calc_Wpm(Nu_p, Nv_p, state.wu, state.wv)
    A, diag = IO.calc_Amat(cam, Nz, W4, P["depth_precision"], P["sparse_precision"], P["sparse_ids"], c)
    b = IO.rhs(state.A, W4, P["nx"], P["ny"], P["depth_precision"], P["z_prior"], P["sparse_precision"], P["sparse_depth"],
               P["sparse_ids"], c)
    return csr_matrix(A), b, diag, P["z"].copy()


def matvec_ld(A, x):
    """A x in long double (SciPy's sparse types stop at float64: entry by entry through the COO form)."""
    coo = A.tocoo()
    y = np.zeros(A.shape[0], np.longdouble)
    np.add.at(y, coo.row, coo.data.astype(np.longdouble) * np.asarray(x, np.longdouble)[coo.col])
    return y


def residual_ld(A, b, z):
    return np.asarray(b, np.longdouble) - matvec_ld(A, z)


def norm_ld(v):
    v = np.asarray(v, np.longdouble)
    return np.sqrt(np.sum(v * v))


def true_residual(A, b, z):
    """|b - A z|_2 / |b|_2, evaluated in long double."""
    return float(norm_ld(residual_ld(A, b, z)) / norm_ld(b))


def direct(A, b):
    """Sparse LU solve, and the same after one refinement step whose residual is formed in long double:
    (refined, unrefined)."""
    lu = splu(A.tocsc())
    x0 = lu.solve(np.asarray(b, np.float64))
    x1 = x0 + lu.solve(np.asarray(residual_ld(A, b, x0), np.float64))
    return x1, x0


def jacobi(diag):
    n = len(diag)
    return csr_matrix((1 / np.clip(diag, 1e-5, None), np.arange(n), np.arange(n + 1)), shape=(n, n))


def scipy_pcg(A, b, z0, diag, rtol, maxiter=5000):
    """The oracle's call of scipy.sparse.linalg.cg (integration_oracle.integrate): (solution, iterations)."""
    its = [0]

    def cb(_x):
        its[0] += 1

    z, _ = cg(A, b, x0=z0.copy(), M=jacobi(diag), maxiter=maxiter, rtol=rtol, callback=cb)
    return z, its[0]


def pcg_ld(A, b, z0, diag, k):
    """Exactly k iterations of preconditioned CG in long double, the recurrences of scipy.sparse.linalg.cg (no stopping test)."""
    ld = np.longdouble
    minv = 1 / np.clip(np.asarray(diag, ld), ld(1e-5), None)
    x = np.asarray(z0, ld).copy()
    r = residual_ld(A, b, x)
    p = rho_prev = None
    for it in range(k):
        zz = minv * r
        rho = np.sum(r * zz)
        p = zz.copy() if it == 0 else zz + (rho / rho_prev) * p
        q = matvec_ld(A, p)
        alpha = rho / np.sum(p * q)
        x += alpha * p
        r -= alpha * q
        rho_prev = rho
    return x


# ---- one reference per size, computed once and left unchanged -----------------------------------------------------------------

STEP_CONF = dict(max_iter=1, cg_tol=1e-10, scale_filter=False)


def oracle_run(maps, **conf):
    """integration_oracle.integrate: dict(z, changed, energies, cg_iters, wu, wv), z = log(depth) or None."""
    depth, changed, state, info = IO.integrate(inputs(maps, conf))
    return dict(z=None if depth is None else np.log(depth).ravel(), changed=changed, energies=np.array(info["energies"]),
                cg_iters=list(info["cg_iters"]), wu=state.wu.copy(), wv=state.wv.copy())


def rel_gap(a, b, floor=1e-12):
    """Largest relative difference of two reference results, with a floor: the unit of the GPU bounds."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return max(float(np.max(np.abs(a - b) / np.abs(b))), floor)


def abs_gap(a, b, floor=1e-12):
    return max(float(np.max(np.abs(np.asarray(a) - np.asarray(b)))), floor)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, dict):
            _freeze(v)
    return d


@lru_cache(maxsize=None)
def step_reference(H, W):
    """Everything reference-only that the one-step tests need at one size."""
    maps = build_maps(H, W)
    A, b, diag, z0 = system(maps, STEP_CONF)
    zd, zd0 = direct(A, b)
    zc, its = scipy_pcg(A, b, z0, diag, STEP_CONF["cg_tol"])
    o10 = oracle_run(maps, **STEP_CONF)
    o12 = oracle_run(maps, **dict(STEP_CONF, cg_tol=1e-12))
    d_cg, d_ref = float(np.max(np.abs(zc - zd))), float(np.max(np.abs(zd - zd0)))
    z12, its12 = scipy_pcg(A, b, z0, diag, 1e-12)
    return _freeze(dict(
        cg_iters12=its12, res_cg12=true_residual(A, b, z12),
        maps=maps, A=A, b=b, diag=diag, z0=z0, z_direct=zd, z_direct_unrefined=zd0, z_cg=zc, cg_iters=its, o10=o10, o12=o12,
        res_cg=true_residual(A, b, zc), res_direct=true_residual(A, b, zd), d_cg=d_cg, d_refine=d_ref,
        z_bound=10 * max(d_cg, d_ref, 1e-15),
        e1_bound=10 * rel_gap(o10["energies"][1], o12["energies"][1]),
        w_bound=10 * max(abs_gap(o10["wu"], o12["wu"]), abs_gap(o10["wv"], o12["wv"])),
    ))


def after_step(maps, z, conf=None):
    """(energy, wu, wv) the oracle's IRLS loop forms from a solution z of step 0: update_W, calc_Wpm, calc_energy."""
    inp = inputs(maps, conf or STEP_CONF)
    c = inp.conf
    P = IO.prepare(inp)
    cam = IO.CamData(*P["shape"])
    state = IO.IntState()
    _, Nu_p, Nv_p, _, _ = IO.init_int_vars(cam, P["z"], inp.K, P["nx"], P["ny"], P["nz"], P["Vnx"], P["Vny"], P["Vnz"], c, state)
    wu, wv = IO.update_W(z, state.A, c["k"])
    e = IO.calc_energy(state.A, IO.calc_Wpm(Nu_p, Nv_p, wu, wv), z, P["nx"], P["ny"], P["depth_precision"], P["z_prior"],
                       P["sparse_precision"], P["sparse_depth"], P["sparse_ids"], c)
    return float(e), wu, wv


def reordered_pcg(R, perm):
    """The oracle's PCG on the symmetrically permuted system of a `step_reference`: the same iterates in exact arithmetic,
    another order of the fp64 sums.  Returns (z in the original order, iterations)."""
    zp, its = scipy_pcg(R["A"][perm][:, perm].tocsr(), R["b"][perm], R["z0"][perm], R["diag"][perm], STEP_CONF["cg_tol"])
    z = np.empty_like(zp)
    z[perm] = zp
    return z, its


def with_outlier(maps):
    """The maps with one more sparse point, on the last column, whose depth is twice the prior's: the scale filter of
    `_integrate` drops it (factor 1.5), so the two `scale_filter` settings solve different systems."""
    H, W = maps["depth_prior"].shape
    y = H // 2 + 1
    d = 2.0 * maps["depth_prior"][y, W - 1]
    return dict(maps, kps=np.concatenate([maps["kps"], [[W - 1, y]]]), depth3d=np.append(maps["depth3d"], d),
                zvars3d=np.append(maps["zvars3d"], (0.01 * d) ** 2))


STEPS_CONF = dict(max_iter=4, tol=0, cg_tol=1e-10)  # tol = 0: no early stop


@lru_cache(maxsize=None)
def steps_reference(H, W, scale_filter):
    """Four IRLS steps of the oracle on `with_outlier` at cg_tol 1e-10 and 1e-12: (o10, o12)."""
    maps = with_outlier(step_reference(H, W)["maps"])
    conf = dict(STEPS_CONF, scale_filter=scale_filter)
    return _freeze(oracle_run(maps, **conf)), _freeze(oracle_run(maps, **dict(conf, cg_tol=1e-12)))
