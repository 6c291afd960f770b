"""Reference solution of a reduced camera system and the measure the dense solve is held to.

Reference: one fp64 Cholesky factorisation, then iterative refinement with the residual formed in np.longdouble (x87
extended, 64-bit mantissa).  With kappa(S) u << 1 every step gains a factor ~kappa u; the iteration stalls where the
residual's own rounding stops it (2^-64 cond for the plain product, ~2^-64 once the residual is accumulated with
compensation), far below the fp64 unit roundoff u = 2^-53.

Measure: rho(y) = (|y - y*|_inf / |y*|_inf) / (u cond(S, y*)), the forward error in units of what a componentwise
backward-stable fp64 solver may lose on THIS system: cond = | |S^-1| (|S| |y*| + |rhs|) |_inf / |y*|_inf is Skeel's condition
number (Higham, Accuracy and Stability of Numerical Algorithms, 7.2).  A correct solver has rho of order one at every
size and conditioning; a dropped tile product has rho of order 1 / (u cond)."""

import numpy as np
from scipy.linalg import cho_factor, cho_solve

U = 2.0 ** -53
LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble is no wider than fp64 here: no extended-precision residual"

# Largest rho of fp64 NumPy solvers on the oracle's S and rhs of every case of graph_scenes.CASES with n <= 2100, radii 1e4
# and 1e-1 (measured by test_dense_graphs_cpu.py, which holds these literals to what it measures; per case in DESIGN.md 4a-2).
RHO_NUMPY = {"lu": 8.23, "cholesky": 5.37, "plan_accumulators": 6.99, "plan_back_levels": 6.99}
# The bound of every device check: 8 x the largest of them (the project's usual margin over a NumPy ratio).
# Never widened from a device result.
C_RHO = 65.84


_SPLIT = LD(2.0 ** 32 + 1.0)  # Veltkamp's constant for a 64-bit mantissa: two halves of at most 32 bits, whose products are exact


def _split(a):
    c = _SPLIT * a
    hi = c - (c - a)
    return hi, a - hi


def _residual_compensated(St, rl, y, block=128):
    """rl - S y in np.longdouble as if accumulated in twice its precision (Ogita, Rump, Oishi: Dot2): Dekker's error-free
    products, every partial sum with its rounding error (TwoSum).  St = S^T, C-contiguous, np.longdouble."""
    s, c = rl.copy(), np.zeros_like(rl)
    for j0 in range(0, St.shape[0], block):
        A, b = St[j0:j0 + block], y[j0:j0 + block, None]
        (Ah, Al), (bh, bl) = _split(A), _split(b)
        P = A * b
        c -= (Al * bl - (((P - Ah * bh) - Al * bh) - Ah * bl)).sum(axis=0)  # what the rounded products lost
        for x in P:
            t = s - x
            z = t - s
            c += (s - (t - z)) - (x + z)
            s = t
    return s + c


def solve_refined(S, rhs, max_steps=16):
    """Returns (y* as np.longdouble, size of the last correction relative to |y*|_inf).  The last correction is the one that
    no longer shrank and was NOT applied: an estimate of what y* itself is off by.  Fails (AssertionError) when that is
    above 2^-3 u.

    The plain long-double residual stalls at ~2^-64 cond (1e-17 where cond is near 1e3, too close to the bound to hold on
    every run), so from there the refinement goes on with the compensated residual until that stalls too."""
    c = cho_factor(S, lower=True)
    Sl, rl = S.astype(LD), rhs.astype(LD)
    y = cho_solve(c, rhs).astype(LD)
    last, St = np.inf, None
    for step in range(max_steps):
        r = rl - Sl @ y if St is None else _residual_compensated(St, rl, y)
        d = cho_solve(c, r.astype(np.float64))
        dn = float(np.abs(d).max())
        if step >= 3 and not dn < last:  # at least three corrections applied and this one no longer shrinks
            if St is not None:
                last = dn
                break
            St, last = np.ascontiguousarray(Sl.T), np.inf  # (the plain residual's floor says nothing about the other's)
            continue
        y = y + d.astype(LD)
        last = dn
    scale = float(np.abs(y).max())
    assert scale > 0 and np.isfinite(scale)
    assert last <= 2.0 ** -3 * U * scale, f"refinement stalled at {last / scale:.2e} |y|, above 2^-3 u = {2.0 ** -3 * U:.2e}"
    return y, last / scale


class Reference:
    """y*, Skeel's condition number and the norms of one system (the inverse is formed once, every solver's y is then measured
    against the same numbers)."""

    def __init__(self, S, rhs):
        self.S, self.rhs = S, rhs
        self.y, self.stall = solve_refined(S, rhs)
        self.scale = float(np.abs(self.y).max())
        ya = np.abs(self.y).astype(np.float64)
        self.cond = float((np.abs(np.linalg.inv(S)) @ (np.abs(S) @ ya + np.abs(rhs))).max()) / self.scale
        self.norm_S = float(np.abs(S).sum(axis=1).max())

    def rho(self, y):
        """Forward error of y over u cond; inf for a y that is not finite."""
        y = np.asarray(y)
        if not np.isfinite(y).all():
            return np.inf
        return float(np.abs(y.astype(LD) - self.y).max()) / self.scale / (U * self.cond)

    def eta(self, y):
        """Normwise backward error |rhs - S y|_inf / (|S|_inf |y|_inf + |rhs|_inf) (for the record: the inverse-accumulator
        path need not be backward stable, so nothing is asserted on it)."""
        y = np.asarray(y)
        if not np.isfinite(y).all():
            return np.inf
        r = self.rhs.astype(LD) - self.S.astype(LD) @ y.astype(LD)
        return float(np.abs(r).max()) / (self.norm_S * float(np.abs(y).max()) + float(np.abs(self.rhs).max()))


def rho(y, ref):
    return ref.rho(y)
