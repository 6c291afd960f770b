"""The device paths of the lean math of csrc/common.h through mpsfm_debug_math_probe, against numpy's long double: lean_log within
1 ulp on 1 M depths log-uniform in e^+-10, 1 M values 1 + 2^-k u, 1 M values in [0.5, 1.5], every binade boundary with its
neighbours and subnormals, +inf -> +inf; sin(n)/n and cos(n) of quat_plus within 1 ulp on 1 M values n^2 in [0, (pi/4)^2], exact at
0, both sides of the branch within 2 ulp of each other at the threshold; 10 k quaternion updates with |d| from 0 to 3, unit to 4e-16
and equal to the formula exp(d) * q in long double to 1e-15, across the branch.  (The CPU twin: tests/test_lean_math_cpu.py.)"""

import numpy as np
import pytest

from mpsfm_amd import capi

pytestmark = pytest.mark.gpu

LD = np.longdouble
ZMAX = 0.61685027506808491368  # kQuatPolyMaxZ, (pi/4)^2
N = 1_000_000


def probe(kind: int, x: np.ndarray) -> np.ndarray:
    x = np.ascontiguousarray(x, np.float64)
    n = x.size // (7 if kind == 2 else 1)
    out = np.empty(n * (1, 2, 4)[kind], np.float64)
    assert capi.lib().mpsfm_debug_math_probe(kind, x.ctypes.data, n, out.ctypes.data) == 0, capi.lib().mpsfm_last_error()
    return out


def ulp_err(got: np.ndarray, ref: np.ndarray) -> np.ndarray:
    """|got - ref| in units of the spacing of doubles at ref (ref: long double)"""
    e = np.maximum(np.frexp(np.abs(ref).astype(np.float64))[1] - 1, -1022)
    return (np.abs(got.astype(LD) - ref) / np.ldexp(LD(1.0), e - 52)).astype(np.float64)


def check_log(name: str, x: np.ndarray) -> None:
    got = probe(0, x)
    err = ulp_err(got, np.log(x.astype(LD)))
    i = int(np.argmax(err))
    print(f"lean_log {name}: n={x.size} worst {err[i]:.4f} ulp at x={x[i]!r}")
    assert np.isfinite(got).all() and err[i] <= 1.0


def test_lean_log_depths():
    check_log("depths", np.exp(np.random.default_rng(1).uniform(-10.0, 10.0, N)))


def test_lean_log_near_one():
    rng = np.random.default_rng(2)
    check_log("1 + 2^-k u", 1.0 + np.ldexp(rng.uniform(-1.0, 1.0, N), -(np.arange(N) % 53).astype(np.int32)))


def test_lean_log_half_to_three_halves():
    check_log("[0.5, 1.5]", np.random.default_rng(3).uniform(0.5, 1.5, N))


def test_lean_log_binades_subnormals_and_infinity():
    p = np.ldexp(1.0, np.arange(-1074, 1024, dtype=np.int32))
    edge = np.concatenate([p, np.nextafter(p, np.inf)[:-1], np.nextafter(p[1:], 0.0), [np.finfo(np.float64).max],
                           np.nextafter(np.sqrt(0.5), [0.0, 1.0]), [np.sqrt(0.5)], np.nextafter(np.sqrt(2.0), [0.0, 2.0]), [np.sqrt(2.0)]])
    check_log("binade boundaries", edge)
    rng = np.random.default_rng(4)
    bits = rng.integers(1, 1 << 52, 100_000, dtype=np.uint64) >> rng.integers(0, 52, 100_000, dtype=np.uint64)
    check_log("subnormals", np.maximum(bits, 1).view(np.float64))
    got = probe(0, np.array([np.inf, 1.0]))
    assert got[0] == np.inf and got[1] == 0.0


def test_quaternion_sine_and_cosine_polynomials():
    rng = np.random.default_rng(5)
    z = np.concatenate([rng.uniform(0.0, ZMAX, N - 250_002), ZMAX * np.exp(-40.0 * rng.uniform(0.0, 1.0, 250_000)), [0.0, ZMAX]])
    got = probe(1, z).reshape(-1, 2)
    n = np.sqrt(z.astype(LD))
    with np.errstate(invalid="ignore", divide="ignore"):
        rs = np.where(z == 0.0, LD(1.0), np.sin(n) / n)
    es, ec = ulp_err(got[:, 0], rs), ulp_err(got[:, 1], np.cos(n))
    print(f"sin(n)/n worst {es.max():.4f} ulp at z={z[int(np.argmax(es))]!r}; cos(n) worst {ec.max():.4f} ulp at z={z[int(np.argmax(ec))]!r}")
    assert es.max() <= 1.0 and ec.max() <= 1.0
    assert got[-2, 0] == 1.0 and got[-2, 1] == 1.0  # z == 0 is exact
    # the last value of the polynomials against the first of the far branch: the function itself moves by far less than an ulp
    edge = probe(1, np.array([ZMAX, np.nextafter(ZMAX, 1.0)])).reshape(2, 2)
    d = ulp_err(edge[1], edge[0].astype(LD))
    print(f"branch threshold: {d[0]:.1f} / {d[1]:.1f} ulp between the two sides")
    assert d.max() <= 2.0


def test_quaternion_updates_across_the_branch():
    rng = np.random.default_rng(6)
    n = 10_000
    q = rng.normal(size=(n, 4)).astype(LD)
    q = (q / np.sqrt((q * q).sum(1))[:, None]).astype(np.float64)
    d = rng.normal(size=(n, 3))
    d *= (np.linspace(0.0, 3.0, n) / np.sqrt((d * d).sum(1)))[:, None]
    got = probe(2, np.concatenate([q, d], axis=1).ravel()).reshape(n, 4)
    assert (got[0] == q[0]).all()  # |d| == 0 returns q itself
    ql, dl = q.astype(LD), d.astype(LD)
    t = np.sqrt((dl * dl).sum(1))
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(t == 0.0, LD(1.0), np.sin(t) / t)
    px, py, pz, pw = s * dl[:, 0], s * dl[:, 1], s * dl[:, 2], np.cos(t)
    qx, qy, qz, qw = ql.T
    ref = np.stack([pw * qx + px * qw + py * qz - pz * qy, pw * qy - px * qz + py * qw + pz * qx,
                    pw * qz + px * qy - py * qx + pz * qw, pw * qw - px * qx - py * qy - pz * qz], axis=1)
    gl = got.astype(LD)
    unit = np.abs(np.sqrt((gl * gl).sum(1)) - 1.0).astype(np.float64)
    diff = np.abs(gl - ref).max(1).astype(np.float64)
    near = (d * d).sum(1) <= ZMAX
    print(f"{int(near.sum())} updates on the polynomials, {int((~near).sum())} beyond; | |q'| - 1 | worst {unit.max():.3e}, "
          f"|q' - formula| worst {diff.max():.3e} (near {diff[near].max():.3e}, far {diff[~near].max():.3e})")
    assert near.any() and (~near).any()
    assert unit.max() <= 4e-16 and diff.max() <= 1e-15
