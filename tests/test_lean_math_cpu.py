"""The host paths of the lean math of csrc/common.h — lean_log and the two polynomials of quat_plus — against long double, by a
small stand-alone host program built from the header (tests/lean_math_check.hip, host side only; no device is touched).  Bounds:
lean_log within 1 ulp of the exactly rounded logarithm on depths log-uniform in e^+-10, on 1 + 2^-k u, on [0.5, 1.5], on every
binade boundary and its neighbours and on subnormals, +inf -> +inf; sin(n)/n and cos(n) within 1 ulp on n^2 in [0, (pi/4)^2] and
exact at 0; both sides of quat_plus' branch within 2 ulp of each other at the threshold.  The ulp is the spacing of doubles at the
reference value; long double's own error (2^-11 of that) is far below the bounds.  The same program can be built with
-fsanitize=address,undefined and run on its own."""

import functools
import os
import subprocess

from mpsfm_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def figures(tmp: str) -> dict:
    exe = os.path.join(tmp, "lean_math_check")
    src = os.path.join(ROOT, "tests", "lean_math_check.hip")
    r = subprocess.run([build._hipcc(), "--cuda-host-only", "-O2", "-std=c++17", "-o", exe, src], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe, "4000000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    print(r.stdout)
    return {k: float(v) for k, v in (line.split() for line in r.stdout.strip().splitlines())}


def test_lean_log_host_path_is_within_one_ulp(tmp_path_factory):
    f = figures(str(tmp_path_factory.getbasetemp()))
    for name in ("log_depths", "log_near_one", "log_half_to_three_halves", "log_binades", "log_subnormals"):
        assert f[name] <= 1.0, (name, f[name])
    assert f["log_inf"] == 1 and f["log_one_exact"] == 1


def test_quaternion_polynomials_host_path(tmp_path_factory):
    f = figures(str(tmp_path_factory.getbasetemp()))
    assert f["sinc_poly"] <= 1.0 and f["cos_poly"] <= 1.0, (f["sinc_poly"], f["cos_poly"])
    assert f["sinc_zero_exact"] == 1 and f["cos_zero_exact"] == 1 and f["plus_zero_exact"] == 1
    assert f["branch_threshold"] <= 2.0, f["branch_threshold"]
    assert f["plus_far_norm_err"] <= 4e-16, f["plus_far_norm_err"]
