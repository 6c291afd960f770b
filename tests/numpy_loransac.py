"""numpy_loransac.py — TEST INFRASTRUCTURE, NOT PRODUCT CODE.

What the NumPy restatements of the two LO-RANSAC estimators (numpy_absolute_pose.py, numpy_relative_pose.py) share: the
documented counter-based sampler computed with Python ints, ``RANSAC::ComputeNumTrials`` and the support measure of
``InlierSupportMeasurer``.  Their ``estimate`` loops stay apart: the fragile-decision bookkeeping differs.
"""

from __future__ import annotations

import math

MASK64 = (1 << 64) - 1
PHI = 0x9E3779B97F4A7C15


def _mix(z: int) -> int:
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def sample(seed: int, t: int, n: int, k: int) -> list[int]:
    """The k distinct indices of trial t: base = mix(seed + (t + 1) PHI), r_j = mix(base + j PHI), idx = r_j n >> 64."""
    base = _mix((seed + (t + 1) * PHI) & MASK64)
    out, j = [], 0
    while len(out) < k:
        j += 1
        c = (_mix((base + j * PHI) & MASK64) * n) >> 64
        if c not in out:
            out.append(c)
    return out


def num_trials(num_inliers: int, n: int, confidence: float, multiplier: float, sample_size: int) -> float:
    """RANSAC::ComputeNumTrials with kMinNumSamples = sample_size (math.inf for size_t max)."""
    ratio = num_inliers / n
    nom = 1.0 - confidence
    if nom <= 0:
        return math.inf
    denom = 1.0 - math.pow(ratio, float(sample_size))
    if denom <= 0:
        return 1
    if denom == 1.0:
        return math.inf
    return math.ceil(math.log(nom) / math.log(denom) * multiplier)


def _support(res, thr2):
    inl = res <= thr2
    return int(inl.sum()), float(res[inl].sum())


def _better(a, b):
    return a[0] > b[0] or (a[0] == b[0] and a[1] < b[1])
