"""Writes tests/golden/exact_candidates.npz: the candidate cases of tests/exact_geometry.py (inputs of
mpsfm_tri_estimate_batch) and, per residual type, what the exact walk of the LO-RANSAC loop (exact_loransac, mpmath at 60
digits) finds for each: ok, the inlier mask, the index set of the final model, its point, its 4 x 4 matrix and eigenvalues
(each as two float64, 106 bits), the margin, the number of trials and of improving local-optimisation rounds.  Data only.

    PYTHONPATH=.:tests python tests/golden/make_golden_exact_candidates.py

takes a few minutes; tests/test_exact_geometry_cpu.py walks a handful of the candidates again and compares."""

import pathlib
import sys
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
import exact_geometry as G  # noqa: E402


def main():
    t0 = time.time()
    arr = G.candidate_cases().arrays()
    out = dict(arr)
    out.update(G.walk_candidates(arr))
    path = pathlib.Path(__file__).parent / G.CAND_GOLDEN
    np.savez_compressed(path, **out)
    for rt in (0, 1):
        m = out[f"margin{rt}"]
        print(f"residual type {rt}: {int(out[f'ok{rt}'].sum())} of {len(m)} succeed, open: {[str(l) for l, v in zip(arr['labels'], m) if not v > 1]}")
    print(f"{path} {path.stat().st_size} bytes, {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
