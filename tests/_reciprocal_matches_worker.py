"""Run as a subprocess with MPSFM_POISON=1 (tests/test_gpu_reciprocal_matches.py): every device block the calls get is filled
with 0xFF first, so a kernel that reads what nobody wrote shows up as a wrong answer."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy_reciprocal_matches as NR  # noqa: E402
from mpsfm_amd import capi  # noqa: E402


def main():
    assert os.environ.get("MPSFM_POISON") == "1"
    errors = []
    for rep in range(3):  # later calls get recycled, poisoned blocks
        for name in ("seeds65", "C33", "S1", "iter2"):
            A, B, S, max_iter = NR.sweep_inputs(name)
            r = NR.fast_reciprocal_nns(A, B, S, max_iter)
            i1, i2, info = capi.reciprocal_nns(A, B, S, max_iter, return_info=True)
            if not (np.array_equal(i1, r["idx1"]) and np.array_equal(i2, r["idx2"]) and info["nn_queries"] == r["nn_queries"]):
                errors.append(f"reciprocal_nns {name} rep {rep}")
        feats, qonfs, S = NR.fixture_inputs("small")
        want = NR.extract_correspondences(feats, qonfs, S)
        got = capi.dense_correspondences(feats, qonfs, S)
        if not all(np.array_equal(a, b) for a, b in zip(got, want)):
            errors.append(f"dense_correspondences rep {rep}")
    print("errors:", errors)
    return 1 if errors else 0


if __name__ == "__main__":
    sys.exit(main())
