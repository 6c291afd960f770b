"""Run as a subprocess with MPSFM_POISON=1 (tests/test_gpu_retrieval.py): every device block the calls get is filled with 0xFF
first, so a kernel that reads what nobody wrote shows up as a wrong answer."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy_retrieval as NR  # noqa: E402
from mpsfm_amd import capi  # noqa: E402


def main():
    assert os.environ.get("MPSFM_POISON") == "1"
    rng = np.random.default_rng(12)
    errors = []
    for rep in range(3):  # later calls get recycled, poisoned blocks
        nq, nd, dim = ((130, 70, 24), (65, 200, 37), (257, 129, 64))[rep]
        q, db = (rng.integers(-4, 5, (nq, dim)) / 8.0).astype(np.float32), (rng.integers(-4, 5, (nd, dim)) / 8.0).astype(np.float32)
        sim = NR.similarities(q, db)
        qi, di = rng.integers(0, 40, nq).astype(np.int32), rng.integers(0, 40, nd).astype(np.int32)
        for k, ms, ids, cr in ((5, 0.0, False, 0), (20, None, True, 1), (64, 0.25, True, 2), (70, None, False, 3)):
            args = (qi, di) if ids else (None, None)
            got = capi.retrieve_topk(q, db, k, ms, *args, column_ranges=cr)
            want = NR.topk_similarities(sim, k, ms, *args)[:3]
            if not all(np.array_equal(a, b) for a, b in zip(got, want)):
                errors.append(f"retrieve_topk {nq} x {nd} x {dim} k {k} min_score {ms} ids {ids} ranges {cr}")
    print("errors:", errors)
    return 1 if errors else 0


if __name__ == "__main__":
    sys.exit(main())
