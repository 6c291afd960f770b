"""Run as a subprocess with MPSFM_POISON=1 (tests/test_gpu_descriptor_matches_batch.py): every device block the calls get is filled
with 0xFF first, so a kernel that reads what nobody wrote shows up as a wrong answer.  Three batches in a row: the later ones get
recycled, poisoned blocks, and within a batch of several groups every group after the first finds the previous group's records in
the tables.  The descriptors are dyadic, so the fp64 restatement is exact and everything is compared bitwise."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy_descriptor_matches as NM  # noqa: E402
from mpsfm_amd import capi  # noqa: E402


def main():
    assert os.environ.get("MPSFM_POISON") == "1"
    rng = np.random.default_rng(13)
    errors = []
    for rep in range(3):
        sizes, dim = (((130, 70, 1, 200), 24), ((65, 200, 0, 3, 129), 37), ((257, 129, 64), 64))[rep]
        d = [(rng.integers(-4, 5, (n, dim)) / 8.0).astype(np.float32) for n in sizes]
        pairs = [(i, j) for i in range(len(d)) for j in range(len(d))]
        for kw in (dict(), dict(ratio_threshold=0.9, distance_threshold=1.1), dict(do_mutual_check=False)):
            for layout in (dict(), dict(pairs_per_group=3, column_ranges=2)):
                ms, ss = capi.match_descriptors_batch(d, pairs, **kw, **layout)
                for (i, j), m, s in zip(pairs, ms, ss):
                    rm, rs, _ = NM.match_descriptors(d[i], d[j], **kw)
                    if not (np.array_equal(m, rm) and s.tobytes() == rs.tobytes()):
                        errors.append(f"batch {rep} pair {(i, j)} {kw} {layout}")
    print("errors:", errors)
    return 1 if errors else 0


if __name__ == "__main__":
    sys.exit(main())
