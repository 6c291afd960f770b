"""Run as a subprocess with MPSFM_POISON=1 (tests/test_gpu_direct_assemble.py): every device block the handle gets is filled with
0xFF first, so a tile of A, an inverse accumulator or a vector that the direct form of the front reads without having zeroed it
shows up as a wrong answer."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_direct_assemble as T  # noqa: E402


def main():
    assert os.environ.get("MPSFM_POISON") == "1"
    for rep in range(2):  # the second pass gets recycled, poisoned blocks
        T.check_parity("chain_constant")
        T._solves.cache_clear()
        for ending in ("tolerance", "rejected_steps"):
            for second in (0, 1):
                d, l = T._solves(ending, "split", "direct")[second], T._solves(ending, "split", "launch")[second]
                assert d[6] and not l[6]
                T.assert_same(d, l)
    return 0


if __name__ == "__main__":
    sys.exit(main())
