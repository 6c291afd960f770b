"""Run as a subprocess with MPSFM_POISON=1 (tests/test_gpu_pt_handoff.py): every device block the handle gets is filled with 0xFF
first, so a slot of the hand-off buffer that is read without having been written shows up as a wrong answer."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pytest  # noqa: E402
import test_gpu_pt_handoff as T  # noqa: E402


def main():
    assert os.environ.get("MPSFM_POISON") == "1"
    mp = pytest.MonkeyPatch()
    try:
        for rep in range(2):  # the second pass gets recycled, poisoned blocks
            T.check_constant_scenes(lambda prob, **env: T.gpu_solve(prob, mp, **env)[:2])
    finally:
        mp.undo()
    return 0


if __name__ == "__main__":
    sys.exit(main())
