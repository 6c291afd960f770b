"""The host phases of the table build (csrc/build_host.hip) against the tables of the commit before they were split out of
`build()`: tests/golden/build_tables.npz, recorded on the MI355X from handles created with MPSFM_DEV_BUILD=0
(tests/golden/make_golden_build_tables.py).  The phases run here through mpsfm_debug_host_build, which calls build_tables()
(csrc/ba_build.hip) — the function mpsfm_ba_create runs — for one rank and without the device stages.  Every table bit for bit (dtype, length, SHA-256); rec_d / fx_d = log depth, the only values that pass
through libm, within 4 spacings where the golden stores them in full (the bound tests/test_gpu_devbuild.py uses between two
implementations of log) — the cases that store digests only skip those two tables unless they hold no logarithm (case j: no
depth priors)."""

import os

import pytest

from build_table_cases import CASES, LOG_TABLES, assert_matches_golden, environment, host_tables, load_golden


@pytest.fixture(scope="module")
def golden(golden_dir):
    return load_golden(os.path.join(golden_dir, "build_tables.npz"))


@pytest.mark.parametrize("case", sorted(CASES))
def test_host_phases_reproduce_the_recorded_tables(golden, case):
    make, env, full = CASES[case]
    prob = make()
    with environment({"MPSFM_DEV_BUILD": "0", **env}):
        t = host_tables(prob)
    has_log = prob.n_dobs > 0
    assert_matches_golden(golden, case, t, log_spacings=4, skip=() if full or not has_log else LOG_TABLES)


def test_the_golden_covers_what_it_is_meant_to(golden):
    """The cases reach the paths they were chosen for (read from the recorded lengths)."""
    index, _ = golden
    n = lambda case, name: index[case]["tables"][name][1]  # noqa: E731
    assert n("c", "sky_first") > 0 and n("c", "sky_index") == 0 and n("b", "sky_index") > 0   # skyline / index form
    assert n("d", "ents") > 0 and n("b", "ents") == 0                                         # pair tables everywhere
    assert n("e", "chunks") > n("b", "chunks")                                                # the records override
    assert n("f", "fx_cam") > 0 and n("g", "ents") > 0 and n("h", "lhdr") > 0                 # fixed records, general chunks, long track
    assert n("j", "rec_cam") >= 65536 and n("j", "order") >= 16384 and n("j", "chunks") // 12 >= 96   # the thread splits
    assert [c for c in sorted(index) if not index[c]["device_build_by_default"]] == ["c", "h"]
