"""The tables of `mpsfm_ba_create` against those of the commit before `build()` was split into its phases:
tests/golden/build_tables.npz (tests/golden/make_golden_build_tables.py, recorded on the MI355X).  With MPSFM_DEV_BUILD=0 — the
host phases — every table bit for bit, rec_d / fx_d included: same machine, same libm.  Under the default environment the handle
is built on the device exactly where it was, and its tables are the same (rec_d / fx_d within 4 spacings: the device's log is not
libm's, the bound of tests/test_gpu_devbuild.py)."""

import os

import numpy as np
import pytest

from build_table_cases import CASES, LOG_TABLES, assert_matches_golden, environment, handle_tables, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    return load_golden(os.path.join(golden_dir, "build_tables.npz"))


@pytest.mark.parametrize("case", sorted(CASES))
def test_host_build_reproduces_the_recorded_tables(golden, case):
    make, env, _ = CASES[case]
    with environment({"MPSFM_DEV_BUILD": "0", **env}):
        t = handle_tables(make())
    assert_matches_golden(golden, case, t)


@pytest.mark.parametrize("case", sorted(CASES))
def test_default_environment_builds_where_it_did_and_the_same_tables(golden, case):
    make, env, full = CASES[case]
    on_device = golden[0][case]["device_build_by_default"]
    with environment({"MPSFM_DEV_BUILD": None, **env}):
        t = handle_tables(make())
    assert t["built_on_device"][0] == on_device
    if case == "h":
        assert on_device == 0   # long tracks take the host build
    # a device-built handle: the flag differs from the recording by design, and the two log tables are the device's
    assert_matches_golden(golden, case, t, log_spacings=4 if on_device else 0,
                          skip=("built_on_device",) + (LOG_TABLES if on_device and not full and make().n_dobs > 0 else ()))
