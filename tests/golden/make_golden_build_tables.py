"""Records the tables of the bundle-adjustment table build (`mpsfm_ba_create`) as tests/golden/build_tables.npz, so that a change
of the build that must not change any table can be checked against the commit before it.

Per case of tests/build_table_cases.py (all with MPSFM_DEV_BUILD=0: the host phases) and per table of `mpsfm_debug_table`:
dtype, length and SHA-256 of the bytes (one JSON document, `index`); rec_d and fx_d (log depth: the only values that go through
libm) in full for the small cases.  Also per case whether the handle is built on the device when MPSFM_DEV_BUILD is not set.

Run on the MI355X:  python tests/golden/make_golden_build_tables.py
"""

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))

from build_table_cases import CASES, LOG_TABLES, digest, environment, handle_tables  # noqa: E402


def main():
    index, out = {}, {}
    for case, (make, env, full) in CASES.items():
        prob = make()
        with environment({"MPSFM_DEV_BUILD": "0", **env}):
            t = handle_tables(prob)
        assert t["built_on_device"][0] == 0, case
        index[case] = {"tables": {name: [str(a.dtype), len(a), digest(a)] for name, a in t.items()}}
        if full:
            for name in LOG_TABLES:
                out[f"{case}/{name}"] = t[name]
        with environment({"MPSFM_DEV_BUILD": None, **env}):
            index[case]["device_build_by_default"] = int(handle_tables(prob)["built_on_device"][0])
        print(case, "records", len(t["rec_cam"]), "chunks", len(t["chunks"]) // 12, "fixed", len(t["fx_cam"]), "long", len(t["lhdr"]) // 6,
              "pairs", len(t["ents"]), "device build by default:", index[case]["device_build_by_default"], flush=True)
    path = os.path.join(HERE, "build_tables.npz")
    np.savez_compressed(path, index=np.array(json.dumps(index, sort_keys=True)), **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
