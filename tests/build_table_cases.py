"""The cases and the table map of the build-table golden (tests/golden/build_tables.npz): shared by the script that records it
(tests/golden/make_golden_build_tables.py) and the two tests that read it (test_gpu_build_tables.py through a handle,
test_build_tables_cpu.py through the device-free mpsfm_debug_host_build).  The numbering is mpsfm_debug_table's."""

import ctypes as C
import hashlib
import json
import os
from contextlib import contextmanager

import numpy as np

from mpsfm_amd import capi
from mpsfm_amd.synthetic import R_from_quat, local_window, make_scene

TABLES = {0: ("chunks", np.int32), 1: ("chunk_cams", np.int32), 2: ("rec_cam", np.int32), 3: ("rec_pt", np.int32), 4: ("rec_meta", np.uint32),
          5: ("rec_xy", np.float64), 6: ("rec_d", np.float64), 7: ("rec_m", np.float64), 8: ("rec_a", np.float64), 9: ("pt_rec_start", np.int32),
          10: ("pt_kv", np.uint16), 11: ("fx_cam", np.int32), 12: ("fx_pt", np.int32), 13: ("fx_meta", np.uint32), 14: ("fx_xy", np.float64),
          15: ("fx_d", np.float64), 16: ("fx_m", np.float64), 17: ("fx_a", np.float64), 18: ("order", np.int32), 19: ("red_dests", np.int32),
          20: ("red_srcs", np.int32), 21: ("cam_slot", np.int32), 22: ("built_on_device", np.uint8), 23: ("blk_desc", np.uint32),
          24: ("blk_ent_start", np.int32), 25: ("ents", np.uint32), 27: ("lhdr", np.int32), 28: ("sky_index", np.int32),
          29: ("sky_first", np.int32), 30: ("sky_start", np.int64), 31: ("cmask", np.float64), 32: ("cam_of_slot", np.int32),
          33: ("dense_plan", np.int64)}
LOG_TABLES = ("rec_d", "fx_d")  # the only tables that go through a logarithm


def _scene(*a, **kw):
    return make_scene(*a, **kw)[0]


def _local_window():
    base, _ = make_scene(30, 1500, True, seed=11)
    prob = local_window(base, list(range(8, 14)), ref_cam=10)[0]
    prob.pt_const[::7] = 1
    prob.pose_const[-1] = 0  # a variable camera that may have no block at all
    return prob


def _general_chunks():
    prob, _ = make_scene(40, 3000, True, seed=2, max_track=40, track_mean=12.0)
    dup = np.flatnonzero(prob.obs_pt == 5)[:1]   # a second reprojection block of one camera on landmark 5
    prob.obs_cam = np.concatenate([prob.obs_cam, prob.obs_cam[dup]]); prob.obs_pt = np.concatenate([prob.obs_pt, prob.obs_pt[dup]])
    prob.obs_xy = np.concatenate([prob.obs_xy, prob.obs_xy[dup] + 0.5])
    return prob


def _long_track():
    prob, truth = make_scene(300, 2000, False, seed=4)
    R = R_from_quat(truth["cam_quat"])
    Xc = R @ truth["pts"][0] + truth["cam_t"]
    uv = np.stack([1200 * Xc[:, 0] / Xc[:, 2] + 800, 1200 * Xc[:, 1] / Xc[:, 2] + 600], 1)
    prob.obs_cam = np.concatenate([prob.obs_cam, np.arange(300, dtype=np.int32)]); prob.obs_pt = np.concatenate([prob.obs_pt, np.zeros(300, np.int32)])
    prob.obs_xy = np.concatenate([prob.obs_xy, uv])
    return prob


# name -> (problem, environment beside MPSFM_DEV_BUILD=0, rec_d / fx_d stored in full)
CASES = {
    "a": (lambda: _scene(6, 300, True, seed=5), {}, True),
    "b": (lambda: _scene(24, 2000, True, seed=3), {}, True),
    "c": (lambda: _scene(24, 2000, True, seed=3), {"MPSFM_CHOL_GRAPH": "0"}, True),
    "d": (lambda: _scene(24, 2000, True, seed=3), {"MPSFM_SWEEP_DENSE": "0"}, True),
    "e": (lambda: _scene(24, 2000, True, seed=3), {"MPSFM_CHUNK_RECORDS": "64"}, True),
    "f": (_local_window, {}, True),
    "g": (_general_chunks, {}, False),
    "h": (_long_track, {}, True),
    "i": (lambda: _scene(130, 4000, True, seed=6), {}, False),
    "j": (lambda: _scene(50, 20000, False, seed=0), {}, False),
}


@contextmanager
def environment(env):
    """The process environment with `env` applied (a value of None removes the variable) for the duration of the block."""
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _read(call):
    out = {}
    buf = np.zeros(1 << 20, np.uint8)
    for which, (name, dt) in TABLES.items():
        n = call(which, buf.ctypes.data, len(buf))
        assert n >= 0, name
        if n > len(buf):  # the call only reported the size
            buf = np.zeros(n, np.uint8)
            assert call(which, buf.ctypes.data, n) == n, name
        out[name] = buf[:n].view(dt).copy()
    return out


def handle_tables(prob):
    """Every table of a handle created from `prob` under the current environment."""
    L = capi.lib()
    with capi.BAHandle(prob.copy()) as h:
        return _read(lambda which, out, cap: L.mpsfm_debug_table(h._h, which, out, cap))


def host_tables(prob):
    """The same tables from the host phases alone (mpsfm_debug_host_build: no device involved)."""
    L = capi.lib()
    cp = prob.c_problem()
    return _read(lambda which, out, cap: L.mpsfm_debug_host_build(C.byref(cp), which, out, cap))


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def load_golden(path):
    """(index, arrays): the JSON index {case: {"tables": {name: [dtype, length, sha256]}, "device_build_by_default": 0 | 1}} and
    the tables stored in full, "<case>/<name>"."""
    z = np.load(path)
    return json.loads(str(z["index"])), {k: z[k] for k in z.files if k != "index"}


def assert_matches_golden(golden, case, t, log_spacings=0, skip=()):
    """Tables `t` of `case` against the golden: dtype, length and SHA-256 of the bytes; rec_d / fx_d, where the golden stores
    them in full, within `log_spacings` spacings (0: bit for bit)."""
    index, arrays = golden
    for name, (dtype, length, sha) in sorted(index[case]["tables"].items()):
        if name in skip:
            continue
        a = t[name]
        assert str(a.dtype) == dtype and len(a) == length, (case, name)
        if name in LOG_TABLES and log_spacings > 0 and f"{case}/{name}" in arrays:
            g = arrays[f"{case}/{name}"]
            assert np.all(np.abs(a - g) <= log_spacings * np.spacing(np.abs(g))), (case, name)
        else:
            assert digest(a) == sha, (case, name)
