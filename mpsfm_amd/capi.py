"""Python wrappers over libmpsfm_hip.so (include/mpsfm_hip.h); abi.py declares the structs, the signatures and the loader.

This is the only door between the Python host layer and the HIP kernels.  There is no CPU
fallback: every call fails loudly when the library is missing or no gfx950 device is visible.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from .abi import (  # noqa: F401 - declared in abi.py; these names stay importable from here
    ALLREDUCE_FN, LIB_PATH, SIGNATURES, CAbsPoseOptions, CAbsPoseResult, CAlign3dOptions, CAlign3dResult, CCorrGraphInfo, CDcImage, CDebugLmCtl, CDebugLmOpts, CDcSummary, CDepthGather, CDepthPriorConf,
    CDepthPriorOutput, CDepthPriorProblem, CIcpOptions, CIcpResult, CInitCandidates, CInitPair, CIntProblem, CIntSummary, CLiftInfo, CLiftMaps, CMatchBatchReport, CMatchInfo, CMatchOptions, CNmsInfo,
    CNormalPriorConf, CNormalPriorOutput, CNormalPriorProblem, COptions, CPriorSummary, CProblem, CRansacOptions, CRecipInfo,
    CRecipOptions, CRegImage, CRelPoseOptions, CRetrievalInfo, CSceneFilterInfo, CSceneFilterOptions, CSceneQueryInfo, CTriGraph, CTriState, CRetrievalOptions, CRelPoseResult, CState, CSummary, CTracks, CTriCandidates, CTwoViewBatchReport, CTwoViewLeg, CTwoViewOptions,
    CTwoViewResult, CWarpInfo, CWarpOptions, MpsfmHipError, lib,
)
from .problem import BAProblem, Tracks

EXPORTS = list(SIGNATURES)  # every function of include/mpsfm_hip.h
# names that callers outside the package have read from here; they are the table's own lists, not second declarations
_MATCH_DESC_ARGS = SIGNATURES["mpsfm_match_descriptors"][1]
_MATCH_MAP_ARGS = SIGNATURES["mpsfm_match_map_descriptors"][1]
_SIMPLE_NMS_ARGS = SIGNATURES["mpsfm_simple_nms"][1]
_KPIDS_ARGS = SIGNATURES["mpsfm_kpids_to_matches0"][1]
_WARP_ARGS = SIGNATURES["mpsfm_warp_matches"][1]


def _check(rc: int):
    if rc != 0:
        raise MpsfmHipError(rc, (lib().mpsfm_last_error() or b"").decode())


def device_count() -> int:
    return int(lib().mpsfm_device_count())


def default_options(**kw) -> COptions:
    o = COptions()
    lib().mpsfm_ba_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def comm_unique_id() -> bytes:
    """128 bytes for COptions.comm_id (ncclGetUniqueId of the RCCL library in the process)."""
    buf = (C.c_uint8 * 128)()
    _check(lib().mpsfm_comm_unique_id(C.addressof(buf)))
    return bytes(buf)


def make_allreduce(fn):
    """fn(ptr:int, count:int, on_device:bool, stream:int) -> None must sum the buffer over ranks."""

    def _cb(user, buf, count, on_device, stream):
        try:
            fn(C.addressof(buf.contents), int(count), bool(on_device), int(stream or 0))
            return 0
        except Exception as e:  # noqa: BLE001 - must not propagate through C
            import sys

            print(f"[mpsfm_amd] all-reduce hook raised: {e!r}", file=sys.stderr)
            return -1

    return ALLREDUCE_FN(_cb)


# Handles still open when the interpreter exits are closed from a Python atexit hook, i.e. BEFORE the C runtime's own exit
# handlers: a handle destroyed later (garbage collection at shutdown, static destruction) calls into a HIP runtime that may already
# be gone — under rocprofv3, whose tool finalisation runs first, that was a segmentation fault at exit.
_open_handles: "weakref.WeakSet" = None


def _track(handle):
    global _open_handles
    import atexit
    import weakref

    if _open_handles is None:
        _open_handles = weakref.WeakSet()

        def _close_all():
            for h in list(_open_handles):
                try:
                    h.close()
                except Exception:  # noqa: BLE001
                    pass

        atexit.register(_close_all)
    _open_handles.add(handle)


class BAHandle:
    """Resident problem: the observation lists, poses and points live in HBM between calls."""

    def __init__(self, prob: BAProblem, options: COptions | None = None):
        self._h = C.c_void_p(None)
        self.prob = prob
        self.options = options if options is not None else default_options()
        cp, cs = prob.c_problem(), prob.c_state()
        _check(lib().mpsfm_ba_create(C.byref(cp), C.byref(cs), C.byref(self.options), C.byref(self._h)))
        _track(self)

    def close(self):
        if self._h:
            lib().mpsfm_ba_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_state(self, prob: BAProblem | None = None):
        cs = (prob or self.prob).c_state()
        _check(lib().mpsfm_ba_set_state(self._h, C.byref(cs)))

    def reset_state(self):
        _check(lib().mpsfm_ba_reset_state(self._h))

    def solve(self) -> dict:
        sm = CSummary()
        _check(lib().mpsfm_ba_solve_resident(self._h, C.byref(sm)))
        return sm.to_dict()

    def get_state(self, prob: BAProblem | None = None):
        """Writes the resident poses/points into prob (default: the problem given at creation)."""
        cs = (prob or self.prob).c_state()
        _check(lib().mpsfm_ba_get_state(self._h, C.byref(cs)))

    def eval_cost(self) -> tuple[float, float]:
        a, b = C.c_double(0), C.c_double(0)
        _check(lib().mpsfm_ba_eval_cost(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    @property
    def reduced_dim(self) -> int:
        return int(lib().mpsfm_ba_reduced_dim(self._h))

    def dense_plan(self) -> dict:
        """How the handle factors the reduced camera system (slot order, elimination-tree levels, launch counts)."""
        v = (C.c_int64 * 10)()
        _check(lib().mpsfm_ba_dense_plan(self._h, v))
        keys = ["slots", "tile_columns", "levels", "nd_depth", "inverse_accumulators", "work_items", "tile_products", "inverse_roles",
                "s_blocks", "backsub_launches"]
        return dict(zip(keys, (int(x) for x in v)))

    def pt_handoff(self) -> bool:
        """True when the handle's track sweep hands the landmark factors to its update sweep, False when that sweep recomputes them."""
        return bool(lib().mpsfm_debug_pt_handoff(self._h))

    def direct_front(self) -> bool:
        """True when a solve on this handle, under the switches set now, adds the slab sums straight into the tiles of the dense
        solve; False when it launches k_assemble."""
        return bool(lib().mpsfm_debug_direct_front(self._h))

    def direct_assemble(self, radius: float = 1e4) -> dict:
        """One track sweep and slab reduction at `radius` in both forms.  parent / direct: the tiles [tile][32][32] behind k_assemble and
        of the direct form (undamped, padding diagonals zero); damp [32 nt]: what the first level launch adds to the diagonal, -1 for a padding
        column (set to 1); live [tile]; nt, n; unzeroed: words of the inverse accumulators and y the direct form did not leave zero."""
        nt = self.dense_plan()["tile_columns"]
        ntiles = (nt + 1) * (nt + 2) // 2
        ap, ad = np.zeros((ntiles, 32, 32)), np.zeros((ntiles, 32, 32))
        damp, live, info = np.zeros(32 * nt), np.zeros(ntiles, np.uint8), np.zeros(4, np.int64)
        _check(lib().mpsfm_debug_direct_assemble(self._h, float(radius), ap.ctypes.data, ad.ctypes.data, damp.ctypes.data, live.ctypes.data, info.ctypes.data))
        assert int(info[0]) == nt
        return dict(parent=ap, direct=ad, damp=damp, live=live.astype(bool), nt=nt, n=int(info[1]), n_live=int(info[2]), unzeroed=int(info[3]))

    def debug_table(self, which: int, dtype) -> np.ndarray:
        """Table `which` of the handle (the codes of mpsfm_debug_table) as an array of `dtype`."""
        return _table(lambda out, cap: lib().mpsfm_debug_table(self._h, which, out, cap), dtype)

    def sweep_order(self) -> np.ndarray:
        """The chunk every workgroup of the dense track sweep takes, in launch order (heaviest first)."""
        return self.debug_table(35, np.int32)

    def sweep_once(self, radius: float = 1e4) -> float:
        ms = C.c_float(0)
        _check(lib().mpsfm_ba_sweep_once(self._h, radius, C.byref(ms)))
        return ms.value

    def sweep_parts(self) -> dict:
        """HIP-event times of the parts of the last sweep_once and the chunk counts behind them."""
        ms, info = (C.c_float * 3)(), (C.c_int64 * 4)()
        _check(lib().mpsfm_ba_sweep_parts(self._h, ms, info))
        return dict(dense_ms=ms[0], reduce_ms=ms[1], general_ms=ms[2], dense_chunks=int(info[0]), general_chunks=int(info[1]),
                    long_tracks=int(info[2]), reduce_parts=int(info[3]))

    def dense_solve_once(self) -> float:
        ms = C.c_float(0)
        _check(lib().mpsfm_ba_dense_solve_once(self._h, C.byref(ms)))
        return ms.value

    def dense_solve_given(self, S: np.ndarray, rhs: np.ndarray) -> bool:
        """dense_solve_once on the given system (caller's camera order, zero outside the handle's block pattern) instead of the last
        sweep's; True when the factorisation met a pivot that is not positive.  Needs one sweep_once before it."""
        n = self.reduced_dim
        S, rhs = np.ascontiguousarray(S, np.float64), np.ascontiguousarray(rhs, np.float64)
        assert S.shape == (n, n) and rhs.shape == (n,)
        failed = C.c_int32(0)
        _check(lib().mpsfm_debug_dense_solve_given(self._h, S.ctypes.data, rhs.ctypes.data, n, C.byref(failed)))
        return bool(failed.value)

    def reduced_system(self):
        n = self.reduced_dim
        S, rhs = np.zeros((n, n)), np.zeros(n)
        _check(lib().mpsfm_ba_get_reduced_system(self._h, S.ctypes.data, rhs.ctypes.data, n))
        return S, rhs

    def dense_solution(self):
        n = self.reduced_dim
        y = np.zeros(n)
        _check(lib().mpsfm_ba_get_dense_solution(self._h, y.ctypes.data, n))
        return y

    UPDATE_SCALARS = ("cand_cost", "bad", "mcc", "step_sq_pts", "xn_sq_pts", "step_sq_cams", "xn_sq_cams", "gmax_cams")

    def update_once(self, radius: float, yc: np.ndarray, handoff: bool = False, fused_cam: bool = False) -> dict:
        """One update sweep at the handle's state, `radius` and the given camera step `yc` (scaled coordinates, the order of
        dense_solution()), behind a track sweep at `radius`; handoff: the landmark factors come from that track sweep, otherwise the
        update sweep recomputes them; fused_cam: workgroup 0 of the update sweep forms the candidate cameras, otherwise k_cam_update.
        A form the handle cannot take raises (MPSFM_EUNSUPPORTED).  Returns pts2 (caller's landmark order), q2, t2, part2 (the rows of
        the chunks and long tracks, columns as UPDATE_SCALARS[:5]), the eight scalars by name, the state (pts, q, t) and the column scales the
        sweeps ran with (cs, ps).  The handle's state is unchanged."""
        n = self.reduced_dim
        yc = np.ascontiguousarray(yc, np.float64)
        assert yc.shape == (n,), (yc.shape, n)
        info = (C.c_int64 * 4)()
        _check(lib().mpsfm_ba_sweep_parts(self._h, None, info))
        rows = int(info[0] + info[1] + info[2])
        st = self.prob.copy()
        self.get_state(st)  # what a landmark no block references keeps
        pts2, q2, t2 = st.pts.copy(), np.full((self.prob.n_cams, 4), np.nan), np.full((self.prob.n_cams, 3), np.nan)
        part2, scal = np.full((rows, 8), np.nan), np.full(8, np.nan)
        cs, ps = np.zeros((self.prob.n_cams, 6)), np.zeros((self.prob.n_pts, 3))  # (an unreferenced landmark is no variable: scale 0)
        _check(lib().mpsfm_debug_update_once(self._h, float(radius), yc.ctypes.data, n, int(bool(handoff)) | (int(bool(fused_cam)) << 1), pts2.ctypes.data,
                                             q2.ctypes.data, t2.ctypes.data, part2.ctypes.data, rows, scal.ctypes.data, cs.ctypes.data, ps.ctypes.data))
        out = dict(pts2=pts2, q2=q2, t2=t2, part2=part2[:, :5], pts=st.pts, q=st.cam_quat, t=st.cam_t, cs=cs, ps=ps)
        out.update({k: float(v) for k, v in zip(self.UPDATE_SCALARS, scal)})
        return out


def _table(call, dtype) -> np.ndarray:
    n = int(call(None, 0))
    if n < 0:
        raise MpsfmHipError(n, (lib().mpsfm_last_error() or b"").decode())
    buf = np.zeros(max(n, 1), np.uint8)
    if n > 0 and int(call(buf.ctypes.data, n)) != n:
        raise MpsfmHipError(-1, "table changed size between two reads")
    return buf[:n].view(dtype).copy()


def host_build_table(prob: BAProblem, which: int, dtype) -> np.ndarray:
    """Table `which` (the codes of mpsfm_debug_table) from the host phases of the table build alone: no device involved."""
    cp = prob.c_problem()
    return _table(lambda out, cap: lib().mpsfm_debug_host_build(C.byref(cp), which, out, cap), dtype)


def ba_solve(prob: BAProblem, options: COptions | None = None) -> dict:
    """One-shot mpsfm_ba_solve: refines prob.cam_quat / cam_t / pts in place."""
    o = options if options is not None else default_options()
    cp, cs, sm = prob.c_problem(), prob.c_state(), CSummary()
    _check(lib().mpsfm_ba_solve(C.byref(cp), C.byref(cs), C.byref(o), C.byref(sm)))
    return sm.to_dict()


def point_covs(prob: BAProblem, device: int = 0) -> np.ndarray:
    covs = np.zeros((prob.n_pts, 3, 3))
    cp, cs = prob.c_problem(), prob.c_state()
    _check(lib().mpsfm_point_covs(C.byref(cp), C.byref(cs), device, covs.ctypes.data))
    return covs


def debug_panel_factor(dx: np.ndarray, waves: int = 4):
    """Probe of the dense solve's panel factorisation: one workgroup factors the stacked 64 x 32 matrix [D; X] with `waves`
    (1 or 4) waves.  Returns (out, ok): rows 0..31 of out hold L (lower triangle), rows 32..63 X L^-T; ok is False when a
    pivot was not positive."""
    dx = np.ascontiguousarray(dx, np.float64)
    assert dx.shape == (64, 32), dx.shape
    out, ok = np.zeros((64, 32)), C.c_int(0)
    _check(lib().mpsfm_debug_panel_factor(dx.ctypes.data, int(waves), out.ctypes.data, C.byref(ok)))
    return out, bool(ok.value)


def debug_lm_constants() -> dict:
    """Sizes the decision kernels are built with: bytes of the control block's head and of the whole block, slots of the all-reduced
    scalar tail, threads of k_lm_reduce_decide.  No device involved."""
    info = np.zeros(4, np.int64)
    _check(lib().mpsfm_debug_lm_decide(0, None, None, None, None, None, None, 0, 0, None, None, info.ctypes.data))
    return dict(head_bytes=int(info[0]), ctl_bytes=int(info[1]), redsc_slots=int(info[2]), reduce_threads=int(info[3]))


LM_DECIDE_FORMS = {"scalars": 0, "redsc": 1, "reduce": 2}


def debug_lm_decide(ctl: CDebugLmCtl, opts: CDebugLmOpts, scal, form: str = "scalars", redsc=None, part=None, part2=None, fill: int = 0xA5):
    """One launch of a decision kernel of the trust-region loop on the block `ctl`: k_lm_decide on the 16 scalars ("scalars"), k_lm_decide
    with the all-reduced tail `redsc` ("redsc"), or k_lm_reduce_decide on the partial tables part [rows][4], part2 [rows][8] ("reduce").
    The pinned host copy starts as the byte `fill`.  Returns (device block, host copy, the scalars as the kernel left them)."""
    scal = np.array(scal, np.float64)
    assert scal.shape == (16,)
    rows = 0
    if form == "redsc":
        redsc = np.ascontiguousarray(redsc, np.float64)
        assert redsc.shape == (debug_lm_constants()["redsc_slots"],)
    if form == "reduce":
        part, part2 = np.ascontiguousarray(part, np.float64), np.ascontiguousarray(part2, np.float64)
        rows = part.shape[0]
        assert part.shape == (rows, 4) and part2.shape == (rows, 8)
    dev, host = CDebugLmCtl(), CDebugLmCtl()
    _check(lib().mpsfm_debug_lm_decide(LM_DECIDE_FORMS[form], C.addressof(ctl), C.addressof(opts), scal.ctypes.data,
                                       redsc.ctypes.data if form == "redsc" else None, part.ctypes.data if rows else None,
                                       part2.ctypes.data if rows else None, rows, int(fill), C.addressof(dev), C.addressof(host), None))
    return dev, host, scal


def debug_resources(device: int = 0) -> tuple:
    """(live device blocks, their bytes, outstanding pooled streams, events, pinned blocks) of this process on `device`."""
    out = np.zeros(5, np.int64)
    _check(lib().mpsfm_debug_resources(int(device), out.ctypes.data))
    return tuple(int(v) for v in out)


def triangulate_tracks(tr: Tracks, device: int = 0) -> np.ndarray:
    xyz = np.zeros((tr.n_tracks, 3))
    ct = tr.c_tracks()
    _check(lib().mpsfm_triangulate_tracks(C.byref(ct), device, xyz.ctypes.data))
    return xyz


def filter_tracks(tr: Tracks, xyz: np.ndarray, device: int = 0):
    xyz = np.ascontiguousarray(xyz, np.float64)
    ang, err, front = np.zeros(tr.n_tracks), np.zeros(tr.n_el), np.zeros(tr.n_el, np.uint8)
    ct = tr.c_tracks()
    _check(lib().mpsfm_filter_tracks(C.byref(ct), xyz.ctypes.data, device, ang.ctypes.data, err.ctypes.data, front.ctypes.data))
    return ang, err, front.astype(bool)


def lift_tracks(tr: Tracks, xyz, activated, depth_maps, valid_maps, sx, sy, min_angle_deg, device=0) -> dict:
    """mpsfm_lift_tracks: the depth lifting of the low-parallax points among `tr` in one call.  `activated`, `depth_maps`,
    `valid_maps`, `sx`, `sy`: one entry per camera of `tr`; the maps of a camera that is not activated may be None.
    Returns dict(risky bool [n_tracks], lift_el int32 [n_tracks] (-1: no lift), lift_depth [n_tracks], lift_xyz [n_tracks,3],
    el_keep bool [n_el], info dict)."""
    n_cams = tr.cam_quat.shape[0]
    if not (len(activated) == len(depth_maps) == len(valid_maps) == len(sx) == len(sy) == n_cams):
        raise ValueError("lift_tracks: one entry per camera of the tracks")
    xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    if len(xyz) != tr.n_tracks:
        raise ValueError("lift_tracks: one point per track")
    act = np.ascontiguousarray(activated, np.uint8)
    dm = [None if m is None else np.ascontiguousarray(m, np.float64) for m in depth_maps]
    vm = [None if m is None else np.ascontiguousarray(m.view(np.uint8) if getattr(m, "dtype", None) == np.bool_ else m, np.uint8) for m in valid_maps]
    for d, v in zip(dm, vm):
        if d is not None and v is not None and (d.ndim != 2 or d.shape != v.shape):
            raise ValueError("lift_tracks: depth and valid maps must be [H,W] arrays of one shape")
    hh = np.array([0 if m is None else m.shape[0] for m in dm], np.int32)
    ww = np.array([0 if m is None else m.shape[1] for m in dm], np.int32)
    sx, sy = np.ascontiguousarray(sx, np.float64), np.ascontiguousarray(sy, np.float64)
    dptr = (C.c_void_p * max(n_cams, 1))(*[None if m is None else m.ctypes.data for m in dm])
    vptr = (C.c_void_p * max(n_cams, 1))(*[None if m is None else m.ctypes.data for m in vm])
    M = CLiftMaps()
    M.activated, M.map_h, M.map_w = act.ctypes.data, hh.ctypes.data, ww.ctypes.data
    M.depth_map, M.valid_map = C.addressof(dptr), C.addressof(vptr)
    M.sx, M.sy = sx.ctypes.data, sy.ctypes.data
    nt, ne = tr.n_tracks, tr.n_el
    risky, keep = np.zeros(nt, np.uint8), np.zeros(ne, np.uint8)
    lift_el, lift_depth, lift_xyz = np.full(nt, -1, np.int32), np.zeros(nt), np.zeros((nt, 3))
    I = CLiftInfo()
    ct = tr.c_tracks()
    _check(lib().mpsfm_lift_tracks(C.byref(ct), xyz.ctypes.data, C.byref(M), float(np.deg2rad(float(min_angle_deg))), int(device),
                                   risky.ctypes.data, lift_el.ctypes.data, lift_depth.ctypes.data, lift_xyz.ctypes.data, keep.ctypes.data,
                                   C.byref(I)))
    info = {k: getattr(I, k) for k, _ in CLiftInfo._fields_}
    return dict(risky=risky.astype(bool), lift_el=lift_el, lift_depth=lift_depth, lift_xyz=lift_xyz, el_keep=keep.astype(bool), info=info)


def _depth_gather(depth_maps, valid_maps, sx, sy, cam_quat, cam_t, obs_img, obs_xy, obs_var, obs_pt, pts, scale_filter_factor, multiplier):
    """Fills a CDepthGather; returns (G, the arrays it points into, n_images, n_obs)."""
    n_img = len(depth_maps)
    dm = [np.ascontiguousarray(m, np.float64) for m in depth_maps]
    vm = [np.ascontiguousarray(m, np.uint8) for m in valid_maps]
    hh = np.array([m.shape[0] for m in dm], np.int32)
    ww = np.array([m.shape[1] for m in dm], np.int32)
    f64 = lambda a, shape=None: np.ascontiguousarray(a, np.float64).reshape(shape) if shape else np.ascontiguousarray(a, np.float64)  # noqa: E731
    sx, sy, cam_quat, cam_t = f64(sx), f64(sy), f64(cam_quat, (-1, 4)), f64(cam_t, (-1, 3))
    obs_img, obs_pt = np.ascontiguousarray(obs_img, np.int32), np.ascontiguousarray(obs_pt, np.int32)
    obs_xy, obs_var, pts = f64(obs_xy, (-1, 2)), f64(obs_var), f64(pts, (-1, 3))
    n = len(obs_img)
    G = CDepthGather()
    G.n_images = n_img
    G.map_h, G.map_w = hh.ctypes.data, ww.ctypes.data
    dptr = (C.c_void_p * max(n_img, 1))(*[m.ctypes.data for m in dm])
    vptr = (C.c_void_p * max(n_img, 1))(*[m.ctypes.data for m in vm])
    G.depth_map, G.valid_map = C.addressof(dptr), C.addressof(vptr)
    G.sx, G.sy, G.cam_quat_xyzw, G.cam_t = sx.ctypes.data, sy.ctypes.data, cam_quat.ctypes.data, cam_t.ctypes.data
    G.n_obs = n
    G.obs_img, G.obs_xy, G.obs_var, G.obs_pt = obs_img.ctypes.data, obs_xy.ctypes.data, obs_var.ctypes.data, obs_pt.ctypes.data
    G.n_pts, G.pts = len(pts), pts.ctypes.data
    G.scale_filter, G.scale_filter_factor, G.gross_outliers, G.multiplier = 1, float(scale_filter_factor), 0, float(multiplier)
    return G, (dm, vm, hh, ww, sx, sy, cam_quat, cam_t, obs_img, obs_pt, obs_xy, obs_var, pts, dptr, vptr), n_img, n


def depth_blocks(depth_maps, valid_maps, sx, sy, cam_quat, cam_t, obs_img, obs_xy, obs_var, obs_pt, pts, scale_filter_factor=1.5,
                 multiplier=2.0, device=0):
    """mpsfm_depth_blocks: the depth-block selection of a whole bundle in one launch.  `depth_maps` / `valid_maps`: one
    [H,W] array per image.  Returns dict(flags uint8 [n], depth, depth3d, magnitude, param, whitened float64 [n])."""
    G, _keep, n_img, n = _depth_gather(depth_maps, valid_maps, sx, sy, cam_quat, cam_t, obs_img, obs_xy, obs_var, obs_pt, pts,
                                       scale_filter_factor, multiplier)
    out = {k: np.zeros(n) for k in ("depth", "depth3d", "magnitude", "param", "whitened")}
    out["flags"] = np.zeros(n, np.uint8)
    _check(lib().mpsfm_depth_blocks(C.byref(G), device, out["flags"].ctypes.data, out["depth"].ctypes.data, out["depth3d"].ctypes.data,
                                    out["magnitude"].ctypes.data, out["param"].ctypes.data, out["whitened"].ctypes.data))
    return out


STATS_FIT, STATS_SIGMA = 1, 2              # MPSFM_DEPTH_STATS_FIT / _SIGMA
STATS_EMPTY, STATS_EMPTY_METRIC = 1, 2     # flag bits of a fitted image
SEL_VALID, SEL_FIT, SEL_SIGMA = 1, 2, 4    # bits of `selected`


def depth_stats(depth_maps, valid_maps, sx, sy, cam_quat, cam_t, obs_img, obs_xy, obs_var, obs_pt, pts, what=STATS_FIT | STATS_SIGMA,
                mode=None, filter=None, im_scale=None, map_scale=None, scale_filter_factor=1.5, per_obs=False, device=0):
    """mpsfm_depth_stats: the per-image prior scale fit (what & STATS_FIT) and the whole-call robust sigma (what & STATS_SIGMA)
    with exact medians selected on the device.  The arguments of depth_blocks plus, per image, `mode` (0 skip / 1 fit; default 1),
    `filter` (0 none / 1 scale / 2 metric scale; default 0), `im_scale` and `map_scale` (default 1).  `obs_img` must not decrease.
    Returns dict(n_valid, n_sel, n_nan int64 [n_img], ratio_lo, ratio_hi float64 [n_img], flags uint32 [n_img], sigma_n_sel,
    sigma_n_nan, mu, mad) — the keys of the parts asked for — and with per_obs also ratio, whitened float64 [n], selected uint8 [n]."""
    G, _keep, n_img, n = _depth_gather(depth_maps, valid_maps, sx, sy, cam_quat, cam_t, obs_img, obs_xy, obs_var, obs_pt, pts,
                                       scale_filter_factor, 1.0)
    per_image = lambda a, dtype, fill: np.full(n_img, fill, dtype) if a is None else np.ascontiguousarray(a, dtype)  # noqa: E731
    mode, filter = per_image(mode, np.uint8, 1), per_image(filter, np.uint8, 0)
    im_scale, map_scale = per_image(im_scale, np.float64, 1.0), per_image(map_scale, np.float64, 1.0)
    if not (len(mode) == len(filter) == len(im_scale) == len(map_scale) == n_img):
        raise ValueError("mode, filter, im_scale and map_scale take one entry per image")
    counts, ratio2, flags = np.zeros((max(n_img, 1), 3), np.int64), np.zeros((max(n_img, 1), 2)), np.zeros(max(n_img, 1), np.uint32)
    s_counts, s_stats = np.zeros(2, np.int64), np.zeros(2)
    obs = dict(ratio=np.zeros(n), whitened=np.zeros(n), selected=np.zeros(n, np.uint8)) if per_obs else {}
    ptr = lambda k: obs[k].ctypes.data if per_obs else None  # noqa: E731
    _check(lib().mpsfm_depth_stats(C.byref(G), int(what), mode.ctypes.data, filter.ctypes.data, im_scale.ctypes.data, map_scale.ctypes.data,
                                   int(device), counts.ctypes.data, ratio2.ctypes.data, flags.ctypes.data, s_counts.ctypes.data,
                                   s_stats.ctypes.data, ptr("ratio"), ptr("whitened"), ptr("selected")))
    out = dict(obs)
    if what & STATS_FIT:
        out.update(n_valid=counts[:n_img, 0].copy(), n_sel=counts[:n_img, 1].copy(), n_nan=counts[:n_img, 2].copy(),
                   ratio_lo=ratio2[:n_img, 0].copy(), ratio_hi=ratio2[:n_img, 1].copy(), flags=flags[:n_img].copy())
    if what & STATS_SIGMA:
        out.update(sigma_n_sel=int(s_counts[0]), sigma_n_nan=int(s_counts[1]), mu=float(s_stats[0]), mad=float(s_stats[1]))
    return out


INT_DEFAULT_CONF = dict(
    large_number=1e6, max_iter=10, tol=5e-2, step_size=1, cg_max_iter=5000, cg_tol=1e-3, lambda1=1, lambda2=1, k=1,
    depth_magnitude_multiplier=1, normals_magnitude_multiplier=1, scale_filter=True, scale_filter_factor=1.5,
)


def _int_problem(depth_prior, depth_uncertainty, valid, normals, normals_var, depth_init, K, kps, depth3d, zvars3d, conf,
                 init=True, integrated=False, energy_old=0.0, wu=None, wv=None):
    """Fills a CIntProblem; returns (P, keepalive tuple, (H, W), wu, wv)."""
    c = dict(INT_DEFAULT_CONF)
    c.update(conf or {})
    f64 = lambda a: np.ascontiguousarray(a, np.float64)  # noqa: E731
    depth_prior, depth_uncertainty, depth_init = f64(depth_prior), f64(depth_uncertainty), f64(depth_init)
    H, W = depth_prior.shape
    valid = np.ascontiguousarray(valid, np.uint8)
    normals, normals_var = f64(normals).reshape(H, W, 3), f64(normals_var).reshape(H, W, 3)
    kps = np.ascontiguousarray(kps, np.int64).reshape(-1, 2)
    sx, sy = np.ascontiguousarray(kps[:, 0], np.int32), np.ascontiguousarray(kps[:, 1], np.int32)
    depth3d, zvars3d = f64(depth3d), f64(zvars3d)
    wu = np.zeros(H * W) if wu is None else f64(wu).copy()
    wv = np.zeros(H * W) if wv is None else f64(wv).copy()
    P = CIntProblem()
    P.H, P.W = H, W
    P.depth_prior, P.depth_uncertainty, P.valid = depth_prior.ctypes.data, depth_uncertainty.ctypes.data, valid.ctypes.data
    P.normals, P.normals_var, P.depth_init = normals.ctypes.data, normals_var.ctypes.data, depth_init.ctypes.data
    P.K = (C.c_double * 4)(*[float(v) for v in K])
    P.n_sparse = len(sx)
    P.sparse_x, P.sparse_y = (sx.ctypes.data, sy.ctypes.data) if len(sx) else (None, None)
    P.sparse_depth3d, P.sparse_zvar = (depth3d.ctypes.data, zvars3d.ctypes.data) if len(sx) else (None, None)
    for k in ("large_number", "tol", "step_size", "cg_tol", "lambda1", "lambda2", "k", "depth_magnitude_multiplier",
              "normals_magnitude_multiplier", "scale_filter_factor"):
        setattr(P, k, float(c[k]))
    P.max_iter, P.cg_max_iter, P.scale_filter = int(c["max_iter"]), int(c["cg_max_iter"]), int(bool(c["scale_filter"]))
    P.init, P.integrated, P.energy_old = int(bool(init)), int(bool(integrated)), float(energy_old or 0.0)
    P.wu, P.wv = wu.ctypes.data, wv.ctypes.data
    keep = (depth_prior, depth_uncertainty, depth_init, valid, normals, normals_var, sx, sy, depth3d, zvars3d)
    return P, keep, (H, W), wu, wv


def integrate_depth(depth_prior, depth_uncertainty, valid, normals, normals_var, depth_init, K, kps, depth3d, zvars3d,
                    conf=None, init=True, integrated=False, energy_old=0.0, wu=None, wv=None, device=0):
    """mpsfm_integrate_depth.  Returns (depth map or None, summary dict, wu, wv)."""
    P, _keep, (H, W), wu, wv = _int_problem(depth_prior, depth_uncertainty, valid, normals, normals_var, depth_init, K, kps,
                                            depth3d, zvars3d, conf, init, integrated, energy_old, wu, wv)
    out = np.zeros((H, W))
    S = CIntSummary()
    _check(lib().mpsfm_integrate_depth(C.byref(P), device, out.ctypes.data, C.byref(S)))
    n = S.irls_iterations
    summary = dict(changed=bool(S.changed), irls_iterations=n, cg_iterations_total=S.cg_iterations_total,
                   integrated=bool(S.integrated_out), energy_old=S.energy_old_out, energy_initial=S.energy_initial,
                   energy_final=S.energy_final, cg_iters=[S.cg_iters[i] for i in range(n)],
                   energies=[S.energies[i] for i in range(n + 1)], ms=S.ms)
    return (out if S.changed else None), summary, wu, wv


def _int_summary_dict(S):
    n = S.irls_iterations
    return dict(changed=bool(S.changed), irls_iterations=n, cg_iterations_total=S.cg_iterations_total,
                integrated=bool(S.integrated_out), energy_old=S.energy_old_out, energy_initial=S.energy_initial,
                energy_final=S.energy_final, cg_iters=[S.cg_iters[i] for i in range(n)],
                energies=[S.energies[i] for i in range(n + 1)], ms=S.ms)


def integrate_depth_batch(items, conf=None, device=0):
    """mpsfm_integrate_depth_batch.  `items`: list of dicts with the arguments of `integrate_depth`
    (depth_prior, depth_uncertainty, valid, normals, normals_var, depth_init, K, kps, depth3d, zvars3d and
    optionally init, integrated, energy_old, wu, wv); all maps of one size.  Returns a list of
    (depth map or None, summary dict, wu, wv) in the same order."""
    n = len(items)
    if n == 0:
        return []
    Ps = (CIntProblem * n)()
    Ss = (CIntSummary * n)()
    keep, outs, wus, wvs = [], [], [], []
    for i, it in enumerate(items):
        P, k, (H, W), wu, wv = _int_problem(it["depth_prior"], it["depth_uncertainty"], it["valid"], it["normals"], it["normals_var"],
                                            it["depth_init"], it["K"], it["kps"], it["depth3d"], it["zvars3d"], conf,
                                            it.get("init", True), it.get("integrated", False), it.get("energy_old", 0.0),
                                            it.get("wu"), it.get("wv"))
        Ps[i] = P
        keep.append(k)
        outs.append(np.zeros((H, W)))
        wus.append(wu)
        wvs.append(wv)
    ptrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    _check(lib().mpsfm_integrate_depth_batch(n, C.byref(Ps), device, C.byref(ptrs), C.byref(Ss)))
    return [((outs[i] if Ss[i].changed else None), _int_summary_dict(Ss[i]), wus[i], wvs[i]) for i in range(n)]


def integration_variances(depth_prior, depth_uncertainty, valid, normals, normals_var, depth_checkpoint, K, query_xy,
                          kps=None, depth3d=None, zvars3d=None, use_sparse=False, conf=None, rtol=1e-10, max_iter=50000,
                          device=0, return_field=False):
    """mpsfm_integration_variances: var(log depth) propagated through the integration at integer pixels
    `query_xy` [n,2] (x, y).  Returns (variances [n], summary dict[, field [H,W]])."""
    empty = np.zeros((0, 2), np.int64)
    P, _keep, (H, W), _, _ = _int_problem(depth_prior, depth_uncertainty, valid, normals, normals_var, depth_checkpoint, K,
                                          empty if kps is None else kps, [] if depth3d is None else depth3d,
                                          [] if zvars3d is None else zvars3d, conf, init=False)
    q = np.ascontiguousarray(query_xy, np.int64).reshape(-1, 2)
    qx, qy = np.ascontiguousarray(q[:, 0], np.int32), np.ascontiguousarray(q[:, 1], np.int32)
    out = np.zeros(len(q))
    field = np.zeros((H, W)) if return_field else None
    S = CIntSummary()
    _check(lib().mpsfm_integration_variances(C.byref(P), device, int(bool(use_sparse)), len(q), qx.ctypes.data if len(q) else None,
                                             qy.ctypes.data if len(q) else None, float(rtol), int(max_iter),
                                             out.ctypes.data if len(q) else None, field.ctypes.data if return_field else None,
                                             C.byref(S)))
    summary = dict(converged=bool(S.changed), cg_iterations=S.cg_iterations_total, ms=S.ms)
    return (out, summary, field) if return_field else (out, summary)


def tri_estimate_batch(cand_start, view_cam_from_world, view_intr, view_xy, min_tri_angle, max_error, residual_type=0,
                       min_num_trials=None, device=0):
    """mpsfm_tri_estimate_batch: COLMAP's EstimateTriangulation for many candidate tracks in one launch.
    Returns (xyz [n,3], ok [n] bool, inlier [n_views] bool)."""
    cs = np.ascontiguousarray(cand_start, np.int64)
    n = len(cs) - 1
    P = np.ascontiguousarray(view_cam_from_world, np.float64).reshape(-1, 12)
    K = np.ascontiguousarray(view_intr, np.float64).reshape(-1, 4)
    xy = np.ascontiguousarray(view_xy, np.float64).reshape(-1, 2)
    if len(cs) and int(cs[0]) != 0:  # the library's own check, made before the arrays below are sized from cs[-1]
        raise MpsfmHipError(-1, "cand_start[0] must be 0")
    if not (len(P) == len(K) == len(xy) == (int(cs[-1]) if n >= 0 and len(cs) else 0)):
        raise ValueError("view arrays do not match cand_start")
    mt = None if min_num_trials is None else np.ascontiguousarray(min_num_trials, np.int64)
    c = CTriCandidates(n, cs.ctypes.data, P.ctypes.data, K.ctypes.data, xy.ctypes.data, float(min_tri_angle), float(max_error),
                       int(residual_type), None if mt is None else mt.ctypes.data)
    xyz, ok, inl = np.zeros((max(n, 0), 3)), np.zeros(max(n, 0), np.uint8), np.zeros(len(P), np.uint8)
    _check(lib().mpsfm_tri_estimate_batch(C.byref(c), device, xyz.ctypes.data, ok.ctypes.data, inl.ctypes.data))
    return xyz, ok.astype(bool), inl.astype(bool)


DC_IN, DC_SURFACE, DC_OCCL, DC_INVALID = 1, 2, 4, 8  # code bits of depth_consistency(return_codes=True)


def depth_consistency(images, pairs, c=15.0, score_thresh=0.6, device=0, return_codes=False):
    """mpsfm_depth_consistency: both legs of every pair (a, b) in one launch sequence.

    `images`: list of dicts with depth [H,W] float64 (C-contiguous; values <= 0 are set to 0.1 IN PLACE, as the reference
    does), variance [H,W], prior_std_multiplier, intr_scaled (fx sx, fy sy, cx sx, cy sy), intr (fx fy cx cy) and
    cam_from_world [3,4].  `pairs`: list of (a, b) indices into `images`.
    Returns (counts int64 [n_pairs, 2, 4] = {in canvas, surface, occluded, invalid} per leg (0: a -> b, 1: b -> a),
    summary dict[, codes: list over pairs of (codes of a [Ha,Wa], codes of b [Hb,Wb]) uint8]) ."""
    n_img, n_pairs = len(images), len(pairs)
    arr = (CDcImage * max(n_img, 1))()
    keep = []
    for k, im in enumerate(images):
        d = im["depth"]
        if not (isinstance(d, np.ndarray) and d.dtype == np.float64 and d.ndim == 2 and d.flags.c_contiguous and d.flags.writeable):
            raise ValueError("depth maps must be writable C-contiguous float64 [H, W] arrays (the clamp is written back)")
        v = np.ascontiguousarray(im["variance"], np.float64)
        if v.shape != d.shape:
            raise ValueError("variance and depth maps differ in shape")
        keep.append(v)
        e = arr[k]
        e.H, e.W = d.shape
        e.depth, e.variance = d.ctypes.data, v.ctypes.data
        e.prior_std_multiplier = float(im["prior_std_multiplier"])
        e.intr_scaled = (C.c_double * 4)(*[float(x) for x in im["intr_scaled"]])
        e.intr = (C.c_double * 4)(*[float(x) for x in im["intr"]])
        e.cam_from_world = (C.c_double * 12)(*[float(x) for x in np.asarray(im["cam_from_world"], np.float64).reshape(12)])
    pa = np.ascontiguousarray([p[0] for p in pairs], np.int32)
    pb = np.ascontiguousarray([p[1] for p in pairs], np.int32)
    counts = np.zeros((n_pairs, 2, 4), np.int64)
    codes, cptr = None, None
    if return_codes:
        codes = []
        for a, b in pairs:
            sa = images[a]["depth"].shape if 0 <= a < n_img else (0, 0)
            sb = images[b]["depth"].shape if 0 <= b < n_img else (0, 0)
            codes.append((np.zeros(sa, np.uint8), np.zeros(sb, np.uint8)))
        cptr = (C.c_void_p * max(2 * n_pairs, 1))(*[m.ctypes.data for cd in codes for m in cd])
    S = CDcSummary()
    _check(lib().mpsfm_depth_consistency(n_img, C.addressof(arr), n_pairs, pa.ctypes.data, pb.ctypes.data, float(c),
                                         float(score_thresh), int(device), counts.ctypes.data,
                                         C.addressof(cptr) if cptr is not None else None, C.byref(S)))
    summary = dict(ms=S.ms, n_legs=S.n_legs, n_pixels=S.n_pixels)
    return (counts, summary, codes) if return_codes else (counts, summary)


def _ransac_options(defaults: dict, options: dict) -> CRansacOptions:
    """`options` over `defaults` as the C struct; a key that is not in `defaults` is a KeyError."""
    o = dict(defaults)
    unknown = set(options) - set(o)
    if unknown:
        raise KeyError(f"unknown option(s) {sorted(unknown)}")
    o.update(options)
    return CRansacOptions(float(o["max_error"]), float(o["min_inlier_ratio"]), float(o["confidence"]), float(o["dyn_num_trials_multiplier"]),
                          int(o["min_num_trials"]), int(o["max_num_trials"]), int(o["seed"]) & ((1 << 64) - 1), int(o["batch_trials"]), 0)


def _ransac_report(R, mask: np.ndarray, n: int) -> dict:
    """The result fields both estimators report."""
    return dict(success=bool(R.success), num_inliers=int(R.num_inliers), inlier_mask=mask[:n].astype(bool), num_trials=int(R.num_trials),
                max_num_trials=int(R.max_num_trials), num_models=int(R.num_models), lo_rounds=int(R.lo_rounds),
                num_batches=int(R.num_batches), ms=float(R.ms))


ABS_POSE_DEFAULTS = dict(max_error=12.0, min_inlier_ratio=0.25, confidence=0.99999, dyn_num_trials_multiplier=3.0, min_num_trials=100,
                         max_num_trials=10000, seed=0, batch_trials=0)


def abs_pose_estimate(points2D, points3D, intr, device=0, **options) -> dict:
    """mpsfm_abs_pose_estimate: LO-RANSAC (P3P + EPnP) of one 2D-3D problem with PINHOLE intr = (fx, fy, cx, cy).
    `options`: keys of ABS_POSE_DEFAULTS.  Returns dict(success, cam_from_world [3,4], num_inliers, inlier_mask bool [n],
    num_trials, max_num_trials, num_models, lo_rounds, num_batches, ms)."""
    opt = _ransac_options(ABS_POSE_DEFAULTS, options)
    p2 = np.ascontiguousarray(points2D, np.float64).reshape(-1, 2)
    p3 = np.ascontiguousarray(points3D, np.float64).reshape(-1, 3)
    if len(p2) != len(p3):
        raise ValueError("points2D and points3D differ in length")
    K = np.ascontiguousarray(intr, np.float64).reshape(4)
    n = len(p2)
    mask = np.zeros(max(n, 1), np.uint8)
    R = CAbsPoseResult()
    _check(lib().mpsfm_abs_pose_estimate(n, p2.ctypes.data, p3.ctypes.data, K.ctypes.data, C.byref(opt), int(device), mask.ctypes.data,
                                         C.byref(R)))
    return dict(_ransac_report(R, mask, n), cam_from_world=np.array(R.cam_from_world[:]).reshape(3, 4))


# pycolmap 3.11 RANSACOptions() as recalled
REL_POSE_DEFAULTS = dict(max_error=4.0, min_inlier_ratio=0.01, confidence=0.9999, dyn_num_trials_multiplier=3.0, min_num_trials=1000,
                         max_num_trials=100000, seed=0, batch_trials=0)


def rel_pose_estimate(points1, points2, intr1, intr2, device=0, **options) -> dict:
    """mpsfm_rel_pose_estimate: LO-RANSAC (five-point) of one two-view problem with PINHOLE intr = (fx, fy, cx, cy), then the
    pose.  `options`: keys of REL_POSE_DEFAULTS.  Returns dict(success, E [3,3], cam2_from_cam1 [3,4], num_inliers,
    inlier_mask bool [n], num_trials, max_num_trials, num_models, lo_rounds, num_batches, num_cheirality_points, ms)."""
    opt = _ransac_options(REL_POSE_DEFAULTS, options)
    p1 = np.ascontiguousarray(points1, np.float64).reshape(-1, 2)
    p2 = np.ascontiguousarray(points2, np.float64).reshape(-1, 2)
    if len(p1) != len(p2):
        raise ValueError("points1 and points2 differ in length")
    K1 = np.ascontiguousarray(intr1, np.float64).reshape(4)
    K2 = np.ascontiguousarray(intr2, np.float64).reshape(4)
    n = len(p1)
    mask = np.zeros(max(n, 1), np.uint8)
    R = CRelPoseResult()
    _check(lib().mpsfm_rel_pose_estimate(n, p1.ctypes.data, p2.ctypes.data, K1.ctypes.data, K2.ctypes.data, C.byref(opt), int(device),
                                         mask.ctypes.data, C.byref(R)))
    return dict(_ransac_report(R, mask, n), E=np.array(R.E[:]).reshape(3, 3), cam2_from_cam1=np.array(R.cam2_from_cam1[:]).reshape(3, 4),
                num_cheirality_points=int(R.num_cheirality_points))


# the reference's icp/main.py where it sets a value (pts_bound 0.1, 5000 trials), pycolmap 3.11 RANSACOptions() as recalled otherwise
ALIGN3D_DEFAULTS = dict(max_error=0.1, min_inlier_ratio=0.1, confidence=0.99, dyn_num_trials_multiplier=3.0, min_num_trials=100,
                        max_num_trials=5000, seed=0, batch_trials=0)


def _align3d_report(R, mask: np.ndarray, n: int) -> dict:
    return dict(_ransac_report(R, mask, n), tgt_from_src=np.array(R.tgt_from_src[:]).reshape(3, 4), scale=float(R.scale))


def _point_pairs(src, tgt):
    p = np.ascontiguousarray(src, np.float64).reshape(-1, 3)
    q = np.ascontiguousarray(tgt, np.float64).reshape(-1, 3)
    if len(p) != len(q):
        raise ValueError("src and tgt differ in length")
    return p, q


def align3d_estimate(src, tgt, with_scale=False, device=0, **options) -> dict:
    """mpsfm_align3d_estimate: LO-RANSAC of tgt ~ s R src + t (s = 1 unless with_scale) over [n, 3] point pairs.
    `options`: keys of ALIGN3D_DEFAULTS.  Returns dict(success, tgt_from_src [3,4] = [R | t], scale, num_inliers,
    inlier_mask bool [n], num_trials, max_num_trials, num_models, lo_rounds, num_batches, ms)."""
    opt = _ransac_options(ALIGN3D_DEFAULTS, options)
    p, q = _point_pairs(src, tgt)
    n = len(p)
    mask = np.zeros(max(n, 1), np.uint8)
    R = CAlign3dResult()
    _check(lib().mpsfm_align3d_estimate(n, p.ctypes.data, q.ctypes.data, int(bool(with_scale)), C.byref(opt), int(device), mask.ctypes.data,
                                        C.byref(R)))
    return _align3d_report(R, mask, n)


def align3d_fit(src, tgt, mask=None, with_scale=False, device=0) -> dict:
    """mpsfm_align3d_fit: the least-squares tgt ~ s R src + t over the pairs that `mask` keeps (None: all).  Returns
    dict(success, tgt_from_src [3,4], scale, num_inliers = points used, ms)."""
    p, q = _point_pairs(src, tgt)
    n = len(p)
    sel = None
    if mask is not None:
        sel = np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, np.uint8)
        if len(sel) != n:
            raise ValueError("mask and points differ in length")
    R = CAlign3dResult()
    _check(lib().mpsfm_align3d_fit(n, p.ctypes.data, q.ctypes.data, None if sel is None else sel.ctypes.data, int(bool(with_scale)),
                                   int(device), C.byref(R)))
    return dict(success=bool(R.success), tgt_from_src=np.array(R.tgt_from_src[:]).reshape(3, 4), scale=float(R.scale),
                num_inliers=int(R.num_inliers), ms=float(R.ms))


def _depth_map(depth, intr):
    """A float32 or float64 [H, W] map as the float64 array the library reads (float32 widens exactly), and its intrinsics."""
    d = np.asarray(depth)
    if d.ndim != 2 or d.dtype not in (np.float32, np.float64):
        raise ValueError("a depth map is a float32 or float64 [H, W] array")
    return np.ascontiguousarray(d, np.float64), np.ascontiguousarray(intr, np.float64).reshape(4)


def lift_keypoints(depth, intr, xy, device=0):
    """mpsfm_lift_keypoints: keypoints [n, 2] (pixels of the map) bilinearly sampled from the point map of `depth` [H, W] with
    PINHOLE intr = (fx, fy, cx, cy).  Returns (xyz float64 [n, 3], valid bool [n]); invalid keypoints are zeros."""
    d, K = _depth_map(depth, intr)
    kp = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    n = len(kp)
    xyz, valid = np.zeros((max(n, 1), 3)), np.zeros(max(n, 1), np.uint8)
    _check(lib().mpsfm_lift_keypoints(d.shape[0], d.shape[1], d.ctypes.data, K.ctypes.data, n, kp.ctypes.data, int(device),
                                      xyz.ctypes.data, valid.ctypes.data))
    return xyz[:n], valid[:n].astype(bool)


def depth_pair_register(depth0, intr0, depth1, intr1, xy0, xy1, matches, with_scale=False, device=0, **options) -> dict:
    """mpsfm_depth_pair_register: both ends of matches [m, 2] (keypoint of image 0, of image 1) lifted through their depth maps
    and aligned, source = image 0.  `options`: keys of ALIGN3D_DEFAULTS.  Returns align3d_estimate's dict with inlier_mask
    over the matches, plus valid bool [m], lifted0 and lifted1 float64 [m, 3]."""
    opt = _ransac_options(ALIGN3D_DEFAULTS, options)
    d0, K0 = _depth_map(depth0, intr0)
    d1, K1 = _depth_map(depth1, intr1)
    k0 = np.ascontiguousarray(xy0, np.float64).reshape(-1, 2)
    k1 = np.ascontiguousarray(xy1, np.float64).reshape(-1, 2)
    mt = np.ascontiguousarray(matches, np.int32).reshape(-1, 2)
    m = len(mt)
    valid, mask = np.zeros(max(m, 1), np.uint8), np.zeros(max(m, 1), np.uint8)
    l0, l1 = np.zeros((max(m, 1), 3)), np.zeros((max(m, 1), 3))
    R = CAlign3dResult()
    _check(lib().mpsfm_depth_pair_register(d0.shape[0], d0.shape[1], d0.ctypes.data, K0.ctypes.data, d1.shape[0], d1.shape[1],
                                           d1.ctypes.data, K1.ctypes.data, len(k0), k0.ctypes.data, len(k1), k1.ctypes.data, m,
                                           mt.ctypes.data, int(bool(with_scale)), C.byref(opt), int(device), valid.ctypes.data,
                                           mask.ctypes.data, l0.ctypes.data, l1.ctypes.data, C.byref(R)))
    return dict(_align3d_report(R, mask, m), valid=valid[:m].astype(bool), lifted0=l0[:m], lifted1=l1[:m])


ICP_DEFAULTS = dict(max_distance=0.1, max_angle_deg=30.0, edge_ratio=0.05, eps_rotation=1e-6, eps_translation=1e-6, max_iterations=30,
                    min_pairs=100, stride=1)
ICP_STATUS = ("converged", "max_iterations", "too_few_pairs", "singular")  # MPSFM_ICP_*


def _icp_options(options: dict) -> CIcpOptions:
    o = dict(ICP_DEFAULTS)
    unknown = set(options) - set(o)
    if unknown:
        raise KeyError(f"unknown option(s) {sorted(unknown)}")
    o.update(options)
    return CIcpOptions(float(o["max_distance"]), float(o["max_angle_deg"]), float(o["edge_ratio"]), float(o["eps_rotation"]),
                       float(o["eps_translation"]), int(o["max_iterations"]), int(o["min_pairs"]), int(o["stride"]), 0)


def _icp_report(R, trace: np.ndarray) -> dict:
    it = int(R.iterations)
    return dict(tgt_from_src=np.array(R.tgt_from_src[:]).reshape(3, 4), scale=float(R.scale), info=np.array(R.info[:]).reshape(6, 6),
                rhs=np.array(R.rhs[:]), rmse=float(R.rmse), num_pairs=int(R.num_pairs), rejected=[int(v) for v in R.rejected],
                iterations=it, status=ICP_STATUS[int(R.status)], trace=trace[:it].copy(), ms=float(R.ms))


def depth_normals(depth, intr, edge_ratio=ICP_DEFAULTS["edge_ratio"], device=0):
    """mpsfm_depth_normals: the camera-facing normals of a depth map [H, W] by central differences of its vertex map.  Returns
    (normals float64 [H, W, 3], valid bool [H, W]); pixels without a normal (border, hole, depth edge) are zeros."""
    d, K = _depth_map(depth, intr)
    H, W = d.shape
    normals, valid = np.zeros((H, W, 3)), np.zeros((H, W), np.uint8)
    _check(lib().mpsfm_depth_normals(H, W, d.ctypes.data, K.ctypes.data, float(edge_ratio), int(device), normals.ctypes.data,
                                     valid.ctypes.data))
    return normals, valid.astype(bool)


def depth_pair_icp(depth0, intr0, depth1, intr1, init, scale=1.0, device=0, **options) -> dict:
    """mpsfm_depth_pair_icp: dense point-to-plane ICP of map 0 onto map 1 from init [3, 4] = [R | t] at the fixed `scale`.
    `options`: keys of ICP_DEFAULTS.  Returns dict(tgt_from_src [3,4], scale, info [6,6], rhs [6], rmse, num_pairs, rejected [4],
    iterations, status (a name of ICP_STATUS), trace [iterations, 4] = pair count, rmse, |w|, |v|, ms)."""
    opt = _icp_options(options)
    d0, K0 = _depth_map(depth0, intr0)
    d1, K1 = _depth_map(depth1, intr1)
    T = np.ascontiguousarray(init, np.float64).reshape(12)
    trace = np.zeros((max(int(opt.max_iterations), 1), 4))
    R = CIcpResult()
    _check(lib().mpsfm_depth_pair_icp(d0.shape[0], d0.shape[1], d0.ctypes.data, K0.ctypes.data, d1.shape[0], d1.shape[1], d1.ctypes.data,
                                      K1.ctypes.data, T.ctypes.data, float(scale), C.byref(opt), int(device), trace.ctypes.data, C.byref(R)))
    return _icp_report(R, trace)


def depth_pair_register_dense(depth0, intr0, depth1, intr1, xy0, xy1, matches, with_scale=False, device=0, icp=None, **options) -> dict:
    """mpsfm_depth_pair_register_dense: depth_pair_register, then depth_pair_icp from its model on the maps already on the
    device.  `options`: keys of ALIGN3D_DEFAULTS; `icp`: a dict with keys of ICP_DEFAULTS.  Returns depth_pair_register's dict
    plus refined = depth_pair_icp's dict (None when no model was found)."""
    opt = _ransac_options(ALIGN3D_DEFAULTS, options)
    iopt = _icp_options(dict(icp or {}))
    d0, K0 = _depth_map(depth0, intr0)
    d1, K1 = _depth_map(depth1, intr1)
    k0 = np.ascontiguousarray(xy0, np.float64).reshape(-1, 2)
    k1 = np.ascontiguousarray(xy1, np.float64).reshape(-1, 2)
    mt = np.ascontiguousarray(matches, np.int32).reshape(-1, 2)
    m = len(mt)
    valid, mask = np.zeros(max(m, 1), np.uint8), np.zeros(max(m, 1), np.uint8)
    l0, l1 = np.zeros((max(m, 1), 3)), np.zeros((max(m, 1), 3))
    trace = np.zeros((max(int(iopt.max_iterations), 1), 4))
    R, RI = CAlign3dResult(), CIcpResult()
    _check(lib().mpsfm_depth_pair_register_dense(d0.shape[0], d0.shape[1], d0.ctypes.data, K0.ctypes.data, d1.shape[0], d1.shape[1],
                                                 d1.ctypes.data, K1.ctypes.data, len(k0), k0.ctypes.data, len(k1), k1.ctypes.data, m,
                                                 mt.ctypes.data, int(bool(with_scale)), C.byref(opt), C.byref(iopt), int(device),
                                                 valid.ctypes.data, mask.ctypes.data, l0.ctypes.data, l1.ctypes.data, C.byref(R),
                                                 trace.ctypes.data, C.byref(RI)))
    return dict(_align3d_report(R, mask, m), valid=valid[:m].astype(bool), lifted0=l0[:m], lifted1=l1[:m],
                refined=_icp_report(RI, trace) if R.success else None)


# COLMAP 3.11 TwoViewGeometryOptions as recalled (mpsfm_two_view_default_options)
TWO_VIEW_DEFAULTS = dict(max_error=4.0, min_inlier_ratio=0.25, confidence=0.999, dyn_num_trials_multiplier=3.0, min_num_trials=100,
                         max_num_trials=10000, seed=0, batch_trials=0, min_num_inliers=15, min_E_F_inlier_ratio=0.95,
                         max_H_inlier_ratio=0.8, watermark_min_inlier_ratio=0.7, watermark_border_size=0.1, detect_watermark=True,
                         compute_relative_pose=False)
TWO_VIEW_LEGS = ("E", "F", "H", "T")  # T: the translation of the watermark test


def _two_view_options(options: dict) -> CTwoViewOptions:
    """`options` over TWO_VIEW_DEFAULTS as the C struct; an unknown key is a KeyError."""
    o = dict(TWO_VIEW_DEFAULTS)
    unknown = set(options) - set(o)
    if unknown:
        raise KeyError(f"unknown option(s) {sorted(unknown)}")
    o.update(options)
    ransac = _ransac_options({k: TWO_VIEW_DEFAULTS[k] for k in REL_POSE_DEFAULTS}, {k: o[k] for k in REL_POSE_DEFAULTS})
    return CTwoViewOptions(ransac, int(o["min_num_inliers"]), float(o["min_E_F_inlier_ratio"]), float(o["max_H_inlier_ratio"]),
                           float(o["watermark_min_inlier_ratio"]), float(o["watermark_border_size"]), int(bool(o["detect_watermark"])),
                           int(bool(o["compute_relative_pose"])))


def _two_view_pair(points1, points2, intr1, intr2, size1, size2):
    """The arrays of one pair as the C entry points read them."""
    p1 = np.ascontiguousarray(points1, np.float64).reshape(-1, 2)
    p2 = np.ascontiguousarray(points2, np.float64).reshape(-1, 2)
    if len(p1) != len(p2):
        raise ValueError("points1 and points2 differ in length")
    return (p1, p2, np.ascontiguousarray(intr1, np.float64).reshape(4), np.ascontiguousarray(intr2, np.float64).reshape(4),
            np.ascontiguousarray(size1, np.int32).reshape(2), np.ascontiguousarray(size2, np.int32).reshape(2))


def _two_view_result(R, mask: np.ndarray) -> dict:
    legs = {name: dict(num_inliers=int(g.num_inliers), num_trials=int(g.num_trials), max_num_trials=int(g.max_num_trials),
                       lo_rounds=int(g.lo_rounds), num_batches=int(g.num_batches), success=bool(g.success))
            for name, g in zip(TWO_VIEW_LEGS, R.leg)}
    return dict(config=int(R.config), success=bool(R.success), E=np.array(R.E[:]).reshape(3, 3), F=np.array(R.F[:]).reshape(3, 3),
                H=np.array(R.H[:]).reshape(3, 3), cam2_from_cam1=np.array(R.cam2_from_cam1[:]).reshape(3, 4), tri_angle=float(R.tri_angle),
                inlier_mask=mask.astype(bool), num_inliers=int(R.num_inliers), num_cheirality_points=int(R.num_cheirality_points),
                num_border_inliers=int(R.num_border_inliers), watermark=bool(R.watermark), legs=legs, ms=float(R.ms))


def two_view_geometry(points1, points2, intr1, intr2, size1, size2, device=0, **options) -> dict:
    """mpsfm_two_view_geometry: calibrated two-view geometry of one image pair (E, F and H LO-RANSAC, COLMAP's decision, the
    watermark test, the relative pose) with PINHOLE intr = (fx, fy, cx, cy) and size = (width, height).  `options`: keys of
    TWO_VIEW_DEFAULTS.  Returns dict(config, success, E, F, H [3,3], cam2_from_cam1 [3,4], tri_angle (radians), inlier_mask
    bool [n], num_inliers, num_cheirality_points, num_border_inliers, watermark, legs {E, F, H, T: dict(num_inliers,
    num_trials, max_num_trials, lo_rounds, num_batches, success)}, ms)."""
    opt = _two_view_options(options)
    p1, p2, K1, K2, s1, s2 = _two_view_pair(points1, points2, intr1, intr2, size1, size2)
    n = len(p1)
    mask = np.zeros(max(n, 1), np.uint8)
    R = CTwoViewResult()
    _check(lib().mpsfm_two_view_geometry(n, p1.ctypes.data, p2.ctypes.data, K1.ctypes.data, K2.ctypes.data, s1.ctypes.data, s2.ctypes.data,
                                         C.byref(opt), int(device), mask.ctypes.data, C.byref(R)))
    return _two_view_result(R, mask[:n])


def two_view_geometry_batch(pairs, device=0, pairs_per_group=0, return_report=False, **options):
    """mpsfm_two_view_geometry_batch: the two-view geometry of many image pairs in one call.  `pairs`: a sequence of
    (points1, points2, intr1, intr2, size1, size2) as two_view_geometry takes them; `options` (keys of TWO_VIEW_DEFAULTS) serve
    every pair.  Returns the list of the dicts two_view_geometry returns, each identical to that pair's single call but for
    `ms`, which is the device time of the whole group the pair ran in; with `return_report` also dict(num_groups, num_syncs,
    num_launches, ms) of the call.  `pairs_per_group` 0: the library's default grouping."""
    opt = _two_view_options(options)
    arrs = [_two_view_pair(*p) for p in pairs]
    P = len(arrs)
    start = np.zeros(P + 1, np.int64)
    if P:
        start[1:] = np.cumsum([len(a[0]) for a in arrs])
    N = int(start[-1])

    def cat(k, cols, dtype):
        return np.ascontiguousarray(np.concatenate([a[k].reshape(-1, cols) for a in arrs]), dtype) if P else np.zeros((0, cols), dtype)

    p1, p2 = cat(0, 2, np.float64), cat(1, 2, np.float64)
    K1, K2 = cat(2, 4, np.float64), cat(3, 4, np.float64)
    s1, s2 = cat(4, 2, np.int32), cat(5, 2, np.int32)
    mask = np.zeros(max(N, 1), np.uint8)
    R = (CTwoViewResult * max(P, 1))()
    rep = CTwoViewBatchReport()
    _check(lib().mpsfm_two_view_geometry_batch(P, start.ctypes.data, p1.ctypes.data, p2.ctypes.data, K1.ctypes.data, K2.ctypes.data,
                                               s1.ctypes.data, s2.ctypes.data, C.byref(opt), int(pairs_per_group), int(device),
                                               mask.ctypes.data, R, C.byref(rep)))
    out = [_two_view_result(R[k], mask[start[k]:start[k + 1]]) for k in range(P)]
    if return_report:
        return out, dict(num_groups=int(rep.num_groups), num_syncs=int(rep.num_syncs), num_launches=int(rep.num_launches), ms=float(rep.ms))
    return out


REG_DROPPED, REG_TRIANGULATED, REG_LIFTED = 0, 1, 2  # `kind` of registration_pairs


def registration_pairs(refs, match_ref, ref_xy, match_pt, pts, pt_risky=None, lifted_registration=True, device=0, return_ms=False):
    """mpsfm_registration_pairs: the 2D-3D pairs of one registration for all reference images in one launch.

    `refs`: list of dicts with depth_map [H,W] (depth.data; may be None when lifted_registration is off), sx, sy,
    intr (fx fy cx cy), quat_xyzw and t of cam_from_world.  Per match: `match_ref` index into refs, `ref_xy` keypoint of the
    reference image, `match_pt` index into `pts` [n_pts,3] or -1; `pt_risky` bool [n_pts] or None.
    Returns (xyz [n,3], kind uint8 [n] in REG_*)[, device ms]."""
    match_ref = np.ascontiguousarray(match_ref, np.int32).reshape(-1)
    match_pt = np.ascontiguousarray(match_pt, np.int32).reshape(-1)
    ref_xy = np.ascontiguousarray(ref_xy, np.float64).reshape(-1, 2)
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    n, n_pts, n_refs = len(match_ref), len(pts), len(refs)
    if not (len(ref_xy) == len(match_pt) == n):
        raise ValueError("match_ref, ref_xy and match_pt differ in length")
    if n and (match_ref.min() < 0 or match_ref.max() >= n_refs):
        raise ValueError("match_ref out of range")
    if n and (match_pt.min() < -1 or match_pt.max() >= n_pts):
        raise ValueError("match_pt out of range")
    risky = None
    if pt_risky is not None:
        risky = np.ascontiguousarray(pt_risky, np.uint8).reshape(-1)
        if len(risky) != n_pts:
            raise ValueError("pt_risky must have one entry per point")
    arr = (CRegImage * max(n_refs, 1))()
    keep = []
    for k, r in enumerate(refs):
        e = arr[k]
        if lifted_registration:
            m = np.ascontiguousarray(r["depth_map"], np.float64)
            if m.ndim != 2 or m.shape[0] < 2 or m.shape[1] < 2:
                raise ValueError("depth maps must be [H, W] arrays of at least 2 x 2")
            keep.append(m)
            e.map_h, e.map_w = m.shape
            e.depth_map = m.ctypes.data
        e.sx, e.sy = float(r["sx"]), float(r["sy"])
        e.intr = (C.c_double * 4)(*[float(v) for v in np.asarray(r["intr"], np.float64).reshape(4)])
        e.quat_xyzw = (C.c_double * 4)(*[float(v) for v in np.asarray(r["quat_xyzw"], np.float64).reshape(4)])
        e.t = (C.c_double * 3)(*[float(v) for v in np.asarray(r["t"], np.float64).reshape(3)])
    xyz, kind, ms = np.zeros((n, 3)), np.zeros(n, np.uint8), C.c_float(0)
    _check(lib().mpsfm_registration_pairs(n_refs, C.addressof(arr), n, match_ref.ctypes.data, ref_xy.ctypes.data, match_pt.ctypes.data,
                                          None if risky is None else risky.ctypes.data, n_pts, pts.ctypes.data,
                                          int(bool(lifted_registration)), int(device), xyz.ctypes.data, kind.ctypes.data, C.addressof(ms)))
    return (xyz, kind, float(ms.value)) if return_ms else (xyz, kind)


INIT_TRIANGULATE, INIT_LIFT = 1, 2
INIT_TRI_MAX_ERROR = float(np.deg2rad(2.0))  # EstimateTriangulationOptions.ransac.max_error of pycolmap 3.11 as recalled


def init_pair_candidates(xy1, xy2, intr1, intr2, cam2_from_cam1, prior_map=None, valid_map=None, sx=1.0, sy=1.0, rescale=1.0,
                         select=None, what=INIT_TRIANGULATE | INIT_LIFT, tri_min_angle=0.0, tri_max_error=INIT_TRI_MAX_ERROR,
                         device=0):
    """mpsfm_init_pair_candidates: the triangulated and the lifted candidate point of every match of an init pair (image 1 at
    the identity, image 2 at `cam2_from_cam1` [3,4]) in one launch.  `prior_map` / `valid_map`: depth.data_prior and
    depth.valid of image 1 (needed with INIT_LIFT).  Returns a dict with, per match, tri_ok, tri_xyz, tri_angle_deg,
    tri_posdepth1/2, lift_xyz, lift_angle_deg, lift_posdepth1/2, d_prior, valid, and the device time `ms`; the angle is the
    reference's (see include/mpsfm_hip.h), in degrees."""
    xy1 = np.ascontiguousarray(xy1, np.float64).reshape(-1, 2)
    xy2 = np.ascontiguousarray(xy2, np.float64).reshape(-1, 2)
    n = len(xy1)
    if len(xy2) != n:
        raise ValueError("xy1 and xy2 differ in length")
    what = int(what)
    if what not in (INIT_TRIANGULATE, INIT_LIFT, INIT_TRIANGULATE | INIT_LIFT):
        raise ValueError("what must be INIT_TRIANGULATE, INIT_LIFT or both")
    P = CInitPair()
    P.n_matches, P.xy1, P.xy2 = n, xy1.ctypes.data, xy2.ctypes.data
    sel = None
    if select is not None:
        sel = np.ascontiguousarray(select, np.uint8).reshape(-1)
        if len(sel) != n:
            raise ValueError("select must have one entry per match")
        P.select = sel.ctypes.data
    P.intr1 = (C.c_double * 4)(*[float(v) for v in np.asarray(intr1, np.float64).reshape(4)])
    P.intr2 = (C.c_double * 4)(*[float(v) for v in np.asarray(intr2, np.float64).reshape(4)])
    P.cam2_from_cam1 = (C.c_double * 12)(*[float(v) for v in np.asarray(cam2_from_cam1, np.float64).reshape(12)])
    pm = vm = None
    if what & INIT_LIFT:
        if prior_map is None or valid_map is None:
            raise ValueError("INIT_LIFT needs prior_map and valid_map")
        pm = np.ascontiguousarray(prior_map, np.float64)
        vm = np.ascontiguousarray(np.asarray(valid_map) != 0, np.uint8)
        if pm.ndim != 2 or pm.shape != vm.shape or pm.shape[0] < 2 or pm.shape[1] < 2:
            raise ValueError("prior_map and valid_map must be [H, W] arrays of one shape, at least 2 x 2")
        P.map_h, P.map_w = pm.shape
        P.prior_map, P.valid_map = pm.ctypes.data, vm.ctypes.data
    P.sx, P.sy, P.rescale = float(sx), float(sy), float(rescale)
    P.tri_min_angle, P.tri_max_error, P.what = float(tri_min_angle), float(tri_max_error), what
    flags = np.zeros(n, np.uint8)
    o = {k: np.zeros(s) for k, s in (("tri_xyz", (n, 3)), ("tri_angle_deg", n), ("lift_xyz", (n, 3)), ("lift_angle_deg", n),
                                     ("d_prior", n))}
    O = CInitCandidates(flags.ctypes.data, o["tri_xyz"].ctypes.data, o["tri_angle_deg"].ctypes.data, o["lift_xyz"].ctypes.data,
                        o["lift_angle_deg"].ctypes.data, o["d_prior"].ctypes.data, 0.0)
    _check(lib().mpsfm_init_pair_candidates(C.byref(P), int(device), C.byref(O)))
    for bit, name in enumerate(("tri_ok", "tri_posdepth1", "tri_posdepth2", "valid", "lift_posdepth1", "lift_posdepth2")):
        o[name] = (flags >> bit & 1).astype(bool)
    o["ms"] = float(O.ms)
    return o


def _nms_info(I) -> dict:
    return dict(rounds=int(I.rounds), launches=int(I.launches), cells=int(I.cells), max_cell_points=int(I.max_cell_points), ms=float(I.ms))


def _xy(a, what="points") -> np.ndarray:
    """[n, 2] float64, C-contiguous (float32 input is widened exactly)."""
    a = np.ascontiguousarray(a, np.float64)
    if a.size == 0:
        return a.reshape(0, 2)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"{what} must be an [n, 2] array")
    return a


def radius_nms(points, scores, radius, order=None, device=0, return_info=False):
    """mpsfm_radius_nms: greedy radius suppression in priority order (`order`, a permutation with the highest priority first,
    else score descending with ties to the lower index).  Returns keep bool [n][, info dict(rounds, launches, cells,
    max_cell_points, ms)]."""
    p = _xy(points)
    n = len(p)
    s = np.ascontiguousarray(scores, np.float64).reshape(-1)
    if len(s) != n:
        raise ValueError("points and scores differ in length")
    o = None
    if order is not None:
        o = np.ascontiguousarray(order, np.int64).reshape(-1)
        if len(o) != n:
            raise ValueError("order must have one entry per point")
    keep, kept, I = np.zeros(max(n, 1), np.uint8), C.c_int64(0), CNmsInfo()
    _check(lib().mpsfm_radius_nms(n, p.ctypes.data, s.ctypes.data, None if o is None else o.ctypes.data, float(radius), int(device),
                                  keep.ctypes.data, C.addressof(kept), C.addressof(I)))
    keep = keep[:n].astype(bool)
    assert int(kept.value) == int(keep.sum())
    return (keep, _nms_info(I)) if return_info else keep


def thin_dense_matches_mask(dense0, dense1, dscores, sparse0=None, sparse1=None, radius=6.0, reference_slice=True, device=0,
                            return_info=False):
    """mpsfm_thin_dense_matches: both suppression passes of one pair's dense matches in one call.  Returns keep bool [n_dense]
    [, info dict].  `reference_slice`: see include/mpsfm_hip.h (the reference's slice drops surviving dense matches when
    matched sparse keypoints suppress each other)."""
    d0, d1 = _xy(dense0, "dense0"), _xy(dense1, "dense1")
    sc = np.ascontiguousarray(dscores, np.float64).reshape(-1)
    nd = len(d0)
    if len(d1) != nd or len(sc) != nd:
        raise ValueError("dense0, dense1 and dscores differ in length")
    s0 = _xy(np.zeros((0, 2)) if sparse0 is None else sparse0, "sparse0")
    s1 = _xy(np.zeros((0, 2)) if sparse1 is None else sparse1, "sparse1")
    if len(s0) != len(s1):
        raise ValueError("sparse0 and sparse1 differ in length")
    keep, kept, I = np.zeros(max(nd, 1), np.uint8), C.c_int64(0), CNmsInfo()
    _check(lib().mpsfm_thin_dense_matches(len(s0), s0.ctypes.data, s1.ctypes.data, nd, d0.ctypes.data, d1.ctypes.data, sc.ctypes.data,
                                          float(radius), int(bool(reference_slice)), int(device), keep.ctypes.data, C.addressof(kept),
                                          C.addressof(I)))
    keep = keep[:nd].astype(bool)
    return (keep, _nms_info(I)) if return_info else keep


def assign_keypoints_ids(query, kps, max_error, device=0, return_ms=False):
    """mpsfm_assign_keypoints: per query the nearest keypoint strictly closer than max_error (lowest index among equidistant
    ones) or -1.  Returns ids int64 [n_query][, device ms]."""
    q, k = _xy(query, "query"), _xy(kps, "kps")
    ids, ms = np.full(len(q), -1, np.int64), C.c_float(0)
    _check(lib().mpsfm_assign_keypoints(len(q), q.ctypes.data, len(k), k.ctypes.data, float(max_error), int(device), ids.ctypes.data,
                                        C.addressof(ms)))
    return (ids, float(ms.value)) if return_ms else ids


def _match_info(I) -> dict:
    return dict(num_matches=int(I.num_matches), ms=float(I.ms), column_ranges=int(I.column_ranges))


def _match_options(ratio_threshold, distance_threshold, score_threshold, do_mutual_check) -> CMatchOptions:
    o = CMatchOptions()
    lib().mpsfm_match_default_options(C.addressof(o))
    o.ratio_threshold = float(ratio_threshold or 0.0)
    o.distance_threshold = float(distance_threshold or 0.0)
    o.score_threshold = float(score_threshold or 0.0)
    o.mutual_check = int(bool(do_mutual_check))
    return o


def _on_device(*xs) -> bool:
    """True when every argument is a torch tensor in device memory (all or none: a mix is a ValueError)."""
    flags = [type(x).__module__.startswith("torch") and bool(getattr(x, "is_cuda", False)) for x in xs]
    if any(flags) and not all(flags):
        raise ValueError("either all arrays are device tensors or none is")
    return all(flags)


def _device_inputs(o, tensors, device):
    """float32, contiguous, on one device; the caller's stream goes into the options `o` (CMatchOptions or CWarpOptions: both have
    inputs_on_device and stream).  Every conversion is enqueued BEFORE the stream is taken or synchronised, so a caller that converts
    further tensors itself does so before this call.  Returns (tensors, device ordinal): the
    ordinal is the tensors' own, and a `device` argument that names another one is a ValueError."""
    import torch

    dev = tensors[0].device
    if any(t.device != dev for t in tensors):
        raise ValueError("device tensors on different devices")
    ordinal = dev.index if dev.index is not None else torch.cuda.current_device()
    if device is not None and int(device) != ordinal:
        raise ValueError(f"device={device} but the tensors are on device {ordinal}")
    for t in tensors:
        if t.dtype not in (torch.float16, torch.float32):
            raise TypeError(f"device tensors must be float16 or float32, not {t.dtype}")
    with torch.cuda.device(dev):
        out = [t.to(torch.float32).contiguous() for t in tensors]  # enqueued on the current stream, which the call waits for
        st = torch.cuda.current_stream(dev)
    o.inputs_on_device = 1
    if st.cuda_stream:
        o.stream = st.cuda_stream
    else:  # the legacy default stream: no stream of the library's ever synchronises with it implicitly
        st.synchronize()
        o.stream = None
    return out, ordinal


def _host_f32(a, what) -> np.ndarray:
    if type(a).__module__.startswith("torch"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.dtype not in (np.float16, np.float32):
        raise TypeError(f"{what} must be float16 or float32, not {a.dtype}")
    return np.ascontiguousarray(a, np.float32)


def match_descriptors(desc0, desc1, ratio_threshold=None, distance_threshold=None, do_mutual_check=True, score_threshold=None,
                      device=None, return_info=False):
    """mpsfm_match_descriptors: desc0 [n0, dim], desc1 [n1, dim], float16 / float32 NumPy arrays, host tensors or device tensors
    (device tensors go in as device pointers with the caller's current stream).  Returns matches0 int64 [n0] (-1: none),
    scores0 float64 [n0][, info dict(num_matches, ms, column_ranges)].  `device`: the ordinal for host inputs (default 0); device
    tensors run on their own device, and naming another one is a ValueError."""
    o = _match_options(ratio_threshold, distance_threshold, score_threshold, do_mutual_check)
    if _on_device(desc0, desc1):
        (a, b), device = _device_inputs(o, [desc0, desc1], device)
        pa, pb = a.data_ptr(), b.data_ptr()
    else:
        a, b = _host_f32(desc0, "desc0"), _host_f32(desc1, "desc1")
        pa, pb = a.ctypes.data, b.ctypes.data
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1]:
        raise ValueError("descriptors must be [n0, dim] and [n1, dim]")
    n0, n1, dim = int(a.shape[0]), int(b.shape[0]), int(a.shape[1])
    m, s, I = np.full(max(n0, 1), -1, np.int32), np.zeros(max(n0, 1)), CMatchInfo()
    _check(lib().mpsfm_match_descriptors(n0, n1, dim, pa or None, pb or None, C.addressof(o), int(device or 0), m.ctypes.data, s.ctypes.data,
                                         C.addressof(I)))
    m, s = m[:n0].astype(np.int64), s[:n0]
    return (m, s, _match_info(I)) if return_info else (m, s)


def match_descriptors_batch(descs, pairs, ratio_threshold=None, distance_threshold=None, do_mutual_check=True, score_threshold=None,
                            device=None, column_ranges=0, pairs_per_group=0, return_info=False):
    """mpsfm_match_descriptors_batch: the match lists of many image pairs in one call.  `descs`: a sequence of [n_i, dim] float16 /
    float32 arrays, one per image (NumPy, host tensors, or device tensors all on one device: those are concatenated on the device and
    go in as one device pointer with the caller's current stream).  `pairs`: a sequence of (i, j) image indices, rows = image i,
    columns = image j.  Returns a list of matches0 int64 [n_i] and a list of scores0 float64 [n_i], one entry per pair, each what
    match_descriptors returns for that pair alone[, info dict(num_matches, num_groups, num_launches, num_syncs, num_workgroups, ms,
    pair_num_matches int64 [num_pairs])].  `column_ranges` / `pairs_per_group` 0: the library's default rules; results depend on
    neither."""
    o = _match_options(ratio_threshold, distance_threshold, score_threshold, do_mutual_check)
    descs = list(descs)
    for d in descs:
        if getattr(d, "ndim", None) != 2:
            raise ValueError("every descriptor set must be [n, dim]")
    if len({int(d.shape[1]) for d in descs}) > 1:
        raise ValueError("descriptor sets of different dim")
    dim = int(descs[0].shape[1]) if descs else 1
    image_start = np.zeros(len(descs) + 1, np.int64)
    if descs:
        image_start[1:] = np.cumsum([int(d.shape[0]) for d in descs])
    if descs and _on_device(*descs):
        import torch

        tensors, device = _device_inputs(o, descs, device)
        with torch.cuda.device(tensors[0].device):
            cat = torch.cat(tensors)  # on the current stream, which the call waits for (or which _device_inputs synchronised)
            if not o.stream:
                torch.cuda.current_stream().synchronize()
        ptr = cat.data_ptr()
    else:
        host = [_host_f32(d, "descs") for d in descs]
        cat = np.ascontiguousarray(np.concatenate(host)) if host else np.zeros((0, dim), np.float32)
        ptr = cat.ctypes.data
    pr = np.asarray(list(pairs), np.int64).reshape(-1, 2)
    if len(pr) and (pr.min() < 0 or pr.max() >= len(descs)):
        raise ValueError("a pair names an image that is not in descs")
    p0, p1 = np.ascontiguousarray(pr[:, 0], np.int32), np.ascontiguousarray(pr[:, 1], np.int32)
    sizes = np.diff(image_start)
    match_start = np.zeros(len(pr) + 1, np.int64)
    match_start[1:] = np.cumsum(sizes[p0])
    rows = int(match_start[-1])
    m, s = np.full(max(rows, 1), -1, np.int32), np.zeros(max(rows, 1))
    cnt, R = np.zeros(max(len(pr), 1), np.int64), CMatchBatchReport()
    _check(lib().mpsfm_match_descriptors_batch(len(descs), image_start.ctypes.data, dim, ptr or None, len(pr), p0.ctypes.data, p1.ctypes.data,
                                               match_start.ctypes.data, C.addressof(o), int(column_ranges), int(pairs_per_group),
                                               int(device or 0), m.ctypes.data, s.ctypes.data, cnt.ctypes.data, C.addressof(R)))
    m = m.astype(np.int64)
    ms = [m[match_start[k]:match_start[k + 1]] for k in range(len(pr))]
    ss = [s[match_start[k]:match_start[k + 1]] for k in range(len(pr))]
    if not return_info:
        return ms, ss
    info = dict(num_matches=int(R.num_matches), num_groups=int(R.num_groups), num_launches=int(R.num_launches), num_syncs=int(R.num_syncs),
                num_workgroups=int(R.num_workgroups), ms=float(R.ms), pair_num_matches=cnt[:len(pr)])
    return ms, ss, info


MAX_NUM_SELECT = 128  # entries of a row's list in k_sim_topk (csrc/sim_topk.h: kMaxSelect)


def retrieve_topk(query, db, num_select, min_score=0.0, query_ids=None, db_ids=None, device=None, column_ranges=0, return_info=False):
    """mpsfm_retrieve_topk: query [nq, D], db [nd, D], float16 / float32 NumPy arrays, host tensors or device tensors (device tensors
    go in as device pointers with the caller's current stream); `query is db` is uploaded once.  Candidates of a query row: every db
    column but those with `query_ids[i] == db_ids[j]` (both id arrays or neither) and those with a similarity below `min_score`
    (None: no score test).  Returns indices int64 [nq, num_select] (-1 beyond the row's count), scores float64 [nq, num_select] (0
    beyond it), counts int64 [nq][, info dict(num_pairs, num_launches, num_syncs, ms, column_ranges)]: the first num_select
    candidates of every row under (similarity descending, index ascending).  `column_ranges` 0: the library's default rule; results
    do not depend on it."""
    o = CRetrievalOptions()
    lib().mpsfm_retrieval_default_options(C.addressof(o))
    o.num_select = int(num_select)
    o.use_min_score = 0 if min_score is None else 1
    o.min_score = 0.0 if min_score is None else float(min_score)
    o.column_ranges = int(column_ranges)
    one = query is db
    if _on_device(query, db):
        tensors, device = _device_inputs(o, [query] if one else [query, db], device)
        a, b = tensors[0], tensors[-1]
        pa, pb = a.data_ptr(), b.data_ptr()
    else:
        a = _host_f32(query, "query")
        b = a if one else _host_f32(db, "db")
        pa, pb = a.ctypes.data, b.ctypes.data
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1]:
        raise ValueError("descriptors must be [nq, dim] and [nd, dim]")
    nq, nd, dim = int(a.shape[0]), int(b.shape[0]), int(a.shape[1])
    if (query_ids is None) != (db_ids is None):
        raise ValueError("query_ids and db_ids: both or neither")
    qi = di = None
    if query_ids is not None:
        qi, di = np.ascontiguousarray(query_ids, np.int32).reshape(-1), np.ascontiguousarray(db_ids, np.int32).reshape(-1)
        if len(qi) != nq or len(di) != nd:
            raise ValueError("one id per descriptor")
        if nq == 0 or nd == 0:  # nothing to compare: an empty array has no address
            qi = di = None
    k = max(int(num_select), 1)
    idx, val, cnt, I = np.full((max(nq, 1), k), -1, np.int32), np.zeros((max(nq, 1), k)), np.zeros(max(nq, 1), np.int32), CRetrievalInfo()
    _check(lib().mpsfm_retrieve_topk(nq, nd, dim, pa or None, pb or None, None if qi is None else qi.ctypes.data,
                                     None if di is None else di.ctypes.data, C.addressof(o), int(device or 0), idx.ctypes.data, val.ctypes.data,
                                     cnt.ctypes.data, C.addressof(I)))
    out = idx[:nq].astype(np.int64), val[:nq], cnt[:nq].astype(np.int64)
    if not return_info:
        return out
    return (*out, dict(num_pairs=int(I.num_pairs), num_launches=int(I.num_launches), num_syncs=int(I.num_syncs), ms=float(I.ms),
                       column_ranges=int(I.column_ranges)))


CORR_STATUS = ("added", "invalid", "self_pair", "duplicate")  # match_status 0 .. 3 of mpsfm_corr_graph_build


def corr_graph_build(kp_start, list_image0, list_image1, list_start, matches, device=0):
    """mpsfm_corr_graph_build: `kp_start` int64 [n_images + 1], lists l of matches[list_start[l] : list_start[l + 1]] int32 [n, 2] between the
    image INDICES list_image0[l], list_image1[l].  Returns a dict of match_status uint8 [n], corr_start int64 [n_kp + 1], corr_kp int64
    [n_corr], image_num_correspondences / image_num_observations int32 [n_images], kp_two_view uint8 [n_kp], pair_image0 / pair_image1
    int32 [n_pairs], pair_start int64 [n_pairs + 1], pair_matches int32 [n_added, 2] and info (matches per status, num_launches,
    num_syncs, ms).  The arrays own their memory."""
    kp_start = np.ascontiguousarray(kp_start, np.int64).reshape(-1)
    li0, li1 = np.ascontiguousarray(list_image0, np.int32).reshape(-1), np.ascontiguousarray(list_image1, np.int32).reshape(-1)
    lstart = np.ascontiguousarray(list_start, np.int64).reshape(-1)
    matches = np.ascontiguousarray(matches, np.int32).reshape(-1, 2)
    n_images, n_lists = len(kp_start) - 1, len(li0)
    if n_images < 0 or len(li1) != n_lists or len(lstart) != n_lists + 1:
        raise ValueError("kp_start is [n_images + 1], list_image0 / list_image1 [n_lists], list_start [n_lists + 1]")
    if int(lstart[-1]) != len(matches):
        raise ValueError("list_start[n_lists] must be the number of matches")
    n_kp, n = max(int(kp_start[-1]), 0), len(matches)
    status, corr_start, corr_kp = np.zeros(max(n, 1), np.uint8), np.zeros(n_kp + 1, np.int64), np.zeros(max(2 * n, 1), np.int64)
    im_corr, im_obs, two_view = np.zeros(max(n_images, 1), np.int32), np.zeros(max(n_images, 1), np.int32), np.zeros(max(n_kp, 1), np.uint8)
    p0, p1, pstart = np.zeros(max(n_lists, 1), np.int32), np.zeros(max(n_lists, 1), np.int32), np.zeros(n_lists + 1, np.int64)
    pm = np.zeros((max(n, 1), 2), np.int32)
    n_corr, n_pairs, I = C.c_int64(0), C.c_int64(0), CCorrGraphInfo()
    _check(lib().mpsfm_corr_graph_build(n_images, kp_start.ctypes.data, n_lists, li0.ctypes.data if n_lists else None,
                                        li1.ctypes.data if n_lists else None, lstart.ctypes.data, matches.ctypes.data if n else None, int(device),
                                        status.ctypes.data, corr_start.ctypes.data, corr_kp.ctypes.data, C.addressof(n_corr), im_corr.ctypes.data,
                                        im_obs.ctypes.data, two_view.ctypes.data, C.addressof(n_pairs), p0.ctypes.data, p1.ctypes.data,
                                        pstart.ctypes.data, pm.ctypes.data, C.addressof(I)))
    nc, npairs = int(n_corr.value), int(n_pairs.value)
    info = dict(num_added=int(I.num_added), num_invalid=int(I.num_invalid), num_self_pairs=int(I.num_self_pairs),
                num_duplicates=int(I.num_duplicates), num_launches=int(I.num_launches), num_syncs=int(I.num_syncs), ms=float(I.ms))
    return dict(match_status=status[:n], corr_start=corr_start, corr_kp=corr_kp[:nc].copy(), image_num_correspondences=im_corr[:n_images],
                image_num_observations=im_obs[:n_images], kp_two_view=two_view[:n_kp], pair_image0=p0[:npairs].copy(), pair_image1=p1[:npairs].copy(),
                pair_start=pstart[:npairs + 1].copy(), pair_matches=pm[:nc // 2].copy(), info=info)


def _ptr(a):
    """The address of an array, NULL for None."""
    return None if a is None else a.ctypes.data


def _scene_query_info(I):
    return dict(num_launches=int(I.num_launches), num_syncs=int(I.num_syncs), num_groups=int(I.num_groups), ms=float(I.ms))


def visibility_scores(kp_start, kp_xy, corr_start, corr_kp, kp_point, image_size, num_levels=6, device=0, return_kp_visible=True):
    """mpsfm_visibility_scores on the arrays of graph_arrays() / state_arrays() (sfm/mapper/track_engine.py): `image_size` int32
    [n_images, 2] (width, height).  Returns a dict of num_visible int32 [n_images], score int64 [n_images], kp_visible uint8 [n_kp]
    (None when not asked for) and info.  The library checks the values (MPSFM_EINVAL); None stands for a NULL pointer."""
    def arr(a, dt):
        return None if a is None else np.ascontiguousarray(a, dt)

    kp_start, kp_xy, corr_start = arr(kp_start, np.int64), arr(kp_xy, np.float64), arr(corr_start, np.int64)
    corr_kp, kp_point, image_size = arr(corr_kp, np.int64), arr(kp_point, np.int64), arr(image_size, np.int32)
    n_images = -1 if kp_start is None else len(kp_start) - 1
    n_kp = 0 if kp_start is None or n_images < 0 else max(int(kp_start[-1]), 0)
    for a, n, what in ((kp_xy, 2 * n_kp, "kp_xy [n_kp, 2]"), (corr_start, n_kp + 1, "corr_start [n_kp + 1]"), (kp_point, n_kp, "kp_point [n_kp]"),
                       (image_size, 2 * max(n_images, 0), "image_size [n_images, 2]")):
        if a is not None and a.size < n:
            raise ValueError(f"{what} is too short")
    if corr_kp is not None and corr_start is not None and len(corr_start) and corr_kp.size < int(corr_start.reshape(-1)[n_kp]):
        raise ValueError("corr_kp is shorter than corr_start[n_kp]")
    nvis, score = np.zeros(max(n_images, 1), np.int32), np.zeros(max(n_images, 1), np.int64)
    vis = np.zeros(max(n_kp, 1), np.uint8) if return_kp_visible else None
    I = CSceneQueryInfo()
    _check(lib().mpsfm_visibility_scores(n_images, _ptr(kp_start), _ptr(kp_xy), _ptr(corr_start), _ptr(corr_kp), _ptr(kp_point), _ptr(image_size),
                                         int(num_levels), int(device), nvis.ctypes.data, score.ctypes.data, _ptr(vis), C.addressof(I)))
    n = max(n_images, 0)
    return dict(num_visible=nvis[:n], score=score[:n], kp_visible=None if vis is None else vis[:n_kp], info=_scene_query_info(I))


def local_bundles(kp_start, registered, cam_quat_xyzw, cam_t, kp_point, xyz, ref_image, num_images, min_tri_angle_deg, device=0):
    """mpsfm_local_bundles on the arrays of state_arrays(): `ref_image` image INDICES.  Returns a dict of bundle int32
    [n_refs, num_images - 1] (padded with -1), bundle_len int32 [n_refs], shared int32 [n_refs, n_images], angle75 float64
    [n_refs, n_images] (radians, -1 where shared == 0) and info.  The library checks the values (MPSFM_EINVAL)."""
    kp_start = np.ascontiguousarray(kp_start, np.int64).reshape(-1)
    n_images = len(kp_start) - 1
    n_kp = max(int(kp_start[-1]), 0) if n_images >= 0 else 0
    reg = np.ascontiguousarray(registered, np.uint8).reshape(-1)
    quat, trans = np.ascontiguousarray(cam_quat_xyzw, np.float64).reshape(-1, 4), np.ascontiguousarray(cam_t, np.float64).reshape(-1, 3)
    kp_point, xyz = np.ascontiguousarray(kp_point, np.int64).reshape(-1), np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    refs = np.ascontiguousarray(ref_image, np.int32).reshape(-1)
    if len(reg) != max(n_images, 0) or len(quat) != len(reg) or len(trans) != len(reg) or len(kp_point) < n_kp:
        raise ValueError("registered / cam_quat_xyzw / cam_t are [n_images], kp_point is [n_kp]")
    n_refs, width = len(refs), max(int(num_images) - 1, 0)
    bundle, blen = np.full((max(n_refs, 1), max(width, 1)), -1, np.int32), np.zeros(max(n_refs, 1), np.int32)
    shared = np.zeros((max(n_refs, 1), max(n_images, 1)), np.int32)
    angle75 = np.full((max(n_refs, 1), max(n_images, 1)), -1.0)
    st = CTriState(reg.ctypes.data if len(reg) else None, quat.ctypes.data if len(reg) else None, trans.ctypes.data if len(reg) else None,
                   kp_point.ctypes.data if n_kp else None, len(xyz), xyz.ctypes.data if len(xyz) else None)
    I = CSceneQueryInfo()
    _check(lib().mpsfm_local_bundles(n_images, kp_start.ctypes.data, C.addressof(st), n_refs, refs.ctypes.data if n_refs else None, int(num_images),
                                     float(min_tri_angle_deg), int(device), bundle.ctypes.data, blen.ctypes.data, shared.ctypes.data,
                                     angle75.ctypes.data, C.addressof(I)))
    n = max(n_images, 0)
    return dict(bundle=bundle[:n_refs, :width], bundle_len=blen[:n_refs], shared=shared[:n_refs, :n], angle75=angle75[:n_refs, :n],
                info=_scene_query_info(I))


def filter_scene(kp_start, kp_xy, intr, registered, cam_quat_xyzw, cam_t, kp_point, xyz, max_reproj_error, min_tri_angle_deg,
                 risky_min_tri_angle_deg=1.5, in_bundle=None, kp_invalid_depth=None, point_sel=None, negative_depth=True, device=0,
                 return_values=True) -> dict:
    """mpsfm_filter_scene on the arrays of graph_arrays() / state_arrays() (sfm/mapper/track_engine.py): the whole filter behind a
    bundle adjustment in one call.  `in_bundle` uint8 [n_images] and `kp_invalid_depth` uint8 [n_kp] describe the risky set (None: no
    such set), `point_sel` uint8 [n_points] the points of the second pass (None: every point).  Angles in degrees, converted with
    np.deg2rad: the thresholds are bit for bit those of sfm/scene/observations.py.  Returns a dict of kp_deleted uint8 [n_kp],
    point_fate uint8 [n_points] (0 .. 6 as in include/mpsfm_hip.h), point_risky uint8 [n_points], point_max_angle float64 [n_points] and kp_sq_err
    float64 [n_kp] (both None unless `return_values`) and info.  The library checks the values (MPSFM_EINVAL)."""
    kp_start = np.ascontiguousarray(kp_start, np.int64).reshape(-1)
    n_images = len(kp_start) - 1
    if n_images < 0:
        raise ValueError("filter_scene: kp_start is [n_images + 1]")
    n_kp = max(int(kp_start[-1]), 0)
    kp_xy, intr = np.ascontiguousarray(kp_xy, np.float64).reshape(-1, 2), np.ascontiguousarray(intr, np.float64).reshape(-1, 4)
    reg = np.ascontiguousarray(registered, np.uint8).reshape(-1)
    quat, trans = np.ascontiguousarray(cam_quat_xyzw, np.float64).reshape(-1, 4), np.ascontiguousarray(cam_t, np.float64).reshape(-1, 3)
    kp_point, xyz = np.ascontiguousarray(kp_point, np.int64).reshape(-1), np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    n_points = len(xyz)
    if not (len(intr) == len(reg) == len(quat) == len(trans) == n_images):
        raise ValueError("filter_scene: intr / registered / cam_quat_xyzw / cam_t are [n_images]")
    if len(kp_xy) < n_kp or len(kp_point) < n_kp:
        raise ValueError("filter_scene: kp_xy / kp_point are [n_kp]")

    def flags(a, n, what):
        if a is None:
            return None
        a = np.ascontiguousarray(np.asarray(a) != 0, np.uint8).reshape(-1)
        if len(a) != n:
            raise ValueError(f"filter_scene: {what}")
        return a

    in_bundle = flags(in_bundle, n_images, "in_bundle is [n_images]")
    kp_invalid_depth = flags(kp_invalid_depth, n_kp, "kp_invalid_depth is [n_kp]")
    point_sel = flags(point_sel, n_points, "point_sel is [n_points]")
    o = CSceneFilterOptions(float(max_reproj_error), float(np.deg2rad(float(min_tri_angle_deg))), float(np.deg2rad(float(risky_min_tri_angle_deg))),
                            1 if negative_depth else 0, 0)
    g = CTriGraph(n_images, kp_start.ctypes.data, kp_xy.ctypes.data if n_kp else None, intr.ctypes.data if n_images else None, None, None)
    st = CTriState(reg.ctypes.data if n_images else None, quat.ctypes.data if n_images else None, trans.ctypes.data if n_images else None,
                   kp_point.ctypes.data if n_kp else None, n_points, xyz.ctypes.data if n_points else None)
    deleted, fate, risky = np.zeros(max(n_kp, 1), np.uint8), np.zeros(max(n_points, 1), np.uint8), np.zeros(max(n_points, 1), np.uint8)
    angle = np.zeros(max(n_points, 1)) if return_values else None
    sq_err = np.zeros(max(n_kp, 1)) if return_values else None
    I = CSceneFilterInfo()
    _check(lib().mpsfm_filter_scene(C.addressof(g), C.addressof(st), _ptr(in_bundle) if n_images else None, _ptr(kp_invalid_depth) if n_kp else None,
                                    _ptr(point_sel) if n_points else None, C.addressof(o), int(device), deleted.ctypes.data, fate.ctypes.data,
                                    risky.ctypes.data, _ptr(angle), _ptr(sq_err), C.addressof(I)))
    info = {k: (float if k.startswith("ms") else int)(getattr(I, k)) for k, _ in CSceneFilterInfo._fields_}
    return dict(kp_deleted=deleted[:n_kp], point_fate=fate[:n_points], point_risky=risky[:n_points],
                point_max_angle=None if angle is None else angle[:n_points], kp_sq_err=None if sq_err is None else sq_err[:n_kp], info=info)


def match_map_descriptors(map0, conf0, map1, conf1, kps0, kps1, score_threshold=None, ratio_threshold=None, distance_threshold=None,
                          do_mutual_check=True, device=None, return_info=False):
    """mpsfm_match_map_descriptors: channel-last maps [H, W, C] and confidences [H, W] (float16 / float32; NumPy, host tensors
    or device tensors), keypoints [n, 2] (x, y) on the host.  Returns matches0 int64 [n0], scores0 float64 [n0]
    (sqrt(conf0 conf1) of the matched rows)[, info]."""
    o = _match_options(ratio_threshold, distance_threshold, score_threshold, do_mutual_check)
    if _on_device(map0, conf0, map1, conf1):
        arrs, device = _device_inputs(o, [map0, conf0, map1, conf1], device)
        ptrs = [t.data_ptr() for t in arrs]
    else:
        arrs = [_host_f32(x, w) for x, w in ((map0, "map0"), (conf0, "conf0"), (map1, "map1"), (conf1, "conf1"))]
        ptrs = [x.ctypes.data for x in arrs]
    m0, c0, m1, c1 = arrs
    if m0.ndim != 3 or m1.ndim != 3 or m0.shape[2] != m1.shape[2] or tuple(c0.shape) != tuple(m0.shape[:2]) or tuple(c1.shape) != tuple(m1.shape[:2]):
        raise ValueError("maps must be [H, W, C] with one C, confidences [H, W]")
    k0, k1 = _xy(kps0, "kps0"), _xy(kps1, "kps1")
    n0, n1 = len(k0), len(k1)
    m, s, I = np.full(max(n0, 1), -1, np.int32), np.zeros(max(n0, 1)), CMatchInfo()
    _check(lib().mpsfm_match_map_descriptors(ptrs[0] or None, ptrs[1] or None, int(m0.shape[0]), int(m0.shape[1]), ptrs[2] or None, ptrs[3] or None,
                                             int(m1.shape[0]), int(m1.shape[1]), int(m0.shape[2]), n0, k0.ctypes.data, n1, k1.ctypes.data,
                                             C.addressof(o), int(device or 0), m.ctypes.data, s.ctypes.data, C.addressof(I)))
    m, s = m[:n0].astype(np.int64), s[:n0]
    return (m, s, _match_info(I)) if return_info else (m, s)


def _recip_info(I) -> dict:
    return dict(n_seeds=int(I.n_seeds), n_converged=int(I.n_converged), iterations=int(I.iterations), nn_queries=int(I.nn_queries),
                column_ranges=int(I.column_ranges), ms=float(I.ms))


def _recip_options(subsample, max_iter) -> CRecipOptions:
    o = CRecipOptions()
    lib().mpsfm_recip_default_options(C.addressof(o))
    o.subsample, o.max_iter = int(subsample), int(max_iter)
    return o


def recip_seed_count(H, W, subsample) -> int:
    """mpsfm_recip_seed_count: the seeds of an H x W map (pixels S/2, S/2 + S, ... along both axes)."""
    return int(lib().mpsfm_recip_seed_count(int(H), int(W), int(subsample)))


def _recip_maps(o, arrays, names, device):
    """The maps of a reciprocal-matching call as (arrays kept alive, pointers, device ordinal): device tensors go in as device pointers
    with the caller's current stream, everything else as float32 host arrays."""
    if _on_device(*arrays):
        arrs, device = _device_inputs(o, list(arrays), device)
        return arrs, [t.data_ptr() for t in arrs], device
    arrs = [_host_f32(x, w) for x, w in zip(arrays, names)]
    return arrs, [x.ctypes.data for x in arrs], device


def reciprocal_nns(A, B, subsample=8, max_iter=10, device=None, return_info=False):
    """mpsfm_reciprocal_nns: one descent from the seed grid of A [H1, W1, C] into B [H2, W2, C] (float16 / float32; NumPy, host
    tensors or device tensors).  Returns the converged pairs as linear indices idx1, idx2 int32, unique and sorted by
    (idx1, idx2)[, info dict(n_seeds, n_converged, iterations, nn_queries, column_ranges, ms)]."""
    o = _recip_options(subsample, max_iter)
    (a, b), (pa, pb), device = _recip_maps(o, (A, B), ("A", "B"), device)
    if a.ndim != 3 or b.ndim != 3 or a.shape[2] != b.shape[2]:
        raise ValueError("maps must be [H, W, C] with one C")
    cap = max(recip_seed_count(a.shape[0], a.shape[1], o.subsample), 1)
    i1, i2, n, I = np.zeros(cap, np.int32), np.zeros(cap, np.int32), C.c_int64(0), CRecipInfo()
    _check(lib().mpsfm_reciprocal_nns(pa or None, int(a.shape[0]), int(a.shape[1]), pb or None, int(b.shape[0]), int(b.shape[1]), int(a.shape[2]),
                                      C.addressof(o), int(device or 0), cap, i1.ctypes.data, i2.ctypes.data, C.addressof(n), C.addressof(I)))
    i1, i2 = i1[:n.value].copy(), i2[:n.value].copy()
    return (i1, i2, _recip_info(I)) if return_info else (i1, i2)


def dense_correspondences(feats, qonfs, subsample=8, max_iter=10, device=None, return_info=False):
    """mpsfm_dense_correspondences: feats = (feat11, feat21, feat22, feat12) [H, W, C], qonfs = (qonf11, qonf21, qonf22, qonf12) [H, W], the
    order of the reference's extract_correspondences.  Returns xy1, xy2 int64 [n, 2] (x, y) and scores float32 [n][, info]."""
    o = _recip_options(subsample, max_iter)
    names = ["feat11", "feat21", "feat22", "feat12", "qonf11", "qonf21", "qonf22", "qonf12"]
    arrs, ptrs, device = _recip_maps(o, tuple(feats) + tuple(qonfs), names, device)
    f, q = arrs[:4], arrs[4:]
    if any(x.ndim != 3 for x in f) or len({int(x.shape[2]) for x in f}) != 1:
        raise ValueError("maps must be [H, W, C] with one C")
    s1, s2 = tuple(f[0].shape[:2]), tuple(f[1].shape[:2])
    if [tuple(x.shape[:2]) for x in f] != [s1, s2, s2, s1] or [tuple(x.shape) for x in q] != [s1, s2, s2, s1]:
        raise ValueError("feat11, feat12, qonf11, qonf12 share one [H1, W1], feat21, feat22, qonf21, qonf22 one [H2, W2]")
    cap = max(2 * (recip_seed_count(*s1, o.subsample) + recip_seed_count(*s2, o.subsample)), 1)
    xy1, xy2, sc, n, I = np.zeros((cap, 2), np.int32), np.zeros((cap, 2), np.int32), np.zeros(cap, np.float32), C.c_int64(0), CRecipInfo()
    _check(lib().mpsfm_dense_correspondences(*[p or None for p in ptrs], int(s1[0]), int(s1[1]), int(s2[0]), int(s2[1]), int(f[0].shape[2]),
                                             C.addressof(o), int(device or 0), cap, xy1.ctypes.data, xy2.ctypes.data, sc.ctypes.data,
                                             C.addressof(n), C.addressof(I)))
    xy1, xy2, sc = xy1[:n.value].astype(np.int64), xy2[:n.value].astype(np.int64), sc[:n.value].copy()
    return (xy1, xy2, sc, _recip_info(I)) if return_info else (xy1, xy2, sc)


def _warp_info(I) -> dict:
    return dict(num_dense=int(I.num_dense), num_valid=int(I.num_valid), num_matches=int(I.num_matches), ms=float(I.ms))


WARP_DENSE, WARP_SPARSE = 1, 2


def _warp_options(**kw) -> CWarpOptions:
    o = CWarpOptions()
    lib().mpsfm_warp_default_options(C.addressof(o))
    for k, v in kw.items():
        if k in ("scale0", "scale1"):
            v = np.asarray(v, np.float64).reshape(-1)
            if v.shape != (2,):
                raise ValueError(f"{k} must hold two values")
            setattr(o, k, (C.c_double * 2)(float(v[0]), float(v[1])))
        else:
            setattr(o, k, int(v) if k == "nms_radius" else float(v))
    return o


def simple_nms_map(scores, radius, device=None, return_info=False):
    """mpsfm_simple_nms: the reference's simple_nms of a 2-D float16 / float32 map, bitwise torch's.  A device tensor gives a float32
    device tensor (the map never leaves the device), anything else a float32 NumPy array.  [, info dict(..., ms)]."""
    o, I = CWarpOptions(), CWarpInfo()
    L = lib()
    if _on_device(scores):
        import torch

        (s,), device = _device_inputs(o, [scores], device)
        if s.ndim != 2:
            raise ValueError("scores must be a 2-D map")
        if s.numel() == 0:
            return (s.clone(), _warp_info(I)) if return_info else s.clone()
        out = torch.empty_like(s)
        _check(L.mpsfm_simple_nms(int(s.shape[0]), int(s.shape[1]), s.data_ptr(), int(radius), 1, o.stream, int(device), out.data_ptr(), C.addressof(I)))
    else:
        s = _host_f32(scores, "scores")
        if s.ndim != 2:
            raise ValueError("scores must be a 2-D map")
        if s.size == 0:
            return (s.copy(), _warp_info(I)) if return_info else s.copy()
        out = np.empty_like(s)
        _check(L.mpsfm_simple_nms(int(s.shape[0]), int(s.shape[1]), s.ctypes.data, int(radius), 0, None, int(device or 0), out.ctypes.data,
                                  C.addressof(I)))
    return (out, _warp_info(I)) if return_info else out


def _host_scores_f32(a) -> np.ndarray:
    """float32 [n]; float64 values are taken only when float32 holds them exactly (a rounding could create ties)"""
    if type(a).__module__.startswith("torch"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a).reshape(-1)
    if a.dtype == np.float64:
        b = a.astype(np.float32)
        if not np.array_equal(b.astype(np.float64), a, equal_nan=True):
            raise TypeError("float64 scores that float32 does not hold exactly")
        return np.ascontiguousarray(b)
    if a.dtype not in (np.float16, np.float32):
        raise TypeError(f"scores must be float16 or float32, not {a.dtype}")
    return np.ascontiguousarray(a, np.float32)


def _host_ids(a) -> np.ndarray:
    """int64 [n]; anything but integers is refused (a float id would be truncated silently)"""
    if type(a).__module__.startswith("torch"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a).reshape(-1)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"keypoint ids must be integers, not {a.dtype}")
    return np.ascontiguousarray(a, np.int64)


def kpids_to_matches0_arrays(ids0, ids1, scores, n0=None, n1=None, device=0, return_info=False):
    """mpsfm_kpids_to_matches0: ids int [n] (-1: none), scores float16 / float32 [n]; host arrays, or device tensors (all three).  n0 / n1: the numbers of
    keypoints (default: 1 + the largest id).  Returns matches0 int32 [n_kps0], scores0 float32 [n_kps0] with the reference's
    length n_kps0 = 1 + the largest matched ids0 [, info dict(num_valid, num_matches, ms, ...)]."""
    on_device, stream = _on_device(ids0, ids1, scores), None
    if on_device:  # int64 ids and float32 scores, contiguous, on one device
        import torch

        if ids0.device != scores.device or ids1.device != scores.device:
            raise ValueError("device tensors on different devices")
        if any(t.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64) for t in (ids0, ids1)):
            raise TypeError(f"keypoint ids must be integers, not {ids0.dtype} / {ids1.dtype}")
        with torch.cuda.device(scores.device):  # the ids first: whatever a conversion enqueues lies in front of the point the call waits for
            a, b = (t.reshape(-1).to(torch.int64).contiguous() for t in (ids0, ids1))
        o = CWarpOptions()
        (s,), device = _device_inputs(o, [scores.reshape(-1)], device or None)  # converts, then takes (or synchronises) the stream
        stream = o.stream
        pa, pb, ps = a.data_ptr(), b.data_ptr(), s.data_ptr()
    else:
        a, b = _host_ids(ids0), _host_ids(ids1)
        s = _host_scores_f32(scores)
        pa, pb, ps = a.ctypes.data, b.ctypes.data, s.ctypes.data
    if not (len(a) == len(b) == len(s)):
        raise ValueError("ids0, ids1 and scores differ in length")
    n = len(a)
    n0 = int(n0) if n0 is not None else (int(a.max()) + 1 if n else 0)
    n1 = int(n1) if n1 is not None else (int(b.max()) + 1 if n else 0)
    m, sc, nk, I = np.full(max(n0, 1), -1, np.int32), np.zeros(max(n0, 1), np.float32), C.c_int64(0), CWarpInfo()
    _check(lib().mpsfm_kpids_to_matches0(n, pa or None, pb or None, ps or None, n0, n1, int(on_device), stream, int(device or 0), m.ctypes.data,
                                         sc.ctypes.data, C.addressof(nk), C.addressof(I)))
    k = int(nk.value)
    return (m[:k], sc[:k], _warp_info(I)) if return_info else (m[:k], sc[:k])


def warp_matches(warp, certainty, sizes, mode=WARP_DENSE | WARP_SPARSE, skpts0=None, skpts1=None, scale0=(1.0, 1.0), scale1=(1.0, 1.0),
                 nms_radius=8, sample_thresh=0.1, max_error=2.0, device=None, return_info=False):
    """mpsfm_warp_matches: certainty [H, W] and warp [H, W, 4] or [H W, 4] (float16 / float32; NumPy, host tensors or device tensors
    that stay on the device), sizes = (H_A, W_A, H_B, W_B).  Returns a dict with dkeypoints0 / dkeypoints1 float32 [n, 2] and dscores
    float32 [n] (dense leg), smatches0 int32 [n_kps0] and smatching_scores0 float32 [n_kps0] (sparse leg) [, info]."""
    mode = int(mode)
    o = _warp_options(scale0=scale0, scale1=scale1, nms_radius=nms_radius, sample_thresh=sample_thresh, max_error=max_error)
    if _on_device(warp, certainty):
        (w, c), device = _device_inputs(o, [warp, certainty], device)
        pw, pc = w.data_ptr(), c.data_ptr()
    else:
        w, c = _host_f32(warp, "warp"), _host_f32(certainty, "certainty")
        pw, pc = w.ctypes.data, c.ctypes.data
    if c.ndim != 2 or w.shape[-1] != 4 or int(np.prod(w.shape[:-1])) != int(c.shape[0]) * int(c.shape[1]):
        raise ValueError("certainty must be [H, W] and warp [H, W, 4] or [H W, 4]")
    H, W = int(c.shape[0]), int(c.shape[1])
    px = H * W
    HA, WA, HB, WB = (int(v) for v in sizes)
    dense, sparse = bool(mode & WARP_DENSE), bool(mode & WARP_SPARSE)
    k0 = _xy(np.zeros((0, 2)) if skpts0 is None else skpts0, "skpts0")
    k1 = _xy(np.zeros((0, 2)) if skpts1 is None else skpts1, "skpts1")
    out, I = {}, CWarpInfo()
    if px == 0:
        if dense:
            out.update(dkeypoints0=np.zeros((0, 2), np.float32), dkeypoints1=np.zeros((0, 2), np.float32), dscores=np.zeros(0, np.float32))
        if sparse:
            out.update(smatches0=np.zeros(0, np.int32), smatching_scores0=np.zeros(0, np.float32))
        return (out, _warp_info(I)) if return_info else out
    d0 = np.empty((px if dense else 1, 2), np.float32)
    d1 = np.empty((px if dense else 1, 2), np.float32)
    ds = np.empty(px if dense else 1, np.float32)
    m, sc = np.full(max(len(k0), 1), -1, np.int32), np.zeros(max(len(k0), 1), np.float32)
    nd, nk = C.c_int64(0), C.c_int64(0)
    _check(lib().mpsfm_warp_matches(H, W, pc, pw, HA, WA, HB, WB, mode, C.addressof(o), len(k0), k0.ctypes.data, len(k1), k1.ctypes.data,
                                    int(device or 0), d0.ctypes.data, d1.ctypes.data, ds.ctypes.data, C.addressof(nd), m.ctypes.data, sc.ctypes.data,
                                    C.addressof(nk), C.addressof(I)))
    if dense:
        k = int(nd.value)
        out.update(dkeypoints0=d0[:k].copy(), dkeypoints1=d1[:k].copy(), dscores=ds[:k].copy())
    if sparse:
        k = int(nk.value)
        out.update(smatches0=m[:k].copy(), smatching_scores0=sc[:k].copy())
    return (out, _warp_info(I)) if return_info else out


# ---- monocular depth / normal priors (csrc/mono_priors.hip) --------------------------------------------------------------
def _prior_values(item, names, shape_tail=()):
    """The value maps of one image in ONE precision: float32 when every present map is float32, float64 otherwise.
    Returns (is_float32, {name: C-contiguous array or None})."""
    present = [np.asarray(item[k]) for k in names if item.get(k) is not None]
    f32 = bool(present) and all(a.dtype == np.float32 for a in present)
    dt = np.float32 if f32 else np.float64
    out = {}
    for k in names:
        a = item.get(k)
        out[k] = None if a is None else np.ascontiguousarray(a, dt)
    shape = out[names[0]].shape if out[names[0]] is not None else None
    for k, a in out.items():
        if a is not None and shape is not None and a.shape[:2] != shape[:2]:
            raise ValueError(f"{k} and {names[0]} differ in shape")
    return f32, out


def _prior_mask(a):
    """bool / numeric mask -> C-contiguous uint8 (non-zero = true), None stays None"""
    if a is None:
        return None
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError("masks are [H, W]")
    return np.ascontiguousarray(a != 0 if a.dtype != np.bool_ else a).view(np.uint8)


def _ptr(a):
    return None if a is None else a.ctypes.data


def depth_priors(items, conf, device=0, return_summary=False):
    """mpsfm_depth_priors: the depth priors of all `items` in one call.

    `items`: list of dicts with depth [h,w] (float32 or float64), optional depth2, depth_variance, depth_variance2,
    valid, valid2 [h,w], optional mask (any shape), size = (int_height, int_width), kps [n,2], sx, sy.  `conf`: mapping with
    the keys of Depth.default_conf.  Nothing passed in is modified.
    Returns a list of dicts(data_prior, uncertainty float64 [H,W]; valid, continuity_mask bool [H,W]; uncertainty_update [n])."""
    n = len(items)
    P = (CDepthPriorProblem * max(n, 1))()
    O = (CDepthPriorOutput * max(n, 1))()
    keep, outs = [], []
    for k, it in enumerate(items):
        f32, v = _prior_values(it, ("depth", "depth2", "depth_variance", "depth_variance2"))
        if v["depth"] is None or v["depth"].ndim != 2:
            raise ValueError("depth must be an [h, w] map")
        h, w = v["depth"].shape
        masks = {m: _prior_mask(it.get(m)) for m in ("valid", "valid2", "mask")}
        for m in ("valid", "valid2"):
            if masks[m] is not None and masks[m].shape != (h, w):
                raise ValueError(f"{m} and depth differ in shape")
        kps = np.ascontiguousarray(np.asarray(it.get("kps", np.zeros((0, 2))), np.float64).reshape(-1, 2))
        H, W = (int(x) for x in it["size"])
        e = P[k]
        e.height, e.width, e.int_height, e.int_width = h, w, H, W
        e.mask_height, e.mask_width = masks["mask"].shape if masks["mask"] is not None else (0, 0)
        e.is_float32, e.n_kps = int(f32), len(kps)
        e.depth, e.depth2, e.depth_variance, e.depth_variance2 = (_ptr(v[m]) for m in ("depth", "depth2", "depth_variance", "depth_variance2"))
        e.valid, e.valid2, e.mask = _ptr(masks["valid"]), _ptr(masks["valid2"]), _ptr(masks["mask"])
        e.kps = kps.ctypes.data if len(kps) else None
        e.sx, e.sy = float(it["sx"]), float(it["sy"])
        ok = H > 0 and W > 0
        shape = (H, W) if ok else (0, 0)  # every entry is written by the call
        o = dict(data_prior=np.empty(shape), uncertainty=np.empty(shape), valid=np.empty(shape, np.uint8),
                 continuity_mask=np.empty(shape, np.uint8), uncertainty_update=np.empty(len(kps)))
        O[k].data_prior, O[k].uncertainty, O[k].valid = o["data_prior"].ctypes.data, o["uncertainty"].ctypes.data, o["valid"].ctypes.data
        O[k].continuity_mask, O[k].uncertainty_update = o["continuity_mask"].ctypes.data, o["uncertainty_update"].ctypes.data
        keep.append((v, masks, kps))
        outs.append(o)
    cf = CDepthPriorConf()
    for name in ("inherent_noise", "std_multiplier", "prior_std_multiplier", "fixed_uncertainty_val"):
        setattr(cf, name, float(conf[name]))
    for name in ("max_std", "depth_lim", "depth_uncertainty"):
        val = conf[name]
        setattr(cf, "has_" + name, int(val is not None))
        setattr(cf, name, 0.0 if val is None else float(val))
    for name in ("use_continuity", "fixed_uncertainty", "prior_uncertainty", "flip_consistency"):
        setattr(cf, name, int(bool(conf[name])))
    S = CPriorSummary()
    _check(lib().mpsfm_depth_priors(n, C.addressof(P), C.addressof(cf), int(device), C.addressof(O), C.addressof(S)))
    for o in outs:
        o["valid"], o["continuity_mask"] = o["valid"].view(np.bool_), o["continuity_mask"].view(np.bool_)
    return (outs, dict(ms=S.ms, n_images=S.n_images, n_pixels=S.n_pixels)) if return_summary else outs


def normal_priors(items, conf, device=0, return_summary=False):
    """mpsfm_normal_priors: the normal priors of all `items` in one call.

    `items`: list of dicts with normals [h,w,3], normals_variance [h,w] (float32 or float64), optional normals2,
    normals2_variance, optional mask (any shape), optional continuity_mask [H,W], size = (H, W).  `conf`: mapping with the
    keys of Normals.default_conf.  Nothing passed in is modified.
    Returns a list of dicts(data [H,W,3], uncertainty [H,W,3,3], data_downscaled [Hd,Wd,3], uncertainty_downscaled [Hd,Wd,3,3])."""
    n = len(items)
    P = (CNormalPriorProblem * max(n, 1))()
    O = (CNormalPriorOutput * max(n, 1))()
    f = conf["downscale_factor"]
    keep, outs = [], []
    for k, it in enumerate(items):
        f32, v = _prior_values(it, ("normals", "normals2", "normals_variance", "normals2_variance"))
        nm = v["normals"]
        if nm is None or nm.ndim != 3 or nm.shape[2] != 3:
            raise ValueError("normals must be an [h, w, 3] map")
        if v["normals2"] is not None and v["normals2"].shape != nm.shape:
            raise ValueError("normals2 and normals differ in shape")
        for m in ("normals_variance", "normals2_variance"):
            if v[m] is not None and v[m].shape != nm.shape[:2]:
                raise ValueError(f"{m} must be [h, w]")
        h, w = nm.shape[:2]
        H, W = (int(x) for x in it["size"])
        mask, cont = _prior_mask(it.get("mask")), _prior_mask(it.get("continuity_mask"))
        if cont is not None and cont.shape != (H, W):
            raise ValueError("continuity_mask must have the target size")
        e = P[k]
        e.height, e.width, e.int_height, e.int_width = h, w, H, W
        e.mask_height, e.mask_width = mask.shape if mask is not None else (0, 0)
        e.is_float32 = int(f32)
        e.normals, e.normals2, e.normals_variance, e.normals2_variance = (_ptr(v[m]) for m in ("normals", "normals2", "normals_variance", "normals2_variance"))
        e.mask, e.continuity_mask = _ptr(mask), _ptr(cont)
        ok = H > 0 and W > 0 and f > 0
        Hd, Wd = (max(int(H // f), 0), max(int(W // f), 0)) if ok else (0, 0)
        e.half_height, e.half_width = Hd, Wd
        if not ok:
            H = W = 0
        o = dict(data=np.empty((H, W, 3)), uncertainty=np.empty((H, W, 3, 3)), data_downscaled=np.empty((Hd, Wd, 3)),
                 uncertainty_downscaled=np.empty((Hd, Wd, 3, 3)))  # every entry is written by the call
        O[k].data, O[k].uncertainty = o["data"].ctypes.data, o["uncertainty"].ctypes.data
        O[k].data_downscaled, O[k].uncertainty_downscaled = o["data_downscaled"].ctypes.data, o["uncertainty_downscaled"].ctypes.data
        keep.append((v, mask, cont))
        outs.append(o)
    cf = CNormalPriorConf()
    for name in ("inherent_polar_noise", "std_multiplier", "lc_std_multiplier", "prior_std_multiplier", "downscale_factor"):
        setattr(cf, name, float(conf[name]))
    cf.flip_consistency = int(bool(conf["flip_consistency"]))
    S = CPriorSummary()
    _check(lib().mpsfm_normal_priors(n, C.addressof(P), C.addressof(cf), int(device), C.addressof(O), C.addressof(S)))
    return (outs, dict(ms=S.ms, n_images=S.n_images, n_pixels=S.n_pixels)) if return_summary else outs
