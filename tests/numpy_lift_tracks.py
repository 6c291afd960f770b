"""NumPy restatement of mpsfm_lift_tracks (mpsfm_amd/csrc/lift_tracks.hip) with capi.lift_tracks's signature and outputs.

Vectorised over the track elements and in the kernel's operation order: every product and sum is an elementwise NumPy
operation rounded on its own (no np.dot, no @, no BLAS in a decision).  The angles are the oracle's (oracle/tri_oracle.c
through O.filter_tracks), or the caller's (`angles=`) where a test wants both sides to decide on one set of numbers.
Beyond the outputs of the library it returns, per track, `scale` = |ray d| + |t| of the lifting camera (the size the lift's
rounding errors are relative to) and, per element, `z`: the depth of the lifted point in the element's camera."""

import numpy as np

from mpsfm_amd.sfm.scene.priorutils import bilinear_at_kps
from oracle import cpu_oracle as O

EPS = 2.0**-52


def rotations(quat_xyzw):
    """quat_to_R of csrc/common.h, operation by operation: [n, 9] row-major."""
    q = np.asarray(quat_xyzw, np.float64).reshape(-1, 4)
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.stack([1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)], 1)


def _len3(v):
    return np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])


def lift_tracks(tr, xyz, activated, depth_maps, valid_maps, sx, sy, min_angle_deg, device=0, angles=None):
    nt, ne = tr.n_tracks, tr.n_el
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    start = tr.track_start
    out = dict(risky=np.zeros(nt, bool), lift_el=np.full(nt, -1, np.int32), lift_depth=np.zeros(nt), lift_xyz=np.zeros((nt, 3)),
               el_keep=np.zeros(ne, bool), scale=np.zeros(nt), z=np.zeros(ne),
               info=dict(n_risky=0, n_lifted=0, n_no_lift=0, n_maps_uploaded=0, bytes_uploaded=0, ms=0.0))
    if nt == 0:
        return out
    ang = np.asarray(O.filter_tracks(tr, xyz)[0] if angles is None else angles, np.float64)
    risky = ang < float(np.deg2rad(float(min_angle_deg)))
    out["risky"] = risky
    out["info"]["n_risky"] = int(risky.sum())
    if not risky.any():
        return out
    track_of = np.repeat(np.arange(nt), np.diff(start))
    pos = np.arange(ne) - start[track_of]
    cam = tr.el_cam.astype(np.int64)
    act = np.asarray(activated, bool)
    in_risky = risky[track_of]
    # validity and depth samples of the elements of risky tracks in activated cameras, camera by camera
    ok, d = np.zeros(ne, bool), np.zeros(ne)
    for c in np.unique(cam[in_risky & act[cam]]):
        sel = np.flatnonzero(in_risky & (cam == c))
        H, W = np.asarray(depth_maps[c]).shape
        out["info"]["n_maps_uploaded"] += 1
        out["info"]["bytes_uploaded"] += 9 * H * W
        ok[sel] = bilinear_at_kps(np.asarray(valid_maps[c], np.uint8).astype(np.float64), tr.el_xy[sel], sx[c], sy[c]) == 1.0
        d[sel] = bilinear_at_kps(np.asarray(depth_maps[c], np.float64), tr.el_xy[sel], sx[c], sy[c])
    big = np.iinfo(np.int64).max
    first = np.full(nt, big)
    np.minimum.at(first, track_of[ok], pos[ok])
    lifted = first < big
    out["info"]["n_lifted"] = int(lifted.sum())
    out["info"]["n_no_lift"] = int(risky.sum() - lifted.sum())
    t_l = np.flatnonzero(lifted)
    e_l = start[t_l] + first[t_l]
    R, t, K = rotations(tr.cam_quat), tr.cam_t, tr.cam_intr[tr.cam_intr_idx]
    c_l = cam[e_l]
    x, y, dd = tr.el_xy[e_l, 0], tr.el_xy[e_l, 1], d[e_l]
    p = np.stack([(x - K[c_l, 2]) / K[c_l, 0] * dd, (y - K[c_l, 3]) / K[c_l, 1] * dd, dd], 1)
    q = p - t[c_l]
    X = np.zeros((nt, 3))
    for k in range(3):
        X[t_l, k] = R[c_l, k] * q[:, 0] + R[c_l, 3 + k] * q[:, 1] + R[c_l, 6 + k] * q[:, 2]
    out["lift_el"][t_l] = first[t_l]
    out["lift_depth"][t_l] = dd
    out["lift_xyz"] = X
    out["scale"][t_l] = _len3(p) + _len3(t[c_l])
    els = np.flatnonzero(lifted[track_of])
    Xe, ce = X[track_of[els]], cam[els]
    z = R[ce, 6] * Xe[:, 0] + R[ce, 7] * Xe[:, 1] + R[ce, 8] * Xe[:, 2] + t[ce, 2]
    out["z"][els] = z
    out["el_keep"][els] = z >= EPS
    return out
