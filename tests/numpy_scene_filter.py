"""TEST SCAFFOLDING: mpsfm_filter_scene (include/mpsfm_hip.h) restated the way the sequential code works, not the way the kernel
does: per-point Python lists, `delete_observation` called once per bad observation with COLMAP's "a track of length <= 2 goes with
its point" rule, `set.intersection` over the bundle images' flagged points, then the two `filter_points3D` passes (reprojection
over the whole id list, then angles over what is left of it).  Only the per-element arithmetic is vectorised, in NumPy and in the
kernel's operation order: every NumPy operation rounds on its own, as the kernel's do with contraction off.  The angle goes
through np.arccos.

`filter_scene` has the signature and the return value of mpsfm_amd.capi.filter_scene, so it also serves as
BundleFilter(backend=...)."""

from __future__ import annotations

import numpy as np

EPS = 2.220446049250313e-16  # 2^-52


def image_records(quat_xyzw, trans):
    """R [n, 9] and the centres C [n, 3], in the operation order of k_sf_images."""
    q = np.asarray(quat_xyzw, np.float64).reshape(-1, 4)
    t = np.asarray(trans, np.float64).reshape(-1, 3)
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.stack([1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)], 1)
    C = np.stack([-((R[:, k] * t[:, 0] + R[:, 3 + k] * t[:, 1]) + R[:, 6 + k] * t[:, 2]) for k in range(3)], 1)
    return R, C


def element_numerics(kp_image, kp_xy, intr, R, t, kp_point, xyz):
    """zc, front and sq_err of every keypoint (the values of keypoints without a point are meaningless)."""
    im = np.asarray(kp_image)
    X = xyz[np.maximum(kp_point, 0)] if len(xyz) else np.zeros((len(kp_point), 3))
    r, tt, K = R[im], t[im], intr[im]
    with np.errstate(all="ignore"):
        xc = ((r[:, 0] * X[:, 0] + r[:, 1] * X[:, 1]) + r[:, 2] * X[:, 2]) + tt[:, 0]
        yc = ((r[:, 3] * X[:, 0] + r[:, 4] * X[:, 1]) + r[:, 5] * X[:, 2]) + tt[:, 1]
        zc = ((r[:, 6] * X[:, 0] + r[:, 7] * X[:, 1]) + r[:, 8] * X[:, 2]) + tt[:, 2]
        du = ((K[:, 0] * xc) / zc + K[:, 2]) - kp_xy[:, 0]
        dv = ((K[:, 1] * yc) / zc + K[:, 3]) - kp_xy[:, 1]
        sq_err = du * du + dv * dv
    return zc, zc >= EPS, sq_err


def max_pair_angle(C, X):
    """The largest pairwise angle of the centres C [L, 3] seen from X, k_filter's pair formula; 0 for fewer than two."""
    if len(C) < 2:
        return 0.0
    d = X[None, :] - C
    r = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    e = C[:, None, :] - C[None, :, :]
    b2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    with np.errstate(all="ignore"):
        den = 2.0 * np.sqrt(r[:, None] * r[None, :])
        cs = np.clip(((r[:, None] + r[None, :]) - b2) / den, -1.0, 1.0)
        ang = np.abs(np.arccos(cs))
        ang = np.fmin(ang, np.pi - ang)
    ang = np.where(den == 0.0, 0.0, ang)
    ang[np.arange(len(C)), np.arange(len(C))] = 0.0  # a pair is two elements
    return float(np.fmax.reduce(ang.ravel(), initial=0.0))


def filter_scene(kp_start, kp_xy, intr, registered, cam_quat_xyzw, cam_t, kp_point, xyz, max_reproj_error, min_tri_angle_deg,
                 risky_min_tri_angle_deg=1.5, in_bundle=None, kp_invalid_depth=None, point_sel=None, negative_depth=True, device=0,
                 return_values=True, details=None) -> dict:
    kp_start = np.asarray(kp_start, np.int64)
    n_images, n_kp = len(kp_start) - 1, int(kp_start[-1])
    kp_xy, intr = np.asarray(kp_xy, np.float64).reshape(-1, 2), np.asarray(intr, np.float64).reshape(-1, 4)
    kp_point, xyz = np.asarray(kp_point, np.int64), np.asarray(xyz, np.float64).reshape(-1, 3)
    n_points = len(xyz)
    kp_image = np.repeat(np.arange(n_images), np.diff(kp_start))
    reg = np.asarray(registered).astype(bool)
    if np.any((kp_point >= 0) & ~reg[kp_image]):
        raise ValueError("a keypoint of an image that is not registered has a point")
    R, C = image_records(cam_quat_xyzw, cam_t)
    zc, front, sq_err = element_numerics(kp_image, kp_xy, intr, R, np.asarray(cam_t, np.float64).reshape(-1, 3), kp_point, xyz)
    max_sq = float(max_reproj_error) * float(max_reproj_error)
    thr_a, thr_b = float(np.deg2rad(float(risky_min_tri_angle_deg))), float(np.deg2rad(float(min_tri_angle_deg)))

    # the scene as the sequential code holds it: a track per point, a point per keypoint
    tracks = {}
    for k in np.flatnonzero(kp_point >= 0).tolist():
        tracks.setdefault(int(kp_point[k]), []).append(k)
    point_of = {k: p for p, els in tracks.items() for k in els}
    deleted = np.zeros(n_kp, np.uint8)
    fate, risky_out, angle_out = np.zeros(n_points, np.uint8), np.zeros(n_points, np.uint8), np.zeros(n_points)
    angles_compared = []  # (angle, threshold) of every angle test, for the margins of the test builders

    def delete_point3D(p, why):
        for k in tracks.pop(p):
            del point_of[k]
        fate[p] = why

    def delete_observation(k, mark, why):
        """COLMAP ObservationManager::DeleteObservation"""
        p = point_of[k]
        if len(tracks[p]) <= 2:
            delete_point3D(p, why)
            return
        tracks[p].remove(k)
        del point_of[k]
        deleted[k] = mark

    # filter_observations_with_negative_depth
    num_negative = 0
    if negative_depth:
        for k in np.flatnonzero((kp_point >= 0) & ~front).tolist():
            if k not in point_of:  # its point went away with an earlier deletion
                continue
            delete_observation(k, 1, 2)
            num_negative += 1

    # find_invalid_depth_points of the bundle's images, intersected
    risky = set()
    if in_bundle is not None and kp_invalid_depth is not None and np.any(in_bundle):
        flagged = np.asarray(kp_invalid_depth).astype(bool)
        per_image = []
        for i in np.flatnonzero(in_bundle).tolist():
            per_image.append({point_of[k] for k in range(int(kp_start[i]), int(kp_start[i + 1])) if k in point_of and flagged[k]})
        risky = set.intersection(*per_image)
    for p in risky:
        risky_out[p] = 1

    def filter_points3D(ids, thr, mark, fate_err, fate_angle):
        n = 0
        ids = sorted(ids)
        for p in ids:  # reprojection errors first
            if p not in tracks:
                continue
            els = list(tracks[p])
            bad = [k for k in els if (not front[k]) or sq_err[k] > max_sq]
            if len(els) < 2 or len(bad) >= len(els) - 1:
                n += len(els)
                delete_point3D(p, fate_err)
                continue
            n += len(bad)
            for k in bad:
                delete_observation(k, mark, fate_err)
        for p in ids:  # then the angles
            if p not in tracks:
                continue
            a = max_pair_angle(C[kp_image[tracks[p]]], xyz[p])
            angle_out[p] = a
            angles_compared.append((a, thr))
            if not (a >= thr):
                n += 1
                delete_point3D(p, fate_angle)
        return n

    num_a = filter_points3D(risky, thr_a, 2, 3, 4)
    selected = range(n_points) if point_sel is None else np.flatnonzero(point_sel).tolist()
    num_b = filter_points3D(selected, thr_b, 3, 5, 6)
    deleted[(kp_point >= 0) & (fate[np.maximum(kp_point, 0)] >= 2)] = 0  # what goes with a whole point is not marked
    touched = np.unique(kp_point[deleted != 0])  # kept, observations removed
    fate[touched[fate[touched] == 0]] = 1
    err_out = np.where(kp_point >= 0, sq_err, 0.0)
    if details is not None:
        details.update(zc=zc, front=front, sq_err=sq_err, angles_compared=angles_compared, max_sq=max_sq, kp_image=kp_image)
    info = dict(num_negative=num_negative, num_changed_a=num_a, num_changed_b=num_b, n_points_deleted=int((fate >= 2).sum()),
                n_observations_deleted=int((deleted != 0).sum()), num_syncs=0, ms=0.0, ms_tracks=0.0)
    return dict(kp_deleted=deleted, point_fate=fate, point_risky=risky_out, point_max_angle=angle_out if return_values else None,
                kp_sq_err=err_out if return_values else None, info=info)
