"""TEST SCAFFOLDING: hand-built scenes for mpsfm_filter_scene as the flat arrays of the call, shared by tests/test_scene_filter_cpu.py
and tests/test_gpu_scene_filter.py.

Every camera has the identity rotation and fx = fy = 1, cx = cy = 0, so the camera-frame point is X - C and its projection
(xc / zc, yc / zc): with power-of-two coordinates every operation of the kernel is exact and a value can sit exactly on a bound.
A track is a list of elements (image, du, dv, flagged): the keypoint is the projection of the point plus (du, dv).  The elements of a
track lie in ascending image order, so the position of an element in its track is the rank of its image.

`check_margins` asserts, on the restatement's own values, what makes exact agreement between two correctly rounded evaluations a
legitimate demand: every zc and every sq_err is exactly on its bound or 1e-9 away from it, and every compared angle keeps
|a - thr| >= 1e3 eps / min(a, thr) or is exactly 0 (acos near 1 turns a few eps of its argument into a few eps / a of the angle).
"""

from __future__ import annotations

import copy

import numpy as np

import numpy_scene_filter as N
from numpy_scene import NumpyCorrespondenceGraph, scene_from_problem
from mpsfm_amd.sfm.mapper.filtering import BundleFilter
from mpsfm_amd.sfm.scene.scene_queries import SceneQueries
from mpsfm_amd.synthetic import make_scene

EPS = np.finfo(float).eps
MAX_ERR = 4.0


def build(cams, points, bundle=(), registered=None, empty_images=()):
    """cams: [(cx, cy, cz)] camera centres; points: [(xyz, [(image, du, dv, flagged), ...])]; bundle: image indices.
    Returns the keyword arguments of filter_scene (without thresholds) and `kp_of[(point, image, nth)]`."""
    n_images = len(cams)
    per_image = [[] for _ in range(n_images)]  # (point, x, y, flagged)
    for p, (xyz, els) in enumerate(points):
        for image, du, dv, flagged in els:
            assert image not in empty_images
            xc, yc, zc = (float(xyz[k]) - float(cams[image][k]) for k in range(3))
            with np.errstate(all="ignore"):
                u, v = np.float64(xc) / np.float64(zc), np.float64(yc) / np.float64(zc)
            u, v = (0.0 if not np.isfinite(u) else float(u)), (0.0 if not np.isfinite(v) else float(v))
            per_image[image].append((p, u + du, v + dv, flagged))
    kp_start, kp_xy, kp_point, flags, kp_of, seen = [0], [], [], [], {}, {}
    for i in range(n_images):
        if i not in empty_images:  # every image but the empty ones starts with a keypoint that has no point
            kp_xy.append((1.0, 1.0)); kp_point.append(-1); flags.append(1)
        for p, x, y, flagged in per_image[i]:
            nth = seen.get((p, i), 0)
            seen[(p, i)] = nth + 1
            kp_of[(p, i, nth)] = len(kp_point)
            kp_xy.append((x, y)); kp_point.append(p); flags.append(1 if flagged else 0)
        kp_start.append(len(kp_point))
    quat = np.tile([0.0, 0.0, 0.0, 1.0], (n_images, 1))
    in_bundle = np.zeros(n_images, np.uint8)
    in_bundle[list(bundle)] = 1
    args = dict(kp_start=np.array(kp_start, np.int64), kp_xy=np.array(kp_xy, np.float64).reshape(-1, 2),
                intr=np.tile([1.0, 1.0, 0.0, 0.0], (n_images, 1)), registered=np.ones(n_images, np.uint8) if registered is None else np.asarray(registered, np.uint8),
                cam_quat_xyzw=quat, cam_t=-np.array(cams, np.float64).reshape(-1, 3), kp_point=np.array(kp_point, np.int64),
                xyz=np.array([xyz for xyz, _ in points], np.float64).reshape(-1, 3),
                in_bundle=in_bundle if len(bundle) else None, kp_invalid_depth=np.array(flags, np.uint8) if len(bundle) else None)
    return args, kp_of


def check_margins(details, kp_point):
    pointed = np.asarray(kp_point) >= 0
    zc, err = details["zc"][pointed], details["sq_err"][pointed]
    on = np.isin(zc, [2.0**-52, 2.0**-53, 0.0])
    assert np.all(on | (np.abs(zc - 2.0**-52) >= 1e-9)), "a depth is neither on the cheirality bound nor 1e-9 away from it"
    fin = np.isfinite(err)
    ulp_above = np.nextafter(details["max_sq"], np.inf)
    on = (err == details["max_sq"]) | (err == ulp_above)
    assert np.all(~fin | on | (np.abs(err - details["max_sq"]) >= 1e-9)), "an error is neither on the bound nor 1e-9 away from it"
    for a, thr in details["angles_compared"]:
        assert a == 0.0 or abs(a - thr) >= 1e3 * EPS / min(a, thr), f"angle {a} too close to its threshold {thr}"


def run_restatement(args, min_tri_angle_deg, point_sel=None, negative_depth=True, risky_deg=1.5, max_err=MAX_ERR):
    details = {}
    out = N.filter_scene(max_reproj_error=max_err, min_tri_angle_deg=min_tri_angle_deg, risky_min_tri_angle_deg=risky_deg, point_sel=point_sel,
                         negative_depth=negative_depth, details=details, **args)
    check_margins(details, args["kp_point"])
    return out


# ---- the pieces the scenes are made of ------------------------------------------------------------------------------------------------
def line_cams(n, spacing=2.0**-6, behind=()):
    """n cameras on the x axis around 0; those listed in `behind` stand one unit behind the plane z = 8 (the point is not in front)."""
    return [((i - n // 2) * spacing, 0.0, 9.0 if i in behind else 0.0) for i in range(n)]


def track(images, bad=(), flagged=(), err=8.0):
    """elements in the listed images; those at the POSITIONS `bad` miss their keypoint by `err` pixels"""
    return [(im, err if pos in bad else 0.0, 0.0, pos in flagged) for pos, im in enumerate(images)]


POINT = (0.0, 0.0, 8.0)       # seen under about 0.11 degrees per camera step of 2^-6: beyond 1.5 degrees from 14 steps on
LENGTHS = (1, 2, 3, 63, 64, 65, 128, 129, 200)


def risky_scene(bundle):
    cams = line_cams(7, behind=(6,))
    points = [(POINT, track([0, 1, 2], flagged=(0,))), (POINT, track([0, 1, 2], flagged=(0, 1))), (POINT, track([0, 1, 2], flagged=(0, 1, 2))),
              (POINT, track([0, 1, 3, 4, 6], flagged=(0, 1, 4))),           # its flagged element in image 6 is behind the camera
              (POINT, track([0, 0, 1], flagged=(0, 1)))]                    # two flagged keypoints of image 0
    return build(cams, points, bundle=bundle)


def valid_call():
    """The keyword arguments of a filter_scene call that is accepted."""
    args, _ = risky_scene((0, 1))
    return dict(args, max_reproj_error=4.0, min_tri_angle_deg=0.001)


# ---- synthetic scenes with rotated cameras, as scene objects -------------------------------------------------------------------------
def reproject(sc, pid):
    """moves the keypoints of a point's track onto the point's projections"""
    p = sc.points3D[pid]
    for e in p.track.elements:
        im = sc.images[e.image_id]
        Xc = im.cam_from_world.rotation.matrix() @ p.xyz + im.cam_from_world.translation
        fx, fy, cx, cy = sc.rec.cameras[im.camera_id].params
        im.kps[e.point2D_idx] = [fx * Xc[0] / Xc[2] + cx, fy * Xc[1] / Xc[2] + cy]


def make_filter_scene(seed, n_cams=6):
    """A scene with every defect the filter looks for, and images 1 .. 3 without a valid prior depth."""
    prob, truth = make_scene(n_cams, 400, True, seed=seed, perturb=False, track_mean=2.0)
    sc = scene_from_problem(prob, truth, seed=seed)
    rng = np.random.default_rng(seed + 7)
    pids = np.array(sorted(sc.points3D))
    rng.shuffle(pids)
    for pid in pids[:40].tolist():       # behind some of its cameras
        sc.points3D[pid].xyz[:] = sc.points3D[pid].xyz * -4.0 + rng.normal(0, 3, 3)
    for pid in pids[40:120].tolist():    # off by decimetres: bad observations
        sc.points3D[pid].xyz += rng.normal(0, 0.3, 3)
    for k, pid in enumerate(pids[120:220].tolist()):  # far along the first ray, consistently observed: little or no parallax
        el = sc.points3D[pid].track.elements[0]
        im = sc.images[el.image_id]
        C = -im.cam_from_world.rotation.matrix().T @ im.cam_from_world.translation
        sc.points3D[pid].xyz[:] = C + (sc.points3D[pid].xyz - C) * (1e7 if k % 2 else 300.0)
        reproject(sc, pid)
    for im in sc.images.values():        # single gross keypoint errors
        idx = rng.choice(len(im.kps), max(1, len(im.kps) // 20), replace=False)
        im.kps[idx] += rng.uniform(-40, 40, (len(idx), 2))
    for imid in (1, 2, 3):
        sc.images[imid].depth.valid[:] = 0.0
    # what the scene is for: a filter of the fixed bundle meets every fate (on a copy, through the restatement)
    trial = copy.deepcopy(sc)
    bf = BundleFilter({}, trial, SceneQueries(trial, empty_graph(trial)), backend=N.filter_scene)
    bf.filter_bundle(fixed_bundle(trial))
    fates = np.bincount(bf.last_result["point_fate"], minlength=7)
    assert np.all(fates > 0), f"make_filter_scene({seed}, {n_cams}) does not bring out every fate: {fates.tolist()}"
    return sc


def empty_graph(sc):
    """A correspondence graph that knows the scene's images and nothing else: what a SceneQueries needs for its keypoint arrays."""
    cg = NumpyCorrespondenceGraph()
    for imid, im in sc.images.items():
        cg.add_image(imid, len(im.kps))
    return cg


def fixed_bundle(sc):
    """Images 1 .. 3 around image 2; the points of image 2, and those of image 1 as constant points."""
    bundle = {"ref_id": 2, "optim_ids": {1, 2, 3}}
    bundle["pts3D"] = set(sc.images[2].point3D_ids(sc.images[2].get_observation_point2D_idxs()).tolist())
    bundle["constpoints"] = set(sc.images[1].point3D_ids(sc.images[1].get_observation_point2D_idxs()).tolist()) - bundle["pts3D"]
    return bundle


def assert_same_scene(a, b):
    assert sorted(a.points3D) == sorted(b.points3D)
    for pid, p in a.points3D.items():
        assert [(e.image_id, e.point2D_idx) for e in p.track.elements] == [(e.image_id, e.point2D_idx) for e in b.points3D[pid].track.elements]
    for imid, im in a.images.items():
        np.testing.assert_array_equal(im.kp_point3D, b.images[imid].kp_point3D)
        assert im.has_pose == b.images[imid].has_pose


def assert_same_errors(a, b):
    """Point3D.error of two scenes that went through the same filters on two paths.  Both evaluate the same formula in f64 on
    coordinates below 2e3 px with a few dozen roundings, in another order: below 1e-11 px apart; 1e-9 px is asked for."""
    assert sorted(a.points3D) == sorted(b.points3D)
    ids = sorted(a.points3D)
    np.testing.assert_allclose([a.points3D[p].error for p in ids], [b.points3D[p].error for p in ids], rtol=1e-9, atol=1e-9)
