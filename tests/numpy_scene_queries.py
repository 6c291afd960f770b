"""NumPy / plain-Python restatement of mpsfm_visibility_scores and mpsfm_local_bundles (include/mpsfm_hip.h), written the way COLMAP
3.11 computes them, not the way the kernels do: the visibility pyramid is a list of integer count matrices incremented point by point
(VisibilityPyramid::SetPoint with cx >>= 1), visibility comes from walking the correspondences of the keypoints that have a 3-D point
(ObservationManager::SetObservationAsTriangulated), the local bundle uses dicts, Python's sort with the stated tie rule and
sorted(angles)[idx] (IncrementalMapper::FindLocalBundle, Percentile).  Also the hand-built scenes that the CPU and the GPU tests share.
"""
import math
from collections import defaultdict

import numpy as np

ANGLE_DIV = (1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 5.0, 6.0)
SHARED_RATIO = (0.6, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1, 0.1)


# ---- visibility ---------------------------------------------------------------------------------------------------------------------
def pyramid_cell(x, size, D):
    """clamp((int64) trunc(D x / size), 0, D - 1); a negative or NaN operand gives 0."""
    with np.errstate(all="ignore"):
        v = np.float64(D) * np.float64(x) / np.float64(size)
    if not v >= 0:
        return 0
    return D - 1 if v >= D else int(v)


class VisibilityPyramid:
    def __init__(self, num_levels, width, height):
        self.num_levels, self.width, self.height, self.score = num_levels, width, height, 0
        self.pyramid = [np.zeros((1 << (level + 1), 1 << (level + 1)), np.int64) for level in range(num_levels)]

    def set_point(self, x, y):
        D = 1 << self.num_levels
        cx, cy = pyramid_cell(x, self.width, D), pyramid_cell(y, self.height, D)
        for i in range(self.num_levels - 1, -1, -1):
            level = self.pyramid[i]
            level[cy, cx] += 1
            if level[cy, cx] == 1:
                self.score += level.size
            cx >>= 1
            cy >>= 1


def visibility(kp_start, kp_xy, corr_start, corr_kp, kp_point, image_size, num_levels=6):
    """dict(num_visible, score, kp_visible)"""
    n_images, n_kp = len(kp_start) - 1, int(kp_start[-1])
    kp_image = np.repeat(np.arange(n_images), np.diff(kp_start))
    pyramids = [VisibilityPyramid(num_levels, int(image_size[i][0]), int(image_size[i][1])) for i in range(n_images)]
    have = np.zeros(n_kp, np.int64)  # num_correspondences_have_point3D
    num_visible = np.zeros(n_images, np.int32)
    for k in range(n_kp):
        if kp_point[k] < 0:
            continue
        for c in range(int(corr_start[k]), int(corr_start[k + 1])):  # SetObservationAsTriangulated(k)
            p = int(corr_kp[c])
            have[p] += 1
            if have[p] == 1:
                num_visible[kp_image[p]] += 1
                pyramids[kp_image[p]].set_point(kp_xy[p][0], kp_xy[p][1])
    return dict(num_visible=num_visible, score=np.array([p.score for p in pyramids], np.int64), kp_visible=(have > 0).astype(np.uint8))


# ---- local bundles ------------------------------------------------------------------------------------------------------------------
def quat_to_R(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def tri_angle(c1, c2, X):
    """CalculateTriangulationAngle: the law of cosines, the smaller of the angle and pi - angle"""
    b2 = float(np.sum((c1 - c2) ** 2))
    r1, r2 = float(np.sum((X - c1) ** 2)), float(np.sum((X - c2) ** 2))
    den = 2.0 * math.sqrt(r1 * r2)
    if den == 0.0:
        return 0.0
    ang = abs(math.acos(min(1.0, max(-1.0, (r1 + r2 - b2) / den))))
    return min(ang, math.pi - ang)


def percentile75(angles):
    return sorted(angles)[int(math.floor(0.75 * (len(angles) - 1) + 0.5))]  # Percentile rounds


def local_bundle(kp_start, registered, cam_quat_xyzw, cam_t, kp_point, xyz, ref, num_images, min_tri_angle_deg):
    """dict(bundle [image indices], shared [n_images], angle75 [n_images], compared [(angle75, threshold)] of the walk, angles [all])"""
    n_images = len(kp_start) - 1
    centres = [-quat_to_R(cam_quat_xyzw[i]).T @ np.asarray(cam_t[i], np.float64) for i in range(n_images)]
    tracks = defaultdict(list)  # point -> [(image, keypoint)] over the registered images
    for i in range(n_images):
        if registered[i]:
            for k in range(int(kp_start[i]), int(kp_start[i + 1])):
                if kp_point[k] >= 0:
                    tracks[int(kp_point[k])].append((i, k))
    shared_of = defaultdict(int)
    ref_points = set()
    T = 0
    for k in range(int(kp_start[ref]), int(kp_start[ref + 1])):
        if kp_point[k] < 0:
            continue
        T += 1
        ref_points.add(int(kp_point[k]))
        for image, _ in tracks[int(kp_point[k])]:
            if image != ref:
                shared_of[image] += 1
    overlapping = sorted(shared_of.items(), key=lambda e: (-e[1], e[0]))
    shared, angle75 = np.zeros(n_images, np.int32), np.full(n_images, -1.0)
    all_angles = []
    for image, n in overlapping:
        shared[image] = n
        angles = [tri_angle(centres[ref], centres[image], np.asarray(xyz[int(kp_point[k])], np.float64))
                  for k in range(int(kp_start[image]), int(kp_start[image + 1])) if int(kp_point[k]) in ref_points]
        angle75[image] = percentile75(angles)
        all_angles += angles
    N = num_images - 1
    E = min(N, len(overlapping))
    compared = []
    if len(overlapping) == E:
        bundle = [image for image, _ in overlapping]
    else:
        bundle, used = [], set()
        min_tri_angle_rad = min_tri_angle_deg * (math.pi / 180.0)
        for div, ratio in zip(ANGLE_DIV, SHARED_RATIO):
            if len(bundle) >= E:
                break
            for image, n in overlapping:
                if n < ratio * T:
                    break
                if image in used:
                    continue
                compared.append((angle75[image], min_tri_angle_rad / div))
                if angle75[image] >= min_tri_angle_rad / div:
                    bundle.append(image)
                    used.add(image)
                    if len(bundle) >= E:
                        break
        for image, _ in overlapping:
            if len(bundle) >= E:
                break
            if image not in used:
                bundle.append(image)
                used.add(image)
    return dict(bundle=bundle, shared=shared, angle75=angle75, compared=compared, angles=all_angles)


# ---- scenes placed by hand ----------------------------------------------------------------------------------------------------------
def make_scene(centres, points, observations, registered=None):
    """Images with identity rotation at the given projection centres (t = -C); observations[i]: the point index of every keypoint of
    image i (-1: no point).  The arrays of mpsfm_tri_state plus kp_start."""
    n = len(centres)
    nkp = [len(o) for o in observations]
    quat = np.zeros((n, 4))
    quat[:, 3] = 1.0
    return dict(kp_start=np.concatenate([[0], np.cumsum(nkp)]).astype(np.int64),
                registered=np.ones(n, np.uint8) if registered is None else np.asarray(registered, np.uint8), cam_quat_xyzw=quat,
                cam_t=-np.asarray(centres, np.float64).reshape(n, 3),
                kp_point=np.concatenate([np.asarray(o, np.int64) for o in observations]) if sum(nkp) else np.zeros(0, np.int64),
                xyz=np.asarray(points, np.float64).reshape(-1, 3))


def state_args(scene):
    return [scene[k] for k in ("kp_start", "registered", "cam_quat_xyzw", "cam_t", "kp_point", "xyz")]


def _baseline_for(angle, depth=10.0):
    """The x offset of a camera that sees a point at (0, 0, depth) under `angle` from a camera at the origin."""
    return depth * math.tan(angle)


def walk_scene(shared_and_angle, T, extra_ref=()):
    """Reference image 0 at the origin with T keypoints on the points 0 .. T - 1, all at (0, 0, 10); image j = 1, 2, ... at the baseline
    that gives every shared point the angle asked for, observing the points 0 .. shared - 1 once each."""
    centres = [(0.0, 0.0, 0.0)] + [(_baseline_for(a), 0.0, 0.0) for _, a in shared_and_angle]
    points = [(0.0, 0.0, 10.0)] * T
    obs = [list(range(T)) + list(extra_ref)] + [list(range(s)) for s, _ in shared_and_angle]
    return make_scene(centres, points, obs)


MIN_TRI_ANGLE_DEG = 6.0  # COLMAP's local_ba_min_tri_angle; thresholds 0.1047, 0.0698, 0.0524, 0.0419, 0.0349, 0.0262, 0.0209, 0.01745 rad


def walk_cases():
    """name -> (scene, ref, num_images, expected bundle).  T = 10 (20 in "overlap break") keypoints of the reference have a point."""
    cases = {}
    # fewer overlapping images than asked for: all of them, by shared
    cases["take all"] = (walk_scene([(3, 0.2), (9, 0.012), (5, 0.05)], 10), 0, 6, [2, 3, 1])
    # image 2 passes at once; image 1 only when the angle is halved (third threshold, 0.5 T = 5 shared); image 3 would pass there too
    cases["third threshold"] = (walk_scene([(9, 0.06), (8, 0.2), (7, 0.055), (2, 0.3)], 10), 0, 3, [2, 1])
    # image 3 has the widest angle but 1 shared point of T = 20: below 0.1 T, so no threshold ever reaches it, and the fill takes image 2
    cases["overlap break"] = (walk_scene([(18, 0.2), (5, 0.012), (1, 0.3)], 20), 0, 3, [1, 2])
    # no angle reaches the last threshold (0.01745): everything comes from the fill, in order
    cases["fill up"] = (walk_scene([(4, 0.012), (9, 0.013), (6, 0.011), (7, 0.0125)], 10), 0, 3, [2, 4])
    # equal shared counts: the lower image index first
    cases["ties"] = (walk_scene([(6, 0.2), (7, 0.012), (6, 0.2), (6, 0.012)], 10), 0, 3, [1, 3])
    # two keypoints of the reference on point 0 and two keypoints of image 2 on point 1: shared[2] = 2 + 1 + 1 + 1 = 5 with the
    # multiplicity of the reference's side, one angle per keypoint of image 2 (4 entries); without it image 2 would tie with image 1
    # (shared 4) and lose to its lower index
    sc = make_scene([(0, 0, 0), (_baseline_for(0.2), 0, 0), (_baseline_for(0.15), 0, 0)], [(0, 0, 10.0)] * 4,
                    [[0, 0, 1, 2, 3], [1, 2, 3, 3], [0, 1, 1, 2]])
    cases["multiplicity"] = (sc, 0, 2, [2])
    return cases


def assert_margins(result, zero_allowed=False, min_angle=1e-2):
    """What lets the GPU tests compare decisions exactly: every angle75 a walk compares lies 1e-9 rad from its threshold, and every
    angle is at least `min_angle`: acos turns a last-bit difference of its argument (1e-16) into 1e-16 / sin(angle), 1e-14 rad at
    1e-2, far below both the 1e-9 and the 1e-12 the angles are compared with."""
    for a, thr in result["compared"]:
        assert abs(a - thr) >= 1e-9, (a, thr)
    for a in result["angles"]:
        assert a >= min_angle or (zero_allowed and a == 0.0), a


def order_statistic_scene(lengths, seed=0, equal=(), two_values=(), zero_at=None):
    """Reference image 0 at the origin with max(lengths) points; image j observes the first lengths[j - 1] of them.  The points are
    spread so that the angles differ, every one above 0.02 rad.  `equal`: images that observe point 0 with every keypoint; `two_values`:
    images whose first third of keypoints sees point 0 and the rest point 1; `zero_at`: an image at whose projection centre point 2
    lies (angle 0)."""
    rng = np.random.default_rng(seed)
    n_pts = max(max(lengths), 3)
    points = np.stack([rng.uniform(-2, 2, n_pts), rng.uniform(-2, 2, n_pts), rng.uniform(6, 40, n_pts)], 1)
    centres = [(0.0, 0.0, 0.0)] + [(1.5 + 1.0 * j, 0.4 * j + 0.05 * j * j, 0.0) for j in range(len(lengths))]  # no three on a line
    obs = [list(range(n_pts))]
    for j, n in enumerate(lengths, start=1):
        o = list(rng.permutation(n)) if n > 1 else list(range(n))
        if j in equal:
            o = [0] * n
        if j in two_values:
            o = [0] * (n // 3) + [1] * (n - n // 3)
        obs.append(o)
    if zero_at is not None:
        points[2] = centres[zero_at]
    return make_scene(centres, points, obs)
