"""depth_icp_scenes.py — TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The RGB-D pairs that the CPU and the GPU tests of the dense ICP share, with the restatement's answers computed once per scene:
alignment_scenes.depth_pair_scene's surface and pose at any map size (the whole scene at another resolution, or a window of it),
optionally with a fronto-parallel rectangular occluder in front of it, rendered analytically into both maps."""

import functools
import math

import numpy as np

import numpy_depth_icp as NDI

MAX_REDRAWS = 8
# name -> (H, W, occluder, icp options).  "tight" narrows the angle gate so that it rejects pairs while the pose is still off.
LOOP_SCENES = {
    "pair": (60, 80, False, dict(stride=1)),
    "pair_stride2": (60, 80, False, dict(stride=2)),
    "occluder": (60, 80, True, dict(stride=1)),
    "tight": (60, 80, False, dict(stride=1, max_angle_deg=2.0)),
    "large": (240, 320, False, dict(stride=1)),
}
# (H, W, whole scene): interior source-pixel counts (H - 2)(W - 2) on the edges of k_icp_link's partition: 255, 256, 257, 1023, 1024,
# 1025 (windows of the scene), and 75684 (the whole scene), past the 256 x 256 pixels that one sweep of the largest grid covers
EDGE_MAPS = [(17, 19, False), (18, 18, False), (3, 259, False), (35, 33, False), (34, 34, False), (27, 43, False), (240, 320, True)]
LOOP_EPS = 1e-10
# |dR|_F and |dt| of the restatement's fixed point from the truth on the 60 x 80 pair, rounded up (test_depth_icp_cpu.py pins them;
# DESIGN.md section 4x): the bias of nearest-pixel association on a curved surface
FIXED_POINT_BIAS = (9.65e-5, 2.11e-4)
# the starts: truth, a small and a large perturbation, as |dR|_F ~ sqrt(2) angle and |dt|
STARTS = ((0.0, 0.0), (0.0076 / math.sqrt(2.0), 0.0088), (0.038 / math.sqrt(2.0), 0.054))


def scene_intr(H, W):
    """The 60 x 80 scene's field of view on an H x W map."""
    return np.array([70.0 * W / 80.0, 68.0 * H / 60.0, (W - 1) / 2.0, (H - 1) / 2.0])


def window_intr(H, W):
    """An H x W window at the 60 x 80 scene's resolution: a sub-map."""
    return np.array([70.0, 68.0, (W - 1) / 2.0, (H - 1) / 2.0])


def _rodrigues(axis, ang):
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def render_pair(H, W, intr, occluder=False, draw=0):
    """dict(depth0, depth1 [H, W], intr, R, t (camera 1 from camera 0)).  Map 1 is ray-cast against the surface by Newton to
    1e-12; map 0 has a hole of zeros.  `draw` moves the pose a little."""
    fx, fy, cx, cy = intr
    su, sv = 70.0 / fx, 68.0 / fy  # pixel -> pixel of the 60 x 80 scene's camera (fx 70, fy 68)

    def surface(u, v):
        return 3.0 + 0.3 * np.sin(u * su / 15.0) + 0.2 * np.cos(v * sv / 11.0)

    def project(X):
        return X[..., 0] / X[..., 2] * fx + cx, X[..., 1] / X[..., 2] * fy + cy

    R = _rodrigues([0.2, 1.0, 0.1], 0.06 + 0.004 * draw)
    t = np.array([-0.18, 0.03, 0.05]) + 0.003 * draw * np.array([1.0, -1.0, 0.5])
    vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = np.stack([(uu - cx) / fx, (vv - cy) / fy, np.ones_like(uu)], -1)
    depth0 = surface(uu, vv)
    z1 = np.full((H, W), 3.0)
    for _ in range(60):
        X0 = (rays * z1[..., None] - t) @ R  # R^T (X1 - t)
        g = X0[..., 2] - surface(*project(X0))
        z1 = z1 - g / (rays @ R)[..., 2]
    assert np.abs(g).max() < 1e-12
    depth1 = z1
    if occluder:  # the rectangle |x - 0.15| <= 0.45, |y + 0.1| <= 0.3 of the plane z = 2.2 of camera 0: a depth step of ~0.8
        z_o, lo, hi = 2.2, np.array([-0.30, -0.40]), np.array([0.60, 0.20])
        X0 = rays * z_o
        hit0 = (X0[..., 0] >= lo[0]) & (X0[..., 0] <= hi[0]) & (X0[..., 1] >= lo[1]) & (X0[..., 1] <= hi[1]) & (z_o < depth0)
        depth0 = np.where(hit0, z_o, depth0)
        zo1 = (z_o + (R.T @ t)[2]) / (rays @ R)[..., 2]  # (R^T (ray z - t))_z = z_o
        X0 = (rays * zo1[..., None] - t) @ R
        hit1 = (X0[..., 0] >= lo[0]) & (X0[..., 0] <= hi[0]) & (X0[..., 1] >= lo[1]) & (X0[..., 1] <= hi[1]) & (zo1 > 0) & (zo1 < depth1)
        depth1 = np.where(hit1, zo1, depth1)
    depth0 = depth0.copy()
    r0, c0 = H // 3, (3 * W) // 8
    depth0[r0:r0 + max(1, H // 10), c0:c0 + max(1, (6 * W) // 80)] = 0.0  # a hole
    return dict(depth0=depth0, depth1=depth1, intr=np.asarray(intr, np.float64), R=R, t=t)


def starts(R, t, draw=0):
    """The three start poses [3, 4]: the truth and the two perturbed ones; `draw` turns the direction of the perturbation."""
    out = []
    axis, along = np.random.default_rng(120 + draw).normal(size=(2, 3))
    for ang, shift in STARTS:
        out.append(np.c_[_rodrigues(axis, ang) @ R, t + shift * along / np.linalg.norm(along)])
    return out


def _frozen(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def loop_scene(name):
    """render_pair's dict plus starts, options, refs (the restatement's result per start) and redraws: the first draw k < 8 on
    which the restatement reports no fragile decision from any start.  Callers do not modify the arrays."""
    H, W, occluder, opts = LOOP_SCENES[name]
    options = dict(opts, eps_rotation=LOOP_EPS, eps_translation=LOOP_EPS)
    for k in range(MAX_REDRAWS):
        s = render_pair(H, W, scene_intr(H, W), occluder, k)
        st = starts(s["R"], s["t"], k)
        refs = [NDI.icp(s["depth0"], s["intr"], s["depth1"], s["intr"], T, **options) for T in st]
        if not any(r["fragile"] for r in refs):
            return _frozen(dict(s, starts=st, options=options, refs=refs, redraws=k))
    raise AssertionError(f"no draw without a fragile decision for {name}")


@functools.lru_cache(maxsize=None)
def edge_scene(H, W, whole):
    """One linearisation at the small perturbed start on an H x W map: render_pair's dict plus start, options, ref, redraws."""
    options = dict(max_iterations=1, min_pairs=6)
    for k in range(MAX_REDRAWS):
        s = render_pair(H, W, scene_intr(H, W) if whole else window_intr(H, W), False, k)
        T = starts(s["R"], s["t"], k)[1]
        ref = NDI.icp(s["depth0"], s["intr"], s["depth1"], s["intr"], T, **options)
        # the step is not compared on these maps, so its decisions (pivot, eps) do not count
        if not [f for f in ref["fragile"] if not (f.startswith("pivot") or f.startswith("|"))]:
            return _frozen(dict(s, start=T, options=options, ref=ref, redraws=k))
    raise AssertionError(f"no draw without a fragile decision for {(H, W, whole)}")
