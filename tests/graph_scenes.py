"""Bundle-adjustment scenes whose variable-camera co-visibility graph is a GIVEN graph.

`make_scene` only ever produces an orbit: every camera shares landmarks with its azimuth neighbours.  The dense solve picks
its factorisation and substitution paths by the size and the structure of the camera graph, so its tests need the other
graphs too: path, star, complete, lattice, random, cameras that share nothing with anyone, separate scenes.  Here every
edge of the graph gets its own two-view landmarks and nothing else couples two variable cameras."""

import numpy as np

from mpsfm_amd.problem import BAProblem
from mpsfm_amd.synthetic import CX, CY, FX, FY, make_scene

BOX = np.array([2.0, 2.0, 1.5])  # landmarks in [-2,2]^2 x [-1.5,1.5]: in front of every camera of the orbit of radius 10
ANCHORS = 4                      # landmarks every variable camera shares with camera 0 only


def ring_graph(n, reach, extra=0, seed=0):
    """Cameras on a closed orbit, every camera sharing landmarks with the `reach` next ones, plus a few random long links."""
    rng = np.random.default_rng(seed)
    adj = np.zeros((n, n), np.uint8)
    for i in range(n):
        for d in range(1, reach + 1):
            adj[i, (i + d) % n] = adj[(i + d) % n, i] = 1
    for _ in range(extra):
        a, b = rng.integers(0, n, 2)
        if a != b:
            adj[a, b] = adj[b, a] = 1
    return adj


def graph(kind, n, seed=0):
    """Adjacency (n x n, uint8, symmetric, zero diagonal).  path, star, complete, grid, random and isolated are the graphs of
    test_chol_plan_cpu (same definitions, same seeds give the same graphs); star_last has its hub as the last node,
    two_rings is two separate orbits of n / 2 cameras with reach 4, ring_links an orbit with reach 5 and two long links."""
    rng = np.random.default_rng(seed)
    adj = np.zeros((n, n), np.uint8)
    if kind == "path":
        for i in range(n - 1):
            adj[i, i + 1] = 1
    elif kind == "star":
        adj[0, 1:] = 1
    elif kind == "star_last":
        adj[n - 1, :n - 1] = 1
    elif kind == "complete":
        adj[:] = 1
    elif kind == "grid":
        w = int(np.sqrt(n))
        for i in range(n):
            for d in (1, w, w + 1, w - 1):
                j = i + d
                if j < n and not (d == 1 and j % w == 0):
                    adj[i, j] = 1
    elif kind == "random":
        m = rng.random((n, n)) < 6.0 / n
        adj[m] = 1
    elif kind == "isolated":
        for i in range(40):
            for d in (1, 2, 3):
                if i + d < 40:
                    adj[i, i + d] = 1
        adj[50:62, 50:62] = 1
    elif kind == "two_rings":
        assert n % 2 == 0
        a = ring_graph(n // 2, 4)
        adj[:n // 2, :n // 2] = a
        adj[n // 2:, n // 2:] = a
    elif kind == "ring_links":
        adj = ring_graph(n, 5, extra=2, seed=seed)
    else:
        raise ValueError(kind)
    adj = np.maximum(adj, adj.T)
    np.fill_diagonal(adj, 0)
    return adj


def _R(q):
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)


def graph_scene(adj, per_edge=2, seed=0, with_depth=True):
    """BAProblem with adj.shape[0] + 1 cameras: camera 0 constant, camera i + 1 is node i of the graph.  Two variable cameras
    share a landmark exactly where `adj` has an edge (`per_edge` two-view landmarks each); every variable camera also shares
    ANCHORS landmarks with camera 0, which keeps leaves and isolated cameras determined without adding an edge.  Poses,
    intrinsics, their perturbation, noise, outliers, depth priors and the loss settings are those of make_scene."""
    adj = np.asarray(adj)
    n = adj.shape[0]
    assert adj.shape == (n, n) and (adj == adj.T).all() and not np.diag(adj).any()
    base, truth = make_scene(n + 1, 2, with_depth, seed=seed)  # the cameras depend on the seed only
    rng = np.random.default_rng([seed, 7])
    ei, ej = np.nonzero(np.triu(adj, 1))
    cam_a = np.concatenate([np.repeat(ei + 1, per_edge), np.repeat(np.arange(1, n + 1), ANCHORS)])
    cam_b = np.concatenate([np.repeat(ej + 1, per_edge), np.zeros(n * ANCHORS, np.int64)])
    n_pts = cam_a.size
    X = rng.uniform(-BOX, BOX, (n_pts, 3))
    obs_cam = np.stack([cam_a, cam_b], axis=1).ravel()
    obs_pt = np.repeat(np.arange(n_pts), 2)
    Xc = np.einsum("oij,oj->oi", _R(truth["cam_quat"])[obs_cam], X[obs_pt]) + truth["cam_t"][obs_cam]
    z = Xc[:, 2]
    assert (z > 0.5).all(), "a landmark behind (or too near) one of its cameras"
    n_obs = obs_cam.size
    xy = np.stack([FX * Xc[:, 0] / z + CX, FY * Xc[:, 1] / z + CY], axis=1) + rng.normal(0.0, 1.0, (n_obs, 2))
    out = rng.uniform(size=n_obs) < 0.05
    xy[out] += rng.uniform(-20.0, 20.0, (int(out.sum()), 2))
    xy = xy.astype(np.float16).astype(np.float64)
    kw = {}
    if with_depth:
        sigma_l = 0.0263
        d = z * np.exp(rng.normal(0.0, sigma_l, n_obs))
        d[rng.uniform(size=n_obs) < 0.03] *= 1.5
        valid = rng.uniform(size=n_obs) >= 0.10
        var = np.maximum((sigma_l * d) ** 2, 0.02 ** 2)
        kw = dict(dobs_cam=obs_cam[valid], dobs_pt=obs_pt[valid], dobs_depth=d[valid],
                  dobs_magnitude=(d ** 2 / np.clip(var, 1e-6, None))[valid], dobs_param=(2.0 * np.sqrt(var) / d)[valid],
                  depth_loss_type=base.depth_loss_type)
    return BAProblem(
        cam_quat=base.cam_quat, cam_t=base.cam_t, pts=X + rng.normal(0.0, 0.05, (n_pts, 3)), cam_intr=base.cam_intr,
        cam_intr_idx=base.cam_intr_idx, pose_const=base.pose_const, pt_const=np.zeros(n_pts, np.uint8),
        obs_cam=obs_cam, obs_pt=obs_pt, obs_xy=xy, gauge_axis_cam=base.gauge_axis_cam,
        reproj_loss_type=base.reproj_loss_type, reproj_loss_scale=base.reproj_loss_scale,
        reproj_loss_magnitude=base.reproj_loss_magnitude, **kw)


def covisibility(prob):
    """Adjacency of the variable cameras (camera i + 1 -> node i) as the observations define it."""
    n = prob.n_cams - 1
    seen = np.zeros((prob.n_pts, prob.n_cams), bool)
    seen[prob.obs_pt, prob.obs_cam] = True
    co = (seen[:, 1:].T.astype(np.float32) @ seen[:, 1:].astype(np.float32)) > 0
    np.fill_diagonal(co, False)
    assert co.shape == (n, n)
    return co.astype(np.uint8)


# The cases of the dense-solve tests: name -> (kind, variable cameras, landmarks per edge, seed).  The smallest shapes that still
# reach the code: see DESIGN.md 4a-2 for which path each one is for.
TILE_EDGE = {f"complete{n}": ("complete", n, 2, n) for n in (1, 2, 5, 6, 16, 17, 21, 22)}
KINDS = {
    "path90": ("path", 90, 2, 90), "star70": ("star", 70, 2, 70), "star70_hub_last": ("star_last", 70, 2, 70),
    "complete40": ("complete", 40, 2, 40), "grid144": ("grid", 144, 2, 144), "random100": ("random", 100, 2, 100),
    "isolated75": ("isolated", 75, 2, 75), "two_rings60": ("two_rings", 120, 2, 60),
}
LARGE_STRUCTURED = {"ring343_links": ("ring_links", 343, 2, 343), "grid19x19": ("grid", 361, 2, 361)}
LARGE_DENSE = {"complete343": ("complete", 343, 1, 343), "complete348": ("complete", 348, 1, 348)}
CASES = {**TILE_EDGE, **KINDS, **LARGE_STRUCTURED, **LARGE_DENSE}

_cache = {}


def case(name):
    """(adjacency, problem) of a named case; built once per process, callers copy the problem before they change it."""
    if name not in _cache:
        kind, n, per_edge, seed = CASES[name]
        adj = graph(kind, n, seed)
        _cache[name] = (adj, graph_scene(adj, per_edge, seed))
    return _cache[name]
