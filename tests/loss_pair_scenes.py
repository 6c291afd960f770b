"""The scene that takes every (reprojection loss, depth loss) pair through the regimes of the robust weight, shared by
tests/test_lm_step_cpu.py (which asserts its coverage), tests/test_gpu_update_once.py and tests/test_gpu_loss_pairs.py.

chunk_cap_scenes.scene: 5 cameras (camera 0 constant), 300 tracks of 2 to 4 cameras, a depth prior on every observation.  On top of that
  - dobs_param log-uniform in [1e-3, 10] and dobs_magnitude log-uniform in [1e-2, 1e4], so that the ratio rd^2 / a^2 of the depth blocks
    leaves the narrow band one variance formula gives it;
  - 6 % of the observations moved by 200 .. 400 px and 6 % set to the projection at the problem's own initial state plus 0.003 px, so
    that s / a^2 of the reprojection blocks spans [1e-4, 1e4] as well;
  - 6 % of the depth priors off by a factor 3 either way, 6 % equal to the depth at the initial state to 1e-6 (relative)."""

import functools
import itertools

import numpy as np

import chunk_cap_scenes as CS
from mpsfm_amd.problem import LOSS_CAUCHY, LOSS_SOFT_L1, LOSS_TRIVIAL
from mpsfm_amd.synthetic import R_from_quat

LOSSES = {"trivial": LOSS_TRIVIAL, "softl1": LOSS_SOFT_L1, "cauchy": LOSS_CAUCHY}
PAIRS = list(itertools.product(LOSSES, LOSSES))  # (reprojection, depth)
LARGE_STEP = 50.0                                # the factor of the large-step case
ZMAX = 0.61685027506808491368                    # kQuatPolyMaxZ of csrc/common.h: |d|^2 up to which quat_plus takes its polynomials
SEED = 41


@functools.lru_cache(maxsize=None)
def _base():
    rng = np.random.default_rng(SEED)
    prob = CS.scene(5, CS.random_tracks(rng, 300, np.arange(5), 2, 4), seed=SEED, every_depth=True)
    n = prob.n_obs
    assert prob.n_dobs == n and (prob.dobs_cam == prob.obs_cam).all() and (prob.dobs_pt == prob.obs_pt).all()
    P = np.einsum("nij,nj->ni", R_from_quat(prob.cam_quat)[prob.obs_cam], prob.pts[prob.obs_pt]) + prob.cam_t[prob.obs_cam]
    K = prob.cam_intr[prob.cam_intr_idx[prob.obs_cam]]
    proj = np.stack([K[:, 0] * P[:, 0] / P[:, 2] + K[:, 2], K[:, 1] * P[:, 1] / P[:, 2] + K[:, 3]], 1)
    assert (P[:, 2] > 0.5).all()
    prob.dobs_param = np.exp(rng.uniform(np.log(1e-3), np.log(10.0), n))
    prob.dobs_magnitude = np.exp(rng.uniform(np.log(1e-2), np.log(1e4), n))
    u = rng.uniform(size=n)
    gross, exact = u < 0.06, (u >= 0.06) & (u < 0.12)
    ang = rng.uniform(0.0, 2 * np.pi, n)
    far = rng.uniform(200.0, 400.0, n)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    prob.obs_xy = np.where(gross[:, None], prob.obs_xy + far, np.where(exact[:, None], proj + rng.normal(0.0, 0.003, (n, 2)), prob.obs_xy))
    v = rng.uniform(size=n)
    dgross, dexact = v < 0.06, (v >= 0.06) & (v < 0.12)
    prob.dobs_depth = np.where(dgross, prob.dobs_depth * np.where(rng.uniform(size=n) < 0.5, 3.0, 1.0 / 3.0),
                               np.where(dexact, P[:, 2] * (1.0 + rng.normal(0.0, 1e-6, n)), prob.dobs_depth))
    return prob


def problem(reproj="softl1", depth="cauchy", shift_logscale=False, fixed=False):
    """A fresh copy of the scene under the given pair of losses.  shift_logscale: a shift and a log-scale per camera on the depth
    priors; fixed: two more constant cameras and every third landmark constant, so that blocks of a constant camera and a constant
    landmark exist (the fixed-cost records)."""
    prob = _base().copy()
    prob.reproj_loss_type, prob.depth_loss_type = LOSSES[reproj], LOSSES[depth]
    if shift_logscale:
        rng = np.random.default_rng([SEED, 2])
        prob.shift_logscale = np.stack([rng.uniform(-0.3, 0.3, prob.n_cams), rng.uniform(-0.05, 0.05, prob.n_cams)], 1)
    if fixed:
        prob.pose_const[[1, 3]] = 1
        prob.pt_const[::3] = 1
    return prob
