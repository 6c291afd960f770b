"""The problems, radii and camera steps on which one Levenberg-Marquardt step is compared with tests/numpy_lm_step.py, and the
yardsticks of that comparison; shared by tests/test_lm_step_cpu.py and tests/test_gpu_update_once.py.

Scenes: the eight of tests/chunk_cap_scenes.py and the scene of tests/loss_pair_scenes.py under its nine loss pairs and once with
shift_logscale ("lp:<reprojection>:<depth>[:shift]").  Per scene: both RADII, and the camera steps "solve" (the reduced system's own
solution), "large" (that times loss_pair_scenes.LARGE_STEP) and "zero".

ETA_F64 and MCC_F64 are the largest landmark-step backward error (LMStep.eta_p) and model-cost-change measure (LMStep.mcc_measure) that
the float64 run of the restatement reaches against its long-double run over all of these, with the CPU oracle's camera step:
test_lm_step_cpu.py measures them again and fails when they are exceeded or when they are more than 1.5 times what it measures.  The
bounds of the kernels are 8 times these numbers: the margin is for the kernels' other summation order (DPP segmented scan, LDS atomics,
up to 253 records per landmark) and their one-ulp reciprocals and roots, neither of which is an error of the method."""

import functools

import chunk_cap_scenes as CS
import loss_pair_scenes as LP
import numpy_lm_step as NS
from oracle import cpu_oracle as O

RADII = (1e3, 3.0)  # test_gpu_chunk_caps.RADII
STEPS = {"solve": 1.0, "large": LP.LARGE_STEP, "zero": 0.0}
LP_NAMES = [f"lp:{r}:{d}" for r, d in LP.PAIRS] + ["lp:softl1:cauchy:shift"]
NAMES = list(CS.SCENES) + LP_NAMES
ALL_DENSE = CS.ALL_DENSE  # the scenes of chunk_cap_scenes whose handles take all four forms (every lp: scene does too)

ETA_F64 = 5.0e-13  # measured 4.79e-13: lp:cauchy:softl1, radius 3, the reduced system's own step
MCC_F64 = 4.0e-15  # measured 3.70e-15: lp:cauchy:trivial, radius 3, zero camera step
ETA_BOUND, MCC_BOUND = 8 * ETA_F64, 8 * MCC_F64


def problem(name):
    if name.startswith("lp:"):
        part = name.split(":")
        return LP.problem(part[1], part[2], shift_logscale=len(part) > 3)
    return CS.problem(name)


def environment_of(name):
    return {} if name.startswith("lp:") else CS.environment_of(name)


@functools.lru_cache(maxsize=None)
def oracle_systems(name):
    """radius -> oracle.reduced_system of the scene (column scales, camera step, landmark step, model cost change)"""
    prob = problem(name)
    return {r: O.reduced_system(prob, radius=r) for r in RADII}


@functools.lru_cache(maxsize=None)
def reference(name, radius, step):
    """The long-double step of the scene at `radius` behind the ORACLE's camera step times STEPS[step]."""
    ref = oracle_systems(name)[radius]
    return NS.LMStep(problem(name), ref["cam_scale"], ref["pt_scale"], ref["yc"] * STEPS[step], radius)
