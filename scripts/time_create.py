"""Where mpsfm_ba_create spends its time (host table build, uploads): python scripts/time_create.py [C3 | CAMS/POINTS] [CREATES]
A configuration of mpsfm_amd.synthetic.CONFIGS, or a scene of CAMS cameras and POINTS landmarks with depth priors (12/4000: the
local bundle adjustment of DESIGN.md §4b-2).  CREATES (default 3) handles are created one after the other; the minimum is printed last."""
import sys, time
sys.path.insert(0, '.')
from mpsfm_amd import capi
from mpsfm_amd.synthetic import make_config, make_scene
name = sys.argv[1] if len(sys.argv) > 1 else "C3"
prob, _ = make_scene(*(int(x) for x in name.split("/")), True, seed=3) if "/" in name else make_config(name)
times = []
for i in range(int(sys.argv[2]) if len(sys.argv) > 2 else 3):
    t0 = time.perf_counter(); h = capi.BAHandle(prob); t1 = time.perf_counter(); h.close()
    times.append(1e3 * (t1 - t0))
    print("create %.2f ms" % times[-1], flush=True)
print("create min %.3f ms of %d" % (min(times), len(times)), flush=True)
o = capi.default_options(verbose=2)
h = capi.BAHandle(prob, options=o); h.close()
for i in range(3):
    p = prob.copy(); t0 = time.perf_counter(); s = capi.ba_solve(p); t1 = time.perf_counter()
    print("one-shot %.2f ms (%d iterations, solve %.2f ms)" % (1e3 * (t1 - t0), s["num_iterations"], 1e3 * s["time_total_s"]), flush=True)
capi.ba_solve(prob.copy(), o)
