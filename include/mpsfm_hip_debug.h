/*
 * mpsfm_hip_debug.h - test and diagnostic hooks of libmpsfm_hip.so.
 *
 * These entry points are OUTSIDE the stable ABI of mpsfm_hip.h: the tests and the scripts under scripts/ call them, nothing
 * else should.  They may change or disappear without a change of MPSFM_ABI_VERSION.  The files that define them
 * (csrc/ba_debug.hip, csrc/dense_chol.hip, csrc/chol_plan.hip, csrc/dev_resources.hip) include this header, so every definition is checked
 * against its declaration; mpsfm_amd/abi.py declares the same signatures for ctypes (tests/test_abi_cpu.py compares).
 */
#ifndef MPSFM_HIP_DEBUG_H
#define MPSFM_HIP_DEBUG_H

#include "mpsfm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpsfm_plan_handle mpsfm_plan_handle;

/* process-wide ablation flags: bits 0-7 dense solve, bits 8-15 track sweep; 0: off */
void mpsfm_debug_set(int f);
/* registers a device buffer for the phase timeline of the factorisation (100 MHz stamps, 2 x 8 per step) with the solves launched from now on; NULL: off */
int mpsfm_debug_set_chol_trace(long long* dev_buf);
/* one workgroup factors the stacked host matrix dx [64][32] = [D; X] with `waves` (1 or 4) waves; out: L, X L^-T; *ok: every pivot positive */
int mpsfm_debug_panel_factor(const double* dx, int waves, double* out, int* ok);

/* the Cholesky plan of a camera graph, no device involved; adj: n x n bytes; depth -2: choose among the level-structure dissections, -3: what a handle
   does (the window-separator orders compete too), >= -1: that order; NULL on bad arguments */
mpsfm_plan_handle* mpsfm_debug_plan_create(const uint8_t* adj, int32_t n, int32_t depth, int32_t pinv_max_tiles, int32_t inv_rows);
/* frees a plan of mpsfm_debug_plan_create; NULL is allowed */
void mpsfm_debug_plan_destroy(mpsfm_plan_handle* h);
/* table `what` (0 header ... 13 col_of_slot, 14 the launch records as int32, 16 per item: see csrc/chol_plan.hip) of a plan; returns its length, copies min(length, cap) entries */
int64_t mpsfm_debug_plan_get(const mpsfm_plan_handle* h, int32_t what, int32_t* out, int64_t cap);

/* no device involved: `count` host blocks of `bytes` through the block cache twice; returns how many of the second round were recycled */
int64_t mpsfm_debug_host_cache(int64_t bytes, int32_t count);
/* no device involved: `reps` rounds of an `nparts`-part job through the table build's worker pool; returns the parts that did not run exactly once */
int64_t mpsfm_debug_run_parts(int32_t nparts, int32_t reps);
/* no device involved: the camera-graph union of `world` ranks (adj: world x n x n bytes) as the all-reduce computes it; out: n x n bytes; returns the digits per double */
int mpsfm_debug_graph_union(const uint8_t* adj, int32_t world, int32_t n, uint8_t* out);

/* 1: the handle's track sweep hands the landmark factors to its update sweep, 0: the update sweep recomputes them */
int mpsfm_debug_pt_handoff(mpsfm_ba_handle* h);
/* 1: a solve on this handle, under the switches set now, adds the slab sums straight into the tiles of the dense solve (no k_assemble), 0: it launches k_assemble */
int mpsfm_debug_direct_front(mpsfm_ba_handle* h);
/* one track sweep and slab reduction at `radius` in both forms: the tiles behind k_assemble and the tiles of the direct form ((nt+1)(nt+2)/2 x 1024 doubles each), damp [32 nt] (what the first level launch adds to the diagonal, -1: padding column), live [(nt+1)(nt+2)/2], info: nt, n, live tiles, accumulator and y words not left zero */
int mpsfm_debug_direct_assemble(mpsfm_ba_handle* h, double radius, double* A_parent, double* A_direct, double* damp, uint8_t* live, int64_t info[4]);
/* mpsfm_ba_dense_solve_once on the given system (S n x n and rhs in the caller's camera order, zero outside the handle's block pattern) instead of the last sweep's; *failed: a pivot was not positive */
int mpsfm_debug_dense_solve_given(mpsfm_ba_handle* h, const double* S, const double* rhs, int32_t n, int32_t* failed);
/* ONE update sweep at the handle's state, `radius` and the GIVEN camera step yc [n = reduced dim] (scaled coordinates, caller's camera order), behind a track sweep at `radius`;
   form: bit 0 hand-off of the landmark factors, bit 1 fused camera update (MPSFM_EUNSUPPORTED where the handle cannot take it).  Out: pts2 [n_pts][3] (caller's order; unreferenced
   landmarks untouched), q2 [n_cams][4], t2 [n_cams][3], part2 [rows = chunks + long tracks][8] (NaN before the launch), scal [8] = U_CAND_COST, U_BAD, U_MCC, U_STEP_SQ_PTS,
   U_XN_SQ_PTS, U_STEP_SQ_CAMS, U_XN_SQ_CAMS, U_GMAX_CAMS; cs [n_cams][6], ps [n_pts][3] (NULL allowed): the column scales the sweeps ran with.  The handle's state (cameras, landmarks) is not changed; its scratch is: the dense solution (yc takes its place), the reduced buffer, the scalars of the last sweep and the candidates */
int mpsfm_debug_update_once(mpsfm_ba_handle* h, double radius, const double* yc, int32_t n, int32_t form, double* pts2, double* q2, double* t2, double* part2, int64_t rows,
                            double* scal, double* cs, double* ps);
/* the first `count` 8-byte words of the landmark-diagonal buffer, where the dense sweep leaves its phase stamps under debug flag 128 */
int mpsfm_debug_read_trace(mpsfm_ba_handle* h, long long* out, int64_t count);
/* table `which` (numbering in csrc/ba_debug.hip) of the handle copied to `out` (at most `cap` bytes); returns its size in bytes or a negative error code */
int64_t mpsfm_debug_table(mpsfm_ba_handle* h, int32_t which, void* out, int64_t cap);
/* no device involved: builds the tables of `P` as mpsfm_ba_create does for a single rank, then as mpsfm_debug_table; rebuilds on every call */
int64_t mpsfm_debug_host_build(const mpsfm_ba_problem* P, int32_t which, void* out, int64_t cap);
/* phase clocks of the last single-launch solve, 100 MHz ticks; returns 0 when the handle does not take that path */
int mpsfm_debug_local_clocks(mpsfm_ba_handle* h, int64_t out[12]);
/* in every single-launch solve from now on workgroup `chunk` waits `ticks` (at most 200000) at each phase point of `phase_mask` (bits 0-4); (0, 0, 0): off */
int mpsfm_debug_local_skew(int32_t chunk, int32_t phase_mask, int64_t ticks);
/* the Levenberg-Marquardt control block of the device (LmCtl of csrc/common.h, field for field) and the options its decisions read (LmOpts) */
typedef struct mpsfm_debug_lm_ctl {
  double radius, decrease_factor, x_norm, cur_cost, fixed_cost, initial_cost;
  double last_x_cost, last_cand, last_rel, last_step_norm, last_mcc;
  int32_t term, iter, invalid_run, check_gradient, accepted, n_success, n_unsuccess, n_cost_evals, n_jac_evals, last_chol_fail, trace_len, pad_;
  double trace_cost[MPSFM_MAX_TRACE], trace_radius[MPSFM_MAX_TRACE];
  uint8_t trace_accepted[MPSFM_MAX_TRACE];
} mpsfm_debug_lm_ctl;
typedef struct mpsfm_debug_lm_opts {
  double function_tolerance, gradient_tolerance, parameter_tolerance, min_relative_decrease, max_radius, min_radius;
  int32_t max_iterations, max_invalid_steps;
} mpsfm_debug_lm_opts;
/* ONE launch of a decision kernel on the given block, through the solver's own launch wrappers, with a pinned host copy as its destination.
   form 0: k_lm_decide on scal [16]; 1: k_lm_decide with redsc (scal [16] and the all-reduced tail redsc [info[2]]); 2: k_lm_reduce_decide on scal [16] and the partial
   tables part [rows][4], part2 [rows][8].  The pinned copy starts as `fill` in every byte.  Out: ctl_out the device block, host_out the pinned copy, scal as the kernel
   left it.  info (may be NULL, filled also when every other argument is NULL): sizeof(LmHead), sizeof(LmCtl), the slots of redsc, the threads of k_lm_reduce_decide */
int mpsfm_debug_lm_decide(int32_t form, const mpsfm_debug_lm_ctl* ctl_in, const mpsfm_debug_lm_opts* opts, double* scal, const double* redsc, const double* part,
                          const double* part2, int64_t rows, int32_t fill, mpsfm_debug_lm_ctl* ctl_out, mpsfm_debug_lm_ctl* host_out, int64_t info[4]);
/* what the process holds of `device`'s caches: live device blocks, their bytes, and the pooled streams, events and pinned blocks handed out and not yet given back */
int mpsfm_debug_resources(int32_t device, int64_t out[5]);
/* the device paths of csrc/common.h's lean math over n items (at most 2^24).  kind 0: out[i] = lean_log(x[i]); 1: out[2i], out[2i + 1] = sin(t) / t and
   cos(t) for t^2 = x[i]; 2: out[4i ..] = quat_plus(q = x[7i .. 7i + 3], d = x[7i + 4 .. 7i + 6]) */
int mpsfm_debug_math_probe(int32_t kind, const double* x, int64_t n, double* out);

#ifdef __cplusplus
}
#endif
#endif /* MPSFM_HIP_DEBUG_H */
