// The solve of libmpsfm_hip's bundle adjustment: the Levenberg-Marquardt control loop (Ceres 2.1 TrustRegionMinimizer semantics
// with the default pyceres.SolverOptions() that reference mpsfm/sfm/mapper/bundle_adjustment.py:285-293 uses), as a chain of
// launches or, for small problems, as one cooperative launch (local_lm.hip), and the core C ABI of include/mpsfm_hip.h: create,
// solve, state and cost.  All arithmetic on problem data runs in the HIP kernels behind ba_launch.h; this file decides the form of
// a solve once (solve_form: the only reader of the run-time switches), orders launches and reads the accept/reject decisions from a
// handful of scalars.  Handle creation: ba_build.hip; sums over ranks: ba_comm.hip; probes: ba_debug.hip, which enqueue the pieces
// of an iteration defined here with fields of the form overridden.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ba_handle.h"

namespace mpsfm {

LocalSkew g_local_skew;

// Every run-time switch of a solve is read here, per solve and per probe call, and combined with what the handle can do.
SolveForm solve_form(const mpsfm_ba_handle* h) {
  auto on = [](const char* name, int unset) { const char* e = std::getenv(name); return e ? (std::atoi(e) != 0 ? 1 : 0) : unset; };
  auto is = [](const char* name, const char* value) { const char* e = std::getenv(name); return e && std::strcmp(e, value) == 0; };
  SolveForm f{};
  f.sweep_order = on("MPSFM_SWEEP_ORDER", 1);
  f.entry_list = is("MPSFM_CHOL_ENTRY", "list");
  f.pt_handoff = on("MPSFM_PT_HANDOFF", 1) && h->d_pt_fac != nullptr;
  f.fused_prologue = on("MPSFM_FUSE_PROLOGUE", 1) && all_dense(h);
  f.fused_cam = on("MPSFM_FUSE_CAM", 1) && f.fused_prologue;
  // (the zero fill of the direct form rides on the fused prologue; d_red_cols exists only on one rank with all_dense and a level
  // plan that damps in its first launch: build_direct_tables)
  f.direct = f.fused_prologue && !is("MPSFM_ASSEMBLE", "launch") && h->d_red_cols != nullptr && !sharded(h) && h->n > 0 &&
             dense_level(&h->ov, &h->lp) && dense_pinv(h->d_dwork, h->nt, &h->ov, &h->lp) != nullptr;
  f.speculate = on("MPSFM_LM_SPECULATE", 1);
  f.force_split = on("MPSFM_LM_SPLIT", -1);
  f.can_split = f.speculate && !sharded(h) && f.fused_prologue;
  return f;
}

SweepArgs sweep_args(mpsfm_ba_handle* h, const SolveForm& f, double radius, const LmCtl* ctl) {
  SweepArgs a{};
  a.ctl = ctl;
  a.chunks = h->d_chunks; a.chunk_cams = h->d_chunk_cams; a.rec_cam = h->rt.rec_cam; a.rec_meta = h->rt.rec_meta;
  a.rec_xy = h->rt.rec_xy; a.rec_d = h->rt.rec_d; a.rec_m = h->rt.rec_m; a.rec_a = h->rt.rec_a;
  a.pt_rec_start = h->rt.pt_rec_start; a.pt_kv = h->rt.pt_kv; a.blk_desc = h->d_blk_desc; a.blk_ent_start = h->d_blk_ent_start; a.ents = h->d_ents;
  a.camtab = h->d_camtab; a.pts = h->d_pts; a.ps = h->d_ps; a.loss = h->loss;
  a.radius = radius; a.min_diag = h->opt.min_lm_diagonal; a.max_diag = h->opt.max_lm_diagonal; a.ncv = h->ncv; a.dbg = (g_dbg_flags >> 8) & 0xff;
  a.lhdr = h->d_lhdr; a.nlong = h->nlong; a.nchunks = h->nchunks; a.cam_slot = h->d_cam_slot; a.wl = h->d_wl;
  a.sky = h->sky;
  a.Sblk = h->d_Sblk; a.gc = h->d_gc; a.wv = h->d_wv; a.diagU = h->d_diagU; a.part = h->d_part; a.diagV = h->d_diagV;
  a.yc = h->d_yc; a.camtab2 = h->d_camtab2; a.pts2 = h->d_pts2; a.part2 = h->d_part2;
  a.slab = h->d_slab; a.chunk0 = 0;
  a.order = f.sweep_order ? h->d_sweep_order : nullptr;
  if (f.pt_handoff) a.pt_fac = h->d_pt_fac;  // written by the dense track sweep, read by the update sweep; nobody else looks
  return a;
}

// cost of the fixed records (constant camera and constant landmark) or of all the others at the current state, enqueued:
// out[0] reprojection, out[1] depth, out[2] bad count (device values)
static void launch_record_cost(mpsfm_ba_handle* h, bool fixed, double* out) {
  const RecTablesDev& r = h->rt;
  const int64_t nrec = fixed ? h->nfixed : h->nrec;
  const int nb = (int)std::min<int64_t>(1024, (nrec + kThreads - 1) / kThreads);
  const CostArgs c = fixed ? CostArgs{nrec, r.fx_cam, r.fx_pt, r.fx_meta, r.fx_xy, r.fx_d, r.fx_m, r.fx_a, h->d_camtab, h->d_pts, h->loss, h->d_costpart}
                           : CostArgs{nrec, r.rec_cam, r.rec_pt, r.rec_meta, r.rec_xy, r.rec_d, r.rec_m, r.rec_a, h->d_camtab, h->d_pts, h->loss, h->d_costpart};
  launch_cost_records(c, nb, h->stream);
  launch_reduce_cols(h->d_costpart, nb, 4, 3, 0u, out, h->stream);
}
static void launch_fixed_cost(mpsfm_ba_handle* h, double* out) {
  if (h->nfixed > 0) launch_record_cost(h, true, out);
}
// the same as host values, complete on return
static int cost_of_records(mpsfm_ba_handle* h, bool fixed, double* out3) {
  out3[0] = out3[1] = out3[2] = 0.0;
  if ((fixed ? h->nfixed : h->nrec) <= 0) return 0;
  launch_record_cost(h, fixed, h->d_scal);
  MPSFM_TRY(hipMemcpyAsync(h->h_scal, h->d_scal, sizeof(double) * 3, hipMemcpyDeviceToHost, h->stream));
  MPSFM_TRY(hipStreamSynchronize(h->stream));
  out3[0] = h->h_scal[0]; out3[1] = h->h_scal[1]; out3[2] = h->h_scal[2];
  return 0;
}

void unit_camtab(mpsfm_ba_handle* h) {
  launch_cam_scales(h->nc, h->d_cam_slot, h->d_cmask, h->d_diagU, 0, h->d_cs, h->stream);
  launch_build_camtab(h->nc, h->d_q, h->d_t, h->d_intr, h->d_intr_idx, h->d_cs, h->d_camtab, h->stream);
}
int prepare_scales(mpsfm_ba_handle* h, const SolveForm& f) {
  hipStream_t s = h->stream;
  launch_pt_scales(h->np, h->rt.pt_kv, h->d_diagV, 0, h->d_ps, s);
  unit_camtab(h);
  if (h->opt.jacobi_scaling) {
    MPSFM_TRY(hipMemsetAsync(h->d_diagU, 0, sizeof(double) * (size_t)std::max(h->n_user, 1), s));
    MPSFM_TRY(hipMemsetAsync(h->d_diagV, 0, sizeof(double) * 3 * (size_t)std::max<int64_t>(h->np, 1), s));
    launch_track_sweep(sweep_args(h, f, 1.0, nullptr), h->nchunks, true, s);
    if (int rc = allreduce_dev(h, h->d_diagU, h->n_user)) return rc;
    launch_cam_scales(h->nc, h->d_cam_slot, h->d_cmask, h->d_diagU, 1, h->d_cs, s);
    launch_pt_scales(h->np, h->rt.pt_kv, h->d_diagV, 1, h->d_ps, s);
    launch_build_camtab(h->nc, h->d_q, h->d_t, h->d_intr, h->d_intr_idx, h->d_cs, h->d_camtab, s);
  }
  MPSFM_TRY(hipGetLastError());
  h->scales_ready = true;
  return 0;
}

// dense chunks through their slabs (k_track_sweep_dense + k_reduce_slabs), the others and the long tracks through the general
// kernels (global atomics)
int launch_sweeps(mpsfm_ba_handle* h, SweepArgs a, bool direct, hipEvent_t* marks) {
  hipStream_t s = h->stream;
  launch_track_sweep_dense(a, h->n_dense, s);
  if (marks) MPSFM_TRY(hipEventRecord(marks[0], s));
  const DirectAsm da{h->d_red_cols, h->d_A, h->d_diag_col, h->nt};
  launch_reduce_slabs(h->d_red_dests, h->n_red_dests, h->d_red_srcs, h->d_slab, h->d_Sblk, h->d_gc, h->d_wv, h->d_diagU, a.ctl, s, direct ? &da : nullptr);
  if (marks) MPSFM_TRY(hipEventRecord(marks[1], s));
  a.chunk0 = h->n_dense;
  launch_track_sweep(a, h->nchunks - h->n_dense, false, s);
  return 0;
}

void direct_zero_args(mpsfm_ba_handle* h, SweepArgs& a) {
  a.red = h->d_gc; a.nred = h->red_count - h->sblk_count;  // Sblk is neither written nor read
  a.zero_p[0] = h->d_yc; a.zero_n[0] = h->n_user;
  a.zero_p[1] = h->d_diag_col; a.zero_n[1] = (int64_t)h->nt * 32;
  a.zero_A = h->d_A; a.zero_tiles = h->lp.d_asm_tiles; a.zero_ntiles = h->lp.n_asm;
  a.zero_P = dense_pinv(h->d_dwork, h->nt, &h->ov, &h->lp); a.zero_ptiles = h->lp.d_pinv_tiles; a.zero_nptiles = h->lp.n_pinv_tiles;
}

int run_track_sweep(mpsfm_ba_handle* h, const SolveForm& f, double radius, const LmCtl* ctl, bool in_loop) {
  hipStream_t s = h->stream;
  const bool adopt = in_loop && f.fused_prologue, direct = adopt && f.direct;
  if (!in_loop) launch_zero(h->d_red, h->red_count, ctl, s);
  SweepArgs a = sweep_args(h, f, radius, ctl);
  if (adopt) {
    a.adopt_on = 1; a.adopt_nc = h->nc;
    a.pts_rw = h->d_pts; a.q_rw = h->d_q; a.t_rw = h->d_t; a.camtab_rw = h->d_camtab; a.q2 = h->d_q2; a.t2 = h->d_t2;
    a.red = h->d_red; a.nred = h->red_count;
    if (direct) direct_zero_args(h, a);
  }
  if (int rc = launch_sweeps(h, a, direct)) return rc;
  if (h->nchunks + h->nlong > 0 && !(in_loop && !sharded(h)))
    launch_reduce_cols(h->d_part, h->nchunks + h->nlong, 4, 3, 1u << 2, h->d_redsc, s, sharded(h) ? nullptr : h->d_scal + U_X_COST,
                       sharded(h) ? (h->opt.rank > 0 ? h->opt.rank : 0) % kMaxRankSlots : -1);
  else if (sharded(h)) launch_gmax_to_slot(h->d_redsc, h->opt.rank > 0 ? h->opt.rank : 0, s);  // (a rank without chunks: its slot from the zeroed buffer)
  h->last_radius = radius;
  return 0;
}

void run_assemble(mpsfm_ba_handle* h, double radius, const LmCtl* ctl) {
  // the level-scheduled factorisation without inverse accumulators only touches the tiles of its plan
  const bool level = dense_level(&h->ov, &h->lp);
  double* pinv = dense_pinv(h->d_dwork, h->nt, &h->ov, &h->lp);
  const bool listed = level && !pinv;
  AssembleArgs as{h->sky, h->d_Sblk, h->d_gc, h->d_wv, h->d_diagU, h->ncv, h->n, h->nt, radius,
                  h->opt.min_lm_diagonal, h->opt.max_lm_diagonal, h->d_A, pinv, listed ? h->lp.d_asm_tiles : nullptr, listed ? h->lp.n_asm : 0,
                  h->lp.d_col_slot, h->n_user, (level && pinv) ? h->d_yc : nullptr, (level && pinv) ? h->lp.d_tile_live : nullptr, ctl};
  launch_assemble(as, h->stream);
}

int run_dense(mpsfm_ba_handle* h, const SolveForm& f, double radius, const LmCtl* ctl) {
  // d_fail is zero here: cleared at creation and re-armed by k_cam_update after every read
  if (h->n > 0) {
    if (!f.direct) run_assemble(h, radius, ctl);
    const DampArgs damp{h->d_diag_col, h->lp.d_col_slot, h->lp.d_level0, h->n, h->opt.min_lm_diagonal, h->opt.max_lm_diagonal, radius};
    h->ov.entry_list = f.entry_list;  // (the field launch_dense_solve reads)
    launch_dense_solve(h->d_A, h->d_dwork, h->nt, h->n, h->d_yc, h->d_fail, h->stream, &h->ov, &h->lp, ctl, f.direct ? &damp : nullptr);
  }
  return 0;
}

// k_cam_update unless the update sweep forms the candidate cameras itself (f.fused_cam: CamUpdArgs), then the update sweep
void enqueue_update(mpsfm_ba_handle* h, const SolveForm& f, double radius, const LmCtl* ctl) {
  const CamUpdArgs cu{1, h->nc, h->d_cam_slot, h->d_cam_of_slot, h->d_q, h->d_t, h->d_cs, h->d_gc, h->d_intr, h->d_intr_idx,
                      h->d_q2, h->d_t2, h->d_camtab2, h->d_scal, h->d_fail};
  if (!f.fused_cam)
    launch_cam_update(h->nc, h->d_cam_slot, h->d_q, h->d_t, h->d_cs, h->d_yc, h->d_gc, h->d_q2, h->d_t2, h->d_scal, h->stream,
                      h->d_intr, h->d_intr_idx, h->d_camtab2, h->d_fail, ctl);
  launch_update_sweep(sweep_args(h, f, radius, ctl), h->nchunks, h->stream, f.fused_cam ? &cu : nullptr);
}

// ---- what the two forms of the trust-region loop share ---------------------------------------------------------------------
static LmOpts lm_opts_of(const mpsfm_ba_options& o) {
  return LmOpts{o.function_tolerance, o.gradient_tolerance, o.parameter_tolerance, o.min_relative_decrease, o.max_trust_region_radius,
                o.min_trust_region_radius, o.max_num_iterations, o.max_num_consecutive_invalid_steps};
}
static LmCtl initial_ctl(const mpsfm_ba_options& o) {  // x_norm and fixed_cost are filled in on the device
  LmCtl c0;
  std::memset(&c0, 0, sizeof(c0));
  c0.radius = o.initial_trust_region_radius; c0.decrease_factor = 2.0;
  c0.term = kLmRunning; c0.check_gradient = 1;
  return c0;
}
// the verbose line of iteration `it` from the control block as that iteration left it
static void print_iteration(int it, const LmHead& l, double fixed_cost) {
  if (l.last_mcc > 0.0 && l.last_cand != DBL_MAX)
    std::fprintf(stderr, "[mpsfm_ba] it %3d cost %.9e cand %.9e rel %.3e radius %.3e |step| %.3e\n", it, l.last_x_cost + fixed_cost, l.last_cand + fixed_cost,
                 l.last_rel, l.radius, l.last_step_norm);
  else
    std::fprintf(stderr, "[mpsfm_ba] it %3d invalid step (chol_fail=%d mcc=%.3e) radius %.3e\n", it, l.last_chol_fail, l.last_mcc, l.radius);
}
// what a finished loop reports, from its last control block
static int summary_from_ctl(mpsfm_ba_handle* h, const LmCtl& last, mpsfm_ba_summary* sum) {
  h->last_radius = last.radius;
  sum->num_jacobian_evals = last.n_jac_evals;
  sum->num_residual_evals = (int64_t)h->nblocks_reduced_global * ((int64_t)last.n_cost_evals + last.n_jac_evals);
  if (last.term == kLmNumericError)
    return fail(MPSFM_ENUMERIC, "the initial point cannot be evaluated (non-finite residual or depth <= 0 in a log-depth block)");
  sum->initial_cost = last.initial_cost;
  sum->fixed_cost = last.fixed_cost;  // (one rank: formed on the device)
  sum->final_cost = last.cur_cost + last.fixed_cost;
  sum->num_iterations = last.iter;
  sum->num_successful_steps = last.n_success;
  sum->num_unsuccessful_steps = last.n_unsuccess;
  sum->termination = last.term;
  sum->final_radius = last.radius;
  sum->trace_len = last.trace_len;
  for (int i = 0; i < last.trace_len; ++i) { sum->trace_cost[i] = last.trace_cost[i]; sum->trace_radius[i] = last.trace_radius[i]; sum->trace_accepted[i] = last.trace_accepted[i]; }
  return 0;
}

// Small problems (local bundle adjustment): fixed cost, column scales, the trust-region loop and the state norm without a single
// host synchronisation before the end — the loop is ONE cooperative launch (local_lm.hip).  Returns kLocalRefused when the launch
// is not accepted (nothing has changed the state then: the launch chain takes over).
constexpr int kLocalRefused = 1;
// Shortest front half of an iteration (ev0 -> ev1, seconds) behind which the back half is enqueued only once the iteration before
// has been decided (solve_impl).  Twice the shortest front measured on MI355X, 19 us, where the forced split still did not lose
// (DESIGN.md, round 9): the host's wake-up from the event wait varies from call to call.
constexpr double kSplitMinFront = 40e-6;
// What both forms of the loop start from: the cost of the fixed records in three free slots of the zeroed scalar block (it stays on
// the device and enters the control block there), the column scales, the initial control block
static int enqueue_lm_preamble(mpsfm_ba_handle* h, const SolveForm& f) {
  MPSFM_TRY(hipMemsetAsync(h->d_scal, 0, sizeof(double) * U_COUNT, h->stream));
  launch_fixed_cost(h, h->d_scal + 12);
  if (int rc = prepare_scales(h, f)) return rc;
  h->h_ctl[0] = initial_ctl(h->opt);  // x_norm and fixed_cost: from the device scalars
  MPSFM_TRY(hipMemcpyAsync(h->d_ctl, &h->h_ctl[0], sizeof(LmCtl), hipMemcpyHostToDevice, h->stream));
  return 0;
}

static int solve_local(mpsfm_ba_handle* h, const SolveForm& f, mpsfm_ba_summary* sum) {
  hipStream_t s = h->stream;
  const mpsfm_ba_options& o = h->opt;
  unit_camtab(h);  // the camera table at the initial point (unit scales) for the fixed cost
  if (int rc = enqueue_lm_preamble(h, f)) return rc;
  MPSFM_TRY(hipMemsetAsync(h->d_local_acc, 0, sizeof(double) * 2 * kLocalAccDoubles, s));
  MPSFM_TRY(hipMemsetAsync(h->d_local_sync, 0, sizeof(int64_t) * 16, s));
  LocalArgs la{};
  la.A = sweep_args(h, f, 0.0, nullptr);  // (the hand-off: phase A -> phase D of the chunk's own workgroup)
  la.ctl = h->d_ctl;
  la.o = lm_opts_of(o);
  la.log = o.verbose > 0 ? h->d_local_log : nullptr;
  la.acc[0] = h->d_local_acc; la.acc[1] = h->d_local_acc + kLocalAccDoubles;
  la.part[0] = h->d_part; la.part[1] = h->d_part + (size_t)h->nchunks * 4;  // (nlong == 0 here; the chain only ever uses the first half)
  la.bar = reinterpret_cast<int32_t*>(h->d_local_sync); la.clk = reinterpret_cast<long long*>(h->d_local_sync + 1);
  la.ncv = h->ncv; la.nc = h->nc; la.nchunks = h->nchunks;
  la.q = h->d_q; la.t = h->d_t; la.camtab = h->d_camtab; la.pts = h->d_pts; la.cs = h->d_cs; la.fixed_parts = h->d_scal + 12;
  la.skew_chunk = g_local_skew.chunk; la.skew_mask = g_local_skew.ticks > 0 ? g_local_skew.mask : 0; la.skew_ticks = g_local_skew.ticks;
  if (launch_local_lm(la, s) != (int)hipSuccess) {
    (void)hipGetLastError();
    MPSFM_TRY(hipStreamSynchronize(s));  // the pinned control block is free again
    return kLocalRefused;
  }
  static_assert(sizeof(int64_t) * 8 <= sizeof(double) * U_COUNT * 2, "the pinned scalar block holds the sync words");
  int64_t* hs = reinterpret_cast<int64_t*>(h->h_scal);
  MPSFM_TRY(hipMemcpyAsync(&h->h_ctl[0], h->d_ctl, sizeof(LmCtl), hipMemcpyDeviceToHost, s));
  MPSFM_TRY(hipMemcpyAsync(hs, h->d_local_sync, sizeof(int64_t) * 8, hipMemcpyDeviceToHost, s));
  MPSFM_TRY(hipStreamSynchronize(s));
  MPSFM_TRY(hipGetLastError());
  if (reinterpret_cast<const int32_t*>(hs)[1] != 0)
    return fail(MPSFM_EHIP, "single-launch solver: a grid barrier did not complete (workgroups not co-resident?); MPSFM_LOCAL_LM=0 selects the launch chain");
  const LmCtl& last = h->h_ctl[0];
  sum->fixed_cost = last.fixed_cost;
  sum->time_linearize_s = 1e-8 * (double)(hs[1] + hs[2]); sum->time_dense_s = 1e-8 * (double)hs[3]; sum->time_update_s = 1e-8 * (double)(hs[4] + hs[5] + hs[6]);
  if (o.verbose > 0) {
    const int nlog = std::min(last.iter + 1, h->local_log_cap);
    std::vector<LmHead> log((size_t)std::max(nlog, 0));
    if (nlog > 0) MPSFM_TRY(hipMemcpy(log.data(), h->d_local_log, sizeof(LmHead) * (size_t)nlog, hipMemcpyDeviceToHost));
    for (int i = 0; i < nlog; ++i)
      if (log[(size_t)i].iter == i + 1 || i == nlog - 1) print_iteration(i + 1, log[(size_t)i], last.fixed_cost);
  }
  return summary_from_ctl(h, last, sum);
}

static int solve_impl(mpsfm_ba_handle* h, mpsfm_ba_summary* sum) {
  using clk = std::chrono::steady_clock;
  MPSFM_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const mpsfm_ba_options& o = h->opt;
  const SolveForm f = solve_form(h);  // decided once: solve_local and every launch below take it from here
  std::memset(sum, 0, sizeof(*sum));
  MPSFM_TRY(hipStreamSynchronize(s));
  const auto t_begin = clk::now();
  sum->num_residual_blocks = (int64_t)h->nblocks_global;
  sum->reduced_dim = h->n_user;
  std::fill(g_launches, g_launches + kLfCount, (int64_t)0);
  auto finish = [&](int rc) {
    std::copy(g_launches, g_launches + kLfCount, h->last_launches);
    sum->time_total_s = std::chrono::duration<double>(clk::now() - t_begin).count();
    return rc;
  };
  if (h->local_ok) {
    const int rc = solve_local(h, f, sum);
    if (rc != kLocalRefused) return finish(rc);
  }

  unit_camtab(h);  // the camera table at the initial point (unit scales) for the fixed cost
  if (h->n == 0 && h->nvarpts_global == 0.0) {  // nothing to solve: the two costs as host values
    double fx[3], c3[3];
    if (int rc = cost_of_records(h, true, fx)) return rc;
    double fixed = fx[0] + fx[1];
    if (int rc = allreduce_host(h, &fixed, 1)) return rc;
    sum->fixed_cost = fixed;
    if (int rc = cost_of_records(h, false, c3)) return rc;
    double c = c3[0] + c3[1];
    if (int rc = allreduce_host(h, &c, 1)) return rc;
    sum->initial_cost = sum->final_cost = c + fixed;
    sum->termination = MPSFM_TERM_NO_VARIABLES;
    return finish(0);
  }
  // Nothing in front of the loop needs the host — the cost of the fixed blocks and the state norm stay on the device and enter
  // the control block there (k_lm_init); three stream synchronisations less per solve.  Sharded runs sum them over the ranks
  // in one small exchange on the device.
  if (int rc = enqueue_lm_preamble(h, f)) return rc;
  if (h->np > 0) MPSFM_TRY(hipMemcpyAsync(h->d_pts2, h->d_pts, sizeof(double) * 3 * h->np, hipMemcpyDeviceToDevice, s));
  // initial x norm: cameras through a zero-step camera update, landmarks by a reduction
  MPSFM_TRY(hipMemsetAsync(h->d_yc, 0, sizeof(double) * (size_t)std::max(h->n_user, 1), s));
  MPSFM_TRY(hipMemsetAsync(h->d_gc, 0, sizeof(double) * (size_t)std::max(h->n_user, 1), s));
  launch_cam_update(h->nc, h->d_cam_slot, h->d_q, h->d_t, h->d_cs, h->d_yc, h->d_gc, h->d_q2, h->d_t2, h->d_scal, s);
  const int nb = (int)std::min<int64_t>(1024, std::max<int64_t>(1, (h->np + kThreads - 1) / kThreads));
  launch_pts_sqnorm(h->np, h->rt.pt_kv, h->d_pts, h->d_costpart, nb, s);
  launch_reduce_cols(h->d_costpart, nb, 1, 1, 0u, h->d_scal + U_XN_SQ_PTS, s);

  // ---- Levenberg-Marquardt loop.  The decisions are taken on the device (k_lm_decide, LmCtl in common.h): the host
  // enqueues iteration i+1 BEFORE it looks at the outcome of iteration i, so the stream never runs dry, and only reads a
  // pinned copy of the control block one iteration late.  When that copy says the solve is over, what is queued
  // ahead returns at once in every kernel.  Every rank of a sharded run sees the same decisions at the same iteration, so
  // all of them enqueue the same sequence of collectives.
  //   Queued ahead is the whole iteration, or only its front half (sweeps and slab reduction) with the back half (dense solve ...
  // decision) following once the outcome of iteration i is known to be "go on": the solve then ends with two dead launches instead
  // of some twenty.  The host has the front's run time to wake up, read the control block and enqueue the first back launch, so
  // the split is taken where the front measured long enough for that (kSplitMinFront), on one rank and with all chunks dense.
  double* sums = nullptr;
  if (sharded(h)) {
    sums = h->d_costpart;  // (free again: its reductions are queued in front)
    launch_lm_pack(h->d_scal, sums, s);
    if (int rc = allreduce_dev(h, sums, 3)) return rc;
  }
  launch_lm_init(h->d_ctl, h->d_scal, sums, s);
  const LmOpts lo = lm_opts_of(o);
  const LmCtl* ctl = h->d_ctl;
  const double no_radius = 0.0;  // inside the loop the kernels read the radius from the control block
  auto enqueue_front = [&](int it) -> int {
    hipEvent_t* ev = (it & 1) ? h->ev2 : h->ev;
    MPSFM_TRY(hipEventRecord(ev[0], s));
    if (!f.fused_prologue)
      launch_lm_prologue(h->d_ctl, h->d_red, h->red_count, h->nc, h->np, h->d_q, h->d_t, h->d_camtab, h->d_pts, h->d_q2, h->d_t2, h->d_camtab2, h->d_pts2, s);
    if (int rc = run_track_sweep(h, f, no_radius, ctl, /*in_loop=*/true)) return rc;
    if (int rc = allreduce_dev(h, h->d_red, h->red_count)) return rc;
    MPSFM_TRY(hipEventRecord(ev[1], s));
    return 0;
  };
  auto enqueue_back = [&](int it) -> int {
    hipEvent_t* ev = (it & 1) ? h->ev2 : h->ev;
    if (int rc = run_dense(h, f, no_radius, ctl)) return rc;
    MPSFM_TRY(hipEventRecord(ev[2], s));
    enqueue_update(h, f, no_radius, ctl);
    if (!sharded(h)) {
      launch_lm_reduce_decide(h->d_part, h->d_part2, h->nchunks + h->nlong, h->d_ctl, h->d_scal, lo, &h->h_ctl[it & 1], s);
    } else {
      if (h->nchunks + h->nlong > 0) launch_reduce_cols(h->d_part2, h->nchunks + h->nlong, 8, 5, 0u, h->d_scal, s);
      if (int rc = allreduce_dev(h, h->d_scal, 5)) return rc;
      // the all-reduced scalars of the track sweep: cost and bad count summed, landmark-gradient maximum over the rank slots
      launch_lm_decide(h->d_ctl, h->d_scal, lo, &h->h_ctl[it & 1], s, h->d_redsc);
    }
    MPSFM_TRY(hipEventRecord(ev[3], s));
    return 0;
  };
  auto enqueue_iteration = [&](int it) -> int {
    if (int rc = enqueue_front(it)) return rc;
    return enqueue_back(it);
  };
  LmCtl last = h->h_ctl[0];
  if (last.term == kLmRunning) {
    if (int rc = enqueue_iteration(1)) return rc;
    for (int it = 1;; ++it) {
      // ahead of the news about iteration `it`; the front's length: ev0 -> ev1 of the last iteration read (this handle's previous solve at first)
      // (MPSFM_LM_SPLIT forces the choice between the whole iteration and its front half where the split is possible at all)
      const bool split = f.can_split && (f.force_split >= 0 ? f.force_split == 1 : h->split_front_s >= kSplitMinFront);
      if (f.speculate) { if (int rc = split ? enqueue_front(it + 1) : enqueue_iteration(it + 1)) return rc; }
      hipEvent_t* ev = (it & 1) ? h->ev2 : h->ev;
      MPSFM_TRY(hipEventSynchronize(ev[3]));
      MPSFM_TRY(hipGetLastError());
      float ms;
      MPSFM_TRY(hipEventElapsedTime(&ms, ev[0], ev[1])); sum->time_linearize_s += 1e-3 * ms;
      h->split_front_s = 1e-3 * ms;
      MPSFM_TRY(hipEventElapsedTime(&ms, ev[1], ev[2])); sum->time_dense_s += 1e-3 * ms;
      MPSFM_TRY(hipEventElapsedTime(&ms, ev[2], ev[3])); sum->time_update_s += 1e-3 * ms;
      last = h->h_ctl[it & 1];
      if (o.verbose > 0) print_iteration(it, last, last.fixed_cost);
      if (last.term != kLmRunning) break;
      if (!f.speculate) { if (int rc = enqueue_iteration(it + 1)) return rc; }
      else if (split) { if (int rc = enqueue_back(it + 1)) return rc; }
    }
    // the iteration that ended the solve may have been accepted (iteration or radius limit); the copy is idempotent
    launch_lm_accept(h->d_ctl, h->nc, h->np, h->d_q, h->d_t, h->d_camtab, h->d_pts, h->d_q2, h->d_t2, h->d_camtab2, h->d_pts2, s);
    MPSFM_TRY(hipStreamSynchronize(s));  // what was queued ahead has drained (every kernel of it returned at once)
  }
  return finish(summary_from_ctl(h, last, sum));
}
}  // namespace mpsfm

using namespace mpsfm;

// ---- C ABI ---------------------------------------------------------------------------------------
extern "C" {

int mpsfm_abi_version(void) { return MPSFM_ABI_VERSION; }
const char* mpsfm_last_error(void) { return g_err.c_str(); }

int mpsfm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  int good = 0;
  for (int i = 0; i < n; ++i) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, i) == hipSuccess && std::strncmp(p.gcnArchName, "gfx950", 6) == 0) ++good;
  }
  return good;
}

void mpsfm_ba_default_options(mpsfm_ba_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->max_num_iterations = 50;
  o->function_tolerance = 1e-6;
  o->gradient_tolerance = 1e-10;
  o->parameter_tolerance = 1e-8;
  o->initial_trust_region_radius = 1e4;
  o->max_trust_region_radius = 1e16;
  o->min_trust_region_radius = 1e-32;
  o->min_relative_decrease = 1e-3;
  o->min_lm_diagonal = 1e-6;
  o->max_lm_diagonal = 1e32;
  o->max_num_consecutive_invalid_steps = 5;
  o->jacobi_scaling = 1;
}

int mpsfm_ba_create(const mpsfm_ba_problem* problem, const mpsfm_ba_state* initial, const mpsfm_ba_options* options,
                    mpsfm_ba_handle** out) {
  return create_impl(problem, initial, options, out);
}

int mpsfm_ba_set_state(mpsfm_ba_handle* h, const mpsfm_ba_state* state) {
  if (!h) return fail(MPSFM_EINVAL, "handle is NULL");
  if (hipSetDevice(h->device) != hipSuccess) return fail(MPSFM_EHIP, "hipSetDevice failed");
  return upload_state(h, state, false);
}

int mpsfm_ba_reset_state(mpsfm_ba_handle* h) {
  if (!h) return fail(MPSFM_EINVAL, "handle is NULL");
  MPSFM_TRY(hipSetDevice(h->device));
  MPSFM_TRY(hipMemcpyAsync(h->d_q, h->d_q0, sizeof(double) * 4 * h->nc, hipMemcpyDeviceToDevice, h->stream));
  MPSFM_TRY(hipMemcpyAsync(h->d_t, h->d_t0, sizeof(double) * 3 * h->nc, hipMemcpyDeviceToDevice, h->stream));
  if (h->np > 0) MPSFM_TRY(hipMemcpyAsync(h->d_pts, h->d_pts0, sizeof(double) * 3 * h->np, hipMemcpyDeviceToDevice, h->stream));
  h->scales_ready = false;
  return 0;
}

int mpsfm_ba_solve_resident(mpsfm_ba_handle* h, mpsfm_ba_summary* summary) {
  if (!h || !summary) return fail(MPSFM_EINVAL, "handle or summary is NULL");
  return solve_impl(h, summary);
}

int mpsfm_ba_get_state(mpsfm_ba_handle* h, mpsfm_ba_state* st) {
  if (!h || !st) return fail(MPSFM_EINVAL, "handle or state is NULL");
  MPSFM_TRY(hipSetDevice(h->device));
  MPSFM_TRY(hipStreamSynchronize(h->stream));  // copies on the handle's own stream, never the legacy null stream (see solve_impl)
  if (h->nc > 0) {
    MPSFM_TRY(hipMemcpyAsync(st->cam_quat_xyzw, h->d_q, sizeof(double) * 4 * h->nc, hipMemcpyDeviceToHost, h->stream));
    MPSFM_TRY(hipMemcpyAsync(st->cam_t, h->d_t, sizeof(double) * 3 * h->nc, hipMemcpyDeviceToHost, h->stream));
  }
  if (h->d_perm) {  // back into the caller's order on the device, one copy straight into the caller's array
    launch_permute_pts(h->np, h->d_perm, h->d_pts, h->d_user_pts, true, h->stream);
    MPSFM_TRY(hipMemcpyAsync(st->pts, h->d_user_pts, sizeof(double) * 3 * h->np, hipMemcpyDeviceToHost, h->stream));
    MPSFM_TRY(hipStreamSynchronize(h->stream));
    return 0;
  }
  std::vector<double> sorted((size_t)h->np * 3);
  if (h->np > 0) MPSFM_TRY(hipMemcpyAsync(sorted.data(), h->d_pts, sizeof(double) * 3 * h->np, hipMemcpyDeviceToHost, h->stream));
  MPSFM_TRY(hipStreamSynchronize(h->stream));
  parallel_ranges(h->np, 16384, [&](int64_t k0, int64_t k1) {
    for (int64_t k = k0; k < k1; ++k) {
      double* d = st->pts + 3 * (size_t)h->perm[(size_t)k];
      d[0] = sorted[3 * (size_t)k]; d[1] = sorted[3 * (size_t)k + 1]; d[2] = sorted[3 * (size_t)k + 2];
    }
  });
  return 0;
}

void mpsfm_ba_destroy(mpsfm_ba_handle* h) { free_handle(h); }

int mpsfm_ba_solve(const mpsfm_ba_problem* problem, mpsfm_ba_state* state, const mpsfm_ba_options* options,
                   mpsfm_ba_summary* summary) {
  if (!state || !summary) return fail(MPSFM_EINVAL, "state or summary is NULL");
  mpsfm_ba_handle* h = nullptr;
  const Lap lap = stopwatch(options && options->verbose >= 2, "[mpsfm_ba] one-shot: %-25s %8.2f ms\n");
  int rc = create_impl(problem, state, options, &h);
  if (rc) return rc;
  lap("create");
  rc = solve_impl(h, summary);
  lap("solve");
  if (rc == 0) rc = mpsfm_ba_get_state(h, state);
  lap("get_state");
  free_handle(h);
  lap("destroy");
  return rc;
}

int mpsfm_ba_eval_cost(mpsfm_ba_handle* h, double* cost_reproj, double* cost_depth) {
  if (!h) return fail(MPSFM_EINVAL, "handle is NULL");
  MPSFM_TRY(hipSetDevice(h->device));
  unit_camtab(h);
  h->scales_ready = false;
  double a[3], b[3];
  if (int rc = cost_of_records(h, false, a)) return rc;
  if (int rc = cost_of_records(h, true, b)) return rc;
  if (cost_reproj) *cost_reproj = a[0] + b[0];
  if (cost_depth) *cost_depth = a[1] + b[1];
  return 0;
}

int mpsfm_ba_reduced_dim(mpsfm_ba_handle* h) { return h ? h->n_user : MPSFM_EINVAL; }

}  // extern "C"
