// Test hooks, timing probes and table dumps of libmpsfm_hip: every mpsfm_debug_* entry point and the single-phase runs of the
// bundle adjustment (one sweep, one dense solve, the reduced system).  Nothing here is on the path of a solve; the single-phase runs
// enqueue the solve's own pieces (ba_handle.h) under a SolveForm whose fields they override, and read no switch themselves.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/mpsfm_hip_debug.h"
#include "ba_handle.h"

using namespace mpsfm;

// the ten numbers of mpsfm_ba_dense_plan; `work`: the dense workspace (only compared with NULL)
static void dense_plan_numbers(int ncv, int nt, const CholPlan& P, const DenseOverlap& ov, const LevelPlanDev& lp, double* work, int64_t sblk, int64_t v[10]) {
  const bool level = dense_level(&ov, &lp);
  const bool pinv = level && dense_pinv(work, nt, &ov, &lp) != nullptr;
  const int64_t w[10] = {ncv, nt, level ? P.nlevels : nt, P.nd_depth, pinv ? 1 : 0, (int64_t)P.items.size(), P.products, P.roles, sblk,
                         pinv ? 1 : (level ? P.nlevels : (nt + 3) / 4 + 1)};
  for (int i = 0; i < 10; ++i) v[i] = w[i];
}

// Test hook (tests/test_host_cpu.py; no device involved): takes and gives back `count` host blocks of `bytes` each through
// the block cache twice; returns how many blocks of the second round were recycled ones of the first (by address).
extern "C" int64_t mpsfm_debug_host_cache(int64_t bytes, int32_t count) {
  std::vector<mpsfm::HostBuf<uint8_t>> first((size_t)count), second((size_t)count);
  std::vector<const void*> seen;
  for (auto& b : first) { b.alloc((size_t)bytes); b[0] = 1; b[(size_t)bytes - 1] = 2; seen.push_back(b.data()); }
  first.clear();
  int64_t reused = 0;
  for (auto& b : second) {
    b.alloc((size_t)bytes);
    b[0] = 3;
    reused += std::find(seen.begin(), seen.end(), (const void*)b.data()) != seen.end() ? 1 : 0;
  }
  return reused;
}

// Test hook (tests/test_host_cpu.py; no device involved): `reps` rounds of an `nparts`-part job through the table build's
// worker pool; returns the number of parts that did not run exactly once.
extern "C" int64_t mpsfm_debug_run_parts(int32_t nparts, int32_t reps) {
  int64_t bad = 0;
  for (int r = 0; r < reps; ++r) {
    std::vector<std::atomic<int>> hits((size_t)std::max(nparts, 1));
    for (auto& x : hits) x.store(0);
    mpsfm::run_parts(nparts, [&](int t, int np) {
      if (np != std::max(nparts, 1) || t < 0 || t >= np) return;
      volatile double acc = 0.0;
      for (int k = 0; k < 2000; ++k) acc = acc + (double)k * 1e-9;  // a little work, so that parts overlap
      hits[(size_t)t].fetch_add(1);
    });
    for (auto& x : hits) bad += x.load() == 1 ? 0 : 1;
  }
  return bad;
}

// Test hook (tests/test_dist_cpu.py; no device involved): the camera-graph union of a landmark-sharded run as the ranks
// compute it — `world` adjacency matrices (n x n bytes each) packed per rank, summed like the all-reduce does, unpacked
// into `out` (n x n bytes).  Returns the digits per double used.
extern "C" int mpsfm_debug_graph_union(const uint8_t* adj, int32_t world, int32_t n, uint8_t* out) {
  std::vector<double> sum;
  for (int r = 0; r < world; ++r) {
    mpsfm::CamGraph g;
    g.init(n);
    for (int a = 0; a < n; ++a)
      for (int b = 0; b < n; ++b)
        if (adj[((size_t)r * n + a) * n + b]) g.set(a, b);
    std::vector<double> packed;
    mpsfm::pack_graph(g, world, packed);
    if (sum.empty()) sum.assign(packed.size(), 0.0);
    for (size_t i = 0; i < packed.size(); ++i) sum[i] += packed[i];
  }
  mpsfm::CamGraph u;
  u.init(n);
  mpsfm::unpack_graph(sum, world, u);
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b) out[(size_t)a * n + b] = u.get(a, b) ? 1 : 0;
  return mpsfm::graph_digits(world);
}

// Test hook (tests/test_gpu_lm_control.py): one launch of a decision kernel of the trust-region loop on a given control block, through
// the wrappers solve_impl calls and with a pinned block as the host copy's destination, as there.  The mirror structs of the header
// are LmCtl and LmOpts field for field:
#define MPSFM_SAME_FIELD(T, U, f) static_assert(offsetof(T, f) == offsetof(U, f) && sizeof(T::f) == sizeof(U::f), "mirror field " #f)
static_assert(sizeof(mpsfm_debug_lm_ctl) == sizeof(LmCtl) && sizeof(mpsfm_debug_lm_opts) == sizeof(LmOpts), "mirror sizes");
MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, radius); MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, decrease_factor); MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, x_norm);
MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, cur_cost); MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, fixed_cost); MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, initial_cost);
MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, last_x_cost); MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, last_cand); MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, last_rel);
MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, last_step_norm); MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, last_mcc); MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, term);
MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, iter); MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, invalid_run); MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, check_gradient);
MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, accepted); MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, n_success); MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, n_unsuccess);
MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, n_cost_evals); MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, n_jac_evals); MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, last_chol_fail);
MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, trace_len); MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, pad_); MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, trace_cost);
MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, trace_radius); MPSFM_SAME_FIELD(mpsfm_debug_lm_ctl, LmCtl, trace_accepted);
MPSFM_SAME_FIELD(mpsfm_debug_lm_opts, LmOpts, function_tolerance); MPSFM_SAME_FIELD(mpsfm_debug_lm_opts, LmOpts, gradient_tolerance);
MPSFM_SAME_FIELD(mpsfm_debug_lm_opts, LmOpts, parameter_tolerance); MPSFM_SAME_FIELD(mpsfm_debug_lm_opts, LmOpts, min_relative_decrease);
MPSFM_SAME_FIELD(mpsfm_debug_lm_opts, LmOpts, max_radius); MPSFM_SAME_FIELD(mpsfm_debug_lm_opts, LmOpts, min_radius);
MPSFM_SAME_FIELD(mpsfm_debug_lm_opts, LmOpts, max_iterations); MPSFM_SAME_FIELD(mpsfm_debug_lm_opts, LmOpts, max_invalid_steps);
#undef MPSFM_SAME_FIELD
static_assert(sizeof(LmCtl) <= kPinnedBytes, "the pinned block holds a control block");

extern "C" int mpsfm_debug_lm_decide(int32_t form, const mpsfm_debug_lm_ctl* ctl_in, const mpsfm_debug_lm_opts* opts, double* scal, const double* redsc,
                                     const double* part, const double* part2, int64_t rows, int32_t fill, mpsfm_debug_lm_ctl* ctl_out,
                                     mpsfm_debug_lm_ctl* host_out, int64_t info[4]) {
  if (info) { info[0] = (int64_t)sizeof(LmHead); info[1] = (int64_t)sizeof(LmCtl); info[2] = SC_COUNT; info[3] = kReduceThreads; }
  if (!ctl_in && !opts && !scal && !ctl_out && !host_out && info) return 0;  // the constants alone
  if (!ctl_in || !opts || !scal || !ctl_out || !host_out || form < 0 || form > 2) return fail(MPSFM_EINVAL, "block, options, scalars or output is NULL, or unknown form");
  if ((form == 1 && !redsc) || (form == 2 && (rows < 0 || (rows > 0 && (!part || !part2))))) return fail(MPSFM_EINVAL, "the form's tables are missing");
  if (ctl_in->trace_len < 0 || ctl_in->trace_len > MPSFM_MAX_TRACE) return fail(MPSFM_EINVAL, "trace_len outside the trace arrays");
  DeviceBlocks own;  // waits for the stream before the blocks go back
  hipStream_t s = nullptr;
  MPSFM_TRY(own.stream(&s));
  void* pinned = nullptr;
  MPSFM_TRY(own.pinned(&pinned));
  const size_t nrows = form == 2 ? (size_t)rows : 0;
  LmCtl* d_ctl = own.alloc<LmCtl>(1);
  double* d_scal = own.alloc<double>(U_COUNT);
  double* d_redsc = own.alloc<double>(SC_COUNT);
  double* d_part = own.alloc<double>(nrows * 4);
  double* d_part2 = own.alloc<double>(nrows * 8);
  if (!own.ok()) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  std::memset(pinned, fill & 0xff, sizeof(LmCtl));
  MPSFM_TRY(hipMemcpyAsync(d_ctl, ctl_in, sizeof(LmCtl), hipMemcpyHostToDevice, s));
  MPSFM_TRY(hipMemcpyAsync(d_scal, scal, sizeof(double) * U_COUNT, hipMemcpyHostToDevice, s));
  if (form == 1) MPSFM_TRY(hipMemcpyAsync(d_redsc, redsc, sizeof(double) * SC_COUNT, hipMemcpyHostToDevice, s));
  if (nrows > 0) {
    MPSFM_TRY(hipMemcpyAsync(d_part, part, sizeof(double) * nrows * 4, hipMemcpyHostToDevice, s));
    MPSFM_TRY(hipMemcpyAsync(d_part2, part2, sizeof(double) * nrows * 8, hipMemcpyHostToDevice, s));
  }
  LmOpts o;
  std::memcpy(&o, opts, sizeof(o));
  if (form == 2) launch_lm_reduce_decide(d_part, d_part2, rows, d_ctl, d_scal, o, static_cast<LmCtl*>(pinned), s);
  else launch_lm_decide(d_ctl, d_scal, o, static_cast<LmCtl*>(pinned), s, form == 1 ? d_redsc : nullptr);
  MPSFM_TRY(hipGetLastError());
  MPSFM_TRY(hipMemcpyAsync(ctl_out, d_ctl, sizeof(LmCtl), hipMemcpyDeviceToHost, s));
  MPSFM_TRY(hipMemcpyAsync(scal, d_scal, sizeof(double) * U_COUNT, hipMemcpyDeviceToHost, s));
  MPSFM_TRY(hipStreamSynchronize(s));
  std::memcpy(host_out, pinned, sizeof(LmCtl));
  return 0;
}

// Test hook (tests/test_gpu_lean_math.py): the device paths of the lean math of common.h over an array of n items.
// kind 0: out[i] = lean_log(x[i]);  kind 1: out[2i], out[2i + 1] = sin(n) / n and cos(n) for n^2 = x[i] (quat_sinc_cos, both sides
// of its branch);  kind 2: out[4i .. 4i + 3] = quat_plus(q = x[7i .. 7i + 3], d = x[7i + 4 .. 7i + 6]).
__global__ __launch_bounds__(256) void k_math_probe(int kind, const double* __restrict__ x, int64_t n, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (kind == 0) {
    out[i] = lean_log(x[i]);
  } else if (kind == 1) {
    double s, c;
    quat_sinc_cos(x[i], s, c);
    out[2 * i] = s; out[2 * i + 1] = c;
  } else {
    double q[4], d[3], o[4];
    for (int k = 0; k < 4; ++k) q[k] = x[7 * i + k];
    for (int k = 0; k < 3; ++k) d[k] = x[7 * i + 4 + k];
    quat_plus(q, d, o);
    for (int k = 0; k < 4; ++k) out[4 * i + k] = o[k];
  }
}
extern "C" int mpsfm_debug_math_probe(int32_t kind, const double* x, int64_t n, double* out) {
  if (kind < 0 || kind > 2 || n < 0 || n > (int64_t)1 << 24 || (n > 0 && (!x || !out))) return fail(MPSFM_EINVAL, "math probe: unknown kind, n outside [0, 2^24] or a NULL array");
  if (n == 0) return 0;
  const size_t nin = (size_t)n * (kind == 2 ? 7 : 1), nout = (size_t)n * (kind == 0 ? 1 : (kind == 1 ? 2 : 4));
  DeviceBlocks own;  // waits for the stream before the blocks go back
  hipStream_t s = nullptr;
  MPSFM_TRY(own.stream(&s));
  double* d_x = own.alloc<double>(nin);
  double* d_out = own.alloc<double>(nout);
  if (!own.ok()) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  MPSFM_TRY(hipMemcpyAsync(d_x, x, sizeof(double) * nin, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_math_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (int)kind, d_x, n, d_out);
  MPSFM_TRY(hipGetLastError());
  MPSFM_TRY(hipMemcpyAsync(out, d_out, sizeof(double) * nout, hipMemcpyDeviceToHost, s));
  MPSFM_TRY(hipStreamSynchronize(s));
  return 0;
}

extern "C" {

int mpsfm_ba_dense_plan(mpsfm_ba_handle* h, int64_t info[10]) {
  if (!h || !info) return fail(MPSFM_EINVAL, "handle or info is NULL");
  dense_plan_numbers(h->ncv, h->nt, h->plan, h->ov, h->lp, h->d_dwork, h->spat.nblk, info);
  return 0;
}

// 1: the handle's track sweep hands the landmark factors to its update sweep (every chunk dense, no long track; MPSFM_PT_HANDOFF=0
// still selects the recompute form per solve), 0: its update sweep recomputes them
int mpsfm_debug_pt_handoff(mpsfm_ba_handle* h) { return h && h->d_pt_fac != nullptr ? 1 : 0; }

// 1: a solve on this handle, under the switches set now, takes the direct form of the front (the slab reduction adds into the tiles of
// the dense solve, no k_assemble), 0: it launches k_assemble
int mpsfm_debug_direct_front(mpsfm_ba_handle* h) { return h && solve_form(h).direct ? 1 : 0; }

// Test hook (tests/test_gpu_direct_assemble.py): one track sweep and slab reduction at the current state and `radius` in both forms.
// A_parent: the tiles k_assemble leaves behind Sblk; A_direct: the tiles the direct slab reduction leaves, after the sweep's own zero
// fill — both (nt + 1)(nt + 2) / 2 x 1024 doubles; the tiles start as zeros (dead) and NaNs (live), the inverse accumulators the roles
// write, y and diag U by column as NaNs.  damp [32 nt]: what the first level launch adds to the diagonal of column g, -1: a padding
// column, set to 1.
// live [(nt + 1)(nt + 2) / 2]: 1 for the tiles the factorisation reads.  info: nt, n, live tiles, words of the inverse accumulators and
// of y that the direct form did not leave exactly zero.
int mpsfm_debug_direct_assemble(mpsfm_ba_handle* h, double radius, double* A_parent, double* A_direct, double* damp, uint8_t* live, int64_t info[4]) {
  if (!h || !A_parent || !A_direct || !damp || !live || !info) return fail(MPSFM_EINVAL, "handle or output is NULL");
  SolveForm f = solve_form(h);
  if (!f.direct) return fail(MPSFM_EUNSUPPORTED, "the handle does not take the direct form of the front");
  MPSFM_TRY(hipSetDevice(h->device));
  f.pt_handoff = f.fused_prologue = f.direct = false;  // the parent's form first; neither sweep starts writing pt_fac here
  if (!h->scales_ready) if (int rc = prepare_scales(h, f)) return rc;
  hipStream_t s = h->stream;
  const int nt = h->nt;
  const size_t ntiles = (size_t)(nt + 1) * (size_t)(nt + 2) / 2;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> img(ntiles * 1024, 0.0);
  std::fill(live, live + ntiles, (uint8_t)0);
  for (int32_t id : h->plan.asm_tiles) { live[(size_t)id] = 1; std::fill(img.begin() + (size_t)id * 1024, img.begin() + ((size_t)id + 1) * 1024, nan); }
  // the parent's form: zeroed reduced buffer, sweep, reduction into Sblk, k_assemble
  MPSFM_TRY(hipMemcpyAsync(h->d_A, img.data(), sizeof(double) * img.size(), hipMemcpyHostToDevice, s));
  if (int rc = run_track_sweep(h, f, radius, nullptr, /*in_loop=*/false)) return rc;
  run_assemble(h, radius);
  MPSFM_TRY(hipMemcpyAsync(A_parent, h->d_A, sizeof(double) * img.size(), hipMemcpyDeviceToHost, s));
  MPSFM_TRY(hipStreamSynchronize(s));
  // the direct form: the sweep zeroes, the reduction adds into the tiles — the front solve_impl enqueues, through run_track_sweep
  SweepArgs a{};
  direct_zero_args(h, a);  // (only to know what the zero fill covers)
  MPSFM_TRY(hipMemcpyAsync(h->d_A, img.data(), sizeof(double) * img.size(), hipMemcpyHostToDevice, s));
  for (int k = 0; k < 2; ++k) MPSFM_TRY(hipMemsetAsync(a.zero_p[k], 0xff, sizeof(double) * (size_t)a.zero_n[k], s));
  // the inverse accumulators: the ones the roles write as NaNs, the others are zero since the handle's creation and stay so
  const size_t npinv = (size_t)nt * (size_t)(nt + 1) / 2 * 1024;
  std::vector<double> pimg(npinv, 0.0);
  for (const CholItem& it : h->plan.items)
    if (it.type == kItemRole)
      for (uint32_t q = 0; q < it.nsrc; ++q) {
        const size_t id = (size_t)lt_tile(h->plan.rows[(size_t)it.aux + q], it.tk);
        std::fill(pimg.begin() + id * 1024, pimg.begin() + (id + 1) * 1024, nan);
      }
  MPSFM_TRY(hipMemcpyAsync(a.zero_P, pimg.data(), sizeof(double) * npinv, hipMemcpyHostToDevice, s));
  f.fused_prologue = f.direct = true;
  if (int rc = run_track_sweep(h, f, radius, nullptr, /*in_loop=*/true)) return rc;  // (no control block: nothing is adopted, the zero fill runs)
  std::vector<double> pinv(npinv), y((size_t)std::max(h->n_user, 1)), dcol((size_t)nt * 32);
  MPSFM_TRY(hipMemcpyAsync(A_direct, h->d_A, sizeof(double) * img.size(), hipMemcpyDeviceToHost, s));
  MPSFM_TRY(hipMemcpyAsync(pinv.data(), a.zero_P, sizeof(double) * pinv.size(), hipMemcpyDeviceToHost, s));
  MPSFM_TRY(hipMemcpyAsync(y.data(), h->d_yc, sizeof(double) * (size_t)h->n_user, hipMemcpyDeviceToHost, s));
  MPSFM_TRY(hipMemcpyAsync(dcol.data(), h->d_diag_col, sizeof(double) * dcol.size(), hipMemcpyDeviceToHost, s));
  MPSFM_TRY(hipStreamSynchronize(s));
  MPSFM_TRY(hipGetLastError());
  const int32_t* slot_of_col = h->plan.slot_of_col.empty() ? nullptr : h->plan.slot_of_col.data();
  for (int g = 0; g < nt * 32; ++g)
    damp[g] = vec_index(slot_of_col, g, h->n) < 0 ? -1.0 : std::min(std::max(dcol[(size_t)g], h->opt.min_lm_diagonal), h->opt.max_lm_diagonal) / radius;
  int64_t bad = 0;
  for (double v : pinv) bad += v == 0.0 ? 0 : 1;
  for (int i = 0; i < h->n_user; ++i) bad += y[(size_t)i] == 0.0 ? 0 : 1;
  info[0] = nt; info[1] = h->n; info[2] = (int64_t)h->plan.asm_tiles.size(); info[3] = bad;
  return 0;
}

int mpsfm_ba_sweep_once(mpsfm_ba_handle* h, double radius, float* elapsed_ms) {
  if (!h) return fail(MPSFM_EINVAL, "handle is NULL");
  MPSFM_TRY(hipSetDevice(h->device));
  SolveForm f = solve_form(h);
  f.pt_handoff = f.fused_prologue = f.direct = false;  // the plain sweep into the zeroed reduced buffer; pt_fac is not written
  if (!h->scales_ready) if (int rc = prepare_scales(h, f)) return rc;
  MPSFM_TRY(hipMemsetAsync(h->d_red, 0, sizeof(double) * (size_t)h->red_count, h->stream));
  // the three launches of the solve's sweep between events (mpsfm_ba_sweep_parts): ev0 and ev3 bracket them alone
  MPSFM_TRY(hipEventRecord(h->ev[0], h->stream));
  if (int rc = launch_sweeps(h, sweep_args(h, f, radius, nullptr), false, h->ev + 1)) return rc;
  MPSFM_TRY(hipEventRecord(h->ev[3], h->stream));
  if (h->nchunks + h->nlong > 0) launch_reduce_cols(h->d_part, h->nchunks + h->nlong, 4, 3, 1u << 2, h->d_redsc, h->stream);
  MPSFM_TRY(hipStreamSynchronize(h->stream));
  MPSFM_TRY(hipGetLastError());
  h->last_radius = radius;
  float ms = 0.f;
  MPSFM_TRY(hipEventElapsedTime(&ms, h->ev[0], h->ev[3]));
  if (elapsed_ms) *elapsed_ms = ms;
  return 0;
}

// Test hook (tests/test_gpu_update_once.py): ONE update sweep at the handle's current state, `radius` and a GIVEN camera step, in the
// form asked for.  The track sweep runs first through run_track_sweep (it leaves g_c for the gradient maximum and, with the hand-off,
// F and g_p of every landmark); then enqueue_update, the piece solve_impl's enqueue_back runs (camera update, update sweep), without a
// control block; then the reduction of part2 in the order of the one-rank loop (reduce_cols_block's, which k_lm_reduce_decide repeats).
// yc [n = reduced_dim]: the camera step in scaled coordinates, caller's camera order (what mpsfm_ba_get_dense_solution returns).
// form: bit 0 hand-off of the landmark factors (needs the handle's buffer), bit 1 fused camera update (needs every chunk dense and no
// long track); a form the handle cannot take is refused with MPSFM_EUNSUPPORTED.  Out: pts2 [n_pts][3] in the caller's landmark order
// (a landmark no block references keeps what the caller put there, as in mpsfm_ba_get_state), q2 [n_cams][4], t2 [n_cams][3], part2
// [rows][8] with rows = chunks + long tracks (NaN before the launch: columns 5-7 stay so), scal [8]: U_CAND_COST .. U_GMAX_CAMS; cs
// [n_cams][6] and ps [n_pts][3] (either may be NULL): the column scales the sweeps ran with, ps in the caller's order like pts2.  The
// state of the handle (cameras, landmarks) is not changed.  Its scratch is not preserved: d_yc holds the caller's step afterwards (so
// mpsfm_ba_get_dense_solution returns yc), the reduced buffer is the track sweep's at `radius`, d_scal loses what the last sweep left
// (U_X_COST among it), and the candidates (q2, t2, camtab2, pts2), part2 and pt_fac are this call's.
int mpsfm_debug_update_once(mpsfm_ba_handle* h, double radius, const double* yc, int32_t n, int32_t form, double* pts2, double* q2, double* t2,
                            double* part2, int64_t rows, double* scal, double* cs, double* ps) {
  if (!h || !pts2 || !q2 || !t2 || !scal) return fail(MPSFM_EINVAL, "handle or output is NULL");
  if (n != h->n_user || (n > 0 && !yc)) return fail(MPSFM_EINVAL, "n does not match the reduced dimension, or yc is NULL");
  if (!(radius > 0.0) || !std::isfinite(radius)) return fail(MPSFM_EINVAL, "radius must be positive and finite");
  if (form < 0 || form > 3) return fail(MPSFM_EINVAL, "form: bit 0 hand-off, bit 1 fused camera update");
  if (rows != (int64_t)h->nchunks + h->nlong || (rows > 0 && !part2)) return fail(MPSFM_EINVAL, "rows must be chunks + long tracks, part2 not NULL");
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(yc[i])) return fail(MPSFM_EINVAL, "yc is not finite");
  if (sharded(h)) return fail(MPSFM_EUNSUPPORTED, "update_once: one rank only");
  SolveForm f = solve_form(h);
  f.pt_handoff = (form & 1) != 0; f.fused_cam = (form & 2) != 0;  // the caller's form, whatever the switches say
  if (f.pt_handoff && !h->d_pt_fac) return fail(MPSFM_EUNSUPPORTED, "the handle has no hand-off buffer (a general chunk or a long track)");
  if (f.fused_cam && !all_dense(h)) return fail(MPSFM_EUNSUPPORTED, "the fused camera update needs every chunk dense and no long track");
  MPSFM_TRY(hipSetDevice(h->device));
  if (!h->scales_ready) if (int rc = prepare_scales(h, f)) return rc;
  hipStream_t s = h->stream;
  if (int rc = run_track_sweep(h, f, radius, nullptr, /*in_loop=*/false)) return rc;
  std::vector<double> ys((size_t)std::max(h->n_user, 1), 0.0);
  for (int i = 0; i < n; ++i) ys[(size_t)(6 * h->nat_slot[(size_t)(i / 6)] + i % 6)] = yc[i];
  MPSFM_TRY(hipMemcpyAsync(h->d_yc, ys.data(), sizeof(double) * ys.size(), hipMemcpyHostToDevice, s));
  if (h->np > 0) MPSFM_TRY(hipMemcpyAsync(h->d_pts2, h->d_pts, sizeof(double) * 3 * h->np, hipMemcpyDeviceToDevice, s));  // (as solve_impl: landmarks outside every chunk)
  if (rows > 0) MPSFM_TRY(hipMemsetAsync(h->d_part2, 0xff, sizeof(double) * 8 * (size_t)rows, s));  // NaN: a row no workgroup writes shows
  MPSFM_TRY(hipMemsetAsync(h->d_scal, 0xff, sizeof(double) * U_COUNT, s));
  enqueue_update(h, f, radius, nullptr);
  if (rows > 0) launch_reduce_cols(h->d_part2, rows, 8, 5, 0u, h->d_scal, s);
  std::vector<double> sorted((size_t)h->np * 3), sorted_ps((size_t)h->np * 3), sc((size_t)U_COUNT);
  if (h->np > 0) MPSFM_TRY(hipMemcpyAsync(sorted.data(), h->d_pts2, sizeof(double) * 3 * (size_t)h->np, hipMemcpyDeviceToHost, s));
  if (h->np > 0 && ps) MPSFM_TRY(hipMemcpyAsync(sorted_ps.data(), h->d_ps, sizeof(double) * 3 * (size_t)h->np, hipMemcpyDeviceToHost, s));
  if (h->nc > 0 && cs) MPSFM_TRY(hipMemcpyAsync(cs, h->d_cs, sizeof(double) * 6 * (size_t)h->nc, hipMemcpyDeviceToHost, s));
  if (h->nc > 0) {
    MPSFM_TRY(hipMemcpyAsync(q2, h->d_q2, sizeof(double) * 4 * (size_t)h->nc, hipMemcpyDeviceToHost, s));
    MPSFM_TRY(hipMemcpyAsync(t2, h->d_t2, sizeof(double) * 3 * (size_t)h->nc, hipMemcpyDeviceToHost, s));
  }
  if (rows > 0) MPSFM_TRY(hipMemcpyAsync(part2, h->d_part2, sizeof(double) * 8 * (size_t)rows, hipMemcpyDeviceToHost, s));
  MPSFM_TRY(hipMemcpyAsync(sc.data(), h->d_scal, sizeof(double) * U_COUNT, hipMemcpyDeviceToHost, s));
  MPSFM_TRY(hipStreamSynchronize(s));
  MPSFM_TRY(hipGetLastError());
  for (int64_t k = 0; k < h->np; ++k)
    for (int c = 0; c < 3; ++c) {
      pts2[3 * (size_t)h->perm[(size_t)k] + c] = sorted[3 * (size_t)k + c];
      if (ps) ps[3 * (size_t)h->perm[(size_t)k] + c] = sorted_ps[3 * (size_t)k + c];
    }
  for (int i = 0; i < 8; ++i) scal[i] = sc[(size_t)i];
  return 0;
}

// Diagnostics (scripts/dbg_sweep_trace.py): the first `count` 8-byte words of the landmark-diagonal buffer, where the dense sweep leaves
// its phase stamps under debug flag 128.
int mpsfm_debug_read_trace(mpsfm_ba_handle* h, long long* out, int64_t count) {
  if (!h || !out || count < 0 || count > 3 * std::max<int64_t>(h->np, 1)) return fail(MPSFM_EINVAL, "bad trace request");
  MPSFM_TRY(hipSetDevice(h->device));
  MPSFM_TRY(hipMemcpyAsync(out, h->d_diagV, sizeof(long long) * (size_t)count, hipMemcpyDeviceToHost, h->stream));
  MPSFM_TRY(hipStreamSynchronize(h->stream));
  return 0;
}

// Diagnostics / tests (tests/test_gpu_devbuild.py): table `which` of the handle copied to `out` (at most `cap` bytes); returns the
// table's size in bytes, or a negative error code.  which: 0 chunk headers, 1 chunk cameras, 2 rec_cam, 3 rec_pt, 4 rec_meta, 5 rec_xy,
// 6 rec_d, 7 rec_m, 8 rec_a, 9 pt_rec_start, 10 pt_kv, 11 fx_cam, 12 fx_pt, 13 fx_meta, 14 fx_xy, 15 fx_d, 16 fx_m, 17 fx_a,
// 18 landmark order (host), 19 reduction destinations, 20 reduction sources, 21 camera slots (host), 22: 1 byte, built on the device?,
// 23 blk_desc, 24 blk_ent_start, 25 ents (pair tables of the general chunks), 27 long-track headers, 28 sky_index, 29 sky_first,
// 30 sky_start (host), 31 cmask, 32 cam_of_slot, 33 the ten numbers of mpsfm_ba_dense_plan, 34 the launches the last solve on this
// handle enqueued (host, int64 each): track sweeps, k_reduce_slabs, k_assemble, k_chol_level, the rest of the dense solve, update
// sweeps, decisions, scales and camera table, everything else (LaunchFamily of ba_launch.h), 35 the order table of the dense sweep
// (int32 per dense chunk: the chunk the b-th workgroup takes), 36 dense_sweep_cost of every dense chunk (int32, from the headers),
// 37 the slabs as the last dense sweep left them (doubles, ChunkHdr::slab0 in units of 18), 38 pt_fac [np][9] as the last track sweep
// with the hand-off left it (empty: the handle has no such buffer)
int64_t mpsfm_debug_table(mpsfm_ba_handle* h, int32_t which, void* out, int64_t cap) {
  if (!h) return fail(MPSFM_EINVAL, "handle is NULL");
  const void* src = nullptr;
  int64_t bytes = 0;
  bool host = false;
  const int64_t nr = h->nrec, np1 = h->np + 1, nf = h->nfixed;
  switch (which) {
    case 0: src = h->d_chunks; bytes = (int64_t)sizeof(ChunkHdr) * h->nchunks; break;
    case 1: src = h->d_chunk_cams; bytes = 4 * h->n_chunk_cams; break;
    case 2: src = h->rt.rec_cam; bytes = 4 * nr; break;
    case 3: src = h->rt.rec_pt; bytes = 4 * nr; break;
    case 4: src = h->rt.rec_meta; bytes = 4 * nr; break;
    case 5: src = h->rt.rec_xy; bytes = 16 * nr; break;
    case 6: src = h->rt.rec_d; bytes = 8 * nr; break;
    case 7: src = h->rt.rec_m; bytes = 8 * nr; break;
    case 8: src = h->rt.rec_a; bytes = 8 * nr; break;
    case 9: src = h->rt.pt_rec_start; bytes = 4 * np1; break;
    case 10: src = h->rt.pt_kv; bytes = 2 * np1; break;
    case 11: src = h->rt.fx_cam; bytes = 4 * nf; break;
    case 12: src = h->rt.fx_pt; bytes = 4 * nf; break;
    case 13: src = h->rt.fx_meta; bytes = 4 * nf; break;
    case 14: src = h->rt.fx_xy; bytes = 16 * nf; break;
    case 15: src = h->rt.fx_d; bytes = 8 * nf; break;
    case 16: src = h->rt.fx_m; bytes = 8 * nf; break;
    case 17: src = h->rt.fx_a; bytes = 8 * nf; break;
    case 18: src = h->perm.data(); bytes = 4 * (int64_t)h->perm.size(); host = true; break;
    case 19: src = h->d_red_dests; bytes = (int64_t)sizeof(RedDest) * h->n_red_dests; break;
    case 20: src = h->d_red_srcs; bytes = 4 * h->n_red_srcs; break;
    case 21: src = h->cam_slot_h.data(); bytes = 4 * (int64_t)h->cam_slot_h.size(); host = true; break;
    case 23: src = h->d_blk_desc; bytes = 4 * h->n_blk_desc; break;
    case 24: src = h->d_blk_ent_start; bytes = 4 * h->n_blk_ent_start; break;
    case 25: src = h->d_ents; bytes = 4 * h->n_ents; break;
    case 26: src = h->d_part; bytes = 32 * (int64_t)h->nchunks; break;
    case 22: { static uint8_t flag; flag = h->built_on_device ? 1 : 0; src = &flag; bytes = 1; host = true; break; }
    case 27: src = h->d_lhdr; bytes = (int64_t)sizeof(LongHdr) * h->nlong; break;
    case 28: src = h->spat.sky_index.data(); bytes = 4 * (int64_t)h->spat.sky_index.size(); host = true; break;
    case 29: src = h->spat.sky_first.data(); bytes = 4 * (int64_t)h->spat.sky_first.size(); host = true; break;
    case 30: src = h->spat.sky_start.data(); bytes = 8 * (int64_t)h->spat.sky_start.size(); host = true; break;
    case 31: src = h->d_cmask; bytes = 48 * (int64_t)h->nc; break;
    case 32: src = h->d_cam_of_slot; bytes = 4 * (int64_t)std::max(h->ncv, 1); break;
    case 33: { static thread_local int64_t info[10]; if (int rc = mpsfm_ba_dense_plan(h, info)) return rc; src = info; bytes = 80; host = true; break; }
    case 34: src = h->last_launches; bytes = (int64_t)sizeof(h->last_launches); host = true; break;
    case 35: src = h->d_sweep_order; bytes = 4 * (int64_t)h->n_dense; break;
    case 36: {
      static thread_local std::vector<int32_t> cost;
      std::vector<ChunkHdr> hdr((size_t)h->n_dense);
      if (h->n_dense > 0) {
        if (hipSetDevice(h->device) != hipSuccess || hipMemcpy(hdr.data(), h->d_chunks, sizeof(ChunkHdr) * hdr.size(), hipMemcpyDeviceToHost) != hipSuccess)
          return fail(MPSFM_EHIP, "copy failed");
      }
      cost.resize(hdr.size());
      for (size_t c = 0; c < hdr.size(); ++c) cost[c] = dense_sweep_cost(hdr[c].nrec, hdr[c].npt, hdr[c].ncam);
      src = cost.data(); bytes = 4 * (int64_t)cost.size(); host = true;
      break;
    }
    case 37: src = h->d_slab; bytes = 144 * h->slab_units; break;
    case 38: src = h->d_pt_fac; bytes = h->d_pt_fac ? 72 * h->np : 0; break;
    default: return fail(MPSFM_EINVAL, "unknown table");
  }
  if (!out || cap < bytes) return bytes;
  if (bytes == 0) return 0;
  if (host) { std::memcpy(out, src, (size_t)bytes); return bytes; }
  if (hipSetDevice(h->device) != hipSuccess) return fail(MPSFM_EHIP, "hipSetDevice failed");
  if (hipMemcpyAsync(out, src, (size_t)bytes, hipMemcpyDeviceToHost, h->stream) != hipSuccess) return fail(MPSFM_EHIP, "copy failed");
  if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(MPSFM_EHIP, "sync failed");
  return bytes;
}

// Diagnostics / tests (tests/test_build_tables_cpu.py; no device involved): build_tables — the function mpsfm_ba_create runs — for
// a single rank and without the device stages on `P`, then table `which` copied out: numbering, arguments and return value of
// mpsfm_debug_table (26, 37 and 38 are work buffers and do not exist here; 35 and 36 come from the host sort).  Rebuilds on every call.
int64_t mpsfm_debug_host_build(const mpsfm_ba_problem* P, int32_t which, void* out, int64_t cap) {
  if (int rc = check_problem(P)) return rc;
  BuildOptions opt = BuildOptions::from_environment();
  TableBuild B;
  if (int rc = build_tables(P, opt, SumExchange(), false, 0, [](const char*) {}, nullptr, B)) return rc;
  const CameraLayout& cams = B.cams;
  const CholPlan& plan = B.plan;
  const HostTables& T = B.tables.t;
  const SPattern& S = B.spat;
  const SlabTables& slabs = B.slabs;

  const void* src = nullptr;
  int64_t bytes = 0;
  const int64_t nr = T.nrec, nf = T.nfixed;
  std::vector<int32_t> cam_of_slot, sweep_cost;
  int64_t info[10];
  const uint8_t on_device = 0;
  auto vec = [&](const auto& v) { src = v.data(); bytes = (int64_t)(sizeof(v[0]) * v.size()); };
  switch (which) {
    case 0: vec(T.chunks); break;
    case 1: vec(T.chunk_cams); break;
    case 2: src = T.rec_cam.data(); bytes = 4 * nr; break;
    case 3: src = T.rec_pt.data(); bytes = 4 * nr; break;
    case 4: src = T.rec_meta.data(); bytes = 4 * nr; break;
    case 5: src = T.rec_xy.data(); bytes = 16 * nr; break;
    case 6: src = T.rec_d.data(); bytes = 8 * nr; break;
    case 7: src = T.rec_m.data(); bytes = 8 * nr; break;
    case 8: src = T.rec_a.data(); bytes = 8 * nr; break;
    case 9: vec(T.pt_rec_start); break;
    case 10: vec(T.pt_kv); break;
    case 11: src = T.fx_cam.data(); bytes = 4 * nf; break;
    case 12: src = T.fx_pt.data(); bytes = 4 * nf; break;
    case 13: src = T.fx_meta.data(); bytes = 4 * nf; break;
    case 14: src = T.fx_xy.data(); bytes = 16 * nf; break;
    case 15: src = T.fx_d.data(); bytes = 8 * nf; break;
    case 16: src = T.fx_m.data(); bytes = 8 * nf; break;
    case 17: src = T.fx_a.data(); bytes = 8 * nf; break;
    case 18: vec(T.order); break;
    case 19: vec(slabs.dests); break;
    case 20: vec(slabs.srcs); break;
    case 21: vec(cams.slot); break;
    case 22: src = &on_device; bytes = 1; break;
    case 23: vec(T.blk_desc); break;
    case 24: vec(T.blk_ent_start); break;
    case 25: vec(T.ents); break;
    case 27: vec(T.lhdr); break;
    case 28: vec(S.sky_index); break;
    case 29: vec(S.sky_first); break;
    case 30: vec(S.sky_start); break;
    case 31: vec(cams.cmask); break;
    case 32: cam_of_slot = cam_of_slot_table(cams); vec(cam_of_slot); break;
    case 35: vec(slabs.sweep_order); break;
    case 36: for (int c = 0; c < slabs.n_dense; ++c) sweep_cost.push_back(dense_sweep_cost(T.chunks[(size_t)c].nrec, T.chunks[(size_t)c].npt, T.chunks[(size_t)c].ncam)); vec(sweep_cost); break;
    case 33: {
      DenseOverlap ov;
      LevelPlanDev lp;
      opt.apply_dense(cams.nt, plan, ov);
      level_plan_flags(plan, lp);
      double work = 0.0;
      dense_plan_numbers(cams.ncv, cams.nt, plan, ov, lp, &work, S.nblk, info);
      src = info; bytes = 80;
      break;
    }
    default: return fail(MPSFM_EINVAL, "unknown table");
  }
  if (!out || cap < bytes) return bytes;
  if (bytes > 0) std::memcpy(out, src, (size_t)bytes);
  return bytes;
}

int mpsfm_ba_sweep_parts(mpsfm_ba_handle* h, float ms[3], int64_t info[4]) {
  if (!h) return fail(MPSFM_EINVAL, "handle is NULL");
  MPSFM_TRY(hipSetDevice(h->device));
  if (ms)
    for (int k = 0; k < 3; ++k) MPSFM_TRY(hipEventElapsedTime(&ms[k], h->ev[k], h->ev[k + 1]));
  if (info) { info[0] = h->n_dense; info[1] = h->nchunks - h->n_dense; info[2] = h->nlong; info[3] = h->n_red_dests; }
  return 0;
}

// phase clocks of the last single-launch solve (local_lm.hip), 100 MHz ticks: sweep, barrier 1, dense + cameras, update, barrier 2,
// decision, iterations, then (debug flag 64 << 8) inside the dense phase: assemble, stacked factorisations, their barrier, trailing
// updates, back substitution (none of these while mpsfm_debug_local_skew is armed: slot 11 then sums the ticks the hook waited);
// returns 0 when the handle does not take that path
int mpsfm_debug_local_clocks(mpsfm_ba_handle* h, int64_t out[12]) {
  if (!h || !h->local_ok) return 0;
  if (hipSetDevice(h->device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) return 0;
  if (hipMemcpy(out, h->d_local_sync + 1, sizeof(int64_t) * 12, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  return 1;
}
// test hook of the single-launch solver: in every solve launched from now on, workgroup `chunk` (negative: counted from the last;
// reduced modulo the grid) waits `ticks` of the 100 MHz wall clock at each phase point of `phase_mask` (bits: P after barrier 0, A
// track sweep, B after barrier 1, D update sweep, E after barrier 2); clock slot 11 of mpsfm_debug_local_clocks sums the wait.
// (0, 0, 0): off.  At most 2 ms per point, far below the grid barrier's bounded spin.
int mpsfm_debug_local_skew(int32_t chunk, int32_t phase_mask, int64_t ticks) {
  if (ticks < 0 || ticks > kSkewMaxTicks) return fail(MPSFM_EINVAL, "skew ticks must lie in [0, 200000] (2 ms at 100 MHz)");
  if (phase_mask & ~kSkewAll) return fail(MPSFM_EINVAL, "skew phase mask: bits 0-4 (P, A, B, D, E)");
  g_local_skew = LocalSkew{chunk, phase_mask, ticks};
  return 0;
}
int mpsfm_ba_dense_solve_once(mpsfm_ba_handle* h, float* elapsed_ms) {
  if (!h) return fail(MPSFM_EINVAL, "handle is NULL");
  MPSFM_TRY(hipSetDevice(h->device));
  SolveForm f = solve_form(h);
  f.direct = false;  // the system is what the last sweep left in the reduced buffer: k_assemble runs, whatever form a solve would take
  MPSFM_TRY(hipEventRecord(h->ev[0], h->stream));
  if (int rc = run_dense(h, f, h->last_radius, nullptr)) return rc;
  MPSFM_TRY(hipEventRecord(h->ev[1], h->stream));
  MPSFM_TRY(hipMemsetAsync(h->d_fail, 0, sizeof(int), h->stream));  // no k_cam_update follows here to re-arm the flag
  MPSFM_TRY(hipStreamSynchronize(h->stream));
  MPSFM_TRY(hipGetLastError());
  float ms = 0.f;
  MPSFM_TRY(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
  if (elapsed_ms) *elapsed_ms = ms;
  return 0;
}

// Test hook (tests/test_gpu_level_entry.py): mpsfm_ba_dense_solve_once on a GIVEN system instead of the last sweep's.  S (n x n, both
// triangles) and rhs in the caller's camera order, n the reduced dimension; entries outside the handle's block pattern must be zero
// (they have no tile).  The solution is read with mpsfm_ba_get_dense_solution; *failed: the factorisation met a pivot that is not
// positive.  Needs one mpsfm_ba_sweep_once before it (the assemble launch runs first: it zeroes what the solve accumulates into).
int mpsfm_debug_dense_solve_given(mpsfm_ba_handle* h, const double* S, const double* rhs, int32_t n, int32_t* failed) {
  if (!h || !S || !rhs || !failed) return fail(MPSFM_EINVAL, "handle, S, rhs or failed is NULL");
  if (n != h->n_user || h->n <= 0) return fail(MPSFM_EINVAL, "n does not match the reduced dimension");
  MPSFM_TRY(hipSetDevice(h->device));
  run_assemble(h, h->last_radius);
  const int nt = h->nt, N = nt * 32;
  std::vector<int32_t> cam_of_slot((size_t)std::max(h->ncv, 1), -1);
  for (size_t i = 0; i < h->nat_slot.size(); ++i) cam_of_slot[(size_t)h->nat_slot[i]] = (int32_t)i;
  std::vector<int32_t> user((size_t)N, -1);  // column of the system -> row of S, -1: padding
  for (int C = 0; C < N; ++C) {
    const int v = vec_index(h->plan.slot_of_col.empty() ? nullptr : h->plan.slot_of_col.data(), C, h->n);
    if (v >= 0 && cam_of_slot[(size_t)(v / 6)] >= 0) user[(size_t)C] = 6 * cam_of_slot[(size_t)(v / 6)] + v % 6;
  }
  std::vector<double> A((size_t)(nt + 1) * (size_t)(nt + 2) / 2 * 1024, 0.0);
  for (int ti = 0; ti <= nt; ++ti)
    for (int tj = 0; tj <= ti && tj < nt; ++tj) {
      double* T = A.data() + (size_t)lt_tile(ti, tj) * 1024;
      for (int r = 0; r < 32; ++r)
        for (int c = 0; c < 32; ++c) {
          const int uc = user[(size_t)(tj * 32 + c)];
          if (ti == nt) { T[r * 32 + c] = (r == 0 && uc >= 0) ? rhs[uc] : 0.0; continue; }
          const int R = ti * 32 + r, C = tj * 32 + c, ur = user[(size_t)R];
          T[r * 32 + c] = (ur >= 0 && uc >= 0) ? S[(size_t)ur * n + uc] : (R == C ? 1.0 : 0.0);
        }
    }
  MPSFM_TRY(hipMemcpyAsync(h->d_A, A.data(), sizeof(double) * A.size(), hipMemcpyHostToDevice, h->stream));
  h->ov.entry_list = solve_form(h).entry_list;
  launch_dense_solve(h->d_A, h->d_dwork, h->nt, h->n, h->d_yc, h->d_fail, h->stream, &h->ov, &h->lp, nullptr);
  int flag = 0;
  MPSFM_TRY(hipMemcpyAsync(&flag, h->d_fail, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  MPSFM_TRY(hipMemsetAsync(h->d_fail, 0, sizeof(int), h->stream));  // no k_cam_update follows here to re-arm the flag
  MPSFM_TRY(hipStreamSynchronize(h->stream));
  MPSFM_TRY(hipGetLastError());
  *failed = flag ? 1 : 0;
  return 0;
}

// S and rhs of the last sweep (with the LM damping of its radius), plus the last dense solution
// S and the right-hand side in the CALLER's camera order (6 rows per variable camera), whatever slot order the handle uses.
int mpsfm_ba_get_reduced_system(mpsfm_ba_handle* h, double* S, double* rhs, int32_t n) {
  if (!h) return fail(MPSFM_EINVAL, "handle is NULL");
  if (n != h->n_user) return fail(MPSFM_EINVAL, "n does not match the reduced dimension");
  MPSFM_TRY(hipSetDevice(h->device));
  std::vector<double> red((size_t)h->red_count);
  MPSFM_TRY(hipMemcpyAsync(red.data(), h->d_red, sizeof(double) * red.size(), hipMemcpyDeviceToHost, h->stream));
  MPSFM_TRY(hipStreamSynchronize(h->stream));
  const double* Sb = red.data(); const double* gc = Sb + h->sblk_count; const double* wv = gc + h->n_user; const double* dU = wv + h->n_user;
  const mpsfm_ba_options& o = h->opt;
  const BlockSky sky{h->spat.sky_first.data(), h->spat.sky_start.data(), h->spat.sky_index.empty() ? nullptr : h->spat.sky_index.data(), h->ncv};
  for (int R = 0; R < n; ++R)
    for (int C = 0; C < n; ++C) {
      const int br = h->nat_slot[(size_t)(R / 6)], a = R % 6, bc = h->nat_slot[(size_t)(C / 6)], b = C % 6;
      double v;
      const int lo = std::min(br, bc), hi = std::max(br, bc);
      if (!sky_has(sky, lo, hi)) v = 0.0;
      else if (br < bc) v = Sb[sky_block(sky, br, bc) * 36 + a * 6 + b];
      else if (br > bc) v = Sb[sky_block(sky, bc, br) * 36 + b * 6 + a];
      else v = Sb[sky_block(sky, br, br) * 36 + (a <= b ? a * 6 + b : b * 6 + a)];
      if (R == C) v += std::min(std::max(dU[6 * br + a], o.min_lm_diagonal), o.max_lm_diagonal) / h->last_radius;
      if (S) S[(size_t)R * n + C] = v;
    }
  if (rhs) for (int i = 0; i < n; ++i) { const int q = 6 * h->nat_slot[(size_t)(i / 6)] + i % 6; rhs[i] = wv[q] - gc[q]; }
  return 0;
}

int mpsfm_ba_get_dense_solution(mpsfm_ba_handle* h, double* y, int32_t n) {
  if (!h || !y) return fail(MPSFM_EINVAL, "handle or y is NULL");
  if (n != h->n_user) return fail(MPSFM_EINVAL, "n does not match the reduced dimension");
  MPSFM_TRY(hipSetDevice(h->device));
  std::vector<double> ys((size_t)std::max(h->n_user, 1));
  MPSFM_TRY(hipMemcpyAsync(ys.data(), h->d_yc, sizeof(double) * (size_t)h->n_user, hipMemcpyDeviceToHost, h->stream));
  MPSFM_TRY(hipStreamSynchronize(h->stream));
  for (int i = 0; i < n; ++i) y[i] = ys[(size_t)(6 * h->nat_slot[(size_t)(i / 6)] + i % 6)];
  return 0;
}

}  // extern "C"
