// Thinning a dense matcher's output (mpsfm_radius_nms, mpsfm_thin_dense_matches, mpsfm_assign_keypoints; semantics:
// include/mpsfm_hip.h, the argument for exactness: DESIGN.md section 4l).  Both problems are fixed-radius neighbour search
// over 2-D points and stand on point_grid.h.
//
// Greedy suppression as rounds.  With "q above p" meaning q has higher priority and lies within the radius of p:
//   p becomes SUPPRESSED once some q above p is KEPT,
//   p becomes KEPT       once every q above p is SUPPRESSED.
// Both rules only read FINAL states of higher-priority points, and by induction over the priority order the final state of
// every point is the greedy's.  States move from undecided to final and never back, so reading a stale "undecided" can only
// postpone a decision: nothing here depends on one workgroup seeing another's stores inside a launch, the launch boundary
// is the only ordering relied on.  (The state words are read and written with relaxed agent-scope atomics, so a workgroup
// usually does see its neighbours' fresh decisions; that only saves rounds.)
//   k_nms_round   one workgroup per tile of kT consecutive points of the grid's Morton order (a compact patch of cells).
//                 The tile's states live in LDS and the workgroup repeats its pass until a pass changes nothing in the
//                 tile (at most kT + 1 passes: every productive pass decides a point of the tile), so chains inside a tile
//                 cost no launches; neighbours outside the tile are read from memory as they are.  No waiting on other
//                 workgroups anywhere.  Neighbours are streamed from memory run by run: a cell may hold any number of points.
//   host          enqueues rounds in groups of kGroup and reads the groups' undecided counts once per group; loops until a
//                 count is zero.  The globally highest undecided point is decided in every round, so the counts fall
//                 strictly; a group that does not lower the count is reported as an error instead of looping.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include <rocprim/device/device_scan.hpp>

#include "call_scope.h"
#include "common.h"
#include "point_grid.h"  // contraction off from here on

namespace mpsfm {

namespace {
constexpr int kT = kGridT;
constexpr int kGroup = 4;                 // round launches per read of the undecided count
constexpr int64_t kMaxPoints = 1 << 27;   // int32 positions, 18 run bounds per point
constexpr uint32_t kUndecided = 0, kKept = 1, kSuppressed = 2;

__device__ __forceinline__ uint32_t state_load(const uint32_t* s) { return __hip_atomic_load(s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void state_store(uint32_t* s, uint32_t v) { __hip_atomic_store(s, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// descending score, -0.0 as +0.0: the stable ascending sort of these keys leaves equal scores in index order
__global__ __launch_bounds__(kT) void k_score_keys(int32_t n, const double* __restrict__ scores, uint64_t* __restrict__ key, int32_t* __restrict__ val) {
  const int32_t i = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  if (i >= n) return;
  double s = scores[i];
  if (s == 0.0) s = 0.0;
  const uint64_t b = (uint64_t)__double_as_longlong(s);
  const uint64_t asc = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
  key[i] = ~asc;
  val[i] = i;
}
__global__ __launch_bounds__(kT) void k_rank_of_sorted(int32_t n, const int32_t* __restrict__ sorted, int32_t* __restrict__ rank) {
  const int32_t k = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  if (k < n) rank[sorted[k]] = k;
}
__global__ __launch_bounds__(kT) void k_rank_of_order(int32_t n, const int64_t* __restrict__ order, int32_t* __restrict__ rank) {
  const int32_t k = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  if (k < n) rank[order[k]] = k;
}

struct NmsArgs {
  PointGrid g;
  const int32_t* rank;  // [n] by position: 0 is the highest priority
  uint32_t* state;      // [n] by position
  int32_t* tile_left;   // [tiles] undecided points of the tile after its last launch
  double r2;
};

// alive == NULL: every point takes part; else alive[i] == 0 points start out suppressed (they neither keep nor suppress)
__global__ __launch_bounds__(kT) void k_nms_init(int32_t n, const int32_t* __restrict__ perm, const int32_t* __restrict__ rank,
                                                  const uint8_t* __restrict__ alive, int32_t* __restrict__ rank_s, uint32_t* __restrict__ state,
                                                  int32_t* __restrict__ tile_left) {
  const int32_t p = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  if (threadIdx.x == 0) tile_left[blockIdx.x] = 1;
  if (p >= n) return;
  const int32_t i = perm[p];
  rank_s[p] = rank[i];
  state[p] = (alive && !alive[i]) ? kSuppressed : kUndecided;
}

__global__ __launch_bounds__(kT) void k_nms_round(NmsArgs a, int32_t* __restrict__ undecided) {
  __shared__ uint32_t s_state[kT];
  if (a.tile_left[blockIdx.x] == 0) return;  // written by this tile's workgroup in an earlier launch
  const int32_t t0 = (int32_t)blockIdx.x * kT, p = t0 + (int32_t)threadIdx.x;
  const bool live = p < a.g.n;
  uint32_t mine = live ? state_load(a.state + p) : kSuppressed;
  s_state[threadIdx.x] = mine;
  double x = 0.0, y = 0.0;
  int32_t rk = 0;
  if (live) { const double2 v = a.g.xy[p]; x = v.x; y = v.y; rk = a.rank[p]; }
  __syncthreads();
  // every productive pass decides a point of the tile, so kT + 1 passes always suffice; the limit is what bounds the loop
  for (int pass = 0; pass <= kT; ++pass) {
    uint32_t next = mine;
    if (mine == kUndecided) {
      bool blocked = false, hit = false;
      grid_visit_point(a.g, p, [&](int32_t q) {
        if (a.rank[q] >= rk) return true;  // lower priority, or p itself
        const double2 w = a.g.xy[q];
        if (!(grid_d2(x, y, w.x, w.y) <= a.r2)) return true;
        const uint32_t sq = (q >= t0 && q < t0 + kT) ? s_state[q - t0] : state_load(a.state + q);
        if (sq == kKept) { hit = true; return false; }
        if (sq == kUndecided) blocked = true;
        return true;
      });
      next = hit ? kSuppressed : (blocked ? kUndecided : kKept);
    }
    const int changed = __syncthreads_or(next != mine);  // all reads of s_state of this pass are done
    if (next != mine) {
      mine = next;
      s_state[threadIdx.x] = next;
      state_store(a.state + p, next);
    }
    __syncthreads();
    if (!changed) break;
  }
  const int left = __syncthreads_count(mine == kUndecided);
  if (threadIdx.x == 0) {
    a.tile_left[blockIdx.x] = left;
    if (left) atomicAdd(undecided, left);
  }
}

__global__ __launch_bounds__(kT) void k_nms_out(int32_t n, const int32_t* __restrict__ perm, const uint32_t* __restrict__ state, uint8_t* __restrict__ keep) {
  const int32_t p = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  if (p < n) keep[perm[p]] = state[p] == kKept ? 1 : 0;
}

// ---- the two-pass leg: which survivors of a pass go on
__global__ __launch_bounds__(kT) void k_flags(int32_t n, const uint8_t* __restrict__ keep, int32_t* __restrict__ f) {
  const int32_t i = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  if (i <= n) f[i] = i < n ? keep[i] : 0;
}
// pos[i] = kept points before i = position of i in the sorted kept list.  The reference's slice [n_sparse:] of that list
// takes the kept points at positions >= n_sparse, whichever points they are; without it a dense point goes on when kept.
// alive_out [n] (sparse points always 1) and / or dense_out [n - ns]
__global__ __launch_bounds__(kT) void k_thin_select(int32_t n, int32_t ns, int32_t slice, const uint8_t* __restrict__ keep,
                                                     const int32_t* __restrict__ pos, uint8_t* __restrict__ alive_out, uint8_t* __restrict__ dense_out) {
  const int32_t i = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  if (i >= n) return;
  const uint8_t on = (i >= ns && keep[i] && (!slice || pos[i] >= ns)) ? 1 : 0;
  if (alive_out) alive_out[i] = i < ns ? 1 : on;
  if (dense_out && i >= ns) dense_out[i - ns] = on;
}

__global__ __launch_bounds__(kT) void k_assign(PointGrid g, int64_t nq, const double* __restrict__ query, double e2, int64_t* __restrict__ ids) {
  const int64_t i = (int64_t)blockIdx.x * kT + (int64_t)threadIdx.x;
  if (i >= nq) return;
  ids[i] = grid_nearest(g, query[2 * i], query[2 * i + 1], e2);
}

inline dim3 blocks_of(int64_t n) { return dim3((unsigned)((n + kT - 1) / kT)); }

template <class F>
int with_temp(CallScope& A, F&& f) {
  size_t bytes = 0;
  MPSFM_TRY(f(nullptr, bytes));
  void* tmp = A.get(std::max<size_t>(bytes, 16));
  if (!tmp) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  MPSFM_TRY(f(tmp, bytes));
  return 0;
}

// rank[i] of every point from the scores (device) or the caller's order (host, checked)
int make_rank(CallScope& A, int32_t n, const double* d_scores, const int64_t* h_order, int32_t** out) {
  int32_t* rank = A.alloc<int32_t>((size_t)n);
  if (!rank) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  *out = rank;
  if (h_order) {
    const int64_t* d_order = A.put(h_order, (size_t)n);
    if (!d_order) return fail(MPSFM_ENOMEM, "hipMalloc failed");
    hipLaunchKernelGGL(k_rank_of_order, blocks_of(n), dim3(kT), 0, A.st, n, d_order, rank);
    MPSFM_TRY(hipGetLastError());
    return 0;
  }
  uint64_t* k0 = A.alloc<uint64_t>((size_t)n);
  uint64_t* k1 = A.alloc<uint64_t>((size_t)n);
  int32_t* v0 = A.alloc<int32_t>((size_t)n);
  int32_t* v1 = A.alloc<int32_t>((size_t)n);
  if (!k0 || !k1 || !v0 || !v1) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  hipLaunchKernelGGL(k_score_keys, blocks_of(n), dim3(kT), 0, A.st, n, d_scores, k0, v0);
  MPSFM_TRY(hipGetLastError());
  if (int rc = with_temp(A, [&](void* t, size_t& b) { return rocprim::radix_sort_pairs(t, b, k0, k1, v0, v1, (size_t)n, 0, 64, A.st); })) return rc;
  hipLaunchKernelGGL(k_rank_of_sorted, blocks_of(n), dim3(kT), 0, A.st, n, v1, rank);
  MPSFM_TRY(hipGetLastError());
  return 0;
}

struct NmsRun { int32_t rounds = 0, launches = 0, cells = 0, max_cell = 0; };

// the suppression over d_pts[n][2] (device), n >= 1; d_keep[n] by the caller's index.  Synchronises the stream.
int nms_core(CallScope& A, int32_t n, const double* d_pts, const Box2& box, double radius, const int32_t* d_rank, const uint8_t* d_alive,
             uint8_t* d_keep, NmsRun& run) {
  NmsArgs a{};
  if (int rc = grid_build(A, n, d_pts, grid_spec(box, radius), true, a.g)) return rc;
  const dim3 grid = blocks_of(n);
  int32_t* rank_s = A.alloc<int32_t>((size_t)n);
  a.state = A.alloc<uint32_t>((size_t)n);
  a.tile_left = A.alloc<int32_t>((size_t)grid.x);
  int32_t* d_cnt = A.alloc<int32_t>(kGroup);
  if (!rank_s || !a.state || !a.tile_left || !d_cnt) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  a.rank = rank_s;
  a.r2 = radius * radius;
  hipLaunchKernelGGL(k_nms_init, grid, dim3(kT), 0, A.st, n, a.g.perm, d_rank, d_alive, rank_s, a.state, a.tile_left);
  MPSFM_TRY(hipGetLastError());
  int64_t before = (int64_t)n + 1;
  for (;;) {
    MPSFM_TRY(hipMemsetAsync(d_cnt, 0, sizeof(int32_t) * kGroup, A.st));
    for (int g = 0; g < kGroup; ++g) hipLaunchKernelGGL(k_nms_round, grid, dim3(kT), 0, A.st, a, d_cnt + g);
    MPSFM_TRY(hipGetLastError());
    run.launches += kGroup;
    int32_t h_cnt[kGroup];
    MPSFM_TRY(A.down(h_cnt, d_cnt, sizeof(int32_t) * kGroup));
    int done = -1;
    for (int g = 0; g < kGroup && done < 0; ++g)
      if (h_cnt[g] == 0) done = g;
    if (done >= 0) { run.rounds += done + 1; break; }
    run.rounds += kGroup;
    if (h_cnt[kGroup - 1] >= before) return fail(MPSFM_EHIP, "radius NMS: a group of rounds decided no point (internal error)");
    before = h_cnt[kGroup - 1];
  }
  hipLaunchKernelGGL(k_nms_out, grid, dim3(kT), 0, A.st, n, a.g.perm, a.state, d_keep);
  MPSFM_TRY(hipGetLastError());
  int32_t stats[2];
  MPSFM_TRY(A.down(stats, a.g.stats, sizeof(stats)));
  run.cells = std::max(run.cells, stats[0]);
  run.max_cell = std::max(run.max_cell, stats[1]);
  return 0;
}

void fill_info(mpsfm_nms_info* info, const NmsRun& run, double ms) {
  if (!info) return;
  info->rounds = run.rounds; info->launches = run.launches; info->cells = run.cells; info->max_cell_points = run.max_cell;
  info->ms = (float)ms;
}

bool box_ok(const Box2& b) { return std::isfinite(b.hi[0] - b.lo[0]) && std::isfinite(b.hi[1] - b.lo[1]); }
int64_t count_ones(const uint8_t* k, size_t n) {
  int64_t c = 0;
  for (size_t i = 0; i < n; ++i) c += k[i] != 0;
  return c;
}
}  // namespace

}  // namespace mpsfm

using namespace mpsfm;

extern "C" int mpsfm_radius_nms(int64_t n64, const double* points, const double* scores, const int64_t* order, double radius, int32_t device,
                                uint8_t* keep, int64_t* num_kept, mpsfm_nms_info* info) {
  if (info) *info = mpsfm_nms_info{};
  if (num_kept) *num_kept = 0;
  if (n64 < 0) return fail(MPSFM_EINVAL, "negative size");
  if (n64 > kMaxPoints) return fail(MPSFM_EINVAL, "more than 2^27 points");
  if (!num_kept) return fail(MPSFM_EINVAL, "NULL pointer");
  if (n64 > 0 && (!points || !keep || (!scores && !order))) return fail(MPSFM_EINVAL, "NULL pointer");
  if (!std::isfinite(radius) || radius < 0.0) return fail(MPSFM_EINVAL, "radius must be finite and non-negative");
  const int32_t n = (int32_t)n64;
  Box2 box;
  if (!grid_box(points, (size_t)n, box)) return fail(MPSFM_EINVAL, "non-finite point");
  if (!box_ok(box)) return fail(MPSFM_EINVAL, "bounding box wider than DBL_MAX");
  if (scores && !all_finite(scores, (size_t)n)) return fail(MPSFM_EINVAL, "non-finite score");
  if (order) {
    std::vector<uint8_t> seen((size_t)n, 0);
    for (int32_t k = 0; k < n; ++k) {
      if (order[k] < 0 || order[k] >= n || seen[(size_t)order[k]]) return fail(MPSFM_EINVAL, "order is not a permutation of 0 .. n-1");
      seen[(size_t)order[k]] = 1;
    }
  }
  if (n == 0) return 0;
  if (int rc = open_device(device)) return rc;
  CallScope A;
  if (int rc = A.open(true)) return rc;
  const double* d_pts = A.put(points, 2 * (size_t)n);
  const double* d_scores = order ? nullptr : A.put(scores, (size_t)n);
  uint8_t* d_keep = A.alloc<uint8_t>((size_t)n);
  if (!d_pts || (!order && !d_scores) || !d_keep) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  if (int rc = A.begin()) return rc;
  int32_t* d_rank = nullptr;
  if (int rc = make_rank(A, n, d_scores, order, &d_rank)) return rc;
  NmsRun run;
  if (int rc = nms_core(A, n, d_pts, box, radius, d_rank, nullptr, d_keep, run)) return rc;
  if (int rc = A.end()) return rc;
  MPSFM_TRY(A.down(keep, d_keep, (size_t)n));
  *num_kept = count_ones(keep, (size_t)n);
  fill_info(info, run, A.ms);
  return 0;
}

extern "C" int mpsfm_thin_dense_matches(int64_t ns64, const double* sparse0, const double* sparse1, int64_t nd64, const double* dense0,
                                        const double* dense1, const double* dscores, double radius, int32_t reference_slice, int32_t device,
                                        uint8_t* keep, int64_t* num_kept, mpsfm_nms_info* info) {
  if (info) *info = mpsfm_nms_info{};
  if (num_kept) *num_kept = 0;
  if (ns64 < 0 || nd64 < 0) return fail(MPSFM_EINVAL, "negative size");
  if (ns64 + nd64 > kMaxPoints || ns64 > kMaxPoints || nd64 > kMaxPoints) return fail(MPSFM_EINVAL, "more than 2^27 points");
  if (!num_kept) return fail(MPSFM_EINVAL, "NULL pointer");
  if (ns64 > 0 && (!sparse0 || !sparse1)) return fail(MPSFM_EINVAL, "NULL pointer");
  if (nd64 > 0 && (!dense0 || !dense1 || !dscores || !keep)) return fail(MPSFM_EINVAL, "NULL pointer");
  if (!std::isfinite(radius) || radius < 0.0) return fail(MPSFM_EINVAL, "radius must be finite and non-negative");
  const int32_t ns = (int32_t)ns64, nd = (int32_t)nd64, n = ns + nd;
  // [sparse; dense] of both images and the scores [100 ...; dscores], as the reference concatenates them
  std::vector<double> h0(2 * (size_t)n), h1(2 * (size_t)n), hs((size_t)n);
  if (ns) { std::memcpy(h0.data(), sparse0, sizeof(double) * 2 * (size_t)ns); std::memcpy(h1.data(), sparse1, sizeof(double) * 2 * (size_t)ns); }
  if (nd) {
    std::memcpy(h0.data() + 2 * (size_t)ns, dense0, sizeof(double) * 2 * (size_t)nd);
    std::memcpy(h1.data() + 2 * (size_t)ns, dense1, sizeof(double) * 2 * (size_t)nd);
    std::memcpy(hs.data() + ns, dscores, sizeof(double) * (size_t)nd);
  }
  std::fill(hs.begin(), hs.begin() + ns, 100.0);
  Box2 box0, box1;
  if (!grid_box(h0.data(), (size_t)n, box0) || !grid_box(h1.data(), (size_t)n, box1)) return fail(MPSFM_EINVAL, "non-finite point");
  if (!box_ok(box0) || !box_ok(box1)) return fail(MPSFM_EINVAL, "bounding box wider than DBL_MAX");
  if (!all_finite(hs.data(), (size_t)n)) return fail(MPSFM_EINVAL, "non-finite score");
  if (nd == 0) return 0;
  if (int rc = open_device(device)) return rc;
  CallScope A;
  if (int rc = A.open(true)) return rc;
  const double* d0 = A.put(h0.data(), 2 * (size_t)n);
  const double* d1 = A.put(h1.data(), 2 * (size_t)n);
  const double* d_scores = A.put(hs.data(), (size_t)n);
  uint8_t* d_keep = A.alloc<uint8_t>((size_t)n);
  uint8_t* d_alive = A.alloc<uint8_t>((size_t)n);
  uint8_t* d_out = A.alloc<uint8_t>((size_t)nd);
  int32_t* d_flag = A.alloc<int32_t>((size_t)n + 1);
  int32_t* d_pos = A.alloc<int32_t>((size_t)n + 1);
  if (!d0 || !d1 || !d_scores || !d_keep || !d_alive || !d_out || !d_flag || !d_pos) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  if (int rc = A.begin()) return rc;
  int32_t* d_rank = nullptr;  // the priorities depend on scores and indices only: one ranking serves both passes
  if (int rc = make_rank(A, n, d_scores, nullptr, &d_rank)) return rc;
  NmsRun run;
  const int32_t slice = reference_slice ? 1 : 0;
  // Pass 2 runs over ALL of [sparse1; dense1] with the matches pass 1 dropped starting out suppressed: they keep nothing and
  // suppress nothing, and the survivors keep their relative index order, so this is the suppression over the compacted
  // arrays without sizing anything from a count the host would have to wait for.
  for (int pass = 0; pass < 2; ++pass) {
    if (int rc = nms_core(A, n, pass ? d1 : d0, pass ? box1 : box0, radius, d_rank, pass ? d_alive : nullptr, d_keep, run)) return rc;
    hipLaunchKernelGGL(k_flags, blocks_of((int64_t)n + 1), dim3(kT), 0, A.st, n, d_keep, d_flag);
    MPSFM_TRY(hipGetLastError());
    if (int rc = with_temp(A, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, d_flag, d_pos, 0, (size_t)n + 1, rocprim::plus<int32_t>(), A.st); })) return rc;
    hipLaunchKernelGGL(k_thin_select, blocks_of(n), dim3(kT), 0, A.st, n, ns, slice, d_keep, d_pos, pass ? nullptr : d_alive, pass ? d_out : nullptr);
    MPSFM_TRY(hipGetLastError());
  }
  if (int rc = A.end()) return rc;
  MPSFM_TRY(A.down(keep, d_out, (size_t)nd));
  *num_kept = count_ones(keep, (size_t)nd);
  fill_info(info, run, A.ms);
  return 0;
}

extern "C" int mpsfm_assign_keypoints(int64_t nq, const double* query, int64_t nk64, const double* kps, double max_error, int32_t device,
                                      int64_t* ids, float* ms) {
  if (ms) *ms = 0.f;
  if (nq < 0 || nk64 < 0) return fail(MPSFM_EINVAL, "negative size");
  if (nk64 > kMaxPoints) return fail(MPSFM_EINVAL, "more than 2^27 keypoints");
  if (nq > INT32_MAX) return fail(MPSFM_EINVAL, "more than INT32_MAX queries");
  if (nq > 0 && (!query || !ids)) return fail(MPSFM_EINVAL, "NULL pointer");
  if (nk64 > 0 && !kps) return fail(MPSFM_EINVAL, "NULL pointer");
  if (!std::isfinite(max_error) || max_error < 0.0) return fail(MPSFM_EINVAL, "max_error must be finite and non-negative");
  const int32_t nk = (int32_t)nk64;
  Box2 box;
  if (!all_finite(query, 2 * (size_t)nq) || !grid_box(kps, (size_t)nk, box)) return fail(MPSFM_EINVAL, "non-finite point");
  if (!box_ok(box)) return fail(MPSFM_EINVAL, "bounding box wider than DBL_MAX");
  if (nq == 0) return 0;
  if (nk == 0) {
    std::fill(ids, ids + nq, (int64_t)-1);
    return 0;
  }
  if (int rc = open_device(device)) return rc;
  CallScope A;
  if (int rc = A.open(true)) return rc;
  const double* d_kps = A.put(kps, 2 * (size_t)nk);
  const double* d_query = A.put(query, 2 * (size_t)nq);
  int64_t* d_ids = A.alloc<int64_t>((size_t)nq);
  if (!d_kps || !d_query || !d_ids) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  if (int rc = A.begin()) return rc;
  PointGrid g{};
  if (int rc = grid_build(A, nk, d_kps, grid_spec(box, max_error), false, g)) return rc;
  hipLaunchKernelGGL(k_assign, blocks_of(nq), dim3(kT), 0, A.st, g, nq, d_query, max_error * max_error, d_ids);
  MPSFM_TRY(hipGetLastError());
  if (int rc = A.end()) return rc;
  MPSFM_TRY(A.down(ids, d_ids, sizeof(int64_t) * (size_t)nq));
  if (ms) *ms = (float)A.ms;
  return 0;
}
