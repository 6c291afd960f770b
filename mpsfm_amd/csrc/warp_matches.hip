// A dense matcher's warp to match lists (mpsfm_simple_nms, mpsfm_kpids_to_matches0, mpsfm_warp_matches; semantics:
// include/mpsfm_hip.h, the contract, the tie rule and the measurements: DESIGN.md section 4n).
//
//   k_pool<S>        one max-pool stage of simple_nms.  A workgroup owns kTH x kTW outputs.  Row pass: every wave stages one
//                    row of kTW + 2r inputs in LDS and each lane takes the maximum of its 2r + 1 window; the row maxima of
//                    the kTH + 2r rows around the tile stay in LDS.  Column pass: each lane walks its column of row maxima.
//                    2 (2r + 1) compares per output instead of (2r + 1)^2, and the stage's epilogue (mask, suppression flag,
//                    output) is applied to the pooled value in registers.  Five stages, one launch each; the map stays in L2.
//   k_group_max      unique matches: per valid row one 64-bit atomicMax of (order-preserving score bits, ~row) on the row's
//                    ids0 word and one on its ids1 word.  The maximum of a set does not depend on arrival order.
//   k_group_write    a row that holds both of its words is kept: it alone writes matches0 / scores0 of its ids0.
//   k_warp_ids       pixel coordinates and both keypoint lookups (point_grid.h) of one warp row per thread.
//   k_dense_flags / k_dense_compact   selection of the dense leg, compacted in row order through an exclusive scan.
//   k_scan_inputs    device inputs: non-finite values, ids outside -1 .. n - 1.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include <rocprim/device/device_scan.hpp>

#include "call_scope.h"
#include "common.h"
#include "point_grid.h"  // contraction off from here on

// every decision here is exact: no fused multiply-add in the pixel coordinates either
#pragma clang fp contract(off)

namespace mpsfm {

namespace {
constexpr int kPT = 256;                 // threads of every kernel here
constexpr int kWaves = kPT / 64;
constexpr int kTW = 64, kTH = 32;        // outputs of a k_pool workgroup: one lane per column
constexpr int kMaxR = 64;
constexpr int64_t kMaxRows = 1 << 27;    // int32 rows, the low key word holds ~row

enum { kStageMax = 0, kStageSupp = 1, kStageAdd = 2, kStageLast = 3 };

struct PoolArgs {
  int32_t H, W, r, tiles_x;
  const float* s;   // the scores
  uint8_t* mask;    // max_mask
  uint8_t* supp;    // supp_mask of the current round
  float* out;
};

// what stage S pools: the scores, the mask as 0 / 1, or the scores with the suppressed pixels at 0; -inf outside the map
template <int S>
__device__ __forceinline__ float pool_in(const PoolArgs& a, int y, int x) {
  if (y < 0 || y >= a.H || x < 0 || x >= a.W) return -INFINITY;
  const size_t i = (size_t)y * (size_t)a.W + (size_t)x;
  if (S == kStageMax) return a.s[i];
  if (S == kStageSupp) return a.mask[i] ? 1.f : 0.f;
  return a.supp[i] ? 0.f : a.s[i];
}

template <int S>
__global__ __launch_bounds__(kPT) void k_pool(PoolArgs a) {
  __shared__ float s_row[kWaves][kTW + 2 * kMaxR];
  __shared__ float s_max[(kTH + 2 * kMaxR) * kTW];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  // tiles in row-major order on gridDim.x (which reaches 2^31 - 1: a map of 2^27 x 1 has 2^22 tiles in y, beyond gridDim.y)
  const int x0 = (int)(blockIdx.x % (unsigned)a.tiles_x) * kTW, y0 = (int)(blockIdx.x / (unsigned)a.tiles_x) * kTH, r = a.r;
  const int th = min(kTH, a.H - y0);  // >= 1: the grid covers the map exactly
  const int rows = th + 2 * r, span = kTW + 2 * r;
  for (int j0 = 0; j0 < rows; j0 += kWaves) {  // the trip count is the workgroup's: every wave reaches every barrier
    const int j = j0 + wave;
    if (j < rows)
      for (int c = lane; c < span; c += 64) s_row[wave][c] = pool_in<S>(a, y0 - r + j, x0 - r + c);
    __syncthreads();
    if (j < rows) {
      float m = s_row[wave][lane];
      for (int d = 1; d <= 2 * r; ++d) m = fmaxf(m, s_row[wave][lane + d]);
      s_max[j * kTW + lane] = m;
    }
    __syncthreads();
  }
  const int x = x0 + lane;
  for (int t = wave; t < th; t += kWaves) {
    float p = s_max[t * kTW + lane];
    for (int d = 1; d <= 2 * r; ++d) p = fmaxf(p, s_max[(t + d) * kTW + lane]);
    if (x >= a.W) continue;
    const size_t i = (size_t)(y0 + t) * (size_t)a.W + (size_t)x;
    if (S == kStageMax) {
      a.mask[i] = a.s[i] == p ? 1 : 0;
    } else if (S == kStageSupp) {
      a.supp[i] = p > 0.f ? 1 : 0;
    } else {
      const bool sp = a.supp[i] != 0;
      const float sv = a.s[i];
      const float ss = sp ? 0.f : sv;
      const bool m = a.mask[i] != 0 || (ss == p && !sp);
      if (S == kStageAdd) a.mask[i] = m ? 1 : 0;
      else a.out[i] = m ? sv : 0.f;
    }
  }
}

// (score, row) as one word: a higher score is a larger word, among equal scores (-0.0 as +0.0) the lower row is
__device__ __forceinline__ unsigned long long row_key(float s, int32_t row) {
  if (s == 0.f) s = 0.f;
  const uint32_t b = __float_as_uint(s);
  const uint32_t asc = (b >> 31) ? ~b : (b | 0x80000000u);
  return ((unsigned long long)asc << 32) | (unsigned long long)(~(uint32_t)row);
}

struct GroupArgs {
  int32_t n, n0, n1;
  const float* scores;
  unsigned long long* best0;  // [n0], zeroed: every key of a row is above 0
  unsigned long long* best1;  // [n1]
  int32_t* matches0;          // [n0], -1
  float* scores0;             // [n0], 0
  int32_t* counts;            // [3] zeroed: n_kps0, valid rows, kept rows
};

// rows that are not valid, and rows a device scan has reported, take no part
template <typename Id>
__device__ __forceinline__ bool row_ids(const GroupArgs& a, const Id* __restrict__ ids0, const Id* __restrict__ ids1, int32_t i, int32_t& u, int32_t& v) {
  const Id p = ids0[i], q = ids1[i];
  if (p < 0 || q < 0 || p >= (Id)a.n0 || q >= (Id)a.n1) return false;
  u = (int32_t)p; v = (int32_t)q;
  return true;
}

template <typename Id>
__global__ __launch_bounds__(kPT) void k_group_max(GroupArgs a, const Id* __restrict__ ids0, const Id* __restrict__ ids1) {
  const int32_t i = (int32_t)blockIdx.x * kPT + (int32_t)threadIdx.x;
  int32_t u = 0, v = 0;
  const bool valid = i < a.n && row_ids(a, ids0, ids1, i, u, v);
  if (valid) {
    const unsigned long long key = row_key(a.scores[i], i);
    atomicMax(a.best0 + u, key);
    atomicMax(a.best1 + v, key);
  }
  const int cnt = __syncthreads_count(valid);  // one add per workgroup on the counter word
  if (threadIdx.x == 0 && cnt) atomicAdd(a.counts + 1, cnt);
}

template <typename Id>
__global__ __launch_bounds__(kPT) void k_group_write(GroupArgs a, const Id* __restrict__ ids0, const Id* __restrict__ ids1) {
  __shared__ int32_t s_top;  // 1 + the largest ids0 kept in this workgroup
  const int32_t i = (int32_t)blockIdx.x * kPT + (int32_t)threadIdx.x;
  if (threadIdx.x == 0) s_top = 0;
  __syncthreads();
  int32_t u = 0, v = 0;
  bool kept = i < a.n && row_ids(a, ids0, ids1, i, u, v);
  if (kept) {
    const float s = a.scores[i];
    const unsigned long long key = row_key(s, i);
    kept = a.best0[u] == key && a.best1[v] == key;
    if (kept) {
      a.matches0[u] = v;  // the one row that holds the word of group u
      a.scores0[u] = s;
      atomicMax(&s_top, u + 1);
    }
  }
  const int cnt = __syncthreads_count(kept);  // also orders the LDS maxima before the read below
  if (threadIdx.x == 0 && cnt) {
    atomicMax(a.counts, s_top);
    atomicAdd(a.counts + 2, cnt);
  }
}

struct WarpArgs {
  int32_t n;
  const float* warp;  // [n][4]
  float hwA, hhA, hwB, hhB;  // fl32(W / 2), fl32(H / 2) of the two images
  double sx0, sy0, sx1, sy1, e2;
};

__device__ __forceinline__ float to_pixel(float half, float v) {
  const float t = v + 1.f;
  return half * t;
}

__global__ __launch_bounds__(kPT) void k_warp_ids(WarpArgs a, PointGrid g0, PointGrid g1, int32_t* __restrict__ ids0, int32_t* __restrict__ ids1) {
  const int32_t i = (int32_t)blockIdx.x * kPT + (int32_t)threadIdx.x;
  if (i >= a.n) return;
  const float* w = a.warp + 4 * (size_t)i;
  const double xa = (double)to_pixel(a.hwA, w[0]) * a.sx0, ya = (double)to_pixel(a.hhA, w[1]) * a.sy0;
  const int32_t u = grid_nearest(g0, xa, ya, a.e2);
  int32_t v = -1;
  if (u >= 0) {  // a row without id0 is not valid whatever its id1
    const double xb = (double)to_pixel(a.hwB, w[2]) * a.sx1, yb = (double)to_pixel(a.hhB, w[3]) * a.sy1;
    v = grid_nearest(g1, xb, yb, a.e2);
  }
  ids0[i] = u;
  ids1[i] = v;
}

// f[i] for i <= n: the exclusive scan's last entry is the count
__global__ __launch_bounds__(kPT) void k_dense_flags(int32_t n, const float* __restrict__ nms, float thr, int32_t* __restrict__ f) {
  const int32_t i = (int32_t)blockIdx.x * kPT + (int32_t)threadIdx.x;
  if (i <= n) f[i] = (i < n && nms[i] > thr) ? 1 : 0;
}

__global__ __launch_bounds__(kPT) void k_dense_compact(WarpArgs a, const float* __restrict__ nms, const int32_t* __restrict__ f, const int32_t* __restrict__ pos,
                                                       float* __restrict__ k0, float* __restrict__ k1, float* __restrict__ sc) {
  const int32_t i = (int32_t)blockIdx.x * kPT + (int32_t)threadIdx.x;
  if (i >= a.n || !f[i]) return;
  const float* w = a.warp + 4 * (size_t)i;
  const size_t p = (size_t)pos[i];
  k0[2 * p] = to_pixel(a.hwA, w[0]);
  k0[2 * p + 1] = to_pixel(a.hhA, w[1]);
  k1[2 * p] = to_pixel(a.hwB, w[2]);
  k1[2 * p + 1] = to_pixel(a.hhB, w[3]);
  sc[p] = nms[i];
}

// x [nx] finite; ids [ni] (may be NULL) within -1 .. hi - 1
__global__ __launch_bounds__(kPT) void k_scan_inputs(const float* __restrict__ x, int64_t nx, const int64_t* __restrict__ ids, int64_t ni, int64_t hi,
                                                     int32_t* __restrict__ bad) {
  const int64_t first = (int64_t)blockIdx.x * kPT + (int64_t)threadIdx.x, stride = (int64_t)gridDim.x * kPT;
  bool b = false;
  for (int64_t i = first; i < nx; i += stride) b = b || !isfinite(x[i]);
  if (ids)
    for (int64_t i = first; i < ni; i += stride) b = b || ids[i] < -1 || ids[i] >= hi;
  if (b) atomicOr(bad, 1);
}

inline dim3 blocks_of(int64_t n) { return dim3((unsigned)((n + kPT - 1) / kPT)); }

int scan_device(CallScope& A, const float* x, int64_t nx, const int64_t* ids, int64_t ni, int64_t hi, int32_t* d_bad) {
  const int64_t blocks = std::min<int64_t>((std::max(nx, ni) + kPT - 1) / kPT, 4096);
  hipLaunchKernelGGL(k_scan_inputs, dim3((unsigned)std::max<int64_t>(blocks, 1)), dim3(kPT), 0, A.st, x, nx, ids, ni, hi, d_bad);
  MPSFM_TRY(hipGetLastError());
  return 0;
}

bool box_ok(const Box2& b) { return std::isfinite(b.hi[0] - b.lo[0]) && std::isfinite(b.hi[1] - b.lo[1]); }

// the five pool stages of simple_nms over d_s [H][W] into d_out (both on the device, distinct)
int nms_core(CallScope& A, int32_t H, int32_t W, int32_t r, const float* d_s, float* d_out) {
  const size_t px = (size_t)H * (size_t)W;
  const int32_t tiles_x = (W + kTW - 1) / kTW, tiles_y = (H + kTH - 1) / kTH;  // H W <= 2^27: at most 2^27 tiles
  PoolArgs a{H, W, r, tiles_x, d_s, A.alloc<uint8_t>(px), A.alloc<uint8_t>(px), d_out};
  if (!a.mask || !a.supp) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  const dim3 grid((unsigned)((int64_t)tiles_x * tiles_y));
  hipLaunchKernelGGL(k_pool<kStageMax>, grid, dim3(kPT), 0, A.st, a);
  for (int round = 0; round < 2; ++round) {
    hipLaunchKernelGGL(k_pool<kStageSupp>, grid, dim3(kPT), 0, A.st, a);
    if (round == 0) hipLaunchKernelGGL(k_pool<kStageAdd>, grid, dim3(kPT), 0, A.st, a);
    else hipLaunchKernelGGL(k_pool<kStageLast>, grid, dim3(kPT), 0, A.st, a);
  }
  MPSFM_TRY(hipGetLastError());
  return 0;
}

// the unique-match rule over device rows; d_m [n0], d_s0 [n0] and d_counts [3] are the scope's
template <typename Id>
int unique_core(CallScope& A, int32_t n, const Id* d_ids0, const Id* d_ids1, const float* d_scores, int32_t n0, int32_t n1, int32_t** d_m, float** d_s0,
                int32_t** d_counts) {
  GroupArgs a{n, n0, n1, d_scores, A.alloc<unsigned long long>((size_t)n0), A.alloc<unsigned long long>((size_t)n1), A.alloc<int32_t>((size_t)n0),
              A.alloc<float>((size_t)n0), A.alloc<int32_t>(3)};
  if (!a.best0 || !a.best1 || !a.matches0 || !a.scores0 || !a.counts) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  MPSFM_TRY(hipMemsetAsync(a.best0, 0, sizeof(unsigned long long) * (size_t)n0, A.st));
  MPSFM_TRY(hipMemsetAsync(a.best1, 0, sizeof(unsigned long long) * (size_t)n1, A.st));
  MPSFM_TRY(hipMemsetAsync(a.matches0, 0xFF, sizeof(int32_t) * (size_t)n0, A.st));
  MPSFM_TRY(hipMemsetAsync(a.scores0, 0, sizeof(float) * (size_t)n0, A.st));
  MPSFM_TRY(hipMemsetAsync(a.counts, 0, sizeof(int32_t) * 3, A.st));
  hipLaunchKernelGGL(k_group_max<Id>, blocks_of(n), dim3(kPT), 0, A.st, a, d_ids0, d_ids1);
  hipLaunchKernelGGL(k_group_write<Id>, blocks_of(n), dim3(kPT), 0, A.st, a, d_ids0, d_ids1);
  MPSFM_TRY(hipGetLastError());
  *d_m = a.matches0; *d_s0 = a.scores0; *d_counts = a.counts;
  return 0;
}

void fill_empty(int64_t n0, int32_t* matches0, float* scores0) {
  for (int64_t i = 0; i < n0; ++i) { matches0[i] = -1; scores0[i] = 0.f; }
}

int read_bad(CallScope& A, const int32_t* d_bad) {
  if (!d_bad) return 0;
  int32_t bad = 0;
  MPSFM_TRY(A.down(&bad, d_bad, sizeof(bad)));
  if (bad) return fail(MPSFM_EINVAL, "non-finite value or id out of range in a device input");
  return 0;
}

int new_bad_flag(CallScope& A, int32_t** d_bad) {
  *d_bad = A.alloc<int32_t>(1);
  if (!*d_bad) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  MPSFM_TRY(hipMemsetAsync(*d_bad, 0, sizeof(int32_t), A.st));
  return 0;
}
}  // namespace

}  // namespace mpsfm

using namespace mpsfm;

extern "C" void mpsfm_warp_default_options(mpsfm_warp_options* opts) {
  if (!opts) return;
  *opts = mpsfm_warp_options{};
  opts->sample_thresh = 0.1;
  opts->max_error = 2.0;
  opts->scale0[0] = opts->scale0[1] = opts->scale1[0] = opts->scale1[1] = 1.0;
  opts->nms_radius = 8;
}

extern "C" int mpsfm_simple_nms(int32_t H, int32_t W, const float* scores, int32_t radius, int32_t inputs_on_device, void* stream, int32_t device,
                                float* out, mpsfm_warp_info* info) {
  if (info) *info = mpsfm_warp_info{};
  if (H < 1 || W < 1) return fail(MPSFM_EINVAL, "a map needs at least one row and one column");
  if ((int64_t)H * (int64_t)W > kMaxRows) return fail(MPSFM_EINVAL, "more than 2^27 pixels");
  if (radius < 0 || radius > kMaxR) return fail(MPSFM_EINVAL, "radius must be 0 .. 64");
  if (!scores || !out) return fail(MPSFM_EINVAL, "NULL pointer");
  const size_t px = (size_t)H * (size_t)W;
  if (!inputs_on_device && !all_finite(scores, px)) return fail(MPSFM_EINVAL, "non-finite map value");
  // the last stage reads scores around a tile while other workgroups write out: on the device the two must be distinct ranges
  if (inputs_on_device && (uintptr_t)scores < (uintptr_t)out + sizeof(float) * px && (uintptr_t)out < (uintptr_t)scores + sizeof(float) * px)
    return fail(MPSFM_EINVAL, "scores and out overlap");
  if (int rc = open_device(device)) return rc;
  CallScope A;
  if (int rc = A.open(true)) return rc;
  const float* d_s = scores;
  float* d_out = out;
  int32_t* d_bad = nullptr;
  if (inputs_on_device) {
    if (int rc = check_device_pointer(scores, device, "scores")) return rc;
    if (int rc = check_device_pointer(out, device, "out")) return rc;
    if (int rc = wait_for_caller(A, stream)) return rc;
    if (int rc = new_bad_flag(A, &d_bad)) return rc;
  } else {
    d_s = A.put(scores, px);
    d_out = A.alloc<float>(px);
    if (!d_s || !d_out) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  }
  if (int rc = A.begin()) return rc;
  if (d_bad)
    if (int rc = scan_device(A, d_s, (int64_t)px, nullptr, 0, 0, d_bad)) return rc;
  if (int rc = nms_core(A, H, W, radius, d_s, d_out)) return rc;
  if (int rc = A.end()) return rc;
  if (int rc = read_bad(A, d_bad)) return rc;
  if (!inputs_on_device) MPSFM_TRY(A.down(out, d_out, sizeof(float) * px));
  if (info) info->ms = (float)A.ms;
  return 0;
}

extern "C" int mpsfm_kpids_to_matches0(int64_t n, const int64_t* ids0, const int64_t* ids1, const float* scores, int64_t n0, int64_t n1,
                                       int32_t inputs_on_device, void* stream, int32_t device, int32_t* matches0, float* scores0, int64_t* n_kps0,
                                       mpsfm_warp_info* info) {
  if (info) *info = mpsfm_warp_info{};
  if (n_kps0) *n_kps0 = 0;
  if (n < 0 || n0 < 0 || n1 < 0) return fail(MPSFM_EINVAL, "negative size");
  if (n > kMaxRows || n0 > kMaxRows || n1 > kMaxRows) return fail(MPSFM_EINVAL, "more than 2^27 rows or keypoints");
  if (!n_kps0) return fail(MPSFM_EINVAL, "NULL pointer");
  if (n > 0 && (!ids0 || !ids1 || !scores)) return fail(MPSFM_EINVAL, "NULL pointer");
  if (n0 > 0 && (!matches0 || !scores0)) return fail(MPSFM_EINVAL, "NULL pointer");
  int64_t valid = inputs_on_device ? n : 0;
  if (!inputs_on_device) {
    for (int64_t i = 0; i < n; ++i) {
      if (ids0[i] < -1 || ids0[i] >= n0 || ids1[i] < -1 || ids1[i] >= n1) return fail(MPSFM_EINVAL, "keypoint id out of range");
      valid += ids0[i] >= 0 && ids1[i] >= 0;
    }
    if (!all_finite(scores, (size_t)n)) return fail(MPSFM_EINVAL, "non-finite score");
  }
  fill_empty(n0, matches0, scores0);
  if (valid == 0 || n0 == 0 || n1 == 0) return 0;  // host rows none of which is valid need no device either
  if (int rc = open_device(device)) return rc;
  CallScope A;
  if (int rc = A.open(true)) return rc;
  const int64_t *d_i0 = ids0, *d_i1 = ids1;
  const float* d_sc = scores;
  int32_t* d_bad = nullptr;
  if (inputs_on_device) {
    if (int rc = check_device_pointer(ids0, device, "ids0")) return rc;
    if (int rc = check_device_pointer(ids1, device, "ids1")) return rc;
    if (int rc = check_device_pointer(scores, device, "scores")) return rc;
    if (int rc = wait_for_caller(A, stream)) return rc;
    if (int rc = new_bad_flag(A, &d_bad)) return rc;
  } else {
    d_i0 = A.put(ids0, (size_t)n);
    d_i1 = A.put(ids1, (size_t)n);
    d_sc = A.put(scores, (size_t)n);
    if (!d_i0 || !d_i1 || !d_sc) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  }
  if (int rc = A.begin()) return rc;
  if (d_bad) {
    if (int rc = scan_device(A, d_sc, n, d_i0, n, n0, d_bad)) return rc;
    if (int rc = scan_device(A, nullptr, 0, d_i1, n, n1, d_bad)) return rc;
  }
  int32_t *d_m = nullptr, *d_counts = nullptr;
  float* d_s0 = nullptr;
  if (int rc = unique_core<int64_t>(A, (int32_t)n, d_i0, d_i1, d_sc, (int32_t)n0, (int32_t)n1, &d_m, &d_s0, &d_counts)) return rc;
  if (int rc = A.end()) return rc;
  if (int rc = read_bad(A, d_bad)) return rc;
  int32_t counts[3];
  MPSFM_TRY(A.down(counts, d_counts, sizeof(counts)));
  MPSFM_TRY(A.down(matches0, d_m, sizeof(int32_t) * (size_t)n0));
  MPSFM_TRY(A.down(scores0, d_s0, sizeof(float) * (size_t)n0));
  *n_kps0 = counts[0];
  if (info) { info->num_valid = counts[1]; info->num_matches = counts[2]; info->ms = (float)A.ms; }
  return 0;
}

extern "C" int mpsfm_warp_matches(int32_t H, int32_t W, const float* certainty, const float* warp, int32_t H_A, int32_t W_A, int32_t H_B, int32_t W_B,
                                  int32_t mode, const mpsfm_warp_options* opts, int64_t ns0, const double* skpts0, int64_t ns1, const double* skpts1,
                                  int32_t device, float* dkeypoints0, float* dkeypoints1, float* dscores, int64_t* n_dense, int32_t* smatches0,
                                  float* sscores0, int64_t* n_kps0, mpsfm_warp_info* info) {
  if (info) *info = mpsfm_warp_info{};
  if (n_dense) *n_dense = 0;
  if (n_kps0) *n_kps0 = 0;
  mpsfm_warp_options o;
  mpsfm_warp_default_options(&o);
  if (opts) o = *opts;
  const bool dense = (mode & MPSFM_WARP_DENSE) != 0, sparse = (mode & MPSFM_WARP_SPARSE) != 0;
  if ((mode & ~(MPSFM_WARP_DENSE | MPSFM_WARP_SPARSE)) != 0 || (!dense && !sparse)) return fail(MPSFM_EINVAL, "mode must name the dense leg, the sparse leg or both");
  if (H < 1 || W < 1) return fail(MPSFM_EINVAL, "a map needs at least one row and one column");
  if ((int64_t)H * (int64_t)W > kMaxRows) return fail(MPSFM_EINVAL, "more than 2^27 rows");
  if (H_A < 1 || W_A < 1 || H_B < 1 || W_B < 1) return fail(MPSFM_EINVAL, "image sizes must be positive");
  if (!certainty || !warp) return fail(MPSFM_EINVAL, "NULL pointer");
  if (dense) {
    if (!dkeypoints0 || !dkeypoints1 || !dscores || !n_dense) return fail(MPSFM_EINVAL, "NULL pointer");
    if (o.nms_radius < 0 || o.nms_radius > kMaxR) return fail(MPSFM_EINVAL, "radius must be 0 .. 64");
    if (!std::isfinite(o.sample_thresh) || std::fabs(o.sample_thresh) > (double)FLT_MAX) return fail(MPSFM_EINVAL, "sample_thresh is not finite as float32");
  }
  Box2 box0{}, box1{};
  if (sparse) {
    if (ns0 < 0 || ns1 < 0) return fail(MPSFM_EINVAL, "negative size");
    if (ns0 > kMaxRows || ns1 > kMaxRows) return fail(MPSFM_EINVAL, "more than 2^27 keypoints");
    if (!n_kps0 || (ns0 > 0 && (!skpts0 || !smatches0 || !sscores0)) || (ns1 > 0 && !skpts1)) return fail(MPSFM_EINVAL, "NULL pointer");
    if (!std::isfinite(o.max_error) || o.max_error < 0.0) return fail(MPSFM_EINVAL, "max_error must be finite and non-negative");
    for (int d = 0; d < 2; ++d)
      if (!std::isfinite(o.scale0[d]) || !std::isfinite(o.scale1[d])) return fail(MPSFM_EINVAL, "non-finite scale");
    if (!grid_box(skpts0, (size_t)ns0, box0) || !grid_box(skpts1, (size_t)ns1, box1)) return fail(MPSFM_EINVAL, "non-finite keypoint");
    if (!box_ok(box0) || !box_ok(box1)) return fail(MPSFM_EINVAL, "bounding box wider than DBL_MAX");
  }
  const size_t px = (size_t)H * (size_t)W;
  if (!o.inputs_on_device && (!all_finite(certainty, px) || !all_finite(warp, 4 * px))) return fail(MPSFM_EINVAL, "non-finite map or warp value");
  if (sparse) fill_empty(ns0, smatches0, sscores0);
  const bool lookups = sparse && ns0 > 0 && ns1 > 0;
  if (!dense && !lookups) return 0;
  if (int rc = open_device(device)) return rc;
  CallScope A;
  if (int rc = A.open(true)) return rc;
  const float *d_c = certainty, *d_w = warp;
  int32_t* d_bad = nullptr;
  if (o.inputs_on_device) {
    if (int rc = check_device_pointer(certainty, device, "certainty")) return rc;
    if (int rc = check_device_pointer(warp, device, "warp")) return rc;
    if (int rc = wait_for_caller(A, o.stream)) return rc;
    if (int rc = new_bad_flag(A, &d_bad)) return rc;
  } else {
    d_c = A.put(certainty, px);
    d_w = A.put(warp, 4 * px);
    if (!d_c || !d_w) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  }
  const int32_t n = (int32_t)px;
  WarpArgs a{};
  a.n = n;
  a.warp = d_w;
  a.hwA = (float)(W_A / 2.0); a.hhA = (float)(H_A / 2.0); a.hwB = (float)(W_B / 2.0); a.hhB = (float)(H_B / 2.0);
  a.sx0 = o.scale0[0]; a.sy0 = o.scale0[1]; a.sx1 = o.scale1[0]; a.sy1 = o.scale1[1];
  a.e2 = o.max_error * o.max_error;
  const double *d_k0 = nullptr, *d_k1 = nullptr;
  if (lookups) {
    d_k0 = A.put(skpts0, 2 * (size_t)ns0);
    d_k1 = A.put(skpts1, 2 * (size_t)ns1);
    if (!d_k0 || !d_k1) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  }
  if (int rc = A.begin()) return rc;
  if (d_bad) {
    if (int rc = scan_device(A, d_c, (int64_t)px, nullptr, 0, 0, d_bad)) return rc;
    if (int rc = scan_device(A, d_w, 4 * (int64_t)px, nullptr, 0, 0, d_bad)) return rc;
  }
  float *d_nms = nullptr, *d_dk0 = nullptr, *d_dk1 = nullptr, *d_ds = nullptr;
  int32_t* d_pos = nullptr;
  if (dense) {
    d_nms = A.alloc<float>(px);
    d_dk0 = A.alloc<float>(2 * px);
    d_dk1 = A.alloc<float>(2 * px);
    d_ds = A.alloc<float>(px);
    int32_t* d_flag = A.alloc<int32_t>(px + 1);
    d_pos = A.alloc<int32_t>(px + 1);
    if (!d_nms || !d_dk0 || !d_dk1 || !d_ds || !d_flag || !d_pos) return fail(MPSFM_ENOMEM, "hipMalloc failed");
    if (int rc = nms_core(A, H, W, o.nms_radius, d_c, d_nms)) return rc;
    hipLaunchKernelGGL(k_dense_flags, blocks_of((int64_t)n + 1), dim3(kPT), 0, A.st, n, d_nms, (float)o.sample_thresh, d_flag);
    MPSFM_TRY(hipGetLastError());
    size_t bytes = 0;
    MPSFM_TRY(rocprim::exclusive_scan(nullptr, bytes, d_flag, d_pos, 0, px + 1, rocprim::plus<int32_t>(), A.st));
    void* tmp = A.get(std::max<size_t>(bytes, 16));
    if (!tmp) return fail(MPSFM_ENOMEM, "hipMalloc failed");
    MPSFM_TRY(rocprim::exclusive_scan(tmp, bytes, d_flag, d_pos, 0, px + 1, rocprim::plus<int32_t>(), A.st));
    hipLaunchKernelGGL(k_dense_compact, blocks_of(n), dim3(kPT), 0, A.st, a, d_nms, d_flag, d_pos, d_dk0, d_dk1, d_ds);
    MPSFM_TRY(hipGetLastError());
  }
  int32_t *d_m = nullptr, *d_counts = nullptr;
  float* d_s0 = nullptr;
  if (lookups) {
    PointGrid g0{}, g1{};
    if (int rc = grid_build(A, (int32_t)ns0, d_k0, grid_spec(box0, o.max_error), false, g0)) return rc;
    if (int rc = grid_build(A, (int32_t)ns1, d_k1, grid_spec(box1, o.max_error), false, g1)) return rc;
    int32_t* d_i0 = A.alloc<int32_t>(px);
    int32_t* d_i1 = A.alloc<int32_t>(px);
    if (!d_i0 || !d_i1) return fail(MPSFM_ENOMEM, "hipMalloc failed");
    hipLaunchKernelGGL(k_warp_ids, blocks_of(n), dim3(kPT), 0, A.st, a, g0, g1, d_i0, d_i1);
    MPSFM_TRY(hipGetLastError());
    if (int rc = unique_core<int32_t>(A, n, d_i0, d_i1, d_c, (int32_t)ns0, (int32_t)ns1, &d_m, &d_s0, &d_counts)) return rc;
  }
  if (int rc = A.end()) return rc;
  if (int rc = read_bad(A, d_bad)) return rc;
  if (dense) {
    int32_t cnt = 0;
    MPSFM_TRY(A.down(&cnt, d_pos + px, sizeof(cnt)));
    if (cnt > 0) {
      MPSFM_TRY(A.down(dkeypoints0, d_dk0, sizeof(float) * 2 * (size_t)cnt));
      MPSFM_TRY(A.down(dkeypoints1, d_dk1, sizeof(float) * 2 * (size_t)cnt));
      MPSFM_TRY(A.down(dscores, d_ds, sizeof(float) * (size_t)cnt));
    }
    *n_dense = cnt;
    if (info) info->num_dense = cnt;
  }
  if (lookups) {
    int32_t counts[3];
    MPSFM_TRY(A.down(counts, d_counts, sizeof(counts)));
    MPSFM_TRY(A.down(smatches0, d_m, sizeof(int32_t) * (size_t)ns0));
    MPSFM_TRY(A.down(sscores0, d_s0, sizeof(float) * (size_t)ns0));
    *n_kps0 = counts[0];
    if (info) { info->num_valid = counts[1]; info->num_matches = counts[2]; }
  }
  if (info) info->ms = (float)A.ms;
  return 0;
}
