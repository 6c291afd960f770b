// Descriptors to match lists (mpsfm_match_descriptors, mpsfm_match_map_descriptors; semantics: include/mpsfm_hip.h, the
// arithmetic contract, the tie rule and the margin bounds: DESIGN.md section 4m).
//
//   k_sample_descriptors  bilinear samples of a channel-last map and of its confidence map at the keypoints, fp64
//   k_sim_top2<T>         similarity tiles on the matrix pipe (v_mfma_f64_16x16x4_f64), a running top-2 per row in registers;
//                         both directions in one launch, nothing of size n0 x n1 is ever written
//   k_match_decide        ratio / distance tests, mutual check, score threshold, outputs
//
// k_sim_top2: a workgroup of four waves owns a strip of kStrip = 64 rows and streams the columns (all of them, or one of
// gridDim.z ranges of column tiles when there are too few strips to fill the device).  The strip itself, the running top-2 and
// the decisions of a row are the bodies of sim_top2.h, which the batched matcher (descriptor_matches_batch.hip) calls too.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "call_scope.h"
#include "common.h"
#include "sim_tile.h"
#include "bilinear_sample.h"  // contraction off from here on: the decisions round every operation on its own
#include "sim_top2.h"

namespace mpsfm {

namespace {
using namespace sim;  // the tile geometry, before(), load_slice() and the device scan: sim_tile.h; Top2, the strip and the decisions: sim_top2.h

struct SimArgs {
  const void* X[2];   // descriptor sets 0 and 1, [n][dim]
  int32_t n[2];
  int32_t dim;
  int32_t vec;        // both sets allow 4-wide loads
  int32_t splits;     // workgroups that share a strip, each streaming its own range of column tiles (gridDim.z)
  double* val[2];     // [n][splits][2]: top-1 and top-2 similarity of every row of direction d (rows = set d) within a range
  int32_t* idx[2];    // [n][splits][2]: their columns (kNoIndex: the range held fewer than two)
};

template <typename T>
__global__ __launch_bounds__(kMT) void k_sim_top2(SimArgs a) {
  __shared__ double s_A[kKS * kLd];
  __shared__ double s_B[kKS * kLd];
  const int d = (int)blockIdx.y;
  const int32_t nrows = a.n[d], ncols = a.n[1 - d];
  const int32_t row0 = (int32_t)blockIdx.x * kStrip;
  if (row0 >= nrows) return;  // the grid is sized for the larger set
  // this workgroup's range of column tiles; an empty range leaves the sentinels, which every merge ignores
  const int32_t per = ((ncols + kStrip - 1) / kStrip + a.splits - 1) / a.splits * kStrip;
  const int64_t cb = (int64_t)blockIdx.z * per;
  const int32_t col_begin = (int32_t)min(cb, (int64_t)ncols), col_end = (int32_t)min(cb + per, (int64_t)ncols);
  sim_top2_strip<T>(s_A, s_B, (const T*)a.X[d], nrows, row0, (const T*)a.X[1 - d], ncols, col_begin, col_end, a.dim, a.vec != 0, a.splits,
                    (int32_t)blockIdx.z, a.val[d], a.idx[d]);
}

struct DecideArgs {
  int32_t n0, n1, splits;
  const double* val[2];
  const int32_t* idx[2];
  double ratio2, dist2, score_thr;
  int32_t use_ratio, use_dist, use_score, mutual;
  const double* conf0;  // sampled confidences (map entry) or NULL
  const double* conf1;
  int32_t* matches;
  double* scores;
};

__global__ __launch_bounds__(kDT) void k_match_decide(DecideArgs a) {
  const int32_t i = (int32_t)blockIdx.x * kDT + (int32_t)threadIdx.x;
  if (i >= a.n0) return;
  const Top2Table dir0{a.val[0], a.idx[0], a.splits, a.n1}, dir1{a.val[1], a.idx[1], a.splits, a.n0};
  const MatchRule rule{a.ratio2, a.dist2, a.score_thr, a.use_ratio, a.use_dist, a.use_score, a.mutual};
  double score;
  const int32_t m = match_of(dir0, dir1, rule, i, score);
  if (a.conf0) score = m >= 0 ? sqrt(a.conf0[i] * a.conf1[m]) : 0.0;
  a.matches[i] = m;
  a.scores[i] = score;
}

// bilinear() of bilinear_sample.h on one channel of a channel-last map
__device__ __forceinline__ double bilinear_channel(const float* __restrict__ map, int H, int W, int C, int c, double x, double y) {
  const double x0f = floor(x), y0f = floor(y);
  const double wx1 = x - x0f, wy1 = y - y0f;
  const double wx0 = 1.0 - wx1, wy0 = 1.0 - wy1;
  const bool fin = (x0f > -2.0) && (x0f < (double)W + 1.0) && (y0f > -2.0) && (y0f < (double)H + 1.0);
  if (!fin) return 0.0;
  const int x0 = (int)x0f, y0 = (int)y0f;
  double out = 0.0;
  const double w[4] = {wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int xi = x0 + (k & 1), yi = y0 + (k >> 1);
    if (xi >= 0 && xi < W && yi >= 0 && yi < H) {
      const double term = w[k] * (double)map[((size_t)yi * W + xi) * C + c];
      out = out + term;
    }
  }
  return out;
}

// one thread per (keypoint, channel); channel C is the confidence map
__global__ __launch_bounds__(kDT) void k_sample_descriptors(const float* __restrict__ map, const float* __restrict__ conf, int H, int W, int C,
                                                            int64_t n, const double* __restrict__ kps, double* __restrict__ desc,
                                                            double* __restrict__ cs) {
  const int64_t t = (int64_t)blockIdx.x * kDT + (int64_t)threadIdx.x;
  const int64_t i = t / (C + 1);
  const int c = (int)(t - i * (C + 1));
  if (i >= n) return;
  const double x = (double)(float)kps[2 * i], y = (double)(float)kps[2 * i + 1];
  if (c < C) desc[i * C + c] = bilinear_channel(map, H, W, C, c, x, y);
  else cs[i] = bilinear_channel(conf, H, W, 1, 0, x, y);
}

inline dim3 blocks_of(int64_t n) { return dim3((unsigned)((n + kDT - 1) / kDT)); }
// a float32 keypoint coordinate may overflow where the float64 one is finite
bool kps_ok(const double* k, size_t n) {
  for (size_t i = 0; i < 2 * n; ++i)
    if (!std::isfinite(k[i]) || !std::isfinite((float)k[i])) return false;
  return true;
}

// top-2 in both directions, the decisions and the download; d0 / d1 on the device, conf0 / conf1 device or NULL.  d_bad (may be
// NULL): the flag of the device scans, read with the outputs.
template <typename T>
int match_core(CallScope& A, int32_t device, int32_t n0, int32_t n1, int32_t dim, const T* d0, const T* d1, const double* conf0, const double* conf1,
               const mpsfm_match_options& o, const int32_t* d_bad, int32_t* matches0, double* scores0, mpsfm_match_info* info) {
  SimArgs s{};
  s.X[0] = d0; s.X[1] = d1;
  s.n[0] = n0; s.n[1] = n1;
  s.dim = dim;
  s.vec = (dim % 4 == 0 && ((uintptr_t)d0 % (4 * sizeof(T))) == 0 && ((uintptr_t)d1 % (4 * sizeof(T))) == 0) ? 1 : 0;
  const int dirs = o.mutual_check ? 2 : 1;
  const int32_t nmax = dirs == 2 ? std::max(n0, n1) : n0;
  const int32_t strips = (nmax + kStrip - 1) / kStrip;
  // a strip per workgroup leaves most of the device idle up to a few thousand descriptors: the column tiles of a strip are
  // shared out until there are about kFillPerCU workgroups per compute unit
  const int32_t col_tiles = ((dirs == 2 ? nmax : n1) + kStrip - 1) / kStrip;
  int cus = 0;
  MPSFM_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  const int64_t fill = (int64_t)kFillPerCU * std::max(cus, 1), wgs = (int64_t)strips * dirs;
  s.splits = (int32_t)std::max<int64_t>(1, std::min<int64_t>(col_tiles, (fill + wgs - 1) / wgs));
  for (int d = 0; d < dirs; ++d) {
    s.val[d] = A.alloc<double>(2 * (size_t)s.n[d] * s.splits);
    s.idx[d] = A.alloc<int32_t>(2 * (size_t)s.n[d] * s.splits);
    if (!s.val[d] || !s.idx[d]) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  }
  int32_t* d_m = A.alloc<int32_t>((size_t)n0);
  double* d_s = A.alloc<double>((size_t)n0);
  if (!d_m || !d_s) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  hipLaunchKernelGGL(k_sim_top2<T>, dim3((unsigned)strips, (unsigned)dirs, (unsigned)s.splits), dim3(kMT), 0, A.st, s);
  MPSFM_TRY(hipGetLastError());
  DecideArgs a{};
  a.n0 = n0; a.n1 = n1; a.splits = s.splits;
  for (int d = 0; d < 2; ++d) { a.val[d] = s.val[d]; a.idx[d] = s.idx[d]; }
  a.use_ratio = (o.ratio_threshold > 0.0 && n0 > 1 && n1 > 1) ? 1 : 0;
  a.use_dist = o.distance_threshold > 0.0 ? 1 : 0;
  a.use_score = o.score_threshold > 0.0 ? 1 : 0;
  a.ratio2 = o.ratio_threshold * o.ratio_threshold;
  a.dist2 = o.distance_threshold * o.distance_threshold;
  a.score_thr = o.score_threshold;
  a.mutual = o.mutual_check ? 1 : 0;
  a.conf0 = conf0; a.conf1 = conf1;
  a.matches = d_m; a.scores = d_s;
  hipLaunchKernelGGL(k_match_decide, blocks_of(n0), dim3(kDT), 0, A.st, a);
  MPSFM_TRY(hipGetLastError());
  if (int rc = A.end()) return rc;
  if (d_bad) {
    int32_t bad = 0;
    MPSFM_TRY(A.down(&bad, d_bad, sizeof(bad)));
    if (bad) return fail(MPSFM_EINVAL, "non-finite value in a device input");
  }
  MPSFM_TRY(A.down(matches0, d_m, sizeof(int32_t) * (size_t)n0));
  MPSFM_TRY(A.down(scores0, d_s, sizeof(double) * (size_t)n0));
  int64_t cnt = 0;
  for (int32_t i = 0; i < n0; ++i) cnt += matches0[i] >= 0;
  if (info) { info->num_matches = cnt; info->ms = (float)A.ms; info->column_ranges = s.splits; }
  return 0;
}
}  // namespace

}  // namespace mpsfm

using namespace mpsfm;

extern "C" void mpsfm_match_default_options(mpsfm_match_options* opts) {
  if (!opts) return;
  *opts = mpsfm_match_options{};
  opts->mutual_check = 1;
}

extern "C" int mpsfm_match_descriptors(int64_t n0, int64_t n1, int32_t dim, const float* desc0, const float* desc1,
                                       const mpsfm_match_options* opts, int32_t device, int32_t* matches0, double* scores0,
                                       mpsfm_match_info* info) {
  if (info) *info = mpsfm_match_info{};
  mpsfm_match_options o;
  mpsfm_match_default_options(&o);
  if (opts) o = *opts;
  if (n0 < 0 || n1 < 0) return fail(MPSFM_EINVAL, "negative size");
  if (n0 > kMaxDesc || n1 > kMaxDesc) return fail(MPSFM_EINVAL, "more than 2^24 descriptors");
  if (dim < 1 || dim > kMaxDim) return fail(MPSFM_EINVAL, "dim must be 1 .. 1024");
  if ((n0 > 0 && (!desc0 || !matches0 || !scores0)) || (n1 > 0 && !desc1)) return fail(MPSFM_EINVAL, "NULL pointer");
  if (int rc = check_match_options(o)) return rc;
  if (!o.inputs_on_device && (!all_finite(desc0, (size_t)n0 * dim) || !all_finite(desc1, (size_t)n1 * dim)))
    return fail(MPSFM_EINVAL, "non-finite descriptor value");
  if (n0 == 0) return 0;
  if (n1 == 0) { fill_empty(n0, matches0, scores0); return 0; }
  if (int rc = open_device(device)) return rc;
  CallScope A;
  if (int rc = A.open(true)) return rc;
  const float *d0 = desc0, *d1 = desc1;
  int32_t* d_bad = nullptr;
  if (o.inputs_on_device) {
    if (int rc = check_device_pointer(desc0, device, "desc0")) return rc;
    if (int rc = check_device_pointer(desc1, device, "desc1")) return rc;
    if (int rc = wait_for_caller(A, o.stream)) return rc;
    d_bad = A.alloc<int32_t>(1);
    if (!d_bad) return fail(MPSFM_ENOMEM, "hipMalloc failed");
    MPSFM_TRY(hipMemsetAsync(d_bad, 0, sizeof(int32_t), A.st));
  } else {
    d0 = A.put(desc0, (size_t)n0 * dim);
    d1 = A.put(desc1, (size_t)n1 * dim);
    if (!d0 || !d1) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  }
  if (int rc = A.begin()) return rc;
  if (d_bad) {
    if (int rc = scan_device(A, d0, n0 * dim, d_bad)) return rc;
    if (int rc = scan_device(A, d1, n1 * dim, d_bad)) return rc;
  }
  return match_core<float>(A, device, (int32_t)n0, (int32_t)n1, dim, d0, d1, nullptr, nullptr, o, d_bad, matches0, scores0, info);
}

extern "C" int mpsfm_match_map_descriptors(const float* map0, const float* conf0, int32_t H0, int32_t W0, const float* map1, const float* conf1,
                                           int32_t H1, int32_t W1, int32_t C, int64_t n0, const double* kps0, int64_t n1, const double* kps1,
                                           const mpsfm_match_options* opts, int32_t device, int32_t* matches0, double* scores0,
                                           mpsfm_match_info* info) {
  if (info) *info = mpsfm_match_info{};
  mpsfm_match_options o;
  mpsfm_match_default_options(&o);
  if (opts) o = *opts;
  if (n0 < 0 || n1 < 0) return fail(MPSFM_EINVAL, "negative size");
  if (n0 > kMaxDesc || n1 > kMaxDesc) return fail(MPSFM_EINVAL, "more than 2^24 keypoints");
  if (C < 1 || C > kMaxDim) return fail(MPSFM_EINVAL, "C must be 1 .. 1024");
  if (H0 < 2 || W0 < 2 || H1 < 2 || W1 < 2) return fail(MPSFM_EINVAL, "a map needs at least 2 rows and 2 columns");
  if (!map0 || !conf0 || !map1 || !conf1) return fail(MPSFM_EINVAL, "NULL pointer");
  if ((n0 > 0 && (!kps0 || !matches0 || !scores0)) || (n1 > 0 && !kps1)) return fail(MPSFM_EINVAL, "NULL pointer");
  if (int rc = check_match_options(o)) return rc;
  if (!kps_ok(kps0, (size_t)n0) || !kps_ok(kps1, (size_t)n1)) return fail(MPSFM_EINVAL, "non-finite keypoint");
  const size_t px0 = (size_t)H0 * (size_t)W0, px1 = (size_t)H1 * (size_t)W1;
  if (!o.inputs_on_device && (!all_finite(map0, px0 * C) || !all_finite(conf0, px0) || !all_finite(map1, px1 * C) || !all_finite(conf1, px1)))
    return fail(MPSFM_EINVAL, "non-finite map value");
  if (n0 == 0) return 0;
  if (n1 == 0) { fill_empty(n0, matches0, scores0); return 0; }
  if (int rc = open_device(device)) return rc;
  CallScope A;
  if (int rc = A.open(true)) return rc;
  const float* m[2] = {map0, map1};
  const float* c[2] = {conf0, conf1};
  const size_t px[2] = {px0, px1};
  int32_t* d_bad = nullptr;
  if (o.inputs_on_device) {
    for (int s = 0; s < 2; ++s) {
      if (int rc = check_device_pointer(m[s], device, s ? "map1" : "map0")) return rc;
      if (int rc = check_device_pointer(c[s], device, s ? "conf1" : "conf0")) return rc;
    }
    if (int rc = wait_for_caller(A, o.stream)) return rc;
    d_bad = A.alloc<int32_t>(1);
    if (!d_bad) return fail(MPSFM_ENOMEM, "hipMalloc failed");
    MPSFM_TRY(hipMemsetAsync(d_bad, 0, sizeof(int32_t), A.st));
  } else {
    for (int s = 0; s < 2; ++s) {
      m[s] = A.put(m[s], px[s] * C);
      c[s] = A.put(c[s], px[s]);
      if (!m[s] || !c[s]) return fail(MPSFM_ENOMEM, "hipMalloc failed");
    }
  }
  const int64_t n[2] = {n0, n1};
  const double* kh[2] = {kps0, kps1};
  const int32_t H[2] = {H0, H1}, W[2] = {W0, W1};
  double* desc[2];
  double* cs[2];
  const double* kd[2];
  for (int s = 0; s < 2; ++s) {
    kd[s] = A.put(kh[s], 2 * (size_t)n[s]);
    desc[s] = A.alloc<double>((size_t)n[s] * C);
    cs[s] = A.alloc<double>((size_t)n[s]);
    if (!kd[s] || !desc[s] || !cs[s]) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  }
  if (int rc = A.begin()) return rc;
  for (int s = 0; s < 2; ++s) {
    if (d_bad) {
      if (int rc = scan_device(A, m[s], (int64_t)(px[s] * C), d_bad)) return rc;
      if (int rc = scan_device(A, c[s], (int64_t)px[s], d_bad)) return rc;
    }
    hipLaunchKernelGGL(k_sample_descriptors, blocks_of(n[s] * (C + 1)), dim3(kDT), 0, A.st, m[s], c[s], H[s], W[s], C, n[s], kd[s], desc[s], cs[s]);
    MPSFM_TRY(hipGetLastError());
  }
  return match_core<double>(A, device, (int32_t)n0, (int32_t)n1, C, desc[0], desc[1], cs[0], cs[1], o, d_bad, matches0, scores0, info);
}
