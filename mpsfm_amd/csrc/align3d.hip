// Rigid / similarity alignment of two 3D point sets and the RGB-D pair registration built on it (mpsfm_align3d_estimate,
// mpsfm_align3d_fit, mpsfm_lift_keypoints, mpsfm_depth_pair_register; semantics: include/mpsfm_hip.h).  The loop, the scoring
// kernels and the batch tables are lo_ransac.h's; this file describes the problem to it:
//   k_a3_minimal      one thread per trial of a batch: the trial's counter-based sample and the 3-point closed form
//   A3Problem::local  the same closed form on the current inlier set: two fixed-order reductions on the device
//                     (k_a3_pass<1>: count and sums, k_a3_pass<2>: the centred cross and scatter sums) and the 3x3 / 4x4
//                     algebra on the host (align3d_math.h)
// and the lifting side:
//   k_a3_lift          one thread per keypoint: the bilinear sample of the point map that is never materialised
//   k_a3_lift_matches  one thread per match: both ends lifted
//   k_a3_compact       one workgroup: the valid matches in match order as the estimator's SoA points
//   k_a3_scatter       the estimator's mask back to the matches
// a3_register_check / a3_register_device (align3d_device.h) are mpsfm_depth_pair_register in two halves, so that
// mpsfm_depth_pair_register_dense (depth_icp.hip) continues on the same scope and the same uploaded maps.  f64 throughout.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "align3d_device.h"
#include "align3d_math.h"
#include "common.h"
#include "lo_ransac.h"

namespace mpsfm {

namespace {
constexpr int kT = kLoT;

struct A3Pts { const double *px, *py, *pz, *qx, *qy, *qz; };

__global__ __launch_bounds__(kT) void k_a3_minimal(uint64_t seed, int64_t t0, int32_t nb, int32_t n, A3Pts p, int with_scale,
                                                    double* __restrict__ models, int32_t* __restrict__ nmod) {
  const int32_t i = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  if (i >= nb) return;
  int32_t idx[3];
  lo_sample<3>(seed, t0 + i, n, idx);
  double P[3][3], Q[3][3];
  for (int k = 0; k < 3; ++k) {
    P[k][0] = p.px[idx[k]]; P[k][1] = p.py[idx[k]]; P[k][2] = p.pz[idx[k]];
    Q[k][0] = p.qx[idx[k]]; Q[k][1] = p.qy[idx[k]]; Q[k][2] = p.qz[idx[k]];
  }
  double M[kA3Model];
  const bool ok = a3_minimal(P, Q, with_scale, M);
  double* out = models + (size_t)i * kA3Model;
  for (int k = 0; k < kA3Model; ++k) out[k] = ok ? M[k] : 0.0;  // the slot of a trial without a model is scored but never read
  nmod[i] = ok ? 1 : 0;
}

// which points a fit runs over: the inliers of Min (residual <= thr2), or the points a mask keeps (NULL: all)
struct A3Select {
  double Min[kA3Model];
  double thr2;
  const uint8_t* mask;
  int by_model;
};
struct A3PassArgs {
  A3Select sel;
  double mp[3], mq[3];  // pass 2: the centroids
};
template <int PASS> struct A3PassK;
template <> struct A3PassK<1> { static constexpr int K = 7; };   // count, sum p, sum q
template <> struct A3PassK<2> { static constexpr int K = 22; };  // 9 cross terms (row a of source, column b of target), 6 + 6 scatter terms, sum |p - mp|^2

template <int PASS>
__global__ __launch_bounds__(kT) void k_a3_pass(A3PassArgs a, int32_t n, A3Pts p, double* __restrict__ part) {
  constexpr int K = A3PassK<PASS>::K;
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
  for (int32_t i = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x; i < n; i += (int32_t)gridDim.x * kT) {
    const double px = p.px[i], py = p.py[i], pz = p.pz[i], qx = p.qx[i], qy = p.qy[i], qz = p.qz[i];
    const bool in = a.sel.by_model ? a3_residual(a.sel.Min, px, py, pz, qx, qy, qz) <= a.sel.thr2 : (!a.sel.mask || a.sel.mask[i] != 0);
    if (!in) continue;
    if (PASS == 1) {
      acc[0] += 1.0; acc[1] += px; acc[2] += py; acc[3] += pz; acc[4] += qx; acc[5] += qy; acc[6] += qz;
    } else {
      const double d[3] = {px - a.mp[0], py - a.mp[1], pz - a.mp[2]}, e[3] = {qx - a.mq[0], qy - a.mq[1], qz - a.mq[2]};
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[3 * r + c] += d[r] * e[c];
      acc[9] += d[0] * d[0]; acc[10] += d[0] * d[1]; acc[11] += d[0] * d[2]; acc[12] += d[1] * d[1]; acc[13] += d[1] * d[2]; acc[14] += d[2] * d[2];
      acc[15] += e[0] * e[0]; acc[16] += e[0] * e[1]; acc[17] += e[0] * e[2]; acc[18] += e[1] * e[1]; acc[19] += e[1] * e[2]; acc[20] += e[2] * e[2];
      acc[21] += d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    }
  }
  block_reduce_rows<K>(acc, part);
}

// the problem description of lo_ransac.h
struct A3Problem {
  static constexpr int kSample = 3, kModel = kA3Model, kSlots = 1, kLocal = 1;
  static constexpr int kDefaultBatch = 256;  // trials per batch
  using Pts = A3Pts;
  struct Obs { double px, py, pz, qx, qy, qz; };
  static __device__ __forceinline__ Obs load(const Pts& p, int32_t i) { return {p.px[i], p.py[i], p.pz[i], p.qx[i], p.qy[i], p.qz[i]}; }
  static __device__ __forceinline__ double residual(const double* M, const Obs& o) { return a3_residual(M, o.px, o.py, o.pz, o.qx, o.qy, o.qz); }

  int32_t n = 0;
  double thr2 = 0.0;
  Pts pts{};
  int with_scale = 0;
  int npx = 0;  // workgroups of a fit pass
  double* d_part = nullptr;
  std::vector<double> h_part;

  // the blocks of the fit passes; false: out of memory
  bool prepare(CallScope& A) {
    npx = lo_blocks(n, kT);
    d_part = A.alloc<double>((size_t)A3PassK<2>::K * npx);
    h_part.resize((size_t)A3PassK<2>::K * npx);
    return d_part != nullptr;
  }

  void minimal(hipStream_t st, uint64_t seed, int64_t t0, int32_t nb, double* models, int32_t* nmod) const {
    hipLaunchKernelGGL(k_a3_minimal, dim3((unsigned)((nb + kT - 1) / kT)), dim3(kT), 0, st, seed, t0, nb, n, pts, with_scale, models, nmod);
  }

  // one pass: the workgroups' rows summed in order into out[K]
  template <int PASS>
  int pass(CallScope& A, const A3PassArgs& a, double* out) {
    constexpr int K = A3PassK<PASS>::K;
    if (int rc = A.begin()) return rc;
    hipLaunchKernelGGL(k_a3_pass<PASS>, dim3((unsigned)npx), dim3(kT), 0, A.st, a, n, pts, d_part);
    MPSFM_TRY(hipGetLastError());
    MPSFM_TRY(hipMemcpyAsync(h_part.data(), d_part, sizeof(double) * K * (size_t)npx, hipMemcpyDeviceToHost, A.st));
    if (int rc = A.end()) return rc;
    sum_rows(h_part.data(), npx, K, out);
    return 0;
  }

  // the closed form over the selected points; nm = 0: no model.  used: the points selected
  int fit(CallScope& A, const A3Select& sel, double* Mout, int& nm, int64_t& used) {
    nm = 0;
    A3PassArgs a{};
    a.sel = sel;
    double s1[7];
    if (int rc = pass<1>(A, a, s1)) return rc;
    const int64_t m = (int64_t)s1[0];
    used = m;
    if (m < 3) return 0;
    for (int d = 0; d < 3; ++d) { a.mp[d] = s1[1 + d] / (double)m; a.mq[d] = s1[4 + d] / (double)m; }
    double s2[22];
    if (int rc = pass<2>(A, a, s2)) return rc;
    if (a3_scatter_is_line(s2 + 9) || a3_scatter_is_line(s2 + 15)) return 0;
    double S[3][3];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) S[r][c] = s2[3 * r + c];
    if (a3_from_sums(S, s2[21], a.mp, a.mq, with_scale, Mout)) nm = 1;
    return 0;
  }

  int local(CallScope& A, const double* Min, double* Mout, int& nm) {
    A3Select sel{};
    std::memcpy(sel.Min, Min, sizeof(sel.Min));
    sel.thr2 = thr2;
    sel.by_model = 1;
    int64_t used = 0;
    return fit(A, sel, Mout, nm, used);
  }
};

void a3_store_model(const double* M, mpsfm_align3d_result* result) {
  std::memcpy(result->tgt_from_src, M, sizeof(double) * 12);
  result->scale = M[12];
}

// the estimate over points that are on the device (scope open and timed); d_mask [n] receives the mask of a success
int a3_estimate_device(CallScope& A, int32_t n, const A3Pts& pts, int with_scale, const mpsfm_align3d_options& o, uint8_t* d_mask,
                       mpsfm_align3d_result* result) {
  A3Problem prob;
  prob.n = n;
  prob.thr2 = o.max_error * o.max_error;
  prob.pts = pts;
  prob.with_scale = with_scale ? 1 : 0;
  if (!prob.prepare(A)) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  LoReport rep;
  double best_model[kA3Model] = {};
  if (int rc = lo_ransac(prob, A, o, rep, best_model)) return rc;
  result->num_trials = rep.num_trials;
  result->max_num_trials = rep.max_num_trials;
  result->num_models = rep.num_models;
  result->lo_rounds = (int32_t)rep.lo_rounds;
  result->num_batches = (int32_t)rep.num_batches;
  if (rep.best.num_inliers < 3) return 0;
  if (int rc = A.begin()) return rc;
  if (int rc = lo_mask(prob, A, best_model, d_mask)) return rc;
  if (int rc = A.end()) return rc;
  a3_store_model(best_model, result);
  result->num_inliers = rep.best.num_inliers;
  result->success = 1;
  return 0;
}

// [n][3] host rows of both sets as the SoA block px py pz qx qy qz
void a3_soa(int32_t n, const double* src, const double* tgt, std::vector<double>& hs) {
  hs.resize((size_t)6 * n);
  for (int32_t i = 0; i < n; ++i)
    for (int d = 0; d < 3; ++d) {
      hs[(size_t)d * n + i] = src[3 * (size_t)i + d];
      hs[(size_t)(3 + d) * n + i] = tgt[3 * (size_t)i + d];
    }
}
A3Pts a3_pts(const double* d, size_t stride) { return A3Pts{d, d + stride, d + 2 * stride, d + 3 * stride, d + 4 * stride, d + 5 * stride}; }

// ---- lifting -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void k_a3_lift(A3Map m, int64_t n, const double* __restrict__ xy, double* __restrict__ xyz, uint8_t* __restrict__ valid) {
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  double v[3];
  const bool ok = a3_lift(m.depth, m.H, m.W, m.intr, xy[2 * i], xy[2 * i + 1], v);
  xyz[3 * i] = v[0]; xyz[3 * i + 1] = v[1]; xyz[3 * i + 2] = v[2];
  valid[i] = ok ? 1 : 0;
}

__global__ __launch_bounds__(kT) void k_a3_lift_matches(A3Map m0, A3Map m1, int32_t m, const int32_t* __restrict__ matches,
                                                         const double* __restrict__ xy0, const double* __restrict__ xy1,
                                                         double* __restrict__ l0, double* __restrict__ l1, uint8_t* __restrict__ valid) {
  const int32_t i = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  if (i >= m) return;
  const int32_t k0 = matches[2 * (size_t)i], k1 = matches[2 * (size_t)i + 1];  // in range: checked on the host
  double a[3], b[3];
  const bool ok0 = a3_lift(m0.depth, m0.H, m0.W, m0.intr, xy0[2 * (size_t)k0], xy0[2 * (size_t)k0 + 1], a);
  const bool ok1 = a3_lift(m1.depth, m1.H, m1.W, m1.intr, xy1[2 * (size_t)k1], xy1[2 * (size_t)k1 + 1], b);
  for (int d = 0; d < 3; ++d) { l0[3 * (size_t)i + d] = a[d]; l1[3 * (size_t)i + d] = b[d]; }
  valid[i] = ok0 && ok1 ? 1 : 0;
}

// One workgroup walks the matches in chunks of kT: the valid ones, in match order, become the estimator's points
// (SoA rows of stride m in pts) and orig[j] = their match; count[0] = how many
__global__ __launch_bounds__(kT) void k_a3_compact(int32_t m, const uint8_t* __restrict__ valid, const double* __restrict__ l0,
                                                    const double* __restrict__ l1, double* __restrict__ pts, int32_t* __restrict__ orig,
                                                    int32_t* __restrict__ count) {
  __shared__ int wave_cnt[kLoWaves];
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  int32_t base = 0;
  for (int32_t c0 = 0; c0 < m; c0 += kT) {
    const int32_t i = c0 + (int32_t)threadIdx.x;
    const bool v = i < m && valid[i] != 0;
    const unsigned long long bal = __ballot(v);
    if (lane == 0) wave_cnt[wave] = __popcll(bal);
    __syncthreads();
    int32_t before = 0, total = 0;
    for (int w = 0; w < kLoWaves; ++w) {
      if (w < wave) before += wave_cnt[w];
      total += wave_cnt[w];
    }
    if (v) {
      const int32_t j = base + before + __popcll(bal & ((1ull << lane) - 1ull));
      for (int d = 0; d < 3; ++d) {
        pts[(size_t)d * m + j] = l0[3 * (size_t)i + d];
        pts[(size_t)(3 + d) * m + j] = l1[3 * (size_t)i + d];
      }
      orig[j] = i;
    }
    base += total;
    __syncthreads();  // wave_cnt is rewritten by the next chunk
  }
  if (threadIdx.x == 0) count[0] = base;
}

__global__ __launch_bounds__(kT) void k_a3_scatter(int32_t nc, const uint8_t* __restrict__ mask_c, const int32_t* __restrict__ orig,
                                                    uint8_t* __restrict__ mask_m) {
  const int32_t j = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  if (j >= nc) return;
  mask_m[orig[j]] = mask_c[j];
}

bool a3_map_valid(int32_t H, int32_t W, const double* depth, const double* intr) {
  return depth && intr && H >= 1 && W >= 1 && (int64_t)H * W <= INT32_MAX && finite_all(intr, 4) && intr[0] != 0.0 && intr[1] != 0.0;
}
}  // namespace

}  // namespace mpsfm

using namespace mpsfm;

extern "C" int mpsfm_align3d_estimate(int64_t n64, const double* src, const double* tgt, int32_t with_scale, const mpsfm_align3d_options* o,
                                      int32_t device, uint8_t* inlier_mask, mpsfm_align3d_result* result) {
  if (result) *result = mpsfm_align3d_result{};
  if (!src || !tgt || !o || !inlier_mask || !result) return fail(MPSFM_EINVAL, "NULL pointer");
  if (n64 < 3) return fail(MPSFM_EINVAL, "fewer than 3 point pairs");
  if (n64 > INT32_MAX) return fail(MPSFM_EINVAL, "more than INT32_MAX point pairs (int32 indexing)");
  const int32_t n = (int32_t)n64;
  if (!finite_all(src, 3 * (size_t)n) || !finite_all(tgt, 3 * (size_t)n)) return fail(MPSFM_EINVAL, "non-finite point");
  if (!lo_options_valid(*o)) return fail(MPSFM_EINVAL, "invalid RANSAC options");
  if (int rc = open_device(device)) return rc;

  std::vector<double> hs;
  a3_soa(n, src, tgt, hs);
  CallScope A;
  if (int rc = A.open(true)) return rc;
  double* d_pts = A.alloc<double>(6 * (size_t)n);
  uint8_t* d_mask = A.alloc<uint8_t>((size_t)n);
  if (!d_pts || !d_mask) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  MPSFM_TRY(hipMemcpyAsync(d_pts, hs.data(), sizeof(double) * 6 * (size_t)n, hipMemcpyHostToDevice, A.st));
  if (int rc = a3_estimate_device(A, n, a3_pts(d_pts, (size_t)n), with_scale, *o, d_mask, result)) return rc;
  if (result->success) MPSFM_TRY(A.down(inlier_mask, d_mask, (size_t)n));
  else std::memset(inlier_mask, 0, (size_t)n);
  result->ms = (float)A.ms;
  return 0;
}

extern "C" int mpsfm_align3d_fit(int64_t n64, const double* src, const double* tgt, const uint8_t* mask, int32_t with_scale, int32_t device,
                                 mpsfm_align3d_result* result) {
  if (result) *result = mpsfm_align3d_result{};
  if (!src || !tgt || !result) return fail(MPSFM_EINVAL, "NULL pointer");
  if (n64 < 3) return fail(MPSFM_EINVAL, "fewer than 3 point pairs");
  if (n64 > INT32_MAX) return fail(MPSFM_EINVAL, "more than INT32_MAX point pairs (int32 indexing)");
  const int32_t n = (int32_t)n64;
  if (!finite_all(src, 3 * (size_t)n) || !finite_all(tgt, 3 * (size_t)n)) return fail(MPSFM_EINVAL, "non-finite point");
  if (int rc = open_device(device)) return rc;

  std::vector<double> hs;
  a3_soa(n, src, tgt, hs);
  CallScope A;
  if (int rc = A.open(true)) return rc;
  double* d_pts = A.alloc<double>(6 * (size_t)n);
  uint8_t* d_sel = mask ? A.alloc<uint8_t>((size_t)n) : nullptr;
  if (!d_pts || (mask && !d_sel)) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  MPSFM_TRY(hipMemcpyAsync(d_pts, hs.data(), sizeof(double) * 6 * (size_t)n, hipMemcpyHostToDevice, A.st));
  if (mask) MPSFM_TRY(hipMemcpyAsync(d_sel, mask, (size_t)n, hipMemcpyHostToDevice, A.st));
  A3Problem prob;
  prob.n = n;
  prob.pts = a3_pts(d_pts, (size_t)n);
  prob.with_scale = with_scale ? 1 : 0;
  if (!prob.prepare(A)) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  A3Select sel{};
  sel.mask = d_sel;
  double M[kA3Model] = {};
  int nm = 0;
  int64_t used = 0;
  if (int rc = prob.fit(A, sel, M, nm, used)) return rc;
  result->num_inliers = used;
  if (nm) {
    a3_store_model(M, result);
    result->num_models = 1;
    result->success = 1;
  }
  result->ms = (float)A.ms;
  return 0;
}

extern "C" int mpsfm_lift_keypoints(int32_t H, int32_t W, const double* depth, const double* intr, int64_t n, const double* xy, int32_t device,
                                    double* xyz, uint8_t* valid) {
  if (n < 0 || n > INT32_MAX) return fail(MPSFM_EINVAL, "keypoint count out of range");
  if (!a3_map_valid(H, W, depth, intr)) return fail(MPSFM_EINVAL, "depth map or intrinsics invalid (NULL, empty, or a zero / non-finite focal length)");
  if (n > 0 && (!xy || !xyz || !valid)) return fail(MPSFM_EINVAL, "NULL pointer");
  if (n == 0) return 0;
  if (int rc = open_device(device)) return rc;
  CallScope A;
  if (int rc = A.open()) return rc;
  A3Map m{A.put(depth, (size_t)H * W), H, W, {intr[0], intr[1], intr[2], intr[3]}};
  const double* d_xy = A.put(xy, 2 * (size_t)n);
  double* d_xyz = A.alloc<double>(3 * (size_t)n);
  uint8_t* d_valid = A.alloc<uint8_t>((size_t)n);
  if (!m.depth || !d_xy || !d_xyz || !d_valid) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  hipLaunchKernelGGL(k_a3_lift, dim3((unsigned)((n + kT - 1) / kT)), dim3(kT), 0, A.st, m, n, d_xy, d_xyz, d_valid);
  MPSFM_TRY(hipGetLastError());
  MPSFM_TRY(hipMemcpyAsync(xyz, d_xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(A.down(valid, d_valid, (size_t)n));
  return 0;
}

namespace mpsfm {

int a3_register_check(int32_t H0, int32_t W0, const double* depth0, const double* intr0, int32_t H1, int32_t W1,
                       const double* depth1, const double* intr1, int64_t n0, const double* xy0, int64_t n1, const double* xy1, int64_t m64,
                       const int32_t* matches, int32_t with_scale, const mpsfm_align3d_options* o, uint8_t* valid, uint8_t* inlier_mask,
                       double* lifted0, double* lifted1, mpsfm_align3d_result* result) {
  if (result) *result = mpsfm_align3d_result{};
  if (!o || !result) return fail(MPSFM_EINVAL, "NULL pointer");
  if (!a3_map_valid(H0, W0, depth0, intr0) || !a3_map_valid(H1, W1, depth1, intr1))
    return fail(MPSFM_EINVAL, "depth map or intrinsics invalid (NULL, empty, or a zero / non-finite focal length)");
  if (n0 < 0 || n1 < 0 || n0 > INT32_MAX || n1 > INT32_MAX || m64 < 0 || m64 > INT32_MAX) return fail(MPSFM_EINVAL, "count out of range");
  if ((n0 > 0 && !xy0) || (n1 > 0 && !xy1)) return fail(MPSFM_EINVAL, "NULL pointer");
  if (m64 > 0 && (!matches || !valid || !inlier_mask || !lifted0 || !lifted1)) return fail(MPSFM_EINVAL, "NULL pointer");
  const int32_t m = (int32_t)m64;
  for (int32_t i = 0; i < m; ++i)
    if (matches[2 * (size_t)i] < 0 || matches[2 * (size_t)i] >= n0 || matches[2 * (size_t)i + 1] < 0 || matches[2 * (size_t)i + 1] >= n1)
      return fail(MPSFM_EINVAL, "match index out of range");
  if (!lo_options_valid(*o)) return fail(MPSFM_EINVAL, "invalid RANSAC options");
  return 0;
}

int a3_register_device(CallScope& A, int32_t H0, int32_t W0, const double* depth0, const double* intr0, int32_t H1, int32_t W1,
                       const double* depth1, const double* intr1, int64_t n0, const double* xy0, int64_t n1, const double* xy1, int64_t m64,
                       const int32_t* matches, int32_t with_scale, const mpsfm_align3d_options* o, uint8_t* valid, uint8_t* inlier_mask,
                       double* lifted0, double* lifted1, mpsfm_align3d_result* result, A3Map* map0, A3Map* map1) {
  const int32_t m = (int32_t)m64;
  A3Map m0{A.put(depth0, (size_t)H0 * W0), H0, W0, {intr0[0], intr0[1], intr0[2], intr0[3]}};
  A3Map m1{A.put(depth1, (size_t)H1 * W1), H1, W1, {intr1[0], intr1[1], intr1[2], intr1[3]}};
  const double* d_xy0 = A.put(xy0, 2 * (size_t)n0);
  const double* d_xy1 = A.put(xy1, 2 * (size_t)n1);
  const int32_t* d_matches = A.put(matches, 2 * (size_t)m);
  double* d_l0 = A.alloc<double>(3 * (size_t)m);
  double* d_l1 = A.alloc<double>(3 * (size_t)m);
  double* d_pts = A.alloc<double>(6 * (size_t)m);
  uint8_t* d_valid = A.alloc<uint8_t>((size_t)m);
  uint8_t* d_mask_c = A.alloc<uint8_t>((size_t)m);
  uint8_t* d_mask_m = A.alloc<uint8_t>((size_t)m);
  int32_t* d_orig = A.alloc<int32_t>((size_t)m);
  int32_t* d_count = A.alloc<int32_t>(1);
  if (!m0.depth || !m1.depth || !d_xy0 || !d_xy1 || !d_matches || !d_l0 || !d_l1 || !d_pts || !d_valid || !d_mask_c || !d_mask_m || !d_orig || !d_count)
    return fail(MPSFM_ENOMEM, "hipMalloc failed");
  if (int rc = A.begin()) return rc;
  hipLaunchKernelGGL(k_a3_lift_matches, dim3((unsigned)((m + kT - 1) / kT)), dim3(kT), 0, A.st, m0, m1, m, d_matches, d_xy0, d_xy1, d_l0, d_l1, d_valid);
  MPSFM_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_a3_compact, dim3(1), dim3(kT), 0, A.st, m, d_valid, d_l0, d_l1, d_pts, d_orig, d_count);
  MPSFM_TRY(hipGetLastError());
  MPSFM_TRY(hipMemsetAsync(d_mask_m, 0, (size_t)m, A.st));
  int32_t nc = 0;
  MPSFM_TRY(hipMemcpyAsync(&nc, d_count, sizeof(int32_t), hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipMemcpyAsync(valid, d_valid, (size_t)m, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipMemcpyAsync(lifted0, d_l0, sizeof(double) * 3 * (size_t)m, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipMemcpyAsync(lifted1, d_l1, sizeof(double) * 3 * (size_t)m, hipMemcpyDeviceToHost, A.st));
  if (int rc = A.end()) return rc;  // the one wait that delivers the count
  if (nc >= 3) {
    if (int rc = a3_estimate_device(A, nc, a3_pts(d_pts, (size_t)m), with_scale, *o, d_mask_c, result)) return rc;
    if (result->success) {
      if (int rc = A.begin()) return rc;
      hipLaunchKernelGGL(k_a3_scatter, dim3((unsigned)((nc + kT - 1) / kT)), dim3(kT), 0, A.st, nc, d_mask_c, d_orig, d_mask_m);
      MPSFM_TRY(hipGetLastError());
      if (int rc = A.end()) return rc;
    }
  }
  MPSFM_TRY(A.down(inlier_mask, d_mask_m, (size_t)m));
  if (map0) *map0 = m0;
  if (map1) *map1 = m1;
  return 0;
}

}  // namespace mpsfm

extern "C" int mpsfm_depth_pair_register(int32_t H0, int32_t W0, const double* depth0, const double* intr0, int32_t H1, int32_t W1,
                                         const double* depth1, const double* intr1, int64_t n0, const double* xy0, int64_t n1,
                                         const double* xy1, int64_t m64, const int32_t* matches, int32_t with_scale,
                                         const mpsfm_align3d_options* o, int32_t device, uint8_t* valid, uint8_t* inlier_mask,
                                         double* lifted0, double* lifted1, mpsfm_align3d_result* result) {
  if (int rc = a3_register_check(H0, W0, depth0, intr0, H1, W1, depth1, intr1, n0, xy0, n1, xy1, m64, matches, with_scale, o, valid, inlier_mask,
                                 lifted0, lifted1, result))
    return rc;
  if (m64 == 0) return 0;
  if (int rc = open_device(device)) return rc;
  CallScope A;
  if (int rc = A.open(true)) return rc;
  if (int rc = a3_register_device(A, H0, W0, depth0, intr0, H1, W1, depth1, intr1, n0, xy0, n1, xy1, m64, matches, with_scale, o, valid,
                                  inlier_mask, lifted0, lifted1, result, nullptr, nullptr))
    return rc;
  result->ms = (float)A.ms;
  return 0;
}
