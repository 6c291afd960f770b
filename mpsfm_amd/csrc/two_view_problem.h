// What mpsfm_two_view_geometry (two_view.hip) and mpsfm_two_view_geometry_batch (two_view_batch.hip) share: the kernels and
// problem descriptions of the F, H and translation legs (the E leg is rel_pose_problem.h's), the pose kernel, and the host
// stages between the legs (argument checks, decision, watermark selection, pose candidates, winner and median).  As in
// rel_pose_problem.h the kernels have internal linkage: each translation unit carries its own copy, compiled from the same
// text, and drops the ones it does not launch.  The kernels:
//   k_tv_f7        one thread per trial: the seven-index sample, the 7 x 9 nullspace and the cubic in a per-thread LDS slice
//                  (two_view_math.h), up to 3 canonical F in lexicographic order (zeros pad)
//   k_tv_h4        one thread per trial: the four-index sample, Hartley normalisation, the 8 x 9 null vector, one canonical H
//   k_tv_t1        one thread per trial: the translation x2 - x1 of one match (watermark test)
//   k_tv_moments   count and coordinate sums of the inliers of a model            } the local estimators: fixed-order
//   k_tv_gram      upper triangle of the 9 x 9 Gram matrix of the centred design  } reductions, the 9 x 9 eigenvectors,
//                  rows of the inliers (F: one row per match, H: two)             } rank 2 and denormalisation on the host
//   k_tv_tsum      count and summed x2 - x1 of the inliers of a translation
//   k_tv_pose      up to 4 general (R, t) candidates against every chosen inlier in one pass: cheirality counts and the
//                  triangulation angle of every (inlier, candidate)
// f64 throughout.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "common.h"
#include "rel_pose_problem.h"
#include "two_view_math.h"

namespace mpsfm {

namespace {
constexpr int kSevenT = 64;  // trials per k_tv_f7 workgroup: 64 x (TVF_WORK doubles + 7 indices) = 45.75 KiB of LDS
constexpr int kFourT = 64;   // trials per k_tv_h4 workgroup: 64 x TVH_WORK doubles = 44.5 KiB of LDS
constexpr int kMomK = 5, kGram9K = 45, kTsumK = 3;
// trials per batch: the minimum is 100 trials here, not the 1000 of mpsfm_rel_pose_estimate
constexpr int kTvEBatch = 256, kTvFBatch = 256, kTvHBatch = 256, kTvTBatch = 128;

using TvModel = LoModel<9>;

// The bodies of the kernels and of their batched forms (two_view_batch.hip), as in rel_pose_problem.h: the trial, or the
// number nblk of workgroups along the problem's observations, and the output pointers at the problem's rows are arguments.

// trial t of k_tv_f7, by thread threadIdx.x of a workgroup of kSevenT
__device__ __forceinline__ void tv_f7_trial(uint64_t seed, int64_t t, int32_t n, const RpPts& p, double* __restrict__ out, int32_t* __restrict__ nmod) {
  __shared__ double work[kSevenT * TVF_WORK];
  __shared__ int32_t sidx[kSevenT * kTvFSample];  // the sampler indexes its output at run time: LDS too (odd stride, no bank conflict)
  int32_t* idx = sidx + kTvFSample * threadIdx.x;
  lo_sample<kTvFSample>(seed, t, n, idx);
  double u1[kTvFSample], v1[kTvFSample], u2[kTvFSample], v2[kTvFSample];
#pragma unroll
  for (int k = 0; k < kTvFSample; ++k) { u1[k] = p.u1[idx[k]]; v1[k] = p.v1[idx[k]]; u2[k] = p.u2[idx[k]]; v2[k] = p.v2[idx[k]]; }
  const RpW w{work + threadIdx.x, kSevenT};
  const int nm = tv_seven_point(u1, v1, u2, v2, w, out);
  for (int k = 9 * nm; k < 9 * kTvFMaxModels; ++k) out[k] = 0.0;
  *nmod = nm;
}

__global__ __launch_bounds__(kSevenT) void k_tv_f7(uint64_t seed, int64_t t0, int32_t nb, int32_t n, RpPts p, double* __restrict__ models,
                                                    int32_t* __restrict__ nmod) {
  const int32_t i = (int32_t)blockIdx.x * kSevenT + (int32_t)threadIdx.x;
  if (i >= nb) return;
  tv_f7_trial(seed, t0 + i, n, p, models + (size_t)i * 9 * kTvFMaxModels, nmod + i);
}

// trial t of k_tv_h4, by thread threadIdx.x of a workgroup of kFourT
__device__ __forceinline__ void tv_h4_trial(uint64_t seed, int64_t t, int32_t n, const RpPts& p, double* __restrict__ out, int32_t* __restrict__ nmod) {
  __shared__ double work[kFourT * TVH_WORK];
  int32_t idx[kTvHSample];
  lo_sample<kTvHSample>(seed, t, n, idx);
  double u1[kTvHSample], v1[kTvHSample], u2[kTvHSample], v2[kTvHSample];
#pragma unroll
  for (int k = 0; k < kTvHSample; ++k) { u1[k] = p.u1[idx[k]]; v1[k] = p.v1[idx[k]]; u2[k] = p.u2[idx[k]]; v2[k] = p.v2[idx[k]]; }
  const RpW w{work + threadIdx.x, kFourT};
  double H[9];
  const bool ok = tv_four_point(u1, v1, u2, v2, w, H);
#pragma unroll
  for (int k = 0; k < 9; ++k) out[k] = ok ? H[k] : 0.0;
  *nmod = ok ? 1 : 0;
}

__global__ __launch_bounds__(kFourT) void k_tv_h4(uint64_t seed, int64_t t0, int32_t nb, int32_t n, RpPts p, double* __restrict__ models,
                                                   int32_t* __restrict__ nmod) {
  const int32_t i = (int32_t)blockIdx.x * kFourT + (int32_t)threadIdx.x;
  if (i >= nb) return;
  tv_h4_trial(seed, t0 + i, n, p, models + (size_t)i * 9, nmod + i);
}

// trial t of k_tv_t1
__device__ __forceinline__ void tv_t1_trial(uint64_t seed, int64_t t, int32_t n, const RpPts& p, double* __restrict__ out, int32_t* __restrict__ nmod) {
  int32_t idx[1];
  lo_sample<1>(seed, t, n, idx);
  out[0] = p.u2[idx[0]] - p.u1[idx[0]];
  out[1] = p.v2[idx[0]] - p.v1[idx[0]];
  *nmod = 1;
}

__global__ __launch_bounds__(kLoT) void k_tv_t1(uint64_t seed, int64_t t0, int32_t nb, int32_t n, RpPts p, double* __restrict__ models,
                                                 int32_t* __restrict__ nmod) {
  const int32_t i = (int32_t)blockIdx.x * kLoT + (int32_t)threadIdx.x;
  if (i >= nb) return;
  tv_t1_trial(seed, t0 + i, n, p, models + 2 * (size_t)i, nmod + i);
}

template <bool kHomography>
__device__ __forceinline__ double tv_residual(const double* M, double u1, double v1, double u2, double v2) {
  if constexpr (kHomography) return tv_h_residual(M, u1, v1, u2, v2);
  else return rp_sampson(M, u1, v1, u2, v2);
}

template <bool kHomography>
__device__ __forceinline__ void tv_moments_block(const double* M, double thr2, int32_t n, const RpPts& p, int32_t nblk, double* __restrict__ part) {
  double acc[kMomK] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int32_t i = (int32_t)blockIdx.x * kLoT + (int32_t)threadIdx.x; i < n; i += nblk * kLoT) {
    const double u1 = p.u1[i], v1 = p.v1[i], u2 = p.u2[i], v2 = p.v2[i];
    if (!(tv_residual<kHomography>(M, u1, v1, u2, v2) <= thr2)) continue;
    acc[0] += 1.0; acc[1] += u1; acc[2] += v1; acc[3] += u2; acc[4] += v2;
  }
  block_reduce_rows<kMomK>(acc, part);
}

template <bool kHomography>
__global__ __launch_bounds__(kLoT) void k_tv_moments(TvModel M, double thr2, int32_t n, RpPts p, double* __restrict__ part) {
  tv_moments_block<kHomography>(M.m, thr2, n, p, (int32_t)gridDim.x, part);
}

struct TvCentre { double c1x, c1y, c2x, c2y; };

template <bool kHomography>
__device__ __forceinline__ void tv_gram_block(const double* M, double thr2, int32_t n, const RpPts& p, const TvCentre& c, int32_t nblk,
                                              double* __restrict__ part) {
  double acc[kGram9K];
#pragma unroll
  for (int k = 0; k < kGram9K; ++k) acc[k] = 0.0;
  for (int32_t i = (int32_t)blockIdx.x * kLoT + (int32_t)threadIdx.x; i < n; i += nblk * kLoT) {
    const double u1 = p.u1[i], v1 = p.v1[i], u2 = p.u2[i], v2 = p.v2[i];
    if (!(tv_residual<kHomography>(M, u1, v1, u2, v2) <= thr2)) continue;
    const double x1 = u1 - c.c1x, y1 = v1 - c.c1y, x2 = u2 - c.c2x, y2 = v2 - c.c2y;
    if constexpr (kHomography) {
      double a[9], b[9];
      tv_h_rows(x1, y1, x2, y2, a, b);
      int k = 0;
#pragma unroll
      for (int r = 0; r < 9; ++r)
#pragma unroll
        for (int cc = r; cc < 9; ++cc) acc[k++] += a[r] * a[cc] + b[r] * b[cc];
    } else {
      double q[9];
      rp_q_row(x1, y1, x2, y2, q);
      int k = 0;
#pragma unroll
      for (int r = 0; r < 9; ++r)
#pragma unroll
        for (int cc = r; cc < 9; ++cc) acc[k++] += q[r] * q[cc];
    }
  }
  block_reduce_rows<kGram9K>(acc, part);
}

template <bool kHomography>
__global__ __launch_bounds__(kLoT) void k_tv_gram(TvModel M, double thr2, int32_t n, RpPts p, TvCentre c, double* __restrict__ part) {
  tv_gram_block<kHomography>(M.m, thr2, n, p, c, (int32_t)gridDim.x, part);
}

__device__ __forceinline__ void tv_tsum_block(const double* t, double thr2, int32_t n, const RpPts& p, int32_t nblk, double* __restrict__ part) {
  double acc[kTsumK] = {0.0, 0.0, 0.0};
  for (int32_t i = (int32_t)blockIdx.x * kLoT + (int32_t)threadIdx.x; i < n; i += nblk * kLoT) {
    const double dx = p.u2[i] - p.u1[i], dy = p.v2[i] - p.v1[i];
    const double ex = dx - t[0], ey = dy - t[1];
    if (!(ex * ex + ey * ey <= thr2)) continue;
    acc[0] += 1.0; acc[1] += dx; acc[2] += dy;
  }
  block_reduce_rows<kTsumK>(acc, part);
}

__global__ __launch_bounds__(kLoT) void k_tv_tsum(LoModel<2> M, double thr2, int32_t n, RpPts p, double* __restrict__ part) {
  tv_tsum_block(M.m, thr2, n, p, (int32_t)gridDim.x, part);
}

struct TvCands {
  double P[4][12];       // [R | t] row-major
  double C2[4][3];       // -R^T t
  double max_depth[4];   // 1000 |t|
  int32_t ncand;
};

// CheckCheirality of every candidate on the chosen inliers (normalised points): per workgroup the number of inliers
// triangulated in front of both cameras, and per (candidate, match) CalculateTriangulationAngle of that point with
// projection centres 0 and -R^T t (-1 where the match is not chosen or fails the depth test)
__device__ __forceinline__ void tv_pose_block(const TvCands& c, int32_t n, const RpPts& p, const uint8_t* __restrict__ mask, int32_t nblk,
                                              int32_t* __restrict__ part, double* __restrict__ angle /* [4][n] */) {
  int cnt[4] = {0, 0, 0, 0};
  for (int32_t i = (int32_t)blockIdx.x * kLoT + (int32_t)threadIdx.x; i < n; i += nblk * kLoT) {
    const bool on = mask[i] != 0;
    TriView a{}, b{};
    a.P[0] = 1.0; a.P[5] = 1.0; a.P[10] = 1.0;
    a.xn[0] = p.u1[i]; a.xn[1] = p.v1[i];
    b.xn[0] = p.u2[i]; b.xn[1] = p.v2[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      double ang = -1.0;
      if (on && k < c.ncand) {
#pragma unroll
        for (int e = 0; e < 12; ++e) b.P[e] = c.P[k][e];
        double X[3];
        tri_two_view(a, b, X);
        const double d1 = X[2], d2 = tri_depth(b.P, X);
        if (d1 > DBL_EPSILON && d1 < c.max_depth[k] && d2 > DBL_EPSILON && d2 < c.max_depth[k]) {
          cnt[k] += 1;
          const double C1[3] = {0.0, 0.0, 0.0};
          ang = tri_angle(C1, c.C2[k], X);
        }
      }
      angle[(size_t)k * n + i] = ang;
    }
  }
  block_reduce_rows<4>(cnt, part);
}

__global__ __launch_bounds__(kLoT) void k_tv_pose(TvCands c, int32_t n, RpPts p, const uint8_t* __restrict__ mask, int32_t* __restrict__ part,
                                                   double* __restrict__ angle) {
  tv_pose_block(c, n, p, mask, (int32_t)gridDim.x, part, angle);
}

// ---- the problem descriptions of lo_ransac.h ---------------------------------------------------------------------------
// F (kHomography = false) and H (true) on pixel coordinates
template <bool kHomography>
struct TvProblem {
  static constexpr int kSample = kHomography ? kTvHSample : kTvFSample, kModel = 9;
  static constexpr int kSlots = kHomography ? 1 : kTvFMaxModels, kLocal = 1;
  static constexpr int kDefaultBatch = kHomography ? kTvHBatch : kTvFBatch;
  using Pts = RpPts;
  struct Obs { double u1, v1, u2, v2; };
  static __device__ __forceinline__ Obs load(const Pts& p, int32_t i) { return {p.u1[i], p.v1[i], p.u2[i], p.v2[i]}; }
  static __device__ __forceinline__ double residual(const double* M, const Obs& o) { return tv_residual<kHomography>(M, o.u1, o.v1, o.u2, o.v2); }

  int32_t n = 0;
  double thr2 = 0.0;
  Pts pts{};
  int npx = 0;  // reduction workgroups
  double* d_part = nullptr;
  std::vector<double> h_part;

  void minimal(hipStream_t st, uint64_t seed, int64_t t0, int32_t nb, double* models, int32_t* nmod) const {
    if constexpr (kHomography)
      hipLaunchKernelGGL(k_tv_h4, dim3((unsigned)((nb + kFourT - 1) / kFourT)), dim3(kFourT), 0, st, seed, t0, nb, n, pts, models, nmod);
    else
      hipLaunchKernelGGL(k_tv_f7, dim3((unsigned)((nb + kSevenT - 1) / kSevenT)), dim3(kSevenT), 0, st, seed, t0, nb, n, pts, models, nmod);
  }

  // the host half of the local estimator, from the summed rows of k_tv_moments and k_tv_gram: whether the inliers are enough
  // for the Gram stage, the centre that stage subtracts, and the model (RpProblem::local_models' signature)
  static bool enough(const double mom[kMomK]) { return !(mom[0] < (kHomography ? 4.0 : 8.0)); }
  static TvCentre centre(const double mom[kMomK]) { return {mom[1] / mom[0], mom[2] / mom[0], mom[3] / mom[0], mom[4] / mom[0]}; }
  static int local_models(const double mom[kMomK], const double g[kGram9K], double* out) {
    const bool ok = kHomography ? tv_homography_from_gram(mom, g, out) : tv_eight_point_from_gram(mom, g, out);
    return ok ? 1 : 0;
  }

  // the eight-point estimator / the normalised DLT on the inliers of Min: moments, then the centred Gram matrix
  int local(CallScope& A, const double* Min, double* out, int& nm) {
    nm = 0;
    TvModel m;
    std::memcpy(m.m, Min, sizeof(m.m));
    if (int rc = A.begin()) return rc;
    hipLaunchKernelGGL(k_tv_moments<kHomography>, dim3((unsigned)npx), dim3(kLoT), 0, A.st, m, thr2, n, pts, d_part);
    MPSFM_TRY(hipGetLastError());
    MPSFM_TRY(hipMemcpyAsync(h_part.data(), d_part, sizeof(double) * kMomK * (size_t)npx, hipMemcpyDeviceToHost, A.st));
    if (int rc = A.end()) return rc;
    double mom[kMomK];
    sum_rows(h_part.data(), npx, kMomK, mom);
    if (!enough(mom)) return 0;
    const TvCentre c = centre(mom);
    if (int rc = A.begin()) return rc;
    hipLaunchKernelGGL(k_tv_gram<kHomography>, dim3((unsigned)npx), dim3(kLoT), 0, A.st, m, thr2, n, pts, c, d_part);
    MPSFM_TRY(hipGetLastError());
    MPSFM_TRY(hipMemcpyAsync(h_part.data(), d_part, sizeof(double) * kGram9K * (size_t)npx, hipMemcpyDeviceToHost, A.st));
    if (int rc = A.end()) return rc;
    double g[kGram9K];
    sum_rows(h_part.data(), npx, kGram9K, g);
    nm = local_models(mom, g, out);
    return 0;
  }
};

// the 2-D translation of the watermark test: model t, residual |x2 - x1 - t|^2, sample size 1, the mean on the inliers
struct TvTranslation {
  static constexpr int kSample = 1, kModel = 2, kSlots = 1, kLocal = 1, kDefaultBatch = kTvTBatch;
  using Pts = RpPts;
  struct Obs { double dx, dy; };
  static __device__ __forceinline__ Obs load(const Pts& p, int32_t i) { return {p.u2[i] - p.u1[i], p.v2[i] - p.v1[i]}; }
  static __device__ __forceinline__ double residual(const double* t, const Obs& o) {
    const double ex = o.dx - t[0], ey = o.dy - t[1];
    return ex * ex + ey * ey;
  }

  int32_t n = 0;
  double thr2 = 0.0;
  Pts pts{};
  int npx = 0;
  double* d_part = nullptr;
  std::vector<double> h_part;

  void minimal(hipStream_t st, uint64_t seed, int64_t t0, int32_t nb, double* models, int32_t* nmod) const {
    hipLaunchKernelGGL(k_tv_t1, dim3((unsigned)((nb + kLoT - 1) / kLoT)), dim3(kLoT), 0, st, seed, t0, nb, n, pts, models, nmod);
  }

  // the mean of the inliers from the summed k_tv_tsum row (RpProblem::local_models' signature)
  static int local_models(const double* /* moments */, const double s[kTsumK], double* out) {
    if (s[0] < 1.0) return 0;
    out[0] = s[1] / s[0];
    out[1] = s[2] / s[0];
    return 1;
  }

  int local(CallScope& A, const double* tin, double* out, int& nm) {
    nm = 0;
    LoModel<2> m{{tin[0], tin[1]}};
    if (int rc = A.begin()) return rc;
    hipLaunchKernelGGL(k_tv_tsum, dim3((unsigned)npx), dim3(kLoT), 0, A.st, m, thr2, n, pts, d_part);
    MPSFM_TRY(hipGetLastError());
    MPSFM_TRY(hipMemcpyAsync(h_part.data(), d_part, sizeof(double) * kTsumK * (size_t)npx, hipMemcpyDeviceToHost, A.st));
    if (int rc = A.end()) return rc;
    double s[kTsumK];
    sum_rows(h_part.data(), npx, kTsumK, s);
    nm = local_models(nullptr, s, out);
    return 0;
  }
};

// a problem over the SoA block d (u1 v1 u2 v2, n each) with its reduction buffers
template <class P>
int tv_setup(P& prob, CallScope& A, const double* d, int32_t n, double thr2, int part_k) {
  prob.n = n;
  prob.thr2 = thr2;
  prob.npx = lo_blocks(n, kLoT);
  prob.pts = RpPts{d, d + n, d + 2 * (size_t)n, d + 3 * (size_t)n};
  prob.d_part = A.alloc<double>((size_t)part_k * prob.npx);
  if (!prob.d_part) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  prob.h_part.resize((size_t)part_k * prob.npx);
  return 0;
}

void tv_fill_leg(mpsfm_two_view_leg& leg, const LoReport& rep, int sample) {
  leg.num_inliers = rep.best.num_inliers;
  leg.num_trials = rep.num_trials;
  leg.max_num_trials = rep.max_num_trials;
  leg.lo_rounds = rep.lo_rounds;
  leg.num_batches = rep.num_batches;
  leg.success = rep.best.num_inliers >= sample ? 1 : 0;
}

bool tv_options_valid(const mpsfm_two_view_options& o) {
  auto unit = [](double v) { return v >= 0.0 && v <= 1.0; };
  return lo_options_valid(o.ransac) && o.min_num_inliers >= 0 && unit(o.min_E_F_inlier_ratio) && unit(o.max_H_inlier_ratio) &&
         o.watermark_min_inlier_ratio > 0.0 && o.watermark_min_inlier_ratio <= 1.0 && o.watermark_border_size >= 0.0 &&
         o.watermark_border_size <= 0.5 && (o.detect_watermark == 0 || o.detect_watermark == 1) &&
         (o.compute_relative_pose == 0 || o.compute_relative_pose == 1);
}

// ---- the host stages both entry points share ---------------------------------------------------------------------------
// EstimateCalibratedTwoViewGeometry's decision: the config and the leg whose mask is chosen (0 E, 1 F, 2 H; -1: none)
void tv_decide(const mpsfm_two_view_options& o, bool okE, bool okF, bool okH, int64_t nE, int64_t nF, int64_t nH, int& config, int& chosen) {
  const int64_t minI = o.min_num_inliers;
  const double E_F = (double)nE / (double)nF, H_F = (double)nH / (double)nF, H_E = (double)nH / (double)nE;
  config = MPSFM_TVG_DEGENERATE;
  chosen = -1;
  if ((!okE && !okF && !okH) || (nE < minI && nF < minI && nH < minI)) {
    config = MPSFM_TVG_DEGENERATE;
  } else if (okE && E_F > o.min_E_F_inlier_ratio && nE >= minI) {
    chosen = nE >= nF ? 0 : 1;
    const int64_t best = std::max(nE, nF);
    if (H_E > o.max_H_inlier_ratio) {
      config = MPSFM_TVG_PLANAR_OR_PANORAMIC;
      if (nH > best) chosen = 2;
    } else {
      config = MPSFM_TVG_CALIBRATED;
    }
  } else if (okF && nF >= minI) {
    chosen = 1;
    if (H_F > o.max_H_inlier_ratio) {
      config = MPSFM_TVG_PLANAR_OR_PANORAMIC;
      if (nH > nF) chosen = 2;
    } else {
      config = MPSFM_TVG_UNCALIBRATED;
    }
  } else if (okH && nH >= minI) {
    chosen = 2;
    config = MPSFM_TVG_PLANAR_OR_PANORAMIC;
  }
}

// DetectWatermark's selection: the chosen inliers (sel) outside the border box in both images; hpx: the SoA pixel block of the pair
void tv_border(const mpsfm_two_view_options& o, const double* hpx, int32_t n, const uint8_t* sel, const int32_t* size1, const int32_t* size2,
               std::vector<int32_t>& border) {
  const double b1 = o.watermark_border_size * std::sqrt((double)size1[0] * size1[0] + (double)size1[1] * size1[1]);
  const double b2 = o.watermark_border_size * std::sqrt((double)size2[0] * size2[0] + (double)size2[1] * size2[1]);
  auto inside = [](double x, double y, double b, const int32_t* s) { return x >= b && x <= s[0] - b && y >= b && y <= s[1] - b; };
  border.clear();
  for (int32_t i = 0; i < n; ++i)
    if (sel[i] && !inside(hpx[i], hpx[(size_t)n + i], b1, size1) && !inside(hpx[2 * (size_t)n + i], hpx[3 * (size_t)n + i], b2, size2))
      border.push_back(i);
}

// EstimateTwoViewGeometryPose's candidates: the four of E (CALIBRATED), of K2^T F K1 (UNCALIBRATED) or of the homography
void tv_pose_cands(int config, const double* E, const double* F, const double* H, const double* intr1, const double* intr2, TvCands& cand) {
  if (config == MPSFM_TVG_CALIBRATED || config == MPSFM_TVG_UNCALIBRATED) {
    double Em[9];
    if (config == MPSFM_TVG_CALIBRATED) {
      std::memcpy(Em, E, sizeof(Em));
    } else {  // K2^T F K1
      const double K1[9] = {intr1[0], 0.0, intr1[2], 0.0, intr1[1], intr1[3], 0.0, 0.0, 1.0};
      const double K2t[9] = {intr2[0], 0.0, 0.0, 0.0, intr2[1], 0.0, intr2[2], intr2[3], 1.0};
      double T[9];
      tv_mat3_mul(K2t, F, T);
      tv_mat3_mul(T, K1, Em);
      rp_canonical(Em);
    }
    double R1[9], R2[9], t[3];
    rp_decompose(Em, R1, R2, t);
    cand.ncand = 4;
    for (int k = 0; k < 4; ++k) {
      const double* R = (k % 2 == 0) ? R1 : R2;
      const double sg = k < 2 ? 1.0 : -1.0;
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) cand.P[k][4 * r + c] = R[3 * r + c];
        cand.P[k][4 * r + 3] = sg * t[r];
      }
    }
  } else {
    double R[4][9], t[4][3], dev = 0.0;
    cand.ncand = tv_decompose_homography(H, intr1, intr2, R, t, &dev);
    for (int k = 0; k < cand.ncand; ++k)
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) cand.P[k][4 * r + c] = R[k][3 * r + c];
        cand.P[k][4 * r + 3] = t[k][r];
      }
  }
  for (int k = 0; k < cand.ncand; ++k) {
    const double* P = cand.P[k];
    const double t[3] = {P[3], P[7], P[11]};
    for (int c = 0; c < 3; ++c) cand.C2[k][c] = -(P[c] * t[0] + P[4 + c] * t[1] + P[8 + c] * t[2]);
    cand.max_depth[k] = 1000.0 * std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
  }
}

// the candidate with the most cheirality points; the later candidate wins a tie
int tv_pose_winner(const TvCands& cand, const int64_t* count, int64_t& bestc) {
  bestc = -1;
  int bk = 0;
  for (int k = 0; k < cand.ncand; ++k)
    if (count[k] >= bestc) { bestc = count[k]; bk = k; }
  return bk;
}

// the winner's pose, the median of its triangulation angles (ang: its angle row, consumed) and PLANAR / PANORAMIC
void tv_pose_finish(mpsfm_two_view_result& result, const TvCands& cand, int bk, int64_t bestc, std::vector<double>& ang, bool from_E, int& config) {
  ang.erase(std::remove_if(ang.begin(), ang.end(), [](double a) { return a < 0.0; }), ang.end());
  std::sort(ang.begin(), ang.end());
  const size_t m = ang.size();
  result.tri_angle = m == 0 ? 0.0 : (m % 2 ? ang[m / 2] : 0.5 * (ang[m / 2 - 1] + ang[m / 2]));
  std::memcpy(result.cam2_from_cam1, cand.P[bk], sizeof(cand.P[bk]));
  result.num_cheirality_points = bestc;
  if (!from_E) {
    const double* P = cand.P[bk];
    config = (P[3] == 0.0 && P[7] == 0.0 && P[11] == 0.0) ? MPSFM_TVG_PANORAMIC : MPSFM_TVG_PLANAR;
    if (config == MPSFM_TVG_PANORAMIC) result.tri_angle = 0.0;
  }
}

// nullptr, or what is wrong with the cameras of a pair
const char* tv_cameras_invalid(const double* intr1, const double* intr2, const int32_t* size1, const int32_t* size2) {
  for (const double* K : {intr1, intr2})
    if (!finite_all(K, 4) || K[0] == 0.0 || K[1] == 0.0 || K[0] + K[1] == 0.0) return "intrinsics must be finite with non-zero focal lengths";
  if (size1[0] <= 0 || size1[1] <= 0 || size2[0] <= 0 || size2[1] <= 0) return "image sizes must be positive";
  return nullptr;
}
}  // namespace

}  // namespace mpsfm
