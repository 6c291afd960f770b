// The relative-pose problem of lo_ransac.h, shared by rel_pose.hip (mpsfm_rel_pose_estimate) and two_view.hip (the E leg of
// mpsfm_two_view_geometry): the minimal-solver kernel, the local estimator's reduction, the cheirality pass and RpProblem.
// The kernels have internal linkage (unnamed namespace): each translation unit that includes this header carries its own
// copy of them, compiled from the same text.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "rel_pose_math.h"
#include "tri_math.h"
#include "lo_ransac.h"

namespace mpsfm {

namespace {
constexpr int kT = kLoT;
constexpr int kFiveT = 32;          // trials per k_rp_five workgroup: 32 x RP_WORK doubles = 59 KiB of LDS
constexpr int kGramK = 46;          // count, then the upper triangle of Q^T Q row-major

struct RpPts { const double *u1, *v1, *u2, *v2; };

// The kernels below and their batched forms (two_view_batch.hip) are two callers of one body each.  A body takes what its
// callers read from their arguments or from a descriptor row: the trial, or the number nblk of workgroups along the problem's
// observations (its own workgroup is blockIdx.x, as in block_reduce_rows), the points, the model and the output pointers,
// already at the problem's rows.

// Trial t of k_rp_five, by thread threadIdx.x of a workgroup of kFiveT: the five-index sample and the five-point solver in the
// thread's LDS slice; up to kRpMaxModels models at out (zeros pad) and their number.  flatten: wherever two kernels of one
// translation unit call this body the solver's stages have two callers, and the inliner would otherwise leave them as calls
// with their arrays in scratch.
__device__ __forceinline__ __attribute__((flatten)) void rp_five_trial(uint64_t seed, int64_t t, int32_t n, const RpPts& p, double* __restrict__ out,
                                                                       int32_t* __restrict__ nmod) {
  __shared__ double work[kFiveT * RP_WORK];
  int32_t idx[kRpSample];
  lo_sample<kRpSample>(seed, t, n, idx);
  double u1[kRpSample], v1[kRpSample], u2[kRpSample], v2[kRpSample];
#pragma unroll
  for (int k = 0; k < kRpSample; ++k) { u1[k] = p.u1[idx[k]]; v1[k] = p.v1[idx[k]]; u2[k] = p.u2[idx[k]]; v2[k] = p.v2[idx[k]]; }
  const RpW w{work + threadIdx.x, kFiveT};
  int nm = 0;
  if (rp_nullspace5(u1, v1, u2, v2, w)) nm = rp_models_from_nullspace(w, out);
  for (int k = 9 * nm; k < 9 * kRpMaxModels; ++k) out[k] = 0.0;
  *nmod = nm;
}

__global__ __launch_bounds__(kFiveT) void k_rp_five(uint64_t seed, int64_t t0, int32_t nb, int32_t n, RpPts p, double* __restrict__ models,
                                                     int32_t* __restrict__ nmod) {
  const int32_t i = (int32_t)blockIdx.x * kFiveT + (int32_t)threadIdx.x;
  if (i >= nb) return;
  rp_five_trial(seed, t0 + i, n, p, models + (size_t)i * 9 * kRpMaxModels, nmod + i);
}

using RpModel = LoModel<9>;

// k_rp_gram: count and Q^T Q of the inliers of E among the workgroup's observations -> its row of part
__device__ __forceinline__ void rp_gram_block(const double* E, double thr2, int32_t n, const RpPts& p, int32_t nblk, double* __restrict__ part) {
  double acc[kGramK];
#pragma unroll
  for (int k = 0; k < kGramK; ++k) acc[k] = 0.0;
  for (int32_t i = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x; i < n; i += nblk * kT) {
    const double u1 = p.u1[i], v1 = p.v1[i], u2 = p.u2[i], v2 = p.v2[i];
    if (!(rp_sampson(E, u1, v1, u2, v2) <= thr2)) continue;
    double q[9];
    rp_q_row(u1, v1, u2, v2, q);
    acc[0] += 1.0;
    int k = 1;
#pragma unroll
    for (int r = 0; r < 9; ++r)
#pragma unroll
      for (int c = r; c < 9; ++c) acc[k++] += q[r] * q[c];
  }
  block_reduce_rows<kGramK>(acc, part);
}

__global__ __launch_bounds__(kT) void k_rp_gram(RpModel Ein, double thr2, int32_t n, RpPts p, double* __restrict__ part) {
  rp_gram_block(Ein.m, thr2, n, p, (int32_t)gridDim.x, part);
}

struct RpCands { double P[4][12]; double max_depth[4]; };

// CheckCheirality of the four candidates: per workgroup the number of inliers triangulated in front of both cameras
__global__ __launch_bounds__(kT) void k_rp_cheirality(RpCands c, int32_t n, RpPts p, const uint8_t* __restrict__ mask,
                                                       int32_t* __restrict__ part) {
  int cnt[4] = {0, 0, 0, 0};
  for (int32_t i = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x; i < n; i += (int32_t)gridDim.x * kT) {
    if (!mask[i]) continue;
    TriView a{}, b{};
    a.P[0] = 1.0; a.P[5] = 1.0; a.P[10] = 1.0;
    a.xn[0] = p.u1[i]; a.xn[1] = p.v1[i];
    b.xn[0] = p.u2[i]; b.xn[1] = p.v2[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int e = 0; e < 12; ++e) b.P[e] = c.P[k][e];
      double X[3];
      tri_two_view(a, b, X);
      const double d1 = X[2], d2 = tri_depth(b.P, X);
      if (d1 > DBL_EPSILON && d1 < c.max_depth[k] && d2 > DBL_EPSILON && d2 < c.max_depth[k]) cnt[k] += 1;
    }
  }
  block_reduce_rows<4>(cnt, part);
}

// the problem description of lo_ransac.h
struct RpProblem {
  static constexpr int kSample = kRpSample, kModel = 9, kSlots = kRpMaxModels, kLocal = kRpMaxModels;
  static constexpr int kDefaultBatch = 4096;  // trials per batch
  using Pts = RpPts;
  struct Obs { double u1, v1, u2, v2; };
  static __device__ __forceinline__ Obs load(const Pts& p, int32_t i) { return {p.u1[i], p.v1[i], p.u2[i], p.v2[i]}; }
  static __device__ __forceinline__ double residual(const double* E, const Obs& o) { return rp_sampson(E, o.u1, o.v1, o.u2, o.v2); }

  int32_t n = 0;
  double thr2 = 0.0;
  Pts pts{};
  int npx = 0;  // reduction workgroups
  double* d_part = nullptr;
  std::vector<double> h_part;

  void minimal(hipStream_t st, uint64_t seed, int64_t t0, int32_t nb, double* models, int32_t* nmod) const {
    hipLaunchKernelGGL(k_rp_five, dim3((unsigned)((nb + kFiveT - 1) / kFiveT)), dim3(kFiveT), 0, st, seed, t0, nb, n, pts, models, nmod);
  }

  // the host half of the local estimator (one signature for every problem of the two-view legs; this one has no moments
  // stage): the summed k_rp_gram row -> the models of the nullspace of Q^T Q, and their number
  static int local_models(const double* /* moments */, const double g[kGramK], double* out) {
    if (g[0] < kRpSample) return 0;
    double G[9][9], V[9][9], ev[9];
    for (int r = 0, k = 1; r < 9; ++r)
      for (int c = r; c < 9; ++c, ++k) G[r][c] = G[c][r] = g[k];
    sym_eig<9>(G, V, ev);  // ascending
    if (!(ev[4] > kRpRankTol * kRpRankTol * ev[8])) return 0;
    double work[RP_WORK];
    const RpW w{work, 1};
    for (int k = 0; k < 4; ++k)
      for (int i = 0; i < 9; ++i) w[RP_N + 9 * k + i] = V[i][3 - k];
    return rp_models_from_nullspace(w, out);
  }

  // EssentialMatrixFivePointEstimator::Estimate on the inliers of Ein (n > 5: the nullspace of Q^T Q): up to 10 models
  int local(CallScope& A, const double* Ein, double* out, int& nm) {
    nm = 0;
    RpModel m;
    std::memcpy(m.m, Ein, sizeof(m.m));
    if (int rc = A.begin()) return rc;
    hipLaunchKernelGGL(k_rp_gram, dim3((unsigned)npx), dim3(kT), 0, A.st, m, thr2, n, pts, d_part);
    MPSFM_TRY(hipGetLastError());
    MPSFM_TRY(hipMemcpyAsync(h_part.data(), d_part, sizeof(double) * kGramK * (size_t)npx, hipMemcpyDeviceToHost, A.st));
    if (int rc = A.end()) return rc;
    double g[kGramK];
    sum_rows(h_part.data(), npx, kGramK, g);
    nm = local_models(nullptr, g, out);
    return 0;
  }
};
}  // namespace

}  // namespace mpsfm
