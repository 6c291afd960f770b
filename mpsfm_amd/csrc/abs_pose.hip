// Absolute-pose LO-RANSAC of one 2D-3D problem (mpsfm_abs_pose_estimate; semantics, sampler recipe and what is unpinned:
// include/mpsfm_hip.h).  The loop, the scoring kernels and the batch tables are lo_ransac.h's; this file describes the
// problem to it:
//   k_ap_p3p          one thread per trial of a batch: the trial's counter-based sample, P3P, up to 4 models (zeros pad)
//   ApProblem::local  EPnP on the current inlier set: its O(N) passes on the device as fixed-order reductions
//                     (k_ap_pass<1..5>: centroid, scatter, M^T M, the alignment sums of the three beta solutions, their
//                     reprojection sums) and its constant-size algebra on the host (abs_pose_math.h)
// and normalises the PINHOLE inputs and fills the result.  f64 throughout.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "abs_pose_math.h"
#include "common.h"
#include "lo_ransac.h"

namespace mpsfm {

namespace {
constexpr int kT = kLoT;
constexpr int kWaves = kLoWaves;

struct ApPts { const double *X, *Y, *Z, *u, *v; };

__global__ __launch_bounds__(kT) void k_ap_p3p(uint64_t seed, int64_t t0, int32_t nb, int32_t n, ApPts p, double* __restrict__ models,
                                                int32_t* __restrict__ nmod) {
  const int32_t i = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  if (i >= nb) return;
  int32_t idx[3];
  lo_sample<3>(seed, t0 + i, n, idx);
  double x[3][2], X[3][3];
  for (int k = 0; k < 3; ++k) {
    x[k][0] = p.u[idx[k]]; x[k][1] = p.v[idx[k]];
    X[k][0] = p.X[idx[k]]; X[k][1] = p.Y[idx[k]]; X[k][2] = p.Z[idx[k]];
  }
  double* out = models + (size_t)i * 48;
  const int nm = ap_p3p(x, X, out);  // straight into the table: a private array indexed by the model count would live in scratch
  for (int k = 12 * nm; k < 48; ++k) out[k] = 0.0;  // a zero model puts every point at depth 0: no inliers
  nmod[i] = nm;
}

// EPnP passes over the inliers of Pin (residual <= thr2)
struct ApPassArgs {
  double Pin[12];
  double thr2;
  ApEpnpFrame F;
  double ccs[3][4][3];  // pass 4: the three beta solutions' camera-frame control points
  double P3[3][12];     // pass 5: the three candidate models
};
template <int PASS> struct ApPassK;
template <> struct ApPassK<1> { static constexpr int K = 4; };   // count, sum X
template <> struct ApPassK<2> { static constexpr int K = 6; };   // sum (X - c0)(X - c0)^T, upper
template <> struct ApPassK<3> { static constexpr int K = 78; };  // M^T M, upper, row-major
template <> struct ApPassK<4> { static constexpr int K = 39; };  // sum d, then per solution sum pc, sum pc d^T
template <> struct ApPassK<5> { static constexpr int K = 3; };   // per solution sum sqrt(residual)

template <int PASS>
__global__ __launch_bounds__(kT) void k_ap_pass(ApPassArgs a, int32_t n, ApPts p, double* __restrict__ part, int32_t* __restrict__ first) {
  constexpr int K = ApPassK<PASS>::K;
  __shared__ int red_first[kWaves];
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
  int lo = INT32_MAX;
  for (int32_t i = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x; i < n; i += (int32_t)gridDim.x * kT) {
    const double X = p.X[i], Y = p.Y[i], Z = p.Z[i], u = p.u[i], v = p.v[i];
    if (!(ap_residual(a.Pin, X, Y, Z, u, v) <= a.thr2)) continue;
    if (PASS == 1) {
      lo = min(lo, (int)i);
      acc[0] += 1.0; acc[1] += X; acc[2] += Y; acc[3] += Z;
    } else if (PASS == 2) {
      const double d0 = X - a.F.cws[0][0], d1 = Y - a.F.cws[0][1], d2 = Z - a.F.cws[0][2];
      acc[0] += d0 * d0; acc[1] += d0 * d1; acc[2] += d0 * d2; acc[3] += d1 * d1; acc[4] += d1 * d2; acc[5] += d2 * d2;
    } else if (PASS == 3) {
      double al[4], r1[12], r2[12];
      ap_alphas(a.F, X, Y, Z, al);
      ap_m_rows(al, u, v, r1, r2);
      int k = 0;
#pragma unroll
      for (int r = 0; r < 12; ++r)
#pragma unroll
        for (int c = r; c < 12; ++c) acc[k++] += r1[r] * r1[c] + r2[r] * r2[c];
    } else if (PASS == 4) {
      double al[4];
      ap_alphas(a.F, X, Y, Z, al);
      const double d[3] = {X - a.F.cws[0][0], Y - a.F.cws[0][1], Z - a.F.cws[0][2]};
      acc[0] += d[0]; acc[1] += d[1]; acc[2] += d[2];
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        double pc[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) pc[e] = al[0] * a.ccs[s][0][e] + al[1] * a.ccs[s][1][e] + al[2] * a.ccs[s][2][e] + al[3] * a.ccs[s][3][e];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          acc[3 + 12 * s + e] += pc[e];
#pragma unroll
          for (int f = 0; f < 3; ++f) acc[3 + 12 * s + 3 + 3 * e + f] += pc[e] * d[f];
        }
      }
    } else {
#pragma unroll
      for (int s = 0; s < 3; ++s) acc[s] += sqrt(ap_residual(a.P3[s], X, Y, Z, u, v));
    }
  }
  if (PASS == 1) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) lo = min(lo, __shfl_xor(lo, off, 64));
    if (threadIdx.x % 64 == 0) red_first[threadIdx.x / 64] = lo;
  }
  block_reduce_rows<K>(acc, part);  // its barrier publishes red_first too
  if (PASS == 1 && threadIdx.x == 0) {
    int m = INT32_MAX;
    for (int w = 0; w < kWaves; ++w) m = min(m, red_first[w]);
    first[blockIdx.x] = m;
  }
}

// the problem description of lo_ransac.h
struct ApProblem {
  static constexpr int kSample = 3, kModel = 12, kSlots = 4, kLocal = 1;
  static constexpr int kDefaultBatch = 256;  // trials per batch
  using Pts = ApPts;
  struct Obs { double X, Y, Z, u, v; };
  static __device__ __forceinline__ Obs load(const Pts& p, int32_t i) { return {p.X[i], p.Y[i], p.Z[i], p.u[i], p.v[i]}; }
  static __device__ __forceinline__ double residual(const double* P, const Obs& o) { return ap_residual(P, o.X, o.Y, o.Z, o.u, o.v); }

  int32_t n = 0;
  double thr2 = 0.0;
  Pts pts{};
  const double* hs = nullptr;  // the host's copy of the points, SoA: X Y Z u v
  int npx = 0;                 // EPnP pass workgroups
  double* d_part = nullptr;
  int32_t* d_first = nullptr;
  std::vector<double> h_part;
  std::vector<int32_t> h_first;

  void minimal(hipStream_t st, uint64_t seed, int64_t t0, int32_t nb, double* models, int32_t* nmod) const {
    hipLaunchKernelGGL(k_ap_p3p, dim3((unsigned)((nb + kT - 1) / kT)), dim3(kT), 0, st, seed, t0, nb, n, pts, models, nmod);
  }

  // one EPnP pass: the workgroups' rows summed in order into out[K]
  template <int PASS>
  int pass(CallScope& A, const ApPassArgs& a, double* out) {
    constexpr int K = ApPassK<PASS>::K;
    if (int rc = A.begin()) return rc;
    hipLaunchKernelGGL(k_ap_pass<PASS>, dim3((unsigned)npx), dim3(kT), 0, A.st, a, n, pts, d_part, d_first);
    MPSFM_TRY(hipGetLastError());
    MPSFM_TRY(hipMemcpyAsync(h_part.data(), d_part, sizeof(double) * K * (size_t)npx, hipMemcpyDeviceToHost, A.st));
    if (PASS == 1) MPSFM_TRY(hipMemcpyAsync(h_first.data(), d_first, sizeof(int32_t) * (size_t)npx, hipMemcpyDeviceToHost, A.st));
    if (int rc = A.end()) return rc;
    sum_rows(h_part.data(), npx, K, out);
    return 0;
  }

  // EPNPEstimator::Estimate on the inliers of Pin; nm = 0: no model
  int local(CallScope& A, const double* Pin, double* Pout, int& nm) {
    nm = 0;
    auto hX = [&](int32_t i) { return hs[i]; };
    auto hY = [&](int32_t i) { return hs[(size_t)n + i]; };
    auto hZ = [&](int32_t i) { return hs[2 * (size_t)n + i]; };
    ApPassArgs a{};
    std::memcpy(a.Pin, Pin, sizeof(a.Pin));
    a.thr2 = thr2;
    double s1[4];
    if (int rc = pass<1>(A, a, s1)) return rc;
    const int64_t m = (int64_t)s1[0];
    if (m < 4) return 0;
    int32_t first = INT32_MAX;
    for (int b = 0; b < npx; ++b) first = std::min(first, h_first[(size_t)b]);
    const double c0[3] = {s1[1] / (double)m, s1[2] / (double)m, s1[3] / (double)m};
    for (int d = 0; d < 3; ++d) a.F.cws[0][d] = c0[d];
    double sc[6];
    if (int rc = pass<2>(A, a, sc)) return rc;
    if (!ap_epnp_frame(c0, sc, m, a.F)) return 0;
    double mtm[78];
    if (int rc = pass<3>(A, a, mtm)) return rc;
    double MtM[12][12], V[12][12], w[12];
    for (int r = 0, k = 0; r < 12; ++r)
      for (int c = r; c < 12; ++c, ++k) MtM[r][c] = MtM[c][r] = mtm[k];
    sym_eig<12>(MtM, V, w);
    double vs[4][12];
    for (int i = 0; i < 4; ++i)
      for (int k = 0; k < 12; ++k) vs[i][k] = V[k][i];
    ap_epnp_betas(vs, a.F, a.ccs);
    double al0[4];  // SolveForSign: the depth of the first inlier
    ap_alphas(a.F, hX(first), hY(first), hZ(first), al0);
    for (int s = 0; s < 3; ++s) {
      const double z0 = al0[0] * a.ccs[s][0][2] + al0[1] * a.ccs[s][1][2] + al0[2] * a.ccs[s][2][2] + al0[3] * a.ccs[s][3][2];
      if (z0 < 0)
        for (int j = 0; j < 4; ++j)
          for (int d = 0; d < 3; ++d) a.ccs[s][j][d] = -a.ccs[s][j][d];
    }
    double s4[39];
    if (int rc = pass<4>(A, a, s4)) return rc;
    for (int s = 0; s < 3; ++s) {  // EstimateRT
      const double* spc = s4 + 3 + 12 * s;
      const double* spcd = spc + 3;
      double pc0[3], pw0[3], S[3][3];
      for (int e = 0; e < 3; ++e) { pc0[e] = spc[e] / (double)m; pw0[e] = c0[e] + s4[e] / (double)m; }
      for (int wa = 0; wa < 3; ++wa)
        for (int cb = 0; cb < 3; ++cb) S[wa][cb] = spcd[3 * cb + wa] - spc[cb] * s4[wa] / (double)m;
      double R[9];
      ap_horn(S, R);
      for (int r = 0; r < 3; ++r) {
        a.P3[s][4 * r] = R[3 * r]; a.P3[s][4 * r + 1] = R[3 * r + 1]; a.P3[s][4 * r + 2] = R[3 * r + 2];
        a.P3[s][4 * r + 3] = pc0[r] - (R[3 * r] * pw0[0] + R[3 * r + 1] * pw0[1] + R[3 * r + 2] * pw0[2]);
      }
    }
    double err[3];
    if (int rc = pass<5>(A, a, err)) return rc;
    int bi = 0;
    if (err[1] < err[0]) bi = 1;
    if (err[2] < err[bi]) bi = 2;
    std::memcpy(Pout, a.P3[bi], sizeof(double) * 12);
    nm = 1;
    return 0;
  }
};
}  // namespace

}  // namespace mpsfm

using namespace mpsfm;

extern "C" int mpsfm_abs_pose_estimate(int64_t n64, const double* points2D, const double* points3D, const double* intr,
                                       const mpsfm_abs_pose_options* o, int32_t device, uint8_t* inlier_mask,
                                       mpsfm_abs_pose_result* result) {
  if (result) *result = mpsfm_abs_pose_result{};
  if (!points2D || !points3D || !intr || !o || !inlier_mask || !result) return fail(MPSFM_EINVAL, "NULL pointer");
  if (n64 < 3) return fail(MPSFM_EINVAL, "fewer than 3 correspondences");
  if (n64 > INT32_MAX) return fail(MPSFM_EINVAL, "more than INT32_MAX correspondences (int32 indexing)");
  const int32_t n = (int32_t)n64;
  if (!finite_all(points2D, 2 * (size_t)n) || !finite_all(points3D, 3 * (size_t)n)) return fail(MPSFM_EINVAL, "non-finite point");
  if (!finite_all(intr, 4) || intr[0] == 0.0 || intr[1] == 0.0 || intr[0] + intr[1] == 0.0)
    return fail(MPSFM_EINVAL, "intrinsics must be finite with non-zero focal lengths");
  if (!lo_options_valid(*o)) return fail(MPSFM_EINVAL, "invalid RANSAC options");
  if (int rc = open_device(device)) return rc;

  // EstimateAbsolutePose: CamFromImg and CamFromImgThreshold of the PINHOLE camera
  const double fx = intr[0], fy = intr[1], cx = intr[2], cy = intr[3];
  const double thr = o->max_error / ((fx + fy) / 2.0);
  const double thr2 = thr * thr;
  std::vector<double> hs((size_t)5 * n);  // SoA: X Y Z u v
  for (int32_t i = 0; i < n; ++i) {
    hs[i] = points3D[3 * (size_t)i];
    hs[(size_t)n + i] = points3D[3 * (size_t)i + 1];
    hs[2 * (size_t)n + i] = points3D[3 * (size_t)i + 2];
    hs[3 * (size_t)n + i] = (points2D[2 * (size_t)i] - cx) / fx;
    hs[4 * (size_t)n + i] = (points2D[2 * (size_t)i + 1] - cy) / fy;
  }

  CallScope A;
  if (int rc = A.open(true)) return rc;
  ApProblem prob;
  prob.n = n;
  prob.thr2 = thr2;
  prob.hs = hs.data();
  prob.npx = lo_blocks(n, kT);
  double* d_pts = A.alloc<double>(5 * (size_t)n);
  prob.d_part = A.alloc<double>(78 * (size_t)prob.npx);
  prob.d_first = A.alloc<int32_t>((size_t)prob.npx);
  uint8_t* d_mask = A.alloc<uint8_t>((size_t)n);
  if (!d_pts || !prob.d_part || !prob.d_first || !d_mask) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  MPSFM_TRY(hipMemcpyAsync(d_pts, hs.data(), sizeof(double) * 5 * (size_t)n, hipMemcpyHostToDevice, A.st));
  prob.pts = ApPts{d_pts, d_pts + n, d_pts + 2 * (size_t)n, d_pts + 3 * (size_t)n, d_pts + 4 * (size_t)n};
  prob.h_part.resize((size_t)78 * prob.npx);
  prob.h_first.resize((size_t)prob.npx);

  LoReport rep;
  double best_model[12] = {};
  if (int rc = lo_ransac(prob, A, *o, rep, best_model)) return rc;
  result->num_trials = rep.num_trials;
  result->max_num_trials = rep.max_num_trials;
  result->num_models = rep.num_models;
  result->lo_rounds = (int32_t)rep.lo_rounds;
  result->num_batches = (int32_t)rep.num_batches;
  if (rep.best.num_inliers < 3) {
    result->ms = (float)A.ms;
    std::memset(inlier_mask, 0, (size_t)n);
    return 0;
  }
  if (int rc = A.begin()) return rc;
  if (int rc = lo_mask(prob, A, best_model, d_mask)) return rc;
  MPSFM_TRY(hipMemcpyAsync(inlier_mask, d_mask, (size_t)n, hipMemcpyDeviceToHost, A.st));
  if (int rc = A.end()) return rc;
  std::memcpy(result->cam_from_world, best_model, sizeof(best_model));
  result->num_inliers = rep.best.num_inliers;
  result->success = 1;
  result->ms = (float)A.ms;
  return 0;
}
