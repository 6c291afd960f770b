// Absolute-pose LO-RANSAC of one 2D-3D problem (mpsfm_abs_pose_estimate; semantics, sampler recipe and what is unpinned:
// include/mpsfm_hip.h).  The sequential LORANSAC loop is replayed on the host over tables the device fills in batches:
//   k_ap_p3p         one thread per trial of a batch: the trial's counter-based sample, P3P, up to 4 models (zeros pad)
//   k_ap_score       a tile of kTile models in LDS against a grid-stride stream of points: per model inlier count and inlier
//                    residual sum of the workgroup, reduced in a fixed order (wave butterflies, then the waves in order)
//   k_ap_score_sum   one thread per model: the workgroups' partial rows in order -> count and sum (no float atomics: the
//                    table is bitwise identical run to run)
// The host walks the batch's table in trial order (best-model updates, the local optimisation, the dynamic bound, the
// stop rule), so the result is the sequential loop's.  EPnP (the local estimator) runs its O(N) passes on the device as
// fixed-order reductions over the current inlier set (k_ap_pass<1..5>: centroid, scatter, M^T M, the alignment sums of the
// three beta solutions, their reprojection sums) and its constant-size algebra on the host (abs_pose_math.h).
// f64 throughout.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "abs_pose_math.h"
#include "common.h"

namespace mpsfm {

extern thread_local std::string g_err;
static int apfail(int code, const std::string& m) { g_err = m; return code; }
#define AP_TRY(expr)                                                                                  \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess) return apfail(MPSFM_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

namespace {
constexpr int kT = 256;
constexpr int kWaves = kT / 64;
constexpr int kTile = 16;           // models per scoring workgroup
constexpr int kDefaultBatch = 256;  // trials per batch
constexpr int kMaxBatch = 1 << 16;

struct ApPts { const double *X, *Y, *Z, *u, *v; };

// workgroups of the reductions over the points: a function of N alone, so the summation order never changes
int ap_blocks(int32_t n, int per_block) { return (int)std::min<int64_t>(((int64_t)n + per_block - 1) / per_block, 64); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(kT) void k_ap_p3p(uint64_t seed, int64_t t0, int32_t nb, int32_t n, ApPts p, double* __restrict__ models,
                                                int32_t* __restrict__ nmod) {
  const int32_t i = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  if (i >= nb) return;
  int32_t idx[3];
  ap_sample(seed, t0 + i, n, idx);
  double x[3][2], X[3][3];
  for (int k = 0; k < 3; ++k) {
    x[k][0] = p.u[idx[k]]; x[k][1] = p.v[idx[k]];
    X[k][0] = p.X[idx[k]]; X[k][1] = p.Y[idx[k]]; X[k][2] = p.Z[idx[k]];
  }
  double P[4 * 12];
  const int nm = ap_p3p(x, X, P);
  double* out = models + (size_t)i * 48;
  for (int k = 0; k < 48; ++k) out[k] = k < 12 * nm ? P[k] : 0.0;  // a zero model puts every point at depth 0: no inliers
  nmod[i] = nm;
}

__global__ __launch_bounds__(kT) void k_ap_score(const double* __restrict__ models, int32_t nmodels, int32_t n, ApPts p, double thr2,
                                                  int32_t* __restrict__ part_cnt, double* __restrict__ part_sum) {
  __shared__ double sm[kTile * 12];
  __shared__ double red_s[kWaves][kTile];
  __shared__ int red_c[kWaves][kTile];
  const int m0 = (int)blockIdx.y * kTile;
  for (int k = threadIdx.x; k < kTile * 12; k += kT) {
    const int m = m0 + k / 12;
    sm[k] = m < nmodels ? models[(size_t)m0 * 12 + k] : 0.0;
  }
  __syncthreads();
  int cnt[kTile];
  double sum[kTile];
#pragma unroll
  for (int m = 0; m < kTile; ++m) { cnt[m] = 0; sum[m] = 0.0; }
  for (int32_t i = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x; i < n; i += (int32_t)gridDim.x * kT) {
    const double X = p.X[i], Y = p.Y[i], Z = p.Z[i], u = p.u[i], v = p.v[i];
#pragma unroll
    for (int m = 0; m < kTile; ++m) {
      const double r = ap_residual(sm + 12 * m, X, Y, Z, u, v);
      if (r <= thr2) { cnt[m] += 1; sum[m] += r; }
    }
  }
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll
  for (int m = 0; m < kTile; ++m) {
    const int c = wave_sum_i(cnt[m]);
    const double s = wave_sum(sum[m]);
    if (lane == 0) { red_c[wave][m] = c; red_s[wave][m] = s; }
  }
  __syncthreads();
  if (threadIdx.x < kTile) {
    const int m = m0 + (int)threadIdx.x;
    int c = 0;
    double s = 0.0;
    for (int w = 0; w < kWaves; ++w) { c += red_c[w][threadIdx.x]; s += red_s[w][threadIdx.x]; }
    if (m < nmodels) { part_cnt[(size_t)m * gridDim.x + blockIdx.x] = c; part_sum[(size_t)m * gridDim.x + blockIdx.x] = s; }
  }
}

__global__ __launch_bounds__(kT) void k_ap_score_sum(const int32_t* __restrict__ part_cnt, const double* __restrict__ part_sum, int32_t nmodels,
                                                      int32_t nparts, int32_t* __restrict__ cnt, double* __restrict__ sum) {
  const int32_t m = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  if (m >= nmodels) return;
  int c = 0;
  double s = 0.0;
  for (int b = 0; b < nparts; ++b) { c += part_cnt[(size_t)m * nparts + b]; s += part_sum[(size_t)m * nparts + b]; }
  cnt[m] = c;
  sum[m] = s;
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
  __shared__ double red[kWaves][K];
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
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double s = wave_sum(acc[k]);
    if (lane == 0) red[wave][k] = s;
  }
  if (PASS == 1) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) lo = min(lo, __shfl_xor(lo, off, 64));
    if (lane == 0) red_first[wave] = lo;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += kT) {
    double s = 0.0;
    for (int w = 0; w < kWaves; ++w) s += red[w][k];
    part[(size_t)blockIdx.x * K + k] = s;
  }
  if (PASS == 1 && threadIdx.x == 0) {
    int m = INT32_MAX;
    for (int w = 0; w < kWaves; ++w) m = min(m, red_first[w]);
    first[blockIdx.x] = m;
  }
}

__global__ __launch_bounds__(kT) void k_ap_mask(const double* __restrict__ P, int32_t n, ApPts p, double thr2, uint8_t* __restrict__ mask) {
  const int32_t i = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  if (i >= n) return;
  mask[i] = ap_residual(P, p.X[i], p.Y[i], p.Z[i], p.u[i], p.v[i]) <= thr2 ? 1 : 0;
}

struct ApCall {  // a pooled non-blocking stream per call, never the legacy null stream (see DevBuf in tri_kernels.hip)
  std::vector<void*> v;
  hipStream_t st = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  double ms = 0.0;
  ~ApCall() {
    if (st) (void)hipStreamSynchronize(st);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    for (void* p : v) cached_free(p);
    release_stream(st);
  }
  void* get(size_t bytes) { void* p = cached_malloc(bytes ? bytes : 1); if (p) v.push_back(p); return p; }
  int begin() { AP_TRY(hipEventRecord(ev[0], st)); return 0; }
  // closes a timed segment: the stream is idle on return
  int end() {
    AP_TRY(hipEventRecord(ev[1], st));
    AP_TRY(hipStreamSynchronize(st));
    float t = 0.f;
    AP_TRY(hipEventElapsedTime(&t, ev[0], ev[1]));
    ms += t;
    return 0;
  }
};

bool finite_all(const double* a, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(a[i])) return false;
  return true;
}
}  // namespace

}  // namespace mpsfm

using namespace mpsfm;

extern "C" int mpsfm_abs_pose_estimate(int64_t n64, const double* points2D, const double* points3D, const double* intr,
                                       const mpsfm_abs_pose_options* o, int32_t device, uint8_t* inlier_mask,
                                       mpsfm_abs_pose_result* result) {
  if (result) *result = mpsfm_abs_pose_result{};
  if (!points2D || !points3D || !intr || !o || !inlier_mask || !result) return apfail(MPSFM_EINVAL, "NULL pointer");
  if (n64 < 3) return apfail(MPSFM_EINVAL, "fewer than 3 correspondences");
  if (n64 > INT32_MAX) return apfail(MPSFM_EINVAL, "more than INT32_MAX correspondences (int32 indexing)");
  const int32_t n = (int32_t)n64;
  if (!finite_all(points2D, 2 * (size_t)n) || !finite_all(points3D, 3 * (size_t)n)) return apfail(MPSFM_EINVAL, "non-finite point");
  if (!finite_all(intr, 4) || intr[0] == 0.0 || intr[1] == 0.0 || intr[0] + intr[1] == 0.0)
    return apfail(MPSFM_EINVAL, "intrinsics must be finite with non-zero focal lengths");
  if (!(o->max_error > 0.0) || !std::isfinite(o->max_error) || !(o->min_inlier_ratio > 0.0 && o->min_inlier_ratio <= 1.0) ||
      !(o->confidence >= 0.0 && o->confidence <= 1.0) || !(o->dyn_num_trials_multiplier > 0.0) || !std::isfinite(o->dyn_num_trials_multiplier) ||
      o->min_num_trials < 0 || o->max_num_trials < 0 || o->min_num_trials > o->max_num_trials || o->batch_trials < 0 || o->batch_trials > kMaxBatch)
    return apfail(MPSFM_EINVAL, "invalid RANSAC options");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return apfail(MPSFM_ENODEVICE, "no HIP device visible: libmpsfm_hip has no CPU fallback");
  if (device < 0 || device >= ndev) return apfail(MPSFM_EINVAL, "device ordinal out of range");
  if (device >= kMaxDevices) return apfail(MPSFM_EUNSUPPORTED, "device ordinals beyond 15 are not supported (per-device pools)");
  AP_TRY(hipSetDevice(device));

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
  auto hX = [&](int32_t i) { return hs[i]; };
  auto hY = [&](int32_t i) { return hs[(size_t)n + i]; };
  auto hZ = [&](int32_t i) { return hs[2 * (size_t)n + i]; };

  const int64_t max_trials = std::min<int64_t>(
      o->max_num_trials, ap_num_trials((int64_t)(o->min_inlier_ratio * 100000.0), 100000, o->confidence, o->dyn_num_trials_multiplier));
  const int32_t B = o->batch_trials > 0 ? o->batch_trials : kDefaultBatch;
  const int32_t Bcap = (int32_t)std::max<int64_t>(1, std::min<int64_t>(B, max_trials));
  const int32_t Mcap = 4 * Bcap;
  const int nbx = ap_blocks(n, 4 * kT);  // scoring workgroups along the points
  const int npx = ap_blocks(n, kT);      // EPnP pass workgroups

  ApCall A;
  AP_TRY(pooled_stream(&A.st));
  AP_TRY(hipEventCreate(&A.ev[0]));
  AP_TRY(hipEventCreate(&A.ev[1]));
  double* d_pts = (double*)A.get(sizeof(double) * 5 * (size_t)n);
  double* d_models = (double*)A.get(sizeof(double) * 12 * (size_t)Mcap);
  int32_t* d_nmod = (int32_t*)A.get(sizeof(int32_t) * (size_t)Bcap);
  int32_t* d_pcnt = (int32_t*)A.get(sizeof(int32_t) * (size_t)Mcap * nbx);
  double* d_psum = (double*)A.get(sizeof(double) * (size_t)Mcap * nbx);
  int32_t* d_cnt = (int32_t*)A.get(sizeof(int32_t) * (size_t)Mcap);
  double* d_sum = (double*)A.get(sizeof(double) * (size_t)Mcap);
  double* d_part = (double*)A.get(sizeof(double) * 78 * (size_t)npx);
  int32_t* d_first = (int32_t*)A.get(sizeof(int32_t) * (size_t)npx);
  uint8_t* d_mask = (uint8_t*)A.get((size_t)n);
  if (!d_pts || !d_models || !d_nmod || !d_pcnt || !d_psum || !d_cnt || !d_sum || !d_part || !d_first || !d_mask)
    return apfail(MPSFM_ENOMEM, "hipMalloc failed");
  AP_TRY(hipMemcpyAsync(d_pts, hs.data(), sizeof(double) * 5 * (size_t)n, hipMemcpyHostToDevice, A.st));
  const ApPts P{d_pts, d_pts + n, d_pts + 2 * (size_t)n, d_pts + 3 * (size_t)n, d_pts + 4 * (size_t)n};

  std::vector<double> h_models((size_t)12 * Mcap), h_sum((size_t)Mcap);
  std::vector<int32_t> h_nmod((size_t)Bcap), h_cnt((size_t)Mcap);
  std::vector<double> h_part((size_t)78 * npx);
  std::vector<int32_t> h_first((size_t)npx);

  // scores M models already on the device (d_models): counts and sums into h_cnt / h_sum [0, M)
  auto score = [&](int32_t M) -> int {
    const dim3 grid((unsigned)nbx, (unsigned)((M + kTile - 1) / kTile));
    hipLaunchKernelGGL(k_ap_score, grid, dim3(kT), 0, A.st, d_models, M, n, P, thr2, d_pcnt, d_psum);
    AP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_ap_score_sum, dim3((unsigned)((M + kT - 1) / kT)), dim3(kT), 0, A.st, d_pcnt, d_psum, M, nbx, d_cnt, d_sum);
    AP_TRY(hipGetLastError());
    AP_TRY(hipMemcpyAsync(h_cnt.data(), d_cnt, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToHost, A.st));
    AP_TRY(hipMemcpyAsync(h_sum.data(), d_sum, sizeof(double) * (size_t)M, hipMemcpyDeviceToHost, A.st));
    return 0;
  };
  // one EPnP pass: the workgroups' rows summed in order into out[K]
  auto pass = [&](auto tag, const ApPassArgs& a, double* out) -> int {
    constexpr int PASS = decltype(tag)::value;
    constexpr int K = ApPassK<PASS>::K;
    if (int rc = A.begin()) return rc;
    hipLaunchKernelGGL(k_ap_pass<PASS>, dim3((unsigned)npx), dim3(kT), 0, A.st, a, n, P, d_part, d_first);
    AP_TRY(hipGetLastError());
    AP_TRY(hipMemcpyAsync(h_part.data(), d_part, sizeof(double) * K * (size_t)npx, hipMemcpyDeviceToHost, A.st));
    if (PASS == 1) AP_TRY(hipMemcpyAsync(h_first.data(), d_first, sizeof(int32_t) * (size_t)npx, hipMemcpyDeviceToHost, A.st));
    if (int rc = A.end()) return rc;
    for (int k = 0; k < K; ++k) {
      double s = 0.0;
      for (int b = 0; b < npx; ++b) s += h_part[(size_t)b * K + k];
      out[k] = s;
    }
    return 0;
  };
  using P1 = std::integral_constant<int, 1>;
  using P2 = std::integral_constant<int, 2>;
  using P3 = std::integral_constant<int, 3>;
  using P4 = std::integral_constant<int, 4>;
  using P5 = std::integral_constant<int, 5>;

  int lo_rounds = 0;
  // EPNPEstimator::Estimate on the inliers of Pin; false: no model
  auto epnp = [&](const double* Pin, double* Pout, bool& ok) -> int {
    ok = false;
    ApPassArgs a{};
    std::memcpy(a.Pin, Pin, sizeof(a.Pin));
    a.thr2 = thr2;
    double s1[4];
    if (int rc = pass(P1{}, a, s1)) return rc;
    const int64_t m = (int64_t)s1[0];
    if (m < 4) return 0;
    int32_t first = INT32_MAX;
    for (int b = 0; b < npx; ++b) first = std::min(first, h_first[(size_t)b]);
    const double c0[3] = {s1[1] / (double)m, s1[2] / (double)m, s1[3] / (double)m};
    for (int d = 0; d < 3; ++d) a.F.cws[0][d] = c0[d];
    double sc[6];
    if (int rc = pass(P2{}, a, sc)) return rc;
    if (!ap_epnp_frame(c0, sc, m, a.F)) return 0;
    double mtm[78];
    if (int rc = pass(P3{}, a, mtm)) return rc;
    double MtM[12][12], V[12][12], w[12];
    for (int r = 0, k = 0; r < 12; ++r)
      for (int c = r; c < 12; ++c, ++k) MtM[r][c] = MtM[c][r] = mtm[k];
    ap_sym_eig<12>(MtM, V, w);
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
    if (int rc = pass(P4{}, a, s4)) return rc;
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
    if (int rc = pass(P5{}, a, err)) return rc;
    int bi = 0;
    if (err[1] < err[0]) bi = 1;
    if (err[2] < err[bi]) bi = 2;
    std::memcpy(Pout, a.P3[bi], sizeof(double) * 12);
    ok = true;
    return 0;
  };

  TriSupport best{0, DBL_MAX};
  double best_model[12] = {};
  int64_t dyn = max_trials, trials = 0, b0 = 0, bn = 0, models_scored = 0;
  int32_t batches = 0;
  bool abort_ = false;
  for (trials = 0; trials < max_trials; ++trials) {
    if (abort_) { trials += 1; break; }
    if (trials >= b0 + bn) {  // next batch: generate, score, download the table
      b0 = trials;
      bn = std::min<int64_t>(Bcap, max_trials - trials);
      const int32_t M = 4 * (int32_t)bn;
      if (int rc = A.begin()) return rc;
      hipLaunchKernelGGL(k_ap_p3p, dim3((unsigned)((bn + kT - 1) / kT)), dim3(kT), 0, A.st, o->seed, b0, (int32_t)bn, n, P, d_models, d_nmod);
      AP_TRY(hipGetLastError());
      if (int rc = score(M)) return rc;
      AP_TRY(hipMemcpyAsync(h_nmod.data(), d_nmod, sizeof(int32_t) * (size_t)bn, hipMemcpyDeviceToHost, A.st));
      AP_TRY(hipMemcpyAsync(h_models.data(), d_models, sizeof(double) * 12 * (size_t)M, hipMemcpyDeviceToHost, A.st));
      if (int rc = A.end()) return rc;
      ++batches;
      models_scored += M;
    }
    const int64_t lt = trials - b0;
    for (int k = 0; k < h_nmod[(size_t)lt]; ++k) {
      const size_t slot = 4 * (size_t)lt + k;
      const TriSupport sup{h_cnt[slot], h_sum[slot]};
      if (tri_better(sup, best)) {
        best = sup;
        std::memcpy(best_model, &h_models[12 * slot], sizeof(best_model));
        if (sup.num_inliers > 3 && sup.num_inliers >= 4) {  // local optimisation (kMaxNumLocalTrials = 10)
          double in_model[12];
          std::memcpy(in_model, best_model, sizeof(in_model));
          for (int local = 0; local < 10; ++local) {
            const int prev = best.num_inliers;
            double Pl[12];
            bool ok = false;
            ++lo_rounds;
            if (int rc = epnp(in_model, Pl, ok)) return rc;
            if (ok) {
              // the local model goes to the last model slot (the batch's table is on the host already) and is scored alone
              AP_TRY(hipMemcpyAsync(d_models + 12 * (size_t)Mcap - 12, Pl, sizeof(Pl), hipMemcpyHostToDevice, A.st));
              if (int rc = A.begin()) return rc;
              const dim3 grid((unsigned)nbx, 1u);
              hipLaunchKernelGGL(k_ap_score, grid, dim3(kT), 0, A.st, d_models + 12 * (size_t)Mcap - 12, 1, n, P, thr2, d_pcnt, d_psum);
              AP_TRY(hipGetLastError());
              hipLaunchKernelGGL(k_ap_score_sum, dim3(1), dim3(kT), 0, A.st, d_pcnt, d_psum, 1, nbx, d_cnt, d_sum);
              AP_TRY(hipGetLastError());
              int32_t lc = 0;
              double ls = 0.0;
              AP_TRY(hipMemcpyAsync(&lc, d_cnt, sizeof(int32_t), hipMemcpyDeviceToHost, A.st));
              AP_TRY(hipMemcpyAsync(&ls, d_sum, sizeof(double), hipMemcpyDeviceToHost, A.st));
              if (int rc = A.end()) return rc;
              const TriSupport loc{lc, ls};
              if (tri_better(loc, best)) {
                best = loc;
                std::memcpy(best_model, Pl, sizeof(best_model));
                std::memcpy(in_model, Pl, sizeof(in_model));
              }
            }
            if (best.num_inliers <= prev) break;
          }
        }
        dyn = ap_num_trials(best.num_inliers, n, o->confidence, o->dyn_num_trials_multiplier);
      }
      if (trials >= dyn && trials >= o->min_num_trials) { abort_ = true; break; }
    }
  }
  result->num_trials = trials;
  result->max_num_trials = max_trials;
  result->num_models = models_scored;
  result->lo_rounds = lo_rounds;
  result->num_batches = batches;
  if (best.num_inliers < 3) {
    result->ms = (float)A.ms;
    std::memset(inlier_mask, 0, (size_t)n);
    return 0;
  }
  AP_TRY(hipMemcpyAsync(d_models, best_model, sizeof(best_model), hipMemcpyHostToDevice, A.st));
  if (int rc = A.begin()) return rc;
  hipLaunchKernelGGL(k_ap_mask, dim3((unsigned)((n + kT - 1) / kT)), dim3(kT), 0, A.st, d_models, n, P, thr2, d_mask);
  AP_TRY(hipGetLastError());
  AP_TRY(hipMemcpyAsync(inlier_mask, d_mask, (size_t)n, hipMemcpyDeviceToHost, A.st));
  if (int rc = A.end()) return rc;
  std::memcpy(result->cam_from_world, best_model, sizeof(best_model));
  result->num_inliers = best.num_inliers;
  result->success = 1;
  result->ms = (float)A.ms;
  return 0;
}
