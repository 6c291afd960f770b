// Relative-pose LO-RANSAC of one two-view problem (mpsfm_rel_pose_estimate; semantics and what is unpinned:
// include/mpsfm_hip.h).  The sequential LORANSAC loop is replayed on the host over tables the device fills in batches
// (the design of abs_pose.hip):
//   k_rp_five        one thread per trial of a batch: the trial's five-index sample, the five-point solver with its
//                    runtime-indexed arrays in a per-thread LDS slice (rel_pose_math.h), up to 10 canonical models in
//                    lexicographic order (zeros pad: a zero E scores no inlier)
//   k_rp_score       a tile of kTile models in LDS against a grid-stride stream of matches: per model inlier count and
//                    Sampson sum of the workgroup, reduced in a fixed order (wave butterflies, then the waves in order)
//   k_rp_score_sum   one thread per model: the workgroups' partial rows in order (no float atomics)
//   k_rp_gram        Q^T Q (upper 45 entries) and the count over the inliers of a model: the local estimator's input
//   k_rp_mask        the final inlier mask
//   k_rp_cheirality  the four (R, t) candidates of the final E against every inlier in one pass (two-view DLT, depth test)
// The local estimator's 9 x 9 eigenvectors and its five-point algebra, and the decomposition of E, run on the host.
// f64 throughout.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "rel_pose_math.h"
#include "tri_math.h"

namespace mpsfm {

extern thread_local std::string g_err;
static int rpfail(int code, const std::string& m) { g_err = m; return code; }
#define RP_TRY(expr)                                                                                  \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess) return rpfail(MPSFM_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

namespace {
constexpr int kT = 256;
constexpr int kWaves = kT / 64;
constexpr int kFiveT = 32;          // trials per k_rp_five workgroup: 32 x RP_WORK doubles = 59 KiB of LDS
constexpr int kTile = 16;           // models per scoring workgroup
constexpr int kDefaultBatch = 4096;  // trials per batch
constexpr int kMaxBatch = 1 << 16;
constexpr int kGramK = 46;          // count, then the upper triangle of Q^T Q row-major

struct RpPts { const double *u1, *v1, *u2, *v2; };

int rp_blocks(int32_t n, int per_block) { return (int)std::min<int64_t>(((int64_t)n + per_block - 1) / per_block, 64); }

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

__global__ __launch_bounds__(kFiveT) void k_rp_five(uint64_t seed, int64_t t0, int32_t nb, int32_t n, RpPts p, double* __restrict__ models,
                                                     int32_t* __restrict__ nmod) {
  __shared__ double work[kFiveT * RP_WORK];
  const int32_t i = (int32_t)blockIdx.x * kFiveT + (int32_t)threadIdx.x;
  if (i >= nb) return;
  int32_t idx[kRpSample];
  rp_sample(seed, t0 + i, n, idx);
  double u1[kRpSample], v1[kRpSample], u2[kRpSample], v2[kRpSample];
#pragma unroll
  for (int k = 0; k < kRpSample; ++k) { u1[k] = p.u1[idx[k]]; v1[k] = p.v1[idx[k]]; u2[k] = p.u2[idx[k]]; v2[k] = p.v2[idx[k]]; }
  const RpW w{work + threadIdx.x, kFiveT};
  double* out = models + (size_t)i * 9 * kRpMaxModels;
  int nm = 0;
  if (rp_nullspace5(u1, v1, u2, v2, w)) nm = rp_models_from_nullspace(w, out);
  for (int k = 9 * nm; k < 9 * kRpMaxModels; ++k) out[k] = 0.0;
  nmod[i] = nm;
}

__global__ __launch_bounds__(kT) void k_rp_score(const double* __restrict__ models, int32_t nmodels, int32_t n, RpPts p, double thr2,
                                                  int32_t* __restrict__ part_cnt, double* __restrict__ part_sum) {
  __shared__ double sm[kTile * 9];
  __shared__ double red_s[kWaves][kTile];
  __shared__ int red_c[kWaves][kTile];
  const int m0 = (int)blockIdx.y * kTile;
  for (int k = threadIdx.x; k < kTile * 9; k += kT) {
    const int m = m0 + k / 9;
    sm[k] = m < nmodels ? models[(size_t)m0 * 9 + k] : 0.0;
  }
  __syncthreads();
  int cnt[kTile];
  double sum[kTile];
#pragma unroll
  for (int m = 0; m < kTile; ++m) { cnt[m] = 0; sum[m] = 0.0; }
  for (int32_t i = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x; i < n; i += (int32_t)gridDim.x * kT) {
    const double u1 = p.u1[i], v1 = p.v1[i], u2 = p.u2[i], v2 = p.v2[i];
#pragma unroll
    for (int m = 0; m < kTile; ++m) {
      const double r = rp_sampson(sm + 9 * m, u1, v1, u2, v2);
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

__global__ __launch_bounds__(kT) void k_rp_score_sum(const int32_t* __restrict__ part_cnt, const double* __restrict__ part_sum, int32_t nmodels,
                                                      int32_t nparts, int32_t* __restrict__ cnt, double* __restrict__ sum) {
  const int32_t m = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  if (m >= nmodels) return;
  int c = 0;
  double s = 0.0;
  for (int b = 0; b < nparts; ++b) { c += part_cnt[(size_t)m * nparts + b]; s += part_sum[(size_t)m * nparts + b]; }
  cnt[m] = c;
  sum[m] = s;
}

struct RpModel { double E[9]; };

__global__ __launch_bounds__(kT) void k_rp_gram(RpModel Ein, double thr2, int32_t n, RpPts p, double* __restrict__ part) {
  __shared__ double red[kWaves][kGramK];
  double acc[kGramK];
#pragma unroll
  for (int k = 0; k < kGramK; ++k) acc[k] = 0.0;
  for (int32_t i = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x; i < n; i += (int32_t)gridDim.x * kT) {
    const double u1 = p.u1[i], v1 = p.v1[i], u2 = p.u2[i], v2 = p.v2[i];
    if (!(rp_sampson(Ein.E, u1, v1, u2, v2) <= thr2)) continue;
    double q[9];
    rp_q_row(u1, v1, u2, v2, q);
    acc[0] += 1.0;
    int k = 1;
#pragma unroll
    for (int r = 0; r < 9; ++r)
#pragma unroll
      for (int c = r; c < 9; ++c) acc[k++] += q[r] * q[c];
  }
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll
  for (int k = 0; k < kGramK; ++k) {
    const double s = wave_sum(acc[k]);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kGramK; k += kT) {
    double s = 0.0;
    for (int w = 0; w < kWaves; ++w) s += red[w][k];
    part[(size_t)blockIdx.x * kGramK + k] = s;
  }
}

__global__ __launch_bounds__(kT) void k_rp_mask(RpModel E, int32_t n, RpPts p, double thr2, uint8_t* __restrict__ mask) {
  const int32_t i = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  if (i >= n) return;
  mask[i] = rp_sampson(E.E, p.u1[i], p.v1[i], p.u2[i], p.v2[i]) <= thr2 ? 1 : 0;
}

struct RpCands { double P[4][12]; double max_depth[4]; };

// CheckCheirality of the four candidates: per workgroup the number of inliers triangulated in front of both cameras
__global__ __launch_bounds__(kT) void k_rp_cheirality(RpCands c, int32_t n, RpPts p, const uint8_t* __restrict__ mask,
                                                       int32_t* __restrict__ part) {
  __shared__ int red[kWaves][4];
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
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int s = wave_sum_i(cnt[k]);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    int s = 0;
    for (int w = 0; w < kWaves; ++w) s += red[w][threadIdx.x];
    part[(size_t)blockIdx.x * 4 + threadIdx.x] = s;
  }
}

struct RpCall {  // a pooled non-blocking stream per call, never the legacy null stream (see DevBuf in tri_kernels.hip)
  std::vector<void*> v;
  hipStream_t st = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  double ms = 0.0;
  ~RpCall() {
    if (st) (void)hipStreamSynchronize(st);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    for (void* p : v) cached_free(p);
    release_stream(st);
  }
  void* get(size_t bytes) { void* p = cached_malloc(bytes ? bytes : 1); if (p) v.push_back(p); return p; }
  int begin() { RP_TRY(hipEventRecord(ev[0], st)); return 0; }
  int end() {
    RP_TRY(hipEventRecord(ev[1], st));
    RP_TRY(hipStreamSynchronize(st));
    float t = 0.f;
    RP_TRY(hipEventElapsedTime(&t, ev[0], ev[1]));
    ms += t;
    return 0;
  }
};

bool rp_finite_all(const double* a, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(a[i])) return false;
  return true;
}
}  // namespace

}  // namespace mpsfm

using namespace mpsfm;

extern "C" int mpsfm_rel_pose_estimate(int64_t n64, const double* points1, const double* points2, const double* intr1, const double* intr2,
                                       const mpsfm_rel_pose_options* o, int32_t device, uint8_t* inlier_mask, mpsfm_rel_pose_result* result) {
  if (result) *result = mpsfm_rel_pose_result{};
  if (!points1 || !points2 || !intr1 || !intr2 || !o || !inlier_mask || !result) return rpfail(MPSFM_EINVAL, "NULL pointer");
  if (n64 < kRpSample) return rpfail(MPSFM_EINVAL, "fewer than 5 correspondences");
  if (n64 > INT32_MAX) return rpfail(MPSFM_EINVAL, "more than INT32_MAX correspondences (int32 indexing)");
  const int32_t n = (int32_t)n64;
  if (!rp_finite_all(points1, 2 * (size_t)n) || !rp_finite_all(points2, 2 * (size_t)n)) return rpfail(MPSFM_EINVAL, "non-finite point");
  for (const double* K : {intr1, intr2})
    if (!rp_finite_all(K, 4) || K[0] == 0.0 || K[1] == 0.0 || K[0] + K[1] == 0.0)
      return rpfail(MPSFM_EINVAL, "intrinsics must be finite with non-zero focal lengths");
  if (!(o->max_error > 0.0) || !std::isfinite(o->max_error) || !(o->min_inlier_ratio > 0.0 && o->min_inlier_ratio <= 1.0) ||
      !(o->confidence >= 0.0 && o->confidence <= 1.0) || !(o->dyn_num_trials_multiplier > 0.0) || !std::isfinite(o->dyn_num_trials_multiplier) ||
      o->min_num_trials < 0 || o->max_num_trials < 0 || o->min_num_trials > o->max_num_trials || o->batch_trials < 0 || o->batch_trials > kMaxBatch)
    return rpfail(MPSFM_EINVAL, "invalid RANSAC options");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return rpfail(MPSFM_ENODEVICE, "no HIP device visible: libmpsfm_hip has no CPU fallback");
  if (device < 0 || device >= ndev) return rpfail(MPSFM_EINVAL, "device ordinal out of range");
  if (device >= kMaxDevices) return rpfail(MPSFM_EUNSUPPORTED, "device ordinals beyond 15 are not supported (per-device pools)");
  RP_TRY(hipSetDevice(device));

  // EstimateEssentialMatrix: CamFromImg of both PINHOLE cameras, the mean of their normalised thresholds
  const double thr = 0.5 * (o->max_error / ((intr1[0] + intr1[1]) / 2.0) + o->max_error / ((intr2[0] + intr2[1]) / 2.0));
  const double thr2 = thr * thr;
  std::vector<double> hs((size_t)4 * n);  // SoA: u1 v1 u2 v2
  for (int32_t i = 0; i < n; ++i) {
    hs[i] = (points1[2 * (size_t)i] - intr1[2]) / intr1[0];
    hs[(size_t)n + i] = (points1[2 * (size_t)i + 1] - intr1[3]) / intr1[1];
    hs[2 * (size_t)n + i] = (points2[2 * (size_t)i] - intr2[2]) / intr2[0];
    hs[3 * (size_t)n + i] = (points2[2 * (size_t)i + 1] - intr2[3]) / intr2[1];
  }

  const int64_t max_trials = std::min<int64_t>(
      o->max_num_trials, rp_num_trials((int64_t)(o->min_inlier_ratio * 100000.0), 100000, o->confidence, o->dyn_num_trials_multiplier, kRpSample));
  const int32_t B = o->batch_trials > 0 ? o->batch_trials : kDefaultBatch;
  const int32_t Bcap = (int32_t)std::max<int64_t>(1, std::min<int64_t>(B, max_trials));
  const int32_t Mcap = kRpMaxModels * Bcap;  // batch models; kRpMaxModels more slots after them for the local models
  const int nbx = rp_blocks(n, 4 * kT);      // scoring workgroups along the matches
  const int npx = rp_blocks(n, kT);          // reduction workgroups

  RpCall A;
  RP_TRY(pooled_stream(&A.st));
  RP_TRY(hipEventCreate(&A.ev[0]));
  RP_TRY(hipEventCreate(&A.ev[1]));
  double* d_pts = (double*)A.get(sizeof(double) * 4 * (size_t)n);
  double* d_models = (double*)A.get(sizeof(double) * 9 * ((size_t)Mcap + kRpMaxModels));
  int32_t* d_nmod = (int32_t*)A.get(sizeof(int32_t) * (size_t)Bcap);
  int32_t* d_pcnt = (int32_t*)A.get(sizeof(int32_t) * (size_t)Mcap * nbx);
  double* d_psum = (double*)A.get(sizeof(double) * (size_t)Mcap * nbx);
  int32_t* d_cnt = (int32_t*)A.get(sizeof(int32_t) * (size_t)Mcap);
  double* d_sum = (double*)A.get(sizeof(double) * (size_t)Mcap);
  double* d_part = (double*)A.get(sizeof(double) * kGramK * (size_t)npx);
  int32_t* d_ipart = (int32_t*)A.get(sizeof(int32_t) * 4 * (size_t)npx);
  uint8_t* d_mask = (uint8_t*)A.get((size_t)n);
  if (!d_pts || !d_models || !d_nmod || !d_pcnt || !d_psum || !d_cnt || !d_sum || !d_part || !d_ipart || !d_mask)
    return rpfail(MPSFM_ENOMEM, "hipMalloc failed");
  RP_TRY(hipMemcpyAsync(d_pts, hs.data(), sizeof(double) * 4 * (size_t)n, hipMemcpyHostToDevice, A.st));
  const RpPts P{d_pts, d_pts + n, d_pts + 2 * (size_t)n, d_pts + 3 * (size_t)n};
  double* d_local = d_models + 9 * (size_t)Mcap;

  std::vector<double> h_models((size_t)9 * Mcap), h_sum((size_t)Mcap);
  std::vector<int32_t> h_nmod((size_t)Bcap), h_cnt((size_t)Mcap);
  std::vector<double> h_part((size_t)kGramK * npx);
  std::vector<int32_t> h_ipart((size_t)4 * npx);

  // scores M models at dm: counts and sums into hc / hsum [0, M)
  auto score = [&](const double* dm, int32_t M, int32_t* hc, double* hsum) -> int {
    const dim3 grid((unsigned)nbx, (unsigned)((M + kTile - 1) / kTile));
    hipLaunchKernelGGL(k_rp_score, grid, dim3(kT), 0, A.st, dm, M, n, P, thr2, d_pcnt, d_psum);
    RP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_rp_score_sum, dim3((unsigned)((M + kT - 1) / kT)), dim3(kT), 0, A.st, d_pcnt, d_psum, M, nbx, d_cnt, d_sum);
    RP_TRY(hipGetLastError());
    RP_TRY(hipMemcpyAsync(hc, d_cnt, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToHost, A.st));
    RP_TRY(hipMemcpyAsync(hsum, d_sum, sizeof(double) * (size_t)M, hipMemcpyDeviceToHost, A.st));
    return 0;
  };

  int64_t lo_rounds = 0;
  // EssentialMatrixFivePointEstimator::Estimate on the inliers of Ein (n > 5: the nullspace of Q^T Q): up to 10 models
  auto local = [&](const double* Ein, double* out, int& nm) -> int {
    nm = 0;
    RpModel m;
    std::memcpy(m.E, Ein, sizeof(m.E));
    if (int rc = A.begin()) return rc;
    hipLaunchKernelGGL(k_rp_gram, dim3((unsigned)npx), dim3(kT), 0, A.st, m, thr2, n, P, d_part);
    RP_TRY(hipGetLastError());
    RP_TRY(hipMemcpyAsync(h_part.data(), d_part, sizeof(double) * kGramK * (size_t)npx, hipMemcpyDeviceToHost, A.st));
    if (int rc = A.end()) return rc;
    double g[kGramK];
    for (int k = 0; k < kGramK; ++k) {
      double s = 0.0;
      for (int b = 0; b < npx; ++b) s += h_part[(size_t)b * kGramK + k];
      g[k] = s;
    }
    if (g[0] < kRpSample) return 0;
    double G[9][9], V[9][9], ev[9];
    for (int r = 0, k = 1; r < 9; ++r)
      for (int c = r; c < 9; ++c, ++k) G[r][c] = G[c][r] = g[k];
    ap_sym_eig<9>(G, V, ev);  // ascending
    if (!(ev[4] > kRpRankTol * kRpRankTol * ev[8])) return 0;
    double work[RP_WORK];
    const RpW w{work, 1};
    for (int k = 0; k < 4; ++k)
      for (int i = 0; i < 9; ++i) w[RP_N + 9 * k + i] = V[i][3 - k];
    nm = rp_models_from_nullspace(w, out);
    return 0;
  };

  TriSupport best{0, DBL_MAX};
  double best_model[9] = {};
  int64_t dyn = max_trials, trials = 0, b0 = 0, bn = 0, models_scored = 0, batches = 0;
  bool abort_ = false;
  for (trials = 0; trials < max_trials; ++trials) {
    if (abort_) { trials += 1; break; }
    if (trials >= b0 + bn) {  // next batch: generate, score, download the table
      b0 = trials;
      bn = std::min<int64_t>(Bcap, max_trials - trials);
      const int32_t M = kRpMaxModels * (int32_t)bn;
      if (int rc = A.begin()) return rc;
      hipLaunchKernelGGL(k_rp_five, dim3((unsigned)((bn + kFiveT - 1) / kFiveT)), dim3(kFiveT), 0, A.st, o->seed, b0, (int32_t)bn, n, P, d_models,
                         d_nmod);
      RP_TRY(hipGetLastError());
      if (int rc = score(d_models, M, h_cnt.data(), h_sum.data())) return rc;
      RP_TRY(hipMemcpyAsync(h_nmod.data(), d_nmod, sizeof(int32_t) * (size_t)bn, hipMemcpyDeviceToHost, A.st));
      RP_TRY(hipMemcpyAsync(h_models.data(), d_models, sizeof(double) * 9 * (size_t)M, hipMemcpyDeviceToHost, A.st));
      if (int rc = A.end()) return rc;
      ++batches;
      models_scored += M;
    }
    const int64_t lt = trials - b0;
    for (int k = 0; k < h_nmod[(size_t)lt]; ++k) {
      const size_t slot = (size_t)kRpMaxModels * lt + k;
      const TriSupport sup{h_cnt[slot], h_sum[slot]};
      if (tri_better(sup, best)) {
        best = sup;
        std::memcpy(best_model, &h_models[9 * slot], sizeof(best_model));
        if (sup.num_inliers > kRpSample && sup.num_inliers >= kRpSample) {  // local optimisation (kMaxNumLocalTrials = 10)
          for (int round = 0; round < 10; ++round) {
            const int prev = best.num_inliers;
            double Lm[9 * kRpMaxModels];
            int nl = 0;
            ++lo_rounds;
            if (int rc = local(best_model, Lm, nl)) return rc;
            if (nl > 0) {
              RP_TRY(hipMemcpyAsync(d_local, Lm, sizeof(double) * 9 * (size_t)nl, hipMemcpyHostToDevice, A.st));
              if (int rc = A.begin()) return rc;
              int32_t lc[kRpMaxModels];  // the batch's table in h_cnt / h_sum is still being replayed
              double ls_[kRpMaxModels];
              if (int rc = score(d_local, nl, lc, ls_)) return rc;
              if (int rc = A.end()) return rc;
              for (int j = 0; j < nl; ++j) {
                const TriSupport ls{lc[j], ls_[j]};
                if (tri_better(ls, best)) {
                  best = ls;
                  std::memcpy(best_model, Lm + 9 * j, sizeof(best_model));
                }
              }
            }
            if (best.num_inliers <= prev) break;
          }
        }
        dyn = rp_num_trials(best.num_inliers, n, o->confidence, o->dyn_num_trials_multiplier, kRpSample);
      }
      if (trials >= dyn && trials >= o->min_num_trials) { abort_ = true; break; }
    }
  }
  result->num_trials = trials;
  result->max_num_trials = max_trials;
  result->num_models = models_scored;
  result->lo_rounds = lo_rounds;
  result->num_batches = batches;
  if (best.num_inliers < kRpSample) {
    result->ms = (float)A.ms;
    std::memset(inlier_mask, 0, (size_t)n);
    return 0;
  }
  // RANSAC's mask of the best model, then PoseFromEssentialMatrix on its inliers
  RpModel bm;
  std::memcpy(bm.E, best_model, sizeof(bm.E));
  RpCands cand;
  double R1[9], R2[9], t[3];
  rp_decompose(best_model, R1, R2, t);
  for (int k = 0; k < 4; ++k) {
    const double* R = (k % 2 == 0) ? R1 : R2;
    const double sg = k < 2 ? 1.0 : -1.0;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) cand.P[k][4 * r + c] = R[3 * r + c];
      cand.P[k][4 * r + 3] = sg * t[r];
    }
    cand.max_depth[k] = 1000.0 * std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
  }
  if (int rc = A.begin()) return rc;
  hipLaunchKernelGGL(k_rp_mask, dim3((unsigned)((n + kT - 1) / kT)), dim3(kT), 0, A.st, bm, n, P, thr2, d_mask);
  RP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_rp_cheirality, dim3((unsigned)npx), dim3(kT), 0, A.st, cand, n, P, d_mask, d_ipart);
  RP_TRY(hipGetLastError());
  RP_TRY(hipMemcpyAsync(inlier_mask, d_mask, (size_t)n, hipMemcpyDeviceToHost, A.st));
  RP_TRY(hipMemcpyAsync(h_ipart.data(), d_ipart, sizeof(int32_t) * 4 * (size_t)npx, hipMemcpyDeviceToHost, A.st));
  if (int rc = A.end()) return rc;
  int64_t bestc = -1;
  int bk = 0;
  for (int k = 0; k < 4; ++k) {
    int64_t c = 0;
    for (int b = 0; b < npx; ++b) c += h_ipart[(size_t)b * 4 + k];
    if (c >= bestc) { bestc = c; bk = k; }  // the later candidate wins a tie
  }
  std::memcpy(result->E, best_model, sizeof(best_model));
  std::memcpy(result->cam2_from_cam1, cand.P[bk], sizeof(cand.P[bk]));
  result->num_inliers = best.num_inliers;
  result->num_cheirality_points = bestc;
  result->success = 1;
  result->ms = (float)A.ms;
  return 0;
}
