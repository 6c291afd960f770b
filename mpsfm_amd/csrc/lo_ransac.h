// LO-RANSAC (COLMAP's LORANSAC as recalled: include/mpsfm_hip.h) for any problem with a minimal solver, a per-observation
// residual and a local estimator.  The sequential loop is replayed on the host over tables the device fills in batches:
//   P::minimal       one thread per trial of a batch: the trial's counter-based sample (lo_sample), the minimal solver, up
//                    to P::kSlots models per trial (zeros pad: a zero model scores no inlier)
//   k_lo_score       a tile of kLoTile models in LDS against a grid-stride stream of observations: per model inlier count
//                    and inlier residual sum of the workgroup, reduced in a fixed order (wave butterflies, then the waves in
//                    order)
//   k_lo_score_sum   one thread per model: the workgroups' partial rows in order -> count and sum (no float atomics: the
//                    table is bitwise identical run to run)
//   k_lo_mask        the inlier mask of one model
// The host walks the batch's table in trial order (best-model updates, the local optimisation, the dynamic bound, the
// stop rule), so the result is the sequential loop's.
//
// A problem description P is a plain struct (abs_pose.hip, rel_pose.hip, align3d.hip):
//   static constexpr int kSample, kModel (doubles per model), kSlots (models per trial), kLocal (<= kSlots: models of one
//                    local estimate), kDefaultBatch
//   struct Pts (SoA pointers, passed to kernels by value), struct Obs
//   static __device__ __forceinline__ Obs load(const Pts&, int32_t i);  double residual(const double* model, const Obs&)
//   int32_t n;  double thr2;  Pts pts;
//   void minimal(hipStream_t, uint64_t seed, int64_t t0, int32_t nb, double* models, int32_t* nmod)     launch only
//   int  local(CallScope&, const double* model_in, double* models_out, int& n_out)   the local estimator on the inliers of
//                    model_in; may run reductions of its own on the scope's stream
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "tri_math.h"  // TriSupport, tri_better
#include "call_scope.h"

// no contraction into fused multiply-adds from here on, as in the math headers of the problems: a residual rounds as written
#pragma clang fp contract(off)

namespace mpsfm {

constexpr int kLoT = 256;
constexpr int kLoWaves = kLoT / 64;
constexpr int kLoTile = 16;  // models per scoring workgroup
constexpr int kLoMaxBatch = 1 << 16;
constexpr uint64_t kLoPhi = 0x9E3779B97F4A7C15ull;

__host__ __device__ inline uint64_t lo_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__host__ __device__ inline uint64_t lo_mulhi(uint64_t a, uint64_t b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// the K distinct indices of trial t: the first K distinct draws (recipe in include/mpsfm_hip.h)
template <int K>
__host__ __device__ inline void lo_sample(uint64_t seed, int64_t t, int32_t n, int32_t idx[K]) {
  const uint64_t base = lo_mix(seed + (uint64_t)(t + 1) * kLoPhi);
  int k = 0;
  for (uint64_t j = 1; k < K; ++j) {
    const int32_t c = (int32_t)lo_mulhi(lo_mix(base + j * kLoPhi), (uint64_t)n);
    bool dup = false;
    for (int i = 0; i < k; ++i) dup = dup || idx[i] == c;
    if (!dup) idx[k++] = c;
  }
}

// RANSAC::ComputeNumTrials with kMinNumSamples = sample_size
inline int64_t lo_num_trials(int64_t num_inliers, int64_t n, double confidence, double multiplier, int sample_size) {
  const double ratio = (double)num_inliers / (double)n;
  const double nom = 1.0 - confidence;
  if (nom <= 0.0) return INT64_MAX;
  const double denom = 1.0 - pow(ratio, (double)sample_size);
  if (denom <= 0.0) return 1;
  if (denom == 1.0) return INT64_MAX;
  const double v = ceil(log(nom) / log(denom) * multiplier);
  return v >= 9.2e18 ? INT64_MAX : (int64_t)v;
}

inline bool lo_options_valid(const mpsfm_ransac_options& o) {
  return o.max_error > 0.0 && std::isfinite(o.max_error) && o.min_inlier_ratio > 0.0 && o.min_inlier_ratio <= 1.0 && o.confidence >= 0.0 &&
         o.confidence <= 1.0 && o.dyn_num_trials_multiplier > 0.0 && std::isfinite(o.dyn_num_trials_multiplier) && o.min_num_trials >= 0 &&
         o.max_num_trials >= 0 && o.min_num_trials <= o.max_num_trials && o.batch_trials >= 0 && o.batch_trials <= kLoMaxBatch;
}

inline bool finite_all(const double* a, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(a[i])) return false;
  return true;
}

// workgroups of a reduction over n observations: a function of n alone, so the summation order never changes
inline int lo_blocks(int32_t n, int per_block) { return (int)std::min<int64_t>(((int64_t)n + per_block - 1) / per_block, 64); }

// ---- fixed-order reductions ------------------------------------------------------------------------------------------
// (xor butterflies: every lane ends with the sum.  Not the __shfl_down wave_sum of sweep_common.h.)
__device__ __forceinline__ double lo_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ int lo_wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// The tail of a kernel of kLoT threads that reduces K values per thread to one row per workgroup: wave butterfly, then
// the waves in order -> part[blockIdx.x][K].  Every thread of the workgroup calls it (it holds the barrier).
template <int K, class T>
__device__ __forceinline__ void block_reduce_rows(const T (&acc)[K], T* __restrict__ part) {
  __shared__ T red[kLoWaves][K];
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const T s = lo_wave_sum(acc[k]);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += kLoT) {
    T s = 0;
    for (int w = 0; w < kLoWaves; ++w) s += red[w][k];
    part[(size_t)blockIdx.x * K + k] = s;
  }
}

// host: the workgroups' rows added in ascending block order
template <class T, class S>
inline void sum_rows(const T* part, int nblocks, int K, S* out) {
  for (int k = 0; k < K; ++k) {
    S s = 0;
    for (int b = 0; b < nblocks; ++b) s += part[(size_t)b * K + k];
    out[k] = s;
  }
}

// ---- scoring -----------------------------------------------------------------------------------------------------------
// The body of k_lo_score and of its batched form (two_view_batch.hip): workgroup blockIdx.x of the nblk along the n
// observations scores the tile of kLoTile models at blockIdx.y (models: the problem's first model) and writes the tile's row of
// partial counts and sums, part[model][nblk].  Every thread of the workgroup calls it (it holds two barriers).
template <class P>
__device__ __forceinline__ void lo_score_tile(const double* __restrict__ models, int32_t nmodels, int32_t n, const typename P::Pts& p, double thr2,
                                              int32_t nblk, int32_t* __restrict__ part_cnt, double* __restrict__ part_sum) {
  constexpr int K = P::kModel;
  __shared__ double sm[kLoTile * K];
  __shared__ double red_s[kLoWaves][kLoTile];
  __shared__ int red_c[kLoWaves][kLoTile];
  const int m0 = (int)blockIdx.y * kLoTile;
  for (int k = threadIdx.x; k < kLoTile * K; k += kLoT) {
    const int m = m0 + k / K;
    sm[k] = m < nmodels ? models[(size_t)m0 * K + k] : 0.0;
  }
  __syncthreads();
  int cnt[kLoTile];
  double sum[kLoTile];
#pragma unroll
  for (int m = 0; m < kLoTile; ++m) { cnt[m] = 0; sum[m] = 0.0; }
  for (int32_t i = (int32_t)blockIdx.x * kLoT + (int32_t)threadIdx.x; i < n; i += nblk * kLoT) {
    const typename P::Obs o = P::load(p, i);
#pragma unroll
    for (int m = 0; m < kLoTile; ++m) {
      const double r = P::residual(sm + K * m, o);
      if (r <= thr2) { cnt[m] += 1; sum[m] += r; }
    }
  }
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll
  for (int m = 0; m < kLoTile; ++m) {
    const int c = lo_wave_sum(cnt[m]);
    const double s = lo_wave_sum(sum[m]);
    if (lane == 0) { red_c[wave][m] = c; red_s[wave][m] = s; }
  }
  __syncthreads();
  if (threadIdx.x < kLoTile) {
    const int m = m0 + (int)threadIdx.x;
    int c = 0;
    double s = 0.0;
    for (int w = 0; w < kLoWaves; ++w) { c += red_c[w][threadIdx.x]; s += red_s[w][threadIdx.x]; }
    if (m < nmodels) { part_cnt[(size_t)m * nblk + blockIdx.x] = c; part_sum[(size_t)m * nblk + blockIdx.x] = s; }
  }
}

template <class P>
__global__ __launch_bounds__(kLoT) void k_lo_score(const double* __restrict__ models, int32_t nmodels, int32_t n, typename P::Pts p, double thr2,
                                                    int32_t* __restrict__ part_cnt, double* __restrict__ part_sum) {
  lo_score_tile<P>(models, nmodels, n, p, thr2, (int32_t)gridDim.x, part_cnt, part_sum);
}

// The body of k_lo_score_sum and of its batched form: a model's row of nparts partial counts and sums, added in ascending
// block order
__device__ __forceinline__ void lo_score_sum_row(const int32_t* __restrict__ part_cnt, const double* __restrict__ part_sum, int32_t nparts,
                                                 int32_t* __restrict__ cnt, double* __restrict__ sum) {
  int c = 0;
  double s = 0.0;
  for (int b = 0; b < nparts; ++b) { c += part_cnt[b]; s += part_sum[b]; }
  *cnt = c;
  *sum = s;
}

static __global__ __launch_bounds__(kLoT) void k_lo_score_sum(const int32_t* __restrict__ part_cnt, const double* __restrict__ part_sum,
                                                               int32_t nmodels, int32_t nparts, int32_t* __restrict__ cnt, double* __restrict__ sum) {
  const int32_t m = (int32_t)blockIdx.x * kLoT + (int32_t)threadIdx.x;
  if (m >= nmodels) return;
  lo_score_sum_row(part_cnt + (size_t)m * nparts, part_sum + (size_t)m * nparts, nparts, cnt + m, sum + m);
}

template <int K> struct LoModel { double m[K]; };

template <class P>
__global__ __launch_bounds__(kLoT) void k_lo_mask(LoModel<P::kModel> M, int32_t n, typename P::Pts p, double thr2, uint8_t* __restrict__ mask) {
  const int32_t i = (int32_t)blockIdx.x * kLoT + (int32_t)threadIdx.x;
  if (i >= n) return;
  mask[i] = P::residual(M.m, P::load(p, i)) <= thr2 ? 1 : 0;
}

// queues the mask of `model` over the problem's observations on the scope's stream
template <class P>
int lo_mask(const P& prob, CallScope& A, const double* model, uint8_t* d_mask) {
  LoModel<P::kModel> M;
  std::memcpy(M.m, model, sizeof(M.m));
  hipLaunchKernelGGL(k_lo_mask<P>, dim3((unsigned)((prob.n + kLoT - 1) / kLoT)), dim3(kLoT), 0, A.st, M, prob.n, prob.pts, prob.thr2, d_mask);
  MPSFM_TRY(hipGetLastError());
  return 0;
}

// ---- the loop --------------------------------------------------------------------------------------------------------
struct LoReport {
  TriSupport best{0, DBL_MAX};
  int64_t num_trials = 0, max_num_trials = 0, num_models = 0, lo_rounds = 0, num_batches = 0;
};

// the trials a call runs at most: max_num_trials, or what min_inlier_ratio needs at the call's confidence
inline int64_t lo_max_trials(const mpsfm_ransac_options& o, int sample) {
  return std::min<int64_t>(o.max_num_trials, lo_num_trials((int64_t)(o.min_inlier_ratio * 100000.0), 100000, o.confidence, o.dyn_num_trials_multiplier, sample));
}
// trials per batch: batch_trials or the problem's default, at most the call's trials
template <class P>
int64_t lo_batch_cap(const mpsfm_ransac_options& o) {
  const int32_t B = o.batch_trials > 0 ? o.batch_trials : P::kDefaultBatch;
  return std::max<int64_t>(1, std::min<int64_t>(B, lo_max_trials(o, P::kSample)));
}

// best_model [P::kModel]: meaningful when rep.best.num_inliers >= P::kSample.  The scope is open and timed.
template <class P>
int lo_ransac(P& prob, CallScope& A, const mpsfm_ransac_options& o, LoReport& rep, double* best_model) {
  constexpr int K = P::kModel, S = P::kSlots, L = P::kLocal;
  static_assert(L <= S, "the local models are scored in the partial rows of one trial");
  const int32_t n = prob.n;
  const int64_t max_trials = lo_max_trials(o, P::kSample);
  const int32_t Bcap = (int32_t)lo_batch_cap<P>(o);
  const int32_t Mcap = S * Bcap;             // batch models; L more slots after them for the local models
  const int nbx = lo_blocks(n, 4 * kLoT);    // scoring workgroups along the observations

  double* d_models = A.alloc<double>((size_t)K * ((size_t)Mcap + L));
  int32_t* d_nmod = A.alloc<int32_t>((size_t)Bcap);
  int32_t* d_pcnt = A.alloc<int32_t>((size_t)Mcap * nbx);
  double* d_psum = A.alloc<double>((size_t)Mcap * nbx);
  int32_t* d_cnt = A.alloc<int32_t>((size_t)Mcap);
  double* d_sum = A.alloc<double>((size_t)Mcap);
  if (!d_models || !d_nmod || !d_pcnt || !d_psum || !d_cnt || !d_sum) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  double* d_local = d_models + (size_t)K * Mcap;

  std::vector<double> h_models((size_t)K * Mcap), h_sum((size_t)Mcap);
  std::vector<int32_t> h_nmod((size_t)Bcap), h_cnt((size_t)Mcap);

  // scores M models at dm: counts and sums into hc / hsum [0, M)
  auto score = [&](const double* dm, int32_t M, int32_t* hc, double* hsum) -> int {
    const dim3 grid((unsigned)nbx, (unsigned)((M + kLoTile - 1) / kLoTile));
    hipLaunchKernelGGL(k_lo_score<P>, grid, dim3(kLoT), 0, A.st, dm, M, n, prob.pts, prob.thr2, d_pcnt, d_psum);
    MPSFM_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_lo_score_sum, dim3((unsigned)((M + kLoT - 1) / kLoT)), dim3(kLoT), 0, A.st, d_pcnt, d_psum, M, nbx, d_cnt, d_sum);
    MPSFM_TRY(hipGetLastError());
    MPSFM_TRY(hipMemcpyAsync(hc, d_cnt, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToHost, A.st));
    MPSFM_TRY(hipMemcpyAsync(hsum, d_sum, sizeof(double) * (size_t)M, hipMemcpyDeviceToHost, A.st));
    return 0;
  };

  TriSupport& best = rep.best;
  int64_t dyn = max_trials, trials = 0, b0 = 0, bn = 0;
  bool abort_ = false;
  for (trials = 0; trials < max_trials; ++trials) {
    if (abort_) { trials += 1; break; }
    if (trials >= b0 + bn) {  // next batch: generate, score, download the table
      b0 = trials;
      bn = std::min<int64_t>(Bcap, max_trials - trials);
      const int32_t M = S * (int32_t)bn;
      if (int rc = A.begin()) return rc;
      prob.minimal(A.st, o.seed, b0, (int32_t)bn, d_models, d_nmod);
      MPSFM_TRY(hipGetLastError());
      if (int rc = score(d_models, M, h_cnt.data(), h_sum.data())) return rc;
      MPSFM_TRY(hipMemcpyAsync(h_nmod.data(), d_nmod, sizeof(int32_t) * (size_t)bn, hipMemcpyDeviceToHost, A.st));
      MPSFM_TRY(hipMemcpyAsync(h_models.data(), d_models, sizeof(double) * K * (size_t)M, hipMemcpyDeviceToHost, A.st));
      if (int rc = A.end()) return rc;
      ++rep.num_batches;
      rep.num_models += M;
    }
    const int64_t lt = trials - b0;
    for (int k = 0; k < h_nmod[(size_t)lt]; ++k) {
      const size_t slot = (size_t)S * lt + k;
      const TriSupport sup{h_cnt[slot], h_sum[slot]};
      if (tri_better(sup, best)) {
        best = sup;
        std::memcpy(best_model, &h_models[K * slot], sizeof(double) * K);
        // local optimisation (kMaxNumLocalTrials = 10); more inliers than the sample is also what the local estimators need
        if (sup.num_inliers > P::kSample) {
          for (int round = 0; round < 10; ++round) {
            const int prev = best.num_inliers;
            double Lm[K * L];
            int nl = 0;
            ++rep.lo_rounds;
            if (int rc = prob.local(A, best_model, Lm, nl)) return rc;
            if (nl > 0) {
              MPSFM_TRY(hipMemcpyAsync(d_local, Lm, sizeof(double) * K * (size_t)nl, hipMemcpyHostToDevice, A.st));
              if (int rc = A.begin()) return rc;
              int32_t lc[L];  // the batch's table in h_cnt / h_sum is still being replayed
              double ls_[L];
              if (int rc = score(d_local, nl, lc, ls_)) return rc;
              if (int rc = A.end()) return rc;
              for (int j = 0; j < nl; ++j) {
                const TriSupport ls{lc[j], ls_[j]};
                if (tri_better(ls, best)) {
                  best = ls;
                  std::memcpy(best_model, Lm + K * j, sizeof(double) * K);
                }
              }
            }
            if (best.num_inliers <= prev) break;
          }
        }
        dyn = lo_num_trials(best.num_inliers, n, o.confidence, o.dyn_num_trials_multiplier, P::kSample);
      }
      if (trials >= dyn && trials >= o.min_num_trials) { abort_ = true; break; }
    }
  }
  rep.num_trials = trials;
  rep.max_num_trials = max_trials;
  return 0;
}

}  // namespace mpsfm
