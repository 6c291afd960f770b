// Calibrated two-view geometry of many image pairs in one call (mpsfm_two_view_geometry_batch; include/mpsfm_hip.h, DESIGN.md
// section 4k): the pairs of a group run every leg as one lockstep LO-RANSAC.  Each kernel here is a single-pair kernel of
// two_view_problem.h / rel_pose_problem.h / lo_ransac.h with one more grid dimension, the problem, and a descriptor table in
// place of the by-value arguments: it reads its problem's row and calls the body the single-pair kernel calls, so every pair's
// result is bitwise that of mpsfm_two_view_geometry.  f64 throughout.
#include "two_view_problem.h"

namespace mpsfm {

namespace {
// The descriptor of one problem in one launch.  Every workgroup reads its problem's descriptor and then does what the
// single-pair kernel does for that problem, with the problem's own block count (nblk) where the single-pair kernel reads
// gridDim.x; workgroups beyond a problem's extent leave at once.
struct BtDesc {
  double model[9];   // reductions, mask: the model (2 values for the translation)
  double centre[4];  // k_bt_gram
  double thr2;
  uint64_t seed;
  int64_t t0;        // minimal: first trial of the batch
  int64_t base;      // the problem's SoA block u1 v1 u2 v2 (n each) starts at pts + base
  int64_t mod_off;   // minimal, score: the problem's first model in the model table
  int64_t nmod_off;  // minimal: the problem's first trial in the table of model counts
  int64_t part_off;  // score: first entry of the partial counts / sums; reductions: first partial row
  int64_t out_off;   // sum: first count / sum; mask: first byte
  int32_t n, nb, nmodels, nblk;  // observations, trials, models to score, observation blocks (a function of n alone)
};
static_assert(sizeof(BtDesc) == 184, "BtDesc is uploaded as an array");

__device__ __forceinline__ RpPts bt_pts(const double* __restrict__ pts, const BtDesc& d) {
  const double* b = pts + d.base;
  return RpPts{b, b + d.n, b + 2 * (size_t)d.n, b + 3 * (size_t)d.n};
}

// the minimal solvers over (trial, problem)
__global__ __launch_bounds__(kFiveT) void k_bt_five(const BtDesc* __restrict__ D, const double* __restrict__ pts, double* __restrict__ models,
                                                     int32_t* __restrict__ nmod) {
  const BtDesc& d = D[blockIdx.y];
  const int32_t i = (int32_t)blockIdx.x * kFiveT + (int32_t)threadIdx.x;
  if (i >= d.nb) return;
  rp_five_trial(d.seed, d.t0 + i, d.n, bt_pts(pts, d), models + ((size_t)d.mod_off + (size_t)i * kRpMaxModels) * 9, nmod + d.nmod_off + i);
}

__global__ __launch_bounds__(kSevenT) void k_bt_f7(const BtDesc* __restrict__ D, const double* __restrict__ pts, double* __restrict__ models,
                                                    int32_t* __restrict__ nmod) {
  const BtDesc& d = D[blockIdx.y];
  const int32_t i = (int32_t)blockIdx.x * kSevenT + (int32_t)threadIdx.x;
  if (i >= d.nb) return;
  tv_f7_trial(d.seed, d.t0 + i, d.n, bt_pts(pts, d), models + ((size_t)d.mod_off + (size_t)i * kTvFMaxModels) * 9, nmod + d.nmod_off + i);
}

__global__ __launch_bounds__(kFourT) void k_bt_h4(const BtDesc* __restrict__ D, const double* __restrict__ pts, double* __restrict__ models,
                                                   int32_t* __restrict__ nmod) {
  const BtDesc& d = D[blockIdx.y];
  const int32_t i = (int32_t)blockIdx.x * kFourT + (int32_t)threadIdx.x;
  if (i >= d.nb) return;
  tv_h4_trial(d.seed, d.t0 + i, d.n, bt_pts(pts, d), models + ((size_t)d.mod_off + (size_t)i) * 9, nmod + d.nmod_off + i);
}

__global__ __launch_bounds__(kLoT) void k_bt_t1(const BtDesc* __restrict__ D, const double* __restrict__ pts, double* __restrict__ models,
                                                 int32_t* __restrict__ nmod) {
  const BtDesc& d = D[blockIdx.y];
  const int32_t i = (int32_t)blockIdx.x * kLoT + (int32_t)threadIdx.x;
  if (i >= d.nb) return;
  tv_t1_trial(d.seed, d.t0 + i, d.n, bt_pts(pts, d), models + ((size_t)d.mod_off + (size_t)i) * 2, nmod + d.nmod_off + i);
}

// k_lo_score over (observation block, model tile, problem)
template <class P>
__global__ __launch_bounds__(kLoT) void k_bt_score(const BtDesc* __restrict__ D, const double* __restrict__ pts, const double* __restrict__ models,
                                                    int32_t* __restrict__ part_cnt, double* __restrict__ part_sum) {
  const BtDesc& d = D[blockIdx.z];
  if ((int32_t)blockIdx.x >= d.nblk || (int)blockIdx.y * kLoTile >= d.nmodels) return;
  lo_score_tile<P>(models + (size_t)d.mod_off * P::kModel, d.nmodels, d.n, bt_pts(pts, d), d.thr2, d.nblk, part_cnt + d.part_off,
                   part_sum + d.part_off);
}

// k_lo_score_sum over (model, problem)
__global__ __launch_bounds__(kLoT) void k_bt_sum(const BtDesc* __restrict__ D, const int32_t* __restrict__ part_cnt, const double* __restrict__ part_sum,
                                                  int32_t* __restrict__ cnt, double* __restrict__ sum) {
  const BtDesc& d = D[blockIdx.y];
  const int32_t m = (int32_t)blockIdx.x * kLoT + (int32_t)threadIdx.x;
  if (m >= d.nmodels) return;
  const size_t at = (size_t)d.part_off + (size_t)m * d.nblk;
  lo_score_sum_row(part_cnt + at, part_sum + at, d.nblk, cnt + d.out_off + m, sum + d.out_off + m);
}

// the reductions of the local estimators over (observation block, problem): k_tv_moments, k_tv_gram, k_rp_gram, k_tv_tsum
template <bool kHomography>
__global__ __launch_bounds__(kLoT) void k_bt_moments(const BtDesc* __restrict__ D, const double* __restrict__ pts, double* __restrict__ part) {
  const BtDesc& d = D[blockIdx.y];
  if ((int32_t)blockIdx.x >= d.nblk) return;
  tv_moments_block<kHomography>(d.model, d.thr2, d.n, bt_pts(pts, d), d.nblk, part + (size_t)d.part_off * kMomK);
}

template <bool kHomography>
__global__ __launch_bounds__(kLoT) void k_bt_gram(const BtDesc* __restrict__ D, const double* __restrict__ pts, double* __restrict__ part) {
  const BtDesc& d = D[blockIdx.y];
  if ((int32_t)blockIdx.x >= d.nblk) return;
  const TvCentre c{d.centre[0], d.centre[1], d.centre[2], d.centre[3]};
  tv_gram_block<kHomography>(d.model, d.thr2, d.n, bt_pts(pts, d), c, d.nblk, part + (size_t)d.part_off * kGram9K);
}

__global__ __launch_bounds__(kLoT) void k_bt_egram(const BtDesc* __restrict__ D, const double* __restrict__ pts, double* __restrict__ part) {
  const BtDesc& d = D[blockIdx.y];
  if ((int32_t)blockIdx.x >= d.nblk) return;
  rp_gram_block(d.model, d.thr2, d.n, bt_pts(pts, d), d.nblk, part + (size_t)d.part_off * kGramK);
}

__global__ __launch_bounds__(kLoT) void k_bt_tsum(const BtDesc* __restrict__ D, const double* __restrict__ pts, double* __restrict__ part) {
  const BtDesc& d = D[blockIdx.y];
  if ((int32_t)blockIdx.x >= d.nblk) return;
  tv_tsum_block(d.model, d.thr2, d.n, bt_pts(pts, d), d.nblk, part + (size_t)d.part_off * kTsumK);
}

// k_lo_mask over (observation, problem): one line of P's own functions, kept as its own text
template <class P>
__global__ __launch_bounds__(kLoT) void k_bt_mask(const BtDesc* __restrict__ D, const double* __restrict__ pts, uint8_t* __restrict__ mask) {
  const BtDesc& d = D[blockIdx.y];
  const int32_t i = (int32_t)blockIdx.x * kLoT + (int32_t)threadIdx.x;
  if (i >= d.n) return;
  mask[(size_t)d.out_off + i] = P::residual(d.model, P::load(bt_pts(pts, d), i)) <= d.thr2 ? 1 : 0;
}

struct BtPoseDesc {
  TvCands c;
  int64_t base, mask_off, part_off /* rows of 4 */, angle_off;
  int32_t n, nblk;
};

// k_tv_pose over (observation block, pair)
__global__ __launch_bounds__(kLoT) void k_bt_pose(const BtPoseDesc* __restrict__ D, const double* __restrict__ pts, const uint8_t* __restrict__ mask_all,
                                                   int32_t* __restrict__ part, double* __restrict__ angle_all) {
  const BtPoseDesc& d = D[blockIdx.y];
  if ((int32_t)blockIdx.x >= d.nblk) return;
  const double* pb = pts + d.base;
  const RpPts p{pb, pb + d.n, pb + 2 * (size_t)d.n, pb + 3 * (size_t)d.n};
  tv_pose_block(d.c, d.n, p, mask_all + d.mask_off, d.nblk, part + (size_t)d.part_off * 4, angle_all + d.angle_off);
}

// ---- the lockstep engine ---------------------------------------------------------------------------------------------------
// what a call counts, and the descriptor ring of the launches between two synchronisations
struct BtCtx {
  CallScope& A;
  int64_t syncs = 0, launches = 0;
  std::vector<BtDesc> h_desc;  // stays in place until the synchronisation: the uploads read it
  BtDesc* d_desc = nullptr;
  size_t used = 0;

  explicit BtCtx(CallScope& a) : A(a) {}
  int reserve(size_t cap) {
    h_desc.resize(cap);
    d_desc = A.alloc<BtDesc>(cap);
    return d_desc ? 0 : fail(MPSFM_ENOMEM, "hipMalloc failed");
  }
  // the next `count` descriptors of the ring: fill, then up()
  BtDesc* next(size_t count) {
    if (used + count > h_desc.size()) return nullptr;
    for (size_t i = 0; i < count; ++i) h_desc[used + i] = BtDesc{};
    return h_desc.data() + used;
  }
  int up(size_t count, const BtDesc** dev) {
    *dev = d_desc + used;
    MPSFM_TRY(hipMemcpyAsync(d_desc + used, h_desc.data() + used, sizeof(BtDesc) * count, hipMemcpyHostToDevice, A.st));
    used += count;
    return 0;
  }
  int end() {
    used = 0;
    ++syncs;
    return A.end();
  }
};

enum { kBtHead = 0, kBtBatchLoaded, kBtModel, kBtLoRound, kBtLoScored, kBtAfterLo, kBtCheck };
enum { kBtNeedBatch = 1, kBtNeedLo = 2, kBtDone = 3 };

// one problem of a leg: lo_ransac's loop variables, where its replay stands, and where its tables are
struct BtProb {
  int64_t pair = 0;  // index into the call's pairs
  int32_t n = 0;
  double thr2 = 0.0;
  int64_t base = 0;
  int nbx = 0, npx = 0;            // lo_blocks(n, 4 kLoT), lo_blocks(n, kLoT)
  int64_t part_off = 0, red_off = 0;
  LoReport rep;
  double best_model[9] = {};
  int64_t dyn = 0, trials = 0, b0 = 0, bn = 0;
  bool abort_ = false;
  int pc = kBtHead, need = 0, k = 0, round = 0, prev = 0;
  int nl = 0;        // models of the current local estimate
  double Lm[9 * kRpMaxModels];
  int32_t lc[kRpMaxModels];
  double ls[kRpMaxModels];
  double mom[kMomK];
};

// lo_ransac's loop for one problem, resumable: runs the replay of the problem's downloaded table (its row of h_*) until the
// problem needs its next batch (kBtNeedBatch), a round of its local optimisation (kBtNeedLo: the driver leaves the round's
// models in Lm / lc / ls) or is over (kBtDone).  Statement for statement the loop of lo_ransac.
template <class P>
int bt_replay(BtProb& s, const mpsfm_ransac_options& o, int64_t max_trials, const int32_t* h_nmod, const int32_t* h_cnt, const double* h_sum,
              const double* h_models) {
  constexpr int K = P::kModel, S = P::kSlots;
  TriSupport& best = s.rep.best;
  for (;;) {
    switch (s.pc) {
      case kBtHead:
        if (!(s.trials < max_trials) || s.abort_) {
          if (s.trials < max_trials) s.trials += 1;
          s.rep.num_trials = s.trials;
          s.rep.max_num_trials = max_trials;
          return s.need = kBtDone;
        }
        s.pc = kBtBatchLoaded;
        if (s.trials >= s.b0 + s.bn) return s.need = kBtNeedBatch;
        break;
      case kBtBatchLoaded:
        s.k = 0;
        s.pc = kBtModel;
        break;
      case kBtModel: {
        const int64_t lt = s.trials - s.b0;
        if (s.k >= h_nmod[(size_t)lt]) {
          ++s.trials;
          s.pc = kBtHead;
          break;
        }
        const size_t slot = (size_t)S * lt + s.k;
        const TriSupport sup{h_cnt[slot], h_sum[slot]};
        s.pc = kBtCheck;
        if (tri_better(sup, best)) {
          best = sup;
          std::memcpy(s.best_model, &h_models[K * slot], sizeof(double) * K);
          s.round = 0;
          s.pc = sup.num_inliers > P::kSample ? kBtLoRound : kBtAfterLo;
        }
        break;
      }
      case kBtLoRound:
        if (s.round >= 10) { s.pc = kBtAfterLo; break; }
        s.prev = (int)best.num_inliers;
        ++s.rep.lo_rounds;
        s.nl = 0;
        s.pc = kBtLoScored;
        return s.need = kBtNeedLo;
      case kBtLoScored:
        for (int j = 0; j < s.nl; ++j) {
          const TriSupport ls{s.lc[j], s.ls[j]};
          if (tri_better(ls, best)) {
            best = ls;
            std::memcpy(s.best_model, s.Lm + K * j, sizeof(double) * K);
          }
        }
        if (best.num_inliers <= s.prev) { s.pc = kBtAfterLo; break; }
        ++s.round;
        s.pc = kBtLoRound;
        break;
      case kBtAfterLo:
        s.dyn = lo_num_trials(best.num_inliers, s.n, o.confidence, o.dyn_num_trials_multiplier, P::kSample);
        s.pc = kBtCheck;
        break;
      case kBtCheck:
        if (s.trials >= s.dyn && s.trials >= o.min_num_trials) {
          s.abort_ = true;
          ++s.trials;
          s.pc = kBtHead;
          break;
        }
        ++s.k;
        s.pc = kBtModel;
        break;
    }
  }
}

// the reduction row length of a leg's local estimator; its host half is P::local_models (and P::enough, P::centre where the
// estimator has a moments stage), the functions P::local calls
template <class P> struct BtLeg;
template <> struct BtLeg<RpProblem> { static constexpr int kRed = kGramK; };
template <bool kH> struct BtLeg<TvProblem<kH>> { static constexpr int kRed = kGram9K; };
template <> struct BtLeg<TvTranslation> { static constexpr int kRed = kTsumK; };

// device bytes of a problem's tables on a leg: models, partial counts and sums, counts and sums
template <class P>
size_t bt_leg_bytes(int32_t n, int64_t Bcap) {
  const size_t M = (size_t)P::kSlots * (size_t)Bcap;
  return M * (size_t)lo_blocks(n, 4 * kLoT) * 12 + M * (P::kModel * 8 + 12) + (size_t)Bcap * 4;
}

// One leg type over the problems `pr` (ascending pair order) of a group, in lockstep: every step generates, scores and
// downloads the next batch of every problem that needs one, with one synchronisation; the problems then replay their tables
// until they need a local optimisation, whose rounds run together stage by stage, one synchronisation per stage.
template <class P>
int bt_leg(BtCtx& X, const mpsfm_ransac_options& o, const double* d_pts, std::vector<BtProb>& pr) {
  constexpr int K = P::kModel, S = P::kSlots, L = P::kLocal, R = BtLeg<P>::kRed;
  static_assert(L <= kRpMaxModels && K <= 9, "BtProb's local tables");
  const size_t np = pr.size();
  if (np == 0) return 0;
  CallScope& A = X.A;
  const int64_t max_trials = lo_max_trials(o, P::kSample);
  const int64_t Bcap = lo_batch_cap<P>(o);
  const int64_t Mcap = S * Bcap;
  int64_t parts = 0, reds = 0;
  int max_nbx = 0, max_npx = 0;
  for (BtProb& s : pr) {
    s.nbx = lo_blocks(s.n, 4 * kLoT);
    s.npx = lo_blocks(s.n, kLoT);
    s.part_off = parts;
    s.red_off = reds;
    parts += Mcap * s.nbx;
    reds += s.npx;
    s.dyn = max_trials;
    max_nbx = std::max(max_nbx, s.nbx);
    max_npx = std::max(max_npx, s.npx);
  }
  double* d_models = A.alloc<double>((size_t)K * Mcap * np);
  double* d_local = A.alloc<double>((size_t)K * L * np);
  int32_t* d_nmod = A.alloc<int32_t>((size_t)Bcap * np);
  int32_t* d_pcnt = A.alloc<int32_t>((size_t)parts);
  double* d_psum = A.alloc<double>((size_t)parts);
  int32_t* d_cnt = A.alloc<int32_t>((size_t)Mcap * np);
  double* d_sum = A.alloc<double>((size_t)Mcap * np);
  int32_t* d_lcnt = A.alloc<int32_t>((size_t)L * np);
  double* d_lsum = A.alloc<double>((size_t)L * np);
  double* d_red = A.alloc<double>((size_t)R * reds);
  if (!d_models || !d_local || !d_nmod || !d_pcnt || !d_psum || !d_cnt || !d_sum || !d_lcnt || !d_lsum || !d_red)
    return fail(MPSFM_ENOMEM, "hipMalloc failed");
  std::vector<double> h_models((size_t)K * Mcap * np), h_sum((size_t)Mcap * np), h_local((size_t)K * L * np), h_lsum((size_t)L * np),
      h_red((size_t)R * reds);
  std::vector<int32_t> h_nmod((size_t)Bcap * np), h_cnt((size_t)Mcap * np), h_lcnt((size_t)L * np);

  auto replay = [&](size_t i) {
    return bt_replay<P>(pr[i], o, max_trials, &h_nmod[(size_t)Bcap * i], &h_cnt[(size_t)Mcap * i], &h_sum[(size_t)Mcap * i],
                        &h_models[(size_t)K * Mcap * i]);
  };
  // device rows [first, last] of a per-problem table of `per` elements -> the same rows of the host table
  auto down_rows = [&](void* host, const void* dev, size_t elem, size_t per, size_t first, size_t last) -> int {
    MPSFM_TRY(hipMemcpyAsync((char*)host + elem * per * first, (const char*)dev + elem * per * first, elem * per * (last - first + 1),
                             hipMemcpyDeviceToHost, A.st));
    return 0;
  };
  // `who` in runs of consecutive problems: one copy per run and table
  auto for_runs = [&](const std::vector<size_t>& who, auto&& fn) -> int {
    for (size_t a = 0; a < who.size();) {
      size_t b = a;
      while (b + 1 < who.size() && who[b + 1] == who[b] + 1) ++b;
      if (int rc = fn(who[a], who[b])) return rc;
      a = b + 1;
    }
    return 0;
  };
  // scores desc.nmodels models per descriptor (the descriptors are on the device): partial rows, then their sums
  auto score = [&](const BtDesc* dd, size_t count, int max_models, const double* dm, int32_t* dc, double* ds) -> int {
    const dim3 grid((unsigned)max_nbx, (unsigned)((max_models + kLoTile - 1) / kLoTile), (unsigned)count);
    hipLaunchKernelGGL(k_bt_score<P>, grid, dim3(kLoT), 0, A.st, dd, d_pts, dm, d_pcnt, d_psum);
    MPSFM_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_bt_sum, dim3((unsigned)((max_models + kLoT - 1) / kLoT), (unsigned)count), dim3(kLoT), 0, A.st, dd, d_pcnt, d_psum, dc, ds);
    MPSFM_TRY(hipGetLastError());
    X.launches += 2;
    return 0;
  };
  auto base_desc = [&](BtDesc& d, size_t i) {
    const BtProb& s = pr[i];
    d.thr2 = s.thr2;
    d.seed = o.seed;
    d.base = s.base;
    d.n = s.n;
    std::memcpy(d.model, s.best_model, sizeof(double) * K);
  };

  // the next batch of every problem of `who`
  auto step = [&](const std::vector<size_t>& who) -> int {
    BtDesc* hd = X.next(who.size());
    if (!hd) return fail(MPSFM_ENOMEM, "descriptor ring too small");
    int64_t max_bn = 0;
    for (size_t j = 0; j < who.size(); ++j) {
      const size_t i = who[j];
      BtProb& s = pr[i];
      s.b0 = s.trials;
      s.bn = std::min<int64_t>(Bcap, max_trials - s.trials);
      max_bn = std::max(max_bn, s.bn);
      BtDesc& d = hd[j];
      base_desc(d, i);
      d.t0 = s.b0;
      d.nb = (int32_t)s.bn;
      d.nmodels = S * (int32_t)s.bn;
      d.nblk = s.nbx;
      d.mod_off = Mcap * (int64_t)i;
      d.nmod_off = Bcap * (int64_t)i;
      d.part_off = s.part_off;
      d.out_off = Mcap * (int64_t)i;
      ++s.rep.num_batches;
      s.rep.num_models += d.nmodels;
    }
    const BtDesc* dd = nullptr;
    if (int rc = X.up(who.size(), &dd)) return rc;
    if (int rc = A.begin()) return rc;
    const unsigned np_ = (unsigned)who.size();
    if constexpr (std::is_same<P, RpProblem>::value)
      hipLaunchKernelGGL(k_bt_five, dim3((unsigned)((max_bn + kFiveT - 1) / kFiveT), np_), dim3(kFiveT), 0, A.st, dd, d_pts, d_models, d_nmod);
    else if constexpr (std::is_same<P, TvProblem<false>>::value)
      hipLaunchKernelGGL(k_bt_f7, dim3((unsigned)((max_bn + kSevenT - 1) / kSevenT), np_), dim3(kSevenT), 0, A.st, dd, d_pts, d_models, d_nmod);
    else if constexpr (std::is_same<P, TvProblem<true>>::value)
      hipLaunchKernelGGL(k_bt_h4, dim3((unsigned)((max_bn + kFourT - 1) / kFourT), np_), dim3(kFourT), 0, A.st, dd, d_pts, d_models, d_nmod);
    else
      hipLaunchKernelGGL(k_bt_t1, dim3((unsigned)((max_bn + kLoT - 1) / kLoT), np_), dim3(kLoT), 0, A.st, dd, d_pts, d_models, d_nmod);
    MPSFM_TRY(hipGetLastError());
    X.launches += 1;
    if (int rc = score(dd, who.size(), S * (int)max_bn, d_models, d_cnt, d_sum)) return rc;
    if (int rc = for_runs(who, [&](size_t a, size_t b) -> int {
          if (int rc = down_rows(h_nmod.data(), d_nmod, sizeof(int32_t), (size_t)Bcap, a, b)) return rc;
          if (int rc = down_rows(h_models.data(), d_models, sizeof(double), (size_t)K * Mcap, a, b)) return rc;
          if (int rc = down_rows(h_cnt.data(), d_cnt, sizeof(int32_t), (size_t)Mcap, a, b)) return rc;
          return down_rows(h_sum.data(), d_sum, sizeof(double), (size_t)Mcap, a, b);
        }))
      return rc;
    return X.end();
  };

  // one reduction stage of the local estimators of `who` (stage 0: moments of F / H; 1: the Gram matrix, or the sums of the
  // translation): the partial rows of every problem come down in one copy
  auto reduce = [&](const std::vector<size_t>& who, int stage) -> int {
    BtDesc* hd = X.next(who.size());
    if (!hd) return fail(MPSFM_ENOMEM, "descriptor ring too small");
    for (size_t j = 0; j < who.size(); ++j) {
      const BtProb& s = pr[who[j]];
      BtDesc& d = hd[j];
      base_desc(d, who[j]);
      d.nblk = s.npx;
      d.part_off = s.red_off;
      if constexpr (R == kGram9K)
        if (stage == 1) {
          const TvCentre c = P::centre(s.mom);
          d.centre[0] = c.c1x; d.centre[1] = c.c1y; d.centre[2] = c.c2x; d.centre[3] = c.c2y;
        }
    }
    const BtDesc* dd = nullptr;
    if (int rc = X.up(who.size(), &dd)) return rc;
    if (int rc = A.begin()) return rc;
    const dim3 grid((unsigned)max_npx, (unsigned)who.size());
    int rk = R;
    if constexpr (std::is_same<P, RpProblem>::value) {
      hipLaunchKernelGGL(k_bt_egram, grid, dim3(kLoT), 0, A.st, dd, d_pts, d_red);
    } else if constexpr (std::is_same<P, TvTranslation>::value) {
      hipLaunchKernelGGL(k_bt_tsum, grid, dim3(kLoT), 0, A.st, dd, d_pts, d_red);
    } else {
      constexpr bool kH = std::is_same<P, TvProblem<true>>::value;
      if (stage == 0) {
        rk = kMomK;
        hipLaunchKernelGGL(k_bt_moments<kH>, grid, dim3(kLoT), 0, A.st, dd, d_pts, d_red);
      } else {
        hipLaunchKernelGGL(k_bt_gram<kH>, grid, dim3(kLoT), 0, A.st, dd, d_pts, d_red);
      }
    }
    MPSFM_TRY(hipGetLastError());
    X.launches += 1;
    const BtProb &f = pr[who.front()], &l = pr[who.back()];
    const size_t lo = (size_t)rk * f.red_off, hi = (size_t)rk * (l.red_off + l.npx);
    MPSFM_TRY(hipMemcpyAsync(h_red.data() + lo, d_red + lo, sizeof(double) * (hi - lo), hipMemcpyDeviceToHost, A.st));
    return X.end();
  };

  // one round of the local optimisation of every problem of `who`: P::local's steps, each for all of them at once
  auto lo_round = [&](const std::vector<size_t>& who) -> int {
    std::vector<size_t> cur = who, nxt;
    if constexpr (R == kGram9K) {  // F, H: moments first
      if (int rc = reduce(cur, 0)) return rc;
      for (size_t i : cur) {
        BtProb& s = pr[i];
        sum_rows(h_red.data() + (size_t)kMomK * s.red_off, s.npx, kMomK, s.mom);
        if (P::enough(s.mom)) nxt.push_back(i);
      }
      cur.swap(nxt);
      nxt.clear();
    }
    if (!cur.empty()) {
      if (int rc = reduce(cur, 1)) return rc;
      for (size_t i : cur) {
        BtProb& s = pr[i];
        double g[R];
        sum_rows(h_red.data() + (size_t)R * s.red_off, s.npx, R, g);
        s.nl = P::local_models(s.mom, g, s.Lm);
        if (s.nl > 0) nxt.push_back(i);
      }
      cur.swap(nxt);
    }
    if (cur.empty()) return 0;
    // the local models of all problems in one upload, one scoring launch, one download
    BtDesc* hd = X.next(cur.size());
    if (!hd) return fail(MPSFM_ENOMEM, "descriptor ring too small");
    int max_nl = 0;
    for (size_t j = 0; j < cur.size(); ++j) {
      const size_t i = cur[j];
      const BtProb& s = pr[i];
      std::memcpy(&h_local[(size_t)K * L * i], s.Lm, sizeof(double) * K * (size_t)s.nl);
      BtDesc& d = hd[j];
      base_desc(d, i);
      d.nmodels = s.nl;
      d.nblk = s.nbx;
      d.mod_off = (int64_t)L * (int64_t)i;
      d.part_off = s.part_off;
      d.out_off = (int64_t)L * (int64_t)i;
      max_nl = std::max(max_nl, s.nl);
    }
    const size_t a = cur.front(), b = cur.back();
    MPSFM_TRY(hipMemcpyAsync(d_local + (size_t)K * L * a, &h_local[(size_t)K * L * a], sizeof(double) * K * L * (b - a + 1), hipMemcpyHostToDevice, A.st));
    const BtDesc* dd = nullptr;
    if (int rc = X.up(cur.size(), &dd)) return rc;
    if (int rc = A.begin()) return rc;
    if (int rc = score(dd, cur.size(), max_nl, d_local, d_lcnt, d_lsum)) return rc;
    if (int rc = down_rows(h_lcnt.data(), d_lcnt, sizeof(int32_t), (size_t)L, a, b)) return rc;
    if (int rc = down_rows(h_lsum.data(), d_lsum, sizeof(double), (size_t)L, a, b)) return rc;
    if (int rc = X.end()) return rc;
    for (size_t i : cur) {
      BtProb& s = pr[i];
      for (int j = 0; j < s.nl; ++j) { s.lc[j] = h_lcnt[(size_t)L * i + j]; s.ls[j] = h_lsum[(size_t)L * i + j]; }
    }
    return 0;
  };

  for (size_t i = 0; i < np; ++i) replay(i);
  for (;;) {
    std::vector<size_t> batch, wait;
    for (size_t i = 0; i < np; ++i)
      if (pr[i].need == kBtNeedBatch) batch.push_back(i);
    if (!batch.empty()) {
      if (int rc = step(batch)) return rc;
      for (size_t i : batch) replay(i);
    }
    for (size_t i = 0; i < np; ++i)
      if (pr[i].need == kBtNeedLo) wait.push_back(i);
    if (batch.empty() && wait.empty()) break;
    while (!wait.empty()) {
      if (int rc = lo_round(wait)) return rc;
      std::vector<size_t> again;
      for (size_t i : wait)
        if (replay(i) == kBtNeedLo) again.push_back(i);
      wait.swap(again);
    }
  }
  return 0;
}

// The default group: consecutive pairs while the device tables of the three legs stay under
// kBtBudget, at most kBtMaxGroup pairs.  Both figures began as reasoned starting points (256 pairs x 8 workgroups of
// k_bt_five fill the device several times over; 256 MiB is a small share of the device's memory); section 4k's sweep over
// pairs_per_group 16 / 64 / 256 found the largest group the fastest in every cell and left them as they are.
constexpr int64_t kBtMaxGroup = 256;
constexpr size_t kBtBudget = (size_t)256 << 20;
constexpr int64_t kBtGroupLimit = 4096;  // of an explicit pairs_per_group: the problem is a grid dimension
}  // namespace

}  // namespace mpsfm

using namespace mpsfm;

namespace {
struct BtPair {  // a pair that takes part in its group's launches
  int64_t pair;
  int32_t n;
  int64_t off;  // first match among the group's active matches
  const double *intr1, *intr2;
  const int32_t *size1, *size2;
  double thrE;
  double E[9], F[9], H[9];
  int config, chosen;
  int64_t nsel;
};

// one group of consecutive pairs [g0, g1): legs in lockstep, masks, decision, watermark, pose
int bt_group(int64_t g0, int64_t g1, const int64_t* pair_start, const double* points1, const double* points2, const double* intr1,
             const double* intr2, const int32_t* size1, const int32_t* size2, const mpsfm_two_view_options* o, uint8_t* inlier_mask,
             mpsfm_two_view_result* results, mpsfm_two_view_batch_report* rep) {
  std::vector<BtPair> act;
  int64_t Ntot = 0;
  const double max_error = o->ransac.max_error;
  for (int64_t k = g0; k < g1; ++k) {
    const int32_t n = (int32_t)(pair_start[k + 1] - pair_start[k]);
    if (n < o->min_num_inliers || n < kTvHSample) continue;
    BtPair a{};
    a.pair = k;
    a.n = n;
    a.off = Ntot;
    a.intr1 = intr1 + 4 * k; a.intr2 = intr2 + 4 * k;
    a.size1 = size1 + 2 * k; a.size2 = size2 + 2 * k;
    a.thrE = 0.5 * (max_error / ((a.intr1[0] + a.intr1[1]) / 2.0) + max_error / ((a.intr2[0] + a.intr2[1]) / 2.0));
    a.config = MPSFM_TVG_DEGENERATE;
    a.chosen = -1;
    act.push_back(a);
    Ntot += n;
  }
  if (act.empty()) return 0;
  const size_t na = act.size();

  // every pair's SoA blocks u1 v1 u2 v2 one after the other: pixels, and CamFromImg of both PINHOLE cameras
  std::vector<double> hpx((size_t)4 * Ntot), hnm((size_t)4 * Ntot);
  for (const BtPair& a : act) {
    const double* p1 = points1 + 2 * (size_t)pair_start[a.pair];
    const double* p2 = points2 + 2 * (size_t)pair_start[a.pair];
    double* px = &hpx[(size_t)4 * a.off];
    double* nm = &hnm[(size_t)4 * a.off];
    const size_t n = (size_t)a.n;
    for (size_t i = 0; i < n; ++i) {
      const double u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
      px[i] = u1; px[n + i] = v1; px[2 * n + i] = u2; px[3 * n + i] = v2;
      nm[i] = (u1 - a.intr1[2]) / a.intr1[0];
      nm[n + i] = (v1 - a.intr1[3]) / a.intr1[1];
      nm[2 * n + i] = (u2 - a.intr2[2]) / a.intr2[0];
      nm[3 * n + i] = (v2 - a.intr2[3]) / a.intr2[1];
    }
  }

  CallScope A;
  if (int rc = A.open(true)) return rc;
  BtCtx X(A);
  if (int rc = X.reserve(3 * na)) return rc;
  double* d_px = A.alloc<double>(4 * (size_t)Ntot);
  double* d_nm = A.alloc<double>(4 * (size_t)Ntot);
  uint8_t* d_mask = A.alloc<uint8_t>(3 * (size_t)Ntot);  // E, F, H: [3][Ntot]
  if (!d_px || !d_nm || !d_mask) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  MPSFM_TRY(hipMemcpyAsync(d_px, hpx.data(), sizeof(double) * 4 * (size_t)Ntot, hipMemcpyHostToDevice, A.st));
  MPSFM_TRY(hipMemcpyAsync(d_nm, hnm.data(), sizeof(double) * 4 * (size_t)Ntot, hipMemcpyHostToDevice, A.st));
  MPSFM_TRY(hipMemsetAsync(d_mask, 0, 3 * (size_t)Ntot, A.st));

  // the three legs: the same options and the same seed
  mpsfm_ransac_options oe = o->ransac;
  if (oe.batch_trials == 0) oe.batch_trials = kTvEBatch;
  auto problems = [&](int min_n, bool normalised) {
    std::vector<BtProb> pr;
    for (size_t j = 0; j < na; ++j) {
      if (act[j].n < min_n) continue;
      BtProb s;
      s.pair = (int64_t)j;
      s.n = act[j].n;
      s.base = 4 * act[j].off;
      s.thr2 = normalised ? act[j].thrE * act[j].thrE : max_error * max_error;
      pr.push_back(s);
    }
    return pr;
  };
  std::vector<BtProb> pe = problems(kRpSample, true), pf = problems(kTvFSample, false), ph = problems(kTvHSample, false);
  if (int rc = bt_leg<RpProblem>(X, oe, d_nm, pe)) return rc;
  if (int rc = bt_leg<TvProblem<false>>(X, o->ransac, d_px, pf)) return rc;
  if (int rc = bt_leg<TvProblem<true>>(X, o->ransac, d_px, ph)) return rc;
  const int samples[3] = {kRpSample, kTvFSample, kTvHSample};
  std::vector<BtProb>* legs3[3] = {&pe, &pf, &ph};
  for (int l = 0; l < 3; ++l)
    for (const BtProb& s : *legs3[l]) {
      BtPair& a = act[(size_t)s.pair];
      mpsfm_two_view_result& r = results[a.pair];
      tv_fill_leg(r.leg[l], s.rep, samples[l]);
      double* keep = l == 0 ? a.E : l == 1 ? a.F : a.H;
      double* out = l == 0 ? r.E : l == 1 ? r.F : r.H;
      std::memcpy(keep, s.best_model, sizeof(double) * 9);
      if (r.leg[l].success) std::memcpy(out, s.best_model, sizeof(double) * 9);
    }

  // RANSAC's masks of the best models: one launch per leg type over the pairs whose leg has a model
  std::vector<uint8_t> hmask(3 * (size_t)Ntot);
  {
    const BtDesc* dd[3] = {nullptr, nullptr, nullptr};
    size_t cnt[3] = {0, 0, 0};
    int32_t max_n[3] = {0, 0, 0};
    for (int l = 0; l < 3; ++l) {
      BtDesc* hd = X.next(legs3[l]->size());
      if (!hd && !legs3[l]->empty()) return fail(MPSFM_ENOMEM, "descriptor ring too small");
      for (const BtProb& s : *legs3[l]) {
        const BtPair& a = act[(size_t)s.pair];
        if (!results[a.pair].leg[l].success) continue;
        BtDesc& d = hd[cnt[l]++];
        std::memcpy(d.model, s.best_model, sizeof(double) * 9);
        d.thr2 = s.thr2;
        d.base = s.base;
        d.n = s.n;
        d.out_off = (int64_t)l * Ntot + a.off;
        max_n[l] = std::max(max_n[l], s.n);
      }
      if (cnt[l])
        if (int rc = X.up(cnt[l], &dd[l])) return rc;
    }
    if (int rc = A.begin()) return rc;
    if (cnt[0])
      hipLaunchKernelGGL(k_bt_mask<RpProblem>, dim3((unsigned)((max_n[0] + kLoT - 1) / kLoT), (unsigned)cnt[0]), dim3(kLoT), 0, A.st, dd[0], d_nm, d_mask);
    if (cnt[1])
      hipLaunchKernelGGL(k_bt_mask<TvProblem<false>>, dim3((unsigned)((max_n[1] + kLoT - 1) / kLoT), (unsigned)cnt[1]), dim3(kLoT), 0, A.st, dd[1], d_px, d_mask);
    if (cnt[2])
      hipLaunchKernelGGL(k_bt_mask<TvProblem<true>>, dim3((unsigned)((max_n[2] + kLoT - 1) / kLoT), (unsigned)cnt[2]), dim3(kLoT), 0, A.st, dd[2], d_px, d_mask);
    MPSFM_TRY(hipGetLastError());
    X.launches += (cnt[0] != 0) + (cnt[1] != 0) + (cnt[2] != 0);
    MPSFM_TRY(hipMemcpyAsync(hmask.data(), d_mask, 3 * (size_t)Ntot, hipMemcpyDeviceToHost, A.st));
    if (int rc = X.end()) return rc;
  }

  // the decision and the watermark selection of every pair; the pairs that reach the translation leg
  std::vector<BtProb> pt;
  std::vector<double> hb;
  std::vector<size_t> pt_at;  // per translation problem: start of its block in hb
  for (size_t j = 0; j < na; ++j) {
    BtPair& a = act[j];
    mpsfm_two_view_result& r = results[a.pair];
    const mpsfm_two_view_leg* g = r.leg;
    tv_decide(*o, g[MPSFM_TVG_LEG_E].success, g[MPSFM_TVG_LEG_F].success, g[MPSFM_TVG_LEG_H].success, g[MPSFM_TVG_LEG_E].num_inliers,
              g[MPSFM_TVG_LEG_F].num_inliers, g[MPSFM_TVG_LEG_H].num_inliers, a.config, a.chosen);
    r.config = a.config;
    if (a.chosen < 0) continue;
    const uint8_t* sel = hmask.data() + (size_t)a.chosen * Ntot + a.off;
    std::memcpy(inlier_mask + pair_start[a.pair], sel, (size_t)a.n);
    a.nsel = 0;
    for (int32_t i = 0; i < a.n; ++i) a.nsel += sel[i];
    r.num_inliers = a.nsel;
    if (!o->detect_watermark) continue;
    std::vector<int32_t> border;
    const double* px = &hpx[(size_t)4 * a.off];
    tv_border(*o, px, a.n, sel, a.size1, a.size2, border);
    const int32_t m = (int32_t)border.size();
    r.num_border_inliers = m;
    if (m > 0 && (double)m / (double)a.nsel >= o->watermark_min_inlier_ratio) {
      BtProb s;
      s.pair = (int64_t)j;
      s.n = m;
      s.base = (int64_t)hb.size();
      s.thr2 = max_error * max_error;
      hb.resize(hb.size() + (size_t)4 * m);
      double* b = &hb[(size_t)s.base];
      for (int32_t q = 0; q < m; ++q)
        for (int k = 0; k < 4; ++k) b[(size_t)k * m + q] = px[(size_t)k * a.n + border[(size_t)q]];
      pt.push_back(s);
    }
  }
  if (!pt.empty()) {
    double* d_b = A.alloc<double>(hb.size());
    if (!d_b) return fail(MPSFM_ENOMEM, "hipMalloc failed");
    MPSFM_TRY(hipMemcpyAsync(d_b, hb.data(), sizeof(double) * hb.size(), hipMemcpyHostToDevice, A.st));
    mpsfm_ransac_options ow = o->ransac;
    ow.min_inlier_ratio = o->watermark_min_inlier_ratio;
    if (int rc = bt_leg<TvTranslation>(X, ow, d_b, pt)) return rc;
    for (const BtProb& s : pt) {
      BtPair& a = act[(size_t)s.pair];
      mpsfm_two_view_result& r = results[a.pair];
      tv_fill_leg(r.leg[MPSFM_TVG_LEG_T], s.rep, 1);
      if ((double)s.rep.best.num_inliers / (double)a.nsel >= o->watermark_min_inlier_ratio) {
        a.config = MPSFM_TVG_WATERMARK;
        r.watermark = 1;
      }
      r.config = a.config;
    }
  }

  // EstimateTwoViewGeometryPose of every pair that has one: one launch, the counts, then the angle rows in one download
  std::vector<size_t> poses;
  if (o->compute_relative_pose)
    for (size_t j = 0; j < na; ++j) {
      const int c = act[j].config;
      if (act[j].chosen >= 0 && (c == MPSFM_TVG_CALIBRATED || c == MPSFM_TVG_UNCALIBRATED || c == MPSFM_TVG_PLANAR_OR_PANORAMIC)) poses.push_back(j);
    }
  if (!poses.empty()) {
    std::vector<BtPoseDesc> hd(poses.size());
    int64_t rows = 0, angles = 0;
    int max_npx = 0;
    for (size_t q = 0; q < poses.size(); ++q) {
      const BtPair& a = act[poses[q]];
      BtPoseDesc& d = hd[q];
      d = BtPoseDesc{};
      tv_pose_cands(a.config, a.E, a.F, a.H, a.intr1, a.intr2, d.c);
      d.base = 4 * a.off;
      d.mask_off = (int64_t)a.chosen * Ntot + a.off;
      d.part_off = rows;
      d.angle_off = angles;
      d.n = a.n;
      d.nblk = lo_blocks(a.n, kLoT);
      rows += d.nblk;
      angles += 4 * (int64_t)a.n;
      max_npx = std::max(max_npx, (int)d.nblk);
    }
    BtPoseDesc* d_pd = A.alloc<BtPoseDesc>(hd.size());
    int32_t* d_ipart = A.alloc<int32_t>(4 * (size_t)rows);
    double* d_angle = A.alloc<double>((size_t)angles);
    if (!d_pd || !d_ipart || !d_angle) return fail(MPSFM_ENOMEM, "hipMalloc failed");
    std::vector<int32_t> h_ipart(4 * (size_t)rows);
    std::vector<double> h_angle((size_t)angles);
    MPSFM_TRY(hipMemcpyAsync(d_pd, hd.data(), sizeof(BtPoseDesc) * hd.size(), hipMemcpyHostToDevice, A.st));
    if (int rc = A.begin()) return rc;
    hipLaunchKernelGGL(k_bt_pose, dim3((unsigned)max_npx, (unsigned)hd.size()), dim3(kLoT), 0, A.st, d_pd, d_nm, d_mask, d_ipart, d_angle);
    MPSFM_TRY(hipGetLastError());
    X.launches += 1;
    MPSFM_TRY(hipMemcpyAsync(h_ipart.data(), d_ipart, sizeof(int32_t) * 4 * (size_t)rows, hipMemcpyDeviceToHost, A.st));
    MPSFM_TRY(hipMemcpyAsync(h_angle.data(), d_angle, sizeof(double) * (size_t)angles, hipMemcpyDeviceToHost, A.st));
    if (int rc = X.end()) return rc;
    for (size_t q = 0; q < poses.size(); ++q) {
      BtPair& a = act[poses[q]];
      const BtPoseDesc& d = hd[q];
      mpsfm_two_view_result& r = results[a.pair];
      int64_t count[4], bestc = -1;
      sum_rows(h_ipart.data() + 4 * (size_t)d.part_off, d.nblk, 4, count);
      const int bk = tv_pose_winner(d.c, count, bestc);
      const double* row = h_angle.data() + (size_t)d.angle_off + (size_t)bk * a.n;
      std::vector<double> ang(row, row + a.n);
      const bool from_E = a.config == MPSFM_TVG_CALIBRATED || a.config == MPSFM_TVG_UNCALIBRATED;
      tv_pose_finish(r, d.c, bk, bestc, ang, from_E, a.config);
      r.config = a.config;
    }
  }
  for (const BtPair& a : act) {
    mpsfm_two_view_result& r = results[a.pair];
    if (a.chosen >= 0) r.success = 1;
    r.ms = (float)A.ms;
  }
  rep->num_syncs += X.syncs;
  rep->num_launches += X.launches;
  rep->ms += (float)A.ms;
  return 0;
}
}  // namespace

extern "C" int mpsfm_two_view_geometry_batch(int64_t num_pairs, const int64_t* pair_start, const double* points1, const double* points2,
                                             const double* intr1, const double* intr2, const int32_t* size1, const int32_t* size2,
                                             const mpsfm_two_view_options* o, int32_t pairs_per_group, int32_t device, uint8_t* inlier_mask,
                                             mpsfm_two_view_result* results, mpsfm_two_view_batch_report* report) {
  if (num_pairs < 0) return fail(MPSFM_EINVAL, "negative number of pairs");
  if (num_pairs == 0) return 0;
  if (!pair_start || !points1 || !points2 || !intr1 || !intr2 || !size1 || !size2 || !o || !inlier_mask || !results)
    return fail(MPSFM_EINVAL, "NULL pointer");
  if (pairs_per_group < 0) return fail(MPSFM_EINVAL, "negative pairs_per_group");
  if (pair_start[0] != 0) return fail(MPSFM_EINVAL, "pair_start[0] must be 0");
  for (int64_t k = 0; k < num_pairs; ++k) {
    const int64_t n = pair_start[k + 1] - pair_start[k];
    if (n < 0) return fail(MPSFM_EINVAL, "pair " + std::to_string(k) + ": pair_start decreases");
    if (n > INT32_MAX) return fail(MPSFM_EINVAL, "pair " + std::to_string(k) + ": more than INT32_MAX correspondences (int32 indexing)");
  }
  for (int64_t k = 0; k < num_pairs; ++k) {
    const size_t at = 2 * (size_t)pair_start[k], len = 2 * (size_t)(pair_start[k + 1] - pair_start[k]);
    if (!finite_all(points1 + at, len) || !finite_all(points2 + at, len)) return fail(MPSFM_EINVAL, "pair " + std::to_string(k) + ": non-finite point");
    if (const char* why = tv_cameras_invalid(intr1 + 4 * k, intr2 + 4 * k, size1 + 2 * k, size2 + 2 * k))
      return fail(MPSFM_EINVAL, "pair " + std::to_string(k) + ": " + why);
  }
  if (!tv_options_valid(*o)) return fail(MPSFM_EINVAL, "invalid two-view geometry options");
  if (int rc = open_device(device)) return rc;

  const int64_t N = pair_start[num_pairs];
  std::memset(inlier_mask, 0, (size_t)N);
  for (int64_t k = 0; k < num_pairs; ++k) {
    results[k] = mpsfm_two_view_result{};
    for (int r = 0; r < 3; ++r) results[k].cam2_from_cam1[5 * r] = 1.0;
    results[k].config = MPSFM_TVG_DEGENERATE;
  }
  mpsfm_two_view_batch_report rep{};
  mpsfm_ransac_options oe = o->ransac;
  if (oe.batch_trials == 0) oe.batch_trials = kTvEBatch;
  const int64_t BE = lo_batch_cap<RpProblem>(oe), BF = lo_batch_cap<TvProblem<false>>(o->ransac), BH = lo_batch_cap<TvProblem<true>>(o->ransac);
  for (int64_t g0 = 0; g0 < num_pairs;) {
    int64_t g1 = g0;
    if (pairs_per_group > 0) {
      g1 = std::min<int64_t>(num_pairs, g0 + std::min<int64_t>(pairs_per_group, kBtGroupLimit));
    } else {
      size_t bytes = 0;
      while (g1 < num_pairs && g1 - g0 < kBtMaxGroup) {
        const int32_t n = (int32_t)(pair_start[g1 + 1] - pair_start[g1]);
        const size_t b = bt_leg_bytes<RpProblem>(n, BE) + bt_leg_bytes<TvProblem<false>>(n, BF) + bt_leg_bytes<TvProblem<true>>(n, BH);
        if (g1 > g0 && bytes + b > kBtBudget) break;
        bytes += b;
        ++g1;
      }
    }
    if (int rc = bt_group(g0, g1, pair_start, points1, points2, intr1, intr2, size1, size2, o, inlier_mask, results, &rep)) return rc;
    ++rep.num_groups;
    g0 = g1;
  }
  if (report) *report = rep;
  return 0;
}
