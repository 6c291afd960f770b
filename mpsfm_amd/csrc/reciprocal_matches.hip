// Dense reciprocal matches from descriptor maps (mpsfm_reciprocal_nns, mpsfm_dense_correspondences; semantics:
// include/mpsfm_hip.h, the descent rule, the arithmetic contract and the measurements: DESIGN.md section 4p).
//
//   k_recip_init    the seed grid of every search: xy (seed side) = the seed's pixel, xy (other side) = -1, all seeds active
//   k_nn_top1       similarity tiles on the matrix pipe (v_mfma_f64_16x16x4_f64) between the GATHERED rows map[xy[active[j]]] of
//                   a strip of 64 active seeds and all pixels of the other map, a running best per row in registers
//   k_recip_update  merges the column ranges of a row, compares the neighbour with the seed's previous one (equal: converged),
//                   stores it and appends the seeds that go on to the next half-step's active list
//   k_gather_conf   the confidences of the converged pairs
//
// A descent is 2 max_iter half-steps (k_nn_top1 + k_recip_update each), all enqueued at once: the active count of a half-step lives
// on the device (cnt[step], written by the update kernel of the step before), every kernel reads it and a workgroup whose rows lie
// beyond it returns at once.  Up to four searches run in the same launches (blockIdx.y).  The old1 / old2 arrays of the descent rule
// need no storage: a seed's xy is only written by the update that has just compared it, so at the comparison xy IS the value of
// the iteration before.
//
// k_nn_top1 is k_sim_top2 (descriptor_matches.hip) with gathered rows and a top-1: the same tiles, the same zero padding, the same
// instruction sequence for every element, candidates merged under (value descending, index ascending) in the lane, over the 16
// lanes of a row, and over the column ranges.  The order of the active list decides which workgroup and lane a seed's row lands
// in and nothing else: no output depends on it.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "call_scope.h"
#include "common.h"
#include "sim_tile.h"

namespace mpsfm {

namespace {
using namespace sim;

constexpr int kMaxSearch = 4;
constexpr int32_t kMaxIter = 1024;        // 4 launches per iteration are enqueued whether or not a seed is still active
constexpr int32_t kRangeTiles = 32;       // column tiles a workgroup streams at the most while the candidate buffer allows it
constexpr int64_t kCandBudget = 1 << 22;  // candidates (row x column range) per search

struct Search {
  const float* map[2];   // [0]: the map the seeds live in, [1]: the other one; [px][dim]
  const float* conf[2];  // their confidence maps [px], or NULL (mpsfm_reciprocal_nns)
  int32_t px[2];
  int32_t W0, nx;        // width of map[0], seeds per row of the seed grid
  int32_t n;             // seeds
  int32_t vec;           // both maps allow 4-wide loads
};

struct RecipArgs {
  Search s[kMaxSearch];
  int32_t dim, splits, nmax, steps, subsample, pad_;
  int32_t* xy;    // [search][side][nmax]: the seed's pixel on the seed side (0) and on the other side (1)
  int32_t* act;   // [search][step & 1][nmax]: the seeds active in a half-step
  int32_t* cnt;   // [search][steps + 1]: how many
  int32_t* conv;  // [search][nmax]: 1 once a seed has converged
  double* val;    // [search][nmax][splits]: best similarity of an active row within a column range
  int32_t* idx;   // [search][nmax][splits]: its column (kNoIndex: an empty range)
  float* q;       // [search][side][nmax]: confidences of the converged pairs
};

__global__ __launch_bounds__(kDT) void k_recip_init(RecipArgs a) {
  const int si = (int)blockIdx.y;
  const Search& S = a.s[si];
  const int32_t j = (int32_t)blockIdx.x * kDT + (int32_t)threadIdx.x;
  if (j == 0) a.cnt[si * (a.steps + 1)] = S.n;
  if (j >= S.n) return;
  const int32_t y = a.subsample / 2 + (j / S.nx) * a.subsample, x = a.subsample / 2 + (j % S.nx) * a.subsample;
  const size_t o = (size_t)si * 2 * a.nmax + j;
  a.xy[o] = y * S.W0 + x;
  a.xy[o + a.nmax] = -1;
  a.act[o] = j;
  a.conv[(size_t)si * a.nmax + j] = 0;
}

// half-step t: even steps look the seeds' pixels of map[0] up in map[1], odd steps the other way round
__global__ __launch_bounds__(kMT) void k_nn_top1(RecipArgs a, int t) {
  __shared__ double s_A[kKS * kLd];
  __shared__ double s_B[kKS * kLd];
  __shared__ int32_t s_row[kStrip];
  const int si = (int)blockIdx.y, h = t & 1;
  const Search& S = a.s[si];
  const int32_t count = a.cnt[si * (a.steps + 1) + t];
  const int32_t row0 = (int32_t)blockIdx.x * kStrip;
  if (row0 >= count) return;  // the grid is sized for all seeds of the largest search
  const float* R = S.map[h];
  const float* Cc = S.map[1 - h];
  const int32_t nq = S.px[h], ncols = S.px[1 - h];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const bool vec = S.vec != 0;

  // the strip's rows: pixels of the query map, -1 (a row of zeros that is never written) beyond the active list
  if (threadIdx.x < kStrip) {
    const int32_t p = row0 + (int32_t)threadIdx.x;
    int32_t q = -1;
    if (p < count) {
      const size_t o = ((size_t)si * 2 + h) * a.nmax;
      q = a.xy[o + a.act[o + p]];
      if (q < 0 || q >= nq) q = -1;  // cannot happen with finite inputs
    }
    s_row[threadIdx.x] = q;
  }
  __syncthreads();
  const auto row_of = [&](int r) { return s_row[r]; };
  const bool one_slice = a.dim <= kKS;  // the gathered rows are staged once, not once per column tile
  if (one_slice) load_slice_rows<float>(s_A, R, a.dim, 0, vec, row_of);

  double bv[4];
  int32_t bi[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { bv[r] = -INFINITY; bi[r] = kNoIndex; }

  // this workgroup's range of column tiles; an empty range leaves the sentinels, which every merge ignores
  const int32_t per = ((ncols + kStrip - 1) / kStrip + a.splits - 1) / a.splits * kStrip;
  const int64_t cb = (int64_t)blockIdx.z * per;
  const int32_t col_begin = (int32_t)min(cb, (int64_t)ncols), col_end = (int32_t)min(cb + per, (int64_t)ncols);
  for (int32_t col0 = col_begin; col0 < col_end; col0 += kStrip) {
    v4d acc[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[ni] = v4d{0.0, 0.0, 0.0, 0.0};
    for (int32_t k0 = 0; k0 < a.dim; k0 += kKS) {
      __syncthreads();  // the previous slice has been read
      if (!one_slice) load_slice_rows<float>(s_A, R, a.dim, k0, vec, row_of);
      load_slice<float>(s_B, Cc, ncols, col0, a.dim, k0, vec);
      __syncthreads();
      const int steps = (min(a.dim - k0, kKS) + 3) >> 2;
      for (int s = 0; s < steps; ++s) {
        const int x = 8 * (s & 7);
        const double* pa = s_A + (4 * s + lg) * kLd;
        const double* pb = s_B + (4 * s + lg) * kLd;
        const double av = pa[(16 * wave + lr) ^ x];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, pb[(16 * ni + lr) ^ x], acc[ni], 0, 0, 0);
      }
    }
    // this lane's candidates of the tile: columns col0 + 16 ni + lr, rows lg + 4 r of the band
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int32_t col = col0 + 16 * ni + lr;
      if (col < ncols) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (before(acc[ni][r], col, bv[r], bi[r])) { bv[r] = acc[ni][r]; bi[r] = col; }
      }
    }
  }
  // the 16 lanes that share a row
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
      const double ov = __shfl_xor(bv[r], m);
      const int32_t oi = __shfl_xor(bi[r], m);
      if (before(ov, oi, bv[r], bi[r])) { bv[r] = ov; bi[r] = oi; }
    }
    const int32_t p = row0 + 16 * wave + lg + 4 * r;
    if (lr == 0 && p < count) {
      const size_t o = ((size_t)si * a.nmax + p) * a.splits + blockIdx.z;
      a.val[o] = bv[r];
      a.idx[o] = bi[r];
    }
  }
}

__global__ __launch_bounds__(kDT) void k_recip_update(RecipArgs a, int t) {
  const int si = (int)blockIdx.y, h = t & 1;
  const Search& S = a.s[si];
  int32_t* cnt = a.cnt + si * (a.steps + 1);
  const int32_t count = cnt[t];
  const int32_t p = (int32_t)blockIdx.x * kDT + (int32_t)threadIdx.x;
  if (p >= count) return;
  // the ranges' candidates merge in the same total order: the result is the best over all columns, whatever the split
  double v = -INFINITY;
  int32_t i = kNoIndex;
  const size_t o = ((size_t)si * a.nmax + p) * a.splits;
  for (int z = 0; z < a.splits; ++z)
    if (before(a.val[o + z], a.idx[o + z], v, i)) { v = a.val[o + z]; i = a.idx[o + z]; }
  const int32_t j = a.act[((size_t)si * 2 + h) * a.nmax + p];
  if (i < 0 || i >= S.px[1 - h]) return;  // only with non-finite inputs, which the call refuses: the seed is dropped
  int32_t* slot = a.xy + ((size_t)si * 2 + (1 - h)) * a.nmax + j;
  const bool same = *slot == i;
  *slot = i;
  if (same) a.conv[(size_t)si * a.nmax + j] = 1;
  else a.act[((size_t)si * 2 + (1 - h)) * a.nmax + atomicAdd(&cnt[t + 1], 1)] = j;
}

__global__ __launch_bounds__(kDT) void k_gather_conf(RecipArgs a) {
  const int si = (int)blockIdx.y;
  const Search& S = a.s[si];
  const int32_t j = (int32_t)blockIdx.x * kDT + (int32_t)threadIdx.x;
  if (j >= S.n || !a.conv[(size_t)si * a.nmax + j]) return;
  for (int side = 0; side < 2; ++side) {
    const size_t o = ((size_t)si * 2 + side) * a.nmax + j;
    a.q[o] = S.conf[side][a.xy[o]];
  }
}

int32_t seeds_along(int32_t n, int32_t S) { return S / 2 < n ? (n - S / 2 + S - 1) / S : 0; }

struct MapIn { const float* feat; const float* conf; int32_t H, W; const char* name; };
// one search: seeds in maps[a], neighbours in maps[b]
struct SearchIn { int a, b; };

struct Descent {
  std::vector<int32_t> xy, conv, cnt;
  std::vector<float> q;
  int32_t nmax = 0;
};

int check_common(int32_t C, const mpsfm_recip_options& o) {
  if (C < 1 || C > kMaxDim) return fail(MPSFM_EINVAL, "C must be 1 .. 1024");
  if (o.subsample < 1) return fail(MPSFM_EINVAL, "subsample must be at least 1");
  if (o.max_iter < 1 || o.max_iter > kMaxIter) return fail(MPSFM_EINVAL, "max_iter must be 1 .. 1024");
  return 0;
}

int check_map(const MapIn& m, int32_t C, bool with_conf, bool on_device) {
  if (m.H < 1 || m.W < 1) return fail(MPSFM_EINVAL, "a map needs at least one row and one column");
  if ((int64_t)m.H * m.W > kMaxDesc) return fail(MPSFM_EINVAL, "more than 2^24 pixels in a map");
  if (!m.feat || (with_conf && !m.conf)) return fail(MPSFM_EINVAL, "NULL pointer");
  const size_t px = (size_t)m.H * (size_t)m.W;
  if (!on_device && (!all_finite(m.feat, px * C) || (with_conf && !all_finite(m.conf, px)))) return fail(MPSFM_EINVAL, "non-finite map value");
  return 0;
}

// The descents of `ns` searches over `nm` maps in lockstep; the maps are host or device memory as the options say.  Fills D with the
// seeds' pixels, the converged flags, the active counts of every half-step and (with_conf) the confidences, all on the host.
int descend(int nm, const MapIn* maps, int ns, const SearchIn* searches, int32_t C, bool with_conf, const mpsfm_recip_options& o, int32_t device,
            Descent& D, mpsfm_recip_info* info) {
  RecipArgs a{};
  a.dim = C;
  a.subsample = o.subsample;
  a.steps = 2 * o.max_iter;
  int64_t seeds = 0;
  int32_t cols_max = 0;
  for (int s = 0; s < ns; ++s) {
    const MapIn& m = maps[searches[s].a];
    a.s[s].nx = seeds_along(m.W, o.subsample);
    a.s[s].n = a.s[s].nx * seeds_along(m.H, o.subsample);
    a.s[s].W0 = m.W;
    a.s[s].px[0] = m.H * m.W;
    a.s[s].px[1] = maps[searches[s].b].H * maps[searches[s].b].W;
    a.nmax = std::max(a.nmax, a.s[s].n);
    cols_max = std::max(cols_max, std::max(a.s[s].px[0], a.s[s].px[1]));
    seeds += a.s[s].n;
  }
  D.nmax = a.nmax;
  if (info) info->n_seeds = seeds;
  if (a.nmax == 0) return 0;  // no seed anywhere: nothing to compute

  if (int rc = open_device(device)) return rc;
  CallScope A;
  if (int rc = A.open(true)) return rc;
  const float* feat[kMaxSearch];
  const float* conf[kMaxSearch];
  int32_t* d_bad = nullptr;
  if (o.inputs_on_device) {
    for (int m = 0; m < nm; ++m) {
      if (int rc = check_device_pointer(maps[m].feat, device, maps[m].name)) return rc;
      if (with_conf)
        if (int rc = check_device_pointer(maps[m].conf, device, maps[m].name)) return rc;
      feat[m] = maps[m].feat;
      conf[m] = maps[m].conf;
    }
    if (int rc = wait_for_caller(A, o.stream)) return rc;
    d_bad = A.alloc<int32_t>(1);
    if (!d_bad) return fail(MPSFM_ENOMEM, "hipMalloc failed");
    MPSFM_TRY(hipMemsetAsync(d_bad, 0, sizeof(int32_t), A.st));
  } else {
    for (int m = 0; m < nm; ++m) {
      const size_t px = (size_t)maps[m].H * (size_t)maps[m].W;
      feat[m] = A.put(maps[m].feat, px * C);
      conf[m] = with_conf ? A.put(maps[m].conf, px) : nullptr;
      if (!feat[m] || (with_conf && !conf[m])) return fail(MPSFM_ENOMEM, "hipMalloc failed");
    }
  }
  for (int s = 0; s < ns; ++s) {
    const int m[2] = {searches[s].a, searches[s].b};
    bool vec = C % 4 == 0;
    for (int side = 0; side < 2; ++side) {
      a.s[s].map[side] = feat[m[side]];
      a.s[s].conf[side] = with_conf ? conf[m[side]] : nullptr;
      vec = vec && ((uintptr_t)feat[m[side]] % (4 * sizeof(float))) == 0;
    }
    a.s[s].vec = vec ? 1 : 0;
  }

  // Column ranges: as many as fill the device in the first half-step, and at least so many that a workgroup streams no more
  // than kRangeTiles tiles (late half-steps have a strip or two of rows left and nothing else to spread over the device),
  // within the candidate buffer's budget.
  const int32_t strips = (a.nmax + kStrip - 1) / kStrip, col_tiles = (cols_max + kStrip - 1) / kStrip;
  int cus = 0;
  MPSFM_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  const int64_t fill = (int64_t)kFillPerCU * std::max(cus, 1), wgs = (int64_t)strips * ns;
  int64_t splits = std::max<int64_t>((fill + wgs - 1) / wgs, (col_tiles + kRangeTiles - 1) / kRangeTiles);
  splits = std::min<int64_t>(splits, std::max<int64_t>(1, kCandBudget / a.nmax));
  a.splits = (int32_t)std::max<int64_t>(1, std::min<int64_t>(splits, col_tiles));

  const size_t per_side = (size_t)ns * 2 * a.nmax, n_cnt = (size_t)ns * (a.steps + 1);
  a.xy = A.alloc<int32_t>(per_side);
  a.act = A.alloc<int32_t>(per_side);
  a.cnt = A.alloc<int32_t>(n_cnt);
  a.conv = A.alloc<int32_t>((size_t)ns * a.nmax);
  a.val = A.alloc<double>((size_t)ns * a.nmax * a.splits);
  a.idx = A.alloc<int32_t>((size_t)ns * a.nmax * a.splits);
  a.q = with_conf ? A.alloc<float>(per_side) : nullptr;
  if (!a.xy || !a.act || !a.cnt || !a.conv || !a.val || !a.idx || (with_conf && !a.q)) return fail(MPSFM_ENOMEM, "hipMalloc failed");

  if (int rc = A.begin()) return rc;
  if (d_bad)
    for (int m = 0; m < nm; ++m) {
      const int64_t px = (int64_t)maps[m].H * maps[m].W;
      if (int rc = scan_device(A, feat[m], px * C, d_bad)) return rc;
      if (with_conf)
        if (int rc = scan_device(A, conf[m], px, d_bad)) return rc;
    }
  MPSFM_TRY(hipMemsetAsync(a.cnt, 0, sizeof(int32_t) * n_cnt, A.st));
  const dim3 per_seed((unsigned)((a.nmax + kDT - 1) / kDT), (unsigned)ns);
  hipLaunchKernelGGL(k_recip_init, per_seed, dim3(kDT), 0, A.st, a);
  MPSFM_TRY(hipGetLastError());
  for (int t = 0; t < a.steps; ++t) {  // no host wait in here: the kernels size themselves from cnt[t]
    hipLaunchKernelGGL(k_nn_top1, dim3((unsigned)strips, (unsigned)ns, (unsigned)a.splits), dim3(kMT), 0, A.st, a, t);
    MPSFM_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_recip_update, per_seed, dim3(kDT), 0, A.st, a, t);
    MPSFM_TRY(hipGetLastError());
  }
  if (with_conf) {
    hipLaunchKernelGGL(k_gather_conf, per_seed, dim3(kDT), 0, A.st, a);
    MPSFM_TRY(hipGetLastError());
  }
  if (int rc = A.end()) return rc;
  if (d_bad) {
    int32_t bad = 0;
    MPSFM_TRY(A.down(&bad, d_bad, sizeof(bad)));
    if (bad) return fail(MPSFM_EINVAL, "non-finite value in a device input");
  }
  D.xy.resize(per_side);
  D.conv.resize((size_t)ns * a.nmax);
  D.cnt.resize(n_cnt);
  MPSFM_TRY(A.down(D.xy.data(), a.xy, sizeof(int32_t) * per_side));
  MPSFM_TRY(A.down(D.conv.data(), a.conv, sizeof(int32_t) * D.conv.size()));
  MPSFM_TRY(A.down(D.cnt.data(), a.cnt, sizeof(int32_t) * n_cnt));
  if (with_conf) {
    D.q.resize(per_side);
    MPSFM_TRY(A.down(D.q.data(), a.q, sizeof(float) * per_side));
  }
  if (info) {
    for (int s = 0; s < ns; ++s) {
      const int32_t* c = D.cnt.data() + (size_t)s * (a.steps + 1);
      int32_t its = 0;
      for (int t = 0; t < a.steps; ++t) {
        info->nn_queries += c[t];
        if (t % 2 == 0 && c[t] > 0) its = t / 2 + 1;
      }
      info->iterations = std::max(info->iterations, its);
      for (int32_t j = 0; j < a.s[s].n; ++j) info->n_converged += D.conv[(size_t)s * a.nmax + j] != 0;
    }
    info->column_ranges = a.splits;
    info->ms = (float)A.ms;
  }
  return 0;
}

mpsfm_recip_options options_of(const mpsfm_recip_options* opts) {
  mpsfm_recip_options o;
  mpsfm_recip_default_options(&o);
  if (opts) o = *opts;
  return o;
}
}  // namespace

}  // namespace mpsfm

using namespace mpsfm;

extern "C" void mpsfm_recip_default_options(mpsfm_recip_options* opts) {
  if (!opts) return;
  *opts = mpsfm_recip_options{};
  opts->subsample = 8;
  opts->max_iter = 10;
}

extern "C" int64_t mpsfm_recip_seed_count(int32_t H, int32_t W, int32_t subsample) {
  if (H < 1 || W < 1 || subsample < 1) return 0;
  return (int64_t)seeds_along(H, subsample) * seeds_along(W, subsample);
}

extern "C" int mpsfm_reciprocal_nns(const float* A, int32_t H1, int32_t W1, const float* B, int32_t H2, int32_t W2, int32_t C,
                                    const mpsfm_recip_options* opts, int32_t device, int64_t capacity, int32_t* idx1, int32_t* idx2,
                                    int64_t* n_out, mpsfm_recip_info* info) {
  if (info) *info = mpsfm_recip_info{};
  const mpsfm_recip_options o = options_of(opts);
  if (!n_out) return fail(MPSFM_EINVAL, "NULL pointer");
  *n_out = 0;
  if (int rc = check_common(C, o)) return rc;
  const MapIn maps[2] = {{A, nullptr, H1, W1, "A"}, {B, nullptr, H2, W2, "B"}};
  for (const MapIn& m : maps)
    if (int rc = check_map(m, C, false, o.inputs_on_device != 0)) return rc;
  const int64_t seeds = mpsfm_recip_seed_count(H1, W1, o.subsample);
  if (capacity < seeds) return fail(MPSFM_EINVAL, "capacity below mpsfm_recip_seed_count(H1, W1, subsample)");
  if (seeds > 0 && (!idx1 || !idx2)) return fail(MPSFM_EINVAL, "NULL pointer");
  const SearchIn search{0, 1};
  Descent D;
  if (int rc = descend(2, maps, 1, &search, C, false, o, device, D, info)) return rc;
  std::vector<uint64_t> pairs;
  for (int64_t j = 0; j < seeds; ++j)
    if (D.conv[j]) pairs.push_back((uint64_t)D.xy[j] << 32 | (uint32_t)D.xy[D.nmax + j]);
  std::sort(pairs.begin(), pairs.end());
  pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
  for (size_t k = 0; k < pairs.size(); ++k) { idx1[k] = (int32_t)(pairs[k] >> 32); idx2[k] = (int32_t)(pairs[k] & 0xffffffffu); }
  *n_out = (int64_t)pairs.size();
  return 0;
}

extern "C" int mpsfm_dense_correspondences(const float* feat11, const float* feat21, const float* feat22, const float* feat12,
                                           const float* qonf11, const float* qonf21, const float* qonf22, const float* qonf12, int32_t H1,
                                           int32_t W1, int32_t H2, int32_t W2, int32_t C, const mpsfm_recip_options* opts, int32_t device,
                                           int64_t capacity, int32_t* xy1, int32_t* xy2, float* scores, int64_t* n_out, mpsfm_recip_info* info) {
  if (info) *info = mpsfm_recip_info{};
  const mpsfm_recip_options o = options_of(opts);
  if (!n_out) return fail(MPSFM_EINVAL, "NULL pointer");
  *n_out = 0;
  if (int rc = check_common(C, o)) return rc;
  const MapIn maps[4] = {{feat11, qonf11, H1, W1, "feat11 / qonf11"}, {feat21, qonf21, H2, W2, "feat21 / qonf21"},
                         {feat22, qonf22, H2, W2, "feat22 / qonf22"}, {feat12, qonf12, H1, W1, "feat12 / qonf12"}};
  for (const MapIn& m : maps)
    if (int rc = check_map(m, C, true, o.inputs_on_device != 0)) return rc;
  const int64_t seeds = 2 * (mpsfm_recip_seed_count(H1, W1, o.subsample) + mpsfm_recip_seed_count(H2, W2, o.subsample));
  if (capacity < seeds) return fail(MPSFM_EINVAL, "capacity below 2 (seeds of image 1 + seeds of image 2)");
  if (seeds > 0 && (!xy1 || !xy2 || !scores)) return fail(MPSFM_EINVAL, "NULL pointer");
  // the reference's order: (feat11 -> feat21), (feat21 -> feat11), (feat12 -> feat22), (feat22 -> feat12)
  const SearchIn searches[4] = {{0, 1}, {1, 0}, {3, 2}, {2, 3}};
  Descent D;
  if (int rc = descend(4, maps, 4, searches, C, true, o, device, D, info)) return rc;
  if (D.nmax == 0) return 0;
  // the concatenation: odd searches are seeded in image 2, their side 1 is image 1.  A stable sort by (idx1, idx2) leaves the
  // first occurrence of a pair in front: its confidences are the ones merge_corres keeps
  struct Row { uint64_t key; float q1, q2; };
  std::vector<Row> rows;
  for (int s = 0; s < 4; ++s) {
    const int side1 = s & 1, side2 = 1 - side1;
    const int32_t n = (int32_t)mpsfm_recip_seed_count(maps[searches[s].a].H, maps[searches[s].a].W, o.subsample);
    const size_t base = (size_t)s * 2 * D.nmax;
    for (int32_t j = 0; j < n; ++j)
      if (D.conv[(size_t)s * D.nmax + j]) {
        const size_t o1 = base + (size_t)side1 * D.nmax + j, o2 = base + (size_t)side2 * D.nmax + j;
        rows.push_back(Row{(uint64_t)D.xy[o1] << 32 | (uint32_t)D.xy[o2], D.q[o1], D.q[o2]});
      }
  }
  std::stable_sort(rows.begin(), rows.end(), [](const Row& x, const Row& y) { return x.key < y.key; });
  int64_t k = 0;
  for (size_t r = 0; r < rows.size(); ++r) {
    if (r > 0 && rows[r].key == rows[r - 1].key) continue;
    const int32_t i1 = (int32_t)(rows[r].key >> 32), i2 = (int32_t)(rows[r].key & 0xffffffffu);
    xy1[2 * k] = i1 % W1; xy1[2 * k + 1] = i1 / W1;
    xy2[2 * k] = i2 % W2; xy2[2 * k + 1] = i2 / W2;
    const float prod = rows[r].q1 * rows[r].q2;  // float32, each operation rounded on its own, as NumPy does it
    scores[k] = sqrtf(prod);
    ++k;
  }
  *n_out = k;
  return 0;
}
