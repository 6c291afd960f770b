// Descriptors to match lists for many image pairs in one call (mpsfm_match_descriptors_batch; semantics: include/mpsfm_hip.h, the
// contract, the item table, the range rule and the groups: DESIGN.md section 4q).
//
//   k_sim_top2_batch      one workgroup per WORK ITEM of a host-built table: one strip of 64 rows of one pair and direction against
//                         one range of that pair's column tiles, through sim_top2_strip() of sim_top2.h, the body of k_sim_top2
//   k_match_decide_batch  one thread per output row, one workgroup per 256 rows of one pair, through match_of() of sim_top2.h, the
//                         body of k_match_decide
//
// Identity with the single call: both run the same bodies on the same values, and a row's top-2 is a function of the SET of its
// candidates under one total order, so neither the ranges a pair's columns are cut into nor what else the launch holds can show in
// its results.  Items are built only for strips and ranges that exist: no workgroup returns at once, every record is written.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "call_scope.h"
#include "common.h"
#include "sim_tile.h"
#include "sim_top2.h"  // contraction off from here on: the decisions round every operation on its own

namespace mpsfm {

namespace {
using namespace sim;

constexpr int64_t kGroupTableBytes = (int64_t)256 << 20;  // default rule: top-2 tables of a group
constexpr int64_t kRecordBytes = 24;                       // two doubles and two indices per row and range
constexpr int32_t kMaxPairsPerGroup = 4096;                // cap of an explicit pairs_per_group

// One launched pair.  Record offsets count [row][range] records: values at val + 2 t, columns at idx + 2 t.
struct BatchPair {
  int64_t x0, x1;      // first row of image 0 / image 1 in desc
  int64_t t0, t1;      // first record of direction 0 (rows = image 0) / direction 1 in the group's tables
  int64_t out0;        // first row of the pair's slice of the outputs
  int32_t n0, n1;
  int32_t s0, s1;      // ranges the columns of a strip are cut into, direction 0 / 1
  int32_t use_ratio;   // the ratio test is on and both sides hold more than one descriptor
  int32_t pad_;
};
static_assert(sizeof(BatchPair) == 64, "one 64-byte record per pair");

struct BatchItem {
  int32_t pair;        // index into the group's pair records
  int32_t dir;         // 0: rows = image 0, 1: rows = image 1
  int32_t row0;        // first row of the strip
  int32_t col_begin, col_end;  // the range's columns: col_begin a multiple of kStrip, col_end <= ncols
  int32_t z;           // which of the pair's ranges this is: records [row][z]
  int32_t pad_[2];
};
static_assert(sizeof(BatchItem) == 32, "one 32-byte record per work item");

struct DecideItem { int32_t pair, row0; };  // 256 output rows of one pair

struct BatchSimArgs {
  const BatchItem* __restrict__ items;
  const BatchPair* __restrict__ pairs;
  const float* __restrict__ desc;
  int32_t dim, vec;
  double* __restrict__ val;
  int32_t* __restrict__ idx;
};

// Four waves per SIMD: with 40 KB of LDS four workgroups fit a compute unit, and the register budget of 128 lets all four run.  The
// compiler then keeps the accumulators in VGPRs (98 VGPRs, no AGPRs, no scratch) instead of 98 + 32, which admits three.
__global__ __launch_bounds__(kMT) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_sim_top2_batch(BatchSimArgs a) {
  __shared__ double s_A[kKS * kLd];
  __shared__ double s_B[kKS * kLd];
  // wave-uniform records, read once: scalar loads
  const BatchItem it = a.items[blockIdx.x];
  const BatchPair p = a.pairs[it.pair];
  const bool fwd = it.dir == 0;
  const int32_t nrows = fwd ? p.n0 : p.n1, ncols = fwd ? p.n1 : p.n0;
  const int64_t xr = fwd ? p.x0 : p.x1, xc = fwd ? p.x1 : p.x0;
  const int64_t t = fwd ? p.t0 : p.t1;
  const int32_t splits = fwd ? p.s0 : p.s1;
  sim_top2_strip<float>(s_A, s_B, a.desc + (size_t)xr * (size_t)a.dim, nrows, it.row0, a.desc + (size_t)xc * (size_t)a.dim, ncols, it.col_begin,
                        it.col_end, a.dim, a.vec != 0, splits, it.z, a.val + 2 * t, a.idx + 2 * t);
}

struct BatchDecideArgs {
  const DecideItem* __restrict__ items;
  const BatchPair* __restrict__ pairs;
  const double* __restrict__ val;
  const int32_t* __restrict__ idx;
  double ratio2, dist2, score_thr;
  int32_t use_dist, use_score, mutual, pad_;
  int32_t* __restrict__ matches;
  double* __restrict__ scores;
};

__global__ __launch_bounds__(kDT) void k_match_decide_batch(BatchDecideArgs a) {
  const DecideItem it = a.items[blockIdx.x];
  const BatchPair p = a.pairs[it.pair];
  const int32_t i = it.row0 + (int32_t)threadIdx.x;
  if (i >= p.n0) return;
  const Top2Table dir0{a.val + 2 * p.t0, a.idx + 2 * p.t0, p.s0, p.n1}, dir1{a.val + 2 * p.t1, a.idx + 2 * p.t1, p.s1, p.n0};
  const MatchRule rule{a.ratio2, a.dist2, a.score_thr, p.use_ratio, a.use_dist, a.use_score, a.mutual};
  double score;
  const int32_t m = match_of(dir0, dir1, rule, i, score);
  a.matches[p.out0 + i] = m;
  a.scores[p.out0 + i] = score;
}

inline int32_t tiles_of(int64_t n) { return (int32_t)((n + kStrip - 1) / kStrip); }

// `want` workgroups per strip over `tiles` column tiles: the tiles per range, and the ranges that are not empty
inline void cut(int32_t tiles, int64_t want, int32_t* per, int32_t* ranges) {
  const int32_t w = (int32_t)std::max<int64_t>(1, std::min<int64_t>(want, tiles));
  *per = (tiles + w - 1) / w;
  *ranges = (tiles + *per - 1) / *per;
}

struct Group {
  int64_t pair0, pair1;      // its pair records [pair0, pair1) of Plan::pairs
  int64_t item0, nitems;     // its work items
  int64_t ditem0, nditems;   // its decide items
  int64_t records;           // records of its top-2 tables
};

struct Plan {
  std::vector<int64_t> live;  // the pairs that are launched, in order
  std::vector<BatchPair> pairs;
  std::vector<BatchItem> items;
  std::vector<DecideItem> ditems;
  std::vector<Group> groups;
  int64_t max_records = 0;
};

}  // namespace

}  // namespace mpsfm

using namespace mpsfm;

extern "C" int mpsfm_match_descriptors_batch(int32_t num_images, const int64_t* image_start, int32_t dim, const float* desc, int64_t num_pairs,
                                             const int32_t* pair_image0, const int32_t* pair_image1, const int64_t* match_start,
                                             const mpsfm_match_options* opts, int32_t column_ranges, int32_t pairs_per_group, int32_t device,
                                             int32_t* matches0, double* scores0, int64_t* pair_num_matches, mpsfm_match_batch_report* report) {
  if (report) *report = mpsfm_match_batch_report{};
  mpsfm_match_options o;
  mpsfm_match_default_options(&o);
  if (opts) o = *opts;
  // ---- checks, before any HIP call
  if (num_images < 0 || num_pairs < 0) return fail(MPSFM_EINVAL, "negative count");
  if (dim < 1 || dim > kMaxDim) return fail(MPSFM_EINVAL, "dim must be 1 .. 1024");
  if (column_ranges < 0 || pairs_per_group < 0) return fail(MPSFM_EINVAL, "negative column_ranges or pairs_per_group");
  if (int rc = check_match_options(o)) return rc;
  if (!image_start) return fail(MPSFM_EINVAL, "NULL pointer: image_start");
  if (image_start[0] != 0) return fail(MPSFM_EINVAL, "image_start[0] must be 0");
  for (int32_t i = 0; i < num_images; ++i) {
    const int64_t n = image_start[i + 1] - image_start[i];
    if (n < 0) return fail(MPSFM_EINVAL, "image " + std::to_string(i) + ": image_start decreases");
    if (n > kMaxDesc) return fail(MPSFM_EINVAL, "image " + std::to_string(i) + ": more than 2^24 descriptors");
  }
  const int64_t total = image_start[num_images];
  if (total > 0 && !desc) return fail(MPSFM_EINVAL, "NULL pointer: desc");
  if (num_pairs > 0 && (!pair_image0 || !pair_image1)) return fail(MPSFM_EINVAL, "NULL pointer: pair_image0 / pair_image1");
  if (!match_start) return fail(MPSFM_EINVAL, "NULL pointer: match_start");
  if (match_start[0] != 0) return fail(MPSFM_EINVAL, "match_start[0] must be 0");
  for (int64_t k = 0; k < num_pairs; ++k) {
    const int32_t a = pair_image0[k], b = pair_image1[k];
    if (a < 0 || a >= num_images || b < 0 || b >= num_images)
      return fail(MPSFM_EINVAL, "pair " + std::to_string(k) + ": image index outside [0, num_images)");
    if (match_start[k + 1] - match_start[k] != image_start[a + 1] - image_start[a])
      return fail(MPSFM_EINVAL, "pair " + std::to_string(k) + ": its slice of the outputs is not as long as its first image");
  }
  const int64_t rows = match_start[num_pairs];
  if (rows > 0 && (!matches0 || !scores0)) return fail(MPSFM_EINVAL, "NULL pointer: matches0 / scores0");
  if (!o.inputs_on_device)
    for (int32_t i = 0; i < num_images; ++i)
      if (!all_finite(desc + (size_t)image_start[i] * dim, (size_t)(image_start[i + 1] - image_start[i]) * dim))
        return fail(MPSFM_EINVAL, "image " + std::to_string(i) + ": non-finite descriptor value");
  if (num_pairs == 0) return 0;

  // ---- the pairs that need a device
  auto size_of = [&](int32_t img) { return image_start[img + 1] - image_start[img]; };
  Plan P;
  for (int64_t k = 0; k < num_pairs; ++k) {
    const int64_t n0 = size_of(pair_image0[k]), n1 = size_of(pair_image1[k]);
    if (n0 > 0 && n1 > 0) P.live.push_back(k);
    else if (n0 > 0) fill_empty(n0, matches0 + match_start[k], scores0 + match_start[k]);
    if (pair_num_matches) pair_num_matches[k] = 0;
  }
  if (P.live.empty()) return 0;
  if (int rc = open_device(device)) return rc;
  int cus = 0;
  MPSFM_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  const int64_t fill = (int64_t)kFillPerCU * std::max(cus, 1);
  const int dirs = o.mutual_check ? 2 : 1;
  const bool ratio_on = o.ratio_threshold > 0.0;

  // ---- groups: runs of consecutive launched pairs.  A group's ranges follow from its own strips (default rule) or from column_ranges.
  const int64_t L = (int64_t)P.live.size();
  auto strips_of = [&](int64_t li) {  // workgroups of launched pair li with one range per strip
    const int64_t k = P.live[li];
    return (int64_t)tiles_of(size_of(pair_image0[k])) + (dirs == 2 ? (int64_t)tiles_of(size_of(pair_image1[k])) : 0);
  };
  auto records_of = [&](int64_t li, int64_t want) {  // records of launched pair li when a strip asks for `want` ranges
    const int64_t k = P.live[li];
    const int64_t n0 = size_of(pair_image0[k]), n1 = size_of(pair_image1[k]);
    int32_t per, r0, r1;
    cut(tiles_of(n1), want, &per, &r0);
    cut(tiles_of(n0), want, &per, &r1);
    return n0 * r0 + (dirs == 2 ? n1 * r1 : 0);
  };
  auto want_of = [&](int64_t base) { return column_ranges > 0 ? (int64_t)column_ranges : (fill + base - 1) / base; };
  std::vector<std::pair<int64_t, int64_t>> runs;  // [first, last) of every group
  if (pairs_per_group > 0) {
    const int64_t g = std::min(pairs_per_group, kMaxPairsPerGroup);
    for (int64_t a = 0; a < L; a += g) runs.emplace_back(a, std::min(L, a + g));
  } else {
    const int64_t budget = kGroupTableBytes / kRecordBytes;
    int64_t a = 0;
    while (a < L) {
      // grow [a, b) while its tables fit.  While the ranges wanted per strip fall with each pair added (fewer than `fill` strips, so
      // few pairs) the records of all its pairs are recounted; once they stay the count only grows by the new pair's
      int64_t b = a + 1, base = strips_of(a), rec = 0, counted_want = 0;  // counted_want: the `want` rec was counted with, 0: not yet
      while (b < L) {
        const int64_t nbase = base + strips_of(b), want = want_of(nbase);
        int64_t nrec = 0;
        if (want == counted_want) nrec = rec + records_of(b, want);
        else
          for (int64_t li = a; li <= b; ++li) nrec += records_of(li, want);
        if (nrec > budget) break;
        rec = nrec; counted_want = want; base = nbase; ++b;
      }
      runs.emplace_back(a, b);
      a = b;
    }
  }
  int64_t workgroups = 0;
  for (const auto& run : runs) {
    Group G{};
    G.pair0 = (int64_t)P.pairs.size(); G.item0 = (int64_t)P.items.size(); G.ditem0 = (int64_t)P.ditems.size();
    int64_t base = 0;
    for (int64_t li = run.first; li < run.second; ++li) base += strips_of(li);
    const int64_t want = want_of(base);
    int64_t rec = 0;
    for (int64_t li = run.first; li < run.second; ++li) {
      const int64_t k = P.live[li];
      const int32_t i0 = pair_image0[k], i1 = pair_image1[k];
      BatchPair bp{};
      bp.x0 = image_start[i0]; bp.x1 = image_start[i1];
      bp.n0 = (int32_t)size_of(i0); bp.n1 = (int32_t)size_of(i1);
      bp.out0 = match_start[k];
      bp.use_ratio = (ratio_on && bp.n0 > 1 && bp.n1 > 1) ? 1 : 0;
      int32_t per[2];
      cut(tiles_of(bp.n1), want, &per[0], &bp.s0);
      cut(tiles_of(bp.n0), want, &per[1], &bp.s1);
      bp.t0 = rec; rec += (int64_t)bp.n0 * bp.s0;
      if (dirs == 2) { bp.t1 = rec; rec += (int64_t)bp.n1 * bp.s1; }
      else { bp.t1 = bp.t0; bp.s1 = 0; }  // never read without the mutual check
      const int32_t local = (int32_t)(li - run.first);
      for (int d = 0; d < dirs; ++d) {
        const int32_t nr = d ? bp.n1 : bp.n0, nc = d ? bp.n0 : bp.n1, s = d ? bp.s1 : bp.s0;
        for (int32_t row0 = 0; row0 < nr; row0 += kStrip)
          for (int32_t z = 0; z < s; ++z) {
            BatchItem it{};
            it.pair = local; it.dir = d; it.row0 = row0; it.z = z;
            it.col_begin = (int32_t)std::min<int64_t>((int64_t)z * per[d] * kStrip, nc);
            it.col_end = (int32_t)std::min<int64_t>((int64_t)(z + 1) * per[d] * kStrip, nc);
            P.items.push_back(it);
          }
      }
      for (int32_t row0 = 0; row0 < bp.n0; row0 += kDT) P.ditems.push_back(DecideItem{local, row0});
      P.pairs.push_back(bp);
    }
    G.pair1 = (int64_t)P.pairs.size();
    G.nitems = (int64_t)P.items.size() - G.item0;
    G.nditems = (int64_t)P.ditems.size() - G.ditem0;
    G.records = rec;
    if (G.nitems > INT32_MAX || G.nditems > INT32_MAX) return fail(MPSFM_EUNSUPPORTED, "a group of more than 2^31 - 1 workgroups: lower pairs_per_group");
    P.max_records = std::max(P.max_records, rec);
    workgroups += G.nitems;
    P.groups.push_back(G);
  }

  // ---- device: descriptors, tables, outputs
  CallScope A;
  if (int rc = A.open(true)) return rc;
  const float* d_desc = desc;
  int32_t* d_bad = nullptr;
  if (o.inputs_on_device) {
    if (int rc = check_device_pointer(desc, device, "desc")) return rc;
    if (int rc = wait_for_caller(A, o.stream)) return rc;
    d_bad = A.alloc<int32_t>(1);
    if (!d_bad) return fail(MPSFM_ENOMEM, "hipMalloc failed");
    MPSFM_TRY(hipMemsetAsync(d_bad, 0, sizeof(int32_t), A.st));
  } else {
    d_desc = A.put(desc, (size_t)total * dim);
    if (!d_desc) return fail(MPSFM_ENOMEM, "hipMalloc failed: the descriptors of all images must fit the device");
  }
  const BatchPair* d_pairs = A.put(P.pairs.data(), P.pairs.size());
  const BatchItem* d_items = A.put(P.items.data(), P.items.size());
  const DecideItem* d_ditems = A.put(P.ditems.data(), P.ditems.size());
  double* d_val = A.alloc<double>(2 * (size_t)P.max_records);
  int32_t* d_idx = A.alloc<int32_t>(2 * (size_t)P.max_records);
  int32_t* d_m = A.alloc<int32_t>((size_t)rows);
  double* d_s = A.alloc<double>((size_t)rows);
  if (!d_pairs || !d_items || !d_ditems || !d_val || !d_idx || !d_m || !d_s) return fail(MPSFM_ENOMEM, "hipMalloc failed");

  int64_t launches = 0;
  if (int rc = A.begin()) return rc;
  if (d_bad) {
    if (int rc = scan_device(A, d_desc, total * dim, d_bad)) return rc;
    ++launches;
  }
  BatchSimArgs s{};
  s.desc = d_desc; s.dim = dim;
  s.vec = (dim % 4 == 0 && ((uintptr_t)d_desc % (4 * sizeof(float))) == 0) ? 1 : 0;  // then every image starts on 16 bytes
  s.val = d_val; s.idx = d_idx;
  BatchDecideArgs a{};
  a.val = d_val; a.idx = d_idx;
  a.use_dist = o.distance_threshold > 0.0 ? 1 : 0;
  a.use_score = o.score_threshold > 0.0 ? 1 : 0;
  a.ratio2 = o.ratio_threshold * o.ratio_threshold;
  a.dist2 = o.distance_threshold * o.distance_threshold;
  a.score_thr = o.score_threshold;
  a.mutual = o.mutual_check ? 1 : 0;
  a.matches = d_m; a.scores = d_s;
  for (const Group& G : P.groups) {  // back to back: the next group's similarity launch overwrites the tables behind this group's decisions
    s.items = d_items + G.item0; s.pairs = d_pairs + G.pair0;
    hipLaunchKernelGGL(k_sim_top2_batch, dim3((unsigned)G.nitems), dim3(kMT), 0, A.st, s);
    MPSFM_TRY(hipGetLastError());
    a.items = d_ditems + G.ditem0; a.pairs = d_pairs + G.pair0;
    hipLaunchKernelGGL(k_match_decide_batch, dim3((unsigned)G.nditems), dim3(kDT), 0, A.st, a);
    MPSFM_TRY(hipGetLastError());
    launches += 2;
  }
  if (int rc = A.stop()) return rc;
  // ---- everything comes down behind the last launch: one wait
  int32_t bad = 0;
  if (d_bad) MPSFM_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipMemcpyAsync(matches0, d_m, sizeof(int32_t) * (size_t)rows, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipMemcpyAsync(scores0, d_s, sizeof(double) * (size_t)rows, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipStreamSynchronize(A.st));
  float ms = 0.f;
  if (int rc = A.elapsed(&ms)) return rc;
  if (bad) return fail(MPSFM_EINVAL, "non-finite value in a device input");
  for (int64_t k = 0; k < num_pairs; ++k)  // no kernel wrote the rows of a pair without columns
    if (size_of(pair_image1[k]) == 0) fill_empty(match_start[k + 1] - match_start[k], matches0 + match_start[k], scores0 + match_start[k]);
  int64_t all = 0;
  for (int64_t k : P.live) {
    int64_t cnt = 0;
    for (int64_t i = match_start[k]; i < match_start[k + 1]; ++i) cnt += matches0[i] >= 0;
    if (pair_num_matches) pair_num_matches[k] = cnt;
    all += cnt;
  }
  if (report) {
    report->num_matches = all;
    report->num_groups = (int64_t)P.groups.size();
    report->num_launches = launches;
    report->num_syncs = 1;
    report->num_workgroups = workgroups;
    report->ms = ms;
  }
  return 0;
}
