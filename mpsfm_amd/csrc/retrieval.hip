// Global descriptors to image pairs (mpsfm_retrieve_topk; semantics: include/mpsfm_hip.h, the contract, the tie rule, the
// kernels and the margins: DESIGN.md section 4r; reference: mpsfm/extraction/pairs/hloc/pairs_from_retrieval.py).
//
//   k_sim_topk    similarity tiles on the matrix pipe (v_mfma_f64_16x16x4_f64), a running top-k per row in LDS; one of
//                 gridDim.y ranges of column tiles per workgroup; nothing of size nq x nd is ever written
//   k_topk_merge  the ranges of a row under the same order: final lists, scores and counts
//
// The strip, the list and the merge are the bodies of sim_topk.h.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "call_scope.h"
#include "common.h"
#include "sim_tile.h"
#include "sim_topk.h"  // contraction off from here on

namespace mpsfm {

namespace {
using namespace sim;

struct TopkArgs {
  const float* Q;   // [nq][dim]
  const float* D;   // [nd][dim]
  int32_t nq, nd, dim;
  int32_t vec;      // both sets allow 4-wide loads
  int32_t K;
  int32_t splits;   // workgroups that share a strip, each streaming its own range of column tiles (gridDim.y)
  TopkRule rule;
  double* val;      // [nq][splits][K]: the sorted list of every row within a range, tail -inf
  int32_t* idx;     // [nq][splits][K]: their columns, tail kNoIndex
  int32_t* indices; // [nq][K]
  double* scores;   // [nq][K]
  int32_t* counts;  // [nq]
};

__global__ __launch_bounds__(kMT) void k_sim_topk(TopkArgs a) {
  extern __shared__ __attribute__((aligned(16))) double s_topk[];
  const int32_t row0 = (int32_t)blockIdx.x * kStrip;
  // this workgroup's range of column tiles; an empty range writes sentinels, which no merge prefers
  const int32_t per = ((a.nd + kStrip - 1) / kStrip + a.splits - 1) / a.splits * kStrip;
  const int64_t cb = (int64_t)blockIdx.y * per;
  const int32_t col_begin = (int32_t)min(cb, (int64_t)a.nd), col_end = (int32_t)min(cb + per, (int64_t)a.nd);
  sim_topk_strip(s_topk, a.Q, a.nq, row0, a.D, a.nd, col_begin, col_end, a.dim, a.vec != 0, a.rule, a.K, a.splits, (int32_t)blockIdx.y,
                 a.val, a.idx);
}

__global__ __launch_bounds__(64) void k_topk_merge(TopkArgs a) {
  __shared__ uint8_t s_heads[kMaxRanges];
  topk_merge_row(s_heads, a.val, a.idx, (int32_t)blockIdx.x, a.splits, a.K, a.indices, a.scores, a.counts);
}

void fill_empty_lists(int64_t nq, int32_t K, int32_t* indices, double* scores, int32_t* counts) {
  for (int64_t i = 0; i < nq * K; ++i) { indices[i] = -1; scores[i] = 0.0; }
  for (int64_t i = 0; i < nq; ++i) counts[i] = 0;
}
}  // namespace

}  // namespace mpsfm

using namespace mpsfm;

extern "C" void mpsfm_retrieval_default_options(mpsfm_retrieval_options* opts) {
  if (!opts) return;
  *opts = mpsfm_retrieval_options{};
  opts->num_select = 20;
  opts->use_min_score = 1;
  opts->min_score = 0.0;
}

extern "C" int mpsfm_retrieve_topk(int64_t nq, int64_t nd, int32_t dim, const float* query, const float* db, const int32_t* query_id,
                                   const int32_t* db_id, const mpsfm_retrieval_options* opts, int32_t device, int32_t* indices, double* scores,
                                   int32_t* counts, mpsfm_retrieval_info* info) {
  if (info) *info = mpsfm_retrieval_info{};
  mpsfm_retrieval_options o;
  mpsfm_retrieval_default_options(&o);
  if (opts) o = *opts;
  if (nq < 0 || nd < 0) return fail(MPSFM_EINVAL, "negative size");
  if (nq > kMaxDesc || nd > kMaxDesc) return fail(MPSFM_EINVAL, "more than 2^24 descriptors");
  if (dim < 1 || dim > kMaxDimTopk) return fail(MPSFM_EINVAL, "dim must be 1 .. 65536");
  if (o.num_select < 1 || o.num_select > kMaxSelect) return fail(MPSFM_EINVAL, "num_select must be 1 .. 128");
  if (nd > 0 && o.num_select > nd) return fail(MPSFM_EINVAL, "num_select exceeds the number of db descriptors");
  if (o.column_ranges < 0) return fail(MPSFM_EINVAL, "negative column_ranges");
  if ((query_id == nullptr) != (db_id == nullptr)) return fail(MPSFM_EINVAL, "query_id and db_id: both or neither");
  if ((nq > 0 && (!query || !indices || !scores || !counts)) || (nd > 0 && !db)) return fail(MPSFM_EINVAL, "NULL pointer");
  if (!std::isfinite(o.min_score)) return fail(MPSFM_EINVAL, "non-finite min_score");
  const bool same = query == db && nq == nd;  // one set: scanned and uploaded once
  if (!o.inputs_on_device && (!all_finite(query, (size_t)nq * dim) || (!same && !all_finite(db, (size_t)nd * dim))))
    return fail(MPSFM_EINVAL, "non-finite descriptor value");
  if (nq == 0) return 0;
  const int32_t K = o.num_select;
  if (nd == 0) { fill_empty_lists(nq, K, indices, scores, counts); return 0; }
  if (int rc = open_device(device)) return rc;
  CallScope A;
  if (int rc = A.open(true)) return rc;
  const float *dq = query, *dd = db;
  int32_t* d_bad = nullptr;
  if (o.inputs_on_device) {
    if (int rc = check_device_pointer(query, device, "query")) return rc;
    if (int rc = check_device_pointer(db, device, "db")) return rc;
    if (int rc = wait_for_caller(A, o.stream)) return rc;
    d_bad = A.alloc<int32_t>(1);
    if (!d_bad) return fail(MPSFM_ENOMEM, "hipMalloc failed");
    MPSFM_TRY(hipMemsetAsync(d_bad, 0, sizeof(int32_t), A.st));
  } else {
    dq = A.put(query, (size_t)nq * dim);
    dd = same ? dq : A.put(db, (size_t)nd * dim);
    if (!dq || !dd) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  }
  TopkArgs a{};
  a.Q = dq; a.D = dd;
  a.nq = (int32_t)nq; a.nd = (int32_t)nd; a.dim = dim;
  a.vec = (dim % 4 == 0 && ((uintptr_t)dq % 16) == 0 && ((uintptr_t)dd % 16) == 0) ? 1 : 0;
  a.K = K;
  a.rule.min_score = o.min_score;
  a.rule.use_min = o.use_min_score ? 1 : 0;
  if (query_id) {
    a.rule.qid = A.put(query_id, (size_t)nq);
    a.rule.did = A.put(db_id, (size_t)nd);
    if (!a.rule.qid || !a.rule.did) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  }
  // a strip per workgroup leaves most of the device idle up to a few thousand images: the column tiles of a strip are shared out
  // until there are about kFillPerCU workgroups per compute unit (the rule of the descriptor matcher)
  const int32_t strips = (a.nq + kStrip - 1) / kStrip, col_tiles = (a.nd + kStrip - 1) / kStrip;
  const int32_t most = std::min<int32_t>(col_tiles, kMaxRanges);
  if (o.column_ranges > 0) {
    a.splits = std::min<int32_t>(o.column_ranges, most);
  } else {
    int cus = 0;
    MPSFM_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    const int64_t fill = (int64_t)kFillPerCU * std::max(cus, 1);
    a.splits = (int32_t)std::max<int64_t>(1, std::min<int64_t>(most, (fill + strips - 1) / strips));
  }
  const size_t lists = (size_t)nq * a.splits * K;
  a.val = A.alloc<double>(lists);
  a.idx = A.alloc<int32_t>(lists);
  a.indices = A.alloc<int32_t>((size_t)nq * K);
  a.scores = A.alloc<double>((size_t)nq * K);
  a.counts = A.alloc<int32_t>((size_t)nq);
  if (!a.val || !a.idx || !a.indices || !a.scores || !a.counts) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  const size_t lds = topk_lds_bytes(K);
  if (lds > 64 * 1024)  // beyond the default limit of dynamic LDS
    MPSFM_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_sim_topk), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if (int rc = A.begin()) return rc;
  int64_t launches = 0;
  if (d_bad) {
    if (int rc = scan_device(A, dq, nq * dim, d_bad)) return rc;
    ++launches;
    if (dd != dq || nd != nq) {
      if (int rc = scan_device(A, dd, nd * dim, d_bad)) return rc;
      ++launches;
    }
  }
  hipLaunchKernelGGL(k_sim_topk, dim3((unsigned)strips, (unsigned)a.splits), dim3(kMT), lds, A.st, a);
  MPSFM_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_topk_merge, dim3((unsigned)nq), dim3(64), 0, A.st, a);
  MPSFM_TRY(hipGetLastError());
  launches += 2;
  if (int rc = A.stop()) return rc;
  // everything comes down behind the last launch: one wait
  int32_t bad = 0;
  if (d_bad) MPSFM_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipMemcpyAsync(indices, a.indices, sizeof(int32_t) * (size_t)nq * K, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipMemcpyAsync(scores, a.scores, sizeof(double) * (size_t)nq * K, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipMemcpyAsync(counts, a.counts, sizeof(int32_t) * (size_t)nq, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipStreamSynchronize(A.st));
  float ms = 0.f;
  if (int rc = A.elapsed(&ms)) return rc;
  if (bad) return fail(MPSFM_EINVAL, "non-finite value in a device input");
  if (info) {
    int64_t all = 0;
    for (int64_t i = 0; i < nq; ++i) all += counts[i];
    info->num_pairs = all;
    info->num_launches = launches;
    info->num_syncs = 1;
    info->ms = ms;
    info->column_ranges = a.splits;
  }
  return 0;
}
