// Inlier matches of all image pairs to the correspondence graph (mpsfm_corr_graph_build; semantics: include/mpsfm_hip.h, the
// design, what it rests on and the measurements: DESIGN.md section 4s; reference: COLMAP 3.11 CorrespondenceGraph::
// AddCorrespondences + Finalize, restated as a set rule).
//
// A global sort, no atomics and no per-row loop: every step is one thread per entry, so a keypoint matched in a hundred images
// costs what a hundred keypoints matched once cost, and every output is a function of the input alone.
//
//   k_cg_keys        a match -> its status (added so far / invalid / self pair) and its two directed entries, key (src, dst)
//   radix sort       the directed entries by (src, dst), the match position as payload; stable, so equal entries keep the
//                    order of their positions
//   k_cg_first       the first of a run of equal entries stays; the others mark their match a duplicate
//   scan             the place of every kept entry: corr_kp
//   k_cg_fill        corr_kp; the kept entries with src < dst become the pair view's entries, key (image0, image1)
//   k_cg_rows        corr_start[k]: the kept entries below the first entry of keypoint k (a binary search per keypoint)
//   k_cg_kp_flags    kp_two_view
//   k_cg_images      a workgroup per image: correspondences and observations
//   radix sort       the pair view's entries by (image0, image1) only; stable, so (idx0, idx1) stays ascending inside a pair
//   k_cg_pair_first, scan, k_cg_pairs   the distinct pairs and where their matches start
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cstring>
#include <string>

#include "call_scope.h"
#include "common.h"

namespace mpsfm {

namespace {
constexpr int kCT = 256;

enum : uint8_t { kAdded = 0, kInvalid = 1, kSelfPair = 2, kDuplicate = 3 };

inline dim3 cg_blocks(int64_t n) { return dim3((unsigned)((n + kCT - 1) / kCT)); }

template <class F>
int cg_with_temp(CallScope& A, F&& f) {
  size_t bytes = 0;
  MPSFM_TRY(f(nullptr, bytes));
  void* tmp = A.get(std::max<size_t>(bytes, 16));
  if (!tmp) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  MPSFM_TRY(f(tmp, bytes));
  return 0;
}

struct CgArgs {
  int32_t n_images, n_lists;
  int64_t n_kp, M, E;          // E = 2 M directed entries
  uint32_t kp_bits, im_bits;   // 2^kp_bits > n_kp, 2^im_bits > n_images: n_kp and n_images are the sentinels
  const int64_t* kp_start;     // [n_images + 1]
  const int32_t *li0, *li1;    // [n_lists]
  const int64_t* lstart;       // [n_lists + 1]
  const int32_t* matches;      // [M][2]
  uint8_t* status;             // [M]
  int32_t* mlist;              // [M] the list of a match
  uint64_t *key_a, *key_b;     // [E]
  uint32_t *val_a, *val_b;     // [E]
  uint64_t *pval_a, *pval_b;   // [E] (idx0, idx1) of the pair view, idx0 in the low word
  int32_t *flag, *pos;         // [E + 1]
  int64_t* corr_start;         // [n_kp + 1]
  int64_t* corr_kp;            // [E]
  int32_t *im_corr, *im_obs;   // [n_images]
  uint8_t* two_view;           // [n_kp]
  int32_t *pair_im0, *pair_im1;  // [n_lists]
  int64_t* pair_start;           // [n_lists + 1]
  int32_t* totals;               // [2] kept directed entries, pairs
};

__global__ __launch_bounds__(kCT) void k_cg_keys(CgArgs a) {
  const int64_t m = (int64_t)blockIdx.x * kCT + threadIdx.x;
  if (m >= a.M) return;
  // the list of match m: the last l with lstart[l] <= m (empty lists share their start with the next one)
  int32_t lo = 0, hi = a.n_lists;  // lstart[lo] <= m < lstart[hi]
  while (hi - lo > 1) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (a.lstart[mid] <= m) lo = mid; else hi = mid;
  }
  const int32_t ia = a.li0[lo], ib = a.li1[lo];
  const int2 mm = reinterpret_cast<const int2*>(a.matches)[m];
  const int64_t ka = a.kp_start[ia], kb = a.kp_start[ib];
  const int64_t na = a.kp_start[ia + 1] - ka, nb = a.kp_start[ib + 1] - kb;
  uint8_t st = kAdded;
  if (ia == ib) st = kSelfPair;
  else if (mm.x < 0 || mm.x >= na || mm.y < 0 || mm.y >= nb) st = kInvalid;
  a.status[m] = st;
  a.mlist[m] = lo;
  const uint64_t none = (uint64_t)a.n_kp << a.kp_bits;
  uint64_t k0 = none, k1 = none;
  if (st == kAdded) {
    const uint64_t g0 = (uint64_t)(ka + mm.x), g1 = (uint64_t)(kb + mm.y);
    k0 = (g0 << a.kp_bits) | g1;
    k1 = (g1 << a.kp_bits) | g0;
  }
  reinterpret_cast<ulonglong2*>(a.key_a)[m] = make_ulonglong2(k0, k1);
  reinterpret_cast<uint2*>(a.val_a)[m] = make_uint2((uint32_t)m, (uint32_t)m);
}

// over the sorted entries (key_b, val_b); flag[E] = 0 closes the scan
__global__ __launch_bounds__(kCT) void k_cg_first(CgArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kCT + threadIdx.x;
  if (i > a.E) return;
  if (i == a.E) { a.flag[i] = 0; return; }
  const uint64_t k = a.key_b[i];
  const uint64_t src = k >> a.kp_bits, dst = k & ((1ull << a.kp_bits) - 1);
  const bool valid = src < (uint64_t)a.n_kp;
  const bool first = valid && (i == 0 || a.key_b[i - 1] != k);
  a.flag[i] = first ? 1 : 0;
  if (valid && !first && src < dst) a.status[a.val_b[i]] = kDuplicate;  // one of the two directions says it
}

// corr_kp, and the pair view's entries into (key_a, pval_a): key_a is free since the sort
__global__ __launch_bounds__(kCT) void k_cg_fill(CgArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kCT + threadIdx.x;
  if (i >= a.E) return;
  const uint64_t k = a.key_b[i];
  const uint64_t src = k >> a.kp_bits, dst = k & ((1ull << a.kp_bits) - 1);
  uint64_t pk = (uint64_t)a.n_images << a.im_bits, pv = 0;
  if (a.flag[i]) {
    a.corr_kp[a.pos[i]] = (int64_t)dst;
    if (src < dst) {  // keypoints ascend with the image index: src lies in the lower image
      const int32_t l = a.mlist[a.val_b[i]];
      const int32_t ia = a.li0[l], ib = a.li1[l];
      const int32_t i0 = ia < ib ? ia : ib, i1 = ia < ib ? ib : ia;
      pk = ((uint64_t)i0 << a.im_bits) | (uint64_t)i1;
      pv = (uint64_t)(uint32_t)(src - (uint64_t)a.kp_start[i0]) | ((uint64_t)(uint32_t)(dst - (uint64_t)a.kp_start[i1]) << 32);
    }
  }
  a.key_a[i] = pk;
  a.pval_a[i] = pv;
}

__global__ __launch_bounds__(kCT) void k_cg_rows(CgArgs a) {
  const int64_t k = (int64_t)blockIdx.x * kCT + threadIdx.x;
  if (k > a.n_kp) return;
  const uint64_t want = (uint64_t)k << a.kp_bits;  // below every entry of keypoint k, above every entry before it
  int64_t lo = 0, hi = a.E;                        // the first i with key_b[i] >= want
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (a.key_b[mid] < want) lo = mid + 1; else hi = mid;
  }
  a.corr_start[k] = a.pos[lo];  // pos[E]: all kept entries
}

__global__ __launch_bounds__(kCT) void k_cg_kp_flags(CgArgs a) {
  const int64_t k = (int64_t)blockIdx.x * kCT + threadIdx.x;
  if (k >= a.n_kp) return;
  const int64_t s = a.corr_start[k];
  uint8_t tv = 0;
  if (a.corr_start[k + 1] - s == 1) {
    const int64_t p = a.corr_kp[s];
    tv = a.corr_start[p + 1] - a.corr_start[p] == 1 ? 1 : 0;
  }
  a.two_view[k] = tv;
}

__global__ __launch_bounds__(kCT) void k_cg_images(CgArgs a) {
  __shared__ int32_t s_part[kCT / 64];
  const int32_t im = (int32_t)blockIdx.x;
  const int64_t b = a.kp_start[im], e = a.kp_start[im + 1];
  int32_t n = 0;
  for (int64_t k = b + threadIdx.x; k < e; k += kCT) n += a.corr_start[k + 1] > a.corr_start[k] ? 1 : 0;
  for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t all = 0;
    for (int w = 0; w < kCT / 64; ++w) all += s_part[w];
    a.im_obs[im] = all;
    a.im_corr[im] = (int32_t)(a.corr_start[e] - a.corr_start[b]);
  }
}

// over the sorted pair entries (key_b, pval_b)
__global__ __launch_bounds__(kCT) void k_cg_pair_first(CgArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kCT + threadIdx.x;
  if (i > a.E) return;
  if (i == a.E) { a.flag[i] = 0; return; }
  const uint64_t k = a.key_b[i];
  const bool valid = (k >> a.im_bits) < (uint64_t)a.n_images;
  a.flag[i] = (valid && (i == 0 || a.key_b[i - 1] != k)) ? 1 : 0;
}

__global__ __launch_bounds__(kCT) void k_cg_pairs(CgArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kCT + threadIdx.x;
  if (i > a.E) return;
  const bool valid = i < a.E && (a.key_b[i] >> a.im_bits) < (uint64_t)a.n_images;
  if (valid) {
    if (a.flag[i]) {
      const uint64_t k = a.key_b[i];
      const int32_t p = a.pos[i];  // < n_lists: every distinct pair has a list of its own
      a.pair_im0[p] = (int32_t)(k >> a.im_bits);
      a.pair_im1[p] = (int32_t)(k & ((1ull << a.im_bits) - 1));
      a.pair_start[p] = i;
    }
  } else if (i == 0 || (a.key_b[i - 1] >> a.im_bits) < (uint64_t)a.n_images) {
    a.pair_start[a.pos[i]] = i;  // the end of the last pair: pos is the number of pairs here
  }
}

uint32_t bits_above(int64_t n) {  // the least b with 2^b > n
  uint32_t b = 1;
  while ((1ll << b) <= n) ++b;
  return b;
}
}  // namespace

}  // namespace mpsfm

using namespace mpsfm;

extern "C" int mpsfm_corr_graph_build(int32_t n_images, const int64_t* kp_start, int32_t n_lists, const int32_t* list_image0,
                                      const int32_t* list_image1, const int64_t* list_start, const int32_t* matches, int32_t device,
                                      uint8_t* match_status, int64_t* corr_start, int64_t* corr_kp, int64_t* n_corr,
                                      int32_t* image_num_correspondences, int32_t* image_num_observations, uint8_t* kp_two_view,
                                      int64_t* n_pairs, int32_t* pair_image0, int32_t* pair_image1, int64_t* pair_start, int32_t* pair_matches,
                                      mpsfm_corr_graph_info* info) {
  if (info) *info = mpsfm_corr_graph_info{};
  if (n_images < 0 || n_lists < 0) return fail(MPSFM_EINVAL, "negative size");
  if (!kp_start || !list_start || !corr_start || !n_corr || !n_pairs || !pair_start) return fail(MPSFM_EINVAL, "NULL pointer");
  if (n_images > 0 && (!image_num_correspondences || !image_num_observations)) return fail(MPSFM_EINVAL, "NULL pointer");
  if (n_lists > 0 && (!list_image0 || !list_image1 || !pair_image0 || !pair_image1)) return fail(MPSFM_EINVAL, "NULL pointer");
  if (kp_start[0] != 0 || list_start[0] != 0) return fail(MPSFM_EINVAL, "kp_start[0] and list_start[0] must be 0");
  for (int32_t i = 0; i < n_images; ++i)
    if (kp_start[i + 1] < kp_start[i]) return fail(MPSFM_EINVAL, "kp_start must not decrease");
  for (int32_t l = 0; l < n_lists; ++l) {
    if (list_start[l + 1] < list_start[l]) return fail(MPSFM_EINVAL, "list_start must not decrease");
    if (list_image0[l] < 0 || list_image0[l] >= n_images || list_image1[l] < 0 || list_image1[l] >= n_images)
      return fail(MPSFM_EINVAL, "list image index out of range");
  }
  const int64_t n_kp = kp_start[n_images], M = list_start[n_lists];
  if (n_kp > 0 && !kp_two_view) return fail(MPSFM_EINVAL, "NULL pointer");
  if (M > 0 && (!matches || !match_status || !corr_kp || !pair_matches)) return fail(MPSFM_EINVAL, "NULL pointer");
  if (n_kp >= (1ll << 31)) return fail(MPSFM_EUNSUPPORTED, "2^31 keypoints or more");
  if (M >= (1ll << 30)) return fail(MPSFM_EUNSUPPORTED, "2^31 directed correspondences or more");
  const int64_t E = 2 * M;

  // what an empty graph looks like; the tails behind n_corr / n_pairs of a full one are zero as well
  auto counts_zero = [&] {
    for (int64_t k = 0; k <= n_kp; ++k) corr_start[k] = 0;
    for (int64_t k = 0; k < n_kp; ++k) kp_two_view[k] = 0;
    for (int32_t i = 0; i < n_images; ++i) image_num_correspondences[i] = image_num_observations[i] = 0;
    *n_corr = 0;
    *n_pairs = 0;
    pair_start[0] = 0;
  };
  if (M == 0 || n_kp == 0) {  // no device needed: without keypoints no index is in range
    counts_zero();
    for (int32_t l = 0; l < n_lists; ++l) {
      pair_image0[l] = pair_image1[l] = 0;
      pair_start[l + 1] = 0;
      for (int64_t m = list_start[l]; m < list_start[l + 1]; ++m) match_status[m] = list_image0[l] == list_image1[l] ? kSelfPair : kInvalid;
    }
    if (M > 0) {
      std::memset(corr_kp, 0, sizeof(int64_t) * (size_t)E);
      std::memset(pair_matches, 0, sizeof(int32_t) * (size_t)E);
    }
    if (info)
      for (int64_t m = 0; m < M; ++m) (match_status[m] == kSelfPair ? info->num_self_pairs : info->num_invalid) += 1;
    return 0;
  }

  if (int rc = open_device(device)) return rc;
  CallScope A;
  if (int rc = A.open(true)) return rc;
  CgArgs a{};
  a.n_images = n_images; a.n_lists = n_lists;
  a.n_kp = n_kp; a.M = M; a.E = E;
  a.kp_bits = bits_above(n_kp);
  a.im_bits = bits_above(n_images);
  a.kp_start = A.put(kp_start, (size_t)n_images + 1);
  a.li0 = A.put(list_image0, (size_t)n_lists);
  a.li1 = A.put(list_image1, (size_t)n_lists);
  a.lstart = A.put(list_start, (size_t)n_lists + 1);
  a.matches = A.put(matches, (size_t)E);
  a.status = A.alloc<uint8_t>((size_t)M);
  a.mlist = A.alloc<int32_t>((size_t)M);
  a.key_a = A.alloc<uint64_t>((size_t)E);
  a.key_b = A.alloc<uint64_t>((size_t)E);
  a.val_a = A.alloc<uint32_t>((size_t)E);
  a.val_b = A.alloc<uint32_t>((size_t)E);
  a.pval_a = A.alloc<uint64_t>((size_t)E);
  a.pval_b = A.alloc<uint64_t>((size_t)E);
  a.flag = A.alloc<int32_t>((size_t)E + 1);
  a.pos = A.alloc<int32_t>((size_t)E + 1);
  a.corr_start = A.alloc<int64_t>((size_t)n_kp + 1);
  a.corr_kp = A.alloc<int64_t>((size_t)E);
  a.im_corr = A.alloc<int32_t>((size_t)n_images);
  a.im_obs = A.alloc<int32_t>((size_t)n_images);
  a.two_view = A.alloc<uint8_t>((size_t)n_kp);
  a.pair_im0 = A.alloc<int32_t>((size_t)n_lists);
  a.pair_im1 = A.alloc<int32_t>((size_t)n_lists);
  a.pair_start = A.alloc<int64_t>((size_t)n_lists + 1);
  a.totals = A.alloc<int32_t>(2);
  if (!a.totals || !a.kp_start || !a.li0 || !a.li1 || !a.lstart || !a.matches || !a.status || !a.mlist || !a.key_a || !a.key_b || !a.val_a || !a.val_b ||
      !a.pval_a || !a.pval_b || !a.flag || !a.pos || !a.corr_start || !a.corr_kp || !a.im_corr || !a.im_obs || !a.two_view || !a.pair_im0 ||
      !a.pair_im1 || !a.pair_start)
    return fail(MPSFM_ENOMEM, "hipMalloc failed");
  int64_t launches = 0;
  auto launched = [&]() -> int { MPSFM_TRY(hipGetLastError()); ++launches; return 0; };
  if (int rc = A.begin()) return rc;
  hipLaunchKernelGGL(k_cg_keys, cg_blocks(M), dim3(kCT), 0, A.st, a);
  if (int rc = launched()) return rc;
  if (int rc = cg_with_temp(A, [&](void* t, size_t& b) {
        return rocprim::radix_sort_pairs(t, b, a.key_a, a.key_b, a.val_a, a.val_b, (size_t)E, 0, 2 * a.kp_bits, A.st);
      }))
    return rc;
  hipLaunchKernelGGL(k_cg_first, cg_blocks(E + 1), dim3(kCT), 0, A.st, a);
  if (int rc = launched()) return rc;
  if (int rc = cg_with_temp(A, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, a.flag, a.pos, 0, (size_t)E + 1, rocprim::plus<int32_t>(), A.st); }))
    return rc;
  hipLaunchKernelGGL(k_cg_fill, cg_blocks(E), dim3(kCT), 0, A.st, a);
  if (int rc = launched()) return rc;
  hipLaunchKernelGGL(k_cg_rows, cg_blocks(n_kp + 1), dim3(kCT), 0, A.st, a);
  if (int rc = launched()) return rc;
  hipLaunchKernelGGL(k_cg_kp_flags, cg_blocks(n_kp), dim3(kCT), 0, A.st, a);
  if (int rc = launched()) return rc;
  hipLaunchKernelGGL(k_cg_images, dim3((unsigned)n_images), dim3(kCT), 0, A.st, a);
  if (int rc = launched()) return rc;
  MPSFM_TRY(hipMemcpyAsync(a.totals, a.pos + E, sizeof(int32_t), hipMemcpyDeviceToDevice, A.st));  // before the second scan reuses pos
  // the pair view: key_b is free now
  if (int rc = cg_with_temp(A, [&](void* t, size_t& b) {
        return rocprim::radix_sort_pairs(t, b, a.key_a, a.key_b, a.pval_a, a.pval_b, (size_t)E, 0, 2 * a.im_bits, A.st);
      }))
    return rc;
  hipLaunchKernelGGL(k_cg_pair_first, cg_blocks(E + 1), dim3(kCT), 0, A.st, a);
  if (int rc = launched()) return rc;
  if (int rc = cg_with_temp(A, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, a.flag, a.pos, 0, (size_t)E + 1, rocprim::plus<int32_t>(), A.st); }))
    return rc;
  hipLaunchKernelGGL(k_cg_pairs, cg_blocks(E + 1), dim3(kCT), 0, A.st, a);
  if (int rc = launched()) return rc;
  if (int rc = A.stop()) return rc;
  // everything comes down behind the last launch, at its capacity: one wait of our own.  The caller's arrays are pageable, so the
  // runtime stages these copies (and the uploads above) and may hold the host on each: num_syncs does not count that.
  int32_t h_totals[2] = {0, 0};
  MPSFM_TRY(hipMemcpyAsync(a.totals + 1, a.pos + E, sizeof(int32_t), hipMemcpyDeviceToDevice, A.st));
  MPSFM_TRY(hipMemcpyAsync(h_totals, a.totals, sizeof(h_totals), hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipMemcpyAsync(match_status, a.status, (size_t)M, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipMemcpyAsync(corr_start, a.corr_start, sizeof(int64_t) * ((size_t)n_kp + 1), hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipMemcpyAsync(corr_kp, a.corr_kp, sizeof(int64_t) * (size_t)E, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipMemcpyAsync(image_num_correspondences, a.im_corr, sizeof(int32_t) * (size_t)n_images, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipMemcpyAsync(image_num_observations, a.im_obs, sizeof(int32_t) * (size_t)n_images, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipMemcpyAsync(kp_two_view, a.two_view, (size_t)n_kp, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipMemcpyAsync(pair_image0, a.pair_im0, sizeof(int32_t) * (size_t)n_lists, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipMemcpyAsync(pair_image1, a.pair_im1, sizeof(int32_t) * (size_t)n_lists, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipMemcpyAsync(pair_start, a.pair_start, sizeof(int64_t) * ((size_t)n_lists + 1), hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipMemcpyAsync(pair_matches, a.pval_b, sizeof(uint64_t) * (size_t)M, hipMemcpyDeviceToHost, A.st));  // the kept entries lead
  MPSFM_TRY(hipStreamSynchronize(A.st));
  float ms = 0.f;
  if (int rc = A.elapsed(&ms)) return rc;
  const int32_t h_corr = h_totals[0], h_pairs = h_totals[1];
  if (h_corr < 0 || h_corr > E || h_corr % 2 != 0 || h_pairs < 0 || h_pairs > n_lists) return fail(MPSFM_EHIP, "correspondence graph: impossible counts");
  *n_corr = h_corr;
  *n_pairs = h_pairs;
  // the capacity behind the counts held whatever the device blocks held before
  std::memset(corr_kp + h_corr, 0, sizeof(int64_t) * (size_t)(E - h_corr));
  std::memset(pair_matches + h_corr, 0, sizeof(int32_t) * (size_t)(E - h_corr));  // h_corr / 2 kept matches of two indices
  for (int32_t p = h_pairs; p < n_lists; ++p) pair_image0[p] = pair_image1[p] = 0;
  for (int32_t p = h_pairs + 1; p <= n_lists; ++p) pair_start[p] = 0;
  if (info) {
    for (int64_t m = 0; m < M; ++m) {
      const uint8_t s = match_status[m];
      (s == kAdded ? info->num_added : s == kInvalid ? info->num_invalid : s == kSelfPair ? info->num_self_pairs : info->num_duplicates) += 1;
    }
    info->num_launches = launches;
    info->num_syncs = 1;
    info->ms = ms;
  }
  return 0;
}
