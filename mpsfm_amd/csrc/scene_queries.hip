// What the incremental loop asks of a scene between two registrations (semantics: include/mpsfm_hip.h; the design and the
// measurements: DESIGN.md section 4t): COLMAP 3.11's per-image visibility statistics (mpsfm_visibility_scores) and
// IncrementalMapper::FindLocalBundle for many reference images at once (mpsfm_local_bundles).  Both read the arrays of mpsfm_tri_graph /
// mpsfm_tri_state as the track engine gathers them.
//
//   k_sq_visibility  a workgroup per image: the visible keypoints into a Z-ordered bitmap of the finest pyramid level in LDS, the
//                    coarser levels folded from it, the cells counted with __popcll.  Integers only, no global atomics.
//   k_lb_centres     projection centres of all images
//   k_lb_marks       m_r(p): how many keypoints of reference r observe point p
//   k_lb_angles      a workgroup per run of image j's keypoints and reference: shared count and list length summed in registers and
//                    LDS, one packed integer add per workgroup, which also reserves the workgroup's run inside segment (r, j); then
//                    the angles into that run
//   k_lb_select      a workgroup per segment: the element of rank floor(0.75 (n - 1) + 0.5), by MSB-first radix select over the bit
//                    patterns (non-negative doubles order as their patterns), 256-bin histograms in LDS; short segments are held in LDS
// The threshold walk over the few hundred (shared, angle75) of a reference runs on the host behind the one wait
// (local_bundle_walk.h).
#include <cstring>
#include <string>
#include <vector>

#include "call_scope.h"
#include "common.h"
#include "local_bundle_walk.h"
#include "tri_math.h"

namespace mpsfm {

namespace {
constexpr int kQT = 256;             // threads of every workgroup here
constexpr int kQW = kQT / 64;        // its waves
constexpr int kMaxLevels = 8;        // 4^8 bits = 8 KB of LDS
constexpr int kRun = 4;              // keypoints per thread of k_lb_angles: a run is kQT * kRun keypoints
constexpr int kSelectLds = 2048;     // angles of a segment that k_lb_select keeps in LDS (16 KB)
constexpr int64_t kAngleBudget = 16ll << 20;  // angles (and marks) of one group of references: 128 MB + 64 MB at most

inline dim3 sq_blocks(int64_t n) { return dim3((unsigned)((n + kQT - 1) / kQT)); }

// ---- visibility ---------------------------------------------------------------------------------------------------------------
struct VisArgs {
  int32_t num_levels;
  const int64_t* kp_start;    // [n_images + 1]
  const double* kp_xy;        // [n_kp][2]
  const int64_t* corr_start;  // [n_kp + 1]
  const int64_t* corr_kp;     // [n_corr]
  const int64_t* kp_point;    // [n_kp]
  const int32_t* image_size;  // [n_images][2]
  int32_t* num_visible;       // [n_images]
  int64_t* score;             // [n_images]
  uint8_t* kp_visible;        // [n_kp] or nullptr
};

// clamp((int64) trunc(D x / size), 0, D - 1); a negative or NaN operand gives 0.  D x is exact (a power of two): nothing to contract.
__device__ inline uint32_t pyramid_cell(double x, int32_t size, int32_t D) {
  const double v = (double)D * x / (double)size;
  if (!(v >= 0.0)) return 0;
  return v >= (double)D ? (uint32_t)(D - 1) : (uint32_t)(int64_t)v;
}

// bit 2i of the result is bit i of v (v < 256)
__device__ inline uint32_t spread_bits(uint32_t v) {
  v = (v | (v << 4)) & 0x0f0fu;
  v = (v | (v << 2)) & 0x3333u;
  v = (v | (v << 1)) & 0x5555u;
  return v;
}

__global__ __launch_bounds__(kQT) void k_sq_visibility(VisArgs a) {
  // bit z of the bitmap: the finest cell with Z-order index z = interleave(cy, cx), so the cell of level l is z >> 2 (L - l) and a
  // cell's four children are four neighbouring bits
  __shared__ uint32_t s_bits[(1 << (2 * kMaxLevels)) / 32];
  __shared__ uint32_t s_any[(1 << (2 * kMaxLevels)) / 64];
  __shared__ int32_t s_vis[kQW];
  __shared__ long long s_score[kQW];
  const int32_t im = (int32_t)blockIdx.x, L = a.num_levels, D = 1 << L;
  const int32_t n_bits = 1 << (2 * L);
  const int32_t n_words = n_bits >= 64 ? n_bits / 64 : 1;  // 64-bit words
  for (int w = threadIdx.x; w < 2 * n_words; w += kQT) s_bits[w] = 0;
  __syncthreads();
  const int64_t b = a.kp_start[im], e = a.kp_start[im + 1];
  const int32_t width = a.image_size[2 * im], height = a.image_size[2 * im + 1];
  int32_t nvis = 0;
  for (int64_t k = b + threadIdx.x; k < e; k += kQT) {
    bool vis = false;
    for (int64_t c = a.corr_start[k], ce = a.corr_start[k + 1]; c < ce && !vis; ++c) vis = a.kp_point[a.corr_kp[c]] >= 0;
    if (a.kp_visible) a.kp_visible[k] = vis ? 1 : 0;
    if (!vis) continue;
    ++nvis;
    const double2 xy = reinterpret_cast<const double2*>(a.kp_xy)[k];
    const uint32_t z = spread_bits(pyramid_cell(xy.x, width, D)) | (spread_bits(pyramid_cell(xy.y, height, D)) << 1);
    atomicOr(&s_bits[z >> 5], 1u << (z & 31));
  }
  __syncthreads();
  // levels L, L - 1, L - 2 (cells of 1, 4, 16 bits) and the word's own flag, per 64-bit word
  long long sc = 0;
  for (int w = threadIdx.x; w < n_words; w += kQT) {
    const uint64_t v = (uint64_t)s_bits[2 * w] | ((uint64_t)s_bits[2 * w + 1] << 32);
    sc += (long long)__popcll(v) << (2 * L);
    if (L >= 2) {
      const uint64_t f4 = (v | (v >> 1) | (v >> 2) | (v >> 3)) & 0x1111111111111111ull;
      sc += (long long)__popcll(f4) << (2 * (L - 1));
      if (L >= 3) {
        const uint64_t f16 = (f4 | (f4 >> 4) | (f4 >> 8) | (f4 >> 12)) & 0x0001000100010001ull;
        sc += (long long)__popcll(f16) << (2 * (L - 2));
      }
    }
    s_any[w] = v != 0 ? 1u : 0u;
  }
  __syncthreads();
  // levels L - 3 and coarser: a cell is a run of 1, 4, 16, ... words; s_any is folded in place, four to one per level
  static_assert((1 << (2 * kMaxLevels)) / 64 / 4 <= kQT, "a folded level is at most one cell per thread");
  int32_t n_cells = n_words;
  for (int32_t l = L - 3; l >= 1; --l) {
    for (int w = threadIdx.x; w < n_cells; w += kQT) sc += (long long)s_any[w] << (2 * l);
    if (l == 1) break;
    n_cells >>= 2;
    const int t = threadIdx.x;
    const uint32_t any = t < n_cells ? (s_any[4 * t] | s_any[4 * t + 1] | s_any[4 * t + 2] | s_any[4 * t + 3]) : 0u;
    __syncthreads();  // every read of the finer level lies before the writes of the coarser one
    if (t < n_cells) s_any[t] = any;
    __syncthreads();
  }
  for (int off = 32; off > 0; off >>= 1) {
    nvis += __shfl_down(nvis, off, 64);
    sc += __shfl_down(sc, off, 64);
  }
  if ((threadIdx.x & 63) == 0) { s_vis[threadIdx.x >> 6] = nvis; s_score[threadIdx.x >> 6] = sc; }
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t v = 0;
    long long s = 0;
    for (int w = 0; w < kQW; ++w) { v += s_vis[w]; s += s_score[w]; }
    a.num_visible[im] = v;
    a.score[im] = s;
  }
}

// ---- local bundles ------------------------------------------------------------------------------------------------------------
struct LbArgs {
  int32_t n_images, n_group;       // references of this group
  int64_t n_kp, n_points;
  const int64_t* kp_start;         // [n_images + 1]
  const double *quat, *trans;      // [n_images][4], [n_images][3]
  const int64_t* kp_point;         // [n_kp]
  const double* xyz;               // [n_points][3]
  const int32_t* ref;              // [n_group] of this group
  const int32_t* run_image;        // [n_runs] runs of at most kQT * kRun keypoints of one registered image
  const int64_t* run_begin;        // [n_runs] first keypoint (global index); the run ends with its image
  double* centre;                  // [n_images][3]
  int32_t* mark;                   // [n_group][n_points]
  unsigned long long* count;       // [n_group][n_images] list length in the low word, shared count in the high word
  double* angle;                   // [n_group][n_kp]: segment (g, j) starts at g n_kp + kp_start[j], capacity nkp(j)
  int32_t* shared;                 // [n_group][n_images] of this group
  double* angle75;                 // [n_group][n_images]
};

__global__ __launch_bounds__(kQT) void k_lb_centres(LbArgs a) {
  const int32_t i = (int32_t)(blockIdx.x * kQT + threadIdx.x);
  if (i >= a.n_images) return;
  double R[9];
  quat_to_R(a.quat + 4 * i, R);
  const double* t = a.trans + 3 * i;
  for (int k = 0; k < 3; ++k) a.centre[3 * i + k] = -(R[k] * t[0] + R[3 + k] * t[1] + R[6 + k] * t[2]);
}

// grid (runs of the longest reference image, n_group).  Integer adds: the sums do not depend on arrival order.
__global__ __launch_bounds__(kQT) void k_lb_marks(LbArgs a) {
  const int32_t g = (int32_t)blockIdx.y, r = a.ref[g];
  const int64_t k = a.kp_start[r] + (int64_t)blockIdx.x * kQT + threadIdx.x;
  if (k >= a.kp_start[r + 1]) return;
  const int64_t p = a.kp_point[k];
  if (p >= 0) atomicAdd(&a.mark[(int64_t)g * a.n_points + p], 1);
}

// grid (n_runs, n_group)
__global__ __launch_bounds__(kQT) void k_lb_angles(LbArgs a) {
  __shared__ int32_t s_cnt[kQW];
  __shared__ long long s_sum[kQW];
  __shared__ long long s_base;
  const int32_t g = (int32_t)blockIdx.y, r = a.ref[g], j = a.run_image[blockIdx.x];
  if (j == r) return;
  const int64_t begin = a.run_begin[blockIdx.x], image_end = a.kp_start[j + 1];
  const int32_t* mark = a.mark + (int64_t)g * a.n_points;
  int64_t pt[kRun];
  int32_t cnt = 0;
  long long sum = 0;
#pragma unroll
  for (int i = 0; i < kRun; ++i) {
    const int64_t k = begin + i * kQT + threadIdx.x;
    pt[i] = -1;
    if (k < image_end) {
      const int64_t p = a.kp_point[k];
      const int32_t m = p >= 0 ? mark[p] : 0;
      if (m > 0) { pt[i] = p; ++cnt; sum += m; }
    }
  }
  // where this thread's angles go inside the workgroup's run: an exclusive prefix of cnt over the threads
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int32_t incl = cnt;
  for (int off = 1; off < 64; off <<= 1) {
    const int32_t up = __shfl_up(incl, off, 64);
    if (lane >= off) incl += up;
  }
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
  if (lane == 63) s_cnt[wave] = incl;
  if (lane == 0) s_sum[wave] = sum;
  __syncthreads();
  int32_t before = 0, total = 0;
  for (int w = 0; w < kQW; ++w) {
    if (w < wave) before += s_cnt[w];
    total += s_cnt[w];
  }
  if (total == 0) return;  // the same for every thread
  if (threadIdx.x == 0) {
    long long all = 0;
    for (int w = 0; w < kQW; ++w) all += s_sum[w];
    const unsigned long long old =
        atomicAdd(&a.count[(int64_t)g * a.n_images + j], ((unsigned long long)all << 32) | (unsigned long long)(uint32_t)total);
    s_base = (long long)(old & 0xffffffffull);
  }
  __syncthreads();
  // at most nkp(j) entries reach segment (g, j): one per keypoint of j
  double* out = a.angle + (int64_t)g * a.n_kp + a.kp_start[j] + s_base + before + (incl - cnt);
  const double *Cr = a.centre + 3 * r, *Cj = a.centre + 3 * j;
#pragma unroll
  for (int i = 0; i < kRun; ++i)
    if (pt[i] >= 0) *out++ = tri_angle(Cr, Cj, a.xyz + 3 * pt[i]);
}

// grid (n_images, n_group)
__global__ __launch_bounds__(kQT) void k_lb_select(LbArgs a) {
  __shared__ uint64_t s_buf[kSelectLds];
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_wave[kQW];
  __shared__ uint32_t s_pick[2];  // the bin that holds the rank, the elements below it
  const int32_t j = (int32_t)blockIdx.x, g = (int32_t)blockIdx.y;
  const int64_t seg = (int64_t)g * a.n_images + j;
  const unsigned long long packed = a.count[seg];
  const uint32_t n = (uint32_t)(packed & 0xffffffffull);
  if (threadIdx.x == 0) {
    a.shared[seg] = (int32_t)(packed >> 32);
    if (n == 0) a.angle75[seg] = -1.0;
  }
  if (n == 0) return;
  const uint64_t* src = reinterpret_cast<const uint64_t*>(a.angle + (int64_t)g * a.n_kp + a.kp_start[j]);
  if (n <= (uint32_t)kSelectLds) {
    for (uint32_t i = threadIdx.x; i < n; i += kQT) s_buf[i] = src[i];
    src = s_buf;  // generic pointer: the reads below go to LDS
  }
  uint32_t rank = (3u * (n - 1) + 2u) / 4u;  // floor(0.75 (n - 1) + 0.5): Percentile with std::round
  uint64_t prefix = 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int byte = 7; byte >= 0; --byte) {
    s_hist[threadIdx.x] = 0;
    __syncthreads();  // also: s_buf is written
    const uint64_t above = byte == 7 ? 0ull : ~0ull << (8 * (byte + 1));
    for (uint32_t i = threadIdx.x; i < n; i += kQT) {
      const uint64_t v = src[i];
      if ((v & above) == prefix) atomicAdd(&s_hist[(v >> (8 * byte)) & 255u], 1u);
    }
    __syncthreads();
    // the bin t with below(t) <= rank < below(t) + hist[t]: exactly one, since rank < the number of elements under the prefix
    const uint32_t h = s_hist[threadIdx.x];
    uint32_t incl = h;
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t up = __shfl_up(incl, off, 64);
      if (lane >= off) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t below = incl - h;
    for (int w = 0; w < wave; ++w) below += s_wave[w];
    if (below <= rank && rank < below + h) { s_pick[0] = threadIdx.x; s_pick[1] = below; }
    __syncthreads();
    prefix |= (uint64_t)s_pick[0] << (8 * byte);
    rank -= s_pick[1];
  }
  if (threadIdx.x == 0) {
    double v;
    memcpy(&v, &prefix, sizeof(v));
    a.angle75[seg] = v;
  }
}

int check_kp_start(int32_t n_images, const int64_t* kp_start) {
  if (kp_start[0] != 0) return fail(MPSFM_EINVAL, "kp_start[0] must be 0");
  for (int32_t i = 0; i < n_images; ++i)
    if (kp_start[i + 1] < kp_start[i]) return fail(MPSFM_EINVAL, "kp_start must not decrease");
  if (kp_start[n_images] >= (1ll << 31)) return fail(MPSFM_EUNSUPPORTED, "2^31 keypoints or more");
  return 0;
}
}  // namespace

}  // namespace mpsfm

using namespace mpsfm;

extern "C" int mpsfm_visibility_scores(int32_t n_images, const int64_t* kp_start, const double* kp_xy, const int64_t* corr_start,
                                       const int64_t* corr_kp, const int64_t* kp_point, const int32_t* image_size, int32_t num_levels,
                                       int32_t device, int32_t* num_visible, int64_t* score, uint8_t* kp_visible,
                                       mpsfm_scene_query_info* info) {
  if (info) *info = mpsfm_scene_query_info{};
  if (n_images < 0) return fail(MPSFM_EINVAL, "negative size");
  if (num_levels < 1 || num_levels > kMaxLevels) return fail(MPSFM_EINVAL, "num_levels must lie in 1 .. 8");
  if (!kp_start) return fail(MPSFM_EINVAL, "NULL pointer");
  if (n_images > 0 && (!image_size || !num_visible || !score)) return fail(MPSFM_EINVAL, "NULL pointer");
  if (int rc = check_kp_start(n_images, kp_start)) return rc;
  const int64_t n_kp = kp_start[n_images];
  if (n_kp > 0 && (!kp_xy || !corr_start || !kp_point)) return fail(MPSFM_EINVAL, "NULL pointer");
  for (int32_t i = 0; i < n_images; ++i)
    if (image_size[2 * i] <= 0 || image_size[2 * i + 1] <= 0) return fail(MPSFM_EINVAL, "image width and height must be positive");
  int64_t n_corr = 0;
  if (n_kp > 0) {
    if (corr_start[0] != 0) return fail(MPSFM_EINVAL, "corr_start[0] must be 0");
    for (int64_t k = 0; k < n_kp; ++k)
      if (corr_start[k + 1] < corr_start[k]) return fail(MPSFM_EINVAL, "corr_start must not decrease");
    n_corr = corr_start[n_kp];
    if (n_corr > 0 && !corr_kp) return fail(MPSFM_EINVAL, "NULL pointer");
    for (int64_t c = 0; c < n_corr; ++c)
      if (corr_kp[c] < 0 || corr_kp[c] >= n_kp) return fail(MPSFM_EINVAL, "corr_kp outside [0, n_kp)");
  }
  if (n_images == 0) return 0;
  if (n_kp == 0) {  // no device needed
    for (int32_t i = 0; i < n_images; ++i) { num_visible[i] = 0; score[i] = 0; }
    return 0;
  }

  if (int rc = open_device(device)) return rc;
  CallScope A;
  if (int rc = A.open(true)) return rc;
  VisArgs a{};
  a.num_levels = num_levels;
  a.kp_start = A.put(kp_start, (size_t)n_images + 1);
  a.kp_xy = A.put(kp_xy, 2 * (size_t)n_kp);
  a.corr_start = A.put(corr_start, (size_t)n_kp + 1);
  a.corr_kp = A.put(corr_kp, (size_t)n_corr);
  a.kp_point = A.put(kp_point, (size_t)n_kp);
  a.image_size = A.put(image_size, 2 * (size_t)n_images);
  a.num_visible = A.alloc<int32_t>((size_t)n_images);
  a.score = A.alloc<int64_t>((size_t)n_images);
  a.kp_visible = kp_visible ? A.alloc<uint8_t>((size_t)n_kp) : nullptr;
  if (!a.kp_start || !a.kp_xy || !a.corr_start || !a.corr_kp || !a.kp_point || !a.image_size || !a.num_visible || !a.score ||
      (kp_visible && !a.kp_visible))
    return fail(MPSFM_ENOMEM, "hipMalloc failed");
  if (int rc = A.begin()) return rc;
  hipLaunchKernelGGL(k_sq_visibility, dim3((unsigned)n_images), dim3(kQT), 0, A.st, a);
  MPSFM_TRY(hipGetLastError());
  if (int rc = A.stop()) return rc;
  MPSFM_TRY(hipMemcpyAsync(num_visible, a.num_visible, sizeof(int32_t) * (size_t)n_images, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipMemcpyAsync(score, a.score, sizeof(int64_t) * (size_t)n_images, hipMemcpyDeviceToHost, A.st));
  if (kp_visible) MPSFM_TRY(hipMemcpyAsync(kp_visible, a.kp_visible, (size_t)n_kp, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipStreamSynchronize(A.st));  // the one wait of the call
  float ms = 0.f;
  if (int rc = A.elapsed(&ms)) return rc;
  if (info) {
    info->num_launches = 1;
    info->num_syncs = 1;
    info->num_groups = 1;
    info->ms = ms;
  }
  return 0;
}

extern "C" int mpsfm_local_bundles(int32_t n_images, const int64_t* kp_start, const mpsfm_tri_state* state, int32_t n_refs,
                                   const int32_t* ref_image, int32_t num_images, double min_tri_angle_deg, int32_t device,
                                   int32_t* bundle, int32_t* bundle_len, int32_t* shared, double* angle75,
                                   mpsfm_scene_query_info* info) {
  if (info) *info = mpsfm_scene_query_info{};
  if (n_images < 0 || n_refs < 0) return fail(MPSFM_EINVAL, "negative size");
  if (num_images < 1) return fail(MPSFM_EINVAL, "num_images must be at least 1");
  if (!(min_tri_angle_deg >= 0.0) || !std::isfinite(min_tri_angle_deg)) return fail(MPSFM_EINVAL, "min_tri_angle_deg must be finite and not negative");
  if (!kp_start || !state) return fail(MPSFM_EINVAL, "NULL pointer");
  if (n_images > 0 && (!state->registered || !state->cam_quat_xyzw || !state->cam_t)) return fail(MPSFM_EINVAL, "NULL pointer");
  if (int rc = check_kp_start(n_images, kp_start)) return rc;
  const int64_t n_kp = kp_start[n_images], n_points = state->n_points;
  if (n_points < 0 || n_points >= (1ll << 31)) return fail(n_points < 0 ? MPSFM_EINVAL : MPSFM_EUNSUPPORTED, "n_points outside [0, 2^31)");
  if ((n_kp > 0 && !state->kp_point) || (n_points > 0 && !state->xyz)) return fail(MPSFM_EINVAL, "NULL pointer");
  if (n_refs > 0 && (!ref_image || !bundle_len || (num_images > 1 && !bundle) || (n_images > 0 && (!shared || !angle75))))
    return fail(MPSFM_EINVAL, "NULL pointer");
  for (int32_t r = 0; r < n_refs; ++r) {
    if (ref_image[r] < 0 || ref_image[r] >= n_images) return fail(MPSFM_EINVAL, "reference image outside [0, n_images)");
    if (!state->registered[ref_image[r]]) return fail(MPSFM_EINVAL, "reference image is not registered");
  }
  for (int64_t k = 0; k < n_kp; ++k)
    if (state->kp_point[k] < -1 || state->kp_point[k] >= n_points) return fail(MPSFM_EINVAL, "kp_point outside [-1, n_points)");
  for (int32_t i = 0; i < n_images; ++i)
    if (state->registered[i] && (!all_finite(state->cam_quat_xyzw + 4 * i, 4) || !all_finite(state->cam_t + 3 * i, 3)))
      return fail(MPSFM_EINVAL, "pose of a registered image is not finite");
  if (!all_finite(state->xyz, 3 * (size_t)n_points)) return fail(MPSFM_EINVAL, "xyz is not finite");
  if (n_refs == 0) return 0;

  const size_t row = (size_t)(num_images - 1);
  // T of every reference, the runs of the registered images' keypoints, the longest reference image
  std::vector<int64_t> ref_T((size_t)n_refs, 0), run_begin;
  std::vector<int32_t> run_image;
  int64_t longest_ref = 0, with_point = 0;
  for (int32_t r = 0; r < n_refs; ++r) {
    const int32_t im = ref_image[r];
    for (int64_t k = kp_start[im]; k < kp_start[im + 1]; ++k) ref_T[r] += state->kp_point[k] >= 0 ? 1 : 0;
    longest_ref = std::max(longest_ref, kp_start[im + 1] - kp_start[im]);
    with_point += ref_T[r];
  }
  for (int32_t i = 0; i < n_images; ++i)
    if (state->registered[i])
      for (int64_t k = kp_start[i]; k < kp_start[i + 1]; k += kQT * kRun) { run_image.push_back(i); run_begin.push_back(k); }
  if (run_image.empty() || with_point == 0 || n_points == 0) {  // nothing can be shared: no device needed
    for (int32_t r = 0; r < n_refs; ++r) {
      bundle_len[r] = 0;
      for (size_t i = 0; i < row; ++i) bundle[r * row + i] = -1;
      for (int32_t j = 0; j < n_images; ++j) { shared[(size_t)r * n_images + j] = 0; angle75[(size_t)r * n_images + j] = -1.0; }
    }
    return 0;
  }

  if (int rc = open_device(device)) return rc;
  CallScope A;
  if (int rc = A.open(true)) return rc;
  // references are worked off in groups that share one workspace; the stream orders the groups, the host waits once at the end
  const int32_t group = (int32_t)std::max<int64_t>(1, std::min<int64_t>(n_refs, kAngleBudget / std::max(n_kp, n_points)));
  LbArgs a{};
  a.n_images = n_images;
  a.n_kp = n_kp; a.n_points = n_points;
  a.kp_start = A.put(kp_start, (size_t)n_images + 1);
  a.quat = A.put(state->cam_quat_xyzw, 4 * (size_t)n_images);
  a.trans = A.put(state->cam_t, 3 * (size_t)n_images);
  a.kp_point = A.put(state->kp_point, (size_t)n_kp);
  a.xyz = A.put(state->xyz, 3 * (size_t)n_points);
  const int32_t* d_ref = A.put(ref_image, (size_t)n_refs);
  a.run_image = A.put(run_image.data(), run_image.size());
  a.run_begin = A.put(run_begin.data(), run_begin.size());
  a.centre = A.alloc<double>(3 * (size_t)n_images);
  a.mark = A.alloc<int32_t>((size_t)group * (size_t)n_points);
  a.count = A.alloc<unsigned long long>((size_t)group * (size_t)n_images);
  a.angle = A.alloc<double>((size_t)group * (size_t)n_kp);
  int32_t* d_shared = A.alloc<int32_t>((size_t)n_refs * (size_t)n_images);
  double* d_angle75 = A.alloc<double>((size_t)n_refs * (size_t)n_images);
  if (!a.kp_start || !a.quat || !a.trans || !a.kp_point || !a.xyz || !d_ref || !a.run_image || !a.run_begin || !a.centre || !a.mark ||
      !a.count || !a.angle || !d_shared || !d_angle75)
    return fail(MPSFM_ENOMEM, "hipMalloc failed");
  int64_t launches = 0, groups = 0;
  auto launched = [&]() -> int { MPSFM_TRY(hipGetLastError()); ++launches; return 0; };
  if (int rc = A.begin()) return rc;
  hipLaunchKernelGGL(k_lb_centres, sq_blocks(n_images), dim3(kQT), 0, A.st, a);
  if (int rc = launched()) return rc;
  for (int32_t g0 = 0; g0 < n_refs; g0 += group, ++groups) {
    a.n_group = std::min(group, n_refs - g0);
    a.ref = d_ref + g0;
    a.shared = d_shared + (size_t)g0 * n_images;
    a.angle75 = d_angle75 + (size_t)g0 * n_images;
    MPSFM_TRY(hipMemsetAsync(a.mark, 0, sizeof(int32_t) * (size_t)a.n_group * (size_t)n_points, A.st));
    MPSFM_TRY(hipMemsetAsync(a.count, 0, sizeof(unsigned long long) * (size_t)a.n_group * (size_t)n_images, A.st));
    if (longest_ref > 0) {
      hipLaunchKernelGGL(k_lb_marks, dim3(sq_blocks(longest_ref).x, (unsigned)a.n_group), dim3(kQT), 0, A.st, a);
      if (int rc = launched()) return rc;
    }
    hipLaunchKernelGGL(k_lb_angles, dim3((unsigned)run_image.size(), (unsigned)a.n_group), dim3(kQT), 0, A.st, a);
    if (int rc = launched()) return rc;
    hipLaunchKernelGGL(k_lb_select, dim3((unsigned)n_images, (unsigned)a.n_group), dim3(kQT), 0, A.st, a);
    if (int rc = launched()) return rc;
  }
  if (int rc = A.stop()) return rc;
  MPSFM_TRY(hipMemcpyAsync(shared, d_shared, sizeof(int32_t) * (size_t)n_refs * (size_t)n_images, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipMemcpyAsync(angle75, d_angle75, sizeof(double) * (size_t)n_refs * (size_t)n_images, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipStreamSynchronize(A.st));  // the one wait of the call
  float ms = 0.f;
  if (int rc = A.elapsed(&ms)) return rc;
  const double min_tri_angle_rad = min_tri_angle_deg * (M_PI / 180.0);
  std::vector<int32_t> order, none(1);
  for (int32_t r = 0; r < n_refs; ++r)
    bundle_len[r] = local_bundle_walk(n_images, shared + (size_t)r * n_images, angle75 + (size_t)r * n_images, ref_T[r], num_images,
                                      min_tri_angle_rad, row ? bundle + r * row : none.data(), order);
  if (info) {
    info->num_launches = launches;
    info->num_syncs = 1;
    info->num_groups = groups;
    info->ms = ms;
  }
  return 0;
}
