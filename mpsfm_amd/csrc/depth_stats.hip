// Row f3, second half: the per-image prior scale fit of Optimizer.__build_shiftscale_problem (reference
// mpsfm/sfm/mapper/bundle_adjustment.py:187-242) and the robust sigma of update_truncation_multiplier (:295-333,
// fit_robust_gaussian_mad :10-15) for ALL images of a call, with one host wait and O(n_images) results (semantics:
// include/mpsfm_hip.h; the design and the measurements: DESIGN.md section 4y).
//
//   k_ds_values      a thread per observation: the samples and the camera-frame depth exactly as k_depth_blocks forms them
//                    (bilinear_sample.h, contraction off), the filter decisions, the ratio r = max(z / d, 1e-6) and the whitened
//                    log-depth error w; the selection as a bit word per observation; the scene's counts through LDS and one
//                    integer add per workgroup
//   k_ds_fit_select  a workgroup per image segment (obs_img does not decrease, so a segment is a range): the counts, then the two
//                    middle order statistics of the selected r in ONE MSB-first radix descent over order-preserving 64-bit keys,
//                    256-bin histograms in LDS; segments of up to kSelectLds observations keep their keys in LDS
//   k_ds_scene_hist  the whole-scene segment of w (signed) is shared by many workgroups: each histograms its part in LDS and adds
//   k_ds_scene_scan  its non-empty bins to 256 global integer bins per rank (the second set counts once the two ranks have parted);
//                    a one-workgroup launch behind it scans them and narrows the prefixes.  Eight such pairs give mu, eight
//                    more over |w - mu| give the MAD.
// Only integers are added atomically: every output is the same bit pattern whatever the scheduling.  NaNs are counted apart and
// never ranked (np.median answers NaN when it meets one: the host does that from the count).  No logarithm of r is taken here:
// log is monotone, so the host takes it of the two order statistics.
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "bilinear_sample.h"  // grid_coord + bilinear, and contraction off for the rest of this file
#include "call_scope.h"

namespace mpsfm {

namespace {
constexpr int kDT = 256;            // threads of every workgroup here
constexpr int kDW = kDT / 64;       // its waves
constexpr int kSelectLds = 2048;    // keys of a segment that k_ds_fit_select keeps in LDS (16 KB)
constexpr int kSceneBlocksMax = 1024;
constexpr int kScenePerThread = 8;  // observations per thread and pass of k_ds_scene_hist before the grid stops growing
constexpr uint8_t kSelValid = 1, kSelFit = 2, kSelSigma = 4;  // the `selected` word of an observation
// the key of no ranked value: a NaN pattern (NaNs are never ranked)
constexpr uint64_t kNoKey = ~0ull;

// doubles order as these keys: the sign bit flipped for non-negative values, all bits for negative ones (-0 sorts below +0; both
// are the value 0, so an order statistic is the same number either way and the key gives back the element's own sign)
__device__ __forceinline__ uint64_t order_key(double v) {
  uint64_t b;
  memcpy(&b, &v, sizeof(b));
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ __forceinline__ double key_value(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
  double v;
  memcpy(&v, &b, sizeof(v));
  return v;
}

// Two adjacent ranks in one descent: they share the prefix until the byte whose bins separate them, then each follows its own.
struct Sel2 {
  uint64_t prefix[2];
  uint32_t rank[2];   // rank among the elements under the prefix
  uint32_t split;     // 1: the prefixes differ; hist[256 ..] counts under prefix[1]
  uint32_t pad_;
};
__device__ __forceinline__ void sel2_begin(Sel2* s, uint32_t n) {  // ranks (n - 1) / 2 and n / 2 of n elements
  s->prefix[0] = s->prefix[1] = 0;
  s->rank[0] = n ? (n - 1) / 2 : 0;
  s->rank[1] = n / 2;
  s->split = 0;
}
// where an element's key counts in the pass over `byte`: 0 / 1 = under prefix[0] / prefix[1], -1 = nowhere
__device__ __forceinline__ int sel2_side(uint64_t key, uint64_t p0, uint64_t p1, uint32_t split, int byte) {
  if (key == kNoKey) return -1;
  if (byte == 7) return 0;
  const uint64_t head = key & (~0ull << (8 * (byte + 1)));
  return head == p0 ? 0 : (split && head == p1 ? 1 : -1);
}
// One byte of the descent from the histograms hist[2][256] (LDS): all kDT threads call it; *s (LDS) is read and updated.
__device__ void sel2_step(Sel2* s, const uint32_t* hist, int byte, uint32_t* s_wave, uint32_t* s_pick) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint32_t split = s->split, r0 = s->rank[0], r1 = s->rank[1];
  if (t < 4) s_pick[t] = 0;
  __syncthreads();
  const int sides = split ? 2 : 1;
  for (int side = 0; side < sides; ++side) {
    const uint32_t h = hist[side * 256 + t];
    uint32_t incl = h;
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t up = __shfl_up(incl, off, 64);
      if (lane >= off) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t below = incl - h;
    for (int w = 0; w < wave; ++w) below += s_wave[w];
    // the bin with below <= rank < below + h: at most one
    if (side == 0 && below <= r0 && r0 < below + h) { s_pick[0] = (uint32_t)t; s_pick[1] = below; }
    if (side == sides - 1 && below <= r1 && r1 < below + h) { s_pick[2] = (uint32_t)t; s_pick[3] = below; }
    __syncthreads();
  }
  if (t == 0) {
    s->prefix[0] |= (uint64_t)s_pick[0] << (8 * byte);
    s->prefix[1] |= (uint64_t)s_pick[2] << (8 * byte);
    s->rank[0] = r0 - s_pick[1];
    s->rank[1] = r1 - s_pick[3];
    if (s_pick[0] != s_pick[2]) s->split = 1;
  }
  __syncthreads();
}

struct StatArgs {
  int64_t n_obs;
  int32_t n_images, what;
  const int32_t* H; const int32_t* W; const int64_t* map_off;  // per image
  const double* sx; const double* sy; const double* q; const double* t;
  const double* depth; const uint8_t* valid;                  // concatenated maps
  const int32_t* obs_img; const double* obs_xy; const double* obs_var; const int32_t* obs_pt;
  const double* pts;
  const uint8_t* mode; const uint8_t* filter; const double* im_scale; const double* map_scale;  // per image (FIT)
  double factor;
  const int64_t* seg_start;  // [n_images + 1]
  double* ratio; double* whitened; uint8_t* sel;  // [n_obs]
  // per-image results
  int64_t* fit_counts;  // [n_images][3] n_valid, n_sel, n_nan
  double* fit_ratio;    // [n_images][2] lo, hi
  uint32_t* fit_flags;  // [n_images]
};

// the whole-scene select: its state between the launches
struct SceneSel {
  Sel2 s;
  uint32_t n_sel, n_nan;  // SIGMA selection and the NaNs among its w (k_ds_values)
  uint32_t nan2, pad_;    // NaNs among |w - mu|
  double mu, mad;
  uint32_t bins[512];
};

__global__ __launch_bounds__(kDT) void k_ds_values(StatArgs G, SceneSel* S) {
  __shared__ uint32_t s_cnt[2];
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kDT + threadIdx.x;
  if (i < G.n_obs) {
    const int im = G.obs_img[i];
    const int H = G.H[im], W = G.W[im];
    const int64_t off = G.map_off[im];
    const double x = grid_coord(G.obs_xy[2 * i], G.sx[im], W), y = grid_coord(G.obs_xy[2 * i + 1], G.sy[im], H);
    const double v = bilinear(G.valid + off, H, W, x, y);
    const double d = bilinear(G.depth + off, H, W, x, y);
    double R[9];
    quat_to_R(G.q + 4 * im, R);
    const double* X = G.pts + 3 * (size_t)G.obs_pt[i];
    const double z = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + G.t[3 * im + 2];
    const bool base = v == 1.0;
    uint8_t c = 0;
    double r = 0.0, w = 0.0;
    if ((G.what & MPSFM_DEPTH_STATS_FIT) && G.mode[im] == 1) {
      bool keep = base;
      const int filt = G.filter[im];
      if (filt == 1) {  // scale filter (:226-231)
        const double div = d / z;
        keep = keep && div < G.factor && div > 1.0 / G.factor;
      } else if (filt == 2) {  // metric-scale filter (:205-214)
        const double s = z / fmax(d, 1e-6);
        const double p = s * G.im_scale[im];
        const double div = G.map_scale[im] / p;
        keep = keep && div < 1.5 && div > 1.0 / 1.5;
      }
      r = z / d;
      r = r != r ? r : fmax(r, 1e-6);  // NumPy's clip: a NaN stays
      c |= (base ? kSelValid : 0) | (keep ? kSelFit : 0);
    }
    if (G.what & MPSFM_DEPTH_STATS_SIGMA) {
      const double sd = sqrt(G.obs_var[i]);
      w = (log(d) - log(z)) / fmax(sd / d, 1e-6);
      if (base && d > 0.0) {
        c |= kSelSigma;
        atomicAdd(&s_cnt[0], 1u);
        if (w != w) atomicAdd(&s_cnt[1], 1u);
      }
    }
    G.ratio[i] = r;
    G.whitened[i] = w;
    G.sel[i] = c;
  }
  __syncthreads();
  if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(threadIdx.x ? &S->n_nan : &S->n_sel, s_cnt[threadIdx.x]);
}

// grid n_images
__global__ __launch_bounds__(kDT) void k_ds_fit_select(StatArgs G) {
  __shared__ uint64_t s_buf[kSelectLds];
  __shared__ uint32_t s_hist[512];
  __shared__ uint32_t s_wave[kDW];
  __shared__ uint32_t s_pick[4];
  __shared__ uint32_t s_cnt[3];
  __shared__ Sel2 s_sel;
  const int im = (int)blockIdx.x;
  const int64_t i0 = G.seg_start[im];
  const uint32_t n = (uint32_t)(G.seg_start[im + 1] - i0);
  const bool fit = G.mode[im] == 1;  // uniform
  if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const double* ratio = G.ratio + i0;
  const uint8_t* sel = G.sel + i0;
  const bool in_lds = n <= (uint32_t)kSelectLds;
  auto key_of = [&](uint32_t i) -> uint64_t {
    const double r = ratio[i];
    return ((sel[i] & kSelFit) && r == r) ? order_key(r) : kNoKey;
  };
  if (fit) {
    uint32_t c_valid = 0, c_sel = 0, c_nan = 0;
    for (uint32_t i = threadIdx.x; i < n; i += kDT) {
      const uint8_t c = sel[i];
      const double r = ratio[i];
      c_valid += (c & kSelValid) ? 1u : 0u;
      c_sel += (c & kSelFit) ? 1u : 0u;
      c_nan += ((c & kSelFit) && r != r) ? 1u : 0u;
      if (in_lds) s_buf[i] = key_of(i);
    }
    if (c_valid) atomicAdd(&s_cnt[0], c_valid);
    if (c_sel) atomicAdd(&s_cnt[1], c_sel);
    if (c_nan) atomicAdd(&s_cnt[2], c_nan);
  }
  __syncthreads();  // also: s_buf is written
  const uint32_t n_sel = s_cnt[1], m = n_sel - s_cnt[2];  // ranked: selected and not NaN
  if (threadIdx.x == 0) {
    G.fit_counts[3 * im] = s_cnt[0]; G.fit_counts[3 * im + 1] = n_sel; G.fit_counts[3 * im + 2] = s_cnt[2];
    uint32_t f = 0;
    if (fit && n_sel == 0) f |= MPSFM_DEPTH_STATS_EMPTY | (G.filter[im] == 2 ? MPSFM_DEPTH_STATS_EMPTY_METRIC : 0u);
    G.fit_flags[im] = f;
    if (m == 0) { G.fit_ratio[2 * im] = G.fit_ratio[2 * im + 1] = __builtin_nan(""); }
    sel2_begin(&s_sel, m);
  }
  if (m == 0) return;  // uniform
  for (int byte = 7; byte >= 0; --byte) {
    s_hist[threadIdx.x] = 0; s_hist[256 + threadIdx.x] = 0;
    __syncthreads();  // also: s_sel of the step before
    const uint64_t p0 = s_sel.prefix[0], p1 = s_sel.prefix[1];
    const uint32_t split = s_sel.split;
    for (uint32_t i = threadIdx.x; i < n; i += kDT) {
      const uint64_t k = in_lds ? s_buf[i] : key_of(i);
      const int side = sel2_side(k, p0, p1, split, byte);
      if (side >= 0) atomicAdd(&s_hist[side * 256 + ((k >> (8 * byte)) & 255u)], 1u);
    }
    __syncthreads();
    sel2_step(&s_sel, s_hist, byte, s_wave, s_pick);
  }
  if (threadIdx.x == 0) {
    G.fit_ratio[2 * im] = key_value(s_sel.prefix[0]);
    G.fit_ratio[2 * im + 1] = key_value(s_sel.prefix[1]);
  }
}

// the scene value of observation i in phase 0 (w) or 1 (|w - mu|); false: not selected, or a NaN of phase 0
__device__ __forceinline__ bool scene_value(const double* whitened, const uint8_t* sel, int64_t i, int phase, double mu, double* out) {
  if (!(sel[i] & kSelSigma)) return false;
  const double w = whitened[i];
  if (w != w) return false;
  *out = phase ? fabs(w - mu) : w;
  return true;
}

__global__ __launch_bounds__(kDT) void k_ds_scene_hist(const double* whitened, const uint8_t* sel, int64_t n_obs, SceneSel* S, int phase,
                                                        int byte) {
  __shared__ uint32_t s_hist[513];  // [512]: NaNs among |w - mu|
  for (int k = threadIdx.x; k < 513; k += kDT) s_hist[k] = 0;
  __syncthreads();
  // the state was written by the launch before this one: plain loads
  const uint64_t p0 = S->s.prefix[0], p1 = S->s.prefix[1];
  const uint32_t split = S->s.split;
  const double mu = S->mu;
  const int64_t stride = (int64_t)gridDim.x * kDT;
  for (int64_t i = (int64_t)blockIdx.x * kDT + threadIdx.x; i < n_obs; i += stride) {
    double v;
    if (!scene_value(whitened, sel, i, phase, mu, &v)) continue;
    if (v != v) {
      if (byte == 7) atomicAdd(&s_hist[512], 1u);
      continue;
    }
    const uint64_t k = order_key(v);
    const int side = sel2_side(k, p0, p1, split, byte);
    if (side >= 0) atomicAdd(&s_hist[side * 256 + ((k >> (8 * byte)) & 255u)], 1u);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 512; k += kDT)
    if (s_hist[k]) atomicAdd(&S->bins[k], s_hist[k]);
  if (threadIdx.x == 0 && s_hist[512]) atomicAdd(&S->nan2, s_hist[512]);
}

// one workgroup
__global__ __launch_bounds__(kDT) void k_ds_scene_scan(SceneSel* S, int phase, int byte) {
  __shared__ uint32_t s_hist[512];
  __shared__ uint32_t s_wave[kDW];
  __shared__ uint32_t s_pick[4];
  __shared__ Sel2 s_sel;
  for (int k = threadIdx.x; k < 512; k += kDT) {
    s_hist[k] = S->bins[k];
    S->bins[k] = 0;  // for the next pass
  }
  const uint32_t m = S->n_sel - S->n_nan;  // ranked in either phase (a NaN of phase 1 makes the MAD a NaN)
  if (threadIdx.x == 0) {
    if (byte == 7) sel2_begin(&s_sel, m);
    else s_sel = S->s;
  }
  __syncthreads();
  sel2_step(&s_sel, s_hist, byte, s_wave, s_pick);
  if (threadIdx.x == 0) {
    if (byte > 0) {
      S->s = s_sel;
    } else {
      const double lo = key_value(s_sel.prefix[0]), hi = key_value(s_sel.prefix[1]);
      double mid = (lo + hi) * 0.5;  // np.median's mean of the two middle elements
      if (m == 0 || (phase == 1 && S->nan2 > 0)) mid = __builtin_nan("");
      if (phase == 0) S->mu = mid; else S->mad = mid;
      sel2_begin(&S->s, 0);
    }
  }
}

}  // namespace

}  // namespace mpsfm

using namespace mpsfm;

extern "C" int mpsfm_depth_stats(const mpsfm_depth_gather* g, int32_t what, const uint8_t* img_mode, const uint8_t* img_filter,
                                 const double* im_scale, const double* map_scale, int32_t device, int64_t* fit_counts, double* fit_ratio,
                                 uint32_t* fit_flags, int64_t* sigma_counts, double* sigma_stats, double* ratio, double* whitened,
                                 uint8_t* selected) {
  if (!g) return fail(MPSFM_EINVAL, "gather descriptor is NULL");
  if (g->n_images < 0 || g->n_obs < 0 || g->n_pts < 0) return fail(MPSFM_EINVAL, "negative size");
  const bool do_fit = (what & MPSFM_DEPTH_STATS_FIT) != 0, do_sigma = (what & MPSFM_DEPTH_STATS_SIGMA) != 0;
  if ((what & ~(MPSFM_DEPTH_STATS_FIT | MPSFM_DEPTH_STATS_SIGMA)) || what == 0) return fail(MPSFM_EINVAL, "`what` must be FIT, SIGMA or both");
  if (do_fit && g->n_images > 0 && (!img_mode || !img_filter || !im_scale || !map_scale)) return fail(MPSFM_EINVAL, "per-image fit arrays are NULL");
  if (do_fit && g->n_images > 0 && (!fit_counts || !fit_ratio || !fit_flags)) return fail(MPSFM_EINVAL, "output pointer is NULL");
  if (do_sigma && (!sigma_counts || !sigma_stats)) return fail(MPSFM_EINVAL, "output pointer is NULL");
  if (do_fit && !(g->scale_filter_factor > 0.0)) return fail(MPSFM_EINVAL, "scale_filter_factor must be positive");
  const size_t ni = (size_t)g->n_images, no = (size_t)g->n_obs;
  for (size_t i = 0; do_fit && i < ni; ++i)
    if (img_mode[i] > 1 || img_filter[i] > 2) return fail(MPSFM_EINVAL, "image mode must be 0 or 1 and filter 0, 1 or 2");
  if (no == 0) {  // nothing to select from
    for (size_t i = 0; do_fit && i < ni; ++i) {
      fit_counts[3 * i] = fit_counts[3 * i + 1] = fit_counts[3 * i + 2] = 0;
      fit_ratio[2 * i] = fit_ratio[2 * i + 1] = NAN;
      fit_flags[i] = img_mode[i] == 1 ? (MPSFM_DEPTH_STATS_EMPTY | (img_filter[i] == 2 ? MPSFM_DEPTH_STATS_EMPTY_METRIC : 0u)) : 0u;
    }
    if (do_sigma) { sigma_counts[0] = sigma_counts[1] = 0; sigma_stats[0] = sigma_stats[1] = NAN; }
    return 0;
  }
  if (g->n_obs >= (1ll << 31)) return fail(MPSFM_EUNSUPPORTED, "2^31 observations or more");
  if (!g->map_h || !g->map_w || !g->depth_map || !g->valid_map || !g->sx || !g->sy || !g->cam_quat_xyzw || !g->cam_t)
    return fail(MPSFM_EINVAL, "image arrays are NULL");
  if (!g->obs_img || !g->obs_xy || !g->obs_var || !g->obs_pt || !g->pts) return fail(MPSFM_EINVAL, "observation arrays are NULL");
  std::vector<int64_t> off(ni + 1, 0), seg(ni + 1, 0);
  for (size_t i = 0; i < ni; ++i) {
    if (g->map_h[i] < 2 || g->map_w[i] < 2 || !g->depth_map[i] || !g->valid_map[i]) return fail(MPSFM_EINVAL, "map missing or smaller than 2x2");
    off[i + 1] = off[i] + (int64_t)g->map_h[i] * g->map_w[i];
  }
  for (int64_t i = 0; i < g->n_obs; ++i) {
    if (g->obs_img[i] < 0 || g->obs_img[i] >= g->n_images || g->obs_pt[i] < 0 || g->obs_pt[i] >= g->n_pts)
      return fail(MPSFM_EINVAL, "observation index out of range");
    if (i > 0 && g->obs_img[i] < g->obs_img[i - 1]) return fail(MPSFM_EINVAL, "obs_img must not decrease");
    ++seg[(size_t)g->obs_img[i] + 1];
  }
  for (size_t i = 0; i < ni; ++i) seg[i + 1] += seg[i];
  if (int rc = open_device(device)) return rc;
  CallScope B;
  if (int rc = B.open()) return rc;
  const size_t npix = (size_t)off[ni];
  StatArgs A{};
  A.n_obs = g->n_obs; A.n_images = g->n_images; A.what = what; A.factor = g->scale_filter_factor;
  if (int rc = B.up(&A.H, g->map_h, ni)) return rc;
  if (int rc = B.up(&A.W, g->map_w, ni)) return rc;
  if (int rc = B.up(&A.map_off, off.data(), ni)) return rc;
  if (int rc = B.up(&A.seg_start, seg.data(), ni + 1)) return rc;
  if (int rc = B.up(&A.sx, g->sx, ni)) return rc;
  if (int rc = B.up(&A.sy, g->sy, ni)) return rc;
  if (int rc = B.up(&A.q, g->cam_quat_xyzw, 4 * ni)) return rc;
  if (int rc = B.up(&A.t, g->cam_t, 3 * ni)) return rc;
  if (do_fit) {
    if (int rc = B.up(&A.mode, img_mode, ni)) return rc;
    if (int rc = B.up(&A.filter, img_filter, ni)) return rc;
    if (int rc = B.up(&A.im_scale, im_scale, ni)) return rc;
    if (int rc = B.up(&A.map_scale, map_scale, ni)) return rc;
  }
  if (int rc = B.up(&A.obs_img, g->obs_img, no)) return rc;
  if (int rc = B.up(&A.obs_xy, g->obs_xy, 2 * no)) return rc;
  if (int rc = B.up(&A.obs_var, g->obs_var, no)) return rc;
  if (int rc = B.up(&A.obs_pt, g->obs_pt, no)) return rc;
  if (int rc = B.up(&A.pts, g->pts, 3 * (size_t)g->n_pts)) return rc;
  double* d_depth = B.alloc<double>(npix);
  uint8_t* d_valid = B.alloc<uint8_t>(npix);
  if (!d_depth || !d_valid) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  for (size_t i = 0; i < ni; ++i) {
    const size_t n = (size_t)(off[i + 1] - off[i]);
    if (int rc = staged_upload(d_depth + off[i], g->depth_map[i], sizeof(double) * n)) return rc;
    if (int rc = staged_upload(d_valid + off[i], g->valid_map[i], n)) return rc;
  }
  A.depth = d_depth; A.valid = d_valid;
  A.ratio = B.alloc<double>(no); A.whitened = B.alloc<double>(no); A.sel = B.alloc<uint8_t>(no);
  A.fit_counts = B.alloc<int64_t>(3 * ni); A.fit_ratio = B.alloc<double>(2 * ni); A.fit_flags = B.alloc<uint32_t>(ni);
  SceneSel* S = B.alloc<SceneSel>(1);
  if (!A.ratio || !A.whitened || !A.sel || !A.fit_counts || !A.fit_ratio || !A.fit_flags || !S) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  if (int rc = staged_drain()) return rc;
  MPSFM_TRY(hipMemsetAsync(S, 0, sizeof(SceneSel), B.st));
  hipLaunchKernelGGL(k_ds_values, dim3((unsigned)((no + kDT - 1) / kDT)), dim3(kDT), 0, B.st, A, S);
  MPSFM_TRY(hipGetLastError());
  if (do_fit) {
    hipLaunchKernelGGL(k_ds_fit_select, dim3((unsigned)ni), dim3(kDT), 0, B.st, A);
    MPSFM_TRY(hipGetLastError());
  }
  if (do_sigma) {
    const size_t per = (size_t)kDT * kScenePerThread;
    const unsigned blocks = (unsigned)std::min<size_t>((no + per - 1) / per, (size_t)kSceneBlocksMax);
    for (int phase = 0; phase < 2; ++phase)
      for (int byte = 7; byte >= 0; --byte) {
        hipLaunchKernelGGL(k_ds_scene_hist, dim3(blocks), dim3(kDT), 0, B.st, A.whitened, A.sel, g->n_obs, S, phase, byte);
        hipLaunchKernelGGL(k_ds_scene_scan, dim3(1), dim3(kDT), 0, B.st, S, phase, byte);
      }
    MPSFM_TRY(hipGetLastError());
  }
  // results: everything is queued, then the call's one wait
  SceneSel* hS = B.host<SceneSel>(1);
  if (!hS) return fail(MPSFM_ENOMEM, "hipHostMalloc failed");
  if (do_fit) {
    MPSFM_TRY(hipMemcpyAsync(fit_counts, A.fit_counts, sizeof(int64_t) * 3 * ni, hipMemcpyDeviceToHost, B.st));
    MPSFM_TRY(hipMemcpyAsync(fit_ratio, A.fit_ratio, sizeof(double) * 2 * ni, hipMemcpyDeviceToHost, B.st));
    MPSFM_TRY(hipMemcpyAsync(fit_flags, A.fit_flags, sizeof(uint32_t) * ni, hipMemcpyDeviceToHost, B.st));
  }
  if (do_sigma) MPSFM_TRY(hipMemcpyAsync(hS, S, sizeof(SceneSel), hipMemcpyDeviceToHost, B.st));
  if (ratio) MPSFM_TRY(hipMemcpyAsync(ratio, A.ratio, sizeof(double) * no, hipMemcpyDeviceToHost, B.st));
  if (whitened) MPSFM_TRY(hipMemcpyAsync(whitened, A.whitened, sizeof(double) * no, hipMemcpyDeviceToHost, B.st));
  if (selected) MPSFM_TRY(hipMemcpyAsync(selected, A.sel, no, hipMemcpyDeviceToHost, B.st));
  MPSFM_TRY(hipStreamSynchronize(B.st));
  if (do_sigma) {
    sigma_counts[0] = hS->n_sel; sigma_counts[1] = hS->n_nan;
    sigma_stats[0] = hS->mu; sigma_stats[1] = hS->mad;
  }
  return 0;
}
