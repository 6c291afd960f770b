// Monocular depth and normal priors of all images of a scene (reference mpsfm/sfm/scene/image/depth.py:34-130 Depth._init,
// image/utils.py:6-36 get_continuity_mask, image/normals.py:12-246 Normals._init), one call per kind.  The image is the
// grid's y index; no launch is per image.
//   depth    k_dp_source   one thread per SOURCE pixel: mean / variance lists of the four flip_consistency x
//                          prior_uncertainty branches, inverse-variance fusion, the uncertainty branch table, clip,
//                          validity and the continuity test (in the map's own precision)
//            k_dp_target   one thread per TARGET pixel: copy or resize of the four source-size maps, external mask
//                          (nearest), the 1e6 / 0.1 / depth_lim fills
//            k_dp_kps      one thread per keypoint: the finished uncertainty sampled with bilinear_sample.h
//   normals  k_np_full     one thread per full-size pixel: resize + normalise of both normal maps, resized variances (kept
//                          for the dependent half-size pass), mean normal and 3x3 covariance, mask fills
//            k_np_half     one thread per half-size pixel: the same from the NORMALISED full-size maps
// fp64; every product and sum rounded on its own (resize_taps.h / bilinear_sample.h switch contraction off), IEEE
// division and square root (no fast-math), NaN-propagating maximum like NumPy's.
#include <string>
#include <vector>

#include "call_scope.h"
#include "common.h"
#include "resize_taps.h"

namespace mpsfm {

namespace {
constexpr int kT = 256;
constexpr double kLarge = 1e6;
constexpr double kTwoPi = 2.0 * 3.141592653589793;
constexpr double kPi = 3.141592653589793;

__device__ __forceinline__ double np_maximum(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }
__device__ __forceinline__ double np_minimum(double a, double b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }

// a value map of either precision in the call's byte pool
__device__ __forceinline__ double load_val(const uint8_t* pool, int64_t off, int f32, int64_t i) {
  return f32 ? (double)((const float*)(pool + off))[i] : ((const double*)(pool + off))[i];
}

// ---------------------------------------------------------------------------------------------------- depth
struct DpImage {
  int32_t H, W, Ht, Wt, Hm, Wm, f32, nk;
  int64_t val_off[4];             // depth, depth2, depth_variance, depth_variance2: bytes into the pool, -1 absent
  int64_t valid_off, valid2_off;  // bytes into the pool, -1 absent
  int64_t mask_off;               // bytes into the pool, -1 absent
  int64_t kps_off;                // bytes into the pool (doubles)
  int64_t src_off, dst_off, upd_off;  // elements into the source-size, target-size and keypoint arrays
  double sx, sy;
};

struct DpConf {
  double noise2, std2, psm2, max_std2, depth_lim, fixed_unc, depth_unc;
  int32_t has_max_std, has_depth_lim, has_depth_unc, use_continuity, fixed_uncertainty, prior_uncertainty, flip;
};

// get_continuity_mask for one pixel of one map, in the map's own precision T
template <typename T>
__device__ __forceinline__ bool continuous_at(const T* m, int H, int W, int y, int x) {
  const T eps = (T)1e-6, thr = (T)1.015, one = (T)1;
  auto inv = [&](int yy, int xx) {
    const T v = m[(size_t)yy * W + xx];
    return one / (v < eps ? eps : v);  // clip(min=eps) keeps NaN
  };
  const T c = inv(y, x);
  bool ok = true;
  auto pair = [&](T o) { ok = ok && !(c / o > thr) && !(o / c > thr); };  // NaN ratios compare false
  if (x > 0) pair(inv(y, x - 1));
  if (x + 1 < W) pair(inv(y, x + 1));
  if (y > 0) pair(inv(y - 1, x));
  if (y + 1 < H) pair(inv(y + 1, x));
  return ok;
}

__global__ __launch_bounds__(kT) void k_dp_source(const DpImage* __restrict__ imgs, const uint8_t* __restrict__ pool, DpConf cf,
                                                   double* __restrict__ prior_s, double* __restrict__ unc_s,
                                                   uint8_t* __restrict__ valid_s, uint8_t* __restrict__ cont_s) {
  const DpImage& I = imgs[blockIdx.y];
  const int32_t n = I.H * I.W;
  const int32_t i = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  if (i >= n) return;
  const double d = load_val(pool, I.val_off[0], I.f32, i);
  double mew[2], var[2];
  int nm = 1, nv = 0;
  if (cf.flip && !cf.prior_uncertainty) {  // loop consistency alone
    const double d2 = load_val(pool, I.val_off[1], I.f32, i);
    mew[0] = (d2 + d) / 2.0;
    const double e = d - d2;
    var[0] = e * e;
    nv = 1;
  } else if (cf.flip) {  // loop consistency and predicted variances
    mew[0] = d;
    mew[1] = load_val(pool, I.val_off[1], I.f32, i);
    var[0] = load_val(pool, I.val_off[2], I.f32, i);
    var[1] = load_val(pool, I.val_off[3], I.f32, i);
    nm = nv = 2;
  } else if (cf.prior_uncertainty) {
    mew[0] = d;
    var[0] = load_val(pool, I.val_off[2], I.f32, i);
    nv = 1;
  } else {
    mew[0] = d;
  }
  // inverse-variance sums in the order of Python's sum(): (0 + a) + b
  double prior = mew[0];
  if (nm > 1) {
    const double num = mew[0] / (var[0] + 1e-6) + mew[1] / (var[1] + 1e-6);
    const double den = 1.0 / (var[0] + 1e-6) + 1.0 / (var[1] + 1e-6);
    prior = num / (den + 1e-6);
  }
  double unc;
  if (cf.has_depth_unc) {
    if (cf.prior_uncertainty) {
      double nvv[2];
      for (int k = 0; k < nv; ++k) {  // zip(mews, variances): nv <= nm here
        const double s = mew[k] * cf.depth_unc;
        nvv[k] = np_maximum(var[k] * cf.psm2, s * s);
      }
      unc = nv > 1 ? 1.0 / ((1.0 / (nvv[0] + 1e-6) + 1.0 / (nvv[1] + 1e-6)) + 1e-6) : nvv[0];
    } else {
      const double s = prior * cf.depth_unc;
      unc = s * s;
    }
  } else if (cf.flip) {
    double den = 1.0 / (var[0] + 1e-6);
    if (nv > 1) den = den + 1.0 / (var[1] + 1e-6);
    unc = (1.0 / (den + 1e-6)) * cf.psm2;
  } else if (cf.fixed_uncertainty) {
    unc = cf.fixed_unc;  // ones * fixed_uncertainty_val * std_multiplier^2, folded on the host
  } else {
    unc = var[0];  // the host refuses this branch without a variance
  }
  unc = np_maximum(unc, cf.noise2);
  if (cf.has_max_std) unc = np_minimum(unc, cf.max_std2);
  unc = unc * cf.std2;

  bool valid = d > 0.0;
  if (I.valid_off >= 0) valid = valid && pool[I.valid_off + i] != 0;
  if (I.valid2_off >= 0) valid = valid && pool[I.valid2_off + i] != 0;
  bool cont = true;
  if (cf.use_continuity) {
    const int y = i / I.W, x = i % I.W;
    for (int k = 0; k < 2; ++k) {
      if (I.val_off[k] < 0) continue;
      cont = cont && (I.f32 ? continuous_at((const float*)(pool + I.val_off[k]), I.H, I.W, y, x)
                            : continuous_at((const double*)(pool + I.val_off[k]), I.H, I.W, y, x));
    }
  }
  const int64_t o = I.src_off + i;
  prior_s[o] = prior;
  unc_s[o] = unc;
  valid_s[o] = valid ? 1 : 0;
  cont_s[o] = cont ? 1 : 0;
}

__global__ __launch_bounds__(kT) void k_dp_target(const DpImage* __restrict__ imgs, const uint8_t* __restrict__ pool, DpConf cf,
                                                   const double* __restrict__ prior_s, const double* __restrict__ unc_s,
                                                   const uint8_t* __restrict__ valid_s, const uint8_t* __restrict__ cont_s,
                                                   double* __restrict__ prior_o, double* __restrict__ unc_o,
                                                   uint8_t* __restrict__ valid_o, uint8_t* __restrict__ cont_o) {
  const DpImage& I = imgs[blockIdx.y];
  const int32_t n = I.Ht * I.Wt;
  const int32_t i = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  if (i >= n) return;
  const int y = i / I.Wt, x = i % I.Wt;
  double prior, unc;
  bool valid, cont;
  if (I.H == I.Ht && I.W == I.Wt) {
    const int64_t s = I.src_off + i;
    prior = prior_s[s];
    unc = unc_s[s];
    valid = valid_s[s] != 0;
    cont = cont_s[s] != 0;
  } else {
    const Tap ty = linear_tap(I.H, I.Ht, y), tx = linear_tap(I.W, I.Wt, x);
    const int64_t s = I.src_off;
    const int W = I.W;
    prior = resize_sample(ty, tx, [&](int yy, int xx) { return prior_s[s + (int64_t)yy * W + xx]; });
    unc = resize_sample(ty, tx, [&](int yy, int xx) { return unc_s[s + (int64_t)yy * W + xx]; });
    valid = resize_mask_all(ty, tx, [&](int yy, int xx) { return valid_s[s + (int64_t)yy * W + xx] != 0; });
    cont = resize_mask_all(ty, tx, [&](int yy, int xx) { return cont_s[s + (int64_t)yy * W + xx] != 0; });
  }
  if (I.mask_off >= 0) {
    const int my = (I.Hm == I.Ht && I.Wm == I.Wt) ? y : nearest_tap(I.Hm, I.Ht, y);
    const int mx = (I.Hm == I.Ht && I.Wm == I.Wt) ? x : nearest_tap(I.Wm, I.Wt, x);
    valid = valid && pool[I.mask_off + (int64_t)my * I.Wm + mx] != 0;
  }
  if (!valid) unc = kLarge;
  if (prior == 0.0) {
    prior = 0.1;
    valid = false;
  }
  if (cf.has_depth_lim && prior > cf.depth_lim) valid = false;
  const int64_t o = I.dst_off + i;
  prior_o[o] = prior;
  unc_o[o] = unc;
  valid_o[o] = valid ? 1 : 0;
  cont_o[o] = cont ? 1 : 0;
}

__global__ __launch_bounds__(kT) void k_dp_kps(const DpImage* __restrict__ imgs, const uint8_t* __restrict__ pool,
                                                const double* __restrict__ unc_o, double* __restrict__ upd) {
  const DpImage& I = imgs[blockIdx.y];
  const int32_t i = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  if (i >= I.nk) return;
  const double* kp = (const double*)(pool + I.kps_off) + 2 * (int64_t)i;
  const double x = grid_coord(kp[0], I.sx, I.Wt), y = grid_coord(kp[1], I.sy, I.Ht);
  upd[I.upd_off + i] = bilinear(unc_o + I.dst_off, I.Ht, I.Wt, x, y);
}

// ---------------------------------------------------------------------------------------------------- normals
struct NpImage {
  int32_t H, W, Ht, Wt, Hd, Wd, Hm, Wm, f32, pad;
  int64_t val_off[4];  // normals, normals2, normals_variance, normals2_variance: bytes into the pool, -1 absent
  int64_t mask_off, cont_off;  // bytes into the pool, -1 absent
  int64_t full_off, half_off;  // pixels into the full-size and half-size arrays
};

struct NpConf {
  double noise, std2, lc2, psm2;
  int32_t flip;
};

struct V3 { double x, y, z; };

__device__ __forceinline__ V3 unit(V3 n) {  // n / np.linalg.norm(n): a zero vector gives NaN
  const double l = sqrt(n.x * n.x + n.y * n.y + n.z * n.z);
  return V3{n.x / l, n.y / l, n.z / l};
}

// Jacobian(sphere) of normals.py:82-94, row-major 3x2 (J[2][1] = 0)
__device__ __forceinline__ void sphere_jacobian(double theta, double phi, double J[6]) {
  const double ct = cos(theta), cp = cos(phi), st = sin(theta), sp = sin(phi);
  J[0] = ct * cp; J[1] = -st * sp;
  J[2] = ct * sp; J[3] = st * cp;
  J[4] = -st;     J[5] = 0.0;
}

// U = (J C) J^T with C = [[a, b], [b, c]], in matmul's association
__device__ __forceinline__ void jcjt(const double J[6], double a, double b, double c, double U[9]) {
  double M[6];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    M[2 * r] = J[2 * r] * a + J[2 * r + 1] * b;
    M[2 * r + 1] = J[2 * r] * b + J[2 * r + 1] * c;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) U[3 * r + k] = M[2 * r] * J[2 * k] + M[2 * r + 1] * J[2 * k + 1];
}

// cart_to_spherical (normals.py:17-30)
__device__ __forceinline__ void cart_to_spherical(V3 n, double s[2]) {
  n = unit(n);
  s[0] = acos(n.z);
  const double sg = n.y > 0.0 ? 1.0 : (n.y < 0.0 ? -1.0 : n.y);  // np.sign: 0 -> 0, NaN -> NaN
  s[1] = sg * acos(n.x / (1e-6 + sqrt(n.x * n.x + n.y * n.y)));
}

__device__ __forceinline__ double diff_angle(double a, double b) {
  const double d = fabs(a - b);
  return np_minimum(d, kTwoPi - d);
}

// mean normal and Cartesian covariance of one pixel, before std_multiplier^2 and the mask fills:
//   without flip  J(data) diag(v, v) J(data)^T with v rounded to float32 and the Cartesian x, y read as angles (:220-230)
//   with flip     two_view_covariance through covar_sphere_thorough_spherical_mean (:97-134)
__device__ __forceinline__ void normal_cov(const NpConf& cf, V3 n1, V3 n2, double v1, double v2, V3& data, double U[9]) {
  double J[6];
  if (!cf.flip) {
    data = n1;
    const double v = (double)(float)v1;
    sphere_jacobian(n1.x, n1.y, J);
    jcjt(J, v, 0.0, v, U);
    return;
  }
  data = unit(V3{(n2.x + n1.x) / 2.0, (n2.y + n1.y) / 2.0, (n2.z + n1.z) / 2.0});
  double s1[2], s2[2], mean[2];
  cart_to_spherical(n1, s1);
  cart_to_spherical(n2, s2);
#pragma unroll
  for (int k = 0; k < 2; ++k) {  // the representative of s2 closest to s1
    const double diff = s2[k] - s1[k];
    if (diff > kPi) s2[k] = s2[k] - kTwoPi;
    if (diff < -kPi) s2[k] = s2[k] + kTwoPi;
    mean[k] = (s1[k] + s2[k]) / 2.0;
  }
  const double a1 = diff_angle(s1[0], mean[0]), b1 = diff_angle(s1[1], mean[1]);
  const double a2 = diff_angle(s2[0], mean[0]), b2 = diff_angle(s2[1], mean[1]);
  double a = np_maximum(a1 * a1 + a2 * a2, 0.0);  // .clip(0)
  double c = np_maximum(b1 * b1 + b2 * b2, 0.0);
  double b = a1 * b1 + a2 * b2;
  // R max(Lambda, noise) R^T by the closed-form symmetric 2x2 eigen-decomposition: rotation angle t with
  // tan 2t = 2b / (a - c), eigenvalues (a + c) / 2 +- hypot((a - c) / 2, b); the noise is compared unsquared
  {
    const double hm = (a + c) / 2.0, hd = (a - c) / 2.0;
    const double r = sqrt(hd * hd + b * b);
    const double l1 = np_maximum(hm + r, cf.noise), l2 = np_maximum(hm - r, cf.noise);
    const double t = 0.5 * atan2(2.0 * b, a - c);
    const double ce = cos(t), se = sin(t);
    a = l1 * ce * ce + l2 * se * se;
    c = l1 * se * se + l2 * ce * ce;
    b = (l1 - l2) * ce * se;
  }
  a = a * cf.lc2; b = b * cf.lc2; c = c * cf.lc2;
  const double w1 = v1 * cf.psm2, w2 = v2 * cf.psm2;
  a = np_maximum(np_maximum(a, w1), w2);
  c = np_maximum(np_maximum(c, w1), w2);
  sphere_jacobian(mean[0], mean[1], J);
  jcjt(J, a, b, c, U);
  U[0] = np_maximum(U[0], 0.0);
  U[4] = np_maximum(U[4], 0.0);
  U[8] = np_maximum(U[8], 0.0);
}

// the three channels of an interleaved [h][w][3] map resized to one destination pixel
template <typename F>
__device__ __forceinline__ V3 resize_v3(const Tap& ty, const Tap& tx, F at) {
  return V3{resize_sample(ty, tx, [&](int y, int x) { return at(y, x, 0); }),
            resize_sample(ty, tx, [&](int y, int x) { return at(y, x, 1); }),
            resize_sample(ty, tx, [&](int y, int x) { return at(y, x, 2); })};
}

__global__ __launch_bounds__(kT) void k_np_full(const NpImage* __restrict__ imgs, const uint8_t* __restrict__ pool, NpConf cf,
                                                 double* __restrict__ n1f, double* __restrict__ n2f, double* __restrict__ v1f,
                                                 double* __restrict__ v2f, double* __restrict__ data_o, double* __restrict__ unc_o) {
  const NpImage& I = imgs[blockIdx.y];
  const int32_t n = I.Ht * I.Wt;
  const int32_t i = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  if (i >= n) return;
  const int y = i / I.Wt, x = i % I.Wt;
  const bool same = I.H == I.Ht && I.W == I.Wt;
  Tap ty, tx;
  if (same) {
    ty = Tap{y, y, 0.0};
    tx = Tap{x, x, 0.0};
  } else {
    ty = linear_tap(I.H, I.Ht, y);
    tx = linear_tap(I.W, I.Wt, x);
  }
  const int W = I.W, f32 = I.f32;
  auto vec = [&](int64_t off) {
    return unit(resize_v3(ty, tx, [&](int yy, int xx, int ch) { return load_val(pool, off, f32, ((int64_t)yy * W + xx) * 3 + ch); }));
  };
  auto scal = [&](int64_t off) {
    return resize_sample(ty, tx, [&](int yy, int xx) { return load_val(pool, off, f32, (int64_t)yy * W + xx); });
  };
  const int64_t o = I.full_off + i;
  const V3 n1 = vec(I.val_off[0]);
  const double v1 = scal(I.val_off[2]);
  V3 n2 = n1;
  double v2 = v1;
  n1f[3 * o] = n1.x; n1f[3 * o + 1] = n1.y; n1f[3 * o + 2] = n1.z;
  v1f[o] = v1;
  if (cf.flip) {
    n2 = vec(I.val_off[1]);
    v2 = scal(I.val_off[3]);
    n2f[3 * o] = n2.x; n2f[3 * o + 1] = n2.y; n2f[3 * o + 2] = n2.z;
    v2f[o] = v2;
  }
  V3 data;
  double U[9];
  normal_cov(cf, n1, n2, v1, v2, data, U);
  bool keep = true;
  if (I.mask_off >= 0) {
    const bool eq = I.Hm == I.Ht && I.Wm == I.Wt;
    const int my = eq ? y : nearest_tap(I.Hm, I.Ht, y), mx = eq ? x : nearest_tap(I.Wm, I.Wt, x);
    keep = pool[I.mask_off + (int64_t)my * I.Wm + mx] != 0;
  }
  if (I.cont_off >= 0) keep = keep && pool[I.cont_off + i] != 0;
  data_o[3 * o] = data.x; data_o[3 * o + 1] = data.y; data_o[3 * o + 2] = data.z;
#pragma unroll
  for (int k = 0; k < 9; ++k) unc_o[9 * o + k] = keep ? U[k] * cf.std2 : kLarge;
}

__global__ __launch_bounds__(kT) void k_np_half(const NpImage* __restrict__ imgs, NpConf cf, const double* __restrict__ n1f,
                                                 const double* __restrict__ n2f, const double* __restrict__ v1f,
                                                 const double* __restrict__ v2f, double* __restrict__ data_o,
                                                 double* __restrict__ unc_o) {
  const NpImage& I = imgs[blockIdx.y];
  const int32_t n = I.Hd * I.Wd;
  const int32_t i = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  if (i >= n) return;
  const int y = i / I.Wd, x = i % I.Wd;
  const bool same = I.Hd == I.Ht && I.Wd == I.Wt;
  Tap ty, tx;
  if (same) {
    ty = Tap{y, y, 0.0};
    tx = Tap{x, x, 0.0};
  } else {
    ty = linear_tap(I.Ht, I.Hd, y);
    tx = linear_tap(I.Wt, I.Wd, x);
  }
  const int W = I.Wt;
  const int64_t base = I.full_off;
  auto vec = [&](const double* m) {
    return unit(resize_v3(ty, tx, [&](int yy, int xx, int ch) { return m[(base + (int64_t)yy * W + xx) * 3 + ch]; }));
  };
  auto scal = [&](const double* m) { return resize_sample(ty, tx, [&](int yy, int xx) { return m[base + (int64_t)yy * W + xx]; }); };
  const V3 d1 = vec(n1f);
  const double dv1 = scal(v1f);
  V3 d2 = d1;
  double dv2 = dv1;
  if (cf.flip) {
    d2 = vec(n2f);
    dv2 = scal(v2f);
  }
  V3 data;
  double U[9];
  normal_cov(cf, d1, d2, dv1, dv2, data, U);
  const int64_t o = I.half_off + i;
  data_o[3 * o] = data.x; data_o[3 * o + 1] = data.y; data_o[3 * o + 2] = data.z;
#pragma unroll
  for (int k = 0; k < 9; ++k) unc_o[9 * o + k] = U[k] * cf.std2;
}

// ---------------------------------------------------------------------------------------------------- host
constexpr int64_t kMaxPixels = (int64_t)1 << 27;  // per map: 32-bit pixel indices with room for the factor 9

// the inputs of a call, gathered into one device block: (host pointer, bytes) -> byte offset, 8-byte aligned
struct Pool {
  struct Part { const void* src; size_t bytes; int64_t off; };
  std::vector<Part> parts;
  int64_t size = 0;
  int64_t add(const void* src, size_t bytes) {
    if (!src) return -1;
    const int64_t off = size;
    parts.push_back(Part{src, bytes, off});
    size += (int64_t)((bytes + 7) & ~(size_t)7);
    return off;
  }
  int upload(uint8_t* dev) const {
    for (const Part& p : parts)
      if (p.bytes)
        if (int rc = staged_upload(dev + p.off, p.src, p.bytes)) return rc;
    return 0;
  }
};

// Python's `a // b` on floats (CPython float_floor_div): not floor(a / b), e.g. 77 // 1.1 is 69 while floor(77 / 1.1) is 70
double py_floordiv(double a, double b) {
  double mod = std::fmod(a, b);
  double div = (a - mod) / b;
  if (mod != 0.0 && ((b < 0.0) != (mod < 0.0))) div -= 1.0;
  if (div == 0.0) return std::copysign(0.0, a / b);
  double fl = std::floor(div);
  if (div - fl > 0.5) fl += 1.0;
  return fl;
}

unsigned blocks_for(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + kT - 1) / kT); }

}  // namespace

}  // namespace mpsfm

using namespace mpsfm;

extern "C" int mpsfm_depth_priors(int32_t n_images, const mpsfm_depth_prior_problem* problems, const mpsfm_depth_prior_conf* conf,
                                  int32_t device, const mpsfm_depth_prior_output* outputs, mpsfm_prior_summary* summary) {
  if (n_images == 0) return 0;  // touches nothing
  if (summary) *summary = mpsfm_prior_summary{};
  if (n_images < 0) return fail(MPSFM_EINVAL, "negative size");
  if (!problems || !conf || !outputs) return fail(MPSFM_EINVAL, "NULL pointer");
  if (n_images > 65535) return fail(MPSFM_EINVAL, "more than 65535 images (images are the grid's y dimension)");
  const bool flip = conf->flip_consistency != 0, pu = conf->prior_uncertainty != 0;
  if (!conf->has_depth_uncertainty && !flip && !conf->fixed_uncertainty && !pu)
    return fail(MPSFM_EINVAL, "no source of uncertainty: depth_uncertainty is None without flip_consistency, fixed_uncertainty or prior_uncertainty");

  Pool pool;
  std::vector<DpImage> imgs((size_t)n_images);
  int64_t src = 0, dst = 0, nk = 0, max_src = 0, max_dst = 0, max_k = 0;
  for (int32_t k = 0; k < n_images; ++k) {
    const mpsfm_depth_prior_problem& P = problems[k];
    const mpsfm_depth_prior_output& O = outputs[k];
    if (P.height <= 0 || P.width <= 0 || P.int_height <= 0 || P.int_width <= 0) return fail(MPSFM_EINVAL, "non-positive map size");
    if ((int64_t)P.height * P.width > kMaxPixels || (int64_t)P.int_height * P.int_width > kMaxPixels)
      return fail(MPSFM_EINVAL, "map larger than 2^27 pixels");
    if (!P.depth) return fail(MPSFM_EINVAL, "depth map is NULL");
    if (flip && !P.depth2) return fail(MPSFM_EINVAL, "flip_consistency needs depth2");
    if (pu && !P.depth_variance) return fail(MPSFM_EINVAL, "prior_uncertainty needs depth_variance");
    if (flip && pu && !P.depth_variance2) return fail(MPSFM_EINVAL, "flip_consistency with prior_uncertainty needs depth_variance2");
    if (P.mask && (P.mask_height <= 0 || P.mask_width <= 0 || (int64_t)P.mask_height * P.mask_width > kMaxPixels))
      return fail(MPSFM_EINVAL, "mask size out of range");
    if (P.n_kps < 0 || (P.n_kps > 0 && !P.kps)) return fail(MPSFM_EINVAL, "keypoints are NULL or their count is negative");
    if (!O.data_prior || !O.uncertainty || !O.valid || !O.continuity_mask || (P.n_kps > 0 && !O.uncertainty_update))
      return fail(MPSFM_EINVAL, "NULL output pointer");
    DpImage& I = imgs[(size_t)k];
    I.H = P.height; I.W = P.width; I.Ht = P.int_height; I.Wt = P.int_width;
    I.Hm = P.mask ? P.mask_height : 0; I.Wm = P.mask ? P.mask_width : 0;
    I.f32 = P.is_float32 != 0; I.nk = P.n_kps;
    const size_t ns = (size_t)P.height * P.width, vb = ns * (I.f32 ? 4 : 8);
    const void* vals[4] = {P.depth, P.depth2, P.depth_variance, P.depth_variance2};
    for (int j = 0; j < 4; ++j) I.val_off[j] = pool.add(vals[j], vb);
    I.valid_off = pool.add(P.valid, ns);
    I.valid2_off = pool.add(P.valid2, ns);
    I.mask_off = pool.add(P.mask, (size_t)I.Hm * I.Wm);
    I.kps_off = P.n_kps ? pool.add(P.kps, sizeof(double) * 2 * (size_t)P.n_kps) : 0;
    I.src_off = src; I.dst_off = dst; I.upd_off = nk;
    I.sx = P.sx; I.sy = P.sy;
    const int64_t nd = (int64_t)I.Ht * I.Wt;
    src += (int64_t)ns; dst += nd; nk += P.n_kps;
    max_src = std::max(max_src, (int64_t)ns); max_dst = std::max(max_dst, nd); max_k = std::max(max_k, (int64_t)P.n_kps);
  }
  if (int rc = open_device(device)) return rc;

  DpConf cf{};
  cf.noise2 = conf->inherent_noise * conf->inherent_noise;
  cf.std2 = conf->std_multiplier * conf->std_multiplier;
  cf.psm2 = conf->prior_std_multiplier * conf->prior_std_multiplier;
  cf.max_std2 = conf->max_std * conf->max_std;
  cf.depth_lim = conf->depth_lim;
  cf.fixed_unc = 1.0 * conf->fixed_uncertainty_val * cf.std2;
  cf.depth_unc = conf->depth_uncertainty;
  cf.has_max_std = conf->has_max_std; cf.has_depth_lim = conf->has_depth_lim; cf.has_depth_unc = conf->has_depth_uncertainty;
  cf.use_continuity = conf->use_continuity; cf.fixed_uncertainty = conf->fixed_uncertainty;
  cf.prior_uncertainty = pu; cf.flip = flip;

  CallScope B;
  if (int rc = B.open(true)) return rc;
  uint8_t* d_pool = B.alloc<uint8_t>((size_t)pool.size);
  DpImage* d_imgs = B.alloc<DpImage>(imgs.size());
  double* d_prior_s = B.alloc<double>((size_t)src);
  double* d_unc_s = B.alloc<double>((size_t)src);
  uint8_t* d_valid_s = B.alloc<uint8_t>((size_t)src);
  uint8_t* d_cont_s = B.alloc<uint8_t>((size_t)src);
  // the outputs in one block: [prior | uncertainty | update | valid | continuity]
  const size_t out_bytes = sizeof(double) * (2 * (size_t)dst + (size_t)nk) + 2 * (size_t)dst;
  uint8_t* d_out = B.alloc<uint8_t>(out_bytes);
  if (!d_pool || !d_imgs || !d_prior_s || !d_unc_s || !d_valid_s || !d_cont_s || !d_out) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  double* d_prior = (double*)d_out;
  double* d_unc = d_prior + dst;
  double* d_upd = d_unc + dst;
  uint8_t* d_valid = (uint8_t*)(d_upd + nk);
  uint8_t* d_cont = d_valid + dst;
  if (int rc = pool.upload(d_pool)) return rc;
  if (int rc = staged_upload(d_imgs, imgs.data(), sizeof(DpImage) * imgs.size())) return rc;
  if (int rc = staged_drain()) return rc;

  if (int rc = B.begin()) return rc;
  hipLaunchKernelGGL(k_dp_source, dim3(blocks_for(max_src), (unsigned)n_images), dim3(kT), 0, B.st, d_imgs, d_pool, cf, d_prior_s,
                     d_unc_s, d_valid_s, d_cont_s);
  MPSFM_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_dp_target, dim3(blocks_for(max_dst), (unsigned)n_images), dim3(kT), 0, B.st, d_imgs, d_pool, cf, d_prior_s,
                     d_unc_s, d_valid_s, d_cont_s, d_prior, d_unc, d_valid, d_cont);
  MPSFM_TRY(hipGetLastError());
  if (max_k > 0) {
    hipLaunchKernelGGL(k_dp_kps, dim3(blocks_for(max_k), (unsigned)n_images), dim3(kT), 0, B.st, d_imgs, d_pool, d_unc, d_upd);
    MPSFM_TRY(hipGetLastError());
  }
  if (int rc = B.stop()) return rc;
  // straight into the caller's arrays: a host copy of the whole block would cost more than the kernels
  for (int32_t k = 0; k < n_images; ++k) {
    const DpImage& I = imgs[(size_t)k];
    const mpsfm_depth_prior_output& O = outputs[k];
    const size_t nd = (size_t)I.Ht * I.Wt;
    MPSFM_TRY(hipMemcpyAsync(O.data_prior, d_prior + I.dst_off, sizeof(double) * nd, hipMemcpyDeviceToHost, B.st));
    MPSFM_TRY(hipMemcpyAsync(O.uncertainty, d_unc + I.dst_off, sizeof(double) * nd, hipMemcpyDeviceToHost, B.st));
    MPSFM_TRY(hipMemcpyAsync(O.valid, d_valid + I.dst_off, nd, hipMemcpyDeviceToHost, B.st));
    MPSFM_TRY(hipMemcpyAsync(O.continuity_mask, d_cont + I.dst_off, nd, hipMemcpyDeviceToHost, B.st));
    if (I.nk) MPSFM_TRY(hipMemcpyAsync(O.uncertainty_update, d_upd + I.upd_off, sizeof(double) * (size_t)I.nk, hipMemcpyDeviceToHost, B.st));
  }
  MPSFM_TRY(hipStreamSynchronize(B.st));
  if (summary) {
    float ms = 0.f;
    if (int rc = B.elapsed(&ms)) return rc;
    summary->ms = ms;
    summary->n_images = n_images;
    summary->n_pixels = dst;
  }
  return 0;
}

extern "C" int mpsfm_normal_priors(int32_t n_images, const mpsfm_normal_prior_problem* problems, const mpsfm_normal_prior_conf* conf,
                                   int32_t device, const mpsfm_normal_prior_output* outputs, mpsfm_prior_summary* summary) {
  if (n_images == 0) return 0;  // touches nothing
  if (summary) *summary = mpsfm_prior_summary{};
  if (n_images < 0) return fail(MPSFM_EINVAL, "negative size");
  if (!problems || !conf || !outputs) return fail(MPSFM_EINVAL, "NULL pointer");
  if (n_images > 65535) return fail(MPSFM_EINVAL, "more than 65535 images (images are the grid's y dimension)");
  const bool flip = conf->flip_consistency != 0;
  if (conf->std_multiplier != 1.0 && (conf->lc_std_multiplier != 1.0 || conf->prior_std_multiplier != 1.0))
    return fail(MPSFM_EINVAL, "std_multiplier != 1 needs lc_std_multiplier == 1 and prior_std_multiplier == 1");
  if (!(conf->downscale_factor > 0.0)) return fail(MPSFM_EINVAL, "downscale_factor must be positive");

  Pool pool;
  std::vector<NpImage> imgs((size_t)n_images);
  int64_t full = 0, half = 0, max_full = 0, max_half = 0;
  for (int32_t k = 0; k < n_images; ++k) {
    const mpsfm_normal_prior_problem& P = problems[k];
    const mpsfm_normal_prior_output& O = outputs[k];
    if (P.height <= 0 || P.width <= 0 || P.int_height <= 0 || P.int_width <= 0) return fail(MPSFM_EINVAL, "non-positive map size");
    if ((int64_t)P.height * P.width > kMaxPixels || (int64_t)P.int_height * P.int_width > kMaxPixels)
      return fail(MPSFM_EINVAL, "map larger than 2^27 pixels");
    if (!P.normals) return fail(MPSFM_EINVAL, "normals map is NULL");
    if (flip && !P.normals2) return fail(MPSFM_EINVAL, "flip_consistency needs normals2");
    if (!P.normals_variance) return fail(MPSFM_EINVAL, "normals_variance is NULL");
    if (flip && !P.normals2_variance) return fail(MPSFM_EINVAL, "flip_consistency needs normals2_variance");
    if (P.mask && (P.mask_height <= 0 || P.mask_width <= 0 || (int64_t)P.mask_height * P.mask_width > kMaxPixels))
      return fail(MPSFM_EINVAL, "mask size out of range");
    NpImage& I = imgs[(size_t)k];
    I.H = P.height; I.W = P.width; I.Ht = P.int_height; I.Wt = P.int_width;
    const double wd = py_floordiv((double)I.Wt, conf->downscale_factor), hd = py_floordiv((double)I.Ht, conf->downscale_factor);
    if (!(wd >= 1.0) || !(hd >= 1.0)) return fail(MPSFM_EINVAL, "non-positive downscaled map size");
    if (wd * hd > (double)kMaxPixels) return fail(MPSFM_EINVAL, "map larger than 2^27 pixels");
    I.Hd = (int32_t)hd; I.Wd = (int32_t)wd;
    // the caller sized the half-size outputs: a size computed by another rule must not become a write past them
    if (P.half_height != I.Hd || P.half_width != I.Wd)
      return fail(MPSFM_EINVAL, "half_height / half_width are not int(int_height // downscale_factor), int(int_width // downscale_factor)");
    if (!O.data || !O.uncertainty || !O.data_downscaled || !O.uncertainty_downscaled) return fail(MPSFM_EINVAL, "NULL output pointer");
    I.Hm = P.mask ? P.mask_height : 0; I.Wm = P.mask ? P.mask_width : 0;
    I.f32 = P.is_float32 != 0; I.pad = 0;
    const size_t ns = (size_t)P.height * P.width, eb = I.f32 ? 4 : 8;
    I.val_off[0] = pool.add(P.normals, ns * 3 * eb);
    I.val_off[1] = flip ? pool.add(P.normals2, ns * 3 * eb) : -1;
    I.val_off[2] = pool.add(P.normals_variance, ns * eb);
    I.val_off[3] = flip ? pool.add(P.normals2_variance, ns * eb) : -1;
    I.mask_off = pool.add(P.mask, (size_t)I.Hm * I.Wm);
    I.cont_off = pool.add(P.continuity_mask, (size_t)I.Ht * I.Wt);
    I.full_off = full; I.half_off = half;
    const int64_t nf = (int64_t)I.Ht * I.Wt, nh = (int64_t)I.Hd * I.Wd;
    full += nf; half += nh;
    max_full = std::max(max_full, nf); max_half = std::max(max_half, nh);
  }
  if (int rc = open_device(device)) return rc;

  NpConf cf{};
  cf.noise = conf->inherent_polar_noise;
  cf.std2 = conf->std_multiplier * conf->std_multiplier;
  cf.lc2 = conf->lc_std_multiplier * conf->lc_std_multiplier;
  cf.psm2 = conf->prior_std_multiplier * conf->prior_std_multiplier;
  cf.flip = flip;

  CallScope B;
  if (int rc = B.open(true)) return rc;
  uint8_t* d_pool = B.alloc<uint8_t>((size_t)pool.size);
  NpImage* d_imgs = B.alloc<NpImage>(imgs.size());
  double* d_n1 = B.alloc<double>(3 * (size_t)full);
  double* d_v1 = B.alloc<double>((size_t)full);
  double* d_n2 = flip ? B.alloc<double>(3 * (size_t)full) : nullptr;
  double* d_v2 = flip ? B.alloc<double>((size_t)full) : nullptr;
  // the outputs in one block: [data | uncertainty | data_downscaled | uncertainty_downscaled]
  const size_t out_count = 12 * ((size_t)full + (size_t)half);
  double* d_out = B.alloc<double>(out_count);
  if (!d_pool || !d_imgs || !d_n1 || !d_v1 || (flip && (!d_n2 || !d_v2)) || !d_out) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  double* d_data = d_out;
  double* d_unc = d_data + 3 * full;
  double* d_data_h = d_unc + 9 * full;
  double* d_unc_h = d_data_h + 3 * half;
  if (int rc = pool.upload(d_pool)) return rc;
  if (int rc = staged_upload(d_imgs, imgs.data(), sizeof(NpImage) * imgs.size())) return rc;
  if (int rc = staged_drain()) return rc;

  if (int rc = B.begin()) return rc;
  hipLaunchKernelGGL(k_np_full, dim3(blocks_for(max_full), (unsigned)n_images), dim3(kT), 0, B.st, d_imgs, d_pool, cf, d_n1, d_n2, d_v1,
                     d_v2, d_data, d_unc);
  MPSFM_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_np_half, dim3(blocks_for(max_half), (unsigned)n_images), dim3(kT), 0, B.st, d_imgs, cf, d_n1, d_n2, d_v1, d_v2,
                     d_data_h, d_unc_h);
  MPSFM_TRY(hipGetLastError());
  if (int rc = B.stop()) return rc;
  for (int32_t k = 0; k < n_images; ++k) {
    const NpImage& I = imgs[(size_t)k];
    const mpsfm_normal_prior_output& O = outputs[k];
    const size_t nf = (size_t)I.Ht * I.Wt, nh = (size_t)I.Hd * I.Wd;
    MPSFM_TRY(hipMemcpyAsync(O.data, d_data + 3 * I.full_off, sizeof(double) * 3 * nf, hipMemcpyDeviceToHost, B.st));
    MPSFM_TRY(hipMemcpyAsync(O.uncertainty, d_unc + 9 * I.full_off, sizeof(double) * 9 * nf, hipMemcpyDeviceToHost, B.st));
    MPSFM_TRY(hipMemcpyAsync(O.data_downscaled, d_data_h + 3 * I.half_off, sizeof(double) * 3 * nh, hipMemcpyDeviceToHost, B.st));
    MPSFM_TRY(hipMemcpyAsync(O.uncertainty_downscaled, d_unc_h + 9 * I.half_off, sizeof(double) * 9 * nh, hipMemcpyDeviceToHost, B.st));
  }
  MPSFM_TRY(hipStreamSynchronize(B.st));
  if (summary) {
    float ms = 0.f;
    if (int rc = B.elapsed(&ms)) return rc;
    summary->ms = ms;
    summary->n_images = n_images;
    summary->n_pixels = full;
  }
  return 0;
}
