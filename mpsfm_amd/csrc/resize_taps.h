// The resize rules of the prior construction (mono_priors.hip), restated from OpenCV's sampling rule because OpenCV is
// not a dependency.  One axis at a time:
//   bilinear  sample position (i + 0.5) * (1 / (n_dst / n_src)) - 0.5, replicated border, the fraction rounded to float32:
//             the rows of mpsfm_amd.sfm.scene.integration._linear_taps, operation by operation
//   nearest   source index min(floor(i * n_src / n_dst), n_src - 1), in integers
// Every product and sum is rounded on its own (the taps must equal NumPy's): include after bilinear_sample.h, which
// switches contraction off for the rest of the translation unit.
#pragma once
#include "bilinear_sample.h"

namespace mpsfm {

struct Tap {
  int lo, hi;   // source indices, lo <= hi <= lo + 1
  double frac;  // weight of hi; 1 - frac is the weight of lo; 0 on the replicated border
};

__device__ __forceinline__ Tap linear_tap(int n_src, int n_dst, int i) {
  const double scale = 1.0 / ((double)n_dst / (double)n_src);
  const double pos = ((double)i + 0.5) * scale - 0.5;
  const double lof = floor(pos);
  int lo = (int)lof;
  double frac = (double)(float)(pos - lof);
  if (lo < 0 || lo >= n_src - 1) frac = 0.0;
  lo = lo < 0 ? 0 : (lo > n_src - 1 ? n_src - 1 : lo);
  Tap t;
  t.lo = lo;
  t.hi = lo + 1 < n_src ? lo + 1 : n_src - 1;
  t.frac = frac;
  return t;
}

__device__ __forceinline__ int nearest_tap(int n_src, int n_dst, int i) {
  const long long s = ((long long)i * n_src) / n_dst;
  return s < n_src - 1 ? (int)s : n_src - 1;
}

// One bilinear sample: rows first, then columns, as `T_y @ img @ T_x^T` associates.  A tap of zero weight is not read,
// so a NaN next to the border sample stays where it is.  `at(y, x)` returns the source value as double.
template <typename F>
__device__ __forceinline__ double resize_sample(const Tap& ty, const Tap& tx, F at) {
  auto column = [&](int x) {
    const double a = at(ty.lo, x);
    return ty.frac == 0.0 ? a : (1.0 - ty.frac) * a + ty.frac * at(ty.hi, x);
  };
  const double c0 = column(tx.lo);
  return tx.frac == 0.0 ? c0 : (1.0 - tx.frac) * c0 + tx.frac * column(tx.hi);
}

// `resize(mask.astype(float)) == 1`: true iff every tap with a non-zero weight is true
template <typename F>
__device__ __forceinline__ bool resize_mask_all(const Tap& ty, const Tap& tx, F at) {
  bool ok = at(ty.lo, tx.lo);
  if (tx.frac != 0.0) ok = ok && at(ty.lo, tx.hi);
  if (ty.frac != 0.0) {
    ok = ok && at(ty.hi, tx.lo);
    if (tx.frac != 0.0) ok = ok && at(ty.hi, tx.hi);
  }
  return ok;
}

}  // namespace mpsfm
