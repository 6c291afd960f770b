// Bilinear sampling of a per-image map at a keypoint: PriorUtils._data_at_kps (reference
// mpsfm/sfm/scene/image/mixins/priorutils.py:49-62: torch grid_sample, bilinear, zero padding, align_corners=True,
// keypoints scaled by camera.sx / sy) in the operation order of the restatement
// (mpsfm_amd/sfm/scene/priorutils.py:bilinear_at_kps), shared by k_depth_blocks (prior_kernels.hip) and the registration
// kernels (registration.hip).
//
// hipcc contracts a * b + c into one fused multiply-add by default, and the __dmul_rn / __dadd_rn wrappers of the HIP
// headers are plain operators compiled with contraction allowed (their instructions carry the `contract` flag into
// the caller).  The bit-exact validity decision (sample == 1) needs every product and sum rounded on its own, like
// NumPy / torch on the CPU do: plain operators under this pragma.  At file scope it holds until the end of the
// translation unit: include this header AFTER the headers whose arithmetic must keep the default contraction.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace mpsfm {

// pixel coordinate of grid_sample(align_corners=True) for a keypoint coordinate k scaled by s on an axis of `size`
// samples, in the operation order of the restatement (mpsfm_amd/sfm/scene/priorutils.py:bilinear_at_kps)
__device__ __forceinline__ double grid_coord(double k, double s, int size) {
  const double sm1 = (double)(size - 1);
  double v = k * s;
  v = v / sm1;
  v = v * 2.0;
  v = v - 1.0;
  v = v + 1.0;
  v = v * 0.5;
  return v * sm1;
}

template <typename T>
__device__ __forceinline__ double bilinear(const T* map, int H, int W, double x, double y) {
  const double x0f = floor(x), y0f = floor(y);
  const double wx1 = x - x0f, wy1 = y - y0f;
  const double wx0 = 1.0 - wx1, wy0 = 1.0 - wy1;
  // out-of-range coordinates (also NaN / huge) contribute nothing: zero padding
  const bool fin = (x0f > -2.0) && (x0f < (double)W + 1.0) && (y0f > -2.0) && (y0f < (double)H + 1.0);
  if (!fin) return 0.0;
  const int x0 = (int)x0f, y0 = (int)y0f;
  double out = 0.0;
  const double w[4] = {wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int xi = x0 + (k & 1), yi = y0 + (k >> 1);
    if (xi >= 0 && xi < W && yi >= 0 && yi < H) {
      const double term = w[k] * (double)map[(size_t)yi * W + xi];
      out = out + term;
    }
  }
  return out;
}

}  // namespace mpsfm
