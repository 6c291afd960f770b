// What the similarity kernels share (k_sim_top2 of descriptor_matches.hip, k_nn_top1 of reciprocal_matches.hip; the arithmetic
// contract and the tie rule: DESIGN.md sections 4m and 4p): the tile geometry, the total order of candidates, the staging of one
// k slice of 64 rows in LDS, and the scan that refuses non-finite device inputs.
#pragma once
#include <algorithm>

#include "call_scope.h"
#include "common.h"

namespace mpsfm {
namespace sim {

constexpr int kStrip = 64;        // rows of a workgroup, columns of a tile
constexpr int kKS = 32;           // k values of a slice
constexpr int kLd = 80;           // doubles per k row of a slice in LDS: the four k rows of one MFMA step sit 32 banks apart
constexpr int kMT = 256;          // threads of the similarity kernels
constexpr int kDT = 256;          // threads of the element-wise kernels
constexpr int32_t kMaxDim = 1024;
constexpr int64_t kMaxDesc = 1 << 24;
constexpr int32_t kNoIndex = INT32_MAX;
constexpr int32_t kFillPerCU = 8; // workgroups per compute unit that fill the device: LDS for four at a time, two rounds

__device__ __forceinline__ bool before(double v, int32_t i, double w, int32_t j) { return v > w || (v == w && i < j); }

template <typename T> struct Vec4;
template <> struct Vec4<float> { typedef float4 type; };
template <> struct Vec4<double> { typedef double4 type; };

// One slice: s[k][column ^ 8 (k / 4 & 7)] = X[row_of(column)][k0 + k], zeros where row_of() is negative and beyond dim.  Thread ->
// (row, four consecutive k): eight lanes read 32 consecutive k of a row; the XOR spreads their LDS stores over all banks and is the
// same for the four k rows an MFMA step reads, so the reads stay conflict free.
template <typename T, typename RowOf>
__device__ __forceinline__ void load_slice_rows(double* __restrict__ s, const T* __restrict__ X, int32_t dim, int32_t k0, bool vec, RowOf row_of) {
#pragma unroll
  for (int j = 0; j < kStrip * kKS / 4 / kMT; ++j) {
    const int e = (int)threadIdx.x + kMT * j;
    const int kq = e & 7, r = e >> 3;
    const int32_t row = row_of(r), k = k0 + 4 * kq;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    if (row >= 0 && k < dim) {
      const T* p = X + (size_t)row * (size_t)dim + k;
      if (vec) {  // dim % 4 == 0 and an aligned base: k + 3 < dim
        const typename Vec4<T>::type q = *reinterpret_cast<const typename Vec4<T>::type*>(p);
        v[0] = (double)q.x; v[1] = (double)q.y; v[2] = (double)q.z; v[3] = (double)q.w;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (k + c < dim) v[c] = (double)p[c];
      }
    }
    const int col = r ^ (8 * kq);
#pragma unroll
    for (int c = 0; c < 4; ++c) s[(4 * kq + c) * kLd + col] = v[c];
  }
}

// the rows row0 .. row0 + 63 of a set of nrows
template <typename T>
__device__ __forceinline__ void load_slice(double* __restrict__ s, const T* __restrict__ X, int32_t nrows, int32_t row0, int32_t dim, int32_t k0,
                                           bool vec) {
  load_slice_rows<T>(s, X, dim, k0, vec, [=](int r) { return row0 + r < nrows ? row0 + r : -1; });
}

static __global__ __launch_bounds__(kDT) void k_scan_finite(const float* __restrict__ x, int64_t n, int32_t* __restrict__ bad) {
  int64_t i = (int64_t)blockIdx.x * kDT + (int64_t)threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kDT;
  bool b = false;
  for (; i < n; i += stride) b = b || !isfinite(x[i]);
  if (b) atomicOr(bad, 1);
}

inline int scan_device(CallScope& A, const float* x, int64_t n, int32_t* d_bad) {
  const int64_t blocks = std::min<int64_t>((n + kDT - 1) / kDT, 4096);
  hipLaunchKernelGGL(k_scan_finite, dim3((unsigned)blocks), dim3(kDT), 0, A.st, x, n, d_bad);
  MPSFM_TRY(hipGetLastError());
  return 0;
}

}  // namespace sim
}  // namespace mpsfm
