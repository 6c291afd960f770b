// Constant-size arithmetic of the 3D-3D alignment (align3d.hip): the residual of tgt ~ s R src + t, the closed form
// (Horn's quaternion for R, Umeyama's ratio for s) from centred sums, its two degeneracy rules, the 3-point minimal
// solver and the bilinear lift of a keypoint through a depth map.  COLMAP 3.11 EstimateRigid3dRobust / EstimateSim3dRobust
// semantics as recalled (include/mpsfm_hip.h, mpsfm_align3d_estimate): parity with pycolmap unpinned.
#pragma once
#include "abs_pose_math.h"  // sym_eig, ap_horn
#include "common.h"

// No contraction into fused multiply-adds (nor in align3d.hip, which includes it): every expression rounds as written, as
// in the NumPy restatement (tests/numpy_alignment.py) and, for the lift, as in the reference's float64 NumPy arithmetic.
#pragma clang fp contract(off)

namespace mpsfm {

constexpr int kA3Model = 13;  // [R | t] row-major, then the scale

// |q - (s R p + t)|^2
__host__ __device__ inline double a3_residual(const double* M, double px, double py, double pz, double qx, double qy, double qz) {
  const double s = M[12];
  const double dx = qx - (s * (M[0] * px + M[1] * py + M[2] * pz) + M[3]);
  const double dy = qy - (s * (M[4] * px + M[5] * py + M[6] * pz) + M[7]);
  const double dz = qz - (s * (M[8] * px + M[9] * py + M[10] * pz) + M[11]);
  return dx * dx + dy * dy + dz * dz;
}

// The model from the centroids mp, mq, the centred cross sums S[a][b] = sum (p - mp)_a (q - mq)_b and spp = sum |p - mp|^2:
// R by Horn, s = sum (q - mq)^T R (p - mp) / spp (1 for a rigid fit), t = mq - s R mp.  false: the scale is not finite
// and positive.
__host__ __device__ inline bool a3_from_sums(const double S[3][3], double spp, const double mp[3], const double mq[3], int with_scale,
                                             double* M) {
  double R[9];
  ap_horn(S, R);
  double s = 1.0;
  if (with_scale) {
    double num = 0.0;
    for (int b = 0; b < 3; ++b)
      for (int a = 0; a < 3; ++a) num += R[3 * b + a] * S[a][b];
    s = num / spp;
    if (!(isfinite(s) && s > 0.0)) return false;
  }
  for (int r = 0; r < 3; ++r) {
    M[4 * r] = R[3 * r]; M[4 * r + 1] = R[3 * r + 1]; M[4 * r + 2] = R[3 * r + 2];
    M[4 * r + 3] = mq[r] - s * (R[3 * r] * mp[0] + R[3 * r + 1] * mp[1] + R[3 * r + 2] * mp[2]);
  }
  M[12] = s;
  return true;
}

// a scatter matrix (upper: xx xy xz yy yz zz) spans no plane: its second-largest eigenvalue is <= 1e-12 of its largest
__host__ __device__ inline bool a3_scatter_is_line(const double sc[6]) {
  double A[3][3] = {{sc[0], sc[1], sc[2]}, {sc[1], sc[3], sc[4]}, {sc[2], sc[4], sc[5]}}, V[3][3], w[3];
  sym_eig<3>(A, V, w);
  return !(w[1] > 1e-12 * w[2]);
}

// three points on a line (or two of them coincident): sin^2 of the angle at the first point <= 1e-20, P3P's test
__host__ __device__ inline bool a3_collinear(const double X[3][3]) {
  double e1[3], e2[3];
  for (int k = 0; k < 3; ++k) { e1[k] = X[1][k] - X[0][k]; e2[k] = X[2][k] - X[0][k]; }
  const double cr[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  const double n1 = e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2], n2 = e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2];
  return cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2] <= 1e-20 * n1 * n2;
}

// the minimal solver: P[3][3] source, Q[3][3] target points; false: no model
__host__ __device__ inline bool a3_minimal(const double P[3][3], const double Q[3][3], int with_scale, double* M) {
  if (a3_collinear(P) || a3_collinear(Q)) return false;
  double mp[3], mq[3];
  for (int k = 0; k < 3; ++k) {
    mp[k] = (P[0][k] + P[1][k] + P[2][k]) / 3.0;
    mq[k] = (Q[0][k] + Q[1][k] + Q[2][k]) / 3.0;
  }
  double S[3][3] = {}, spp = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int a = 0; a < 3; ++a) {
      spp += (P[i][a] - mp[a]) * (P[i][a] - mp[a]);
      for (int b = 0; b < 3; ++b) S[a][b] += (P[i][a] - mp[a]) * (Q[i][b] - mq[b]);
    }
  return a3_from_sums(S, spp, mp, mq, with_scale, M);
}

// ---- lifting a keypoint through a depth map -------------------------------------------------------------------------------
// The pixel (c, r) of a PINHOLE depth map as a camera-frame point, as the reference's depth_to_3d forms it
__host__ __device__ inline void a3_pixel_point(double c, double r, double z, const double* intr, double out[3]) {
  out[0] = ((c - intr[2]) * z) / intr[0];
  out[1] = ((r - intr[3]) * z) / intr[1];
  out[2] = z;
}

// The bilinear sample of the (never materialised) point map at (x, y), in the reference's order and association; false
// (and xyz = 0) when the keypoint is invalid by the rule of include/mpsfm_hip.h (mpsfm_lift_keypoints)
__host__ __device__ inline bool a3_lift(const double* depth, int32_t H, int32_t W, const double* intr, double x, double y, double xyz[3]) {
  xyz[0] = xyz[1] = xyz[2] = 0.0;
  if (!(x >= 0.0 && y >= 0.0)) return false;  // NaN fails here
  const double fx0 = trunc(x), fy0 = trunc(y);
  if (!(fx0 + 1.0 <= (double)(W - 1) && fy0 + 1.0 <= (double)(H - 1))) return false;
  const int32_t c0 = (int32_t)fx0, r0 = (int32_t)fy0;
  const double z00 = depth[(size_t)r0 * W + c0], z01 = depth[(size_t)r0 * W + c0 + 1];
  const double z10 = depth[(size_t)(r0 + 1) * W + c0], z11 = depth[(size_t)(r0 + 1) * W + c0 + 1];
  if (!(isfinite(z00) && z00 > 0.0 && isfinite(z01) && z01 > 0.0 && isfinite(z10) && z10 > 0.0 && isfinite(z11) && z11 > 0.0)) return false;
  double a00[3], a01[3], a10[3], a11[3];
  a3_pixel_point((double)c0, (double)r0, z00, intr, a00);
  a3_pixel_point((double)(c0 + 1), (double)r0, z01, intr, a01);
  a3_pixel_point((double)c0, (double)(r0 + 1), z10, intr, a10);
  a3_pixel_point((double)(c0 + 1), (double)(r0 + 1), z11, intr, a11);
  const double ax = x - fx0, ay = y - fy0;
  double v[3];
  for (int k = 0; k < 3; ++k)
    v[k] = a00[k] * (1.0 - ax) * (1.0 - ay) + a01[k] * ax * (1.0 - ay) + a10[k] * (1.0 - ax) * ay + a11[k] * ax * ay;
  if (!(isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]))) return false;  // overflow of a finite input
  xyz[0] = v[0]; xyz[1] = v[1]; xyz[2] = v[2];
  return true;
}

}  // namespace mpsfm
