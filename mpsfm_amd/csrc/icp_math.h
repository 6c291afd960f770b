// Constant-size arithmetic of the dense point-to-plane ICP (depth_icp.hip; rules: include/mpsfm_hip.h, mpsfm_depth_pair_icp):
// the normal of a depth pixel, one source pixel's association and linearisation, and the 6 x 6 step (symmetric scaling,
// Cholesky without pivoting, Rodrigues update).  Restated line by line in tests/numpy_depth_icp.py.
#pragma once
#include "align3d_math.h"  // a3_pixel_point
#include "common.h"

// No contraction into fused multiply-adds (nor in depth_icp.hip, which includes it): every expression rounds as written.
#pragma clang fp contract(off)

namespace mpsfm {

// one thread's (and, reduced, one iteration's) sums: the 21 upper terms of A = sum J J^T row by row, sum J r, sum r^2, the pair
// count and the four rejection counts (counts as doubles: exact below 2^53)
constexpr int kIcpA = 0, kIcpB = 21, kIcpRR = 27, kIcpCount = 28, kIcpRej = 29, kIcpK = 33;
constexpr double kIcpMinPivot = 1e-10;   // of the matrix scaled to unit diagonal
constexpr double kIcpSmallAngle = 1e-12;  // below it exp(w) = I + [w]x

__host__ __device__ inline bool icp_depth_valid(double z) { return isfinite(z) && z > 0.0; }

// The camera-facing unit normal of the interior pixel (r, c) by central differences of the vertex map; false (and n = 0)
// when a vertex of the cross is a hole, a neighbour's depth differs by more than edge_ratio z_c, or the cross product
// degenerates.  The caller keeps border pixels away.
__host__ __device__ inline bool icp_normal(const double* depth, int32_t W, const double* intr, double edge_ratio, int32_t r, int32_t c, double n[3]) {
  n[0] = n[1] = n[2] = 0.0;
  const size_t at = (size_t)r * W + c;
  const double zc = depth[at], zl = depth[at - 1], zr = depth[at + 1], zu = depth[at - W], zd = depth[at + W];
  if (!(icp_depth_valid(zc) && icp_depth_valid(zl) && icp_depth_valid(zr) && icp_depth_valid(zu) && icp_depth_valid(zd))) return false;
  const double edge = edge_ratio * zc;
  if (!(fabs(zl - zc) <= edge && fabs(zr - zc) <= edge && fabs(zu - zc) <= edge && fabs(zd - zc) <= edge)) return false;
  double V[3], Vl[3], Vr[3], Vu[3], Vd[3];
  a3_pixel_point((double)c, (double)r, zc, intr, V);
  a3_pixel_point((double)(c - 1), (double)r, zl, intr, Vl);
  a3_pixel_point((double)(c + 1), (double)r, zr, intr, Vr);
  a3_pixel_point((double)c, (double)(r - 1), zu, intr, Vu);
  a3_pixel_point((double)c, (double)(r + 1), zd, intr, Vd);
  const double a[3] = {Vr[0] - Vl[0], Vr[1] - Vl[1], Vr[2] - Vl[2]}, b[3] = {Vd[0] - Vu[0], Vd[1] - Vu[1], Vd[2] - Vu[2]};
  const double m[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  const double mm = m[0] * m[0] + m[1] * m[1] + m[2] * m[2];
  if (!(isfinite(mm) && mm > 0.0)) return false;
  const double len = sqrt(mm);
  const double u[3] = {m[0] / len, m[1] / len, m[2] / len};
  const double d = u[0] * V[0] + u[1] * V[1] + u[2] * V[2];
  if (!(d < 0.0 || d > 0.0)) return false;
  const double sgn = d > 0.0 ? -1.0 : 1.0;
  n[0] = sgn * u[0]; n[1] = sgn * u[1]; n[2] = sgn * u[2];
  return true;
}

struct IcpTarget {
  const double* depth;
  const double* normals;  // [H][W][3]
  const uint8_t* valid;   // [H][W]
  int32_t H, W;
  double intr[4];
};
struct IcpGates { double scale, max_d2, min_cos; };

// One source pixel (vertex p, normal n0) at the pose T = [R | t]: its association with the target map and its terms added to
// acc[kIcpK].  A pixel fails at the first test it does not pass.
__host__ __device__ inline void icp_link(const double* T, const IcpGates& g, const IcpTarget& m, const double p[3], const double n0[3], double* acc) {
  double x[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) x[k] = g.scale * (T[4 * k] * p[0] + T[4 * k + 1] * p[1] + T[4 * k + 2] * p[2]) + T[4 * k + 3];
  if (!(x[2] > 0.0)) { acc[kIcpRej] += 1.0; return; }
  const double u = (x[0] / x[2]) * m.intr[0] + m.intr[2], v = (x[1] / x[2]) * m.intr[1] + m.intr[3];
  const double cf = floor(u + 0.5), rf = floor(v + 0.5);
  if (!(cf >= 0.0 && cf <= (double)(m.W - 1) && rf >= 0.0 && rf <= (double)(m.H - 1))) { acc[kIcpRej] += 1.0; return; }
  const size_t at = (size_t)(int32_t)rf * m.W + (int32_t)cf;
  if (!m.valid[at]) { acc[kIcpRej + 1] += 1.0; return; }
  double q[3];
  a3_pixel_point(cf, rf, m.depth[at], m.intr, q);
  const double n1[3] = {m.normals[3 * at], m.normals[3 * at + 1], m.normals[3 * at + 2]};
  const double d[3] = {x[0] - q[0], x[1] - q[1], x[2] - q[2]};
  if (!(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] <= g.max_d2)) { acc[kIcpRej + 2] += 1.0; return; }
  double c = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) c += (T[4 * k] * n0[0] + T[4 * k + 1] * n0[1] + T[4 * k + 2] * n0[2]) * n1[k];
  if (!(c >= g.min_cos)) { acc[kIcpRej + 3] += 1.0; return; }
  const double res = n1[0] * d[0] + n1[1] * d[1] + n1[2] * d[2];
  const double J[6] = {x[1] * n1[2] - x[2] * n1[1], x[2] * n1[0] - x[0] * n1[2], x[0] * n1[1] - x[1] * n1[0], n1[0], n1[1], n1[2]};
  int k = kIcpA;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) acc[k++] += J[i] * J[j];
#pragma unroll
  for (int i = 0; i < 6; ++i) acc[kIcpB + i] += J[i] * res;
  acc[kIcpRR] += res * res;
  acc[kIcpCount] += 1.0;
}

// sums[kIcpK] as the symmetric A [6][6] and b = -sum J r
__host__ __device__ inline void icp_system(const double* sums, double* A, double* b) {
  int k = kIcpA;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j, ++k) A[6 * i + j] = A[6 * j + i] = sums[k];
  for (int i = 0; i < 6; ++i) b[i] = -sums[kIcpB + i];
}

// A xi = b by Cholesky of D^-1 A D^-1, D = sqrt(diag A); false: a diagonal entry of A is not > 0 or a pivot of the scaled
// matrix is not > kIcpMinPivot
__host__ __device__ inline bool icp_solve(const double* A, const double* b, double xi[6]) {
  double d[6], L[6][6], y[6];
  for (int i = 0; i < 6; ++i) {
    if (!(A[6 * i + i] > 0.0)) return false;
    d[i] = sqrt(A[6 * i + i]);
  }
  for (int j = 0; j < 6; ++j) {
    double s = A[6 * j + j] / (d[j] * d[j]);
    for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
    if (!(s > kIcpMinPivot)) return false;
    L[j][j] = sqrt(s);
    for (int i = j + 1; i < 6; ++i) {
      double e = A[6 * i + j] / (d[i] * d[j]);
      for (int k = 0; k < j; ++k) e -= L[i][k] * L[j][k];
      L[i][j] = e / L[j][j];
    }
  }
  for (int i = 0; i < 6; ++i) {
    double s = b[i] / d[i];
    for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
    for (int k = i + 1; k < 6; ++k) s -= L[k][i] * xi[k];
    xi[i] = s / L[i][i];
  }
  for (int i = 0; i < 6; ++i) xi[i] = xi[i] / d[i];
  return true;
}

// T <- exp(xi) T for the left increment xi = (w, v): R <- exp(w) R, t <- exp(w) t + v.  norms: |w|, |v|
__host__ __device__ inline void icp_apply(const double xi[6], double* T, double norms[2]) {
  const double* w = xi;
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = sqrt(th2);
  const double Kx[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
  double E[3][3];
  double a = 1.0, b = 0.0;
  if (!(th < kIcpSmallAngle)) {
    const double sh = sin(0.5 * th);
    a = sin(th) / th;
    b = (2.0 * (sh * sh)) / th2;
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) E[i][j] = (i == j ? 1.0 : 0.0) + a * Kx[i][j] + b * (w[i] * w[j] - (i == j ? th2 : 0.0));
  double out[12];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) out[4 * i + j] = E[i][0] * T[j] + E[i][1] * T[4 + j] + E[i][2] * T[8 + j];
    out[4 * i + 3] = E[i][0] * T[3] + E[i][1] * T[7] + E[i][2] * T[11] + xi[3 + i];
  }
  for (int k = 0; k < 12; ++k) T[k] = out[k];
  norms[0] = th;
  norms[1] = sqrt(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5]);
}

}  // namespace mpsfm
