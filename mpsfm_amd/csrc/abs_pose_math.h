// Constant-size arithmetic of the absolute-pose estimator (abs_pose.hip): P3P (Grunert's quartic + Horn's absolute
// orientation), the normalised-plane residual, the symmetric eigen-solver sym_eig (also rel_pose_math.h's) and
// the EPnP algebra that follows the O(N) reductions (control points, 12x12 eigenvectors, L6x10 / rho, the three beta
// approximations with Gauss-Newton, the alignment).  COLMAP 3.11 semantics of P3PEstimator / EPNPEstimator /
// ComputeSquaredReprojectionError as recalled (include/mpsfm_hip.h, mpsfm_abs_pose_estimate):
// parity with the reference's COLMAP fork unpinned.
#pragma once
#include "common.h"
#include "tri_math.h"

// No contraction into fused multiply-adds in this arithmetic (nor in abs_pose.hip, which includes it): every expression rounds
// as written, as in the NumPy restatement (tests/numpy_absolute_pose.py).  Grunert's quartic is ill-conditioned for some
// samples, and contracted coefficients moved 2 % of the P3P poses by more than 1e-9 against it.
#pragma clang fp contract(off)

namespace mpsfm {

// ComputeSquaredReprojectionError for one point: P = [R | t] row-major, x = normalised image point
__host__ __device__ inline double ap_residual(const double* P, double X, double Y, double Z, double u, double v) {
  const double z = P[8] * X + P[9] * Y + P[10] * Z + P[11];
  if (!(z > DBL_EPSILON)) return DBL_MAX;
  const double dx = (P[0] * X + P[1] * Y + P[2] * Z + P[3]) / z - u;
  const double dy = (P[4] * X + P[5] * Y + P[6] * Z + P[7]) / z - v;
  return dx * dx + dy * dy;
}

// ---- symmetric eigen-decomposition (cyclic Jacobi; eigenvalues ascending, eigenvectors in the columns of V) ------------
template <int N>
__host__ __device__ inline void sym_eig(double A[N][N], double V[N][N], double w[N]) {
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < N; ++i) {
      diag += A[i][i] * A[i][i];
      for (int j = i + 1; j < N; ++j) off += A[i][j] * A[i][j];
    }
    if (off <= 1e-34 * diag || off < 1e-300) break;
    for (int p = 0; p < N - 1; ++p)
      for (int q = p + 1; q < N; ++q) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
        for (int k = 0; k < N; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < N; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < N; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  for (int i = 0; i < N; ++i) w[i] = A[i][i];
  for (int i = 1; i < N; ++i) {  // insertion sort, ascending
    for (int j = i; j > 0 && w[j] < w[j - 1]; --j) {
      const double tw = w[j]; w[j] = w[j - 1]; w[j - 1] = tw;
      for (int k = 0; k < N; ++k) { const double tv = V[k][j]; V[k][j] = V[k][j - 1]; V[k][j - 1] = tv; }
    }
  }
}

// Horn's closed-form absolute orientation: the rotation R maximising sum (c_i - c0)^T R (w_i - w0) for
// S[a][b] = sum (w_i - w0)_a (c_i - c0)_b (world, camera); R row-major
__host__ __device__ inline void ap_horn(const double S[3][3], double R[9]) {
  const double Sxx = S[0][0], Sxy = S[0][1], Sxz = S[0][2], Syx = S[1][0], Syy = S[1][1], Syz = S[1][2], Szx = S[2][0], Szy = S[2][1],
               Szz = S[2][2];
  double N[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                    {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                    {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                    {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
  double V[4][4], ev[4];
  sym_eig<4>(N, V, ev);
  double w = V[0][3], x = V[1][3], y = V[2][3], z = V[3][3];
  const double nq = sqrt(w * w + x * x + y * y + z * z);
  w /= nq; x /= nq; y /= nq; z /= nq;
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = 1 - 2 * (x * x + y * y);
}

// ---- P3P ----------------------------------------------------------------------------------------------------------
struct ApCplx { double re, im; };
__host__ __device__ inline ApCplx ap_cadd(ApCplx a, ApCplx b) { return {a.re + b.re, a.im + b.im}; }
__host__ __device__ inline ApCplx ap_csub(ApCplx a, ApCplx b) { return {a.re - b.re, a.im - b.im}; }
__host__ __device__ inline ApCplx ap_cmul(ApCplx a, ApCplx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__host__ __device__ inline ApCplx ap_cdiv(ApCplx a, ApCplx b) {
  const double d = b.re * b.re + b.im * b.im;
  return {(a.re * b.re + a.im * b.im) / d, (a.im * b.re - a.re * b.im) / d};
}

// the four complex roots of c[0] x^4 + c[1] x^3 + ... + c[4] (c[0] != 0): Aberth-Ehrlich iteration, then two Newton steps
__host__ __device__ inline void ap_quartic_roots(const double c[5], ApCplx z[4]) {
  double a[5];
  for (int i = 0; i < 5; ++i) a[i] = c[i] / c[0];
  double rad = 0.0;  // Cauchy bound
  for (int i = 1; i < 5; ++i) rad = fmax(rad, fabs(a[i]));
  rad = 1.0 + rad;
  const double r0 = 0.5 * rad;
  for (int k = 0; k < 4; ++k) {
    const double ang = 0.4 + 1.5707963267948966 * k;
    z[k] = {r0 * cos(ang), r0 * sin(ang)};
  }
  auto eval = [&](ApCplx x, ApCplx& p, ApCplx& dp) {
    p = {a[0], 0.0}; dp = {0.0, 0.0};
    for (int i = 1; i < 5; ++i) { dp = ap_cadd(ap_cmul(dp, x), p); p = ap_cadd(ap_cmul(p, x), {a[i], 0.0}); }
  };
  for (int it = 0; it < 100; ++it) {
    double moved = 0.0;
    for (int k = 0; k < 4; ++k) {
      ApCplx p, dp;
      eval(z[k], p, dp);
      if (p.re == 0.0 && p.im == 0.0) continue;
      const ApCplx ratio = ap_cdiv(p, dp);
      ApCplx sum = {0.0, 0.0};
      for (int j = 0; j < 4; ++j)
        if (j != k) sum = ap_cadd(sum, ap_cdiv({1.0, 0.0}, ap_csub(z[k], z[j])));
      const ApCplx den = ap_csub({1.0, 0.0}, ap_cmul(ratio, sum));
      const ApCplx step = ap_cdiv(ratio, den);
      if (!(isfinite(step.re) && isfinite(step.im))) continue;
      z[k] = ap_csub(z[k], step);
      moved = fmax(moved, sqrt(step.re * step.re + step.im * step.im) / (1.0 + sqrt(z[k].re * z[k].re + z[k].im * z[k].im)));
    }
    if (moved < 1e-16) break;
  }
  for (int k = 0; k < 4; ++k)
    for (int it = 0; it < 2; ++it) {
      ApCplx p, dp;
      eval(z[k], p, dp);
      if (dp.re == 0.0 && dp.im == 0.0) break;
      const ApCplx step = ap_cdiv(p, dp);
      if (!(isfinite(step.re) && isfinite(step.im))) break;
      z[k] = ap_csub(z[k], step);
    }
}

constexpr double kApMaxRootImag = 1e-10;

// P3PEstimator::Estimate: x[3][2] normalised image points, X[3][3] world points; writes up to 4 models (12 doubles each)
__host__ __device__ inline int ap_p3p(const double x[3][2], const double X[3][3], double* models) {
  double e1[3], e2[3];
  for (int k = 0; k < 3; ++k) { e1[k] = X[1][k] - X[0][k]; e2[k] = X[2][k] - X[0][k]; }
  const double cr[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  const double n1 = e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2], n2 = e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2];
  if (cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2] <= 1e-20 * n1 * n2) return 0;  // collinear (or coincident) world points
  double f[3][3];
  for (int i = 0; i < 3; ++i) {
    const double nr = sqrt(x[i][0] * x[i][0] + x[i][1] * x[i][1] + 1.0);
    f[i][0] = x[i][0] / nr; f[i][1] = x[i][1] / nr; f[i][2] = 1.0 / nr;
  }
  double a2 = 0, b2 = 0, c2 = 0;  // |BC|^2, |AC|^2, |AB|^2
  for (int k = 0; k < 3; ++k) {
    a2 += (X[1][k] - X[2][k]) * (X[1][k] - X[2][k]);
    b2 += (X[0][k] - X[2][k]) * (X[0][k] - X[2][k]);
    c2 += (X[0][k] - X[1][k]) * (X[0][k] - X[1][k]);
  }
  const double ca = f[1][0] * f[2][0] + f[1][1] * f[2][1] + f[1][2] * f[2][2];  // angle at the centre between B and C
  const double cb = f[0][0] * f[2][0] + f[0][1] * f[2][1] + f[0][2] * f[2][2];  // A and C
  const double cg = f[0][0] * f[1][0] + f[0][1] * f[1][1] + f[0][2] * f[1][2];  // A and B
  const double amc = (a2 - c2) / b2, apc = (a2 + c2) / b2;
  double c[5];
  c[0] = (amc - 1) * (amc - 1) - 4 * c2 / b2 * ca * ca;
  c[1] = 4 * (amc * (1 - amc) * cb - (1 - apc) * ca * cg + 2 * c2 / b2 * ca * ca * cb);
  c[2] = 2 * (amc * amc - 1 + 2 * amc * amc * cb * cb + 2 * (b2 - c2) / b2 * ca * ca - 4 * apc * ca * cb * cg + 2 * (b2 - a2) / b2 * cg * cg);
  c[3] = 4 * (-amc * (1 + amc) * cb + 2 * a2 / b2 * cg * cg * cb - (1 - apc) * ca * cg);
  c[4] = (1 + amc) * (1 + amc) - 4 * a2 / b2 * cg * cg;
  if (c[0] == 0.0 || !isfinite(c[0])) return 0;
  ApCplx z[4];
  ap_quartic_roots(c, z);
  // the real roots in ascending order: a root finder's own order is arbitrary, and the order of the models decides which one a
  // trial scores first (LO-RANSAC's decisions and its stop inside a trial depend on it)
  // (The list is appended to, insertion-sorted and read with every index a constant after unrolling: indexed by nr or by
  // a loop counter it would live in scratch on the device.  The comparisons and their order are the plain loops'.)
  double vr[4] = {0.0, 0.0, 0.0, 0.0};
  int nr = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (fabs(z[r].im) <= kApMaxRootImag) {
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (s == nr) vr[s] = z[r].re;
      ++nr;
    }
#pragma unroll
  for (int i = 1; i < 4; ++i) {
    bool go = i < nr;  // for (j = i; j > 0 && vr[j] < vr[j - 1]; --j) swap
#pragma unroll
    for (int j = i; j > 0; --j) {
      go = go && vr[j] < vr[j - 1];
      if (go) { const double tv = vr[j]; vr[j] = vr[j - 1]; vr[j - 1] = tv; }
    }
  }
  int nm = 0;
  for (int r = 0; r < nr; ++r) {
    const double v = r == 0 ? vr[0] : r == 1 ? vr[1] : r == 2 ? vr[2] : vr[3];  // s3 / s1
    if (v < 0) continue;
    const double den = 2 * (cg - v * ca);
    if (den == 0.0) continue;
    const double u = ((-1 + amc) * v * v - 2 * amc * cb * v + 1 + amc) / den;  // s2 / s1
    if (u < 0) continue;
    const double s1 = sqrt(b2 / (1 + v * v - 2 * v * cb));
    const double s[3] = {s1, u * s1, v * s1};
    if (!(isfinite(s[1]) && isfinite(s[2]))) continue;
    double Y[3][3], w0[3] = {0, 0, 0}, y0[3] = {0, 0, 0};
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k) {
        Y[i][k] = s[i] * f[i][k];
        w0[k] += X[i][k] / 3.0;
        y0[k] += Y[i][k] / 3.0;
      }
    double S[3][3] = {};
    for (int i = 0; i < 3; ++i)
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) S[a][b] += (X[i][a] - w0[a]) * (Y[i][b] - y0[b]);
    double R[9];
    ap_horn(S, R);
    double* P = models + 12 * nm;
    for (int i = 0; i < 3; ++i) {
      P[4 * i] = R[3 * i]; P[4 * i + 1] = R[3 * i + 1]; P[4 * i + 2] = R[3 * i + 2];
      P[4 * i + 3] = y0[i] - (R[3 * i] * w0[0] + R[3 * i + 1] * w0[1] + R[3 * i + 2] * w0[2]);
    }
    ++nm;
  }
  return nm;
}

// ---- EPnP (host side of the device reductions) ----------------------------------------------------------------------
// least squares min |A x - b| for A [m][k] row-major (m >= k), Householder QR; false when rank deficient
__host__ __device__ inline bool ap_lstsq(const double* A_in, int m, int k, const double* b_in, double* x) {
  double A[6 * 5], b[6];
  for (int i = 0; i < m * k; ++i) A[i] = A_in[i];
  for (int i = 0; i < m; ++i) b[i] = b_in[i];
  for (int j = 0; j < k; ++j) {
    double nrm = 0;
    for (int i = j; i < m; ++i) nrm += A[i * k + j] * A[i * k + j];
    nrm = sqrt(nrm);
    if (nrm == 0.0) return false;
    const double alpha = A[j * k + j] > 0 ? -nrm : nrm;
    double v[6];
    for (int i = 0; i < m; ++i) v[i] = i < j ? 0.0 : A[i * k + j];
    v[j] -= alpha;
    double vv = 0;
    for (int i = j; i < m; ++i) vv += v[i] * v[i];
    if (vv == 0.0) continue;
    for (int c = j; c < k; ++c) {
      double d = 0;
      for (int i = j; i < m; ++i) d += v[i] * A[i * k + c];
      d = 2 * d / vv;
      for (int i = j; i < m; ++i) A[i * k + c] -= d * v[i];
    }
    double d = 0;
    for (int i = j; i < m; ++i) d += v[i] * b[i];
    d = 2 * d / vv;
    for (int i = j; i < m; ++i) b[i] -= d * v[i];
  }
  for (int j = k - 1; j >= 0; --j) {
    double s = b[j];
    for (int c = j + 1; c < k; ++c) s -= A[j * k + c] * x[c];
    if (A[j * k + j] == 0.0) return false;
    x[j] = s / A[j * k + j];
  }
  return true;
}

// control points from the inlier centroid c0 and scatter sum (X - c0)(X - c0)^T (upper: xx xy xz yy yz zz); false when
// the barycentric frame is singular (ComputeBarycentricCoordinates' rank test)
struct ApEpnpFrame { double cws[4][3]; double CCinv[9]; };
__host__ __device__ inline bool ap_epnp_frame(const double c0[3], const double sc[6], int64_t n, ApEpnpFrame& F) {
  double A[3][3] = {{sc[0], sc[1], sc[2]}, {sc[1], sc[3], sc[4]}, {sc[2], sc[4], sc[5]}}, V[3][3], w[3];
  sym_eig<3>(A, V, w);  // ascending: PCA axis i (descending) is column 2 - i
  // an eigenvector's sign is arbitrary (upstream: whatever Eigen's JacobiSVD returns) and, with noise, EPnP's result depends
  // on it: each axis is oriented so that its largest-magnitude component is positive
  for (int c = 0; c < 3; ++c) {
    int im = 0;
    for (int d = 1; d < 3; ++d)
      if (fabs(V[d][c]) > fabs(V[im][c])) im = d;
    if (V[im][c] < 0)
      for (int d = 0; d < 3; ++d) V[d][c] = -V[d][c];
  }
  double k[3];
  for (int i = 0; i < 3; ++i) {
    k[i] = sqrt(fmax(w[2 - i], 0.0) / (double)n);
    for (int d = 0; d < 3; ++d) { F.cws[0][d] = c0[d]; F.cws[i + 1][d] = c0[d] + k[i] * V[d][2 - i]; }
  }
  if (!(k[2] > 6.66e-16 * k[0])) return false;
  double CC[9];  // columns cws[j] - cws[0]
  for (int r = 0; r < 3; ++r)
    for (int j = 0; j < 3; ++j) CC[3 * r + j] = F.cws[j + 1][r] - F.cws[0][r];
  const double det = CC[0] * (CC[4] * CC[8] - CC[5] * CC[7]) - CC[1] * (CC[3] * CC[8] - CC[5] * CC[6]) + CC[2] * (CC[3] * CC[7] - CC[4] * CC[6]);
  if (det == 0.0 || !isfinite(det)) return false;
  F.CCinv[0] = (CC[4] * CC[8] - CC[5] * CC[7]) / det; F.CCinv[1] = (CC[2] * CC[7] - CC[1] * CC[8]) / det; F.CCinv[2] = (CC[1] * CC[5] - CC[2] * CC[4]) / det;
  F.CCinv[3] = (CC[5] * CC[6] - CC[3] * CC[8]) / det; F.CCinv[4] = (CC[0] * CC[8] - CC[2] * CC[6]) / det; F.CCinv[5] = (CC[2] * CC[3] - CC[0] * CC[5]) / det;
  F.CCinv[6] = (CC[3] * CC[7] - CC[4] * CC[6]) / det; F.CCinv[7] = (CC[1] * CC[6] - CC[0] * CC[7]) / det; F.CCinv[8] = (CC[0] * CC[4] - CC[1] * CC[3]) / det;
  return true;
}

__host__ __device__ inline void ap_alphas(const ApEpnpFrame& F, double X, double Y, double Z, double al[4]) {
  const double d0 = X - F.cws[0][0], d1 = Y - F.cws[0][1], d2 = Z - F.cws[0][2];
  al[1] = F.CCinv[0] * d0 + F.CCinv[1] * d1 + F.CCinv[2] * d2;
  al[2] = F.CCinv[3] * d0 + F.CCinv[4] * d1 + F.CCinv[5] * d2;
  al[3] = F.CCinv[6] * d0 + F.CCinv[7] * d1 + F.CCinv[8] * d2;
  al[0] = 1.0 - al[1] - al[2] - al[3];
}

// the two rows of M for one point (fu = fv = 1, uc = vc = 0: the points are normalised)
__host__ __device__ inline void ap_m_rows(const double al[4], double u, double v, double r1[12], double r2[12]) {
  for (int j = 0; j < 4; ++j) {
    r1[3 * j] = al[j]; r1[3 * j + 1] = 0.0; r1[3 * j + 2] = -al[j] * u;
    r2[3 * j] = 0.0; r2[3 * j + 1] = al[j]; r2[3 * j + 2] = -al[j] * v;
  }
}

// the three beta solutions of EPNPEstimator::ComputePose (approximations 1, 2, 3, each refined by 5 Gauss-Newton steps) as
// camera-frame control points ccs[s][j][3]; vs[i] = eigenvector of the i-th smallest eigenvalue of M^T M
__host__ __device__ inline void ap_epnp_betas(const double vs[4][12], const ApEpnpFrame& F, double ccs[3][4][3]) {
  double dv[4][6][3];
  for (int i = 0; i < 4; ++i) {
    int a = 0, b = 1;
    for (int j = 0; j < 6; ++j) {
      for (int d = 0; d < 3; ++d) dv[i][j][d] = vs[i][3 * a + d] - vs[i][3 * b + d];
      if (++b > 3) { ++a; b = a + 1; }
    }
  }
  auto dot = [](const double* p, const double* q) { return p[0] * q[0] + p[1] * q[1] + p[2] * q[2]; };
  double L[6][10];
  for (int i = 0; i < 6; ++i) {
    L[i][0] = dot(dv[0][i], dv[0][i]);
    L[i][1] = 2.0 * dot(dv[0][i], dv[1][i]);
    L[i][2] = dot(dv[1][i], dv[1][i]);
    L[i][3] = 2.0 * dot(dv[0][i], dv[2][i]);
    L[i][4] = 2.0 * dot(dv[1][i], dv[2][i]);
    L[i][5] = dot(dv[2][i], dv[2][i]);
    L[i][6] = 2.0 * dot(dv[0][i], dv[3][i]);
    L[i][7] = 2.0 * dot(dv[1][i], dv[3][i]);
    L[i][8] = 2.0 * dot(dv[2][i], dv[3][i]);
    L[i][9] = dot(dv[3][i], dv[3][i]);
  }
  double rho[6];
  const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {1, 2, 3, 2, 3, 3};
  for (int i = 0; i < 6; ++i) {
    rho[i] = 0.0;
    for (int d = 0; d < 3; ++d) rho[i] += (F.cws[pa[i]][d] - F.cws[pb[i]][d]) * (F.cws[pa[i]][d] - F.cws[pb[i]][d]);
  }
  for (int s = 0; s < 3; ++s) {
    double be[4] = {0, 0, 0, 0};
    if (s == 0) {  // [B11 B12 B13 B14]
      double A[6 * 4], x[4] = {0, 0, 0, 0};
      for (int i = 0; i < 6; ++i) { A[4 * i] = L[i][0]; A[4 * i + 1] = L[i][1]; A[4 * i + 2] = L[i][3]; A[4 * i + 3] = L[i][6]; }
      ap_lstsq(A, 6, 4, rho, x);
      if (x[0] < 0) { be[0] = sqrt(-x[0]); be[1] = -x[1] / be[0]; be[2] = -x[2] / be[0]; be[3] = -x[3] / be[0]; }
      else { be[0] = sqrt(x[0]); be[1] = x[1] / be[0]; be[2] = x[2] / be[0]; be[3] = x[3] / be[0]; }
    } else if (s == 1) {  // [B11 B12 B22]
      double A[6 * 3], x[3] = {0, 0, 0};
      for (int i = 0; i < 6; ++i) { A[3 * i] = L[i][0]; A[3 * i + 1] = L[i][1]; A[3 * i + 2] = L[i][2]; }
      ap_lstsq(A, 6, 3, rho, x);
      if (x[0] < 0) { be[0] = sqrt(-x[0]); be[1] = x[2] < 0 ? sqrt(-x[2]) : 0.0; }
      else { be[0] = sqrt(x[0]); be[1] = x[2] > 0 ? sqrt(x[2]) : 0.0; }
      if (x[1] < 0) be[0] = -be[0];
    } else {  // [B11 B12 B22 B13 B23]
      double A[6 * 5], x[5] = {0, 0, 0, 0, 0};
      for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 5; ++j) A[5 * i + j] = L[i][j];
      ap_lstsq(A, 6, 5, rho, x);
      if (x[0] < 0) { be[0] = sqrt(-x[0]); be[1] = x[2] < 0 ? sqrt(-x[2]) : 0.0; }
      else { be[0] = sqrt(x[0]); be[1] = x[2] > 0 ? sqrt(x[2]) : 0.0; }
      if (x[1] < 0) be[0] = -be[0];
      be[2] = x[3] / be[0];
    }
    for (int it = 0; it < 5; ++it) {  // RunGaussNewton
      double A[6 * 4], r[6], dx[4] = {0, 0, 0, 0};
      for (int i = 0; i < 6; ++i) {
        const double* l = L[i];
        A[4 * i] = 2 * l[0] * be[0] + l[1] * be[1] + l[3] * be[2] + l[6] * be[3];
        A[4 * i + 1] = l[1] * be[0] + 2 * l[2] * be[1] + l[4] * be[2] + l[7] * be[3];
        A[4 * i + 2] = l[3] * be[0] + l[4] * be[1] + 2 * l[5] * be[2] + l[8] * be[3];
        A[4 * i + 3] = l[6] * be[0] + l[7] * be[1] + l[8] * be[2] + 2 * l[9] * be[3];
        r[i] = rho[i] - (l[0] * be[0] * be[0] + l[1] * be[0] * be[1] + l[2] * be[1] * be[1] + l[3] * be[0] * be[2] + l[4] * be[1] * be[2] +
                         l[5] * be[2] * be[2] + l[6] * be[0] * be[3] + l[7] * be[1] * be[3] + l[8] * be[2] * be[3] + l[9] * be[3] * be[3]);
      }
      if (!ap_lstsq(A, 6, 4, r, dx)) break;
      for (int k = 0; k < 4; ++k) be[k] += dx[k];
    }
    for (int j = 0; j < 4; ++j)
      for (int d = 0; d < 3; ++d) {
        double acc = 0.0;
        for (int i = 0; i < 4; ++i) acc += be[i] * vs[i][3 * j + d];
        ccs[s][j][d] = acc;
      }
  }
}

}  // namespace mpsfm
