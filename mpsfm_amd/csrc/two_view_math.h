// Constant-size arithmetic of the two-view geometry estimator (two_view.hip): the seven-point fundamental-matrix solver,
// the four-point homography DLT, the forward transfer error, and on the host the algebra that follows the local
// estimators' reductions (Hartley normalisation from moments, the 9 x 9 Gram matrix -> F or H) and the homography
// decomposition.  COLMAP 3.11 semantics of FundamentalMatrixSevenPointEstimator / FundamentalMatrixEightPointEstimator /
// HomographyMatrixEstimator / DecomposeHomographyMatrix / PoseFromHomographyMatrix as recalled (include/mpsfm_hip.h,
// mpsfm_two_view_geometry): parity with the reference's COLMAP fork unpinned.
//
// As in rel_pose_math.h every runtime-indexed array of a minimal solver lives in a caller-provided work area RpW (on the
// device a strided per-thread slice of LDS, on the host a local array with stride 1), so the kernels need no scratch.
#pragma once
#include "rel_pose_math.h"

// no contraction into fused multiply-adds: every expression rounds as written
#pragma clang fp contract(off)

namespace mpsfm {

constexpr int kTvFSample = 7, kTvFMaxModels = 3;
constexpr int kTvHSample = 4;
constexpr double kTvRankTol = 1e-12;       // Householder column norm (or singular value) / ||A||_F: below it the sample has no model
constexpr double kTvCollinearTol = 1e-10;  // sin of the angle at a point of a triple: at or below it the triple is collinear

// work-area layout of the seven-point solver (doubles): A^T [9][7], Householder scalars [7], nullspace [2][9]
constexpr int TVF_A = 0, TVF_HH = 63, TVF_N = 70, TVF_WORK = 88;
// of the four-point DLT: A^T [9][8], Householder scalars [8], null vector [9]
constexpr int TVH_A = 0, TVH_HH = 72, TVH_N = 80, TVH_WORK = 89;

// Householder QR of the 9 x C matrix at w[a0] (row-major, C columns); the K = 9 - C nullspace vectors H e_C .. H e_8 go to
// w[n0 + 9 k].  false: a column norm at or below kTvRankTol ||A||_F (rank < C)
template <int C>
__host__ __device__ inline bool tv_nullspace(RpW w, int a0, int hh0, int n0) {
  double fro = 0.0;
  for (int i = 0; i < 9 * C; ++i) fro += w[a0 + i] * w[a0 + i];
  fro = sqrt(fro);
  for (int j = 0; j < C; ++j) {
    double nrm = 0.0;
    for (int r = j; r < 9; ++r) nrm += w[a0 + C * r + j] * w[a0 + C * r + j];
    nrm = sqrt(nrm);
    if (!(nrm > kTvRankTol * fro)) return false;
    const double alpha = w[a0 + C * j + j] > 0 ? -nrm : nrm;
    w[a0 + C * j + j] -= alpha;
    double vv = 0.0;
    for (int r = j; r < 9; ++r) vv += w[a0 + C * r + j] * w[a0 + C * r + j];
    w[hh0 + j] = vv;
    for (int c = j + 1; c < C; ++c) {
      double d = 0.0;
      for (int r = j; r < 9; ++r) d += w[a0 + C * r + j] * w[a0 + C * r + c];
      d = 2.0 * d / vv;
      for (int r = j; r < 9; ++r) w[a0 + C * r + c] -= d * w[a0 + C * r + j];
    }
  }
  for (int k = 0; k < 9 - C; ++k) {
    for (int r = 0; r < 9; ++r) w[n0 + 9 * k + r] = r == C + k ? 1.0 : 0.0;
    for (int j = C - 1; j >= 0; --j) {
      double d = 0.0;
      for (int r = j; r < 9; ++r) d += w[a0 + C * r + j] * w[n0 + 9 * k + r];
      d = 2.0 * d / w[hh0 + j];
      for (int r = j; r < 9; ++r) w[n0 + 9 * k + r] -= d * w[a0 + C * r + j];
    }
  }
  return true;
}

// the real roots of c[0] x^3 + c[1] x^2 + c[2] x + c[3] (c[0] != 0) under the rule of rel_pose_math.h: a root counts as real
// when |imag| <= kRpMaxRootImag (1 + |z|).  One real root in closed form (Cardano, or the trigonometric form), polished by
// Newton steps on the cubic; the other two from the deflated quadratic, each real one polished by two Newton steps.
__host__ __device__ inline int tv_cubic_real_roots(double c0, double c1, double c2, double c3, double& x0, double& x1, double& x2) {
  const double a = c1 / c0, b = c2 / c0, d = c3 / c0;
  if (!(isfinite(a) && isfinite(b) && isfinite(d))) return 0;
  const double p = b - a * a / 3.0, q = 2.0 * a * a * a / 27.0 - a * b / 3.0 + d;
  const double disc = q * q / 4.0 + p * p * p / 27.0;
  double t;
  if (disc > 0.0) {
    const double s = sqrt(disc);
    t = cbrt(-q / 2.0 + s) + cbrt(-q / 2.0 - s);
  } else if (p < 0.0) {
    const double m = 2.0 * sqrt(-p / 3.0);
    double arg = 3.0 * q / (p * m);
    arg = arg > 1.0 ? 1.0 : (arg < -1.0 ? -1.0 : arg);
    t = m * cos(acos(arg) / 3.0);
  } else {
    t = 0.0;  // p = q = 0: the triple root
  }
  double r = t - a / 3.0;
  auto newton = [&](double x, int steps) {
    for (int it = 0; it < steps; ++it) {
      const double f = ((x + a) * x + b) * x + d, df = (3.0 * x + 2.0 * a) * x + b;
      if (df == 0.0) break;
      const double step = f / df;
      if (!isfinite(step)) break;
      x -= step;
    }
    return x;
  };
  r = newton(r, 4);
  // (x - r)(x^2 + e x + g)
  const double e = a + r, g = b + r * e;
  const double dq = e * e - 4.0 * g;
  x0 = r;
  if (dq >= 0.0) {
    const double s = sqrt(dq);
    const double qq = e >= 0.0 ? -0.5 * (e + s) : -0.5 * (e - s);
    x1 = newton(qq, 2);
    x2 = newton(qq != 0.0 ? g / qq : 0.0, 2);
    return 3;
  }
  const double re = -0.5 * e, im = 0.5 * sqrt(-dq);
  if (im <= kRpMaxRootImag * (1.0 + sqrt(re * re + im * im))) {  // a conjugate pair that counts as real: its real part, twice
    x1 = x2 = newton(re, 2);
    return 3;
  }
  return 1;
}

// FundamentalMatrixSevenPointEstimator::Estimate on pixel coordinates (no normalisation): up to 3 canonical F in
// lexicographic order into out[3][9]; returns the count (0: rank < 7, or no finite cubic)
__host__ __device__ inline int tv_seven_point(const double u1[7], const double v1[7], const double u2[7], const double v2[7], RpW w, double* out) {
  for (int c = 0; c < 7; ++c) {
    double q[9];
    rp_q_row(u1[c], v1[c], u2[c], v2[c], q);
    for (int r = 0; r < 9; ++r) w[TVF_A + 7 * r + c] = q[r];
  }
  if (!tv_nullspace<7>(w, TVF_A, TVF_HH, TVF_N)) return 0;
  double F1[9], F2[9], D[9];
  for (int i = 0; i < 9; ++i) { F1[i] = w[TVF_N + i]; F2[i] = w[TVF_N + 9 + i]; D[i] = F1[i] - F2[i]; }
  // det(F2 + l D) = c3 l^3 + c2 l^2 + c1 l + c0 over the six permutations
  double cf[4] = {0.0, 0.0, 0.0, 0.0};
  const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  const double sgn[6] = {1.0, -1.0, -1.0, 1.0, 1.0, -1.0};
#pragma unroll
  for (int p = 0; p < 6; ++p) {
    const double a0 = F2[perm[p][0]], a1 = F2[3 + perm[p][1]], a2 = F2[6 + perm[p][2]];
    const double d0 = D[perm[p][0]], d1 = D[3 + perm[p][1]], d2 = D[6 + perm[p][2]];
    cf[3] += sgn[p] * (a0 * a1 * a2);
    cf[2] += sgn[p] * (d0 * a1 * a2 + a0 * d1 * a2 + a0 * a1 * d2);
    cf[1] += sgn[p] * (d0 * d1 * a2 + d0 * a1 * d2 + a0 * d1 * d2);
    cf[0] += sgn[p] * (d0 * d1 * d2);
  }
  if (!(isfinite(cf[0]) && isfinite(cf[1]) && isfinite(cf[2]) && isfinite(cf[3])) || cf[0] == 0.0) return 0;
  double l0 = 0.0, l1 = 0.0, l2 = 0.0;
  const int nr = tv_cubic_real_roots(cf[0], cf[1], cf[2], cf[3], l0, l1, l2);
  int nm = 0;
  auto emit = [&](double l) {
    double F[9];
    for (int i = 0; i < 9; ++i) F[i] = l * F1[i] + (1.0 - l) * F2[i];
    if (!rp_canonical(F)) return;
    int pos = nm;
    while (pos > 0 && rp_lex_less(F, out + 9 * (pos - 1))) {
      for (int i = 0; i < 9; ++i) out[9 * pos + i] = out[9 * (pos - 1) + i];
      --pos;
    }
    for (int i = 0; i < 9; ++i) out[9 * pos + i] = F[i];
    ++nm;
  };
  if (nr > 0) emit(l0);
  if (nr > 1) emit(l1);
  if (nr > 2) emit(l2);
  return nm;
}

// squared forward transfer error |x2 - pi(H x1)|^2; DBL_MAX when the third homogeneous coordinate is 0
__host__ __device__ inline double tv_h_residual(const double* H, double u1, double v1, double u2, double v2) {
  const double x = H[0] * u1 + H[1] * v1 + H[2], y = H[3] * u1 + H[4] * v1 + H[5], z = H[6] * u1 + H[7] * v1 + H[8];
  if (z == 0.0) return DBL_MAX;
  const double du = u2 - x / z, dv = v2 - y / z;
  return du * du + dv * dv;
}

// the two DLT rows of one match (x1 -> x2): [-x1 -y1 -1 0 0 0 x2x1 x2y1 x2], [0 0 0 -x1 -y1 -1 y2x1 y2y1 y2]
__host__ __device__ inline void tv_h_rows(double u1, double v1, double u2, double v2, double a[9], double b[9]) {
  a[0] = -u1; a[1] = -v1; a[2] = -1.0; a[3] = 0.0; a[4] = 0.0; a[5] = 0.0; a[6] = u2 * u1; a[7] = u2 * v1; a[8] = u2;
  b[0] = 0.0; b[1] = 0.0; b[2] = 0.0; b[3] = -u1; b[4] = -v1; b[5] = -1.0; b[6] = v2 * u1; b[7] = v2 * v1; b[8] = v2;
}

// true when a triple of the four points is collinear (sin of the angle at its first point <= kTvCollinearTol), coincident
// points included
__host__ __device__ inline bool tv_any_collinear4(const double x[4], const double y[4]) {
  const int tri[4][3] = {{0, 1, 2}, {0, 1, 3}, {0, 2, 3}, {1, 2, 3}};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double ax = x[tri[k][1]] - x[tri[k][0]], ay = y[tri[k][1]] - y[tri[k][0]];
    const double bx = x[tri[k][2]] - x[tri[k][0]], by = y[tri[k][2]] - y[tri[k][0]];
    const double cr = ax * by - ay * bx;
    const double den = sqrt((ax * ax + ay * ay) * (bx * bx + by * by));
    if (!(fabs(cr) > kTvCollinearTol * den)) return true;
  }
  return false;
}

// Hartley normalisation of m points from their centroid (cx, cy) and summed squared distance to it: the scale s with
// RMS distance sqrt(2); false when the points coincide
__host__ __device__ inline bool tv_hartley_scale(double sumsq, double m, double* s) {
  const double rms = sqrt(sumsq / m);
  if (!(rms > 0.0) || !isfinite(rms)) return false;
  *s = sqrt(2.0) / rms;
  return true;
}

// M = T2^T Fh T1 (fundamental) with T = [[s 0 -s cx] [0 s -s cy] [0 0 1]]
__host__ __device__ inline void tv_denormalise_f(const double Fh[9], double s1, double c1x, double c1y, double s2, double c2x, double c2y, double F[9]) {
  const double T1[9] = {s1, 0.0, -s1 * c1x, 0.0, s1, -s1 * c1y, 0.0, 0.0, 1.0};
  const double T2[9] = {s2, 0.0, -s2 * c2x, 0.0, s2, -s2 * c2y, 0.0, 0.0, 1.0};
  double A[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[3 * i + j] = T2[i] * Fh[j] + T2[3 + i] * Fh[3 + j] + T2[6 + i] * Fh[6 + j];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) F[3 * i + j] = A[3 * i] * T1[j] + A[3 * i + 1] * T1[3 + j] + A[3 * i + 2] * T1[6 + j];
}

// H = T2^-1 Hh T1 with T^-1 = [[1/s 0 cx] [0 1/s cy] [0 0 1]]
__host__ __device__ inline void tv_denormalise_h(const double Hh[9], double s1, double c1x, double c1y, double s2, double c2x, double c2y, double H[9]) {
  const double T1[9] = {s1, 0.0, -s1 * c1x, 0.0, s1, -s1 * c1y, 0.0, 0.0, 1.0};
  const double T2i[9] = {1.0 / s2, 0.0, c2x, 0.0, 1.0 / s2, c2y, 0.0, 0.0, 1.0};
  double A[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[3 * i + j] = T2i[3 * i] * Hh[j] + T2i[3 * i + 1] * Hh[3 + j] + T2i[3 * i + 2] * Hh[6 + j];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) H[3 * i + j] = A[3 * i] * T1[j] + A[3 * i + 1] * T1[3 + j] + A[3 * i + 2] * T1[6 + j];
}

// HomographyMatrixEstimator::Estimate on a minimal sample: normalised DLT, canonical form.  false: a collinear triple in
// either image, or rank < 8
__host__ __device__ inline bool tv_four_point(const double u1[4], const double v1[4], const double u2[4], const double v2[4], RpW w, double H[9]) {
  if (tv_any_collinear4(u1, v1) || tv_any_collinear4(u2, v2)) return false;
  const double c1x = (u1[0] + u1[1] + u1[2] + u1[3]) / 4.0, c1y = (v1[0] + v1[1] + v1[2] + v1[3]) / 4.0;
  const double c2x = (u2[0] + u2[1] + u2[2] + u2[3]) / 4.0, c2y = (v2[0] + v2[1] + v2[2] + v2[3]) / 4.0;
  double q1 = 0.0, q2 = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    q1 += (u1[k] - c1x) * (u1[k] - c1x) + (v1[k] - c1y) * (v1[k] - c1y);
    q2 += (u2[k] - c2x) * (u2[k] - c2x) + (v2[k] - c2y) * (v2[k] - c2y);
  }
  double s1, s2;
  if (!tv_hartley_scale(q1, 4.0, &s1) || !tv_hartley_scale(q2, 4.0, &s2)) return false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double a[9], b[9];
    tv_h_rows(s1 * (u1[k] - c1x), s1 * (v1[k] - c1y), s2 * (u2[k] - c2x), s2 * (v2[k] - c2y), a, b);
#pragma unroll
    for (int r = 0; r < 9; ++r) { w[TVH_A + 8 * r + 2 * k] = a[r]; w[TVH_A + 8 * r + 2 * k + 1] = b[r]; }
  }
  if (!tv_nullspace<8>(w, TVH_A, TVH_HH, TVH_N)) return false;
  double Hh[9];
  for (int i = 0; i < 9; ++i) Hh[i] = w[TVH_N + i];
  tv_denormalise_h(Hh, s1, c1x, c1y, s2, c2x, c2y, H);
  return rp_canonical(H);
}

// ---- host: the algebra after the local estimators' reductions -----------------------------------------------------------
// mom = {count, sum x1, sum y1, sum x2, sum y2} of the inliers; g = upper triangle (row-major, 45) of the Gram matrix of the
// design rows built from CENTRED coordinates (x - centroid): the epipolar rows rp_q_row (fundamental) or the two DLT rows
// tv_h_rows per match (homography).  A centred entry times its Hartley scales is the normalised entry, so the Gram matrix
// of the normalised design matrix is f_i f_j g_ij, and the summed squared distances are diagonal entries of g.
struct TvNorm { double s1, c1x, c1y, s2, c2x, c2y; };

inline bool tv_scaled_gram(const double mom[5], const double g[45], bool homography, double G[9][9], TvNorm* nm) {
  const double m = mom[0];
  double C[9][9];
  for (int r = 0, k = 0; r < 9; ++r)
    for (int c = r; c < 9; ++c, ++k) C[r][c] = C[c][r] = g[k];
  // fundamental rows: x2x1 x2y1 x2 y2x1 y2y1 y2 x1 y1 1; homography rows: -x1 -y1 -1 (0 0 0) x2x1 x2y1 x2 and (0 0 0) -x1 -y1 -1 y2x1 y2y1 y2
  const double q1 = homography ? C[0][0] + C[1][1] : C[6][6] + C[7][7];
  const double q2 = homography ? C[8][8] : C[2][2] + C[5][5];  // homography: both rows of a match add to column 8
  double s1, s2;
  if (!tv_hartley_scale(q1, m, &s1) || !tv_hartley_scale(q2, m, &s2)) return false;
  double f[9];
  if (homography) {
    const double ff[9] = {s1, s1, 1.0, s1, s1, 1.0, s1 * s2, s1 * s2, s2};
    for (int i = 0; i < 9; ++i) f[i] = ff[i];
  } else {
    const double ff[9] = {s2 * s1, s2 * s1, s2, s2 * s1, s2 * s1, s2, s1, s1, 1.0};
    for (int i = 0; i < 9; ++i) f[i] = ff[i];
  }
  for (int r = 0; r < 9; ++r)
    for (int c = 0; c < 9; ++c) G[r][c] = f[r] * f[c] * C[r][c];
  *nm = TvNorm{s1, mom[1] / m, mom[2] / m, s2, mom[3] / m, mom[4] / m};
  return true;
}

// FundamentalMatrixEightPointEstimator::Estimate from the reductions: false when fewer than 8 inliers, coincident points
// or a design matrix of rank < 8
inline bool tv_eight_point_from_gram(const double mom[5], const double g[45], double F[9]) {
  if (mom[0] < 8.0) return false;
  double G[9][9], V[9][9], ev[9];
  TvNorm nm;
  if (!tv_scaled_gram(mom, g, false, G, &nm)) return false;
  sym_eig<9>(G, V, ev);  // ascending
  if (!(ev[1] > kTvRankTol * kTvRankTol * ev[8])) return false;
  double Fh[9];
  for (int i = 0; i < 9; ++i) Fh[i] = V[i][0];
  // rank 2: zero the smallest singular value, Fh - (Fh v3) v3^T with v3 the eigenvector of Fh^T Fh of the smallest eigenvalue
  double A[3][3], W[3][3], e3[3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[i][j] = Fh[i] * Fh[j] + Fh[3 + i] * Fh[3 + j] + Fh[6 + i] * Fh[6 + j];
  sym_eig<3>(A, W, e3);
  const double v3[3] = {W[0][0], W[1][0], W[2][0]};
  for (int r = 0; r < 3; ++r) {
    const double fv = Fh[3 * r] * v3[0] + Fh[3 * r + 1] * v3[1] + Fh[3 * r + 2] * v3[2];
    for (int c = 0; c < 3; ++c) Fh[3 * r + c] -= fv * v3[c];
  }
  tv_denormalise_f(Fh, nm.s1, nm.c1x, nm.c1y, nm.s2, nm.c2x, nm.c2y, F);
  return rp_canonical(F);
}

// HomographyMatrixEstimator::Estimate from the reductions (non-minimal)
inline bool tv_homography_from_gram(const double mom[5], const double g[45], double H[9]) {
  if (mom[0] < 4.0) return false;
  double G[9][9], V[9][9], ev[9];
  TvNorm nm;
  if (!tv_scaled_gram(mom, g, true, G, &nm)) return false;
  sym_eig<9>(G, V, ev);
  if (!(ev[1] > kTvRankTol * kTvRankTol * ev[8])) return false;
  double Hh[9];
  for (int i = 0; i < 9; ++i) Hh[i] = V[i][0];
  tv_denormalise_h(Hh, nm.s1, nm.c1x, nm.c1y, nm.s2, nm.c2x, nm.c2y, H);
  return rp_canonical(H);
}

// ---- host: pose from a homography ---------------------------------------------------------------------------------------
inline void tv_mat3_mul(const double A[9], const double B[9], double C[9]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
inline double tv_det3(const double M[9]) {
  return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}
inline void tv_cross(const double a[3], const double b[3], double c[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

// DecomposeHomographyMatrix: Hn = K2^-1 H K1 scaled by its middle singular value with positive determinant, then either
// the single candidate (R = Hn, t = 0) when max |Hn^T Hn - I| < 1e-3, or the four (R, t) of Hn = R + t n^T.  The four are
// two rotations Ra, Rb (Ra first when its row-major entries compare lexicographically smaller) each with +-t; OUR order:
// (Ra, ta), (Rb, tb), (Ra, -ta), (Rb, -tb) with ta, tb signed so that the largest-magnitude component is positive (the
// first on ties).  Returns the number of candidates (1 or 4); *near_identity = max |Hn^T Hn - I|.
inline int tv_decompose_homography(const double H[9], const double K1[4], const double K2[4], double R[4][9], double t[4][3], double* near_identity) {
  // K2^-1 H K1 with PINHOLE K = [[fx 0 cx] [0 fy cy] [0 0 1]]
  const double K1m[9] = {K1[0], 0.0, K1[2], 0.0, K1[1], K1[3], 0.0, 0.0, 1.0};
  const double K2i[9] = {1.0 / K2[0], 0.0, -K2[2] / K2[0], 0.0, 1.0 / K2[1], -K2[3] / K2[1], 0.0, 0.0, 1.0};
  double A[9], Hn[9];
  tv_mat3_mul(K2i, H, A);
  tv_mat3_mul(A, K1m, Hn);
  double S[3][3], V[3][3], ev[3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) S[i][j] = Hn[i] * Hn[j] + Hn[3 + i] * Hn[3 + j] + Hn[6 + i] * Hn[6 + j];
  sym_eig<3>(S, V, ev);  // ascending eigenvalues of Hn^T Hn
  const double sc = sqrt(ev[1]);
  const double sg = tv_det3(Hn) < 0.0 ? -1.0 : 1.0;
  for (int i = 0; i < 9; ++i) Hn[i] = sg * Hn[i] / sc;
  double dev = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      S[i][j] = Hn[i] * Hn[j] + Hn[3 + i] * Hn[3 + j] + Hn[6 + i] * Hn[6 + j];
      dev = std::max(dev, fabs(S[i][j] - (i == j ? 1.0 : 0.0)));
    }
  *near_identity = dev;
  if (dev < 1e-3) {
    for (int i = 0; i < 9; ++i) R[0][i] = Hn[i];
    t[0][0] = t[0][1] = t[0][2] = 0.0;
    return 1;
  }
  sym_eig<3>(S, V, ev);
  // sigma_1^2 >= sigma_2^2 = 1 >= sigma_3^2 with eigenvectors v1, v2, v3 (right-handed)
  double v1[3] = {V[0][2], V[1][2], V[2][2]}, v2[3] = {V[0][1], V[1][1], V[2][1]}, v3[3];
  tv_cross(v1, v2, v3);
  const double l1 = ev[2], l3 = ev[0];
  const double a = sqrt(std::max(0.0, 1.0 - l3)), b = sqrt(std::max(0.0, l1 - 1.0)), den = sqrt(l1 - l3);
  double Rs[2][9], ts[2][3];
  for (int k = 0; k < 2; ++k) {
    const double sb = k == 0 ? 1.0 : -1.0;
    double u[3], U[9], Wm[9], hv2[3], hu[3], n[3], w3[3];
    for (int d = 0; d < 3; ++d) u[d] = (a * v1[d] + sb * b * v3[d]) / den;
    tv_cross(v2, u, n);
    for (int r = 0; r < 3; ++r) {
      hv2[r] = Hn[3 * r] * v2[0] + Hn[3 * r + 1] * v2[1] + Hn[3 * r + 2] * v2[2];
      hu[r] = Hn[3 * r] * u[0] + Hn[3 * r + 1] * u[1] + Hn[3 * r + 2] * u[2];
    }
    tv_cross(hv2, hu, w3);
    // R = W U^T with U = [v2 u n], W = [H v2, H u, H v2 x H u] as columns
    for (int r = 0; r < 3; ++r) { U[3 * r] = v2[r]; U[3 * r + 1] = u[r]; U[3 * r + 2] = n[r]; Wm[3 * r] = hv2[r]; Wm[3 * r + 1] = hu[r]; Wm[3 * r + 2] = w3[r]; }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) Rs[k][3 * i + j] = Wm[3 * i] * U[3 * j] + Wm[3 * i + 1] * U[3 * j + 1] + Wm[3 * i + 2] * U[3 * j + 2];
    for (int r = 0; r < 3; ++r)
      ts[k][r] = (Hn[3 * r] - Rs[k][3 * r]) * n[0] + (Hn[3 * r + 1] - Rs[k][3 * r + 1]) * n[1] + (Hn[3 * r + 2] - Rs[k][3 * r + 2]) * n[2];
    int im = 0;
    for (int d = 1; d < 3; ++d)
      if (fabs(ts[k][d]) > fabs(ts[k][im])) im = d;
    if (ts[k][im] < 0.0)
      for (int d = 0; d < 3; ++d) ts[k][d] = -ts[k][d];
  }
  const int first = rp_lex_less(Rs[1], Rs[0]) ? 1 : 0;
  for (int k = 0; k < 4; ++k) {
    const int src = (k % 2 == 0) ? first : 1 - first;
    const double sgn = k < 2 ? 1.0 : -1.0;
    for (int i = 0; i < 9; ++i) R[k][i] = Rs[src][i];
    for (int d = 0; d < 3; ++d) t[k][d] = sgn * ts[src][d];
  }
  return 4;
}

}  // namespace mpsfm
