// Constant-size arithmetic of the relative-pose estimator (rel_pose.hip): the squared Sampson error, the five-point
// solver (nullspace -> 10 x 20 cubic constraints -> Gauss-Jordan -> degree-10 polynomial -> real roots -> canonical
// essential matrices in lexicographic order) and the
// essential-matrix decomposition.  COLMAP 3.11 semantics of EssentialMatrixFivePointEstimator / ComputeSquaredSampsonError /
// DecomposeEssentialMatrix / PoseFromEssentialMatrix as recalled (include/mpsfm_hip.h, mpsfm_rel_pose_estimate): parity with
// the reference's COLMAP fork unpinned.
//
// The solver keeps every runtime-indexed array in a caller-provided work area RpW (RP_WORK doubles, element i at p[i * s]):
// on the device a per-thread slice of LDS (stride = threads of the block, so lanes hit different banks), on the host a
// local array with stride 1.  Nothing runtime-indexed lives in registers, so the kernel needs no scratch.
#pragma once
#include "abs_pose_math.h"
#include "common.h"

// no contraction into fused multiply-adds: every expression rounds as written (as in abs_pose_math.h)
#pragma clang fp contract(off)

namespace mpsfm {

constexpr int kRpSample = 5;
constexpr int kRpMaxModels = 10;
constexpr double kRpMaxRootImag = 1e-10;  // relative to 1 + |z|
constexpr double kRpRankTol = 1e-12;      // fifth singular value (or |R_jj|) / ||Q||: a larger nullspace gives no model

// work-area layout (doubles)
constexpr int RP_N = 0;      // nullspace basis N[4][9]
constexpr int RP_A = 36;     // A[10][20]; before it: Q^T [9][5] and Householder scalars; after elimination: AA[10][10]
constexpr int RP_HH = 36 + 45;
constexpr int RP_B = 136;    // B(z) [3][3][5] coefficients, highest power first
constexpr int RP_DET = 181;  // degree-10 polynomial, 11 coefficients, highest power first
constexpr int RP_Z = 192;    // 10 complex roots (re, im)
constexpr int RP_WORK = 236;

struct RpW {
  double* p;
  int s;
  __host__ __device__ double& operator[](int i) const { return p[(size_t)i * s]; }
};

// ComputeSquaredSampsonError of x2^T E x1 (E row-major, normalised points)
__host__ __device__ inline double rp_sampson(const double* E, double u1, double v1, double u2, double v2) {
  const double a0 = E[0] * u1 + E[1] * v1 + E[2];
  const double a1 = E[3] * u1 + E[4] * v1 + E[5];
  const double a2 = E[6] * u1 + E[7] * v1 + E[8];
  const double b0 = E[0] * u2 + E[3] * v2 + E[6];
  const double b1 = E[1] * u2 + E[4] * v2 + E[7];
  const double c = u2 * a0 + v2 * a1 + a2;
  return c * c / (a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1);
}

// row of the epipolar matrix Q for one match: q[3 i + j] = x2_i x1_j
__host__ __device__ inline void rp_q_row(double u1, double v1, double u2, double v2, double q[9]) {
  q[0] = u2 * u1; q[1] = u2 * v1; q[2] = u2;
  q[3] = v2 * u1; q[4] = v2 * v1; q[5] = v2;
  q[6] = u1; q[7] = v1; q[8] = 1.0;
}

// nullspace of the 5 x 9 Q of a minimal sample by Householder QR of Q^T; N rows = H e_5 .. H e_8.  false: rank < 5
__host__ __device__ inline bool rp_nullspace5(const double u1[5], const double v1[5], const double u2[5], const double v2[5], RpW w) {
  double fro = 0.0;
  for (int c = 0; c < 5; ++c) {
    double q[9];
    rp_q_row(u1[c], v1[c], u2[c], v2[c], q);
    for (int r = 0; r < 9; ++r) { w[RP_A + 5 * r + c] = q[r]; fro += q[r] * q[r]; }
  }
  fro = sqrt(fro);
  for (int j = 0; j < 5; ++j) {
    double nrm = 0.0;
    for (int r = j; r < 9; ++r) nrm += w[RP_A + 5 * r + j] * w[RP_A + 5 * r + j];
    nrm = sqrt(nrm);
    if (!(nrm > kRpRankTol * fro)) return false;
    const double alpha = w[RP_A + 5 * j + j] > 0 ? -nrm : nrm;
    w[RP_A + 5 * j + j] -= alpha;  // column j (rows j..8) now holds the Householder vector
    double vv = 0.0;
    for (int r = j; r < 9; ++r) vv += w[RP_A + 5 * r + j] * w[RP_A + 5 * r + j];
    w[RP_HH + j] = vv;
    for (int c = j + 1; c < 5; ++c) {
      double d = 0.0;
      for (int r = j; r < 9; ++r) d += w[RP_A + 5 * r + j] * w[RP_A + 5 * r + c];
      d = 2.0 * d / vv;
      for (int r = j; r < 9; ++r) w[RP_A + 5 * r + c] -= d * w[RP_A + 5 * r + j];
    }
  }
  for (int k = 0; k < 4; ++k) {
    for (int r = 0; r < 9; ++r) w[RP_N + 9 * k + r] = r == 5 + k ? 1.0 : 0.0;
    for (int j = 4; j >= 0; --j) {
      double d = 0.0;
      for (int r = j; r < 9; ++r) d += w[RP_A + 5 * r + j] * w[RP_N + 9 * k + r];
      d = 2.0 * d / w[RP_HH + j];
      for (int r = j; r < 9; ++r) w[RP_N + 9 * k + r] -= d * w[RP_A + 5 * r + j];
    }
  }
  return true;
}

// column of monomial x^ex y^ey z^ez (ex + ey + ez = 3 from three linear factors; the 4th "variable" is the constant 1) in
// the order of the 10 x 20 system: x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
__host__ __device__ inline int rp_monomial(int ex, int ey, int ez) {
  const int key = 16 * ex + 4 * ey + ez;
  switch (key) {
    case 48: return 0;  case 12: return 1;  case 36: return 2;  case 24: return 3;  case 33: return 4;
    case 32: return 5;  case 9: return 6;   case 8: return 7;   case 21: return 8;  case 20: return 9;
    case 18: return 10; case 17: return 11; case 16: return 12; case 6: return 13;  case 5: return 14;
    case 4: return 15;  case 3: return 16;  case 2: return 17;  case 1: return 18;  default: return 19;
  }
}

// adds s * E_a E_b E_c (three linear polynomials of E = x N0 + y N1 + z N2 + N3, entries a, b, c) to row r of A
__host__ __device__ inline void rp_add_triple(RpW w, int r, double s, int a, int b, int c) {
  for (int i = 0; i < 4; ++i) {
    const double ci = s * w[RP_N + 9 * i + a];
    for (int j = 0; j < 4; ++j) {
      const double cij = ci * w[RP_N + 9 * j + b];
      for (int k = 0; k < 4; ++k) {
        const int ex = (i == 0) + (j == 0) + (k == 0), ey = (i == 1) + (j == 1) + (k == 1), ez = (i == 2) + (j == 2) + (k == 2);
        w[RP_A + 20 * r + rp_monomial(ex, ey, ez)] += cij * w[RP_N + 9 * k + c];
      }
    }
  }
}

// the 10 x 20 system: row 0 det(E) = 0, rows 1 + 3 i + j: (2 E E^T E - tr(E E^T) E)_ij = 0
__host__ __device__ inline void rp_constraints(RpW w) {
  for (int i = 0; i < 200; ++i) w[RP_A + i] = 0.0;
  const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  const double sgn[6] = {1.0, -1.0, -1.0, 1.0, 1.0, -1.0};
  for (int p = 0; p < 6; ++p) rp_add_triple(w, 0, sgn[p], perm[p][0], 3 + perm[p][1], 6 + perm[p][2]);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const int r = 1 + 3 * i + j;
      for (int k = 0; k < 3; ++k)
        for (int l = 0; l < 3; ++l) {
          rp_add_triple(w, r, 2.0, 3 * i + l, 3 * k + l, 3 * k + j);  // 2 E_il E_kl E_kj
          rp_add_triple(w, r, -1.0, 3 * k + l, 3 * k + l, 3 * i + j);  // - E_kl E_kl E_ij
        }
    }
}

// Gauss-Jordan with partial pivoting on the left 10 x 10 block; AA = A_left^-1 A_right compacted to RP_A [10][10]
__host__ __device__ inline bool rp_eliminate(RpW w) {
  for (int k = 0; k < 10; ++k) {
    int p = k;
    double best = fabs(w[RP_A + 20 * k + k]);
    for (int r = k + 1; r < 10; ++r)
      if (fabs(w[RP_A + 20 * r + k]) > best) { best = fabs(w[RP_A + 20 * r + k]); p = r; }
    if (!(best > 0.0) || !isfinite(best)) return false;
    if (p != k)
      for (int c = k; c < 20; ++c) { const double t = w[RP_A + 20 * k + c]; w[RP_A + 20 * k + c] = w[RP_A + 20 * p + c]; w[RP_A + 20 * p + c] = t; }
    const double piv = w[RP_A + 20 * k + k];
    for (int c = k; c < 20; ++c) w[RP_A + 20 * k + c] /= piv;
    for (int r = 0; r < 10; ++r) {
      if (r == k) continue;
      const double f = w[RP_A + 20 * r + k];
      if (f == 0.0) continue;
      for (int c = k; c < 20; ++c) w[RP_A + 20 * r + c] -= f * w[RP_A + 20 * k + c];
    }
  }
  for (int r = 0; r < 10; ++r)  // compaction in increasing order: a destination never precedes an unread source
    for (int c = 0; c < 10; ++c) w[RP_A + 10 * r + c] = w[RP_A + 20 * r + 10 + c];
  for (int i = 0; i < 100; ++i)
    if (!isfinite(w[RP_A + i])) return false;
  return true;
}

// B(z) rows k = e - z f, l = g - z h, m = i - z j (leading monomials x^2z, x^2, y^2z, y^2, xyz, xy = AA rows 4..9) and its
// determinant, the degree-10 polynomial
__host__ __device__ inline void rp_det_poly(RpW w) {
  for (int r = 0; r < 3; ++r) {
    const int e = RP_A + 10 * (4 + 2 * r), f = e + 10;
    const int b = RP_B + 15 * r;
    w[b + 0] = 0.0; w[b + 1] = -w[f + 0]; w[b + 2] = w[e + 0] - w[f + 1]; w[b + 3] = w[e + 1] - w[f + 2]; w[b + 4] = w[e + 2];
    w[b + 5] = 0.0; w[b + 6] = -w[f + 3]; w[b + 7] = w[e + 3] - w[f + 4]; w[b + 8] = w[e + 4] - w[f + 5]; w[b + 9] = w[e + 5];
    w[b + 10] = -w[f + 6]; w[b + 11] = w[e + 6] - w[f + 7]; w[b + 12] = w[e + 7] - w[f + 8]; w[b + 13] = w[e + 8] - w[f + 9];
    w[b + 14] = w[e + 9];
  }
  for (int i = 0; i < 11; ++i) w[RP_DET + i] = 0.0;
  const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  const double sgn[6] = {1.0, -1.0, -1.0, 1.0, 1.0, -1.0};
  for (int p = 0; p < 6; ++p) {
    const int b0 = RP_B + 5 * perm[p][0], b1 = RP_B + 15 + 5 * perm[p][1], b2 = RP_B + 30 + 5 * perm[p][2];
    // degree-12 product of the padded quartics; its two leading coefficients are exactly zero
    for (int d = 2; d < 13; ++d) {
      double acc = 0.0;
      for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 5; ++j) {
          const int k = d - i - j;
          if (k < 0 || k > 4) continue;
          acc += w[b0 + i] * w[b1 + j] * w[b2 + k];
        }
      w[RP_DET + d - 2] += sgn[p] * acc;
    }
  }
}

// the ten complex roots of the degree-10 polynomial at RP_DET (leading coefficient non-zero) into RP_Z: Aberth-Ehrlich
// iteration, then two Newton steps
__host__ __device__ inline void rp_roots(RpW w) {
  const double c0 = w[RP_DET];
  double r0 = pow(fabs(w[RP_DET + 10] / c0), 0.1);  // geometric mean of the root magnitudes
  if (!(r0 > 0.0) || !isfinite(r0)) r0 = 1.0;
  for (int k = 0; k < 10; ++k) {
    const double ang = 0.4 + 0.6283185307179586 * k;
    w[RP_Z + 2 * k] = r0 * cos(ang);
    w[RP_Z + 2 * k + 1] = r0 * sin(ang);
  }
  auto eval = [&](ApCplx x, ApCplx& p, ApCplx& dp) {
    p = {1.0, 0.0}; dp = {0.0, 0.0};
    for (int i = 1; i < 11; ++i) { dp = ap_cadd(ap_cmul(dp, x), p); p = ap_cadd(ap_cmul(p, x), {w[RP_DET + i] / c0, 0.0}); }
  };
  for (int it = 0; it < 200; ++it) {
    double moved = 0.0;
    for (int k = 0; k < 10; ++k) {
      const ApCplx zk = {w[RP_Z + 2 * k], w[RP_Z + 2 * k + 1]};
      ApCplx p, dp;
      eval(zk, p, dp);
      if (p.re == 0.0 && p.im == 0.0) continue;
      const ApCplx ratio = ap_cdiv(p, dp);
      ApCplx sum = {0.0, 0.0};
      for (int j = 0; j < 10; ++j)
        if (j != k) sum = ap_cadd(sum, ap_cdiv({1.0, 0.0}, ap_csub(zk, {w[RP_Z + 2 * j], w[RP_Z + 2 * j + 1]})));
      const ApCplx step = ap_cdiv(ratio, ap_csub({1.0, 0.0}, ap_cmul(ratio, sum)));
      if (!(isfinite(step.re) && isfinite(step.im))) continue;
      const ApCplx zn = ap_csub(zk, step);
      w[RP_Z + 2 * k] = zn.re;
      w[RP_Z + 2 * k + 1] = zn.im;
      moved = fmax(moved, sqrt(step.re * step.re + step.im * step.im) / (1.0 + sqrt(zn.re * zn.re + zn.im * zn.im)));
    }
    if (moved < 1e-14) break;  // rounding keeps steps near 1e-16: the Newton steps and rp_polish finish the roots
  }
  for (int k = 0; k < 10; ++k) {
    ApCplx z = {w[RP_Z + 2 * k], w[RP_Z + 2 * k + 1]};
    for (int it = 0; it < 2; ++it) {
      ApCplx p, dp;
      eval(z, p, dp);
      if (dp.re == 0.0 && dp.im == 0.0) break;
      const ApCplx step = ap_cdiv(p, dp);
      if (!(isfinite(step.re) && isfinite(step.im))) break;
      z = ap_csub(z, step);
    }
    w[RP_Z + 2 * k] = z.re;
    w[RP_Z + 2 * k + 1] = z.im;
  }
}

// E / ||E||_F with its largest-magnitude entry positive (the first in row-major order on ties); false if E is 0 or not finite
__host__ __device__ inline bool rp_canonical(double E[9]) {
  double s = 0.0;
  for (int i = 0; i < 9; ++i) s += E[i] * E[i];
  s = sqrt(s);
  if (!(s > 0.0) || !isfinite(s)) return false;
  int im = 0;
  for (int i = 0; i < 9; ++i) {
    E[i] /= s;
    if (fabs(E[i]) > fabs(E[im])) im = i;
  }
  if (E[im] < 0)
    for (int i = 0; i < 9; ++i) E[i] = -E[i];
  return true;
}

__host__ __device__ inline bool rp_lex_less(const double* a, const double* b) {
  for (int i = 0; i < 9; ++i)
    if (a[i] != b[i]) return a[i] < b[i];
  return false;
}

// the ten constraints f(p) = [det E; 2 E E^T E - tr(E E^T) E] at E = x N0 + y N1 + z N2 + N3 and their Jacobian J[10][3]
__host__ __device__ inline void rp_constraint_eval(RpW w, const double p[3], double f[10], double J[10][3]) {
  double E[9];
  for (int i = 0; i < 9; ++i) E[i] = p[0] * w[RP_N + i] + p[1] * w[RP_N + 9 + i] + p[2] * w[RP_N + 18 + i] + w[RP_N + 27 + i];
  double C[9];  // cofactors
  C[0] = E[4] * E[8] - E[5] * E[7]; C[1] = E[5] * E[6] - E[3] * E[8]; C[2] = E[3] * E[7] - E[4] * E[6];
  C[3] = E[2] * E[7] - E[1] * E[8]; C[4] = E[0] * E[8] - E[2] * E[6]; C[5] = E[1] * E[6] - E[0] * E[7];
  C[6] = E[1] * E[5] - E[2] * E[4]; C[7] = E[2] * E[3] - E[0] * E[5]; C[8] = E[0] * E[4] - E[1] * E[3];
  f[0] = E[0] * C[0] + E[1] * C[1] + E[2] * C[2];
  double EEt[9], tr = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) EEt[3 * i + j] = E[3 * i] * E[3 * j] + E[3 * i + 1] * E[3 * j + 1] + E[3 * i + 2] * E[3 * j + 2];
  tr = EEt[0] + EEt[4] + EEt[8];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      f[1 + 3 * i + j] = 2.0 * (EEt[3 * i] * E[j] + EEt[3 * i + 1] * E[3 + j] + EEt[3 * i + 2] * E[6 + j]) - tr * E[3 * i + j];
  for (int k = 0; k < 3; ++k) {
    double D[9];
    for (int i = 0; i < 9; ++i) D[i] = w[RP_N + 9 * k + i];
    double dtr = 0.0, ddet = 0.0;
    for (int i = 0; i < 9; ++i) { dtr += 2.0 * E[i] * D[i]; ddet += C[i] * D[i]; }
    J[0][k] = ddet;
    double DEt[9], EDt[9];  // D E^T and E D^T
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        DEt[3 * i + j] = D[3 * i] * E[3 * j] + D[3 * i + 1] * E[3 * j + 1] + D[3 * i + 2] * E[3 * j + 2];
        EDt[3 * i + j] = E[3 * i] * D[3 * j] + E[3 * i + 1] * D[3 * j + 1] + E[3 * i + 2] * D[3 * j + 2];
      }
    // dG = 2 ((D E^T + E D^T) E + E E^T D) - dtr E - tr D
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double s = 0.0;
        for (int l = 0; l < 3; ++l) s += (DEt[3 * i + l] + EDt[3 * i + l]) * E[3 * l + j] + EEt[3 * i + l] * D[3 * l + j];
        J[1 + 3 * i + j][k] = 2.0 * s - dtr * E[3 * i + j] - tr * D[3 * i + j];
      }
  }
}

// three Gauss-Newton steps on the ten constraints (normal equations, Cramer's rule); a step that is not finite is skipped
__host__ __device__ inline void rp_polish(RpW w, double p[3]) {
  for (int it = 0; it < 3; ++it) {
    double f[10], J[10][3];
    rp_constraint_eval(w, p, f, J);
    double M[3][3], g[3];
    for (int a = 0; a < 3; ++a) {
      g[a] = 0.0;
      for (int r = 0; r < 10; ++r) g[a] += J[r][a] * f[r];
      for (int b = 0; b < 3; ++b) {
        M[a][b] = 0.0;
        for (int r = 0; r < 10; ++r) M[a][b] += J[r][a] * J[r][b];
      }
    }
    const double c00 = M[1][1] * M[2][2] - M[1][2] * M[2][1], c01 = M[1][2] * M[2][0] - M[1][0] * M[2][2], c02 = M[1][0] * M[2][1] - M[1][1] * M[2][0];
    const double det = M[0][0] * c00 + M[0][1] * c01 + M[0][2] * c02;
    if (!(det != 0.0) || !isfinite(det)) return;
    double d[3];
    d[0] = -(g[0] * c00 + g[1] * (M[0][2] * M[2][1] - M[0][1] * M[2][2]) + g[2] * (M[0][1] * M[1][2] - M[0][2] * M[1][1])) / det;
    d[1] = -(g[0] * c01 + g[1] * (M[0][0] * M[2][2] - M[0][2] * M[2][0]) + g[2] * (M[0][2] * M[1][0] - M[0][0] * M[1][2])) / det;
    d[2] = -(g[0] * c02 + g[1] * (M[0][1] * M[2][0] - M[0][0] * M[2][1]) + g[2] * (M[0][0] * M[1][1] - M[0][1] * M[1][0])) / det;
    if (!(isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]))) return;
    for (int a = 0; a < 3; ++a) p[a] += d[a];
  }
}

// the canonical essential matrices of the nullspace at RP_N into out[10][9], lexicographically ascending; returns the count
__host__ __device__ inline int rp_models_from_nullspace(RpW w, double* out) {
  rp_constraints(w);
  if (!rp_eliminate(w)) return 0;
  rp_det_poly(w);
  for (int i = 0; i < 11; ++i)
    if (!isfinite(w[RP_DET + i])) return 0;
  if (w[RP_DET] == 0.0) return 0;
  rp_roots(w);
  int nm = 0;
  for (int k = 0; k < 10; ++k) {
    const double z = w[RP_Z + 2 * k], zi = w[RP_Z + 2 * k + 1];
    if (!(fabs(zi) <= kRpMaxRootImag * (1.0 + sqrt(z * z + zi * zi)))) continue;
    double B[3][3];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        const int b = RP_B + 15 * r + 5 * c;
        double v = w[b];
        for (int d = 1; d < 5; ++d) v = v * z + w[b + d];
        B[r][c] = v;
      }
    // the null vector of B(z): the largest of the three row cross products
    double v[3] = {0.0, 0.0, 0.0}, bestn = -1.0;
    for (int pr = 0; pr < 3; ++pr) {
      const double* a = B[pr == 2 ? 1 : 0];
      const double* b = B[pr == 0 ? 1 : 2];
      const double cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2], cz = a[0] * b[1] - a[1] * b[0];
      const double nn = cx * cx + cy * cy + cz * cz;
      if (nn > bestn) { bestn = nn; v[0] = cx; v[1] = cy; v[2] = cz; }
    }
    if (v[2] == 0.0) continue;
    double pz[3] = {v[0] / v[2], v[1] / v[2], z};
    rp_polish(w, pz);
    double E[9];
    for (int i = 0; i < 9; ++i) E[i] = pz[0] * w[RP_N + i] + pz[1] * w[RP_N + 9 + i] + pz[2] * w[RP_N + 18 + i] + w[RP_N + 27 + i];
    if (!rp_canonical(E)) continue;
    // insertion into the sorted list
    int pos = nm;
    while (pos > 0 && rp_lex_less(E, out + 9 * (pos - 1))) {
      for (int i = 0; i < 9; ++i) out[9 * pos + i] = out[9 * (pos - 1) + i];
      --pos;
    }
    for (int i = 0; i < 9; ++i) out[9 * pos + i] = E[i];
    ++nm;
  }
  return nm;
}

// DecomposeEssentialMatrix (host): R1 = U W V^T, R2 = U W^T V^T, t = U[:, 2] with det U = det V = +1 and t's
// largest-magnitude component positive (first on ties).  V from the Jacobi eigenvectors of E^T E, U from E V.
inline void rp_decompose(const double E[9], double R1[9], double R2[9], double t[3]) {
  double A[3][3], V[3][3], ev[3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[i][j] = E[i] * E[j] + E[3 + i] * E[3 + j] + E[6 + i] * E[6 + j];
  sym_eig<3>(A, V, ev);  // ascending: column 2 = largest
  double v[3][3];           // v[c] = column c of V in descending singular-value order
  for (int c = 0; c < 3; ++c)
    for (int d = 0; d < 3; ++d) v[c][d] = V[d][2 - c];
  const double detv = v[0][0] * (v[1][1] * v[2][2] - v[1][2] * v[2][1]) - v[1][0] * (v[0][1] * v[2][2] - v[0][2] * v[2][1]) +
                      v[2][0] * (v[0][1] * v[1][2] - v[0][2] * v[1][1]);
  if (detv < 0)
    for (int d = 0; d < 3; ++d) v[2][d] = -v[2][d];
  double u[3][3];
  for (int c = 0; c < 2; ++c) {
    double s = 0.0;
    for (int r = 0; r < 3; ++r) {
      u[c][r] = E[3 * r] * v[c][0] + E[3 * r + 1] * v[c][1] + E[3 * r + 2] * v[c][2];
      s += u[c][r] * u[c][r];
    }
    s = sqrt(s);
    for (int r = 0; r < 3; ++r) u[c][r] /= s;
  }
  u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
  u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
  u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
  int im = 0;
  for (int d = 1; d < 3; ++d)
    if (fabs(u[2][d]) > fabs(u[2][im])) im = d;
  if (u[2][im] < 0)  // D = diag(-1, 1, -1) on both sides: the same E, R1 and R2 swapped, t negated
    for (int d = 0; d < 3; ++d) { u[0][d] = -u[0][d]; u[2][d] = -u[2][d]; v[0][d] = -v[0][d]; v[2][d] = -v[2][d]; }
  // U W = [-u1, u0, u2] and U W^T = [u1, -u0, u2] as columns
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      R1[3 * i + j] = -u[1][i] * v[0][j] + u[0][i] * v[1][j] + u[2][i] * v[2][j];
      R2[3 * i + j] = u[1][i] * v[0][j] - u[0][i] * v[1][j] + u[2][i] * v[2][j];
    }
  const double tn = sqrt(u[2][0] * u[2][0] + u[2][1] * u[2][1] + u[2][2] * u[2][2]);
  for (int d = 0; d < 3; ++d) t[d] = u[2][d] / tn;
}

}  // namespace mpsfm
