// Stand-alone check of the host path of csrc/align3d_math.h: the 3-point solver on 1000 sampled triples (degenerate ones
// included), the line rule of the fit and the lift at the edges of a map.  Meant to be built with the host sanitizers and run on a
// CPU:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -x hip scripts/check_align3d_host.cpp -o check_align3d_host
//   ./check_align3d_host
//
// Buffers are exactly as long as the header says, so a read or write past them is the sanitizer's to report.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../mpsfm_amd/csrc/align3d_math.h"

using namespace mpsfm;

static int failures = 0;
#define EXPECT(what, cond)                                       \
  do {                                                           \
    if (!(cond)) { std::printf("FAILED: %s\n", what); ++failures; } \
  } while (0)

static uint64_t rng_state = 0x1234567ull;
static double uniform() {  // splitmix64 -> [0, 1)
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (double)((z ^ (z >> 31)) >> 11) / 9007199254740992.0;
}

static bool proper_rotation(const double* M) {
  double worst = 0.0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double d = 0.0;
      for (int k = 0; k < 3; ++k) d += M[4 * r + k] * M[4 * c + k];
      worst = std::fmax(worst, std::fabs(d - (r == c ? 1.0 : 0.0)));
    }
  const double det = M[0] * (M[5] * M[10] - M[6] * M[9]) - M[1] * (M[4] * M[10] - M[6] * M[8]) + M[2] * (M[4] * M[9] - M[5] * M[8]);
  return worst < 1e-12 && std::fabs(det - 1.0) < 1e-12;
}

int main() {
  // a known similarity: rotation about (1, 2, 2) / 3 by 1.1 rad, s = 1.7
  const double k[3] = {1.0 / 3, 2.0 / 3, 2.0 / 3}, ang = 1.1, s_true = 1.7, t_true[3] = {0.4, -1.2, 0.7};
  double R[3][3];
  const double K[3][3] = {{0, -k[2], k[1]}, {k[2], 0, -k[0]}, {-k[1], k[0], 0}};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double kk = 0.0;
      for (int j = 0; j < 3; ++j) kk += K[r][j] * K[j][c];
      R[r][c] = (r == c ? 1.0 : 0.0) + std::sin(ang) * K[r][c] + (1.0 - std::cos(ang)) * kk;
    }
  const int n = 200;
  std::vector<double> src(3 * n), tgt(3 * n);
  for (int i = 0; i < n; ++i) {
    for (int d = 0; d < 3; ++d) src[3 * i + d] = -2.0 + 4.0 * uniform();
    if (i % 10 == 0 && i > 0)  // every tenth point lies on the line through points 0 and 1: collinear samples occur
      for (int d = 0; d < 3; ++d) src[3 * i + d] = src[d] + (double)i * (src[3 + d] - src[d]);
    for (int r = 0; r < 3; ++r) tgt[3 * i + r] = s_true * (R[r][0] * src[3 * i] + R[r][1] * src[3 * i + 1] + R[r][2] * src[3 * i + 2]) + t_true[r];
  }
  int refused = 0, solved = 0;
  for (int trial = 0; trial < 1000; ++trial) {
    int idx[3];
    for (int j = 0; j < 3; ++j) idx[j] = trial % 4 == 0 ? 10 * (int)(uniform() * (n / 10)) : (int)(uniform() * n);  // repeats are kept: coincident points
    double P[3][3], Q[3][3], M[kA3Model];
    for (int j = 0; j < 3; ++j)
      for (int d = 0; d < 3; ++d) { P[j][d] = src[3 * idx[j] + d]; Q[j][d] = tgt[3 * idx[j] + d]; }
    for (int with_scale = 0; with_scale < 2; ++with_scale) {
      if (!a3_minimal(P, Q, with_scale, M)) { ++refused; continue; }
      ++solved;
      EXPECT("a model is a proper rotation", proper_rotation(M));
      EXPECT("the scale is finite and positive", std::isfinite(M[12]) && M[12] > 0.0 && (with_scale || M[12] == 1.0));
      if (with_scale) {
        EXPECT("a noise-free sample recovers the scale", std::fabs(M[12] - s_true) < 1e-6);
        for (int j = 0; j < 3; ++j) EXPECT("a noise-free sample explains itself", a3_residual(M, P[j][0], P[j][1], P[j][2], Q[j][0], Q[j][1], Q[j][2]) < 1e-12);
      }
    }
  }
  EXPECT("degenerate and regular samples both occurred", refused > 100 && solved > 1000);
  const double coincident[3][3] = {{1, 2, 3}, {1, 2, 3}, {1, 2, 3}}, tri[3][3] = {{0, 0, 1}, {1, 0, 1}, {0, 1, 2}};
  double M[kA3Model];
  EXPECT("coincident source points give no model", !a3_minimal(coincident, tri, 1, M));
  EXPECT("coincident target points give no model", !a3_minimal(tri, coincident, 0, M));
  const double line_sc[6] = {4.0, 2.0, 0.0, 1.0, 0.0, 0.0}, plane_sc[6] = {4.0, 0.0, 0.0, 1.0, 0.0, 0.0}, zero_sc[6] = {0, 0, 0, 0, 0, 0};
  EXPECT("points on a line are refused", a3_scatter_is_line(line_sc));
  EXPECT("a planar set is fine", !a3_scatter_is_line(plane_sc));
  EXPECT("coincident points are refused", a3_scatter_is_line(zero_sc));

  // the lift on a 5 x 4 map: the last valid cell, the borders, the holes
  const int H = 5, W = 4;
  const double kNaN = std::numeric_limits<double>::quiet_NaN(), kInf = std::numeric_limits<double>::infinity();
  const double intr[4] = {3.6, 3.4, 1.7, 2.7};
  std::vector<double> depth(H * W);
  for (double& z : depth) z = 0.5 + 8.5 * uniform();
  double xyz[3];
  EXPECT("the origin is valid", a3_lift(depth.data(), H, W, intr, 0.0, 0.0, xyz) && xyz[2] == depth[0]);
  EXPECT("just inside the last column is valid", a3_lift(depth.data(), H, W, intr, W - 1 - 1e-12, H - 1 - 1e-12, xyz));
  EXPECT("the last column is not", !a3_lift(depth.data(), H, W, intr, W - 1.0, 1.0, xyz) && xyz[0] == 0.0 && xyz[1] == 0.0 && xyz[2] == 0.0);
  EXPECT("the last row is not", !a3_lift(depth.data(), H, W, intr, 1.0, H - 1.0, xyz));
  EXPECT("left of the map is not", !a3_lift(depth.data(), H, W, intr, -1e-9, 1.0, xyz));
  for (double far : {1e9, 1e300, kInf, kNaN, -kInf}) EXPECT("far outside is not", !a3_lift(depth.data(), H, W, intr, far, 1.0, xyz) && !a3_lift(depth.data(), H, W, intr, 1.0, far, xyz));
  for (double hole : {0.0, -1.0, kNaN, kInf})
    for (int corner = 0; corner < 4; ++corner) {
      std::vector<double> d = depth;
      d[(1 + corner / 2) * W + 2 + corner % 2] = hole;
      EXPECT("a hole at a corner is not valid", !a3_lift(d.data(), H, W, intr, 2.5, 1.5, xyz) && xyz[2] == 0.0);
      EXPECT("a hole elsewhere does not matter", a3_lift(d.data(), H, W, intr, 0.5, 3.5, xyz));
    }
  std::printf("%d models, %d refusals, %d failures\n", solved, refused, failures);
  return failures ? 1 : 0;
}
