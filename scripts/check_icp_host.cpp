// Stand-alone check of the host path of the dense ICP: csrc/icp_math.h's scale-factor-solve-update on 1000 random SPD systems and on
// rank-deficient ones, the pose update on both sides of the small-angle switch, the normal and the association at the edges of
// maps held in buffers of exactly H W entries, and the argument checks of the entry points of csrc/depth_icp.hip, which return
// before any HIP call.  Meant to be built with the host sanitizers and run on a CPU:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         scripts/check_icp_host.cpp mpsfm_amd/csrc/depth_icp.hip mpsfm_amd/csrc/align3d.hip mpsfm_amd/csrc/dev_resources.hip \
//         -o check_icp_host
//   ./check_icp_host
//
// Buffers are exactly as long as the header says, so a read or write past them is the sanitizer's to report.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/mpsfm_hip.h"
#include "../mpsfm_amd/csrc/host_parts.h"
#include "../mpsfm_amd/csrc/icp_math.h"

using namespace mpsfm;

// the host thread pool (build_host.hip) is not linked: the hooks dev_resources.hip's staged uploads ask for, never reached here
namespace mpsfm {
int host_threads() { return 1; }
bool host_pool_enabled() { return false; }
HostPool* host_pool() { return nullptr; }
}  // namespace mpsfm

static int failures = 0;
#define EXPECT(what, cond)                                       \
  do {                                                           \
    if (!(cond)) { std::printf("FAILED: %s\n", what); ++failures; } \
  } while (0)

static uint64_t rng_state = 0x9876543ull;
static double uniform() {  // splitmix64 -> [0, 1)
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (double)((z ^ (z >> 31)) >> 11) / 9007199254740992.0;
}

// A = sum of n rows J J^T with column scales over four decades; dependent: column 4 = column 1 - 2 column 3
static void random_system(int n, bool dependent, double* A, double* b) {
  double scale[6];
  for (double& s : scale) s = std::pow(10.0, -2.0 + 4.0 * uniform());
  std::memset(A, 0, sizeof(double) * 36);
  for (int r = 0; r < n; ++r) {
    double J[6];
    for (int k = 0; k < 6; ++k) J[k] = (2.0 * uniform() - 1.0) * scale[k];
    if (dependent) J[4] = J[1] - 2.0 * J[3];
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j < 6; ++j) A[6 * i + j] += J[i] * J[j];
  }
  for (int k = 0; k < 6; ++k) b[k] = (2.0 * uniform() - 1.0) * scale[k];
}

static bool proper_rotation(const double* T, double tol) {
  double worst = 0.0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double d = 0.0;
      for (int k = 0; k < 3; ++k) d += T[4 * r + k] * T[4 * c + k];
      worst = std::fmax(worst, std::fabs(d - (r == c ? 1.0 : 0.0)));
    }
  return worst < tol;
}

int main() {
  const double kNaN = std::numeric_limits<double>::quiet_NaN(), kInf = std::numeric_limits<double>::infinity();
  // ---- the step
  int solved = 0, refused = 0;
  for (int trial = 0; trial < 1000; ++trial) {
    double A[36], b[6], xi[6];
    random_system(40, false, A, b);
    if (!icp_solve(A, b, xi)) { ++refused; continue; }
    ++solved;
    double worst = 0.0, top = 0.0;
    for (int i = 0; i < 6; ++i) {
      double r = -b[i], mag = std::fabs(b[i]);
      for (int j = 0; j < 6; ++j) { r += A[6 * i + j] * xi[j]; mag += std::fabs(A[6 * i + j] * xi[j]); }
      worst = std::fmax(worst, std::fabs(r) / mag);
      top = std::fmax(top, std::fabs(xi[i]));
    }
    EXPECT("a solution satisfies its system", worst < 1e-9 && std::isfinite(top));
    double T[12] = {1, 0, 0, 0.1, 0, 1, 0, -0.2, 0, 0, 1, 0.3}, norms[2];
    for (int k = 0; k < 3; ++k) xi[k] = (2.0 * uniform() - 1.0) * 3.0;  // rotations up to 3 rad per axis
    icp_apply(xi, T, norms);
    EXPECT("an updated pose is a rotation", proper_rotation(T, 1e-14));
  }
  EXPECT("every well-posed system is solved", solved == 1000 && refused == 0);
  int deficient_refused = 0;
  for (int trial = 0; trial < 200; ++trial) {
    double A[36], b[6], xi[6];
    random_system(40, true, A, b);
    if (!icp_solve(A, b, xi)) ++deficient_refused;
  }
  EXPECT("every rank-deficient system is refused", deficient_refused == 200);
  {
    double A[36] = {}, b[6] = {1, 1, 1, 1, 1, 1}, xi[6];
    for (int i = 0; i < 6; ++i) A[7 * i] = 1.0;
    A[14] = 0.0;
    EXPECT("a zero diagonal entry is refused", !icp_solve(A, b, xi));
    A[14] = -1.0;
    EXPECT("a negative diagonal entry is refused", !icp_solve(A, b, xi));
    A[14] = kNaN;
    EXPECT("a NaN diagonal entry is refused", !icp_solve(A, b, xi));
    A[14] = 1e-300;
    EXPECT("a tiny diagonal entry is scaled away", icp_solve(A, b, xi) && std::fabs(xi[2] - 1e300) < 1e286);
  }
  // ---- |w| on both sides of the switch: the two forms agree to the order of |w|^2
  int small_angles = 0;
  for (double ang : {0.0, 1e-150, 1e-13, 0.999e-12, 1e-12, 1.001e-12, 1e-11, 1e-8}) {
    const double xi[6] = {0.6 * ang, 0.0, -0.8 * ang, 0.01, -0.02, 0.03};
    double T[12] = {1, 0, 0, 0.1, 0, 1, 0, -0.2, 0, 0, 1, 0.3}, norms[2];
    icp_apply(xi, T, norms);
    EXPECT("the small-angle update is I + [w]x to rounding", std::fabs(T[1] - 0.8 * ang) <= 1e-16 * (1.0 + ang) && std::fabs(T[9] - 0.6 * ang) <= 1e-16 * (1.0 + ang) &&
                                                                 std::fabs(T[0] - 1.0) <= 1e-15);
    EXPECT("the norms are those of the step", std::fabs(norms[0] - ang) <= 1e-15 * ang && std::fabs(norms[1] - std::sqrt(0.0014)) < 1e-17);
    EXPECT("the translation follows", std::fabs(T[3] - (0.1 + 0.01)) < 1e-8 && std::isfinite(T[7]) && std::isfinite(T[11]));
    ++small_angles;
  }
  // ---- normals and association on maps of exactly H W entries
  const int H = 5, W = 4;
  const double intr[4] = {3.6, 3.4, 1.5, 2.0};
  std::vector<double> depth(H * W);
  for (int i = 0; i < H * W; ++i) depth[i] = 2.0 + 0.02 * (i % W) + 0.03 * (i / W);
  int normals_ok = 0;
  std::vector<double> nrm(3 * H * W, 0.0);
  std::vector<uint8_t> val(H * W, 0);
  for (int r = 1; r <= H - 2; ++r)
    for (int c = 1; c <= W - 2; ++c) {
      double n[3];
      const bool ok = icp_normal(depth.data(), W, intr, 0.05, r, c, n);
      EXPECT("an interior pixel of a smooth map has a unit normal that faces the camera",
             ok && std::fabs(n[0] * n[0] + n[1] * n[1] + n[2] * n[2] - 1.0) < 1e-15 && n[2] < 0.0);
      normals_ok += ok;
      val[r * W + c] = ok;
      for (int k = 0; k < 3; ++k) nrm[3 * (r * W + c) + k] = n[k];
    }
  for (double hole : {0.0, -1.0, kNaN, kInf})
    for (int nb = 0; nb < 5; ++nb) {
      std::vector<double> d = depth;
      const int at[5] = {2 * W + 1, 2 * W, 2 * W + 2, 1 * W + 1, 3 * W + 1};
      d[at[nb]] = hole;
      double n[3];
      EXPECT("a hole in the cross leaves no normal", !icp_normal(d.data(), W, intr, 0.05, 2, 1, n) && n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0);
    }
  {
    std::vector<double> d = depth;
    d[2 * W + 2] *= 1.06;
    double n[3];
    EXPECT("a depth edge leaves no normal", !icp_normal(d.data(), W, intr, 0.05, 2, 1, n));
    EXPECT("a wider edge_ratio keeps it", icp_normal(d.data(), W, intr, 0.1, 2, 1, n));
  }
  const IcpTarget tgt{depth.data(), nrm.data(), val.data(), H, W, {intr[0], intr[1], intr[2], intr[3]}};
  const IcpGates gates{1.0, 0.01, std::cos(30.0 * M_PI / 180.0)};
  const double I4[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  int linked = 0, turned_away = 0;
  const double rays[][3] = {{1.0, 2.0, 1.0}, {(double)(W - 1), (double)(H - 1), 1.0}, {(double)W - 0.5000001, 1.0, 1.0}, {(double)W - 0.5, 1.0, 1.0},
                            {-0.5000001, 1.0, 1.0}, {1.0, -0.51, 1.0}, {1.0, (double)H, 1.0}, {1e300, 1.0, 1.0}, {kNaN, 1.0, 1.0},
                            {1.0, kInf, 1.0}, {1.0, 1.0, -1.0}, {1.0, 1.0, 0.0}, {2.0, 3.0, 1.0}, {2.0, 1.0, 1.3}};
  for (const auto& ray : rays) {
    const int rr = 2, cc = 1;
    const double z = depth[rr * W + cc] * ray[2];
    const double p[3] = {((ray[0] - intr[2]) * z) / intr[0], ((ray[1] - intr[3]) * z) / intr[1], z};
    double acc[kIcpK] = {};
    icp_link(I4, gates, tgt, p, &nrm[3 * (rr * W + cc)], acc);
    double events = acc[kIcpCount];
    for (int k = 0; k < 4; ++k) events += acc[kIcpRej + k];
    EXPECT("a source pixel is counted exactly once", events == 1.0);
    linked += (int)acc[kIcpCount];
    turned_away += (int)(acc[kIcpRej] + acc[kIcpRej + 1]);
  }
  EXPECT("pixels inside link or fail a gate, pixels on the border or outside are turned away", linked >= 1 && turned_away >= 10);

  // ---- the argument checks of the entry points: MPSFM_EINVAL before any HIP call, buffers of exactly the stated length
  std::vector<double> d0(3 * 3, 1.0), d1(3 * 4, 1.0), init(I4, I4 + 12), trace(4 * 2, -1.0);
  std::vector<double> nout(3 * 1 * 1);
  std::vector<uint8_t> vout(1);
  const double K[4] = {2.0, 2.0, 1.0, 1.0};
  mpsfm_icp_options o{0.1, 30.0, 0.05, 1e-6, 1e-6, 2, 100, 1, 0};
  mpsfm_icp_result res;
  int einval = 0;
  auto icp = [&](int32_t H0, int32_t W0, const double* a, const double* Ka, const double* T, double s, const mpsfm_icp_options* opt, mpsfm_icp_result* out) {
    const int rc = mpsfm_depth_pair_icp(H0, W0, a, Ka, 3, 4, d1.data(), K, T, s, opt, 0, trace.data(), out);
    einval += rc == MPSFM_EINVAL;
    return rc;
  };
  icp(2, 3, d0.data(), K, init.data(), 1.0, &o, &res);
  icp(3, 2, d0.data(), K, init.data(), 1.0, &o, &res);
  icp(3, 3, nullptr, K, init.data(), 1.0, &o, &res);
  icp(3, 3, d0.data(), nullptr, init.data(), 1.0, &o, &res);
  icp(3, 3, d0.data(), K, nullptr, 1.0, &o, &res);
  icp(3, 3, d0.data(), K, init.data(), 1.0, nullptr, &res);
  icp(3, 3, d0.data(), K, init.data(), 1.0, &o, nullptr);
  icp(3, 3, d0.data(), K, init.data(), 0.0, &o, &res);
  icp(3, 3, d0.data(), K, init.data(), kNaN, &o, &res);
  icp(46341, 46341, d0.data(), K, init.data(), 1.0, &o, &res);
  const double K0[4] = {0.0, 2.0, 1.0, 1.0}, Kn[4] = {2.0, kInf, 1.0, 1.0};
  icp(3, 3, d0.data(), K0, init.data(), 1.0, &o, &res);
  icp(3, 3, d0.data(), Kn, init.data(), 1.0, &o, &res);
  for (int k = 0; k < 12; ++k) {
    std::vector<double> bad = init;
    bad[k] = k % 2 ? kNaN : kInf;
    icp(3, 3, d0.data(), K, bad.data(), 1.0, &o, &res);
  }
  int checks = 12 + 12;
  for (int field = 0; field < 10; ++field) {
    mpsfm_icp_options b = o;
    switch (field) {
      case 0: b.max_distance = 0.0; break;
      case 1: b.max_distance = kNaN; break;
      case 2: b.max_angle_deg = -1.0; break;
      case 3: b.max_angle_deg = 180.5; break;
      case 4: b.edge_ratio = -1e-9; break;
      case 5: b.eps_rotation = kInf; break;
      case 6: b.eps_translation = -1.0; break;
      case 7: b.max_iterations = MPSFM_ICP_MAX_ITERATIONS + 1; break;
      case 8: b.min_pairs = 5; break;
      default: b.stride = 0; break;
    }
    icp(3, 3, d0.data(), K, init.data(), 1.0, &b, &res);
    ++checks;
  }
  EXPECT("every bad argument is MPSFM_EINVAL", einval == checks);
  EXPECT("a refused call leaves a zeroed result and an untouched trace", res.iterations == 0 && res.num_pairs == 0 && trace[0] == -1.0 && trace[7] == -1.0);
  EXPECT("normals: NULL output", mpsfm_depth_normals(1, 1, d0.data(), K, 0.05, 0, nullptr, vout.data()) == MPSFM_EINVAL);
  EXPECT("normals: empty map", mpsfm_depth_normals(0, 1, d0.data(), K, 0.05, 0, nout.data(), vout.data()) == MPSFM_EINVAL);
  EXPECT("normals: bad edge_ratio", mpsfm_depth_normals(1, 1, d0.data(), K, kNaN, 0, nout.data(), vout.data()) == MPSFM_EINVAL);
  {
    mpsfm_align3d_options ro{0.1, 0.1, 0.99, 3.0, 100, 5000, 0, 0, 0};
    mpsfm_align3d_result rres;
    const double xy[2] = {1.0, 1.0};
    const int32_t match[2] = {0, 0}, bad_match[2] = {0, 1};
    uint8_t valid[1], mask[1];
    double l0[3], l1[3];
    mpsfm_icp_options b = o;
    b.stride = 0;
    EXPECT("dense: bad ICP options", mpsfm_depth_pair_register_dense(3, 3, d0.data(), K, 3, 4, d1.data(), K, 1, xy, 1, xy, 1, match, 0, &ro, &b, 0, valid, mask,
                                                                     l0, l1, &rres, trace.data(), &res) == MPSFM_EINVAL);
    EXPECT("dense: match out of range", mpsfm_depth_pair_register_dense(3, 3, d0.data(), K, 3, 4, d1.data(), K, 1, xy, 1, xy, 1, bad_match, 0, &ro, &o, 0, valid,
                                                                        mask, l0, l1, &rres, trace.data(), &res) == MPSFM_EINVAL);
    EXPECT("dense: a map below 3 x 3", mpsfm_depth_pair_register_dense(2, 3, d0.data(), K, 3, 4, d1.data(), K, 1, xy, 1, xy, 1, match, 0, &ro, &o, 0, valid, mask,
                                                                       l0, l1, &rres, trace.data(), &res) == MPSFM_EINVAL);
    EXPECT("dense: NULL ICP result", mpsfm_depth_pair_register_dense(3, 3, d0.data(), K, 3, 4, d1.data(), K, 1, xy, 1, xy, 1, match, 0, &ro, &o, 0, valid, mask,
                                                                     l0, l1, &rres, trace.data(), nullptr) == MPSFM_EINVAL);
    EXPECT("dense: no matches is no error and zeroes the trace",
           mpsfm_depth_pair_register_dense(3, 3, d0.data(), K, 3, 4, d1.data(), K, 1, xy, 1, xy, 0, nullptr, 0, &ro, &o, 0, nullptr, nullptr, nullptr, nullptr,
                                           &rres, trace.data(), &res) == 0 &&
               rres.success == 0 && trace[0] == 0.0 && trace[7] == 0.0 && res.iterations == 0);
  }
  std::printf("%d systems solved, %d rank-deficient refused, %d small-angle updates, %d normals, %d links, %d argument checks, %d failures\n", solved,
              deficient_refused, small_angles, normals_ok, linked, checks + 8, failures);
  return failures ? 1 : 0;
}
