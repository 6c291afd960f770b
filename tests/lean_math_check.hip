// Stand-alone host program of tests/test_lean_math_cpu.py: the host paths of csrc/common.h's lean_log and of quat_plus' two
// polynomials against long double.  Prints one "name value" line per figure (ulp distances are measured in units of the spacing
// of doubles at the reference value); the test asserts the bounds.  No device is touched.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "../mpsfm_amd/csrc/common.h"

using mpsfm::lean_log;

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t next_u64() {  // splitmix64
  uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
static double uniform01() { return (double)(next_u64() >> 11) * 0x1p-53; }

// |got - ref| in ulps of a double at ref
static double ulp_err(double got, long double ref) {
  if (ref == 0.0L) return got == 0.0 ? 0.0 : std::numeric_limits<double>::infinity();
  int e = std::ilogb((double)ref);
  if (e < -1022) e = -1022;
  return (double)(std::fabs((long double)got - ref) / std::ldexp(1.0L, e - 52));
}
static double g_worst_x = 0.0;
static void check_log(double x, double& worst) {
  const double e = ulp_err(lean_log(x), logl((long double)x));
  if (!(e <= worst)) { worst = e; g_worst_x = x; }
}
static void check_sinc_cos(double z, double& ws, double& wc) {
  const long double n = sqrtl((long double)z);
  const long double rs = z == 0.0 ? 1.0L : sinl(n) / n, rc = cosl(n);
  const double es = ulp_err(mpsfm::quat_sinc_poly(z), rs), ec = ulp_err(mpsfm::quat_cos_poly(z), rc);
  if (!(es <= ws)) ws = es;
  if (!(ec <= wc)) wc = ec;
}

int main(int argc, char** argv) {
  const long n = argc > 1 ? std::atol(argv[1]) : 4000000;
  double w;
  w = 0.0;  // depths, log-uniform in e^-10 .. e^10
  for (long i = 0; i < n; ++i) check_log(std::exp(20.0 * uniform01() - 10.0), w);
  std::printf("log_depths %.6f\n", w);
  w = 0.0;  // 1 + 2^-k u, u in (-1, 1)
  for (long i = 0; i < n; ++i) check_log(1.0 + std::ldexp(2.0 * uniform01() - 1.0, -(int)(i % 53)), w);
  std::printf("log_near_one %.6f\n", w);
  w = 0.0;  // [0.5, 1.5]
  for (long i = 0; i < n; ++i) check_log(0.5 + uniform01(), w);
  std::printf("log_half_to_three_halves %.6f\n", w);
  w = 0.0;  // every binade boundary and its two neighbours, subnormal binades included
  for (int e = -1074; e <= 1023; ++e) {
    const double x = std::ldexp(1.0, e);
    check_log(x, w);
    check_log(std::nextafter(x, HUGE_VAL), w);
    if (e > -1074) check_log(std::nextafter(x, 0.0), w);
  }
  check_log(std::numeric_limits<double>::max(), w);
  check_log(std::sqrt(0.5), w); check_log(std::nextafter(std::sqrt(0.5), 0.0), w); check_log(std::nextafter(std::sqrt(0.5), 1.0), w);
  check_log(std::sqrt(2.0), w); check_log(std::nextafter(std::sqrt(2.0), 0.0), w); check_log(std::nextafter(std::sqrt(2.0), 2.0), w);
  std::printf("log_binades %.6f\n", w);
  w = 0.0;  // subnormals
  for (long i = 0; i < n / 16; ++i) {
    uint64_t bits = next_u64() >> (12 + (int)(i % 52));
    if (bits == 0) bits = 1;
    double x;
    std::memcpy(&x, &bits, 8);
    check_log(x, w);
  }
  std::printf("log_subnormals %.6f\n", w);
  std::printf("log_one_exact %d\n", lean_log(1.0) == 0.0 ? 1 : 0);
  std::printf("log_inf %d\n", lean_log(HUGE_VAL) == HUGE_VAL ? 1 : 0);

  const double zmax = mpsfm::kQuatPolyMaxZ;
  double ws = 0.0, wc = 0.0;
  for (long i = 0; i < n; ++i) check_sinc_cos(zmax * uniform01(), ws, wc);
  for (long i = 0; i < n / 4; ++i) check_sinc_cos(zmax * std::exp(-40.0 * uniform01()), ws, wc);
  check_sinc_cos(zmax, ws, wc); check_sinc_cos(0.0, ws, wc); check_sinc_cos(std::numeric_limits<double>::denorm_min(), ws, wc);
  std::printf("sinc_poly %.6f\ncos_poly %.6f\n", ws, wc);
  std::printf("sinc_zero_exact %d\ncos_zero_exact %d\n", mpsfm::quat_sinc_poly(0.0) == 1.0 ? 1 : 0, mpsfm::quat_cos_poly(0.0) == 1.0 ? 1 : 0);
  // both sides of quat_sinc_cos' branch at the threshold and at its neighbours, in ulps of the polynomial's value
  double wt = 0.0;
  const double zs[3] = {std::nextafter(zmax, 0.0), zmax, std::nextafter(zmax, 1.0)};
  for (double z : zs) {
    double s, c;
    mpsfm::quat_sinc_cos_far(z, s, c);
    wt = std::fmax(wt, std::fmax(ulp_err(s, (long double)mpsfm::quat_sinc_poly(z)), ulp_err(c, (long double)mpsfm::quat_cos_poly(z))));
  }
  std::printf("branch_threshold %.6f\n", wt);
  // the plus itself: z == 0 returns q, a step beyond the threshold stays unit
  const double q[4] = {0.1, -0.7, 0.5, std::sqrt(1.0 - 0.01 - 0.49 - 0.25)}, d0[3] = {0.0, 0.0, 0.0}, d1[3] = {1.5, -2.0, 0.5};
  double o[4];
  mpsfm::quat_plus(q, d0, o);
  std::printf("plus_zero_exact %d\n", (o[0] == q[0] && o[1] == q[1] && o[2] == q[2] && o[3] == q[3]) ? 1 : 0);
  mpsfm::quat_plus(q, d1, o);
  std::printf("plus_far_norm_err %.3e\n", std::fabs(std::sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2] + o[3] * o[3]) - 1.0));
  return 0;
}
