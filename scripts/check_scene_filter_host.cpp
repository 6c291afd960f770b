// Stand-alone check of the host half of mpsfm_filter_scene (csrc/scene_filter.hip, csrc/scene_filter_check.h): every refusal and the
// empty paths, all of which return before any HIP call, plus one valid call, which is refused (MPSFM_ENODEVICE) on a machine
// without a device and computed with one.  Meant to be built with the host sanitizers and run on a CPU:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         scripts/check_scene_filter_host.cpp mpsfm_amd/csrc/scene_filter.hip mpsfm_amd/csrc/dev_resources.hip -o check_scene_filter_host
//   ./check_scene_filter_host
//
// Buffers are exactly as long as the header says, so a read or write past them is the sanitizer's to report.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../include/mpsfm_hip.h"
#include "../mpsfm_amd/csrc/host_parts.h"
#include "../mpsfm_amd/csrc/scene_filter_check.h"

// what the two library files linked here expect from files that are not (as in scripts/check_scene_queries_host.cpp)
namespace mpsfm {
int host_threads() { return 1; }
bool host_pool_enabled() { return false; }
HostPool* host_pool() { return nullptr; }
}  // namespace mpsfm
extern "C" const char* mpsfm_last_error(void) { return mpsfm::g_err.c_str(); }

static int failures = 0;
#define EXPECT(what, cond)                                       \
  do {                                                           \
    if (!(cond)) { std::printf("FAILED: %s\n", what); ++failures; } \
  } while (0)

template <class T>
static T* ptr(std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }

static const double kNaN = std::numeric_limits<double>::quiet_NaN(), kInf = std::numeric_limits<double>::infinity();

struct Scene {
  // image 0 at the origin and image 1 at x = 1 see points 0 and 1; image 2 has no keypoints, image 3 is not registered and sees nothing
  int32_t n_images = 4;
  std::vector<int64_t> kp_start{0, 3, 5, 5, 6}, kp_point{0, 1, -1, 0, 1, -1};
  std::vector<double> xy{0, 0, 0.125, 0, 9, 9, -0.125, 0, 0, 0, 1, 1}, intr{1, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0};
  std::vector<uint8_t> registered{1, 1, 1, 0};
  std::vector<double> quat{0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1}, t{0, 0, 0, -1, 0, 0, 0, 0, 0, kNaN, 0, 0}, xyz{0, 0, 8, 1, 0, 8};
  int64_t n_points = 2;
  std::vector<uint8_t> in_bundle{1, 1, 0, 0}, flags{1, 0, 1, 1, 0, 0}, sel{1, 1};
  mpsfm_scene_filter_options o{4.0, 1e-5, 0.026, 1, 0};
  std::vector<uint8_t> deleted, fate, risky;
  std::vector<double> angle, err;
  bool with_values = true, with_graph = true, with_state = true, with_options = true;
  bool with_deleted = true, with_fate = true, with_risky = true, with_info = true;
  mpsfm_scene_filter_info info;
  int run() {
    const size_t n_kp = kp_start.empty() || kp_start.back() < 0 || kp_start.back() > 1000 ? 0 : (size_t)kp_start.back();
    deleted.assign(n_kp, 9); err.assign(with_values ? n_kp : 0, 9.0);
    const size_t np = n_points > 0 && n_points < 1000 ? (size_t)n_points : 0;
    fate.assign(np, 9); risky.assign(np, 9); angle.assign(with_values ? np : 0, 9.0);
    const mpsfm_tri_graph g{n_images, ptr(kp_start), ptr(xy), ptr(intr), nullptr, nullptr};
    const mpsfm_tri_state st{ptr(registered), ptr(quat), ptr(t), ptr(kp_point), n_points, ptr(xyz)};
    return mpsfm_filter_scene(with_graph ? &g : nullptr, with_state ? &st : nullptr, ptr(in_bundle), ptr(flags), ptr(sel), with_options ? &o : nullptr, 0,
                              with_deleted ? ptr(deleted) : nullptr, with_fate ? ptr(fate) : nullptr, with_risky ? ptr(risky) : nullptr, ptr(angle),
                              ptr(err), with_info ? &info : nullptr);
  }
};

static void check_refusals() {
  { Scene s; s.with_graph = false; EXPECT("NULL graph", s.run() == MPSFM_EINVAL); }
  { Scene s; s.with_state = false; EXPECT("NULL state", s.run() == MPSFM_EINVAL); }
  { Scene s; s.with_options = false; EXPECT("NULL options", s.run() == MPSFM_EINVAL); }
  { Scene s; s.with_deleted = false; EXPECT("NULL kp_deleted", s.run() == MPSFM_EINVAL); }
  { Scene s; s.with_fate = false; EXPECT("NULL point_fate", s.run() == MPSFM_EINVAL); }
  { Scene s; s.with_risky = false; EXPECT("NULL point_risky", s.run() == MPSFM_EINVAL); }
  { Scene s; s.n_images = -1; EXPECT("negative n_images", s.run() == MPSFM_EINVAL); }
  { Scene s; s.kp_start.clear(); EXPECT("NULL kp_start", s.run() == MPSFM_EINVAL); }
  { Scene s; s.kp_start[0] = 1; EXPECT("kp_start[0]", s.run() == MPSFM_EINVAL); }
  { Scene s; s.kp_start = {0, 3, 2, 5, 6}; EXPECT("decreasing kp_start", s.run() == MPSFM_EINVAL); }
  { Scene s; s.kp_start[4] = 1ll << 31; EXPECT("2^31 keypoints", s.run() == MPSFM_EUNSUPPORTED); }
  { Scene s; s.n_points = -1; EXPECT("negative n_points", s.run() == MPSFM_EINVAL); }
  { Scene s; s.n_points = 1ll << 31; EXPECT("2^31 points", s.run() == MPSFM_EUNSUPPORTED); }
  { Scene s; s.xy.clear(); EXPECT("NULL kp_xy", s.run() == MPSFM_EINVAL); }
  { Scene s; s.intr.clear(); EXPECT("NULL cam_intr", s.run() == MPSFM_EINVAL); }
  { Scene s; s.registered.clear(); EXPECT("NULL registered", s.run() == MPSFM_EINVAL); }
  { Scene s; s.quat.clear(); EXPECT("NULL quat", s.run() == MPSFM_EINVAL); }
  { Scene s; s.t.clear(); EXPECT("NULL t", s.run() == MPSFM_EINVAL); }
  { Scene s; s.kp_point.clear(); EXPECT("NULL kp_point", s.run() == MPSFM_EINVAL); }
  { Scene s; s.xyz.clear(); EXPECT("NULL xyz", s.run() == MPSFM_EINVAL); }
  { Scene s; s.kp_point[4] = 2; EXPECT("kp_point too large", s.run() == MPSFM_EINVAL); s.kp_point[4] = -2; EXPECT("kp_point below -1", s.run() == MPSFM_EINVAL); }
  { Scene s; s.kp_point[5] = 0; EXPECT("a point in an unregistered image", s.run() == MPSFM_EINVAL); }
  { Scene s; s.xyz[4] = kNaN; EXPECT("NaN point", s.run() == MPSFM_EINVAL); }
  { Scene s; s.t[3] = kInf; EXPECT("infinite pose", s.run() == MPSFM_EINVAL); }
  { Scene s; s.quat[5] = kNaN; EXPECT("NaN rotation", s.run() == MPSFM_EINVAL); }
  { Scene s; s.intr[14] = kNaN; EXPECT("NaN intrinsics", s.run() == MPSFM_EINVAL); }
  { Scene s; s.o.max_reproj_error = -1.0; EXPECT("negative error", s.run() == MPSFM_EINVAL); s.o.max_reproj_error = kNaN; EXPECT("NaN error", s.run() == MPSFM_EINVAL); }
  { Scene s; s.o.min_tri_angle_rad = -1.0; EXPECT("negative angle", s.run() == MPSFM_EINVAL); s.o.min_tri_angle_rad = kInf; EXPECT("infinite angle", s.run() == MPSFM_EINVAL); }
  { Scene s; s.o.risky_min_tri_angle_rad = kNaN; EXPECT("NaN risky angle", s.run() == MPSFM_EINVAL); }
  { Scene s; s.o.negative_depth = 2; EXPECT("negative_depth 2", s.run() == MPSFM_EINVAL); }
  // a check that fails must leave the outputs alone
  { Scene s; s.o.negative_depth = 2; s.run(); EXPECT("outputs untouched by a refusal", s.deleted[0] == 9 && s.fate[0] == 9 && s.angle[1] == 9.0); }
}

static void check_empty() {
  {
    Scene s;  // no points: zeros without a device
    s.n_points = 0; s.xyz.clear(); s.sel.clear(); s.kp_point.assign(6, -1);
    bool ok = s.run() == 0 && s.info.num_syncs == 0;
    for (uint8_t v : s.deleted) ok = ok && v == 0;
    for (double v : s.err) ok = ok && v == 0.0;
    EXPECT("no points", ok);
  }
  {
    Scene s;  // no keypoints
    s.kp_start = {0, 0, 0, 0, 0}; s.xy.clear(); s.kp_point.clear(); s.flags.clear();
    bool ok = s.run() == 0 && s.info.num_syncs == 0;
    for (uint8_t v : s.fate) ok = ok && v == 0;
    for (uint8_t v : s.risky) ok = ok && v == 0;
    for (double v : s.angle) ok = ok && v == 0.0;
    EXPECT("no keypoints", ok);
  }
  {
    Scene s;  // no image at all
    s.n_images = 0; s.kp_start = {0}; s.xy.clear(); s.intr.clear(); s.registered.clear(); s.quat.clear(); s.t.clear(); s.kp_point.clear();
    s.in_bundle.clear(); s.flags.clear();
    EXPECT("no image", s.run() == 0 && s.fate[0] == 0 && s.fate[1] == 0);
  }
  {
    Scene s;  // point_max_angle, kp_sq_err and info may be NULL: nothing is written through them
    s.n_points = 0; s.xyz.clear(); s.sel.clear(); s.kp_point.assign(6, -1); s.with_values = false; s.with_info = false;
    bool ok = s.run() == 0;
    for (uint8_t v : s.deleted) ok = ok && v == 0;
    EXPECT("no points; no values, no info asked for", ok);
  }
  {
    Scene s;  // the same on the other empty path, where the point outputs are the ones that are zeroed
    s.kp_start = {0, 0, 0, 0, 0}; s.xy.clear(); s.kp_point.clear(); s.flags.clear(); s.with_values = false; s.with_info = false;
    bool ok = s.run() == 0;
    for (uint8_t v : s.fate) ok = ok && v == 0;
    for (uint8_t v : s.risky) ok = ok && v == 0;
    EXPECT("no keypoints; no values, no info asked for", ok);
  }
  {
    Scene s;  // outputs of length 0 may be NULL: no keypoints, so kp_deleted is not needed; no points, so neither are the point outputs
    s.kp_start = {0, 0, 0, 0, 0}; s.xy.clear(); s.kp_point.clear(); s.flags.clear(); s.with_deleted = false;
    EXPECT("NULL kp_deleted without keypoints", s.run() == 0 && s.fate[0] == 0 && s.fate[1] == 0);
  }
  {
    Scene s;
    s.n_points = 0; s.xyz.clear(); s.sel.clear(); s.kp_point.assign(6, -1); s.with_fate = false; s.with_risky = false;
    EXPECT("NULL point outputs without points", s.run() == 0 && s.deleted[0] == 0);
  }
  { Scene s; s.in_bundle.clear(); EXPECT("NULL in_bundle alone", s.run() == 0 || s.run() == MPSFM_ENODEVICE); }
}

int main() {
  check_refusals();
  check_empty();
  for (int variant = 0; variant < 2; ++variant) {
    Scene s;  // the pose of the unregistered image is NaN and never read
    if (variant) { s.in_bundle.clear(); s.flags.clear(); s.sel.clear(); s.with_values = false; }
    const int rc = s.run();
    std::printf("valid call %d: %d (%s)\n", variant, rc, rc == 0 ? "computed" : mpsfm_last_error());
    EXPECT("valid call", rc == MPSFM_ENODEVICE || (rc == 0 && s.fate[0] == 0 && s.fate[1] == 0 && s.info.num_syncs == 1 && s.risky[0] == (variant ? 0 : 1)));
  }
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
