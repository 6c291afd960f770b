// Stand-alone check of the host half of the scene queries (csrc/scene_queries.hip, csrc/local_bundle_walk.h): the threshold walk of
// mpsfm_local_bundles on rows written by hand, the argument checks and the empty paths of both entry points, all of which return
// before any HIP call, plus one valid call each, which is refused (MPSFM_ENODEVICE) on a machine without a device and computed
// with one.  Meant to be built with the host sanitizers and run on a CPU:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         scripts/check_scene_queries_host.cpp mpsfm_amd/csrc/scene_queries.hip mpsfm_amd/csrc/dev_resources.hip -o check_scene_queries_host
//   ./check_scene_queries_host
//
// Buffers are exactly as long as the header says, so a read or write past them is the sanitizer's to report.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../include/mpsfm_hip.h"
#include "../mpsfm_amd/csrc/host_parts.h"
#include "../mpsfm_amd/csrc/local_bundle_walk.h"

// what the two library files linked here expect from files that are not (as in scripts/check_corr_graph_host.cpp): the error text
// (ba_solver.hip) and the host thread pool behind the staged uploads (build_host.hip), which these calls do not use
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

// ---- the walk ----------------------------------------------------------------------------------------------------------------------
static std::vector<int32_t> walk(std::vector<int32_t> shared, std::vector<double> angle75, int64_t T, int32_t num_images, double deg = 6.0) {
  std::vector<int32_t> bundle((size_t)(num_images - 1), 99), order;  // exactly num_images - 1 long
  const int32_t len = mpsfm::local_bundle_walk((int32_t)shared.size(), shared.data(), angle75.data(), T, num_images, deg * (M_PI / 180.0),
                                               ptr(bundle), order);
  for (size_t i = 0; i < bundle.size(); ++i) EXPECT("padding", (i < (size_t)len) == (bundle[i] >= 0));
  bundle.resize((size_t)len);
  return bundle;
}
using V = std::vector<int32_t>;

static void check_walk() {
  // the scenes of tests/numpy_scene_queries.py walk_cases(), as rows; image 0 is the reference
  EXPECT("take all", walk({0, 3, 9, 5}, {-1, 0.2, 0.012, 0.05}, 10, 6) == (V{2, 3, 1}));
  EXPECT("third threshold", walk({0, 9, 8, 7, 2}, {-1, 0.06, 0.2, 0.055, 0.3}, 10, 3) == (V{2, 1}));
  EXPECT("overlap break", walk({0, 18, 5, 1}, {-1, 0.2, 0.012, 0.3}, 20, 3) == (V{1, 2}));
  EXPECT("fill up", walk({0, 4, 9, 6, 7}, {-1, 0.012, 0.013, 0.011, 0.0125}, 10, 3) == (V{2, 4}));
  EXPECT("ties", walk({0, 6, 7, 6, 6}, {-1, 0.2, 0.012, 0.2, 0.012}, 10, 3) == (V{1, 3}));
  EXPECT("ties in the fill", walk({0, 6, 6, 6}, {-1, 0.012, 0.012, 0.012}, 10, 3) == (V{1, 2}));
  // the edges: one image asked for (nothing but the reference), nothing overlapping, no image at all, an angle exactly on a threshold
  EXPECT("num_images 1", walk({0, 3, 9}, {-1, 0.2, 0.2}, 10, 1).empty());
  EXPECT("no overlap", walk({0, 0, 0}, {-1, -1, -1}, 10, 4).empty());
  EXPECT("no image", walk({}, {}, 0, 4).empty());
  const double rad = 6.0 * (M_PI / 180.0);
  EXPECT("on the threshold", walk({0, 9, 8}, {-1, std::nextafter(rad, 0.0), rad}, 10, 2) == (V{2}));
  EXPECT("T = 0", walk({0, 2, 1}, {-1, 0.012, 0.5}, 0, 2) == (V{2}));  // every second number is 0: no break
  EXPECT("more than the walk gives", walk({0, 9, 8, 7}, {-1, 0.012, 0.5, 0.012}, 10, 3) == (V{2, 1}));
}

// ---- the entry points ----------------------------------------------------------------------------------------------------------------
struct Vis {
  std::vector<int64_t> kp_start{0, 2, 3}, corr_start{0, 1, 2, 4}, corr_kp{2, 2, 0, 1}, kp_point{-1, -1, 0};
  std::vector<double> xy{5, 5, 6, 6, 1, 1};
  std::vector<int32_t> size{640, 480, 640, 480}, num_visible{9, 9};
  std::vector<int64_t> score{9, 9};
  std::vector<uint8_t> visible{9, 9, 9};
  int32_t levels = 6, n_images = 2;
  mpsfm_scene_query_info info;
  int run() {
    return mpsfm_visibility_scores(n_images, ptr(kp_start), ptr(xy), ptr(corr_start), ptr(corr_kp), ptr(kp_point), ptr(size), levels, 0,
                                   ptr(num_visible), ptr(score), ptr(visible), &info);
  }
};

static void check_visibility() {
  { Vis v; v.levels = 0; EXPECT("levels 0", v.run() == MPSFM_EINVAL); v.levels = 9; EXPECT("levels 9", v.run() == MPSFM_EINVAL); }
  { Vis v; v.n_images = -1; EXPECT("negative n_images", v.run() == MPSFM_EINVAL); }
  { Vis v; v.kp_start[0] = 1; EXPECT("kp_start[0]", v.run() == MPSFM_EINVAL); }
  { Vis v; v.kp_start = {0, 3, 2}; EXPECT("decreasing kp_start", v.run() == MPSFM_EINVAL); }
  { Vis v; v.kp_start[2] = 1ll << 31; EXPECT("2^31 keypoints", v.run() == MPSFM_EUNSUPPORTED); }
  { Vis v; v.corr_start[0] = 1; EXPECT("corr_start[0]", v.run() == MPSFM_EINVAL); }
  { Vis v; v.corr_start = {0, 2, 1, 4}; EXPECT("decreasing corr_start", v.run() == MPSFM_EINVAL); }
  { Vis v; v.corr_kp[3] = 3; EXPECT("corr_kp too large", v.run() == MPSFM_EINVAL); v.corr_kp[3] = -1; EXPECT("corr_kp negative", v.run() == MPSFM_EINVAL); }
  { Vis v; v.size[3] = 0; EXPECT("height 0", v.run() == MPSFM_EINVAL); }
  { Vis v; v.xy.clear(); EXPECT("NULL kp_xy", v.run() == MPSFM_EINVAL); }
  { Vis v; v.score.clear(); EXPECT("NULL score", v.run() == MPSFM_EINVAL); }
  {
    Vis v;  // images without keypoints: zeros, no device
    v.kp_start = {0, 0, 0}; v.xy.clear(); v.corr_start.clear(); v.corr_kp.clear(); v.kp_point.clear(); v.visible.clear();
    EXPECT("no keypoints", v.run() == 0 && v.num_visible[0] == 0 && v.num_visible[1] == 0 && v.score[0] == 0 && v.score[1] == 0 && v.info.num_syncs == 0);
  }
  Vis v;
  const int rc = v.run();
  std::printf("valid visibility call: %d (%s)\n", rc, rc == 0 ? "computed" : mpsfm_last_error());
  EXPECT("valid visibility call", rc == MPSFM_ENODEVICE || (rc == 0 && v.num_visible[0] == 2 && v.score[0] == 5460 && v.visible[2] == 0));
}

struct Lb {
  // reference 0 at the origin sees points 0 .. 2, image 1 at x = 2 sees points 0 and 1, image 2 (not registered) sees point 2
  std::vector<int64_t> kp_start{0, 3, 5, 6}, kp_point{0, 1, 2, 0, 1, 2};
  std::vector<uint8_t> registered{1, 1, 0};
  std::vector<double> quat{0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1}, t{0, 0, 0, -2, 0, 0, -4, 0, 0}, xyz{0, 0, 10, 0.5, 0, 10, 1, 0, 10};
  std::vector<int32_t> refs{0, 0}, bundle, bundle_len{9, 9}, shared;
  std::vector<double> angle75;
  int32_t num_images = 3, n_images = 3, n_refs = 2;
  int64_t n_points = 3;
  double deg = 6.0;
  mpsfm_scene_query_info info;
  int run() {
    bundle.assign((size_t)(n_refs > 0 ? n_refs : 0) * (size_t)(num_images > 1 ? num_images - 1 : 0), 9);
    shared.assign((size_t)(n_refs > 0 ? n_refs : 0) * 3, 9);
    angle75.assign(shared.size(), 9.0);
    const mpsfm_tri_state st{ptr(registered), ptr(quat), ptr(t), ptr(kp_point), n_points, ptr(xyz)};
    return mpsfm_local_bundles(n_images, ptr(kp_start), &st, n_refs, ptr(refs), num_images, deg, 0, ptr(bundle), ptr(bundle_len), ptr(shared),
                               ptr(angle75), &info);
  }
};

static void check_local_bundles() {
  { Lb b; b.num_images = 0; EXPECT("num_images 0", b.run() == MPSFM_EINVAL); }
  { Lb b; b.n_refs = -1; EXPECT("negative n_refs", b.run() == MPSFM_EINVAL); }
  { Lb b; b.n_images = -1; EXPECT("negative n_images", b.run() == MPSFM_EINVAL); }
  { Lb b; b.refs[1] = 2; EXPECT("reference not registered", b.run() == MPSFM_EINVAL); }
  { Lb b; b.refs[1] = 3; EXPECT("reference too large", b.run() == MPSFM_EINVAL); b.refs[1] = -1; EXPECT("reference negative", b.run() == MPSFM_EINVAL); }
  { Lb b; b.kp_start[0] = 1; EXPECT("kp_start[0]", b.run() == MPSFM_EINVAL); }
  { Lb b; b.kp_point[4] = 3; EXPECT("kp_point too large", b.run() == MPSFM_EINVAL); b.kp_point[4] = -2; EXPECT("kp_point below -1", b.run() == MPSFM_EINVAL); }
  { Lb b; b.n_points = -1; EXPECT("negative n_points", b.run() == MPSFM_EINVAL); }
  { Lb b; b.xyz[4] = std::numeric_limits<double>::quiet_NaN(); EXPECT("NaN point", b.run() == MPSFM_EINVAL); }
  { Lb b; b.t[3] = std::numeric_limits<double>::infinity(); EXPECT("infinite pose", b.run() == MPSFM_EINVAL); }
  { Lb b; b.t[6] = std::numeric_limits<double>::quiet_NaN(); const int rc = b.run(); EXPECT("pose of an unregistered image is not read", rc == 0 || rc == MPSFM_ENODEVICE); }
  { Lb b; b.deg = -1.0; EXPECT("negative angle", b.run() == MPSFM_EINVAL); b.deg = std::numeric_limits<double>::quiet_NaN(); EXPECT("NaN angle", b.run() == MPSFM_EINVAL); }
  { Lb b; b.xyz.clear(); EXPECT("NULL xyz", b.run() == MPSFM_EINVAL); }
  { Lb b; b.quat.clear(); EXPECT("NULL quat", b.run() == MPSFM_EINVAL); }
  { Lb b; b.n_refs = 0; b.refs.clear(); b.bundle_len.clear(); EXPECT("no reference", b.run() == 0); }
  {
    Lb b;  // no keypoint has a point: the empty answer without a device, rows exactly num_images - 1 long
    b.kp_point.assign(6, -1);
    bool ok = b.run() == 0 && b.bundle_len[0] == 0 && b.bundle_len[1] == 0 && b.info.num_syncs == 0;
    for (int32_t v : b.bundle) ok = ok && v == -1;
    for (int32_t v : b.shared) ok = ok && v == 0;
    for (double v : b.angle75) ok = ok && v == -1.0;
    EXPECT("nothing shared", ok);
  }
  { Lb b; b.num_images = 1; b.kp_point.assign(6, -1); EXPECT("num_images 1 needs no bundle", b.run() == 0 && b.bundle.empty()); }
  Lb b;
  const int rc = b.run();
  std::printf("valid local-bundle call: %d (%s)\n", rc, rc == 0 ? "computed" : mpsfm_last_error());
  EXPECT("valid local-bundle call", rc == MPSFM_ENODEVICE || (rc == 0 && b.bundle_len[0] == 1 && b.bundle[0] == 1 && b.bundle[1] == -1 && b.shared[1] == 2 &&
                                                                b.shared[2] == 0 && b.shared[4] == 2 && b.angle75[2] == -1.0 && b.info.num_syncs == 1));
}

int main() {
  check_walk();
  check_visibility();
  check_local_bundles();
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
