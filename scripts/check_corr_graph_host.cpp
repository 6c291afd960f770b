// Stand-alone check of the host half of mpsfm_corr_graph_build (csrc/corr_graph.hip): the argument checks, the limits and the empty
// paths, all of which return before any HIP call, plus one valid call, which is refused (MPSFM_ENODEVICE) on a machine without a
// device and computed with one.  Meant to be built with the host sanitizers and run on a CPU:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         scripts/check_corr_graph_host.cpp mpsfm_amd/csrc/corr_graph.hip mpsfm_amd/csrc/dev_resources.hip -o check_corr_graph_host
//   ./check_corr_graph_host
//
// Buffers are exactly as long as the header says, so a read or write past them is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/mpsfm_hip.h"
#include "../mpsfm_amd/csrc/host_parts.h"

// what the two library files linked here expect from files that are not: the error text (ba_solver.hip) and the host thread pool
// behind the staged uploads (build_host.hip), which this call does not use
// These stand-ins repeat declarations of csrc/host_parts.h and dev_resources.h: the program is tied to those internals and has to
// follow them when they move (linking every host object of the library instead would need them all built with the sanitizers).
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

struct Case {
  std::vector<int64_t> kp_start, list_start;
  std::vector<int32_t> li0, li1, matches;
  // outputs at exactly their capacities
  std::vector<uint8_t> status, two_view;
  std::vector<int64_t> corr_start, corr_kp, pair_start;
  std::vector<int32_t> im_corr, im_obs, p0, p1, pm;
  int64_t n_corr = 7, n_pairs = 7;
  mpsfm_corr_graph_info info;

  Case(std::vector<int64_t> kp, std::vector<int32_t> a, std::vector<int32_t> b, std::vector<int64_t> ls, std::vector<int32_t> m)
      : kp_start(kp), list_start(ls), li0(a), li1(b), matches(m) {
    const size_t n_images = kp.size() - 1, n_kp = (size_t)kp.back(), M = m.size() / 2, L = a.size();
    status.assign(M, 9); two_view.assign(n_kp, 9); corr_start.assign(n_kp + 1, 9); corr_kp.assign(2 * M, 9); pair_start.assign(L + 1, 9);
    im_corr.assign(n_images, 9); im_obs.assign(n_images, 9); p0.assign(L, 9); p1.assign(L, 9); pm.assign(2 * M, 9);
  }
  template <class T>
  static T* ptr(std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }
  int run() {
    return mpsfm_corr_graph_build((int32_t)kp_start.size() - 1, kp_start.data(), (int32_t)li0.size(), ptr(li0), ptr(li1), list_start.data(), ptr(matches), 0,
                                  ptr(status), corr_start.data(), ptr(corr_kp), &n_corr, ptr(im_corr), ptr(im_obs), ptr(two_view), &n_pairs, ptr(p0),
                                  ptr(p1), pair_start.data(), ptr(pm), &info);
  }
};

int main() {
  EXPECT("kp_start[0]", Case({1, 2, 5}, {0}, {1}, {0, 1}, {0, 0}).run() == MPSFM_EINVAL);
  EXPECT("list_start[0]", Case({0, 2, 5}, {0}, {1}, {1, 1}, {}).run() == MPSFM_EINVAL);
  EXPECT("decreasing kp_start", Case({0, 5, 2}, {0}, {1}, {0, 1}, {0, 0}).run() == MPSFM_EINVAL);
  {
    Case c({0, 2, 5}, {0, 0}, {1, 1}, {0, 1, 0}, {});
    EXPECT("decreasing list_start", c.run() == MPSFM_EINVAL);
  }
  EXPECT("list image too large", Case({0, 2, 5}, {2}, {1}, {0, 1}, {0, 0}).run() == MPSFM_EINVAL);
  EXPECT("list image negative", Case({0, 2, 5}, {0}, {-1}, {0, 1}, {0, 0}).run() == MPSFM_EINVAL);
  {
    Case c({0, 2, 5}, {0}, {1}, {0, 1}, {0, 0});
    c.kp_start[2] = 1ll << 31;  // read from the start arrays alone: nothing of that size is touched
    EXPECT("2^31 keypoints", c.run() == MPSFM_EUNSUPPORTED);
    c.kp_start[2] = 5;
    c.list_start[1] = 1ll << 30;
    EXPECT("2^30 matches", c.run() == MPSFM_EUNSUPPORTED);
  }
  {
    Case c({0}, {}, {}, {0}, {});  // no image
    EXPECT("no image", c.run() == 0 && c.n_corr == 0 && c.n_pairs == 0 && c.corr_start[0] == 0 && c.pair_start[0] == 0);
  }
  {
    Case c({0, 3, 5}, {0, 1}, {1, 0}, {0, 0, 0}, {});  // lists without a match
    bool ok = c.run() == 0 && c.n_corr == 0 && c.n_pairs == 0;
    for (int64_t v : c.corr_start) ok = ok && v == 0;
    for (uint8_t v : c.two_view) ok = ok && v == 0;
    for (int64_t v : c.pair_start) ok = ok && v == 0;
    EXPECT("no match", ok && c.im_corr[0] == 0 && c.im_obs[1] == 0);
  }
  {
    Case c({0, 0, 0}, {0, 1}, {1, 1}, {0, 2, 3}, {0, 0, 1, -1, 0, 0});  // images without keypoints: no index is in range
    bool ok = c.run() == 0 && c.status[0] == 1 && c.status[1] == 1 && c.status[2] == 2 && c.info.num_invalid == 2 && c.info.num_self_pairs == 1;
    for (int64_t v : c.corr_kp) ok = ok && v == 0;
    for (int32_t v : c.pm) ok = ok && v == 0;
    EXPECT("no keypoint", ok && c.info.num_syncs == 0);
  }
  Case valid({0, 2, 5}, {0, 1}, {1, 0}, {0, 3, 4}, {0, 0, 1, 2, 0, 0, 1, 1});
  const int rc = valid.run();
  std::printf("valid call: %d (%s)\n", rc, rc == 0 ? "computed" : mpsfm_last_error());
  EXPECT("valid call", rc == MPSFM_ENODEVICE || (rc == 0 && valid.n_corr == 6 && valid.n_pairs == 1 && valid.status[2] == 3));
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
