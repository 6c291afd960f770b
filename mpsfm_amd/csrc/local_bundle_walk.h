// The host half of mpsfm_local_bundles (scene_queries.hip): which of the overlapping images form the local bundle of a reference
// image, from the per-image shared counts and 75th-percentile triangulation angles the device computed.  COLMAP 3.11
// IncrementalMapper::FindLocalBundle, restated (include/mpsfm_hip.h; parity unpinned).  Plain C++ and no HIP: a stand-alone
// program drives it under the host sanitizers (scripts/check_scene_queries_host.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace mpsfm {

constexpr int kLocalBundleThresholds = 8;
constexpr double kLocalBundleAngleDiv[kLocalBundleThresholds] = {1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 5.0, 6.0};
constexpr double kLocalBundleSharedRatio[kLocalBundleThresholds] = {0.6, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1, 0.1};

// shared / angle75: the row [n_images] of one reference image (shared[ref] == 0); T: its keypoints with a point;
// bundle [num_images - 1]: image indices, padded with -1.  Returns the number of images taken.
inline int32_t local_bundle_walk(int32_t n_images, const int32_t* shared, const double* angle75, int64_t T, int32_t num_images,
                                 double min_tri_angle_rad, int32_t* bundle, std::vector<int32_t>& order) {
  const int32_t N = num_images - 1;
  for (int32_t i = 0; i < N; ++i) bundle[i] = -1;
  order.clear();
  for (int32_t j = 0; j < n_images; ++j)
    if (shared[j] > 0) order.push_back(j);
  // most shared points first; equal counts by ascending image index (COLMAP leaves them to an unordered map)
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return shared[a] > shared[b]; });
  const int32_t n_over = (int32_t)order.size();
  const int32_t E = std::min(N, n_over);
  if (n_over == E) {
    for (int32_t i = 0; i < E; ++i) bundle[i] = order[i];
    return E;
  }
  std::vector<uint8_t> taken((size_t)n_over, 0);
  int32_t len = 0;
  for (int t = 0; t < kLocalBundleThresholds && len < E; ++t) {
    const double min_angle = min_tri_angle_rad / kLocalBundleAngleDiv[t];
    const double min_shared = kLocalBundleSharedRatio[t] * (double)T;
    for (int32_t i = 0; i < n_over && len < E; ++i) {
      const int32_t j = order[i];
      if ((double)shared[j] < min_shared) break;  // the order is by shared: nothing behind it reaches the number either
      if (taken[i]) continue;
      if (angle75[j] >= min_angle) {
        taken[i] = 1;
        bundle[len++] = j;
      }
    }
  }
  for (int32_t i = 0; i < n_over && len < E; ++i)
    if (!taken[i]) {
      taken[i] = 1;
      bundle[len++] = order[i];
    }
  return len;
}

}  // namespace mpsfm
