// The host half of mpsfm_filter_scene (scene_filter.hip): the argument checks, which run before any device is touched, and the
// empty answer.  The rules are stated in include/mpsfm_hip.h.  Plain C++ and no HIP: a stand-alone program drives every refusal
// under the host sanitizers (scripts/check_scene_filter_host.cpp).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/mpsfm_hip.h"

namespace mpsfm {

struct SceneFilterShape {
  int64_t n_kp = 0, n_points = 0;
  int32_t n_bundle = 0;  // images of the bundle; 0: no risky set (in_bundle or kp_invalid_depth missing, or no image marked)
};

inline bool sf_all_finite(const double* a, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(a[i])) return false;
  return true;
}

// 0, or the status code with *why pointing at a literal
inline int scene_filter_check(const mpsfm_tri_graph* g, const mpsfm_tri_state* st, const uint8_t* in_bundle, const uint8_t* kp_invalid_depth,
                              const mpsfm_scene_filter_options* o, const uint8_t* kp_deleted, const uint8_t* point_fate,
                              const uint8_t* point_risky, SceneFilterShape& s, const char** why) {
  auto refuse = [&](int code, const char* m) { *why = m; return code; };
  if (!g || !st || !o) return refuse(MPSFM_EINVAL, "NULL pointer");
  if (g->n_images < 0) return refuse(MPSFM_EINVAL, "negative size");
  if (!g->kp_start) return refuse(MPSFM_EINVAL, "NULL pointer");
  if (!std::isfinite(o->max_reproj_error) || !(o->max_reproj_error >= 0.0)) return refuse(MPSFM_EINVAL, "max_reproj_error must be finite and not negative");
  if (!std::isfinite(o->min_tri_angle_rad) || !(o->min_tri_angle_rad >= 0.0) || !std::isfinite(o->risky_min_tri_angle_rad) ||
      !(o->risky_min_tri_angle_rad >= 0.0))
    return refuse(MPSFM_EINVAL, "the triangulation angles must be finite and not negative");
  if (o->negative_depth != 0 && o->negative_depth != 1) return refuse(MPSFM_EINVAL, "negative_depth must be 0 or 1");
  const int32_t n_images = g->n_images;
  if (g->kp_start[0] != 0) return refuse(MPSFM_EINVAL, "kp_start[0] must be 0");
  for (int32_t i = 0; i < n_images; ++i)
    if (g->kp_start[i + 1] < g->kp_start[i]) return refuse(MPSFM_EINVAL, "kp_start must not decrease");
  if (g->kp_start[n_images] >= (1ll << 31)) return refuse(MPSFM_EUNSUPPORTED, "2^31 keypoints or more");
  s.n_kp = g->kp_start[n_images];
  s.n_points = st->n_points;
  if (s.n_points < 0) return refuse(MPSFM_EINVAL, "n_points is negative");
  if (s.n_points >= (1ll << 31)) return refuse(MPSFM_EUNSUPPORTED, "2^31 points or more");
  if (n_images > 0 && (!g->cam_intr || !st->registered || !st->cam_quat_xyzw || !st->cam_t)) return refuse(MPSFM_EINVAL, "NULL pointer");
  if (s.n_kp > 0 && (!g->kp_xy || !st->kp_point || !kp_deleted)) return refuse(MPSFM_EINVAL, "NULL pointer");
  if (s.n_points > 0 && (!st->xyz || !point_fate || !point_risky)) return refuse(MPSFM_EINVAL, "NULL pointer");
  for (int32_t i = 0; i < n_images; ++i) {
    const bool reg = st->registered[i] != 0;
    for (int64_t k = g->kp_start[i]; k < g->kp_start[i + 1]; ++k) {
      const int64_t p = st->kp_point[k];
      if (p < -1 || p >= s.n_points) return refuse(MPSFM_EINVAL, "kp_point outside [-1, n_points)");
      if (p >= 0 && !reg) return refuse(MPSFM_EINVAL, "a keypoint of an image that is not registered has a point");
    }
    if (reg && (!sf_all_finite(st->cam_quat_xyzw + 4 * (size_t)i, 4) || !sf_all_finite(st->cam_t + 3 * (size_t)i, 3)))
      return refuse(MPSFM_EINVAL, "pose of a registered image is not finite");
  }
  if (!sf_all_finite(g->cam_intr, 4 * (size_t)n_images)) return refuse(MPSFM_EINVAL, "cam_intr is not finite");
  if (!sf_all_finite(st->xyz, 3 * (size_t)s.n_points)) return refuse(MPSFM_EINVAL, "xyz is not finite");
  s.n_bundle = 0;
  if (in_bundle && kp_invalid_depth)
    for (int32_t i = 0; i < n_images; ++i) s.n_bundle += in_bundle[i] ? 1 : 0;
  return 0;
}

// the answer of a call that filters nothing
inline void scene_filter_zero(const SceneFilterShape& s, uint8_t* kp_deleted, uint8_t* point_fate, uint8_t* point_risky, double* point_max_angle,
                              double* kp_sq_err) {
  if (s.n_kp > 0) {
    std::memset(kp_deleted, 0, (size_t)s.n_kp);
    if (kp_sq_err) std::memset(kp_sq_err, 0, sizeof(double) * (size_t)s.n_kp);
  }
  if (s.n_points > 0) {
    std::memset(point_fate, 0, (size_t)s.n_points);
    std::memset(point_risky, 0, (size_t)s.n_points);
    if (point_max_angle) std::memset(point_max_angle, 0, sizeof(double) * (size_t)s.n_points);
  }
}

}  // namespace mpsfm
