// Row f3: the per-image depth-block selection of Optimizer.__build_problem
// (reference mpsfm/sfm/mapper/bundle_adjustment.py:124-161, Appendix B of SURVEY.md) and the whitened log-depth errors
// of update_truncation_multiplier (:295-333) for ALL images of a bundle in one launch:
//   bilinear sample of the validity mask and of the depth map at every keypoint that has a 3-D point
//     (PriorUtils._data_at_kps, mpsfm/sfm/scene/image/mixins/priorutils.py:49-62: torch grid_sample, bilinear,
//      zero padding, align_corners=True, keypoints scaled by camera.sx / sy),
//   the camera-frame depth of that point (Points3DUtils.project_image_3d_points -> geometry.project3D),
//   the masks (valid == 1, depth > 0, scale filter, gross-outlier test) and the loss weights
//     magnitude = d^2 / clip(var, 1e-6),  param = m sqrt(var) / d.
// The mask decisions are booleans compared exactly with the NumPy restatement (which is pinned by vectors computed by
// the reference's own PriorUtils): the interpolation below therefore repeats its arithmetic operation by operation
// with explicitly rounded multiplies and adds (no fused multiply-add contraction).
#include <string>
#include <vector>

#include "common.h"
#include "bilinear_sample.h"  // grid_coord + bilinear, and contraction off for the rest of this file
#include "call_scope.h"

namespace mpsfm {

struct GatherArgs {
  int64_t n_obs;
  const int32_t* H; const int32_t* W; const int64_t* map_off;  // per image
  const double* sx; const double* sy; const double* q; const double* t;
  const double* depth; const uint8_t* valid;                  // concatenated maps
  const int32_t* obs_img; const double* obs_xy; const double* obs_var; const int32_t* obs_pt;
  const double* pts;
  int32_t scale_filter, gross_outliers;
  double factor, mult;
  uint8_t* flags; double* d_out; double* z_out; double* mag; double* par; double* whi;
};

__global__ __launch_bounds__(256) void k_depth_blocks(GatherArgs G) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= G.n_obs) return;
  const int im = G.obs_img[i];
  const int H = G.H[im], W = G.W[im];
  const int64_t off = G.map_off[im];
  const double x = grid_coord(G.obs_xy[2 * i], G.sx[im], W), y = grid_coord(G.obs_xy[2 * i + 1], G.sy[im], H);
  const double v = bilinear(G.valid + off, H, W, x, y);
  const double d = bilinear(G.depth + off, H, W, x, y);
  double R[9];
  quat_to_R(G.q + 4 * im, R);
  const double* X = G.pts + 3 * (size_t)G.obs_pt[i];
  const double z = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + G.t[3 * im + 2];
  const double var = G.obs_var[i];
  uint8_t f = 0;
  if (v == 1.0) f |= 1;
  if (d > 0.0) f |= 2;
  const double div = d / z;
  if (div < G.factor && div > 1.0 / G.factor) f |= 4;
  const double sd = sqrt(var);
  // gross-outlier test of :145-147 (log clipped from below at 1e-6, as the reference writes it)
  const double wh_g = fabs(fmax(log(d), 1e-6) - fmax(log(z), 1e-6)) / sd;
  if (wh_g < 3.0) f |= 8;
  G.flags[i] = f;
  G.d_out[i] = d;
  G.z_out[i] = z;
  G.mag[i] = d * d * (1.0 / fmax(var, 1e-6));
  G.par[i] = G.mult * sd / d;
  // whitened log-depth error of update_truncation_multiplier (:323-329)
  G.whi[i] = (log(d) - log(z)) / fmax(sd / d, 1e-6);
}

}  // namespace mpsfm

using namespace mpsfm;

extern "C" int mpsfm_depth_blocks(const mpsfm_depth_gather* g, int32_t device, uint8_t* flags, double* depth, double* depth3d,
                                  double* magnitude, double* param, double* whitened) {
  if (!g) return fail(MPSFM_EINVAL, "gather descriptor is NULL");
  if (g->n_images < 0 || g->n_obs < 0 || g->n_pts < 0) return fail(MPSFM_EINVAL, "negative size");
  if (g->n_obs == 0) return 0;
  if (!flags || !depth || !depth3d || !magnitude || !param || !whitened) return fail(MPSFM_EINVAL, "output pointer is NULL");
  if (!g->map_h || !g->map_w || !g->depth_map || !g->valid_map || !g->sx || !g->sy || !g->cam_quat_xyzw || !g->cam_t)
    return fail(MPSFM_EINVAL, "image arrays are NULL");
  if (!g->obs_img || !g->obs_xy || !g->obs_var || !g->obs_pt || !g->pts) return fail(MPSFM_EINVAL, "observation arrays are NULL");
  if (!(g->scale_filter_factor > 0.0)) return fail(MPSFM_EINVAL, "scale_filter_factor must be positive");
  std::vector<int64_t> off((size_t)g->n_images + 1, 0);
  for (int i = 0; i < g->n_images; ++i) {
    if (g->map_h[i] < 2 || g->map_w[i] < 2 || !g->depth_map[i] || !g->valid_map[i]) return fail(MPSFM_EINVAL, "map missing or smaller than 2x2");
    off[(size_t)i + 1] = off[(size_t)i] + (int64_t)g->map_h[i] * g->map_w[i];
  }
  for (int64_t i = 0; i < g->n_obs; ++i)
    if (g->obs_img[i] < 0 || g->obs_img[i] >= g->n_images || g->obs_pt[i] < 0 || g->obs_pt[i] >= g->n_pts)
      return fail(MPSFM_EINVAL, "observation index out of range");
  if (int rc = open_device(device)) return rc;
  CallScope B;
  if (int rc = B.open()) return rc;
  const size_t ni = (size_t)g->n_images, no = (size_t)g->n_obs, npix = (size_t)off[ni];
  GatherArgs A{};
  A.n_obs = g->n_obs;
  if (int rc = B.up(&A.H, g->map_h, ni)) return rc;
  if (int rc = B.up(&A.W, g->map_w, ni)) return rc;
  if (int rc = B.up(&A.map_off, off.data(), ni)) return rc;
  if (int rc = B.up(&A.sx, g->sx, ni)) return rc;
  if (int rc = B.up(&A.sy, g->sy, ni)) return rc;
  if (int rc = B.up(&A.q, g->cam_quat_xyzw, 4 * ni)) return rc;
  if (int rc = B.up(&A.t, g->cam_t, 3 * ni)) return rc;
  if (int rc = B.up(&A.obs_img, g->obs_img, no)) return rc;
  if (int rc = B.up(&A.obs_xy, g->obs_xy, 2 * no)) return rc;
  if (int rc = B.up(&A.obs_var, g->obs_var, no)) return rc;
  if (int rc = B.up(&A.obs_pt, g->obs_pt, no)) return rc;
  if (int rc = B.up(&A.pts, g->pts, 3 * (size_t)g->n_pts)) return rc;
  double* d_depth = B.alloc<double>(npix);
  uint8_t* d_valid = B.alloc<uint8_t>(npix);
  if (!d_depth || !d_valid) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  for (size_t i = 0; i < ni; ++i) {
    const size_t n = (size_t)(off[i + 1] - off[i]);
    if (int rc = staged_upload(d_depth + off[i], g->depth_map[i], sizeof(double) * n)) return rc;
    if (int rc = staged_upload(d_valid + off[i], g->valid_map[i], n)) return rc;
  }
  A.depth = d_depth; A.valid = d_valid;
  A.scale_filter = g->scale_filter; A.gross_outliers = g->gross_outliers; A.factor = g->scale_filter_factor; A.mult = g->multiplier;
  A.flags = B.alloc<uint8_t>(no);
  double* outs[5];
  for (auto& o : outs) { o = B.alloc<double>(no); if (!o) return fail(MPSFM_ENOMEM, "hipMalloc failed"); }
  if (!A.flags) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  A.d_out = outs[0]; A.z_out = outs[1]; A.mag = outs[2]; A.par = outs[3]; A.whi = outs[4];
  if (int rc = staged_drain()) return rc;
  hipLaunchKernelGGL(k_depth_blocks, dim3((unsigned)((no + 255) / 256)), dim3(256), 0, B.st, A);
  MPSFM_TRY(hipGetLastError());
  MPSFM_TRY(hipMemcpyAsync(flags, A.flags, no, hipMemcpyDeviceToHost, B.st));
  double* hosts[5] = {depth, depth3d, magnitude, param, whitened};
  for (int k = 0; k < 5; ++k) MPSFM_TRY(hipMemcpyAsync(hosts[k], outs[k], sizeof(double) * no, hipMemcpyDeviceToHost, B.st));
  MPSFM_TRY(hipStreamSynchronize(B.st));
  return 0;
}
