// Calibrated two-view geometry of one image pair (mpsfm_two_view_geometry; semantics and what is unpinned:
// include/mpsfm_hip.h): three LO-RANSACs over the same matches with the same seed (E on normalised points, F and H on
// pixels), COLMAP's decision between them, the watermark test and the relative pose with its triangulation angle.  The
// loop, the scoring kernels and the batch tables are lo_ransac.h's; the E leg is RpProblem (rel_pose_problem.h).  The
// kernels of the F, H and translation legs, the pose kernel and the host stages between the legs are two_view_problem.h's,
// shared with mpsfm_two_view_geometry_batch (two_view_batch.hip).
#include "two_view_problem.h"

using namespace mpsfm;

extern "C" void mpsfm_two_view_default_options(mpsfm_two_view_options* o) {
  if (!o) return;
  *o = mpsfm_two_view_options{};
  o->ransac.max_error = 4.0;
  o->ransac.min_inlier_ratio = 0.25;
  o->ransac.confidence = 0.999;
  o->ransac.dyn_num_trials_multiplier = 3.0;
  o->ransac.min_num_trials = 100;
  o->ransac.max_num_trials = 10000;
  o->min_num_inliers = 15;
  o->min_E_F_inlier_ratio = 0.95;
  o->max_H_inlier_ratio = 0.8;
  o->watermark_min_inlier_ratio = 0.7;
  o->watermark_border_size = 0.1;
  o->detect_watermark = 1;
  o->compute_relative_pose = 0;
}

extern "C" int mpsfm_two_view_geometry(int64_t n64, const double* points1, const double* points2, const double* intr1, const double* intr2,
                                       const int32_t* size1, const int32_t* size2, const mpsfm_two_view_options* o, int32_t device,
                                       uint8_t* inlier_mask, mpsfm_two_view_result* result) {
  if (result) {
    *result = mpsfm_two_view_result{};
    for (int r = 0; r < 3; ++r) result->cam2_from_cam1[5 * r] = 1.0;
  }
  if (!points1 || !points2 || !intr1 || !intr2 || !size1 || !size2 || !o || !inlier_mask || !result) return fail(MPSFM_EINVAL, "NULL pointer");
  if (n64 < 0) return fail(MPSFM_EINVAL, "negative number of correspondences");
  if (n64 > INT32_MAX) return fail(MPSFM_EINVAL, "more than INT32_MAX correspondences (int32 indexing)");
  const int32_t n = (int32_t)n64;
  if (!finite_all(points1, 2 * (size_t)n) || !finite_all(points2, 2 * (size_t)n)) return fail(MPSFM_EINVAL, "non-finite point");
  if (const char* why = tv_cameras_invalid(intr1, intr2, size1, size2)) return fail(MPSFM_EINVAL, why);
  if (!tv_options_valid(*o)) return fail(MPSFM_EINVAL, "invalid two-view geometry options");
  if (int rc = open_device(device)) return rc;

  result->config = MPSFM_TVG_DEGENERATE;
  std::memset(inlier_mask, 0, (size_t)n);
  if (n < o->min_num_inliers || n < kTvHSample) return 0;

  // SoA blocks u1 v1 u2 v2: pixels (F, H, watermark) and CamFromImg of both PINHOLE cameras (E, pose)
  const double max_error = o->ransac.max_error;
  const double thrE = 0.5 * (max_error / ((intr1[0] + intr1[1]) / 2.0) + max_error / ((intr2[0] + intr2[1]) / 2.0));
  std::vector<double> hpx((size_t)4 * n), hnm((size_t)4 * n);
  for (int32_t i = 0; i < n; ++i) {
    const double a = points1[2 * (size_t)i], b = points1[2 * (size_t)i + 1], c = points2[2 * (size_t)i], d = points2[2 * (size_t)i + 1];
    hpx[i] = a; hpx[(size_t)n + i] = b; hpx[2 * (size_t)n + i] = c; hpx[3 * (size_t)n + i] = d;
    hnm[i] = (a - intr1[2]) / intr1[0];
    hnm[(size_t)n + i] = (b - intr1[3]) / intr1[1];
    hnm[2 * (size_t)n + i] = (c - intr2[2]) / intr2[0];
    hnm[3 * (size_t)n + i] = (d - intr2[3]) / intr2[1];
  }

  CallScope A;
  if (int rc = A.open(true)) return rc;
  double* d_px = A.alloc<double>(4 * (size_t)n);
  double* d_nm = A.alloc<double>(4 * (size_t)n);
  uint8_t* d_mask = A.alloc<uint8_t>(3 * (size_t)n);  // E, F, H
  if (!d_px || !d_nm || !d_mask) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  MPSFM_TRY(hipMemcpyAsync(d_px, hpx.data(), sizeof(double) * 4 * (size_t)n, hipMemcpyHostToDevice, A.st));
  MPSFM_TRY(hipMemcpyAsync(d_nm, hnm.data(), sizeof(double) * 4 * (size_t)n, hipMemcpyHostToDevice, A.st));
  MPSFM_TRY(hipMemsetAsync(d_mask, 0, 3 * (size_t)n, A.st));

  RpProblem pe;
  TvProblem<false> pf;
  TvProblem<true> ph;
  if (int rc = tv_setup(pe, A, d_nm, n, thrE * thrE, kGramK)) return rc;
  if (int rc = tv_setup(pf, A, d_px, n, max_error * max_error, kGram9K)) return rc;
  if (int rc = tv_setup(ph, A, d_px, n, max_error * max_error, kGram9K)) return rc;

  // the three legs: the same options and the same seed
  LoReport re, rf, rh;
  double E[9] = {}, F[9] = {}, H[9] = {};
  mpsfm_ransac_options oe = o->ransac;
  if (oe.batch_trials == 0) oe.batch_trials = kTvEBatch;
  if (n >= kRpSample)
    if (int rc = lo_ransac(pe, A, oe, re, E)) return rc;
  if (n >= kTvFSample)
    if (int rc = lo_ransac(pf, A, o->ransac, rf, F)) return rc;
  if (int rc = lo_ransac(ph, A, o->ransac, rh, H)) return rc;
  mpsfm_two_view_leg* legs = result->leg;
  tv_fill_leg(legs[MPSFM_TVG_LEG_E], re, kRpSample);
  tv_fill_leg(legs[MPSFM_TVG_LEG_F], rf, kTvFSample);
  tv_fill_leg(legs[MPSFM_TVG_LEG_H], rh, kTvHSample);
  const bool okE = legs[MPSFM_TVG_LEG_E].success, okF = legs[MPSFM_TVG_LEG_F].success, okH = legs[MPSFM_TVG_LEG_H].success;
  if (okE) std::memcpy(result->E, E, sizeof(E));
  if (okF) std::memcpy(result->F, F, sizeof(F));
  if (okH) std::memcpy(result->H, H, sizeof(H));

  // RANSAC's masks of the three best models (zeros for a leg without a model)
  std::vector<uint8_t> hmask(3 * (size_t)n);
  if (int rc = A.begin()) return rc;
  if (okE)
    if (int rc = lo_mask(pe, A, E, d_mask)) return rc;
  if (okF)
    if (int rc = lo_mask(pf, A, F, d_mask + n)) return rc;
  if (okH)
    if (int rc = lo_mask(ph, A, H, d_mask + 2 * (size_t)n)) return rc;
  MPSFM_TRY(hipMemcpyAsync(hmask.data(), d_mask, 3 * (size_t)n, hipMemcpyDeviceToHost, A.st));
  if (int rc = A.end()) return rc;

  // EstimateCalibratedTwoViewGeometry's decision
  int config = MPSFM_TVG_DEGENERATE, chosen = -1;  // chosen: 0 E, 1 F, 2 H
  tv_decide(*o, okE, okF, okH, re.best.num_inliers, rf.best.num_inliers, rh.best.num_inliers, config, chosen);
  result->config = config;
  if (chosen < 0) {
    result->ms = (float)A.ms;
    return 0;
  }
  const uint8_t* sel = hmask.data() + (size_t)chosen * n;
  const uint8_t* d_sel = d_mask + (size_t)chosen * n;
  std::memcpy(inlier_mask, sel, (size_t)n);
  int64_t nsel = 0;
  for (int32_t i = 0; i < n; ++i) nsel += sel[i];
  result->num_inliers = nsel;

  // DetectWatermark: chosen inliers outside the border box in both images, then a translation LO-RANSAC over them
  if (o->detect_watermark) {
    std::vector<int32_t> border;
    tv_border(*o, hpx.data(), n, sel, size1, size2, border);
    const int32_t m = (int32_t)border.size();
    result->num_border_inliers = m;
    if (m > 0 && (double)m / (double)nsel >= o->watermark_min_inlier_ratio) {
      std::vector<double> hb((size_t)4 * m);
      for (int32_t j = 0; j < m; ++j)
        for (int k = 0; k < 4; ++k) hb[(size_t)k * m + j] = hpx[(size_t)k * n + border[(size_t)j]];
      double* d_b = A.alloc<double>(4 * (size_t)m);
      if (!d_b) return fail(MPSFM_ENOMEM, "hipMalloc failed");
      MPSFM_TRY(hipMemcpyAsync(d_b, hb.data(), sizeof(double) * 4 * (size_t)m, hipMemcpyHostToDevice, A.st));
      TvTranslation pt;
      if (int rc = tv_setup(pt, A, d_b, m, max_error * max_error, kTsumK)) return rc;
      mpsfm_ransac_options ow = o->ransac;
      ow.min_inlier_ratio = o->watermark_min_inlier_ratio;
      LoReport rt;
      double T[2] = {};
      if (int rc = lo_ransac(pt, A, ow, rt, T)) return rc;
      tv_fill_leg(legs[MPSFM_TVG_LEG_T], rt, 1);
      if ((double)rt.best.num_inliers / (double)nsel >= o->watermark_min_inlier_ratio) {
        config = MPSFM_TVG_WATERMARK;
        result->watermark = 1;
      }
    }
  }
  result->config = config;

  // EstimateTwoViewGeometryPose
  const bool from_E = config == MPSFM_TVG_CALIBRATED || config == MPSFM_TVG_UNCALIBRATED;
  if (o->compute_relative_pose && (from_E || config == MPSFM_TVG_PLANAR_OR_PANORAMIC)) {
    TvCands cand{};
    tv_pose_cands(config, E, F, H, intr1, intr2, cand);
    const int npx = pe.npx;
    int32_t* d_ipart = A.alloc<int32_t>(4 * (size_t)npx);
    double* d_angle = A.alloc<double>(4 * (size_t)n);
    if (!d_ipart || !d_angle) return fail(MPSFM_ENOMEM, "hipMalloc failed");
    std::vector<int32_t> h_ipart((size_t)4 * npx);
    if (int rc = A.begin()) return rc;
    hipLaunchKernelGGL(k_tv_pose, dim3((unsigned)npx), dim3(kLoT), 0, A.st, cand, n, pe.pts, d_sel, d_ipart, d_angle);
    MPSFM_TRY(hipGetLastError());
    MPSFM_TRY(hipMemcpyAsync(h_ipart.data(), d_ipart, sizeof(int32_t) * 4 * (size_t)npx, hipMemcpyDeviceToHost, A.st));
    if (int rc = A.end()) return rc;
    int64_t count[4];
    sum_rows(h_ipart.data(), npx, 4, count);
    int64_t bestc = -1;
    const int bk = tv_pose_winner(cand, count, bestc);
    std::vector<double> ang((size_t)n);
    MPSFM_TRY(A.down(ang.data(), d_angle + (size_t)bk * n, sizeof(double) * (size_t)n));
    tv_pose_finish(*result, cand, bk, bestc, ang, from_E, config);
    result->config = config;
  }
  result->success = 1;
  result->ms = (float)A.ms;
  return 0;
}
