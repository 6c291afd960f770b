// Relative-pose LO-RANSAC of one two-view problem (mpsfm_rel_pose_estimate; semantics and what is unpinned:
// include/mpsfm_hip.h).  The loop, the scoring kernels and the batch tables are lo_ransac.h's; this file describes the
// problem to it:
//   k_rp_five         one thread per trial of a batch: the trial's five-index sample, the five-point solver with its
//                     runtime-indexed arrays in a per-thread LDS slice (rel_pose_math.h), up to 10 canonical models in
//                     lexicographic order (zeros pad: a zero E scores no inlier)
//   RpProblem::local  the five-point estimator on the inliers of a model: k_rp_gram (Q^T Q, upper 45 entries, and the
//                     count) on the device, its 9 x 9 eigenvectors and the five-point algebra on the host
// and normalises the inputs, decomposes the final E and fills the result:
//   k_rp_cheirality   the four (R, t) candidates of the final E against every inlier in one pass (two-view DLT, depth test)
// f64 throughout.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "rel_pose_problem.h"

using namespace mpsfm;

extern "C" int mpsfm_rel_pose_estimate(int64_t n64, const double* points1, const double* points2, const double* intr1, const double* intr2,
                                       const mpsfm_rel_pose_options* o, int32_t device, uint8_t* inlier_mask, mpsfm_rel_pose_result* result) {
  if (result) *result = mpsfm_rel_pose_result{};
  if (!points1 || !points2 || !intr1 || !intr2 || !o || !inlier_mask || !result) return fail(MPSFM_EINVAL, "NULL pointer");
  if (n64 < kRpSample) return fail(MPSFM_EINVAL, "fewer than 5 correspondences");
  if (n64 > INT32_MAX) return fail(MPSFM_EINVAL, "more than INT32_MAX correspondences (int32 indexing)");
  const int32_t n = (int32_t)n64;
  if (!finite_all(points1, 2 * (size_t)n) || !finite_all(points2, 2 * (size_t)n)) return fail(MPSFM_EINVAL, "non-finite point");
  for (const double* K : {intr1, intr2})
    if (!finite_all(K, 4) || K[0] == 0.0 || K[1] == 0.0 || K[0] + K[1] == 0.0)
      return fail(MPSFM_EINVAL, "intrinsics must be finite with non-zero focal lengths");
  if (!lo_options_valid(*o)) return fail(MPSFM_EINVAL, "invalid RANSAC options");
  if (int rc = open_device(device)) return rc;

  // EstimateEssentialMatrix: CamFromImg of both PINHOLE cameras, the mean of their normalised thresholds
  const double thr = 0.5 * (o->max_error / ((intr1[0] + intr1[1]) / 2.0) + o->max_error / ((intr2[0] + intr2[1]) / 2.0));
  const double thr2 = thr * thr;
  std::vector<double> hs((size_t)4 * n);  // SoA: u1 v1 u2 v2
  for (int32_t i = 0; i < n; ++i) {
    hs[i] = (points1[2 * (size_t)i] - intr1[2]) / intr1[0];
    hs[(size_t)n + i] = (points1[2 * (size_t)i + 1] - intr1[3]) / intr1[1];
    hs[2 * (size_t)n + i] = (points2[2 * (size_t)i] - intr2[2]) / intr2[0];
    hs[3 * (size_t)n + i] = (points2[2 * (size_t)i + 1] - intr2[3]) / intr2[1];
  }

  CallScope A;
  if (int rc = A.open(true)) return rc;
  RpProblem prob;
  prob.n = n;
  prob.thr2 = thr2;
  prob.npx = lo_blocks(n, kT);
  const int npx = prob.npx;
  double* d_pts = A.alloc<double>(4 * (size_t)n);
  prob.d_part = A.alloc<double>(kGramK * (size_t)npx);
  int32_t* d_ipart = A.alloc<int32_t>(4 * (size_t)npx);
  uint8_t* d_mask = A.alloc<uint8_t>((size_t)n);
  if (!d_pts || !prob.d_part || !d_ipart || !d_mask) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  MPSFM_TRY(hipMemcpyAsync(d_pts, hs.data(), sizeof(double) * 4 * (size_t)n, hipMemcpyHostToDevice, A.st));
  prob.pts = RpPts{d_pts, d_pts + n, d_pts + 2 * (size_t)n, d_pts + 3 * (size_t)n};
  prob.h_part.resize((size_t)kGramK * npx);
  std::vector<int32_t> h_ipart((size_t)4 * npx);

  LoReport rep;
  double best_model[9] = {};
  if (int rc = lo_ransac(prob, A, *o, rep, best_model)) return rc;
  result->num_trials = rep.num_trials;
  result->max_num_trials = rep.max_num_trials;
  result->num_models = rep.num_models;
  result->lo_rounds = rep.lo_rounds;
  result->num_batches = rep.num_batches;
  if (rep.best.num_inliers < kRpSample) {
    result->ms = (float)A.ms;
    std::memset(inlier_mask, 0, (size_t)n);
    return 0;
  }
  // RANSAC's mask of the best model, then PoseFromEssentialMatrix on its inliers
  RpCands cand;
  double R1[9], R2[9], t[3];
  rp_decompose(best_model, R1, R2, t);
  for (int k = 0; k < 4; ++k) {
    const double* R = (k % 2 == 0) ? R1 : R2;
    const double sg = k < 2 ? 1.0 : -1.0;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) cand.P[k][4 * r + c] = R[3 * r + c];
      cand.P[k][4 * r + 3] = sg * t[r];
    }
    cand.max_depth[k] = 1000.0 * std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
  }
  if (int rc = A.begin()) return rc;
  if (int rc = lo_mask(prob, A, best_model, d_mask)) return rc;
  hipLaunchKernelGGL(k_rp_cheirality, dim3((unsigned)npx), dim3(kT), 0, A.st, cand, n, prob.pts, d_mask, d_ipart);
  MPSFM_TRY(hipGetLastError());
  MPSFM_TRY(hipMemcpyAsync(inlier_mask, d_mask, (size_t)n, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipMemcpyAsync(h_ipart.data(), d_ipart, sizeof(int32_t) * 4 * (size_t)npx, hipMemcpyDeviceToHost, A.st));
  if (int rc = A.end()) return rc;
  int64_t count[4];
  sum_rows(h_ipart.data(), npx, 4, count);
  int64_t bestc = -1;
  int bk = 0;
  for (int k = 0; k < 4; ++k)
    if (count[k] >= bestc) { bestc = count[k]; bk = k; }  // the later candidate wins a tie
  std::memcpy(result->E, best_model, sizeof(best_model));
  std::memcpy(result->cam2_from_cam1, cand.P[bk], sizeof(cand.P[bk]));
  result->num_inliers = rep.best.num_inliers;
  result->num_cheirality_points = bestc;
  result->success = 1;
  result->ms = (float)A.ms;
  return 0;
}
