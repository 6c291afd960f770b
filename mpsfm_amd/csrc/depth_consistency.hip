// Depth-consistency check of a newly registered image against its local bundle (reference
// mpsfm/sfm/mapper/depthconsistency.py:62-159 check_depth_consistency, :224-246 check_bundle_depth_concistency, with
// reconstruction/mixins/depth_utils.py:9-48 reproject_depth and points3D_utils.py:27-62 for the lifted covariances).
// A call takes an image table and a list of pairs; every pair has two legs (a -> b and b -> a) and all legs of the call
// share one sequence of launches with the leg as the grid's y index:
//   memset     winner buffers to -1, counters to 0
//   k_dc_project   one thread per source pixel: project into the other image, write the target pixel (or -1) and the
//                  depth there, atomicMax(winner[target], source index).  The reference's z-buffer `find_min_buffer`
//                  compares against an all-inf buffer, so its fancy-index assignment keeps the LAST writer in raster
//                  order: the largest source index, whatever its depth.
//   k_dc_classify  one thread per source pixel: gather the winner's depth at the target, the lifted depth covariance
//                  rotated into the other camera in closed form, the test value t and its class; one code byte per pixel
//                  (bit 0 in canvas, 1 surface, 2 occluded, 3 invalid) and per-wave ballot counts, one 64-bit integer
//                  atomic per wave and counter (exact, identical on every run).
// f64 throughout; NaN / inf test values classify as IEEE comparisons do (no fast-math: build.py does not pass it).
#include <string>
#include <vector>

#include "call_scope.h"
#include "common.h"

namespace mpsfm {

namespace {
constexpr int kT = 256;

enum { DC_IN = 1, DC_SURFACE = 2, DC_OCCL = 4, DC_INVALID = 8 };

struct DcLeg {
  int32_t Hs, Ws, Hd, Wd;   // source and target map sizes
  int64_t src_off, dst_off;  // into the concatenated depth / variance maps
  int64_t pix_off;           // into the per-leg source-pixel arrays (target index, depth there, code)
  int64_t win_off;           // into the per-leg winner buffers (target map size)
  double A[9];               // R_d R_s^T K_s^-1 (map intrinsics): camera-d point = depth * A (x, y, 1) + tb
  double tb[3];              // t_d - R_d R_s^T t_s
  double kd[4];              // target map intrinsics fx fy cx cy (scaled by sx, sy)
  double ks[4];              // source camera intrinsics, unscaled (lifted covariance at map coordinates, as the reference)
  double m[3];               // row 2 of R_d^T R_s: std_bar^2 = m^T C m (rotate_covs_to_world, then _to_cam)
  double psm_s, psm_d;       // depth.conf.prior_std_multiplier of source and target
};

__global__ __launch_bounds__(kT) void k_dc_project(const DcLeg* __restrict__ legs, const double* __restrict__ depth,
                                                    int32_t* __restrict__ tgt, double* __restrict__ dep, int32_t* __restrict__ win) {
  const DcLeg& L = legs[blockIdx.y];
  const int32_t n = L.Hs * L.Ws;
  const int32_t i = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  if (i >= n) return;
  const double x = (double)(i % L.Ws), y = (double)(i / L.Ws);
  const double d = depth[L.src_off + i];
  const double rx = L.A[0] * x + L.A[1] * y + L.A[2];
  const double ry = L.A[3] * x + L.A[4] * y + L.A[5];
  const double rz = L.A[6] * x + L.A[7] * y + L.A[8];
  const double X = d * rx + L.tb[0], Y = d * ry + L.tb[1], Z = d * rz + L.tb[2];
  const double px = L.kd[0] * (X / Z) + L.kd[2];
  const double py = L.kd[1] * (Y / Z) + L.kd[3];
  // reproject_depth's canvas mask (depth_utils.py:36-43); NaN fails every comparison
  const bool in = px >= 0.0 && px + 0.5 < (double)L.Wd && py >= 0.0 && py + 0.5 < (double)L.Hd && Z > 0.0;
  const int32_t t = in ? (int32_t)py * L.Wd + (int32_t)px : -1;  // truncation, as .astype(int)
  tgt[L.pix_off + i] = t;
  dep[L.pix_off + i] = Z;
  if (in) atomicMax(win + L.win_off + t, i);
}

__device__ __forceinline__ double clip1e6(double v) { return v < -1e6 ? -1e6 : (v > 1e6 ? 1e6 : v); }  // np.clip keeps NaN

__global__ __launch_bounds__(kT) void k_dc_classify(const DcLeg* __restrict__ legs, const double* __restrict__ depth,
                                                     const double* __restrict__ var, const int32_t* __restrict__ tgt,
                                                     const double* __restrict__ dep, const int32_t* __restrict__ win,
                                                     uint8_t* __restrict__ codes, unsigned long long* __restrict__ counts,
                                                     double c, double s) {
  const DcLeg& L = legs[blockIdx.y];
  const int32_t n = L.Hs * L.Ws;
  if ((int32_t)blockIdx.x * kT >= n) return;  // whole block past the map: uniform exit, the ballots below see full waves
  const int32_t i = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  uint32_t code = 0;
  if (i < n) {
    const int32_t t = tgt[L.pix_off + i];
    if (t >= 0) {
      code = DC_IN;
      const double buf = dep[L.pix_off + win[L.win_off + t]];  // the winner's depth, not this pixel's
      const double d2 = depth[L.dst_off + t];
      const double std2 = sqrt(var[L.dst_off + t] / (L.psm_d * L.psm_d));
      // lifted_pointcovs_cam at map coordinates with the unscaled intrinsics, sigma_q = 1:
      //   C = var u u^T + diag(a^2, b^2, 0),  u = ((x - cx) / fx, (y - cy) / fy, 1),  a = clip(d / fx), b = clip(d / fy)
      const double x = (double)(i % L.Ws), y = (double)(i / L.Ws);
      const double d = depth[L.src_off + i];
      const double v1 = var[L.src_off + i] / (L.psm_s * L.psm_s);
      const double ifx = 1.0 / L.ks[0], ify = 1.0 / L.ks[1];
      const double ux = (x - L.ks[2]) * ifx, uy = (y - L.ks[3]) * ify;
      const double a = clip1e6(d * ifx), b = clip1e6(d * ify);
      const double mu = L.m[0] * ux + L.m[1] * uy + L.m[2];
      const double s1sq = v1 * (mu * mu) + (L.m[0] * L.m[0]) * (a * a) + (L.m[1] * L.m[1]) * (b * b);
      const double e1 = sqrt(s1sq) * c, e2 = std2 * c;
      const double tv = (buf - d2) / sqrt(e1 * e1 + e2 * e2);
      if (fabs(tv) < s) code |= DC_SURFACE;
      if (tv > s) code |= DC_OCCL;
      if (tv < -s) code |= DC_INVALID;
    }
    if (codes) codes[L.pix_off + i] = (uint8_t)code;
  }
  unsigned long long* cnt = counts + 4 * (size_t)blockIdx.y;
  const bool leader = (threadIdx.x & 63) == 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned long long bal = __ballot((code >> k) & 1u);
    if (leader && bal) atomicAdd(cnt + k, (unsigned long long)__popcll(bal));
  }
}

// 3x3 row-major helpers (host)
void mat3_mul(const double* A, const double* B, double* C) {
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k) C[3 * r + k] = A[3 * r] * B[k] + A[3 * r + 1] * B[3 + k] + A[3 * r + 2] * B[6 + k];
}

void make_leg(const mpsfm_dc_image& S, const mpsfm_dc_image& D, DcLeg& L) {
  L.Hs = S.H; L.Ws = S.W; L.Hd = D.H; L.Wd = D.W;
  double Rs[9], Rd[9], RsT[9], M[9], ts[3], td[3];
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) { Rs[3 * r + k] = S.cam_from_world[4 * r + k]; Rd[3 * r + k] = D.cam_from_world[4 * r + k]; }
    ts[r] = S.cam_from_world[4 * r + 3];
    td[r] = D.cam_from_world[4 * r + 3];
  }
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k) RsT[3 * r + k] = Rs[3 * k + r];
  mat3_mul(Rd, RsT, M);  // camera s -> camera d
  const double fx = S.intr_scaled[0], fy = S.intr_scaled[1], cx = S.intr_scaled[2], cy = S.intr_scaled[3];
  const double Kinv[9] = {1.0 / fx, 0.0, -cx / fx, 0.0, 1.0 / fy, -cy / fy, 0.0, 0.0, 1.0};
  mat3_mul(M, Kinv, L.A);
  for (int r = 0; r < 3; ++r) L.tb[r] = td[r] - (M[3 * r] * ts[0] + M[3 * r + 1] * ts[1] + M[3 * r + 2] * ts[2]);
  for (int k = 0; k < 4; ++k) { L.kd[k] = D.intr_scaled[k]; L.ks[k] = S.intr[k]; }
  // m_k = (R_d^T R_s)[2][k] = sum_j R_d[j][2] R_s[j][k]
  for (int k = 0; k < 3; ++k) L.m[k] = Rd[2] * Rs[k] + Rd[5] * Rs[3 + k] + Rd[8] * Rs[6 + k];
  L.psm_s = S.prior_std_multiplier;
  L.psm_d = D.prior_std_multiplier;
}
}  // namespace

}  // namespace mpsfm

using namespace mpsfm;

extern "C" int mpsfm_depth_consistency(int32_t n_images, mpsfm_dc_image* images, int32_t n_pairs, const int32_t* pair_a,
                                       const int32_t* pair_b, double c, double score_thresh, int32_t device, int64_t* counts,
                                       uint8_t* const* codes, mpsfm_dc_summary* summary) {
  if (summary) *summary = mpsfm_dc_summary{};
  if (n_images < 0 || n_pairs < 0) return fail(MPSFM_EINVAL, "negative size");
  if (n_pairs == 0) return 0;
  if (!images || !pair_a || !pair_b || !counts) return fail(MPSFM_EINVAL, "NULL pointer");
  if (n_pairs > 32767) return fail(MPSFM_EINVAL, "more than 32767 pairs (legs are the grid's y dimension)");
  std::vector<uint8_t> used((size_t)n_images, 0);
  for (int32_t p = 0; p < n_pairs; ++p) {
    const int32_t a = pair_a[p], b = pair_b[p];
    if (a < 0 || a >= n_images || b < 0 || b >= n_images) return fail(MPSFM_EINVAL, "pair index out of range");
    if (a == b) return fail(MPSFM_EINVAL, "a pair of an image with itself");
    used[(size_t)a] = used[(size_t)b] = 1;
  }
  int64_t npix = 0;
  std::vector<int64_t> off((size_t)n_images, -1);
  for (int32_t k = 0; k < n_images; ++k) {
    if (!used[(size_t)k]) continue;
    const mpsfm_dc_image& I = images[k];
    if (I.H <= 0 || I.W <= 0) return fail(MPSFM_EINVAL, "non-positive map size");
    if ((int64_t)I.H * I.W > (int64_t)1 << 30) return fail(MPSFM_EINVAL, "map larger than 2^30 pixels");
    if (!I.depth || !I.variance) return fail(MPSFM_EINVAL, "depth or variance map is NULL");
    off[(size_t)k] = npix;
    npix += (int64_t)I.H * I.W;
  }
  if (int rc = open_device(device)) return rc;

  const int32_t n_legs = 2 * n_pairs;
  std::vector<DcLeg> legs((size_t)n_legs);
  int64_t pix = 0, wpix = 0, max_src = 0;
  for (int32_t p = 0; p < n_pairs; ++p)
    for (int e = 0; e < 2; ++e) {
      const int32_t s = e ? pair_b[p] : pair_a[p], d = e ? pair_a[p] : pair_b[p];
      DcLeg& L = legs[2 * (size_t)p + e];
      make_leg(images[s], images[d], L);
      L.src_off = off[(size_t)s];
      L.dst_off = off[(size_t)d];
      L.pix_off = pix;
      L.win_off = wpix;
      pix += (int64_t)L.Hs * L.Ws;
      wpix += (int64_t)L.Hd * L.Wd;
      max_src = std::max(max_src, (int64_t)L.Hs * L.Ws);
    }

  CallScope B;
  if (int rc = B.open(true)) return rc;
  double* d_depth = B.alloc<double>((size_t)npix);
  double* d_var = B.alloc<double>((size_t)npix);
  DcLeg* d_legs = B.alloc<DcLeg>(legs.size());
  int32_t* d_tgt = B.alloc<int32_t>((size_t)pix);
  double* d_dep = B.alloc<double>((size_t)pix);
  int32_t* d_win = B.alloc<int32_t>((size_t)wpix);
  uint8_t* d_codes = codes ? B.alloc<uint8_t>((size_t)pix) : nullptr;
  unsigned long long* d_cnt = B.alloc<unsigned long long>(4 * (size_t)n_legs);
  if (!d_depth || !d_var || !d_legs || !d_tgt || !d_dep || !d_win || (codes && !d_codes) || !d_cnt)
    return fail(MPSFM_ENOMEM, "hipMalloc failed");

  // reproject_depth clamps the caller's map in place (`depth1[depth1 <= 0] = 0.1`, depth_utils.py:18) for both images of
  // every pair; the clamped maps are what the kernels read.  Each image is uploaded once, however many pairs it is in.
  for (int32_t k = 0; k < n_images; ++k) {
    if (!used[(size_t)k]) continue;
    mpsfm_dc_image& I = images[k];
    const size_t n = (size_t)I.H * I.W;
    for (size_t j = 0; j < n; ++j)
      if (I.depth[j] <= 0.0) I.depth[j] = 0.1;
    if (int rc = staged_upload(d_depth + off[(size_t)k], I.depth, sizeof(double) * n)) return rc;
    if (int rc = staged_upload(d_var + off[(size_t)k], I.variance, sizeof(double) * n)) return rc;
  }
  if (int rc = staged_upload(d_legs, legs.data(), sizeof(DcLeg) * legs.size())) return rc;
  if (int rc = staged_drain()) return rc;

  const dim3 grid((unsigned)((max_src + kT - 1) / kT), (unsigned)n_legs);
  if (int rc = B.begin()) return rc;
  MPSFM_TRY(hipMemsetAsync(d_win, 0xFF, sizeof(int32_t) * (size_t)wpix, B.st));
  MPSFM_TRY(hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long) * 4 * (size_t)n_legs, B.st));
  hipLaunchKernelGGL(k_dc_project, grid, dim3(kT), 0, B.st, d_legs, d_depth, d_tgt, d_dep, d_win);
  MPSFM_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_dc_classify, grid, dim3(kT), 0, B.st, d_legs, d_depth, d_var, d_tgt, d_dep, d_win, d_codes, d_cnt, c,
                     score_thresh);
  MPSFM_TRY(hipGetLastError());
  if (int rc = B.stop()) return rc;
  static_assert(sizeof(int64_t) == sizeof(unsigned long long), "counts are 64-bit");
  MPSFM_TRY(hipMemcpyAsync(counts, d_cnt, sizeof(int64_t) * 4 * (size_t)n_legs, hipMemcpyDeviceToHost, B.st));
  if (codes)
    for (int32_t l = 0; l < n_legs; ++l)
      if (codes[l])
        MPSFM_TRY(hipMemcpyAsync(codes[l], d_codes + legs[(size_t)l].pix_off, (size_t)legs[(size_t)l].Hs * legs[(size_t)l].Ws,
                              hipMemcpyDeviceToHost, B.st));
  MPSFM_TRY(hipStreamSynchronize(B.st));
  if (summary) {
    float ms = 0.f;
    if (int rc = B.elapsed(&ms)) return rc;
    summary->ms = ms;
    summary->n_legs = n_legs;
    summary->n_pixels = pix;
  }
  return 0;
}
