// The per-match arithmetic of image registration (reference mpsfm/sfm/mapper/registration.py), one thread per match:
//   k_reg_pairs        the 2D-3D pairs of register_next_image for all reference images of the call (:68-94, :341-382):
//                      gather of the triangulated point, or bilinear sample of the reference image's depth.data and the lift
//                      into the world frame
//   k_init_candidates  the candidate points of an init pair (:38-66, :384-391, :419-441): the two-view
//                      EstimateTriangulation with the device functions of k_tri_ransac (tri_math.h), the point lifted from
//                      image 1's prior depth, and for both the reference's triangulation angle and positive-depth flags
// f64 throughout.  The work is a gather and about a hundred flops per match (a 4x4 Jacobi eigen-solve for the
// triangulation): a call is bound by its transfers and the launch, not by the CUs.
#include <string>
#include <vector>

#include "common.h"
#include "tri_math.h"         // default contraction, as in triangulator.hip: the two-view estimate equals k_tri_ransac's bit for bit
#include "bilinear_sample.h"  // contraction off from here on: the samples, lifts and angles round every operation on its own
#include "call_scope.h"

namespace mpsfm {

namespace {
constexpr int kT = 256;

struct RegRef {  // one reference image
  int32_t H, W;
  int64_t off;  // into the concatenated depth maps
  double sx, sy;
  double K[4];
  double R[9];  // cam_from_world rotation, row-major
  double t[3];
};

struct RegArgs {
  int64_t n;
  const RegRef* refs;
  const double* depth;
  const int32_t* match_ref; const double* ref_xy; const int32_t* match_pt;
  const uint8_t* risky;  // may be NULL
  const double* pts;
  int32_t lifted;
  double* xyz; uint8_t* kind;
};

__global__ __launch_bounds__(kT) void k_reg_pairs(RegArgs A) {
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (i >= A.n) return;
  const int32_t p = A.match_pt[i];
  double X0 = 0.0, X1 = 0.0, X2 = 0.0;
  uint8_t kind = MPSFM_REG_DROPPED;
  const bool use3d = p >= 0 && !(A.risky && A.risky[p]);
  if (use3d) {
    const double* P = A.pts + 3 * (size_t)p;
    X0 = P[0]; X1 = P[1]; X2 = P[2];
    kind = MPSFM_REG_TRIANGULATED;
  } else if (A.lifted) {
    const RegRef& r = A.refs[A.match_ref[i]];
    const double x = A.ref_xy[2 * i], y = A.ref_xy[2 * i + 1];
    const double d = bilinear(A.depth + r.off, r.H, r.W, grid_coord(x, r.sx, r.W), grid_coord(y, r.sy, r.H));
    // cam_from_world.inverse() * (ray d): R^T (ray d - t)
    const double q0 = (x - r.K[2]) / r.K[0] * d - r.t[0];
    const double q1 = (y - r.K[3]) / r.K[1] * d - r.t[1];
    const double q2 = d - r.t[2];
    X0 = r.R[0] * q0 + r.R[3] * q1 + r.R[6] * q2;
    X1 = r.R[1] * q0 + r.R[4] * q1 + r.R[7] * q2;
    X2 = r.R[2] * q0 + r.R[5] * q1 + r.R[8] * q2;
    kind = MPSFM_REG_LIFTED;
  }
  A.xyz[3 * i] = X0; A.xyz[3 * i + 1] = X1; A.xyz[3 * i + 2] = X2;
  A.kind[i] = kind;
}

struct InitArgs {
  int64_t n;
  const double* xy1; const double* xy2; const uint8_t* select;
  TriView v1, v2;  // P, C, K of the two cameras (tri_make_view on the host); xn / xy are filled per match
  double min_tri_angle, max_residual;
  int32_t H, W;
  const double* prior; const uint8_t* valid;
  double sx, sy, rescale;
  int32_t what;
  uint8_t* flags; double* tri_xyz; double* tri_ang; double* lift_xyz; double* lift_ang; double* d_prior;
};

// calculate_triangulation_angle of mpsfm/utils/geometry.py:54-65 in degrees: on plain lengths where the names say squared
// lengths, kept as it is (the reference's thresholds act on this value)
__device__ __forceinline__ double ref_angle_deg(const double* C1, const double* C2, const double* X) {
  const double b0 = C1[0] - C2[0], b1 = C1[1] - C2[1], b2 = C1[2] - C2[2];
  const double u0 = X[0] - C1[0], u1 = X[1] - C1[1], u2 = X[2] - C1[2];
  const double w0 = X[0] - C2[0], w1 = X[1] - C2[1], w2 = X[2] - C2[2];
  const double b = sqrt(b0 * b0 + b1 * b1 + b2 * b2);
  const double r1 = sqrt(u0 * u0 + u1 * u1 + u2 * u2);
  const double r2 = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
  const double den = 2.0 * sqrt(r1 * r2);
  if (den == 0.0) return 0.0;
  const double a = fabs(acos((r1 + r2 - b) / den));
  const double f = M_PI - a;
  return (f < a ? f : a) * (180.0 / M_PI);  // Python's min(a, pi - a): NaN stays NaN
}

__global__ __launch_bounds__(kT) void k_init_candidates(InitArgs A) {
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (i >= A.n) return;
  uint32_t flags = 0;
  double T[3] = {0.0, 0.0, 0.0}, L[3] = {0.0, 0.0, 0.0};
  double ta = 0.0, la = 0.0, d = 0.0;
  if (!A.select || A.select[i]) {
    const double x1 = A.xy1[2 * i], y1 = A.xy1[2 * i + 1];
    if (A.what & MPSFM_INIT_TRIANGULATE) {
      TriView v[2] = {A.v1, A.v2};
      v[0].xy[0] = x1; v[0].xy[1] = y1;
      v[1].xy[0] = A.xy2[2 * i]; v[1].xy[1] = A.xy2[2 * i + 1];
#pragma unroll
      for (int k = 0; k < 2; ++k) {  // as tri_make_view
        v[k].xn[0] = (v[k].xy[0] - v[k].K[2]) / v[k].K[0];
        v[k].xn[1] = (v[k].xy[1] - v[k].K[3]) / v[k].K[1];
      }
      // tri_ransac of two views: the one pair is the one trial, no local optimisation (it needs more than two inliers),
      // success when both views are inliers of the sample model
      const int pair[2] = {0, 1};
      double X[3];
      bool ok = tri_estimate(v, pair, 2, A.min_tri_angle, X);
      if (ok)
        ok = tri_residual(v[0], X, TRI_RESIDUAL_ANGULAR) <= A.max_residual && tri_residual(v[1], X, TRI_RESIDUAL_ANGULAR) <= A.max_residual;
      if (ok) {
        flags |= MPSFM_INIT_TRI_OK;
        T[0] = X[0]; T[1] = X[1]; T[2] = X[2];
        ta = ref_angle_deg(A.v1.C, A.v2.C, T);
        if (tri_positive_depth(A.v1.P, T)) flags |= MPSFM_INIT_TRI_POSDEPTH1;
        if (tri_positive_depth(A.v2.P, T)) flags |= MPSFM_INIT_TRI_POSDEPTH2;
      }
    }
    if (A.what & MPSFM_INIT_LIFT) {
      const double gx = grid_coord(x1, A.sx, A.W), gy = grid_coord(y1, A.sy, A.H);
      d = bilinear(A.prior, A.H, A.W, gx, gy);
      if (bilinear(A.valid, A.H, A.W, gx, gy) == 1.0) flags |= MPSFM_INIT_VALID;
      const double ds = d * A.rescale;
      L[0] = (x1 - A.v1.K[2]) / A.v1.K[0] * ds;
      L[1] = (y1 - A.v1.K[3]) / A.v1.K[1] * ds;
      L[2] = ds;
      la = ref_angle_deg(A.v1.C, A.v2.C, L);
      if (tri_positive_depth(A.v1.P, L)) flags |= MPSFM_INIT_LIFT_POSDEPTH1;
      if (tri_positive_depth(A.v2.P, L)) flags |= MPSFM_INIT_LIFT_POSDEPTH2;
    }
  }
  A.flags[i] = (uint8_t)flags;
#pragma unroll
  for (int k = 0; k < 3; ++k) { A.tri_xyz[3 * i + k] = T[k]; A.lift_xyz[3 * i + k] = L[k]; }
  A.tri_ang[i] = ta; A.lift_ang[i] = la; A.d_prior[i] = d;
}

}  // namespace

}  // namespace mpsfm

using namespace mpsfm;

extern "C" int mpsfm_registration_pairs(int32_t n_refs, const mpsfm_reg_image* refs, int64_t n_matches, const int32_t* match_ref,
                                        const double* ref_xy, const int32_t* match_pt, const uint8_t* pt_risky, int32_t n_pts,
                                        const double* pts, int32_t lifted_registration, int32_t device, double* xyz, uint8_t* kind,
                                        float* ms) {
  if (ms) *ms = 0.f;
  if (n_refs < 0 || n_matches < 0 || n_pts < 0) return fail(MPSFM_EINVAL, "negative size");
  if (n_matches > 0 && (!match_ref || !ref_xy || !match_pt || !xyz || !kind)) return fail(MPSFM_EINVAL, "NULL pointer");
  if (n_refs > 0 && !refs) return fail(MPSFM_EINVAL, "refs is NULL");
  if (n_pts > 0 && !pts) return fail(MPSFM_EINVAL, "pts is NULL");
  std::vector<RegRef> R((size_t)n_refs);
  int64_t npix = 0;
  for (int32_t r = 0; r < n_refs; ++r) {
    const mpsfm_reg_image& I = refs[r];
    RegRef& o = R[(size_t)r];
    // without lifted_registration no map is read: it may be absent
    if (lifted_registration && (I.map_h < 2 || I.map_w < 2 || !I.depth_map)) return fail(MPSFM_EINVAL, "map missing or smaller than 2x2");
    if (lifted_registration && (int64_t)I.map_h * I.map_w > (int64_t)1 << 30) return fail(MPSFM_EINVAL, "map larger than 2^30 pixels");
    o.H = I.map_h; o.W = I.map_w; o.off = npix;
    if (lifted_registration) npix += (int64_t)I.map_h * I.map_w;
    o.sx = I.sx; o.sy = I.sy;
    for (int k = 0; k < 4; ++k) o.K[k] = I.intr[k];
    quat_to_R(I.quat_xyzw, o.R);
    for (int k = 0; k < 3; ++k) o.t[k] = I.t[k];
  }
  for (int64_t i = 0; i < n_matches; ++i) {
    if (match_ref[i] < 0 || match_ref[i] >= n_refs) return fail(MPSFM_EINVAL, "match_ref out of range");
    if (match_pt[i] < -1 || match_pt[i] >= n_pts) return fail(MPSFM_EINVAL, "match_pt out of range");
  }
  if (int rc = open_device(device)) return rc;
  CallScope B;
  if (int rc = B.open(true)) return rc;
  if (n_matches == 0) return 0;
  const size_t n = (size_t)n_matches;
  RegArgs A{};
  A.n = n_matches;
  A.lifted = lifted_registration ? 1 : 0;
  if (int rc = B.up(&A.refs, R.data(), R.size())) return rc;
  if (int rc = B.up(&A.match_ref, match_ref, n)) return rc;
  if (int rc = B.up(&A.ref_xy, ref_xy, 2 * n)) return rc;
  if (int rc = B.up(&A.match_pt, match_pt, n)) return rc;
  if (pt_risky && n_pts > 0)
    if (int rc = B.up(&A.risky, pt_risky, (size_t)n_pts)) return rc;
  if (int rc = B.up(&A.pts, pts, 3 * (size_t)n_pts)) return rc;
  double* d_depth = B.alloc<double>((size_t)npix);
  A.xyz = B.alloc<double>(3 * n);
  A.kind = B.alloc<uint8_t>(n);
  if (!d_depth || !A.xyz || !A.kind) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  if (lifted_registration)
    for (int32_t r = 0; r < n_refs; ++r)
      if (int rc = staged_upload(d_depth + R[(size_t)r].off, refs[r].depth_map, sizeof(double) * (size_t)R[(size_t)r].H * R[(size_t)r].W)) return rc;
  A.depth = d_depth;
  if (int rc = staged_drain()) return rc;
  if (int rc = B.begin()) return rc;
  hipLaunchKernelGGL(k_reg_pairs, dim3((unsigned)((n + kT - 1) / kT)), dim3(kT), 0, B.st, A);
  MPSFM_TRY(hipGetLastError());
  if (int rc = B.stop()) return rc;
  MPSFM_TRY(hipMemcpyAsync(xyz, A.xyz, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, B.st));
  MPSFM_TRY(hipMemcpyAsync(kind, A.kind, n, hipMemcpyDeviceToHost, B.st));
  MPSFM_TRY(hipStreamSynchronize(B.st));
  if (ms) return B.elapsed(ms);
  return 0;
}

extern "C" int mpsfm_init_pair_candidates(const mpsfm_init_pair* p, int32_t device, mpsfm_init_candidates* out) {
  if (!p || !out) return fail(MPSFM_EINVAL, "NULL argument");
  out->ms = 0.f;
  if (p->n_matches < 0) return fail(MPSFM_EINVAL, "negative size");
  if (p->what == 0 || (p->what & ~(MPSFM_INIT_TRIANGULATE | MPSFM_INIT_LIFT))) return fail(MPSFM_EINVAL, "what must be MPSFM_INIT_TRIANGULATE, MPSFM_INIT_LIFT or both");
  const bool tri = p->what & MPSFM_INIT_TRIANGULATE, lift = p->what & MPSFM_INIT_LIFT;
  if (p->n_matches > 0 && (!p->xy1 || !out->flags || !out->tri_xyz || !out->tri_angle_deg || !out->lift_xyz || !out->lift_angle_deg || !out->d_prior))
    return fail(MPSFM_EINVAL, "NULL pointer");
  if (p->n_matches > 0 && tri && !p->xy2) return fail(MPSFM_EINVAL, "xy2 is NULL");
  if (lift && (p->map_h < 2 || p->map_w < 2 || !p->prior_map || !p->valid_map)) return fail(MPSFM_EINVAL, "map missing or smaller than 2x2");
  if (lift && (int64_t)p->map_h * p->map_w > (int64_t)1 << 30) return fail(MPSFM_EINVAL, "map larger than 2^30 pixels");
  if (tri && !(p->tri_max_error >= 0.0)) return fail(MPSFM_EINVAL, "tri_max_error must be non-negative");
  if (int rc = open_device(device)) return rc;
  CallScope B;
  if (int rc = B.open(true)) return rc;
  if (p->n_matches == 0) return 0;
  const size_t n = (size_t)p->n_matches, npix = lift ? (size_t)p->map_h * p->map_w : 0;
  InitArgs A{};
  A.n = p->n_matches;
  const double Rid[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tid[3] = {0, 0, 0}, xy0[2] = {0, 0};
  const double* P = p->cam2_from_cam1;
  const double R2[9] = {P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10]}, t2[3] = {P[3], P[7], P[11]};
  tri_make_view(Rid, tid, p->intr1, xy0, A.v1);
  tri_make_view(R2, t2, p->intr2, xy0, A.v2);
  A.min_tri_angle = p->tri_min_angle;
  A.max_residual = p->tri_max_error * p->tri_max_error;
  A.H = p->map_h; A.W = p->map_w; A.sx = p->sx; A.sy = p->sy; A.rescale = p->rescale; A.what = p->what;
  if (int rc = B.up(&A.xy1, p->xy1, 2 * n)) return rc;
  if (tri)
    if (int rc = B.up(&A.xy2, p->xy2, 2 * n)) return rc;
  if (p->select)
    if (int rc = B.up(&A.select, p->select, n)) return rc;
  if (lift) {
    if (int rc = B.up(&A.prior, p->prior_map, npix)) return rc;
    if (int rc = B.up(&A.valid, p->valid_map, npix)) return rc;
  }
  // one block for the float64 outputs: tri_xyz [3n] | lift_xyz [3n] | tri_ang [n] | lift_ang [n] | d_prior [n]
  double* d_out = B.alloc<double>(9 * n);
  A.flags = B.alloc<uint8_t>(n);
  if (!d_out || !A.flags) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  A.tri_xyz = d_out; A.lift_xyz = d_out + 3 * n; A.tri_ang = d_out + 6 * n; A.lift_ang = d_out + 7 * n; A.d_prior = d_out + 8 * n;
  if (int rc = staged_drain()) return rc;
  if (int rc = B.begin()) return rc;
  hipLaunchKernelGGL(k_init_candidates, dim3((unsigned)((n + kT - 1) / kT)), dim3(kT), 0, B.st, A);
  MPSFM_TRY(hipGetLastError());
  if (int rc = B.stop()) return rc;
  MPSFM_TRY(hipMemcpyAsync(out->flags, A.flags, n, hipMemcpyDeviceToHost, B.st));
  MPSFM_TRY(hipMemcpyAsync(out->tri_xyz, A.tri_xyz, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, B.st));
  MPSFM_TRY(hipMemcpyAsync(out->lift_xyz, A.lift_xyz, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, B.st));
  MPSFM_TRY(hipMemcpyAsync(out->tri_angle_deg, A.tri_ang, sizeof(double) * n, hipMemcpyDeviceToHost, B.st));
  MPSFM_TRY(hipMemcpyAsync(out->lift_angle_deg, A.lift_ang, sizeof(double) * n, hipMemcpyDeviceToHost, B.st));
  MPSFM_TRY(hipMemcpyAsync(out->d_prior, A.d_prior, sizeof(double) * n, hipMemcpyDeviceToHost, B.st));
  MPSFM_TRY(hipStreamSynchronize(B.st));
  return B.elapsed(&out->ms);
}
