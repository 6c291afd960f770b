// Depth lifting of low-parallax points for a batch of tracks (reference mpsfm/sfm/mapper/triangulator.py:49-83, 125-161:
// the Python loop MpsfmTriangulator runs after every triangulate_image and at the end of every retriangulate):
//   mpsfm_lift_tracks   phase 1: the max triangulation angle per track by k_filter itself (tri_kernels.hip), so that
//                       risky = angle < min_angle is the decision mpsfm_filter_tracks would give, bit for bit;
//                       phase 2, risky tracks only: the first element in track order whose camera is activated and whose
//                       validity sample is exactly 1 lifts the point from its depth map; every element of the track then
//                       keeps or loses its place by the sign of the new point's depth in its camera.
//   k_lift_tracks       one wavefront per risky track.  Lanes take the elements 64 at a time; a ballot and a find-first-set
//                       pick the first valid element of the first chunk that has one (later chunks are not sampled), the
//                       winning lane's keypoint, camera and depth go to all lanes by shuffle, and all lanes write the keep
//                       flags of their elements.  The rotations come per camera from the host, as in registration.hip.
// f64 throughout; a gather and a few dozen flops per element: the call is bound by its transfers and the angle launch.
#include <cmath>
#include <string>
#include <vector>

#include "common.h"
#include "bilinear_sample.h"  // grid_coord + bilinear, and contraction off for the rest of this file
#include "call_scope.h"
#include "tri_launch.h"

namespace mpsfm {

namespace {
constexpr int kWaves = 4;  // risky tracks per workgroup of 256 threads

struct LiftCam {  // one camera of the tracks
  double R[9];    // cam_from_world rotation, row-major
  double t[3];
  double K[4];
  double sx, sy;
  int64_t off;    // into the concatenated maps; read where activated
  int32_t H, W;
  int32_t activated, pad;
};

struct LiftArgs {
  int64_t n_risky;
  const int32_t* risky_track;  // [n_risky] track index, ascending
  const int64_t* start; const int32_t* el_cam; const double* el_xy;  // the tracks, all of them
  const LiftCam* cams;
  const double* depth; const uint8_t* valid;  // concatenated maps of the uploaded cameras
  int32_t* lift_el; double* lift_depth; double* lift_xyz;  // [n_risky], compact
  uint8_t* el_keep;                                         // [n_el], zero on entry
};

__global__ __launch_bounds__(64 * kWaves) void k_lift_tracks(LiftArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (r >= A.n_risky) return;  // whole waves leave: no workgroup barrier below
  const int32_t tr = A.risky_track[r];
  const int64_t e0 = A.start[tr], e1 = A.start[tr + 1];
  int64_t win = -1;
  double wx = 0.0, wy = 0.0, wd = 0.0;
  int wcam = 0;
  for (int64_t base = e0; base < e1; base += 64) {  // wave-uniform trip count
    const int64_t e = base + lane;
    bool ok = false;
    double x = 0.0, y = 0.0, gx = 0.0, gy = 0.0;
    int cam = 0;
    if (e < e1) {
      cam = A.el_cam[e];
      const LiftCam& c = A.cams[cam];
      if (c.activated) {
        x = A.el_xy[2 * e]; y = A.el_xy[2 * e + 1];
        gx = grid_coord(x, c.sx, c.W); gy = grid_coord(y, c.sy, c.H);
        ok = bilinear(A.valid + c.off, c.H, c.W, gx, gy) == 1.0;
      }
    }
    const unsigned long long m = __ballot(ok);
    if (m != 0ull) {
      const int src = __ffsll(m) - 1;  // the first valid element in track order
      double d = 0.0;
      if (lane == src) {
        const LiftCam& c = A.cams[cam];
        d = bilinear(A.depth + c.off, c.H, c.W, gx, gy);
      }
      wd = __shfl(d, src); wx = __shfl(x, src); wy = __shfl(y, src); wcam = __shfl(cam, src);
      win = base + src;
      break;
    }
  }
  if (win < 0) {  // nothing lifts: el_keep stays zero
    if (lane == 0) {
      A.lift_el[r] = -1; A.lift_depth[r] = 0.0;
      A.lift_xyz[3 * r] = 0.0; A.lift_xyz[3 * r + 1] = 0.0; A.lift_xyz[3 * r + 2] = 0.0;
    }
    return;
  }
  // cam_from_world.inverse() * (ray d): R^T (ray d - t), as k_reg_pairs
  const LiftCam& c = A.cams[wcam];
  const double q0 = (wx - c.K[2]) / c.K[0] * wd - c.t[0];
  const double q1 = (wy - c.K[3]) / c.K[1] * wd - c.t[1];
  const double q2 = wd - c.t[2];
  const double X0 = c.R[0] * q0 + c.R[3] * q1 + c.R[6] * q2;
  const double X1 = c.R[1] * q0 + c.R[4] * q1 + c.R[7] * q2;
  const double X2 = c.R[2] * q0 + c.R[5] * q1 + c.R[8] * q2;
  if (lane == 0) {
    A.lift_el[r] = (int32_t)(win - e0); A.lift_depth[r] = wd;
    A.lift_xyz[3 * r] = X0; A.lift_xyz[3 * r + 1] = X1; A.lift_xyz[3 * r + 2] = X2;
  }
  for (int64_t e = e0 + lane; e < e1; e += 64) {
    const LiftCam& k = A.cams[A.el_cam[e]];
    const double zc = k.R[6] * X0 + k.R[7] * X1 + k.R[8] * X2 + k.t[2];
    A.el_keep[e] = zc >= 2.220446049250313e-16 ? 1 : 0;
  }
}

}  // namespace

}  // namespace mpsfm

using namespace mpsfm;

extern "C" int mpsfm_lift_tracks(const mpsfm_tracks* T, const double* xyz, const mpsfm_lift_maps* M, double min_angle_rad, int32_t device,
                                 uint8_t* risky, int32_t* lift_el, double* lift_depth, double* lift_xyz, uint8_t* el_keep,
                                 mpsfm_lift_info* info) {
  if (info) *info = mpsfm_lift_info{};
  if (int rc = check_tracks(T)) return rc;
  if (std::isnan(min_angle_rad) || min_angle_rad < 0.0) return fail(MPSFM_EINVAL, "min_angle_rad is NaN or negative");
  if (T->n_tracks == 0) return 0;
  const int64_t ne = T->track_start[T->n_tracks];
  if (!xyz) return fail(MPSFM_EINVAL, "xyz is NULL");
  if (!risky || !lift_el || !lift_depth || !lift_xyz || (ne > 0 && !el_keep)) return fail(MPSFM_EINVAL, "output pointer is NULL");
  if (!M) return fail(MPSFM_EINVAL, "maps is NULL");
  if (T->n_cams > 0 && (!M->activated || !M->map_h || !M->map_w || !M->depth_map || !M->valid_map || !M->sx || !M->sy))
    return fail(MPSFM_EINVAL, "map arrays are NULL");
  for (int32_t t = 0; t < T->n_tracks; ++t)
    if (T->track_start[t + 1] - T->track_start[t] > (int64_t)INT32_MAX) return fail(MPSFM_EINVAL, "track longer than 2^31 - 1 elements");
  if (int rc = open_device(device)) return rc;
  const size_t nt = (size_t)T->n_tracks, nc = (size_t)T->n_cams;

  // ---- phase 1: the angles of k_filter, the risky flags on the host ------------------------------------------------------
  CallScope B;
  if (int rc = B.open(true)) return rc;
  TrackArgs a{};
  if (int rc = upload_tracks(T, B, a)) return rc;
  const double* dxyz = B.put(xyz, nt * 3);
  double* dang = B.alloc<double>(nt);
  if (!dxyz || !dang) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  if (int rc = B.begin()) return rc;
  launch_filter_tracks(a, dxyz, dang, nullptr, nullptr, B.st);
  MPSFM_TRY(hipGetLastError());
  if (int rc = B.stop()) return rc;
  std::vector<double> ang(nt);
  MPSFM_TRY(B.down(ang.data(), dang, sizeof(double) * nt));
  float ms1 = 0.f, ms2 = 0.f;
  if (int rc = B.elapsed(&ms1)) return rc;

  std::vector<int32_t> rtrack;
  for (size_t t = 0; t < nt; ++t) {
    risky[t] = ang[t] < min_angle_rad ? 1 : 0;
    if (risky[t]) rtrack.push_back((int32_t)t);
    lift_el[t] = -1; lift_depth[t] = 0.0;
    lift_xyz[3 * t] = lift_xyz[3 * t + 1] = lift_xyz[3 * t + 2] = 0.0;
  }
  const size_t nr = rtrack.size();
  if (info) { info->n_risky = (int64_t)nr; info->ms = ms1; }
  if (nr == 0) {
    std::fill(el_keep, el_keep + ne, (uint8_t)0);
    return 0;
  }

  // ---- phase 2: the maps of the activated cameras of the risky tracks, the lift launch -----------------------------------
  std::vector<uint8_t> used(nc, 0);
  for (int32_t t : rtrack)
    for (int64_t e = T->track_start[t]; e < T->track_start[t + 1]; ++e) used[(size_t)T->el_cam[e]] = 1;
  std::vector<LiftCam> cams(nc);
  int64_t npix = 0;
  int32_t n_up = 0;
  for (size_t c = 0; c < nc; ++c) {
    LiftCam& L = cams[c];
    L = LiftCam{};
    quat_to_R(T->cam_quat_xyzw + 4 * c, L.R);
    const double* K = T->cam_intr + 4 * (size_t)T->cam_intr_idx[c];
    for (int k = 0; k < 3; ++k) L.t[k] = T->cam_t[3 * c + k];
    for (int k = 0; k < 4; ++k) L.K[k] = K[k];
    L.sx = M->sx[c]; L.sy = M->sy[c];
    if (!used[c] || !M->activated[c]) continue;  // never sampled: no map goes up
    if (!M->depth_map[c] || !M->valid_map[c] || M->map_h[c] < 2 || M->map_w[c] < 2) return fail(MPSFM_EINVAL, "map missing or smaller than 2x2");
    if ((int64_t)M->map_h[c] * M->map_w[c] > (int64_t)1 << 30) return fail(MPSFM_EINVAL, "map larger than 2^30 pixels");
    L.activated = 1; L.H = M->map_h[c]; L.W = M->map_w[c]; L.off = npix;
    npix += (int64_t)L.H * L.W;
    ++n_up;
  }
  LiftArgs A{};
  A.n_risky = (int64_t)nr;
  A.start = a.start; A.el_cam = a.el_cam; A.el_xy = a.el_xy;
  if (int rc = B.up(&A.risky_track, rtrack.data(), nr)) return rc;
  if (int rc = B.up(&A.cams, cams.data(), nc)) return rc;
  double* d_depth = B.alloc<double>((size_t)npix);
  uint8_t* d_valid = B.alloc<uint8_t>((size_t)npix);
  A.lift_el = B.alloc<int32_t>(nr);
  double* d_out = B.alloc<double>(4 * nr);  // lift_depth [nr] | lift_xyz [3 nr]
  A.el_keep = B.alloc<uint8_t>((size_t)ne);
  if (!d_depth || !d_valid || !A.lift_el || !d_out || !A.el_keep) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  for (size_t c = 0; c < nc; ++c) {
    if (!cams[c].activated) continue;
    const size_t n = (size_t)cams[c].H * cams[c].W;
    if (int rc = staged_upload(d_depth + cams[c].off, M->depth_map[c], sizeof(double) * n)) return rc;
    if (int rc = staged_upload(d_valid + cams[c].off, M->valid_map[c], n)) return rc;
  }
  A.depth = d_depth; A.valid = d_valid;
  A.lift_depth = d_out; A.lift_xyz = d_out + nr;
  if (int rc = staged_drain()) return rc;
  if (ne > 0) MPSFM_TRY(hipMemsetAsync(A.el_keep, 0, (size_t)ne, B.st));
  if (int rc = B.begin()) return rc;
  hipLaunchKernelGGL(k_lift_tracks, dim3((unsigned)((nr + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, B.st, A);
  MPSFM_TRY(hipGetLastError());
  if (int rc = B.stop()) return rc;
  std::vector<int32_t> h_el(nr);
  std::vector<double> h_out(4 * nr);
  MPSFM_TRY(hipMemcpyAsync(h_el.data(), A.lift_el, sizeof(int32_t) * nr, hipMemcpyDeviceToHost, B.st));
  MPSFM_TRY(hipMemcpyAsync(h_out.data(), d_out, sizeof(double) * 4 * nr, hipMemcpyDeviceToHost, B.st));
  if (ne > 0) MPSFM_TRY(hipMemcpyAsync(el_keep, A.el_keep, (size_t)ne, hipMemcpyDeviceToHost, B.st));
  MPSFM_TRY(hipStreamSynchronize(B.st));
  if (int rc = B.elapsed(&ms2)) return rc;
  int64_t n_lifted = 0;
  for (size_t r = 0; r < nr; ++r) {
    const size_t t = (size_t)rtrack[r];
    lift_el[t] = h_el[r];
    if (h_el[r] < 0) continue;
    ++n_lifted;
    lift_depth[t] = h_out[r];
    for (int k = 0; k < 3; ++k) lift_xyz[3 * t + k] = h_out[nr + 3 * r + k];
  }
  if (info) {
    info->n_lifted = n_lifted; info->n_no_lift = (int64_t)nr - n_lifted;
    info->n_maps_uploaded = n_up;
    info->bytes_uploaded = npix * (int64_t)(sizeof(double) + 1);
    info->ms = (double)ms1 + (double)ms2;
  }
  return 0;
}
