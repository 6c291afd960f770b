// Dense point-to-plane ICP of an RGB-D pair (mpsfm_depth_normals, mpsfm_depth_pair_icp, mpsfm_depth_pair_register_dense;
// semantics: include/mpsfm_hip.h, arithmetic: icp_math.h):
//   k_icp_normals  one thread per pixel: the camera-facing normal by central differences of the vertex map
//   k_icp_init     the call's state block: the initial pose, done = 0, a zeroed trace
//   k_icp_link     one thread per interior pixel of map 0 on the stride grid: association with map 1 at the state's pose and
//                  the pixel's 33 terms, reduced to one row per workgroup (block_reduce_rows)
//   k_icp_step     one workgroup: the rows added in block order, the 6 x 6 solve, the pose update, the trace row, the done word
// A call enqueues k_icp_link, k_icp_step max_iterations times on its stream and waits once; a kernel that finds done set
// returns at entry.  The grid of k_icp_link is a function of H0, W0 and stride alone, so the summation order never changes.
// f64 throughout.
#include <cmath>
#include <cstring>

#include "align3d_device.h"
#include "icp_math.h"
#include "lo_ransac.h"

namespace mpsfm {

namespace {
constexpr int kT = kLoT;
constexpr int kIcpMaxBlocks = 256;

struct IcpState {
  double pose[12];
  double sums[kIcpK];  // of the last linearisation formed
  double rmse;
  int32_t iterations, status, done, pad;
};

// the source grid: interior pixels (r, c) = ((i / nc + 1) stride, (i % nc + 1) stride), i < nr nc
struct IcpSource {
  const double* depth;
  const double* normals;
  const uint8_t* valid;
  int32_t W, nr, nc, stride;
  double intr[4];
};
struct IcpRules { double eps_rotation, eps_translation; int32_t max_iterations, min_pairs; };

inline int icp_blocks(int64_t ns) { return (int)std::max<int64_t>(1, std::min<int64_t>((ns + kT - 1) / kT, kIcpMaxBlocks)); }

__global__ __launch_bounds__(kT) void k_icp_normals(A3Map m, double edge_ratio, double* __restrict__ normals, uint8_t* __restrict__ valid) {
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (i >= (int64_t)m.H * m.W) return;
  const int32_t r = (int32_t)(i / m.W), c = (int32_t)(i % m.W);
  double n[3] = {0.0, 0.0, 0.0};
  const bool ok = r >= 1 && r <= m.H - 2 && c >= 1 && c <= m.W - 2 && icp_normal(m.depth, m.W, m.intr, edge_ratio, r, c, n);
  normals[3 * (size_t)i] = n[0]; normals[3 * (size_t)i + 1] = n[1]; normals[3 * (size_t)i + 2] = n[2];
  valid[i] = ok ? 1 : 0;
}

struct IcpPose { double T[12]; };
__global__ __launch_bounds__(kT) void k_icp_init(IcpPose init, int32_t ntrace, IcpState* __restrict__ state, double* __restrict__ trace) {
  for (int32_t k = threadIdx.x; k < ntrace; k += kT) trace[k] = 0.0;
  if (threadIdx.x < 12) state->pose[threadIdx.x] = init.T[threadIdx.x];
  if (threadIdx.x < kIcpK) state->sums[threadIdx.x] = 0.0;
  if (threadIdx.x == 0) {
    state->rmse = 0.0;
    state->iterations = 0;
    state->status = MPSFM_ICP_MAX_ITERATIONS_REACHED;
    state->done = 0;
    state->pad = 0;
  }
}

__global__ __launch_bounds__(kT) void k_icp_link(IcpSource s, IcpTarget t, IcpGates g, const IcpState* __restrict__ state, double* __restrict__ part) {
  if (state->done) return;  // uniform over the grid: k_icp_step alone writes it, between two launches of this kernel
  double T[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) T[k] = state->pose[k];
  double acc[kIcpK];
#pragma unroll
  for (int k = 0; k < kIcpK; ++k) acc[k] = 0.0;
  const int32_t ns = s.nr * s.nc;
  for (int32_t i = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x; i < ns; i += (int32_t)gridDim.x * kT) {
    const int32_t r = (i / s.nc + 1) * s.stride, c = (i % s.nc + 1) * s.stride;
    const size_t at = (size_t)r * s.W + c;
    if (!s.valid[at]) continue;
    double p[3];
    a3_pixel_point((double)c, (double)r, s.depth[at], s.intr, p);
    const double n0[3] = {s.normals[3 * at], s.normals[3 * at + 1], s.normals[3 * at + 2]};
    icp_link(T, g, t, p, n0, acc);
  }
  block_reduce_rows<kIcpK>(acc, part);
}

__global__ __launch_bounds__(64) void k_icp_step(int32_t it, int32_t nblocks, IcpRules o, const double* __restrict__ part, IcpState* __restrict__ state,
                                                 double* __restrict__ trace) {
  if (state->done) return;
  __shared__ double sums[kIcpK];
  if (threadIdx.x < kIcpK) {
    double s = 0.0;
    for (int32_t b = 0; b < nblocks; ++b) s += part[(size_t)b * kIcpK + threadIdx.x];
    sums[threadIdx.x] = s;
    state->sums[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double count = sums[kIcpCount];
  const double rmse = count > 0.0 ? sqrt(sums[kIcpRR] / count) : 0.0;
  double norms[2] = {0.0, 0.0};
  int32_t status = -1;
  if (count < (double)o.min_pairs) {
    status = MPSFM_ICP_TOO_FEW_PAIRS;
  } else {
    double A[36], b[6], xi[6];
    icp_system(sums, A, b);
    if (!icp_solve(A, b, xi)) {
      status = MPSFM_ICP_SINGULAR;
    } else {
      double T[12];
      for (int k = 0; k < 12; ++k) T[k] = state->pose[k];
      icp_apply(xi, T, norms);
      for (int k = 0; k < 12; ++k) state->pose[k] = T[k];
      if (norms[0] <= o.eps_rotation && norms[1] <= o.eps_translation) status = MPSFM_ICP_CONVERGED;
      else if (it + 1 == o.max_iterations) status = MPSFM_ICP_MAX_ITERATIONS_REACHED;
    }
  }
  state->rmse = rmse;
  state->iterations = it + 1;
  if (trace) {
    trace[4 * it] = count; trace[4 * it + 1] = rmse; trace[4 * it + 2] = norms[0]; trace[4 * it + 3] = norms[1];
  }
  if (status >= 0) {
    state->status = status;
    state->done = 1;
  }
}

bool icp_map_valid(int32_t H, int32_t W, const double* depth, const double* intr, int32_t least) {
  return depth && intr && H >= least && W >= least && (int64_t)H * W <= INT32_MAX && finite_all(intr, 4) && intr[0] != 0.0 && intr[1] != 0.0;
}

bool icp_options_valid(const mpsfm_icp_options& o) {
  return std::isfinite(o.max_distance) && o.max_distance > 0.0 && std::isfinite(o.max_angle_deg) && o.max_angle_deg >= 0.0 &&
         o.max_angle_deg <= 180.0 && std::isfinite(o.edge_ratio) && o.edge_ratio >= 0.0 && std::isfinite(o.eps_rotation) && o.eps_rotation >= 0.0 &&
         std::isfinite(o.eps_translation) && o.eps_translation >= 0.0 && o.max_iterations >= 1 && o.max_iterations <= MPSFM_ICP_MAX_ITERATIONS &&
         o.min_pairs >= 6 && o.stride >= 1;
}

// zeroes *result, then the MPSFM_EINVAL cases of mpsfm_depth_pair_icp
int icp_check(int32_t H0, int32_t W0, const double* depth0, const double* intr0, int32_t H1, int32_t W1, const double* depth1, const double* intr1,
              const double* init, double scale, const mpsfm_icp_options* o, mpsfm_icp_result* result) {
  if (result) *result = mpsfm_icp_result{};
  if (!o || !result || !init) return fail(MPSFM_EINVAL, "NULL pointer");
  if (!icp_map_valid(H0, W0, depth0, intr0, 3) || !icp_map_valid(H1, W1, depth1, intr1, 3))
    return fail(MPSFM_EINVAL, "depth map or intrinsics invalid (NULL, smaller than 3 x 3, or a zero / non-finite focal length)");
  if (!finite_all(init, 12) || !(std::isfinite(scale) && scale > 0.0)) return fail(MPSFM_EINVAL, "initial pose or scale not finite, or scale <= 0");
  if (!icp_options_valid(*o)) return fail(MPSFM_EINVAL, "invalid ICP options");
  return 0;
}

int icp_normals_launch(CallScope& A, const A3Map& m, double edge_ratio, double* normals, uint8_t* valid) {
  hipLaunchKernelGGL(k_icp_normals, dim3((unsigned)(((int64_t)m.H * m.W + kT - 1) / kT)), dim3(kT), 0, A.st, m, edge_ratio, normals, valid);
  MPSFM_TRY(hipGetLastError());
  return 0;
}

// the loop over maps that are on the device (scope open and timed, arguments checked); result->ms is the caller's
int icp_device(CallScope& A, const A3Map& m0, const A3Map& m1, const double* init, double scale, const mpsfm_icp_options& o, double* trace,
               mpsfm_icp_result* result) {
  const size_t n0 = (size_t)m0.H * m0.W, n1 = (size_t)m1.H * m1.W;
  const int32_t nr = (m0.H - 2) / o.stride, nc = (m0.W - 2) / o.stride;
  const int nblocks = icp_blocks((int64_t)nr * nc);
  const int32_t ntrace = 4 * o.max_iterations;
  double* d_nrm0 = A.alloc<double>(3 * n0);
  double* d_nrm1 = A.alloc<double>(3 * n1);
  uint8_t* d_val0 = A.alloc<uint8_t>(n0);
  uint8_t* d_val1 = A.alloc<uint8_t>(n1);
  double* d_part = A.alloc<double>((size_t)kIcpK * nblocks);
  double* d_trace = A.alloc<double>((size_t)ntrace);
  IcpState* d_state = A.alloc<IcpState>(1);
  IcpState* h_state = A.host<IcpState>(1);
  if (!d_nrm0 || !d_nrm1 || !d_val0 || !d_val1 || !d_part || !d_trace || !d_state || !h_state) return fail(MPSFM_ENOMEM, "hipMalloc failed");

  IcpSource src{m0.depth, d_nrm0, d_val0, m0.W, nr, nc, o.stride, {m0.intr[0], m0.intr[1], m0.intr[2], m0.intr[3]}};
  IcpTarget tgt{m1.depth, d_nrm1, d_val1, m1.H, m1.W, {m1.intr[0], m1.intr[1], m1.intr[2], m1.intr[3]}};
  const IcpGates gates{scale, o.max_distance * o.max_distance, std::cos(o.max_angle_deg * (M_PI / 180.0))};
  const IcpRules rules{o.eps_rotation, o.eps_translation, o.max_iterations, o.min_pairs};
  IcpPose pose;
  std::memcpy(pose.T, init, sizeof(pose.T));

  if (int rc = A.begin()) return rc;
  hipLaunchKernelGGL(k_icp_init, dim3(1), dim3(kT), 0, A.st, pose, ntrace, d_state, d_trace);
  MPSFM_TRY(hipGetLastError());
  if (int rc = icp_normals_launch(A, m0, o.edge_ratio, d_nrm0, d_val0)) return rc;
  if (int rc = icp_normals_launch(A, m1, o.edge_ratio, d_nrm1, d_val1)) return rc;
  for (int32_t it = 0; it < o.max_iterations; ++it) {
    hipLaunchKernelGGL(k_icp_link, dim3((unsigned)nblocks), dim3(kT), 0, A.st, src, tgt, gates, (const IcpState*)d_state, d_part);
    MPSFM_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_icp_step, dim3(1), dim3(64), 0, A.st, it, (int32_t)nblocks, rules, (const double*)d_part, d_state, d_trace);
    MPSFM_TRY(hipGetLastError());
  }
  if (int rc = A.stop()) return rc;
  MPSFM_TRY(hipMemcpyAsync(h_state, d_state, sizeof(IcpState), hipMemcpyDeviceToHost, A.st));
  if (trace) MPSFM_TRY(hipMemcpyAsync(trace, d_trace, sizeof(double) * (size_t)ntrace, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipStreamSynchronize(A.st));  // the one wait of the loop
  float t = 0.f;
  if (int rc = A.elapsed(&t)) return rc;
  A.ms += t;

  std::memcpy(result->tgt_from_src, h_state->pose, sizeof(result->tgt_from_src));
  result->scale = scale;
  icp_system(h_state->sums, result->info, result->rhs);
  result->rmse = h_state->rmse;
  result->num_pairs = (int64_t)h_state->sums[kIcpCount];
  for (int k = 0; k < 4; ++k) result->rejected[k] = (int64_t)h_state->sums[kIcpRej + k];
  result->iterations = h_state->iterations;
  result->status = h_state->status;
  return 0;
}
}  // namespace

}  // namespace mpsfm

using namespace mpsfm;

extern "C" int mpsfm_depth_normals(int32_t H, int32_t W, const double* depth, const double* intr, double edge_ratio, int32_t device,
                                   double* normals, uint8_t* valid) {
  if (!normals || !valid) return fail(MPSFM_EINVAL, "NULL pointer");
  if (!icp_map_valid(H, W, depth, intr, 1)) return fail(MPSFM_EINVAL, "depth map or intrinsics invalid (NULL, empty, or a zero / non-finite focal length)");
  if (!(std::isfinite(edge_ratio) && edge_ratio >= 0.0)) return fail(MPSFM_EINVAL, "edge_ratio must be finite and >= 0");
  if (int rc = open_device(device)) return rc;
  CallScope A;
  if (int rc = A.open()) return rc;
  const size_t n = (size_t)H * W;
  A3Map m{A.put(depth, n), H, W, {intr[0], intr[1], intr[2], intr[3]}};
  double* d_nrm = A.alloc<double>(3 * n);
  uint8_t* d_val = A.alloc<uint8_t>(n);
  if (!m.depth || !d_nrm || !d_val) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  if (int rc = icp_normals_launch(A, m, edge_ratio, d_nrm, d_val)) return rc;
  MPSFM_TRY(hipMemcpyAsync(normals, d_nrm, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(A.down(valid, d_val, n));
  return 0;
}

extern "C" int mpsfm_depth_pair_icp(int32_t H0, int32_t W0, const double* depth0, const double* intr0, int32_t H1, int32_t W1,
                                    const double* depth1, const double* intr1, const double* init, double scale, const mpsfm_icp_options* o,
                                    int32_t device, double* trace, mpsfm_icp_result* result) {
  if (int rc = icp_check(H0, W0, depth0, intr0, H1, W1, depth1, intr1, init, scale, o, result)) return rc;
  if (int rc = open_device(device)) return rc;
  CallScope A;
  if (int rc = A.open(true)) return rc;
  A3Map m0{A.put(depth0, (size_t)H0 * W0), H0, W0, {intr0[0], intr0[1], intr0[2], intr0[3]}};
  A3Map m1{A.put(depth1, (size_t)H1 * W1), H1, W1, {intr1[0], intr1[1], intr1[2], intr1[3]}};
  if (!m0.depth || !m1.depth) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  if (int rc = icp_device(A, m0, m1, init, scale, *o, trace, result)) return rc;
  result->ms = (float)A.ms;
  return 0;
}

extern "C" int mpsfm_depth_pair_register_dense(int32_t H0, int32_t W0, const double* depth0, const double* intr0, int32_t H1, int32_t W1,
                                               const double* depth1, const double* intr1, int64_t n0, const double* xy0, int64_t n1,
                                               const double* xy1, int64_t m, const int32_t* matches, int32_t with_scale,
                                               const mpsfm_align3d_options* o, const mpsfm_icp_options* io, int32_t device, uint8_t* valid,
                                               uint8_t* inlier_mask, double* lifted0, double* lifted1, mpsfm_align3d_result* result,
                                               double* trace, mpsfm_icp_result* icp) {
  if (icp) *icp = mpsfm_icp_result{};
  if (int rc = a3_register_check(H0, W0, depth0, intr0, H1, W1, depth1, intr1, n0, xy0, n1, xy1, m, matches, with_scale, o, valid, inlier_mask,
                                 lifted0, lifted1, result))
    return rc;
  const double identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};  // the pose is the RANSAC's: only the other arguments are checked here
  if (int rc = icp_check(H0, W0, depth0, intr0, H1, W1, depth1, intr1, identity, 1.0, io, icp)) return rc;
  if (trace) std::memset(trace, 0, sizeof(double) * 4 * (size_t)io->max_iterations);
  if (m == 0) return 0;
  if (int rc = open_device(device)) return rc;
  CallScope A;
  if (int rc = A.open(true)) return rc;
  A3Map m0{}, m1{};
  if (int rc = a3_register_device(A, H0, W0, depth0, intr0, H1, W1, depth1, intr1, n0, xy0, n1, xy1, m, matches, with_scale, o, valid, inlier_mask,
                                  lifted0, lifted1, result, &m0, &m1))
    return rc;
  result->ms = (float)A.ms;
  if (!result->success) return 0;
  A.ms = 0.0;
  if (int rc = icp_device(A, m0, m1, result->tgt_from_src, result->scale, *io, trace, icp)) return rc;
  icp->ms = (float)A.ms;
  return 0;
}
