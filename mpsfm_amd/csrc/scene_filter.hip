// The filter behind a bundle adjustment as one call over the scene's arrays (semantics: include/mpsfm_hip.h; the design and the
// measurements: DESIGN.md section 4v): negative depth, the risky set, and the two reprojection / angle passes of the reference's
// filter_bundle / filter_all (mpsfm/sfm/mapper/base.py:686-797).  Every decision about a point depends on that point's own track.
//
//   k_sf_images      one record per image: rotation, translation, centre, intrinsics (once per image, not per element)
//   k_sf_keys        per keypoint: its image (a search in kp_start) and the sort key, its point or n_points where it has none
//   rocprim          stable radix sort of (key, keypoint): a track's elements come out in ascending keypoint index, grouped by
//                    image; the keypoints without a point sort behind every track
//   k_sf_starts      per point: the first element of its track, a lower bound in the sorted keys
//   k_scene_filter   one wavefront per point, lanes take the elements e0 + lane + 64 c.  Fronts, bad flags and flagged bundle
//                    elements are 64-bit ballots counted with __popcll; the pair angles come from a wave-uniform loop over the
//                    good partners j, whose centre and ray length are broadcast by __shfl, each lane keeping its own maximum;
//                    tracks longer than 64 loop over chunk pairs.  No workgroup barrier: a wave without work leaves.
// The counts are integer atomics, the rest plain stores: nothing depends on the order of arrival.
#include <cmath>
#include <string>

#include <rocprim/device/device_radix_sort.hpp>

#include "call_scope.h"
#include "common.h"
#include "scene_filter_check.h"

// the decisions round every operation on its own, so that tests/numpy_scene_filter.py can follow them operation for operation
#pragma clang fp contract(off)

namespace mpsfm {

namespace {
constexpr int kSfT = 256;         // threads of the element-wise kernels
constexpr int kSfWaves = 4;       // points per workgroup of k_scene_filter
constexpr double kSfEps = 2.220446049250313e-16;  // 2^-52: COLMAP's cheirality bound, as in k_filter

struct SfImage {
  double R[9], t[3], C[3], K[4];
};

struct SfArgs {
  int64_t n_kp, n_points;
  int32_t n_images, n_bundle, negative_depth, pad;
  double max_sq, thr_a, thr_b;
  const int64_t* kp_start;   // [n_images + 1]
  const double* kp_xy;       // [n_kp][2]
  const double* intr;        // [n_images][4]
  const double *quat, *trans;
  const int64_t* kp_point;   // [n_kp]
  const double* xyz;         // [n_points][3]
  const uint8_t *in_bundle, *kp_flag, *point_sel;  // [n_images], [n_kp] (both read where n_bundle > 0), [n_points] or nullptr
  SfImage* images;           // [n_images]
  int32_t* kp_image;         // [n_kp]
  uint32_t *key_in, *key, *val_in, *val;  // [n_kp]
  int32_t* start;            // [n_points + 1]
  uint8_t *kp_deleted, *fate, *risky;     // zero on entry
  double *max_angle, *kp_sq_err;          // zero on entry; may be nullptr
  unsigned long long* counts;             // [5] num_negative, changed_a, changed_b, points deleted, observations deleted
};

inline dim3 sf_blocks(int64_t n) { return dim3((unsigned)((n + kSfT - 1) / kSfT)); }

__global__ __launch_bounds__(kSfT) void k_sf_images(SfArgs a) {
  const int32_t i = (int32_t)(blockIdx.x * kSfT + threadIdx.x);
  if (i >= a.n_images) return;
  SfImage c;
  // quat_to_R of common.h, restated here so that it is compiled without contraction
  const double x = a.quat[4 * i], y = a.quat[4 * i + 1], z = a.quat[4 * i + 2], w = a.quat[4 * i + 3];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  c.R[0] = 1 - (tyy + tzz); c.R[1] = txy - twz;       c.R[2] = txz + twy;
  c.R[3] = txy + twz;       c.R[4] = 1 - (txx + tzz); c.R[5] = tyz - twx;
  c.R[6] = txz - twy;       c.R[7] = tyz + twx;       c.R[8] = 1 - (txx + tyy);
  for (int k = 0; k < 3; ++k) c.t[k] = a.trans[3 * i + k];
  for (int k = 0; k < 3; ++k) c.C[k] = -(c.R[k] * c.t[0] + c.R[3 + k] * c.t[1] + c.R[6 + k] * c.t[2]);
  for (int k = 0; k < 4; ++k) c.K[k] = a.intr[4 * i + k];
  a.images[i] = c;
}

__global__ __launch_bounds__(kSfT) void k_sf_keys(SfArgs a) {
  const int64_t k = (int64_t)blockIdx.x * kSfT + threadIdx.x;
  if (k >= a.n_kp) return;
  // the image i with kp_start[i] <= k < kp_start[i + 1] (images without keypoints are stepped over)
  int32_t lo = 0, hi = a.n_images;  // kp_start[lo] <= k < kp_start[hi]
  while (hi - lo > 1) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (a.kp_start[mid] <= k) lo = mid; else hi = mid;
  }
  a.kp_image[k] = lo;
  const int64_t p = a.kp_point[k];
  a.key_in[k] = (uint32_t)(p >= 0 ? p : a.n_points);
  a.val_in[k] = (uint32_t)k;
}

__global__ __launch_bounds__(kSfT) void k_sf_starts(SfArgs a) {
  const int64_t p = (int64_t)blockIdx.x * kSfT + threadIdx.x;
  if (p > a.n_points) return;
  int64_t lo = 0, hi = a.n_kp;  // the first position whose key is >= p
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if ((int64_t)a.key[mid] < p) lo = mid + 1; else hi = mid;
  }
  a.start[p] = (int32_t)lo;
}

// one element of a track as its lane holds it
struct SfElem {
  double C[3], r;   // projection centre of its image, |X - C|^2
  double sq_err;
  int32_t im;
  bool front, over;  // over: sq_err > max_err^2
};

__device__ inline void sf_elem(const SfArgs& a, const double* X, int64_t k, SfElem& o) {
  const int32_t im = a.kp_image[k];
  const SfImage& c = a.images[im];
  const double xc = c.R[0] * X[0] + c.R[1] * X[1] + c.R[2] * X[2] + c.t[0];
  const double yc = c.R[3] * X[0] + c.R[4] * X[1] + c.R[5] * X[2] + c.t[1];
  const double zc = c.R[6] * X[0] + c.R[7] * X[1] + c.R[8] * X[2] + c.t[2];
  const double du = c.K[0] * xc / zc + c.K[2] - a.kp_xy[2 * k];
  const double dv = c.K[1] * yc / zc + c.K[3] - a.kp_xy[2 * k + 1];
  o.im = im;
  o.front = zc >= kSfEps;
  o.sq_err = du * du + dv * dv;
  o.over = o.sq_err > a.max_sq;
  double r = 0;
  for (int i = 0; i < 3; ++i) { o.C[i] = c.C[i]; r += (X[i] - c.C[i]) * (X[i] - c.C[i]); }
  o.r = r;
}

// How many of the lanes of `mask` start a new image: the elements of a track are grouped by image, so a flagged element opens an
// image when the flagged element before it (`last`: that of the chunks before) belongs to another one.  Called by the whole wave.
__device__ inline int sf_new_images(unsigned long long mask, int32_t im, int lane, int32_t& last) {
  if (mask == 0ull) return 0;  // wave-uniform
  const unsigned long long below = mask & ((1ull << lane) - 1ull);
  const int prev_lane = below ? 63 - __clzll((long long)below) : lane;
  int32_t prev_im = __shfl(im, prev_lane);
  if (!below) prev_im = last;
  const bool opens = ((mask >> lane) & 1ull) && prev_im != im;
  const int n = __popcll(__ballot(opens));
  last = __shfl(im, 63 - __clzll((long long)mask));
  return n;
}

__device__ inline double sf_pair_angle(const double* C1, double r1, const double* C2, double r2) {
  double b2 = 0;
  for (int k = 0; k < 3; ++k) b2 += (C1[k] - C2[k]) * (C1[k] - C2[k]);
  const double den = 2.0 * sqrt(r1 * r2);
  if (den == 0.0) return 0.0;
  double cs = (r1 + r2 - b2) / den;
  cs = cs > 1.0 ? 1.0 : (cs < -1.0 ? -1.0 : cs);
  const double ang = fabs(acos(cs));
  return fmin(ang, M_PI - ang);
}

__global__ __launch_bounds__(64 * kSfWaves) void k_scene_filter(SfArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * kSfWaves + (threadIdx.x >> 6);
  if (p >= a.n_points) return;  // whole waves leave: no workgroup barrier below
  const int64_t e0 = a.start[p], e1 = a.start[p + 1];
  const int n = (int)(e1 - e0);
  if (n == 0) return;
  const double X[3] = {a.xyz[3 * p], a.xyz[3 * p + 1], a.xyz[3 * p + 2]};
  const bool in_sel = a.point_sel ? a.point_sel[p] != 0 : true;
  const bool bundle = a.n_bundle > 0;

  // ---- the counts every decision needs, over the chunks of the track (wave-uniform trip count) ----
  int m = 0, fb = 0;                 // not in front; in front and over the error bound
  int img_all = 0, img_front = 0;    // bundle images with a flagged element / with a flagged element in front
  int32_t last_all = -1, last_front = -1;
  for (int64_t base = e0; base < e1; base += 64) {
    const int64_t e = base + lane;
    const bool valid = e < e1;
    SfElem el;
    el.im = -1; el.front = false; el.over = false;
    bool flag = false;
    if (valid) {
      const int64_t k = a.val[e];
      sf_elem(a, X, k, el);
      if (a.kp_sq_err) a.kp_sq_err[k] = el.sq_err;
      flag = bundle && a.in_bundle[el.im] != 0 && a.kp_flag[k] != 0;
    }
    m += __popcll(__ballot(valid && !el.front));
    fb += __popcll(__ballot(valid && el.front && el.over));
    if (bundle) {
      img_all += sf_new_images(__ballot(flag), el.im, lane, last_all);
      img_front += sf_new_images(__ballot(flag && el.front), el.im, lane, last_front);
    }
  }

  // ---- the decisions: the same in every lane ----
  bool removed0 = false;  // step 0 removed the elements that are not in front
  int removed_pass = 0;   // 2 / 3: pass A / B removed the bad elements
  int fate = 0, nbad = 0;
  long long neg = 0, ca = 0, cb = 0;
  bool risky = false, tested = false;
  double angle = 0.0;
  if (a.negative_depth && m > 0) {
    if (n - m >= 2) { removed0 = true; neg = m; }
    else { fate = 2; neg = n - 1 > 1 ? n - 1 : 1; }
  }
  if (fate == 0) {
    const int L = removed0 ? n - m : n;
    nbad = removed0 ? fb : m + fb;
    risky = bundle && (removed0 ? img_front : img_all) == a.n_bundle;
    if (risky || in_sel) {
      long long& changed = risky ? ca : cb;
      if (L < 2 || nbad >= L - 1) {
        fate = risky ? 3 : 5;
        changed += L;
      } else {
        changed += nbad;
        if (nbad > 0) removed_pass = risky ? 2 : 3;
        tested = true;
      }
    }
  }

  // ---- the largest pairwise angle of the good elements (in front, within the error bound) ----
  if (tested) {
    double best = 0.0;
    const int n_chunks = (n + 63) / 64;
    for (int ci = 0; ci < n_chunks; ++ci) {
      SfElem mine;
      mine.front = false; mine.over = false; mine.r = 0.0; mine.C[0] = mine.C[1] = mine.C[2] = 0.0;
      const int64_t ei = e0 + 64 * (int64_t)ci + lane;
      if (ei < e1) sf_elem(a, X, a.val[ei], mine);
      const bool good_i = ei < e1 && mine.front && !mine.over;
      for (int cj = ci; cj < n_chunks; ++cj) {
        SfElem other = mine;
        bool good_j = good_i;
        if (cj != ci) {
          const int64_t ej = e0 + 64 * (int64_t)cj + lane;
          other.front = false;
          if (ej < e1) sf_elem(a, X, a.val[ej], other);
          good_j = ej < e1 && other.front && !other.over;
        }
        unsigned long long partners = __ballot(good_j);
        while (partners) {  // wave-uniform
          const int j = __ffsll((long long)partners) - 1;
          partners &= partners - 1ull;
          const double Cj[3] = {__shfl(other.C[0], j), __shfl(other.C[1], j), __shfl(other.C[2], j)};
          const double rj = __shfl(other.r, j);
          if (good_i && !(cj == ci && lane == j)) best = fmax(best, sf_pair_angle(mine.C, mine.r, Cj, rj));
        }
      }
    }
    for (int off = 32; off > 0; off >>= 1) best = fmax(best, __shfl_xor(best, off));
    angle = best;
    if (!(angle >= (risky ? a.thr_a : a.thr_b))) {
      fate = risky ? 4 : 6;
      (risky ? ca : cb) += 1;
    } else if (risky && in_sel && !(angle >= a.thr_b)) {  // pass B finds nothing bad left and tests the same elements
      fate = 6;
      cb += 1;
    }
  }
  if (fate == 0 && (removed0 || removed_pass)) fate = 1;

  // ---- the marks of the observations that were removed on their own, where the point lives on ----
  if (fate == 1) {
    for (int64_t base = e0; base < e1; base += 64) {
      const int64_t e = base + lane;
      if (e >= e1) continue;
      const int64_t k = a.val[e];
      SfElem el;
      sf_elem(a, X, k, el);
      int mark = 0;
      if (removed0 && !el.front) mark = 1;
      else if (removed_pass && (!el.front || el.over)) mark = removed_pass;
      if (mark) a.kp_deleted[k] = (uint8_t)mark;
    }
  }
  if (lane == 0) {
    if (fate) a.fate[p] = (uint8_t)fate;
    if (risky) a.risky[p] = 1;
    if (tested && a.max_angle) a.max_angle[p] = angle;
    const long long obs = fate == 1 ? (removed0 ? m : 0) + (removed_pass ? nbad : 0) : 0;
    if (neg) atomicAdd(&a.counts[0], (unsigned long long)neg);
    if (ca) atomicAdd(&a.counts[1], (unsigned long long)ca);
    if (cb) atomicAdd(&a.counts[2], (unsigned long long)cb);
    if (fate >= 2) atomicAdd(&a.counts[3], 1ull);
    if (obs) atomicAdd(&a.counts[4], (unsigned long long)obs);
  }
}

struct SfEvent {  // the events around the track lists, whose share of the device time the call reports
  hipEvent_t e = nullptr;
  ~SfEvent() { if (e) (void)hipEventDestroy(e); }
};
}  // namespace

}  // namespace mpsfm

using namespace mpsfm;

extern "C" int mpsfm_filter_scene(const mpsfm_tri_graph* graph, const mpsfm_tri_state* state, const uint8_t* in_bundle,
                                  const uint8_t* kp_invalid_depth, const uint8_t* point_sel, const mpsfm_scene_filter_options* options,
                                  int32_t device, uint8_t* kp_deleted, uint8_t* point_fate, uint8_t* point_risky, double* point_max_angle,
                                  double* kp_sq_err, mpsfm_scene_filter_info* info) {
  if (info) *info = mpsfm_scene_filter_info{};
  SceneFilterShape s;
  const char* why = "";
  if (int rc = scene_filter_check(graph, state, in_bundle, kp_invalid_depth, options, kp_deleted, point_fate, point_risky, s, &why)) return fail(rc, why);
  scene_filter_zero(s, kp_deleted, point_fate, point_risky, point_max_angle, kp_sq_err);
  if (s.n_points == 0 || s.n_kp == 0) return 0;  // no device needed

  const int32_t n_images = graph->n_images;
  const size_t n_kp = (size_t)s.n_kp, n_points = (size_t)s.n_points;
  if (int rc = open_device(device)) return rc;
  CallScope A;
  if (int rc = A.open(true)) return rc;
  SfEvent first, mid;
  MPSFM_TRY(hipEventCreate(&first.e));
  MPSFM_TRY(hipEventCreate(&mid.e));
  SfArgs a{};
  a.n_kp = s.n_kp; a.n_points = s.n_points;
  a.n_images = n_images; a.n_bundle = s.n_bundle; a.negative_depth = options->negative_depth;
  a.max_sq = options->max_reproj_error * options->max_reproj_error;
  a.thr_a = options->risky_min_tri_angle_rad; a.thr_b = options->min_tri_angle_rad;
  a.kp_start = A.put(graph->kp_start, (size_t)n_images + 1);
  a.kp_xy = A.put(graph->kp_xy, 2 * n_kp);
  a.intr = A.put(graph->cam_intr, 4 * (size_t)n_images);
  a.quat = A.put(state->cam_quat_xyzw, 4 * (size_t)n_images);
  a.trans = A.put(state->cam_t, 3 * (size_t)n_images);
  a.kp_point = A.put(state->kp_point, n_kp);
  a.xyz = A.put(state->xyz, 3 * n_points);
  if (s.n_bundle > 0) {
    a.in_bundle = A.put(in_bundle, (size_t)n_images);
    a.kp_flag = A.put(kp_invalid_depth, n_kp);
    if (!a.in_bundle || !a.kp_flag) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  }
  if (point_sel && !(a.point_sel = A.put(point_sel, n_points))) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  a.images = A.alloc<SfImage>((size_t)n_images);
  a.kp_image = A.alloc<int32_t>(n_kp);
  a.key_in = A.alloc<uint32_t>(n_kp); a.key = A.alloc<uint32_t>(n_kp);
  a.val_in = A.alloc<uint32_t>(n_kp); a.val = A.alloc<uint32_t>(n_kp);
  a.start = A.alloc<int32_t>(n_points + 1);
  a.kp_deleted = A.alloc<uint8_t>(n_kp);
  a.fate = A.alloc<uint8_t>(n_points); a.risky = A.alloc<uint8_t>(n_points);
  a.max_angle = point_max_angle ? A.alloc<double>(n_points) : nullptr;
  a.kp_sq_err = kp_sq_err ? A.alloc<double>(n_kp) : nullptr;
  a.counts = A.alloc<unsigned long long>(5);
  unsigned long long* h_counts = A.host<unsigned long long>(5);
  if (!a.kp_start || !a.kp_xy || !a.intr || !a.quat || !a.trans || !a.kp_point || !a.xyz || !a.images || !a.kp_image || !a.key_in || !a.key ||
      !a.val_in || !a.val || !a.start || !a.kp_deleted || !a.fate || !a.risky || (point_max_angle && !a.max_angle) ||
      (kp_sq_err && !a.kp_sq_err) || !a.counts || !h_counts)
    return fail(MPSFM_ENOMEM, "hipMalloc failed");
  MPSFM_TRY(hipMemsetAsync(a.kp_deleted, 0, n_kp, A.st));
  MPSFM_TRY(hipMemsetAsync(a.fate, 0, n_points, A.st));
  MPSFM_TRY(hipMemsetAsync(a.risky, 0, n_points, A.st));
  if (a.max_angle) MPSFM_TRY(hipMemsetAsync(a.max_angle, 0, sizeof(double) * n_points, A.st));
  if (a.kp_sq_err) MPSFM_TRY(hipMemsetAsync(a.kp_sq_err, 0, sizeof(double) * n_kp, A.st));
  MPSFM_TRY(hipMemsetAsync(a.counts, 0, 5 * sizeof(unsigned long long), A.st));

  unsigned key_bits = 1;  // keys are 0 .. n_points
  while (key_bits < 32 && (s.n_points >> key_bits) != 0) ++key_bits;
  size_t sort_bytes = 0;
  MPSFM_TRY(rocprim::radix_sort_pairs(nullptr, sort_bytes, a.key_in, a.key, a.val_in, a.val, n_kp, 0, key_bits, A.st));
  void* sort_tmp = A.get(std::max<size_t>(sort_bytes, 16));
  if (!sort_tmp) return fail(MPSFM_ENOMEM, "hipMalloc failed");

  if (int rc = A.begin()) return rc;
  MPSFM_TRY(hipEventRecord(first.e, A.st));
  hipLaunchKernelGGL(k_sf_images, sf_blocks(n_images), dim3(kSfT), 0, A.st, a);
  MPSFM_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_sf_keys, sf_blocks(s.n_kp), dim3(kSfT), 0, A.st, a);
  MPSFM_TRY(hipGetLastError());
  MPSFM_TRY(rocprim::radix_sort_pairs(sort_tmp, sort_bytes, a.key_in, a.key, a.val_in, a.val, n_kp, 0, key_bits, A.st));
  hipLaunchKernelGGL(k_sf_starts, sf_blocks(s.n_points + 1), dim3(kSfT), 0, A.st, a);
  MPSFM_TRY(hipGetLastError());
  MPSFM_TRY(hipEventRecord(mid.e, A.st));
  hipLaunchKernelGGL(k_scene_filter, dim3((unsigned)((s.n_points + kSfWaves - 1) / kSfWaves)), dim3(64 * kSfWaves), 0, A.st, a);
  MPSFM_TRY(hipGetLastError());
  if (int rc = A.stop()) return rc;
  MPSFM_TRY(hipMemcpyAsync(kp_deleted, a.kp_deleted, n_kp, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipMemcpyAsync(point_fate, a.fate, n_points, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipMemcpyAsync(point_risky, a.risky, n_points, hipMemcpyDeviceToHost, A.st));
  if (point_max_angle) MPSFM_TRY(hipMemcpyAsync(point_max_angle, a.max_angle, sizeof(double) * n_points, hipMemcpyDeviceToHost, A.st));
  if (kp_sq_err) MPSFM_TRY(hipMemcpyAsync(kp_sq_err, a.kp_sq_err, sizeof(double) * n_kp, hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipMemcpyAsync(h_counts, a.counts, 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost, A.st));
  MPSFM_TRY(hipStreamSynchronize(A.st));  // the one wait of the call
  float ms = 0.f, ms_tracks = 0.f;
  if (int rc = A.elapsed(&ms)) return rc;
  MPSFM_TRY(hipEventElapsedTime(&ms_tracks, first.e, mid.e));
  if (info) {
    info->num_negative = (int64_t)h_counts[0];
    info->num_changed_a = (int64_t)h_counts[1];
    info->num_changed_b = (int64_t)h_counts[2];
    info->n_points_deleted = (int64_t)h_counts[3];
    info->n_observations_deleted = (int64_t)h_counts[4];
    info->num_syncs = 1;
    info->ms = ms;
    info->ms_tracks = ms_tracks;
  }
  return 0;
}
