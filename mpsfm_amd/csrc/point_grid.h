// Fixed-radius neighbour search over a 2-D point set: a uniform cell grid kept as a SORTED CELL LIST.
//
//   cell    c = max(radius (1 + 2^-20), extent / kGridSpan), extent = the longer side of the bounding box; 1 when that is 0
//           (radius 0 over coincident points).  At most kGridSpan + 1 cells per axis whatever the bounding box: one outlier
//           at 1e7 px widens the cells, it does not grow a table.
//   coord   floor((v - v_min) / c), clamped to [-2, kGridSpan + 2] so that a query far outside the box meets no cell.  Two
//           points with |dv| <= radius lie in the same or in adjacent cells: the exact quotients differ by at most
//           radius / c <= 1 - 2^-21 and each computed quotient is off by less than 2^-38 (two roundings of 2^-53 relative
//           on a value below 2^13), so the floors differ by at most 1.
//   key     Morton code of (cx, cy), 28 bits: points sorted by key are in cell order AND a run of consecutive points covers
//           a compact patch of cells, which is what radius_nms' workgroup tiles want.
//   table   none over the cells.  The points are radix-sorted by key (rocPRIM, stable); a cell is the run of its key in the
//           sorted list, found by binary search.  Memory is O(points) and "counts, exclusive scan, scatter" is the sort.
//           grid_build() also leaves, at the first point of every occupied cell, the nine runs of its 3x3 neighbourhood,
//           so a kernel that visits the neighbourhood of the SET'S OWN points many times (the NMS rounds) searches once.
//
// Visitors: grid_visit_query() for an arbitrary query (nine searches), grid_visit_point() for a point of the set (the
// stored runs).  Both hand every candidate's sorted position to the functor, which returns false to stop; the distance
// test is the caller's (grid_d2: fp64 dx*dx + dy*dy, each operation rounded on its own).
#pragma once
#include <rocprim/device/device_radix_sort.hpp>

#include "call_scope.h"
#include "common.h"

// the <= radius^2 and < max_error^2 decisions are bit-exact against NumPy: no fused multiply-add in d2
#pragma clang fp contract(off)

namespace mpsfm {

constexpr int kGridSpan = 4096;  // cells per axis the bounding box is divided into at most
constexpr int kGridBits = 28;    // bits of a cell key: two coordinates of up to kGridSpan + 1 < 2^14
constexpr int kGridT = 256;

struct GridSpec {
  double x0, y0, cell;
};

struct Box2 {
  double lo[2], hi[2];
};

// the bounding box of pts[n][2]; false: a coordinate is not finite (n == 0: an empty box at 0)
inline bool grid_box(const double* pts, size_t n, Box2& b) {
  b = Box2{{0.0, 0.0}, {0.0, 0.0}};
  for (size_t i = 0; i < n; ++i)
    for (int d = 0; d < 2; ++d) {
      const double v = pts[2 * i + d];
      if (!std::isfinite(v)) return false;
      if (i == 0 || v < b.lo[d]) b.lo[d] = v;
      if (i == 0 || v > b.hi[d]) b.hi[d] = v;
    }
  return true;
}

inline GridSpec grid_spec(const Box2& b, double radius) {
  const double extent = std::max(b.hi[0] - b.lo[0], b.hi[1] - b.lo[1]);
  double c = std::max(radius * (1.0 + 0x1p-20), extent / kGridSpan);
  if (!(c > 0.0)) c = 1.0;
  return GridSpec{b.lo[0], b.lo[1], c};
}

__device__ __forceinline__ int grid_coord(double v, double v0, double cell) {
  const double q = floor((v - v0) / cell);
  return (int)fmin(fmax(q, -2.0), (double)(kGridSpan + 2));
}
__device__ __forceinline__ uint32_t grid_spread(uint32_t v) {  // 14 bits -> every other bit
  v &= 0x3fffu;
  v = (v | (v << 8)) & 0x00ff00ffu;
  v = (v | (v << 4)) & 0x0f0f0f0fu;
  v = (v | (v << 2)) & 0x33333333u;
  v = (v | (v << 1)) & 0x55555555u;
  return v;
}
__device__ __forceinline__ bool grid_inside(int cx, int cy) { return cx >= 0 && cy >= 0 && cx <= kGridSpan + 1 && cy <= kGridSpan + 1; }
__device__ __forceinline__ uint32_t grid_key(int cx, int cy) { return grid_spread((uint32_t)cx) | (grid_spread((uint32_t)cy) << 1); }
__device__ __forceinline__ double grid_d2(double ax, double ay, double bx, double by) {
  const double dx = ax - bx, dy = ay - by;
  return dx * dx + dy * dy;
}

// the run [s, e) of `key` in the sorted keys
__device__ __forceinline__ void grid_run(const uint32_t* __restrict__ keys, int32_t n, uint32_t key, int32_t& s, int32_t& e) {
  int32_t lo = 0, hi = n;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  s = lo;
  hi = n;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] <= key) lo = mid + 1; else hi = mid;
  }
  e = lo;
}

// device view of a built grid; positions are indices into the sorted list
struct PointGrid {
  GridSpec spec;
  int32_t n;
  const uint32_t* keys;  // [n] sorted cell keys
  const int32_t* perm;   // [n] position -> index in the caller's array
  const double2* xy;     // [n] the points in sorted order
  const int32_t* head;   // [n] position of the first point of this point's cell
  const int32_t* runs;   // [n][18] at head positions only: (start, end) of the nine neighbour cells, (0, 0) where empty
  const int32_t* stats;  // [2] occupied cells, largest cell population
};

// f(position) for every point in the 3x3 cells around the query; stops when f returns false
template <class F>
__device__ __forceinline__ void grid_visit_query(const PointGrid& g, double x, double y, F&& f) {
  const int cx = grid_coord(x, g.spec.x0, g.spec.cell), cy = grid_coord(y, g.spec.y0, g.spec.cell);
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      if (!grid_inside(cx + dx, cy + dy)) continue;
      int32_t s, e;
      grid_run(g.keys, g.n, grid_key(cx + dx, cy + dy), s, e);
      for (int32_t q = s; q < e; ++q)
        if (!f(q)) return;
    }
}
// the same for the set's own point at position p.  A cell may hold any number of points: they are streamed from memory.
template <class F>
__device__ __forceinline__ void grid_visit_point(const PointGrid& g, int32_t p, F&& f) {
  const int32_t* r = g.runs + (size_t)g.head[p] * 18;
  for (int k = 0; k < 9; ++k) {
    const int32_t s = r[2 * k], e = r[2 * k + 1];
    for (int32_t q = s; q < e; ++q)
      if (!f(q)) return;
  }
}

// the caller's index of the point nearest to (x, y) among those at squared distance strictly below e2, the lowest index among
// equidistant nearest ones; -1: there is none
__device__ __forceinline__ int32_t grid_nearest(const PointGrid& g, double x, double y, double e2) {
  double best = e2;
  int32_t id = -1;
  grid_visit_query(g, x, y, [&](int32_t q) {
    const double2 w = g.xy[q];
    const double d2 = grid_d2(x, y, w.x, w.y);
    if (!(d2 < e2)) return true;
    const int32_t k = g.perm[q];
    if (id < 0 || d2 < best || (d2 == best && k < id)) { best = d2; id = k; }
    return true;
  });
  return id;
}

namespace grid_detail {
namespace {  // one copy per translation unit that includes this header
__global__ __launch_bounds__(kGridT) void k_grid_keys(int32_t n, const double* __restrict__ pts, GridSpec sp, uint32_t* __restrict__ key,
                                                      int32_t* __restrict__ val) {
  const int32_t i = (int32_t)blockIdx.x * kGridT + (int32_t)threadIdx.x;
  if (i >= n) return;
  // points of the set lie inside the box: the clamp to >= 0 only guards the key against a stray rounding
  const int cx = max(grid_coord(pts[2 * (size_t)i], sp.x0, sp.cell), 0), cy = max(grid_coord(pts[2 * (size_t)i + 1], sp.y0, sp.cell), 0);
  key[i] = grid_key(min(cx, kGridSpan + 1), min(cy, kGridSpan + 1));
  val[i] = i;
}

__global__ __launch_bounds__(kGridT) void k_grid_cells(int32_t n, const double* __restrict__ pts, GridSpec sp, const uint32_t* __restrict__ keys,
                                                       const int32_t* __restrict__ perm, double2* __restrict__ xy, int32_t* __restrict__ head,
                                                       int32_t* __restrict__ runs, int32_t* __restrict__ stats) {
  const int32_t p = (int32_t)blockIdx.x * kGridT + (int32_t)threadIdx.x;
  if (p >= n) return;
  const int32_t i = perm[p];
  const double x = pts[2 * (size_t)i], y = pts[2 * (size_t)i + 1];
  xy[p] = make_double2(x, y);
  if (!runs) return;
  const uint32_t key = keys[p];
  if (p > 0 && keys[p - 1] == key) {
    int32_t s, e;
    grid_run(keys, n, key, s, e);
    head[p] = s;
    return;
  }
  head[p] = p;
  const int cx = min(max(grid_coord(x, sp.x0, sp.cell), 0), kGridSpan + 1), cy = min(max(grid_coord(y, sp.y0, sp.cell), 0), kGridSpan + 1);
  int32_t* r = runs + (size_t)p * 18;
  int k = 0;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx, ++k) {
      int32_t s = 0, e = 0;
      if (grid_inside(cx + dx, cy + dy)) grid_run(keys, n, grid_key(cx + dx, cy + dy), s, e);
      r[2 * k] = s; r[2 * k + 1] = e;
    }
  atomicAdd(&stats[0], 1);
  atomicMax(&stats[1], r[9] - r[8]);  // k = 4 is the cell itself
}
}  // namespace
}  // namespace grid_detail

// Builds the grid of d_pts[n][2] (device) on the scope's stream; n >= 1.  `runs` false: keys, perm and xy only (a grid that is
// only queried from outside).  Every block is the scope's and lives as long as it.
inline int grid_build(CallScope& A, int32_t n, const double* d_pts, const GridSpec& sp, bool runs, PointGrid& g) {
  using namespace grid_detail;
  uint32_t* key_in = A.alloc<uint32_t>((size_t)n);
  uint32_t* keys = A.alloc<uint32_t>((size_t)n);
  int32_t* val_in = A.alloc<int32_t>((size_t)n);
  int32_t* perm = A.alloc<int32_t>((size_t)n);
  double2* xy = A.alloc<double2>((size_t)n);
  int32_t* head = A.alloc<int32_t>((size_t)n);
  int32_t* rn = A.alloc<int32_t>(runs ? (size_t)n * 18 : 1);
  int32_t* stats = A.alloc<int32_t>(2);
  if (!key_in || !keys || !val_in || !perm || !xy || !head || !rn || !stats) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  const dim3 grid((unsigned)((n + kGridT - 1) / kGridT)), block(kGridT);
  MPSFM_TRY(hipMemsetAsync(stats, 0, 2 * sizeof(int32_t), A.st));
  hipLaunchKernelGGL(k_grid_keys, grid, block, 0, A.st, n, d_pts, sp, key_in, val_in);
  MPSFM_TRY(hipGetLastError());
  size_t bytes = 0;
  MPSFM_TRY(rocprim::radix_sort_pairs(nullptr, bytes, key_in, keys, val_in, perm, (size_t)n, 0, (unsigned)kGridBits, A.st));
  void* tmp = A.get(std::max<size_t>(bytes, 16));
  if (!tmp) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  MPSFM_TRY(rocprim::radix_sort_pairs(tmp, bytes, key_in, keys, val_in, perm, (size_t)n, 0, (unsigned)kGridBits, A.st));
  hipLaunchKernelGGL(k_grid_cells, grid, block, 0, A.st, n, d_pts, sp, keys, perm, xy, head, runs ? rn : nullptr, stats);
  MPSFM_TRY(hipGetLastError());
  g = PointGrid{sp, n, keys, perm, xy, head, rn, stats};
  return 0;
}

}  // namespace mpsfm
