// What the single and the batched descriptor matcher share on the device (k_sim_top2 / k_match_decide of descriptor_matches.hip,
// k_sim_top2_batch / k_match_decide_batch of descriptor_matches_batch.hip; the arithmetic contract and the tie rule: DESIGN.md
// sections 4m and 4q): the running top-2 of a row, one strip of 64 rows against a range of column tiles, and the decisions
// of one row.  Both matchers call these bodies, so an element goes through the same operation sequence in either and a pair's
// results are bitwise the same from both.
//
// sim_top2_strip: a workgroup of four waves owns a strip of kStrip = 64 rows and streams the columns [col_begin, col_end) in tiles
// of 64 and k in slices of kKS staged through LDS (slices are sized from the LDS budget: dim only sets how many there are).  Wave w
// holds the 16 x 64 band of rows 16 w .. 16 w + 15 as four 16 x 16 accumulators, so all candidates of a row live in the 16 lanes
// of one wave that share the row in the accumulator layout (row (lane >> 4) + 4 reg, column lane & 15).  Edge tiles are
// padded with zeros in k, rows and columns and go through the same instructions as full ones; padded columns are never
// offered as candidates, padded rows never written.
//
// Every merge (a lane's own columns, the 16 lanes of a row, column tiles, column ranges) orders candidates by (value descending,
// index ascending), a total order on distinct columns: the top-2 does not depend on the order in which candidates arrive.
#pragma once
#include "sim_tile.h"

#pragma clang fp contract(off)  // the decisions round every operation on its own

namespace mpsfm {
namespace sim {

struct Top2 { double v1, v2; int32_t i1, i2; };

__device__ __forceinline__ void offer(Top2& t, double v, int32_t i) {
  if (before(v, i, t.v1, t.i1)) { t.v2 = t.v1; t.i2 = t.i1; t.v1 = v; t.i1 = i; }
  else if (before(v, i, t.v2, t.i2)) { t.v2 = v; t.i2 = i; }
}

// The top-2 of rows row0 .. row0 + 63 of R [nrows][dim] over the columns [col_begin, col_end) of Cc [ncols][dim] (col_begin a
// multiple of kStrip), written as range z of `splits`: val / idx [nrows][splits][2].  An empty range leaves the sentinels, which
// every merge ignores.  s_A, s_B: kKS * kLd doubles of LDS each.  All arguments but the LDS contents are workgroup-uniform.
template <typename T>
__device__ __forceinline__ void sim_top2_strip(double* __restrict__ s_A, double* __restrict__ s_B, const T* __restrict__ R, int32_t nrows,
                                               int32_t row0, const T* __restrict__ Cc, int32_t ncols, int32_t col_begin, int32_t col_end,
                                               int32_t dim, bool vec, int32_t splits, int32_t z, double* __restrict__ val,
                                               int32_t* __restrict__ idx) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;

  Top2 top[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) top[r] = Top2{-INFINITY, -INFINITY, kNoIndex, kNoIndex};

  for (int32_t col0 = col_begin; col0 < col_end; col0 += kStrip) {
    v4d acc[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[ni] = v4d{0.0, 0.0, 0.0, 0.0};
    for (int32_t k0 = 0; k0 < dim; k0 += kKS) {
      __syncthreads();  // the previous slice has been read
      load_slice<T>(s_A, R, nrows, row0, dim, k0, vec);
      load_slice<T>(s_B, Cc, ncols, col0, dim, k0, vec);
      __syncthreads();
      const int steps = (min(dim - k0, kKS) + 3) >> 2;
      for (int s = 0; s < steps; ++s) {
        const int x = 8 * (s & 7);
        const double* pa = s_A + (4 * s + lg) * kLd;
        const double* pb = s_B + (4 * s + lg) * kLd;
        const double av = pa[(16 * wave + lr) ^ x];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, pb[(16 * ni + lr) ^ x], acc[ni], 0, 0, 0);
      }
    }
    // this lane's candidates of the tile: columns col0 + 16 ni + lr, rows lg + 4 r of the band
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int32_t col = col0 + 16 * ni + lr;
      if (col < ncols) {
#pragma unroll
        for (int r = 0; r < 4; ++r) offer(top[r], acc[ni][r], col);
      }
    }
  }
  // the 16 lanes that share a row
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
      const double ov1 = __shfl_xor(top[r].v1, m), ov2 = __shfl_xor(top[r].v2, m);
      const int32_t oi1 = __shfl_xor(top[r].i1, m), oi2 = __shfl_xor(top[r].i2, m);
      offer(top[r], ov1, oi1);
      offer(top[r], ov2, oi2);
    }
    const int32_t row = row0 + 16 * wave + lg + 4 * r;
    if (lr == 0 && row < nrows) {
      const size_t o = 2 * ((size_t)row * splits + z);
      val[o] = top[r].v1;
      val[o + 1] = top[r].v2;
      idx[o] = top[r].i1;
      idx[o + 1] = top[r].i2;
    }
  }
}

// the top-2 records of one direction of one pair, [rows][splits][2], and the size of its column set
struct Top2Table {
  const double* val;
  const int32_t* idx;
  int32_t splits, ncols;
};
// the tests of find_nn (squared thresholds) and what follows them
struct MatchRule {
  double ratio2, dist2, score_thr;
  int32_t use_ratio, use_dist, use_score, mutual;
};

// find_nn for one row: the match or -1, and the score
__device__ __forceinline__ int32_t nn_of(const Top2Table& t2, const MatchRule& a, int32_t row, double& score) {
  // the ranges' top-2 lists merge in the same total order: the result is the top-2 over all columns, whatever the split
  Top2 t{-INFINITY, -INFINITY, kNoIndex, kNoIndex};
  for (int z = 0; z < t2.splits; ++z) {
    const size_t o = 2 * ((size_t)row * t2.splits + z);
    offer(t, t2.val[o], t2.idx[o]);
    offer(t, t2.val[o + 1], t2.idx[o + 1]);
  }
  const double s0 = t.v1, s1 = t.v2;
  const int32_t i0 = t.i1;
  const double d0 = 2.0 * (1.0 - s0), d1 = 2.0 * (1.0 - s1);
  bool ok = i0 >= 0 && i0 < t2.ncols;
  if (a.use_ratio) ok = ok && (d0 <= a.ratio2 * d1);
  if (a.use_dist) ok = ok && (d0 <= a.dist2);
  score = ok ? (s0 + 1.0) / 2.0 : 0.0;
  return ok ? i0 : -1;
}

// matches0 / scores0 of row i of set 0: find_nn, the mutual check (dir1: the tables of the other direction, read only with it) and
// the score threshold
__device__ __forceinline__ int32_t match_of(const Top2Table& dir0, const Top2Table& dir1, const MatchRule& a, int32_t i, double& score) {
  int32_t m = nn_of(dir0, a, i, score);
  if (a.mutual && m >= 0) {
    double unused;
    if (nn_of(dir1, a, m, unused) != i) m = -1;
  }
  if (a.use_score && score < a.score_thr) m = -1;
  return m;
}

// ---- host: what both entry files check and fill the same way
inline int check_match_options(const mpsfm_match_options& o) {
  if (!std::isfinite(o.ratio_threshold) || !std::isfinite(o.distance_threshold) || !std::isfinite(o.score_threshold))
    return fail(MPSFM_EINVAL, "non-finite threshold");
  return 0;
}

inline void fill_empty(int64_t n0, int32_t* matches0, double* scores0) {
  for (int64_t i = 0; i < n0; ++i) { matches0[i] = -1; scores0[i] = 0.0; }
}

}  // namespace sim
}  // namespace mpsfm
