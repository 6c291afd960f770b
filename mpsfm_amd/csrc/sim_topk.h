// The running top-k of a row of similarities (k_sim_topk / k_topk_merge of retrieval.hip; the contract, the tie rule and the
// margins: DESIGN.md section 4r).  sim_top2.h keeps the two best candidates of a row in registers; here a row keeps its
// num_select <= kMaxSelect best in LDS, and the strip is otherwise the same: tile geometry, slices, load_slice(), before() of
// sim_tile.h.
//
// Arithmetic contract (the one of DESIGN.md section 4m).  Operands are fp32 values.  A similarity is the fp64 dot product
// accumulated with k ascending by v_mfma_f64_16x16x4_f64.  Every element goes through the same instruction sequence wherever it
// sits: edge tiles are padded with zeros in k, rows and columns.  So identical descriptors give bitwise identical similarities.
//
// Candidates of row i: every column j but those a test removes, which are never offered and never occupy a slot:
//   identity  query_id[i] == db_id[j]   (both id arrays given)
//   score     sim < min_score           (use_min; a similarity EQUAL to min_score stays)
// Result of row i: the first num_select candidates under the order (value descending, index ascending), in that order.  The
// order is total on distinct columns and every merge (a tile into the row's list, the ranges of a row) places an element by
// COUNTING the elements that come before() it, so the result is a function of the set of candidates only: not of tile order, lane
// order, column ranges or scheduling.  There is no atomic operation in either kernel.
//
// sim_topk_strip.  A workgroup of four waves owns a strip of kStrip = 64 rows and streams the columns [col_begin, col_end) in tiles
// of 64 and k in slices of kKS through LDS, exactly as sim_top2_strip does.  Wave w holds rows 16 w .. 16 w + 15; the 16 lanes that
// share a row in the accumulator layout (row (lane >> 4) + 4 reg, column lane & 15) own that row's list: K (value, column) entries
// in LDS, sorted, with the count and the current K-th entry (the admission threshold) in registers.  After the products of a tile
//   1. the candidates that pass the tests AND come before the threshold are compacted into a staging area by ballot and prefix
//      count (the slice buffer of the columns is free between two tiles: one barrier), at most 64 per row;
//   2. every old entry counts the survivors before it and every survivor counts the old entries (binary search) and the survivors
//      before it: the counts are the positions in the merged list, unique because the order is total;
//   3. after all reads, entries with a position below K are stored there.
// A wave touches the lists and the staging area of its own rows only, so the steps are ordered by the wave's in-order LDS pipe
// and a compiler barrier; a wave whose 16 rows admit nothing from a tile skips 2 and 3.
//
// LDS: two slices of kKS x kLd doubles (40 KiB) and 64 rows x K x 12 B: 55 KiB at K = 20 (two workgroups per compute unit of
// 160 KiB), 136 KiB at K = 128 (one).
#pragma once
#include "sim_tile.h"

#pragma clang fp contract(off)  // the decisions round every operation on its own

namespace mpsfm {
namespace sim {

constexpr int kMaxSelect = 128;           // entries of a row's list
constexpr int32_t kMaxDimTopk = 65536;    // the slice staging does not depend on dim: an argument check only
constexpr int kMaxRanges = 4096;          // column ranges of a strip: one byte of LDS per range in k_topk_merge
constexpr int kOldPerLane = kMaxSelect / 16, kNewPerLane = kStrip / 16;

inline size_t topk_lds_bytes(int32_t K) { return 2 * sizeof(double) * kKS * kLd + (size_t)kStrip * K * (sizeof(double) + sizeof(int32_t)); }

// what removes a column from the candidates of a row
struct TopkRule {
  const int32_t* qid;  // [nrows] or NULL
  const int32_t* did;  // [ncols] or NULL: both or neither
  double min_score;
  int32_t use_min;
};

// keeps the compiler from moving LDS accesses across this point; the wave's DS operations complete in order
__device__ __forceinline__ void wave_lds_order() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}

// The top-K of rows row0 .. row0 + 63 of R [nrows][dim] over the columns [col_begin, col_end) of Cc [ncols][dim] (col_begin a
// multiple of kStrip), written as range z of `splits`: val / idx [nrows][splits][K], sorted, the tail (-inf, kNoIndex): sentinels
// that no merge prefers (an empty range writes nothing else).  lds: topk_lds_bytes(K) bytes, 16-byte aligned.  All arguments but the
// LDS contents are workgroup-uniform.
__device__ __forceinline__ void sim_topk_strip(double* __restrict__ lds, const float* __restrict__ R, int32_t nrows, int32_t row0,
                                               const float* __restrict__ Cc, int32_t ncols, int32_t col_begin, int32_t col_end, int32_t dim, bool vec,
                                               const TopkRule& rule, int32_t K, int32_t splits, int32_t z, double* __restrict__ val,
                                               int32_t* __restrict__ idx) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  double* s_A = lds;
  double* s_B = lds + kKS * kLd;
  double* Lv = lds + 2 * kKS * kLd;                             // [64][K]
  int32_t* Li = reinterpret_cast<int32_t*>(Lv + (size_t)kStrip * K);  // [64][K]
  // staging of this wave between two tiles, inside s_B: [4 row groups][64] values, then as many columns
  double* sv = s_B + wave * (kKS * kLd / 4) + lg * kStrip;
  int32_t* si = reinterpret_cast<int32_t*>(s_B + wave * (kKS * kLd / 4) + 4 * kStrip) + lg * kStrip;
  static_assert(kKS * kLd / 4 >= 4 * kStrip + 2 * kStrip, "a wave's staging fits its quarter of a slice");

  int32_t cnt[4], thr_i[4], qid[4];
  double thr_v[4];
  const bool use_ids = rule.qid != nullptr;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    cnt[r] = 0;
    thr_v[r] = -INFINITY;
    thr_i[r] = kNoIndex;
    const int32_t row = row0 + 16 * wave + lg + 4 * r;
    qid[r] = (use_ids && row < nrows) ? rule.qid[row] : 0;
  }

  for (int32_t col0 = col_begin; col0 < col_end; col0 += kStrip) {
    v4d acc[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[ni] = v4d{0.0, 0.0, 0.0, 0.0};
    for (int32_t k0 = 0; k0 < dim; k0 += kKS) {
      __syncthreads();  // the previous slice and the previous tile's staging have been read
      load_slice<float>(s_A, R, nrows, row0, dim, k0, vec);
      load_slice<float>(s_B, Cc, ncols, col0, dim, k0, vec);
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
    __syncthreads();  // every wave has read the last slice: s_B is the staging area until the next tile's first barrier
    // this lane's columns of the tile, col0 + 16 ni + lr, and what the identity test needs of them
    bool col_ok[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) col_ok[ni] = col0 + 16 * ni + lr < ncols;
    int32_t did[4] = {0, 0, 0, 0};
    if (use_ids) {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        if (col_ok[ni]) did[ni] = rule.did[col0 + 16 * ni + lr];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {  // row lg + 4 r of the band: the 16 lanes of group lg
      const int32_t Rl = 16 * wave + lg + 4 * r;
      const bool row_ok = row0 + Rl < nrows;
      // 1. survivors, compacted in the order (ni, lane): a function of the tile alone
      int32_t ns = 0;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int32_t col = col0 + 16 * ni + lr;
        const double v = acc[ni][r];
        bool ok = row_ok && col_ok[ni] && before(v, col, thr_v[r], thr_i[r]);
        if (use_ids) ok = ok && qid[r] != did[ni];
        if (rule.use_min) ok = ok && !(v < rule.min_score);
        const unsigned long long m = __ballot(ok);
        const uint32_t grp = (uint32_t)(m >> (16 * lg)) & 0xffffu;
        const int32_t pos = ns + __popc(grp & ((1u << lr) - 1u));
        if (ok) { sv[pos] = v; si[pos] = col; }
        ns += __popc(grp);
      }
      if (__ballot(ns > 0) == 0ull) continue;  // wave-uniform: none of the four rows admits anything
      wave_lds_order();
      // 2. positions in the merged list
      double* lv = Lv + (size_t)Rl * K;
      int32_t* li = Li + (size_t)Rl * K;
      const int32_t n_old = cnt[r];
      double ov[kOldPerLane], mv[kNewPerLane];
      int32_t oi[kOldPerLane], opos[kOldPerLane], mi[kNewPerLane], mpos[kNewPerLane];
#pragma unroll
      for (int q = 0; q < kOldPerLane; ++q) {
        const int32_t p = lr + 16 * q;
        const bool have = p < n_old;
        ov[q] = have ? lv[p] : -INFINITY;
        oi[q] = have ? li[p] : kNoIndex;
        opos[q] = p;
      }
#pragma unroll
      for (int t = 0; t < kNewPerLane; ++t) {
        const int32_t s = lr + 16 * t;
        const bool have = s < ns;
        mv[t] = have ? sv[s] : -INFINITY;
        mi[t] = have ? si[s] : kNoIndex;
        int32_t lo = 0, hi = have ? n_old : 0;  // old entries before this survivor
        while (lo < hi) {
          const int32_t mid = (lo + hi) >> 1;
          if (before(lv[mid], li[mid], mv[t], mi[t])) lo = mid + 1; else hi = mid;
        }
        mpos[t] = lo;
      }
      for (int32_t s = 0; s < ns; ++s) {
        const double cv = sv[s];
        const int32_t ci = si[s];
#pragma unroll
        for (int q = 0; q < kOldPerLane; ++q) opos[q] += before(cv, ci, ov[q], oi[q]) ? 1 : 0;
#pragma unroll
        for (int t = 0; t < kNewPerLane; ++t) mpos[t] += before(cv, ci, mv[t], mi[t]) ? 1 : 0;
      }
      wave_lds_order();  // all reads of the lists are done
      // 3. the merged list
#pragma unroll
      for (int q = 0; q < kOldPerLane; ++q)
        if (lr + 16 * q < n_old && opos[q] < K) { lv[opos[q]] = ov[q]; li[opos[q]] = oi[q]; }
#pragma unroll
      for (int t = 0; t < kNewPerLane; ++t)
        if (lr + 16 * t < ns && mpos[t] < K) { lv[mpos[t]] = mv[t]; li[mpos[t]] = mi[t]; }
      wave_lds_order();
      cnt[r] = min(K, n_old + ns);
      if (cnt[r] == K) { thr_v[r] = lv[K - 1]; thr_i[r] = li[K - 1]; }
    }
  }
  // the lists of this range
  wave_lds_order();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int32_t Rl = 16 * wave + lg + 4 * r, row = row0 + Rl;
    if (row >= nrows) continue;
    const size_t o = ((size_t)row * splits + z) * K;
    for (int32_t p = lr; p < K; p += 16) {
      const bool have = p < cnt[r];
      val[o + p] = have ? Lv[(size_t)Rl * K + p] : -INFINITY;
      idx[o + p] = have ? Li[(size_t)Rl * K + p] : kNoIndex;
    }
  }
}

// The final list of one row from the sorted lists of its ranges, val / idx [rows][splits][K]: slot by slot the head that comes
// before() all other heads.  One wave per row; lane l owns the heads of the ranges l, l + 64, ...  (heads: kMaxRanges bytes of LDS).
// indices / scores [rows][K] padded with -1 / 0, counts [rows].
__device__ __forceinline__ void topk_merge_row(uint8_t* __restrict__ heads, const double* __restrict__ val, const int32_t* __restrict__ idx,
                                               int32_t row, int32_t splits, int32_t K, int32_t* __restrict__ indices, double* __restrict__ scores,
                                               int32_t* __restrict__ counts) {
  const int lane = (int)threadIdx.x;
  for (int32_t zz = lane; zz < splits; zz += 64) heads[zz] = 0;
  const size_t base = (size_t)row * splits * K;
  int32_t count = 0;
  for (; count < K; ++count) {
    double bv = -INFINITY;
    int32_t bi = kNoIndex, bz = 0;
    for (int32_t zz = lane; zz < splits; zz += 64) {
      const int32_t h = heads[zz];
      if (h >= K) continue;
      const size_t o = base + (size_t)zz * K + h;
      const double v = val[o];
      const int32_t i = idx[o];
      if (before(v, i, bv, bi)) { bv = v; bi = i; bz = zz; }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      const double ov = __shfl_xor(bv, m);
      const int32_t oi = __shfl_xor(bi, m), oz = __shfl_xor(bz, m);
      if (before(ov, oi, bv, bi)) { bv = ov; bi = oi; bz = oz; }
    }
    if (bi == kNoIndex) break;  // only sentinels are left: the same on every lane
    if (lane == 0) { indices[(size_t)row * K + count] = bi; scores[(size_t)row * K + count] = bv; }
    if ((bz & 63) == lane) heads[bz] = (uint8_t)(heads[bz] + 1);  // read and written by its owner alone
  }
  for (int32_t s = count + lane; s < K; s += 64) { indices[(size_t)row * K + s] = -1; scores[(size_t)row * K + s] = 0.0; }
  if (lane == 0) counts[row] = count;
}

}  // namespace sim
}  // namespace mpsfm
