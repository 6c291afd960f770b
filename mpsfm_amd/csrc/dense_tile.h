// Register / LDS building blocks of the tile Cholesky (dense_chol.hip), shared with the single-launch solver of small problems
// (local_lm.hip): the stacked panel factorisation by one wave and by the four waves of a workgroup, and the 16 x 16 quadrant
// products of v_mfma_f64_16x16x4_f64.
#pragma once
#include "common.h"

namespace mpsfm {

constexpr int kTile = 32;
constexpr int kTileElems = kTile * kTile;

__device__ __forceinline__ double readlane_f64(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l),
                          __builtin_amdgcn_readlane(__double2loint(v), l));
}
// 1/sqrt(d): v_rsq_f64 seed + two Newton steps (off the exact-sqrt/divide latency chain)
__device__ __forceinline__ double rsqrt_nr(double d) {
  double y = __builtin_amdgcn_rsq(d);
  const double hd = 0.5 * d;
  y = y * __builtin_fma(-hd * y, y, 1.5);
  y = y * __builtin_fma(-hd * y, y, 1.5);  // second step kept: v_rsq_f64 alone is good to ~2^-26
  return y;
}

#define MPSFM_PIN(x) asm volatile("" : "+v"(x))

// ---- stacked panel factorisation: Cholesky of the diagonal tile and the solve of the workgroup's own tile in ONE wave --
// Lane i < 32 holds row i of the (updated, symmetric, both triangles valid) diagonal tile D, lane 32 + i holds row i of
// the workgroup's own tile X (or of the identity for the workgroup that owns the diagonal tile).  The column
// operations of a Cholesky panel factorisation of the stacked 64 x 32 matrix [D; X] are the same for both halves —
//   l_iJ = a_iJ / sqrt(d_J),   a_ic -= l_iJ l_cJ  (c > J)
// — so the triangular solve X L^-T costs no instruction of its own and needs no second wave, no hand-shake and no
// LDS traffic per column.
//
// One wave issues one instruction per ~4-5 cycles (fp64 multiply-add: 5.5, v_readlane: 4.9, v_rsq_f64 / v_rcp_f64: 16.5;
// a dependent fp64 op waits 8 — scripts/micro/f64_issue.hip), and the 496 rank-1 multiply-adds per lane are fixed, so
// the factorisation is bound by its INSTRUCTION COUNT: per column one transcendental (v_rsq_f64 + one cubic step
// y = y0 (1 + e/2 + 3e^2/8), e = 1 - d y0^2: v_rsq_f64 is good to ~2^-26, the step to ~e^3), the scaling l = a y, and
// the rank-1 update with the multipliers l_cJ broadcast
//   inside a panel of kSP columns   by v_readlane (they sit in lane c, register J — the matrix is symmetric),
//   beyond the panel                from LDS: after a panel its kSP columns of L (rows < 32) are written once and come
//                                   back as uniform-address ds_read_b128; the next panel's columns get the rank-kSP
//                                   update at once, the columns beyond get it one column of L per column of the next
//                                   panel (filling the issue slots its dependent chain leaves empty).
constexpr int kSP = 8;

// Broadcast reads of L rows from LDS are issued in ONE batch well before their use, as explicit ds_read_b128 with one
// s_waitcnt in front of the consumers: left to itself the compiler issues two or three reads and waits for them
// (s_waitcnt lgkmcnt(0)) ten times per panel boundary, exposing the LDS latency each time (0.45 us per boundary
// measured).  LDS operations of a wave return in order, so the compiler's own counted waits stay correct beside these.
typedef double v2d __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t lds_addr(const double* p) { return (uint32_t)(uintptr_t)p; }  // low 32 bits of a __shared__ address = LDS offset
template <int N>
__device__ __forceinline__ void lds_row_load(uint32_t addr, v2d (&m)[N]) {
#pragma unroll
  for (int q = 0; q < N; ++q) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(m[q]) : "v"(addr), "n"(16 * q));
}
// the loaded values pass through the wait, so no consumer can be scheduled in front of it
__device__ __forceinline__ void lds_wait(v2d (&m)[4]) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(m[0]), "+v"(m[1]), "+v"(m[2]), "+v"(m[3])); }
__device__ __forceinline__ void lds_wait(v2d (&m)[8]) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(m[0]), "+v"(m[1]), "+v"(m[2]), "+v"(m[3]), "+v"(m[4]), "+v"(m[5]), "+v"(m[6]), "+v"(m[7]));
}
__device__ __forceinline__ void lds_wait(v2d (&m)[1]) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(m[0])); }

// END (a multiple of kSP): the columns from END on are padding — identity rows in D, zeros in X — and stay what they are, so the
// factorisation stops there (the last tile column of a small system, local_lm.hip)
template <int J0, int J, int END>
__device__ __forceinline__ void stacked_col(double (&a)[kTile], const double* s_P, bool& ok) {
  constexpr int C = J0 + J;
  constexpr bool kHasFar = (J0 > 0) && (J0 + kSP < END);  // the previous panel still owes the columns beyond this panel
  constexpr int F0 = J0 + kSP, NF = kHasFar ? (END - F0) / 2 : 1;
  // column J of the previous panel for the far columns [F0, 32): requested first, consumed after the chain below
  v2d mf[NF];
  if constexpr (kHasFar) lds_row_load<NF>(lds_addr(s_P + J * kTile + F0), mf);
  const double d = readlane_f64(a[C], C);
  ok = ok && (d > 0.0) && isfinite(d);
  const double y0 = __builtin_amdgcn_rsq(d);
  const double h = d * y0;
  const double e = __builtin_fma(-h, y0, 1.0);
  const double p = __builtin_fma(0.375 * e, e, 0.5 * e);
  const double y = __builtin_fma(y0, p, y0);
  const double l = a[C] * y;
  a[C] = l;
#pragma unroll
  for (int c = J + 1; c < kSP; ++c) a[J0 + c] = __builtin_fma(-l, readlane_f64(l, J0 + c), a[J0 + c]);
  if constexpr (kHasFar) {
    const double lk = a[J0 - kSP + J];
    lds_wait(mf);
#pragma unroll
    for (int q = 0; q < NF; ++q) {
      a[F0 + 2 * q] = __builtin_fma(-lk, mf[q].x, a[F0 + 2 * q]);
      a[F0 + 2 * q + 1] = __builtin_fma(-lk, mf[q].y, a[F0 + 2 * q + 1]);
    }
  }
  if constexpr (J + 1 < kSP) stacked_col<J0, J + 1, END>(a, s_P, ok);
}

template <int J0, int END = kTile>
__device__ __forceinline__ void stacked_panel(double (&a)[kTile], int lane, double* s_P, bool& ok) {
  static_assert(END % kSP == 0 && END <= kTile, "whole panels");
  stacked_col<J0, 0, END>(a, s_P, ok);
  if constexpr (J0 + kSP < END) {
    // columns J0 .. J0+kSP-1 of L, rows < 32: s_P[k][c] = L[c][J0 + k].  The far updates of the previous panel read
    // s_P during this panel: they are all issued by now (one wave, DS operations complete in order).
    __builtin_amdgcn_wave_barrier();
    if (lane < kTile) {
#pragma unroll
      for (int k = 0; k < kSP; ++k) s_P[k * kTile + lane] = a[J0 + k];
    }
    // one wave: its DS operations complete in order, so the reads below see the stores above; only the compiler must
    // be kept from moving them (workgroup-scope fences here cost ~0.3 us per panel boundary)
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    // rank-kSP update of the next panel's columns (its chain starts on them): all reads first, two batches
    {
      // 4 reads per column of L; two halves of 16 reads (at most 15 LDS operations are in flight, and 32 rows at once
      // would push the wave past its 256 registers)
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        v2d m[kSP / 2][kSP / 2];
#pragma unroll
        for (int k = 0; k < kSP / 2; ++k) lds_row_load<kSP / 2>(lds_addr(s_P + (half * (kSP / 2) + k) * kTile + J0 + kSP), m[k]);
#pragma unroll
        for (int k = 0; k < kSP / 2; ++k) lds_wait(m[k]);
#pragma unroll
        for (int k = 0; k < kSP / 2; ++k) {
#pragma unroll
          for (int q = 0; q < kSP / 2; ++q) {
            a[J0 + kSP + 2 * q] = __builtin_fma(-a[J0 + half * (kSP / 2) + k], m[k][q].x, a[J0 + kSP + 2 * q]);
            a[J0 + kSP + 2 * q + 1] = __builtin_fma(-a[J0 + half * (kSP / 2) + k], m[k][q].y, a[J0 + kSP + 2 * q + 1]);
          }
        }
      }
    }
    stacked_panel<J0 + kSP, END>(a, lane, s_P, ok);
  }
}

// ---- the same factorisation by the FOUR waves of a workgroup ---------------------------------------------------------------
// The one-wave panel is bound by the instruction count of its wave, and most of those instructions are rank-1 updates of
// columns that are not on the dependent chain yet.  Here wave w holds columns 8 w .. 8 w + 7 of all 64 rows (lane = row, as
// above: 8 doubles per lane).  For p = 0..3: wave p runs the in-panel chain of stacked_col on its columns (source lane
// 8 p + c), writes its 8 columns of L for all 64 rows to LDS, and behind ONE workgroup barrier every wave q > p applies the
// rank-8 update  a[c] = fma(-L[row][8p+k], L[8q+c][8p+k], a[c])  in ascending k: every element receives the operations of
// the one-wave path with the same operands in the same order, so the two paths agree bit for bit.
// LDS: panel p has rows of its own (none is reused, so a hand-off needs no second barrier against overwriting); a row is
// padded to kWgLd doubles, which keeps the 16-byte pieces of neighbouring lanes in different banks.
constexpr int kWgWaves = kTile / kSP;                  // 4
constexpr int kWgLd = kSP + 2;                         // doubles per row of a stored panel
constexpr int kWgPanel = 2 * kTile * kWgLd;            // doubles per stored panel
constexpr int kWgLds = kWgWaves * kWgPanel;            // the last panel is stored too: no branch in the chain
static_assert(kWgLd % 2 == 0, "rows of a stored panel stay 16-byte aligned");

// column J of the wave's panel, d: its pivot (wave-uniform).  dst: this lane's row of the stored panel — every column of L
// is stored as soon as it is final, so that only the last store is still in flight at the barrier.
// The one-wave chain goes through two lane broadcasts per column (the multiplier of row J + 1, then the updated pivot).  Here
// every lane forms the NEXT pivot itself, from the two elements of row J + 1 it depends on (broadcast before y is known, off
// the chain) and with the operations lane J + 1 applies to them — lb = a[J] y and fma(-lb, lb, a[J+1]) — so the value is the
// one the broadcast would have delivered, bit for bit, and the chain per column is v_rsq_f64 and seven multiply-adds.
template <int J>
__device__ __forceinline__ void wg_panel_col(double (&a)[kSP], int c0, double* dst, bool& ok, double d) {
  ok = ok && (d > 0.0) && isfinite(d);
  double vb = 0.0, a11 = 0.0;
  if constexpr (J + 1 < kSP) {
    vb = readlane_f64(a[J], c0 + J + 1);
    a11 = readlane_f64(a[J + 1], c0 + J + 1);
  }
  const double y0 = __builtin_amdgcn_rsq(d);
  const double h = d * y0;
  const double e = __builtin_fma(-h, y0, 1.0);
  const double p = __builtin_fma(0.375 * e, e, 0.5 * e);
  const double y = __builtin_fma(y0, p, y0);
  const double l = a[J] * y;
  a[J] = l;
  dst[J] = l;
  if constexpr (J + 1 < kSP) {
    const double lb = vb * y;                          // l of lane c0 + J + 1
    const double dn = __builtin_fma(-lb, lb, a11);     // its a[J + 1] after this column: the next pivot
    a[J + 1] = __builtin_fma(-l, lb, a[J + 1]);
#pragma unroll
    for (int c = J + 2; c < kSP; ++c) a[c] = __builtin_fma(-l, readlane_f64(l, c0 + c), a[c]);
    wg_panel_col<J + 1>(a, c0, dst, ok, dn);
  }
}

// A hand-off reads, per lane, the 8 own multipliers L[row][8p + k] and the 64 broadcast ones L[8 wave + c][8p + k] as 36
// ds_read_b128, in four groups of k pairs (one own read, eight broadcast reads).  Two groups are in flight while the
// multiply-adds of the group before run: LDS operations return in order, so a counted wait that leaves the 9 newest reads
// outstanding has the group before them in registers.
template <int KK>
__device__ __forceinline__ void wg_group_load(uint32_t a_own, uint32_t a_bc, v2d (&own)[kSP / 2], v2d (&bc)[kSP / 2][kSP]) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(own[KK]) : "v"(a_own), "n"(16 * KK));
#pragma unroll
  for (int c = 0; c < kSP; ++c) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(bc[KK][c]) : "v"(a_bc), "n"(c * kWgLd * 8 + 16 * KK));
}
template <int CNT>
__device__ __forceinline__ void wg_group_wait(v2d& o, v2d (&b)[kSP]) {
  asm volatile("s_waitcnt lgkmcnt(%9)"
               : "+v"(o), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), "+v"(b[4]), "+v"(b[5]), "+v"(b[6]), "+v"(b[7])
               : "n"(CNT));
}
__device__ __forceinline__ void wg_group_fma(double (&a)[kSP], const v2d& o, const v2d (&b)[kSP]) {
#pragma unroll
  for (int c = 0; c < kSP; ++c) a[c] = __builtin_fma(-o.x, b[c].x, a[c]);  // k = 2 KK, then k = 2 KK + 1: ascending per element
#pragma unroll
  for (int c = 0; c < kSP; ++c) a[c] = __builtin_fma(-o.y, b[c].y, a[c]);
}

// `wave` must be wave-uniform (a scalar); every wave of the workgroup calls this, all of them reach its three barriers.
// s_P: kWgLds doubles, 16-byte aligned.  ok: pivots of this wave's own columns.  tr (diagnostics, may be NULL): wall_clock64 of
// the end of panel p's chain in tr[2 p], of the end of the update of panel p + 1 by panel p in tr[2 p + 1].
__device__ __forceinline__ void stacked_panel_wg(double (&a)[kSP], int lane, int wave, double* s_P, bool& ok, long long* tr) {
#pragma nounroll
  for (int p = 0; p < kWgWaves; ++p) {
    if (wave == p) {
      wg_panel_col<0>(a, kSP * p, s_P + p * kWgPanel + lane * kWgLd, ok, readlane_f64(a[0], kSP * p));
      if (tr && lane == 0) tr[2 * p] = wall_clock64();
    }
    if (p + 1 == kWgWaves) break;
    __syncthreads();
    asm volatile("" ::: "memory");
    if (wave > p) {
      // only wave p + 1 is waited for: the waves behind it let its reads go first
      if (wave > p + 1) __builtin_amdgcn_s_sleep(3);
      const uint32_t a_own = lds_addr(s_P + p * kWgPanel + lane * kWgLd), a_bc = lds_addr(s_P + p * kWgPanel + kSP * wave * kWgLd);
      v2d own[kSP / 2], bc[kSP / 2][kSP];
      wg_group_load<0>(a_own, a_bc, own, bc);
      wg_group_load<1>(a_own, a_bc, own, bc);
      wg_group_wait<kSP + 1>(own[0], bc[0]);
      wg_group_fma(a, own[0], bc[0]);
      wg_group_load<2>(a_own, a_bc, own, bc);
      wg_group_wait<kSP + 1>(own[1], bc[1]);
      wg_group_fma(a, own[1], bc[1]);
      wg_group_load<3>(a_own, a_bc, own, bc);
      wg_group_wait<kSP + 1>(own[2], bc[2]);
      wg_group_fma(a, own[2], bc[2]);
      wg_group_wait<0>(own[3], bc[3]);
      wg_group_fma(a, own[3], bc[3]);
      if (tr && wave == p + 1 && lane == 0) tr[2 * p + 1] = wall_clock64();
    }
  }
}

// ---- 16 x 16 quadrants of a 32 x 32 tile in the accumulator layout of v_mfma_f64_16x16x4_f64 (one per wave) -----------
// element r of lane l sits at row 16 mi + (l >> 4) + 4 r, column 16 ni + (l & 15)
template <typename Ptr>
__device__ __forceinline__ void quad_load(Ptr T, int ld, int lane, int mi, int ni, v4d& acc) {
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] = T[(16 * mi + (lane >> 4) + 4 * r) * ld + 16 * ni + (lane & 15)];
}
template <typename Ptr>
__device__ __forceinline__ void quad_store(Ptr T, int ld, int lane, int mi, int ni, const v4d& acc) {
#pragma unroll
  for (int r = 0; r < 4; ++r) T[(16 * mi + (lane >> 4) + 4 * r) * ld + 16 * ni + (lane & 15)] = acc[r];
}
// operands of a quadrant product over k = 0..31: lane l takes row 16 b + (l & 15), columns 8 (l >> 4) .. + 7 of a row-major
// tile (the k index is permuted identically for both operands, which leaves the sum unchanged: 64 contiguous bytes per lane)
__device__ __forceinline__ void quad_operand(const double* __restrict__ T, int lane, int b, double (&o)[8]) {
  const double2* p = reinterpret_cast<const double2*>(T + (16 * b + (lane & 15)) * kTile + 8 * (lane >> 4));
#pragma unroll
  for (int s = 0; s < 4; ++s) { const double2 x = p[s]; o[2 * s] = x.x; o[2 * s + 1] = x.y; }
}
// acc -= A[16 mi .., :] B[16 ni .., :]^T
__device__ __forceinline__ void quad_gemm_sub(const double (&a)[8], const double (&b)[8], v4d& acc) {
#pragma unroll
  for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[s], b[s], acc, 0, 0, 0);
}

}  // namespace mpsfm
