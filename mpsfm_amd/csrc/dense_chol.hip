// Dense solve of the reduced camera system (gfx950): what Ceres' SPARSE_SCHUR hands to CHOLMOD
// (reference call site mpsfm/sfm/mapper/bundle_adjustment.py:285-293), done here as a tiled
// right-looking Cholesky on fp64 MFMA (v_mfma_f64_16x16x4_f64).
//
// Storage: lower triangle of 32x32 tiles, tile (ti, tj) at lt_tile(ti, tj) * 1024 doubles,
// row-major inside a tile.  Tile row `nt` (one extra) carries the right-hand side in its row 0, so
// the forward substitution z = L^-1 rhs falls out of the factorisation; k_backsub then solves
// L^T y = z.
#include "../../include/mpsfm_hip_debug.h"
#include "common.h"
#include "ba_launch.h"
#include "dense_tile.h"
#include "dev_resources.h"

namespace mpsfm {

constexpr int kPlainMaxTiles = 64;  // up to this many tile columns: one outer panel, inverse propagation instead of back substitution

// four elements (rows r0 + k * rstep, k < 4, column c) of tile (ti, tj) of the damped reduced system [S + D / radius | rhs row];
// tile row nt carries the right-hand side in its row 0.  Branch-free per element, so that the three dependent loads
// (column -> slot, slot pair -> block, block -> value) of the four elements overlap.
__device__ __forceinline__ void assemble_quad(const AssembleArgs& P, double lm_radius, int ti, int tj, int r0, int rstep, int c, double out[4]) {
  const int n = P.n;
  const int C = tj * kTile + c;
  const int ic = vec_index(P.col_slot, C, n);
  if (ti == P.nt) {
    const double rhs = (tj < P.nt && ic >= 0) ? P.wv[ic] - P.gc[ic] : 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = (r0 + k * rstep == 0) ? rhs : 0.0;
    return;
  }
  const int icv = ic >= 0 ? ic : 0;
  const int bc = icv / 6, b = icv - bc * 6;
  int ir[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) ir[k] = vec_index(P.col_slot, ti * kTile + r0 + k * rstep, n);
  int64_t off[4];
  bool has[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool real = ir[k] >= 0 && ic >= 0;
    const int irv = ir[k] >= 0 ? ir[k] : 0;
    const int br = irv / 6, a = irv - br * 6;
    const int lo = br < bc ? br : bc, hi = br < bc ? bc : br;
    int64_t blk;
    if (P.sky.index) blk = P.sky.index[(int64_t)hi * P.sky.ns + lo];
    else blk = lo >= P.sky.first[hi] ? P.sky.start[hi] + (lo - P.sky.first[hi]) : -1;
    has[k] = real && blk >= 0;  // no landmark shared by the two cameras: structurally zero
    // the stored block is (lo, hi): transposed when the row's camera comes second; the diagonal block holds its upper triangle
    const int e = br < bc ? a * 6 + b : br > bc ? b * 6 + a : (a <= b ? a * 6 + b : b * 6 + a);
    off[k] = has[k] ? blk * 36 + e : 0;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double v = P.Sblk[off[k]];
    const int R = ti * kTile + r0 + k * rstep;
    const bool real = ir[k] >= 0 && ic >= 0;
    out[k] = has[k] ? v : (!real && R == C) ? 1.0 : 0.0;  // padding columns (tile alignment of the dissection's parts, tail of the last tile): identity
    if (real && R == C) out[k] += fmin(fmax(P.diagU[ir[k]], P.min_diag), P.max_diag) / lm_radius;
  }
}
// one workgroup (256 threads): tile (ti, tj) of the system and / or a zero for its inverse accumulator
// v: the thread's four elements from assemble_quad (rows (e >> 5) + 8 k, column e & 31 for e = threadIdx.x), read when `write`
__device__ __forceinline__ void assemble_tile(const AssembleArgs& P, int ti, int tj, bool write, const double (&v)[4]) {
  const int64_t id = lt_tile(ti, tj);
  if (P.Pinv && ti < P.nt && tj < ti)
    for (int e = threadIdx.x; e < kTileElems; e += 256) P.Pinv[id * kTileElems + e] = 0.0;
  if (!write) return;
  double* T = P.A + id * kTileElems;
  const int e = threadIdx.x;  // elements e + 256 k
#pragma unroll
  for (int k = 0; k < 4; ++k) T[e + 256 * k] = v[k];
}

// one workgroup per lower tile (including the rhs tile row)
__global__ __launch_bounds__(256) void k_assemble(AssembleArgs P) {
  // `term`, the radius and the tile id are requested together; `term` is tested in front of the first store (lm_term_chain)
  const int32_t term = lm_term_chain(P.ctl);
  const double lm_radius = lm_radius_chain(P.ctl, P.radius);
  // decode tile id -> (ti, tj), ti >= tj, ti in [0, nt], tj in [0, nt-1]
  const int64_t id = P.tile_list ? (int64_t)P.tile_list[blockIdx.x] : (int64_t)blockIdx.x;
  int ti = (int)((sqrt(8.0 * (double)id + 1.0) - 1.0) * 0.5);
  while ((int64_t)ti * (ti + 1) / 2 > id) --ti;
  while ((int64_t)(ti + 1) * (ti + 2) / 2 <= id) ++ti;
  const int tj = (int)(id - (int64_t)ti * (ti + 1) / 2);
  const bool write = !(P.live && !P.live[id]);
  double v[4];
  if (write) assemble_quad(P, lm_radius, ti, tj, threadIdx.x >> 5, 8, threadIdx.x & 31, v);  // loads only
  if (lm_over_chain(term)) return;
  if (P.y && blockIdx.x == 0)  // the solution vector is accumulated with atomics (k_inv_y): start from zero
    for (int e = threadIdx.x; e < P.n_vec; e += 256) P.y[e] = 0.0;
  assemble_tile(P, ti, tj, write, v);
}

// C(32x32, C-layout accumulators) -= A(32x32) * B(32x32)^T, A/B row-major tiles in global memory.
// Lane l supplies A[16 mi + (l&15)][8 (l>>4) + s] at k-step s: the k index is permuted identically
// for both operands, which leaves the sum unchanged and lets each lane read 64 contiguous bytes.
__device__ __forceinline__ void tile_syrk_sub(const double* __restrict__ At, const double* __restrict__ Bt, int lane,
                                              v4d acc[2][2]) {
  const int row = lane & 15, kg = lane >> 4;
  double a[2][8], b[2][8];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const double2* pa = reinterpret_cast<const double2*>(At + (16 * h + row) * kTile + 8 * kg);
    const double2* pb = reinterpret_cast<const double2*>(Bt + (16 * h + row) * kTile + 8 * kg);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const double2 x = pa[s], y = pb[s];
      a[h][2 * s] = -x.x; a[h][2 * s + 1] = -x.y;
      b[h][2 * s] = y.x;  b[h][2 * s + 1] = y.y;
    }
  }
#pragma unroll
  for (int s = 0; s < 8; ++s)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi][s], b[ni][s], acc[mi][ni], 0, 0, 0);
}

// C-layout element (mi, ni, reg r) of lane l sits at row 16 mi + (l>>4) + 4 r, col 16 ni + (l&15)
__device__ __forceinline__ void tile_load_acc(const double* __restrict__ T, int lane, v4d acc[2][2]) {
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        acc[mi][ni][r] = T[(16 * mi + (lane >> 4) + 4 * r) * kTile + 16 * ni + (lane & 15)];
}
template <typename Ptr>
__device__ __forceinline__ void tile_store_acc(Ptr T, int ld, int lane, const v4d acc[2][2]) {
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        T[(16 * mi + (lane >> 4) + 4 * r) * ld + 16 * ni + (lane & 15)] = acc[mi][ni][r];
}

// ---- trailing update of an outer panel: 64x64 output block per workgroup ---------------------------
// C(ti, tk) -= sum_{c = c0..j} L(ti, c) L(tk, c)^T for the tiles right of the panel.  One wave per 32x32 output
// tile of a 2x2 tile block; the four operand tiles of a panel column (two row tiles, two column tiles) are
// staged in LDS once per workgroup and double-buffered against the MFMAs, so every operand byte fetched from
// L2 feeds 8 flops instead of 2.7 (the per-tile kernel is L2-bandwidth-bound at ~25 % of the MFMA peak).
constexpr int kLdsLd = 34;  // LDS row stride of a staged tile (doubles): 16-byte aligned rows, banks spread
template <int LD>
__device__ __forceinline__ void tile_syrk_sub_lds(const double* At, const double* Bt, int lane, v4d acc[2][2]) {
  const int row = lane & 15, kg = lane >> 4;
  double a[2][8], b[2][8];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const double2* pa = reinterpret_cast<const double2*>(At + (16 * h + row) * LD + 8 * kg);
    const double2* pb = reinterpret_cast<const double2*>(Bt + (16 * h + row) * LD + 8 * kg);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const double2 x = pa[s], y = pb[s];
      a[h][2 * s] = -x.x; a[h][2 * s + 1] = -x.y;
      b[h][2 * s] = y.x;  b[h][2 * s + 1] = y.y;
    }
  }
#pragma unroll
  for (int s = 0; s < 8; ++s)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi][s], b[ni][s], acc[mi][ni], 0, 0, 0);
}

// Columns [tk0, tk_hi] of the trailing matrix (all rows ti >= tk up to the rhs row nt) receive panel columns c0..j.
__global__ __launch_bounds__(256) void k_big_update(double* A, int nt, int j, int c0, int tk0, int tk_hi) {
  __shared__ __attribute__((aligned(16))) double s_t[2][4][kTile * kLdsLd];
  const int bx = blockIdx.x, by = blockIdx.y;
  if (bx < by) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ti0 = tk0 + 2 * bx, tkb = tk0 + 2 * by;
  const int ti = ti0 + (wave & 1), tk = tkb + (wave >> 1);
  const bool valid = (ti <= nt) && (tk <= tk_hi) && (ti >= tk);
  // staging: thread -> (tile t, 16-byte piece q); 4 tiles x 512 pieces, 8 pieces per thread
  double2 pre[8];
  auto fetch = [&](int c) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = tid + 256 * u, t = idx >> 9, q = idx & 511;
      const int trow = (t < 2) ? ti0 + t : tkb + (t - 2);
      const bool ok = (t < 2) ? (trow <= nt) : (trow <= tk_hi);
      pre[u] = ok ? reinterpret_cast<const double2*>(A + lt_tile(trow, c) * kTileElems)[q] : make_double2(0.0, 0.0);
    }
  };
  auto park = [&](int buf) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = tid + 256 * u, t = idx >> 9, q = idx & 511;
      const int r = q >> 4, c2 = q & 15;  // row, double2 column
      *reinterpret_cast<double2*>(&s_t[buf][t][r * kLdsLd + 2 * c2]) = pre[u];
    }
  };
  v4d acc[2][2];
  double* C = A + lt_tile(valid ? ti : tk0, valid ? tk : tk0) * kTileElems;
  if (valid) tile_load_acc(C, lane, acc);
  fetch(c0);
  park(0);
  __syncthreads();
  for (int c = c0; c <= j; ++c) {
    const int buf = (c - c0) & 1;
    if (c < j) fetch(c + 1);
    if (valid) tile_syrk_sub_lds<kLdsLd>(s_t[buf][wave & 1], s_t[buf][2 + (wave >> 1)], lane, acc);
    if (c < j) park(buf ^ 1);
    __syncthreads();
  }
  if (valid) tile_store_acc(C, kTile, lane, acc);
}

int g_dbg_flags = 0;
thread_local int64_t g_launches[kLfCount] = {};
extern "C" void mpsfm_debug_set(int f) { g_dbg_flags = f; }
// Phase timeline of the factorisation (diagnostics, scripts/dbg_chol_trace.py): when a buffer is registered, the
// workgroup that owns the diagonal tile of every step stores wall_clock64() (100 MHz) at its phase boundaries:
// two rows of 8 stamps per step, the phases in the first, the hand-offs of the four-wave panel in the second.  The pointer is
// kept on the host and travels in the kernels' arguments: a device global would cost every workgroup a load of its own.
static long long* g_chol_trace = nullptr;
extern "C" int mpsfm_debug_set_chol_trace(long long* dev_buf) {
  g_chol_trace = dev_buf;
  return 0;
}
#define MPSFM_STAMP(k) do { if (trace_on && lane == 0) tr[(k)] = wall_clock64(); } while (0)

// Dense outer-panel path (reduced systems without exploitable structure, MPSFM_CHOL_NB): one step of the right-looking
// factorisation, four waves per tile.  j = -1: factor tile column 0 only.
//   trailing tile (tk > j+1):  A[ti][tk] -= L[ti][j] L[tk][j]^T, one quadrant per wave.
//   panel tile (tk == j+1):    every workgroup re-derives the updated diagonal tile; its four waves factor the stacked
//                              [D; X] (panel_section); the workgroup that owns the diagonal tile stores L^-T
//                              (kept for the back substitution).
// c0 is the first tile column whose L is applied to a trailing tile in this
// launch (c0 == j: the plain right-looking step), tk_max the last tile column this launch touches, and
//   kStepNoOwnUpdate  the panel column j+1 has already received column j (first step of an outer panel),
//   kStepBig          no factorisation: every tile (ti, tk), j < tk <= tk_max, gets columns c0..j at once
//                     (one load and one store of the tile for a rank-32*(j-c0+1) update).
constexpr int kStepNoOwnUpdate = 1, kStepBig = 2;
// Inverse propagation (level-scheduled path up to kPlainMaxTiles tile columns, Pinv != NULL).  The back substitution
// y = L^-T z is another chain of dependent tile solves, one launch per level.  Instead the launches also build, in the
// shadow of their latency-bound panel factorisation, the accumulators  P(i,k) = sum_{j=k}^{i-1} L(i,j) X(j,k)  of the
// inverse X = L^-1  (X(k,k) = L(k,k)^-1, X(i,k) = -L(i,i)^-1 P(i,k)), after which
//   y_k = w_k - sum_{i>k} P(i,k)^T w_i,   w_i = L(i,i)^-T z_i
// is two launches.  The launch after column j was factored uses column j of L and L(j,j)^-1, both final:
//   role (j, k), k in the subtree of j (X(j,k) is zero elsewhere):   P(i,k) += L(i,j) X(j,k) for the rows i of struct(j),
//   X(j,k) recomputed from P(j,k) (final: its contributions come from descendants of j, whose roles ran in earlier
//   launches), so no workgroup reads what another one writes in the same launch; two columns of one level have disjoint
//   subtrees, so their roles never write the same accumulator.
#ifndef MPSFM_INV_ROWS
#define MPSFM_INV_ROWS 2
#endif
constexpr int kInvRows = MPSFM_INV_ROWS;  // rows i handled by one inverse-role workgroup (X(j,k) is formed once for all of them)
constexpr int kStepThreads = 256;         // four waves: one 16 x 16 quadrant of a tile each
// irow: the rows of this workgroup, entries from ni_rows on repeat the last one (their loads go nowhere new, their products are skipped)
// term (has_ctl): `term` of the control block, requested by the caller (lm_term_chain) and looked at here behind the first loads
__device__ __forceinline__ void inv_role(const double* A, const double* LinvT, double* Pinv, int nt, int j, const int (&irow)[kInvRows], int ni_rows, int k,
                                         int32_t term, bool has_ctl, double (*s_B)[kTile + 1], double* s_C) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int mi = wave & 1, ni = wave >> 1;
  const int m16 = lane & 15, kg = lane >> 4;
  const double* Li = LinvT + (size_t)j * kTileElems;               // L(j,j)^-T, row-major
  const double* Pjk = Pinv + lt_tile(j, k) * kTileElems;           // only read when k < j
  // accumulators and A operands of every row of this workgroup are requested now: their latency runs under the
  // formation of T.  Lane (m, q) reads L(i,j)[16 mi + m][4 s + kg], s = 0..7.
  v4d acc[kInvRows];
  double aop[kInvRows][8];
#pragma unroll
  for (int r = 0; r < kInvRows; ++r) {
    const int i = irow[r];
    quad_load(Pinv + lt_tile(i, k) * kTileElems, kTile, lane, mi, ni, acc[r]);
    const double* arow = A + lt_tile(i, j) * kTileElems + (16 * mi + m16) * kTile + kg;
#pragma unroll
    for (int s = 0; s < 8; ++s) aop[r][s] = arow[4 * s];
  }
  if (has_ctl && lm_over_chain(term)) return;
  for (int e = tid; e < kTileElems; e += kStepThreads) {
    const int r = e >> 5, c = e & 31;
    s_B[r][c] = Li[e];
    s_C[e] = (k < j) ? Pjk[e] : 0.0;
  }
  __syncthreads();
  // T = X(j,k): k < j: -(L(j,j)^-1 P(j,k)),  T[m][n] = -sum_q LinvT[q][m] Pjk[q][n];  k == j: L(j,j)^-1, T[m][n] = LinvT[n][m]
  v4d t = {0, 0, 0, 0};
  if (k < j) {
#pragma unroll
    for (int s = 0; s < 8; ++s)
      t = __builtin_amdgcn_mfma_f64_16x16x4f64(-s_B[4 * s + kg][16 * mi + m16], s_C[(4 * s + kg) * kTile + 16 * ni + m16], t, 0, 0, 0);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) t[r] = s_B[16 * ni + m16][16 * mi + kg + 4 * r];
  }
  __syncthreads();  // T overwrites L(j,j)^-T in LDS once every wave has consumed it
  quad_store(&s_B[0][0], kTile + 1, lane, mi, ni, t);
  __syncthreads();
  // P(i,k) += L(i,j) T for the rows of this workgroup; the B operand (T) stays in registers
  double bT[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) bT[s] = s_B[4 * s + kg][16 * ni + m16];
#pragma unroll
  for (int r = 0; r < kInvRows; ++r) {
    if (r >= ni_rows) break;
#pragma unroll
    for (int s = 0; s < 8; ++s) acc[r] = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[r][s], bT[s], acc[r], 0, 0, 0);
    quad_store(Pinv + lt_tile(irow[r], k) * kTileElems, kTile, lane, mi, ni, acc[r]);
  }
}

// ---- the panel section of k_chol_step and k_chol_level, from the barrier behind s_T / s_X to the store -----------------------
// Factors the stacked [D; X] (D in s_T, X in s_X) and stores the rows of X L^-T to x_dst (32 x 32, row-major); d_dst (the
// probe only) receives the rows of L.  waves == kWgWaves: all four waves (stacked_panel_wg); otherwise wave 0 alone
// (stacked_panel) and the others leave.  Every argument is workgroup-uniform and all four waves of the workgroup call this.
// s_P: kPanelLds doubles.  fail (may be NULL) is raised when a wave met a pivot that is not positive; tr (may be NULL)
// receives the phase stamps 2 (entry), 3 (factored: by the wave that finishes last) and 4 (stored); the four-wave path also
// stamps its hand-offs into the step's second row (tr[8 ..], see stacked_panel_wg).
constexpr int kPanelLds = kWgLds > kTileElems ? kWgLds : kTileElems;  // inv_role stages a tile in the same buffer
__device__ __forceinline__ void panel_section(int waves, const double (*s_T)[kTile + 1], const double (*s_X)[kTile + 1], double* s_P, bool skip,
                                              double* x_dst, double* d_dst, int* fail, long long* tr) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row = lane & 31;
  const double* sp = (lane < kTile) ? &s_T[row][0] : &s_X[row][0];
  double* dst = (lane < kTile) ? (d_dst ? d_dst + row * kTile : nullptr) : x_dst + row * kTile;
  if (tr && wave == 0 && lane == 0) tr[2] = wall_clock64();
  bool ok = true;
  if (waves == kWgWaves) {
    double a[kSP];
#pragma unroll
    for (int c = 0; c < kSP; ++c) a[c] = sp[kSP * wave + c];
    if (!skip) stacked_panel_wg(a, lane, wave, s_P, ok, tr ? tr + 8 : nullptr);
    const bool last = wave == kWgWaves - 1;
    if (tr && last && lane == 0) tr[3] = wall_clock64();
    if (fail && !ok && lane == 0) atomicExch(fail, 1);
    if (dst) {
      double2* d2 = reinterpret_cast<double2*>(dst + kSP * wave);
#pragma unroll
      for (int c = 0; c < kSP; c += 2) d2[c >> 1] = make_double2(a[c], a[c + 1]);
    }
    if (tr && last && lane == 0) tr[4] = wall_clock64();
    return;
  }
  if (wave != 0) return;
  // stacked factorisation by wave 0: lanes 0..31 rows of D, lanes 32..63 rows of X (identity for the diagonal workgroup)
  double a[kTile];
#pragma unroll
  for (int c = 0; c < kTile; ++c) a[c] = sp[c];
  if (!skip) stacked_panel<0>(a, lane, s_P, ok);
  if (tr && lane == 0) tr[3] = wall_clock64();
  if (fail && !ok && lane == 0) atomicExch(fail, 1);
  if (dst) {
    double2* d2 = reinterpret_cast<double2*>(dst);
#pragma unroll
    for (int c = 0; c < kTile; c += 2) d2[c >> 1] = make_double2(a[c], a[c + 1]);
  }
  if (tr && lane == 0) tr[4] = wall_clock64();
}

__global__ __launch_bounds__(kStepThreads) void k_chol_step(double* A, double* LinvT, int nt, int j, int* fail, int dbg, int c0, int tk_max,
                                                            int mode, int panel_waves, long long* trace) {
  __shared__ double s_T[kTile][kTile + 1];
  __shared__ double s_X[kTile][kTile + 1];
  __shared__ __attribute__((aligned(16))) double s_Lt[kPanelLds];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int mi = wave & 1, ni = wave >> 1;  // this wave's quadrant
  if (dbg & 16) return;  // ablation: the launch chain alone
  const int tk = j + 1 + blockIdx.y, ti = j + 1 + blockIdx.x;
  if (ti < tk || tk >= nt || ti > nt || tk > tk_max) return;
  double* C = A + lt_tile(ti, tk) * kTileElems;
  if (tk != j + 1 || (mode & kStepBig)) {
    // trailing tile: A[ti][tk] -= sum_c L[ti][c] L[tk][c]^T, one quadrant per wave
    v4d acc;
    quad_load(C, kTile, lane, mi, ni, acc);
    if (!(dbg & 4))
      for (int c = c0; c <= j; ++c) {
        double a[8], b[8];
        quad_operand(A + lt_tile(ti, c) * kTileElems, lane, mi, a);
        quad_operand(A + lt_tile(tk, c) * kTileElems, lane, ni, b);
        quad_gemm_sub(a, b, acc);
      }
    quad_store(C, kTile, lane, mi, ni, acc);
    return;
  }
  const bool own_update = (j >= 0) && !(mode & kStepNoOwnUpdate) && !(dbg & 4);
  // ---- panel column j+1 -------------------------------------------------------------------
  const bool diag = (ti == tk);
  long long* tr = trace ? trace + ((size_t)(j + 1) * 2) * 8 : nullptr;
  const bool trace_on = diag && tr != nullptr && wave == 0;
  MPSFM_STAMP(0);
  {
    // every wave: its quadrant of the updated diagonal tile -> s_T and of the workgroup's own updated tile -> s_X
    v4d dacc, xacc;
    quad_load(A + lt_tile(tk, tk) * kTileElems, kTile, lane, mi, ni, dacc);
    if (!diag) quad_load(C, kTile, lane, mi, ni, xacc);
    if (own_update) {
      const double* Lk = A + lt_tile(tk, j) * kTileElems;
      double am[8], bn[8];
      quad_operand(Lk, lane, mi, am);
      quad_operand(Lk, lane, ni, bn);
      quad_gemm_sub(am, bn, dacc);
      if (!diag) {
        quad_operand(A + lt_tile(ti, j) * kTileElems, lane, mi, am);
        quad_gemm_sub(am, bn, xacc);
      }
    }
    quad_store(&s_T[0][0], kTile + 1, lane, mi, ni, dacc);
    if (diag) {  // identity: x L^-T = row of L^-T
#pragma unroll
      for (int r = 0; r < 4; ++r) xacc[r] = (16 * mi + (lane >> 4) + 4 * r == 16 * ni + (lane & 15)) ? 1.0 : 0.0;
    }
    quad_store(&s_X[0][0], kTile + 1, lane, mi, ni, xacc);
  }
  MPSFM_STAMP(1);
  __syncthreads();
  // The factored diagonal tile is NOT written back over A(tk,tk): every workgroup of this panel column loads
  // A(tk,tk) at its start, and one that is scheduled late (a busy GPU) would otherwise find L there instead of the
  // matrix.  Nothing reads L(tk,tk) from memory afterwards — the back substitution uses the stored L^-T of the
  // diagonal tiles.
  panel_section(panel_waves, s_T, s_X, s_Lt, (dbg & 1) != 0, diag ? LinvT + (size_t)tk * kTileElems : C, nullptr, diag ? fail : nullptr,
                diag ? tr : nullptr);
}


// ---- level-scheduled factorisation (chol_plan.h): one launch per level of the tile elimination tree --------------------
// The same three kinds of workgroup as a right-looking step (k_chol_step with kStepEnv), driven by an item table:
//   panel (ti, c)   the tile's column c is at this launch's level.  The updated diagonal tile D(c) and the own tile receive
//                   the children of c that were factored in the previous launch (sources; the rest of the subtree came
//                   through trailing items of earlier launches), then the four waves factor the stacked [D(c); X];
//   trail (ti, tk)  C -= sum over the source columns (all of the previous level that reach the tile: one workgroup per
//                   tile, so independent chains never race on an ancestor's tile and the sum has a fixed order);
//   role  (j, k)    inverse propagation for column j of the previous level and a column k of its subtree.
struct LevelArgs {
  double* A; double* LinvT; double* Pinv;
  const CholItem* items; const int32_t* srcs; const int32_t* rows;
  const LevelHead* heads;  // launch records of this launch's items (chol_plan.h)
  int* fail; int32_t nt, dbg;
  const LmCtl* ctl;
  long long* trace;     // phase timeline (mpsfm_debug_set_chol_trace), NULL: off
  int32_t panel_waves;  // waves that factor a panel: kWgWaves or 1 (MPSFM_CHOL_PANEL_WAVES)
  DampArgs damp;        // direct form of the front (DirectAsm), first launch only (k_chol_level<., true>)
  int32_t nitems;       // ... whose workgroups beyond the items damp the diagonal tiles of the later columns
};

// The damping of the direct form (DampArgs; the first level launch, k_chol_level<., true>): A comes undamped from the slab reduction.
//   A panel item of that launch adds clamp(diag U, min, max) / radius to the diagonal of the tile it factors in front of the tile's way
// to LDS (a padding column: 1.0, its row of A is zero).  A quadrant on the diagonal (mi == ni) keeps element (q, q) in the lane with
// (lane & 15) == (lane >> 4) + 4 r, register r.  Three independent loads per lane — diag U by column, the column's slot, the radius —
// without a branch in front of them, so they travel with the tile requests.
//   The workgroups behind the items do the same in memory for the columns of all later launches, one thread per column (damp_columns):
// nothing else reads or writes those diagonal tiles in the first launch, which has no trailing items.
struct DampReq { double du, radius; int32_t cs; };
__device__ __forceinline__ void damp_request(const DampArgs& P, const LmCtl* ctl, int g, DampReq& q) {
  q.du = P.diag_col[g];
  const int32_t cs = *(P.col_slot ? P.col_slot + min(g, P.n - 1) : reinterpret_cast<const int32_t*>(P.diag_col));
  q.radius = lm_radius_chain(ctl, P.diag_col, P.radius);
  q.cs = g >= P.n ? -1 : (P.col_slot ? cs : 0);
}
__device__ __forceinline__ double damp_value(const DampArgs& P, const DampReq& q, double d) {
  return q.cs < 0 ? 1.0 : d + fmin(fmax(q.du, P.min_diag), P.max_diag) / q.radius;
}
__device__ __forceinline__ void damp_apply(const DampArgs& P, const DampReq& q, int mi, int ni, int lane, v4d& dacc) {
  if (mi != ni || ((lane & 15) & 3) != (lane >> 4)) return;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (r == ((lane & 15) >> 2)) dacc[r] = damp_value(P, q, dacc[r]);
}
__device__ __forceinline__ void damp_columns(const DampArgs& P, const LmCtl* ctl, double* A, int nt, int g) {
  const int32_t term = lm_term_chain(ctl, P.diag_col);
  const bool mine = g < nt * kTile;
  const int gc = mine ? g : 0, tk = gc >> 5, c = gc & 31;
  const uint8_t in_panel = P.level0[tk];
  double* d = A + lt_tile(tk, tk) * kTileElems + c * kTile + c;
  const double v = *d;
  DampReq q;
  damp_request(P, ctl, gc, q);
  if (ctl != nullptr && lm_over_chain(term)) return;
  if (mine && !in_panel) *d = damp_value(P, q, v);
}

// The entry of a level launch.  Every workgroup is a chain of latencies before its first tile is on its way, and the launch ends
// with its slowest workgroup.  Behind the kernel arguments the entry makes one trip for the item's launch record (64 bytes, one
// scalar load: item, sources, rows; a table every launch reads: it hits in L2) and one for the tiles; `term`, which comes from
// memory (lm_term_chain), is requested first and looked at behind the tile requests, and the trace pointer is an argument.  With
// the sources in registers the first sources (a panel item's through LDS, below; a trailing item's as operands) are requested together
// with the tiles they update, and every further source while the products of the one before run.  The products themselves keep their
// order (ascending source, same k-steps),
// so the factor is bit for bit what the list-walking entry (kList: item -> srcs / rows -> operands, MPSFM_CHOL_ENTRY=list) gives.
typedef int32_t v16i __attribute__((ext_vector_type(16)));
static_assert(kInvRows <= kHeadRows, "a role's rows must fit its launch record");
constexpr int kHeadSrc0 = 2, kHeadRow0 = kHeadSrc0 + kInlineSrc, kHeadOver = kHeadRow0 + kHeadRows;  // words of a LevelHead
constexpr int kPanelBatch = 2;  // sources of a panel item staged and requested in front of the first wait (C3: panels have at most two)
constexpr int kTrailBatch = 4;  // the same for a trailing item (C3: at most three, C4 / C5: four)

// source q of an item: from the record, beyond kInlineSrc from the list (a dependent load, no scene of the benchmark gets there)
__device__ __forceinline__ int head_src(const v16i& w, const int32_t* srcs, int q) {
  if (q >= kInlineSrc) return srcs[(uint32_t)w[kHeadOver] + (uint32_t)(q - kInlineSrc)];
  int e = w[kHeadSrc0];
#pragma unroll
  for (int r = 1; r < kInlineSrc; ++r) e = (q == r) ? w[kHeadSrc0 + r] : e;
  return e;
}
struct PanelOps { double am[8], bn[8], ax[8]; };
struct TrailOps { double a[8], b[8]; };
// operands of source e for the panel item (ti, tk): L(tk, c) for both quadrant operands, L(ti, c) where the source reaches the own tile
__device__ __forceinline__ void panel_request(const double* A, int ti, int tk, int e, bool diag, int lane, int mi, int ni, PanelOps& o) {
  const int c = e & 0xffff;
  const double* Lk = A + lt_tile(tk, c) * kTileElems;
  quad_operand(Lk, lane, mi, o.am);
  quad_operand(Lk, lane, ni, o.bn);
  if (!diag && (e & kSrcX)) quad_operand(A + lt_tile(ti, c) * kTileElems, lane, mi, o.ax);
}
__device__ __forceinline__ void panel_apply(const PanelOps& o, int e, bool diag, v4d& dacc, v4d& xacc) {
  quad_gemm_sub(o.am, o.bn, dacc);
  if (!diag && (e & kSrcX)) quad_gemm_sub(o.ax, o.bn, xacc);
}
__device__ __forceinline__ void trail_request(const double* A, int ti, int tk, int c, int lane, int mi, int ni, TrailOps& o) {
  quad_operand(A + lt_tile(ti, c) * kTileElems, lane, mi, o.a);
  quad_operand(A + lt_tile(tk, c) * kTileElems, lane, ni, o.b);
}

// The source tiles of a panel item go through LDS.  Read straight into the operand layout (quad_operand: lane l takes 64 bytes of
// row l & 15) the sixteen lanes of a quarter wave sit in sixteen different cache lines, a wave touches 64 lines per load
// instruction, and the workgroup's 48 instructions per source tile pair keep the CU's one tag lookup per cycle busy for ~1.3 us:
// that, not a chain of dependent loads, is what a source costs (launches 6 and 9 of C3, the two with two-source panels, stood
// out by 1.4 us before and after the sources moved into the launch record).  Staged, the workgroup fetches a tile as 512
// consecutive 16-byte pieces, two per thread (8 lines per instruction), parks them with the row stride of k_big_update's staging
// and reads the operands back in the same layout: the values and the order of the products are unchanged.
constexpr int kStageTile = kTile * kLdsLd;  // doubles of a staged tile
static_assert(kPanelLds >= 2 * kStageTile, "the first source of a panel item is staged in the panel's LDS buffer");
__device__ __forceinline__ void stage_fetch(const double* __restrict__ T, double2& p0, double2& p1) {
  p0 = reinterpret_cast<const double2*>(T)[threadIdx.x];
  p1 = reinterpret_cast<const double2*>(T)[threadIdx.x + kStepThreads];
}
__device__ __forceinline__ void stage_park(const double2& p0, const double2& p1, double* S) {
  const int r = threadIdx.x >> 4, c2 = threadIdx.x & 15;  // row, 16-byte piece of the row; the second piece sits 16 rows below
  *reinterpret_cast<double2*>(S + r * kLdsLd + 2 * c2) = p0;
  *reinterpret_cast<double2*>(S + (r + 16) * kLdsLd + 2 * c2) = p1;
}
// quad_operand on a staged tile
__device__ __forceinline__ void quad_operand_lds(const double* S, int lane, int b, double (&o)[8]) {
  const double2* p = reinterpret_cast<const double2*>(S + (16 * b + (lane & 15)) * kLdsLd + 8 * (lane >> 4));
#pragma unroll
  for (int s = 0; s < 4; ++s) { const double2 x = p[s]; o[2 * s] = x.x; o[2 * s + 1] = x.y; }
}

template <bool kList, bool kDamp>
__global__ __launch_bounds__(kStepThreads) void k_chol_level(LevelArgs G) {
  __shared__ double s_T[kTile][kTile + 1];
  __shared__ double s_X[kTile][kTile + 1];
  __shared__ __attribute__((aligned(16))) double s_Lt[kPanelLds];
  __shared__ __attribute__((aligned(16))) double s_S1[kList ? 2 : 2 * kStageTile];  // staging of a panel item's second source
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int mi = wave & 1, ni = wave >> 1;  // this wave's quadrant
  double* A = G.A;
  if constexpr (kDamp) {
    if ((int)blockIdx.x >= G.nitems) {  // (workgroup-uniform)
      damp_columns(G.damp, G.ctl, A, G.nt, ((int)blockIdx.x - G.nitems) * kStepThreads + (int)threadIdx.x);
      return;
    }
  }
  int type, ti, tk, nsrc;
  int32_t term = kLmRunning;
  const bool has_ctl = !kList && G.ctl != nullptr;  // `term` holds the control block's word
  v16i w = {};
  const int32_t* src = nullptr;
  if constexpr (kList) {
    if (lm_over(G.ctl)) return;
    if (G.dbg & 16) return;  // ablation: the launch chain alone
    const CholItem it = G.items[blockIdx.x];
    type = it.type; ti = it.ti; tk = it.tk; nsrc = it.nsrc;
    src = G.srcs + it.src;
    if (type == kItemRole) {
      if (G.dbg & 8) return;
      int irow[kInvRows];
#pragma unroll
      for (int r = 0; r < kInvRows; ++r) irow[r] = G.rows[it.aux + min(r, nsrc - 1)];
      inv_role(A, G.LinvT, G.Pinv, G.nt, ti, irow, nsrc, tk, kLmRunning, false, s_T, s_Lt);
      return;
    }
  } else {
    // `term` is requested here and looked at behind the operand requests, in front of the first store
    term = lm_term_chain(G.ctl, G.heads);
    w = load_const(reinterpret_cast<const v16i*>(G.heads + blockIdx.x));
    type = w[0] & 0xffff; ti = (uint32_t)w[0] >> 16; tk = w[1] & 0xffff; nsrc = (uint32_t)w[1] >> 16;
    if (G.dbg & 16) return;
    if ((G.dbg & 4) && type != kItemRole) nsrc = 0;  // ablation: no updates (one place for the tile loads: a second one costs waits)
    if (type == kItemRole) {
      if (G.dbg & 8) return;
      int irow[kInvRows];
      irow[0] = w[kHeadRow0];
#pragma unroll
      for (int r = 1; r < kInvRows; ++r) irow[r] = r < nsrc ? w[kHeadRow0 + r] : irow[r - 1];
      inv_role(A, G.LinvT, G.Pinv, G.nt, ti, irow, nsrc, tk, term, has_ctl, s_T, s_Lt);
      return;
    }
  }
  double* C = A + lt_tile(ti, tk) * kTileElems;
  if (type == kItemTrail) {
    v4d acc;
    if constexpr (kList) quad_load(C, kTile, lane, mi, ni, acc);
    if (kList ? !(G.dbg & 4) : true) {
      if constexpr (kList) {
        for (int q = 0; q < nsrc; ++q) {
          const int c = src[q];
          double a[8], b[8];
          quad_operand(A + lt_tile(ti, c) * kTileElems, lane, mi, a);
          quad_operand(A + lt_tile(tk, c) * kTileElems, lane, ni, b);
          quad_gemm_sub(a, b, acc);
        }
      } else {
        TrailOps o[kTrailBatch], cur;
#pragma unroll
        for (int q = 0; q < kTrailBatch; ++q)
          if (q < nsrc) trail_request(A, ti, tk, w[kHeadSrc0 + q], lane, mi, ni, o[q]);
        if (nsrc > kTrailBatch) trail_request(A, ti, tk, head_src(w, G.srcs, kTrailBatch), lane, mi, ni, cur);
        quad_load(C, kTile, lane, mi, ni, acc);  // behind the operands: the compiler waits for an accumulator where it is loaded
#pragma unroll
        for (int q = 0; q < kTrailBatch; ++q)
          if (q < nsrc) quad_gemm_sub(o[q].a, o[q].b, acc);
        for (int q = kTrailBatch; q < nsrc; ++q) {  // source q + 1 is on its way while the products of q run
          TrailOps nxt;
          const bool more = q + 1 < nsrc;
          if (more) trail_request(A, ti, tk, head_src(w, G.srcs, q + 1), lane, mi, ni, nxt);
          quad_gemm_sub(cur.a, cur.b, acc);
          if (more) cur = nxt;
        }
      }
    }
    if (has_ctl && lm_over_chain(term)) return;
    quad_store(C, kTile, lane, mi, ni, acc);
    return;
  }
  // ---- panel tile of column tk ---------------------------------------------------------------
  const bool diag = (ti == tk);
  long long* tr = G.trace ? G.trace + ((size_t)tk * 2) * 8 : nullptr;
  const bool trace_on = diag && tr != nullptr && wave == 0;
  MPSFM_STAMP(0);
  {
    v4d dacc, xacc;
    const double* D = A + lt_tile(tk, tk) * kTileElems;
    [[maybe_unused]] DampReq dq;
    if constexpr (kDamp) damp_request(G.damp, G.ctl, tk * kTile + 16 * ni + (lane & 15), dq);
    if constexpr (kList) {
      quad_load(D, kTile, lane, mi, ni, dacc);
      if (!diag) quad_load(C, kTile, lane, mi, ni, xacc);
    }
    if (kList ? !(G.dbg & 4) : true) {
      if constexpr (kList) {
        for (int q = 0; q < nsrc; ++q) {
          const int e = src[q], c = e & 0xffff;
          const double* Lk = A + lt_tile(tk, c) * kTileElems;
          double am[8], bn[8];
          quad_operand(Lk, lane, mi, am);
          quad_operand(Lk, lane, ni, bn);
          quad_gemm_sub(am, bn, dacc);
          if (!diag && (e & kSrcX)) {
            quad_operand(A + lt_tile(ti, c) * kTileElems, lane, mi, am);
            quad_gemm_sub(am, bn, xacc);
          }
        }
      } else {
        // the first two sources through LDS (above), requested with D and X in front of the first wait
        static_assert(kPanelBatch == 2, "two staged sources, written out (an indexed array of pieces ends up in scratch)");
        const int e0 = w[kHeadSrc0], e1 = w[kHeadSrc0 + 1];
        const bool s0 = nsrc > 0, s1 = nsrc > 1, x0 = s0 && !diag && (e0 & kSrcX), x1 = s1 && !diag && (e1 & kSrcX);
        double2 k0a = {}, k0b = {}, x0a = {}, x0b = {}, k1a = {}, k1b = {}, x1a = {}, x1b = {};
        PanelOps cur;
        int e_cur = 0;
        if (s0) stage_fetch(A + lt_tile(tk, e0 & 0xffff) * kTileElems, k0a, k0b);
        if (x0) stage_fetch(A + lt_tile(ti, e0 & 0xffff) * kTileElems, x0a, x0b);
        if (s1) stage_fetch(A + lt_tile(tk, e1 & 0xffff) * kTileElems, k1a, k1b);
        if (x1) stage_fetch(A + lt_tile(ti, e1 & 0xffff) * kTileElems, x1a, x1b);
        if (nsrc > kPanelBatch) { e_cur = head_src(w, G.srcs, kPanelBatch); panel_request(A, ti, tk, e_cur, diag, lane, mi, ni, cur); }
        quad_load(D, kTile, lane, mi, ni, dacc);
        if (!diag) quad_load(C, kTile, lane, mi, ni, xacc);
        if (has_ctl && lm_over_chain(term)) return;
        if (s0) {
          stage_park(k0a, k0b, s_Lt);
          if (x0) stage_park(x0a, x0b, s_Lt + kStageTile);
          if (s1) stage_park(k1a, k1b, s_S1);
          if (x1) stage_park(x1a, x1b, s_S1 + kStageTile);
          __syncthreads();
          double am[8], bn[8];
          quad_operand_lds(s_Lt, lane, mi, am);
          quad_operand_lds(s_Lt, lane, ni, bn);
          quad_gemm_sub(am, bn, dacc);
          if (x0) {
            quad_operand_lds(s_Lt + kStageTile, lane, mi, am);
            quad_gemm_sub(am, bn, xacc);
          }
          if (s1) {
            quad_operand_lds(s_S1, lane, mi, am);
            quad_operand_lds(s_S1, lane, ni, bn);
            quad_gemm_sub(am, bn, dacc);
            if (x1) {
              quad_operand_lds(s_S1 + kStageTile, lane, mi, am);
              quad_gemm_sub(am, bn, xacc);
            }
          }
        }
        for (int q = kPanelBatch; q < nsrc; ++q) {  // source q + 1 is on its way while the products of q run
          PanelOps nxt;
          const bool more = q + 1 < nsrc;
          const int e_nxt = more ? head_src(w, G.srcs, q + 1) : 0;
          if (more) panel_request(A, ti, tk, e_nxt, diag, lane, mi, ni, nxt);
          panel_apply(cur, e_cur, diag, dacc, xacc);
          if (more) { cur = nxt; e_cur = e_nxt; }
        }
      }
    }
    if constexpr (kDamp) damp_apply(G.damp, dq, mi, ni, lane, dacc);
    quad_store(&s_T[0][0], kTile + 1, lane, mi, ni, dacc);
    if (diag) {  // identity: x L^-T = row of L^-T
#pragma unroll
      for (int r = 0; r < 4; ++r) xacc[r] = (16 * mi + (lane >> 4) + 4 * r == 16 * ni + (lane & 15)) ? 1.0 : 0.0;
    }
    quad_store(&s_X[0][0], kTile + 1, lane, mi, ni, xacc);
  }
  MPSFM_STAMP(1);
  __syncthreads();
  // as in k_chol_step the factored diagonal tile is not written back over A(tk,tk): its column's other workgroups may
  // still be loading it
  panel_section(G.panel_waves, s_T, s_X, s_Lt, (G.dbg & 1) != 0, diag ? G.LinvT + (size_t)tk * kTileElems : C, nullptr, diag ? G.fail : nullptr,
                diag ? tr : nullptr);
}

// ---- probe: one workgroup factors a given stacked [D; X] through panel_section (tests: one wave against four) -----------------
__global__ __launch_bounds__(kStepThreads) void k_panel_probe(const double* dx, int waves, double* out, int* fail) {
  __shared__ double s_T[kTile][kTile + 1];
  __shared__ double s_X[kTile][kTile + 1];
  __shared__ __attribute__((aligned(16))) double s_Lt[kPanelLds];
  for (int e = threadIdx.x; e < kTileElems; e += kStepThreads) {
    s_T[e >> 5][e & 31] = dx[e];
    s_X[e >> 5][e & 31] = dx[kTileElems + e];
  }
  __syncthreads();
  panel_section(waves, s_T, s_X, s_Lt, false, out + kTileElems, out, fail, nullptr);
}
// dx, out: host, 64 x 32 row-major (rows 0..31: D -> L, its upper triangle is not defined; rows 32..63: X -> X L^-T).
// waves: 1 or 4.  *ok: 1 when every pivot was positive and finite.
extern "C" int mpsfm_debug_panel_factor(const double* dx, int waves, double* out, int* ok) {
  if (!dx || !out || !ok || (waves != 1 && waves != kWgWaves)) return MPSFM_EINVAL;
  const size_t bytes = (size_t)2 * kTileElems * sizeof(double);
  DeviceBlocks own;  // the copies below are synchronous: nothing to wait for
  double* d_in = own.alloc<double>((size_t)2 * kTileElems);
  double* d_out = own.alloc<double>((size_t)2 * kTileElems);
  int* d_fail = own.alloc<int>(1);
  hipError_t e = (d_in && d_out && d_fail) ? hipSuccess : hipErrorOutOfMemory;
  int h_fail = 0;
  if (e == hipSuccess) e = hipMemcpy(d_in, dx, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_out, 0, bytes);
  if (e == hipSuccess) e = hipMemset(d_fail, 0, sizeof(int));
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_panel_probe, dim3(1), dim3(kStepThreads), 0, nullptr, d_in, waves, d_out, d_fail);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(&h_fail, d_fail, sizeof(int), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return e == hipErrorOutOfMemory ? MPSFM_ENOMEM : MPSFM_EHIP;
  *ok = h_fail ? 0 : 1;
  return MPSFM_OK;
}

// Backward substitution y = L^-T z by levels, highest first (no inverse accumulators: nt > kPlainMaxTiles).  One workgroup
// per tile column j of the level: v = z_j - sum_{i in struct(j)} L(i,j)^T y_i (all those i are ancestors: final), then
// y_j = L(j,j)^-T v with the stored inverse.  z_j is row 0 of the right-hand-side tile (nt, j).
__global__ __launch_bounds__(256) void k_back_level(const double* A, const double* LinvT, const int32_t* cols, const int32_t* struct_start,
                                                    const int32_t* struct_rows, int nt, int n, double* ybuf, double* y, const int32_t* col_slot, const LmCtl* ctl) {
  __shared__ double s_part[8][kTile];
  __shared__ double s_v[kTile];
  const int32_t term = lm_term_chain(ctl);  // requested with the column's tables, tested in front of the first barrier
  const int j = cols[blockIdx.x];
  const int c = threadIdx.x & 31, part = threadIdx.x >> 5;
  const int r0 = struct_start[j], r1 = struct_start[j + 1] - 1;  // the last entry is the right-hand-side row
  double sacc = 0.0;
  for (int q = r0 + part; q < r1; q += 8) {
    const int i = struct_rows[q];
    const double* Tl = A + lt_tile(i, j) * kTileElems + c;
    const double* yi = ybuf + (size_t)i * kTile;
#pragma unroll 8
    for (int r = 0; r < kTile; ++r) sacc = __builtin_fma(Tl[r * kTile], yi[r], sacc);
  }
  if (lm_over_chain(term)) return;
  s_part[part][c] = sacc;
  __syncthreads();
  if (part == 0) {
    double v = A[lt_tile(nt, j) * kTileElems + c];
#pragma unroll
    for (int q = 0; q < 8; ++q) v -= s_part[q][c];
    s_v[c] = v;
  }
  __syncthreads();
  if (part == 0) {
    const double* Li = LinvT + (size_t)j * kTileElems + c * kTile;
    double yr = 0.0;
#pragma unroll
    for (int q = 0; q < kTile; ++q) yr = __builtin_fma(Li[q], s_v[q], yr);
    ybuf[(size_t)j * kTile + c] = yr;
    const int iy = vec_index(col_slot, j * kTile + c, n);
    if (iy >= 0) y[iy] = yr;
  }
}

// ---- back substitution  y = L^-T z  in groups of kBsG tile rows --------------------------------
// z starts as row 0 of tile row nt (forward substitution came with the factorisation).  Groups are
// processed from the bottom; every workgroup of a launch re-solves the group (its tiles are staged
// in LDS, the diagonal solves are mat-vecs with the stored L^-T tiles), then workgroup w updates the
// slice z_w of one earlier tile column with the group's y.
constexpr int kBsG = 4;

__global__ __launch_bounds__(256) void k_z_init(const double* A, int nt, double* zbuf) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < nt * kTile) zbuf[c] = A[lt_tile(nt, c >> 5) * kTileElems + (c & 31)];
}

__global__ __launch_bounds__(256) void k_backsub_group(const double* A, const double* LinvT, int nt, int n, int t0, int t1,
                                                      double* zbuf, double* y, const int32_t* col_slot) {
  __shared__ double s_tiles[(kBsG + kBsG * (kBsG - 1) / 2) * kTileElems];  // LinvT of the group, then L[tj][c], c<tj in group
  __shared__ double s_z[kBsG * kTile];
  __shared__ double s_y[kBsG * kTile];
  __shared__ double s_part[8 * kTile];
  const int tid = threadIdx.x;
  const int G = t1 - t0;
  // stage tiles
  for (int g = 0; g < G; ++g) {
    const double2* src = reinterpret_cast<const double2*>(LinvT + (size_t)(t0 + g) * kTileElems);
    double2* dst = reinterpret_cast<double2*>(s_tiles + g * kTileElems);
    for (int e = tid; e < kTileElems / 2; e += 256) dst[e] = src[e];
  }
  {
    int slot = kBsG;
    for (int g = 1; g < G; ++g)
      for (int c = 0; c < g; ++c, ++slot) {
        const double2* src = reinterpret_cast<const double2*>(A + lt_tile(t0 + g, t0 + c) * kTileElems);
        double2* dst = reinterpret_cast<double2*>(s_tiles + slot * kTileElems);
        for (int e = tid; e < kTileElems / 2; e += 256) dst[e] = src[e];
      }
  }
  if (tid < G * kTile) s_z[tid] = zbuf[t0 * kTile + tid];
  // prefetch this workgroup's column tiles L[t0+g][w] into registers: thread (part, q) needs rows 4 part .. +3
  const int w = blockIdx.x;
  const bool has_col = (w < t0);
  const int q = tid & 31, part = tid >> 5;
  double lc[kBsG][4];
  if (has_col) {
#pragma unroll
    for (int g = 0; g < kBsG; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        lc[g][r] = (g < G) ? A[lt_tile(t0 + g, w) * kTileElems + (4 * part + r) * kTile + q] : 0.0;
  }
  __syncthreads();
  // solve the group bottom-up
  for (int g = G - 1; g >= 0; --g) {
    // y_g = LinvT_g z_g : thread (part, q): partial over columns 4 part .. +3 of row q
    {
      const double* T = s_tiles + g * kTileElems + q * kTile + 4 * part;
      const double* z = s_z + g * kTile + 4 * part;
      s_part[part * kTile + q] = T[0] * z[0] + T[1] * z[1] + T[2] * z[2] + T[3] * z[3];
    }
    __syncthreads();
    if (tid < kTile) {
      double s = 0.0;
#pragma unroll
      for (int p = 0; p < 8; ++p) s += s_part[p * kTile + tid];
      s_y[g * kTile + tid] = s;
    }
    __syncthreads();
    // z_c -= L[g][c]^T y_g for c < g inside the group
    for (int idx = tid; idx < g * kTile; idx += 256) {
      const int c = idx >> 5, qq = idx & 31;
      const int slot = kBsG + g * (g - 1) / 2 + c;
      const double* Lt = s_tiles + slot * kTileElems;
      double s = 0.0;
#pragma unroll 8
      for (int r = 0; r < kTile; ++r) s += Lt[r * kTile + qq] * s_y[g * kTile + r];
      s_z[c * kTile + qq] -= s;
    }
    __syncthreads();
  }
  // update the slice of an earlier tile column
  if (has_col) {
    double s = 0.0;
#pragma unroll
    for (int g = 0; g < kBsG; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r) s += (g < G) ? lc[g][r] * s_y[g * kTile + 4 * part + r] : 0.0;
    s_part[part * kTile + q] = s;
  }
  __syncthreads();
  if (has_col && tid < kTile) {
    double s = 0.0;
#pragma unroll
    for (int p = 0; p < 8; ++p) s += s_part[p * kTile + tid];
    zbuf[w * kTile + tid] -= s;
  }
  if (w == 0 && tid < G * kTile) {
    const int gidx = t0 * kTile + tid;
    const int iy = vec_index(col_slot, gidx, n);
    if (iy >= 0) y[iy] = s_y[tid];
  }
}

// ---- y = L^-T z from the inverse accumulators (one launch) ----------------------------------------------
// y_k = w_k - sum_{i>k} P(i,k)^T w_i,  w_i = L(i,i)^-T z_i,  z_i = row 0 of the right-hand-side tile (nt, i).  The long columns
// are cut into kInvSplit workgroups (i = k+1+s mod kInvSplit); every workgroup first forms the w_i it needs itself (a
// 32 x 32 product each — cheaper than a launch of its own for them), split 0 also w_k.  y starts from zero (k_assemble).
constexpr int kInvSplit = 4;
constexpr int kInvPre = 8;  // accumulator tiles of a workgroup requested in front of its barrier (C3: at most 10 per workgroup)
__global__ __launch_bounds__(256) void k_inv_y(const double* A, const double* LinvT, const double* Pinv, int nt, int n, double* y,
                                               const int32_t* col_slot, const LmCtl* ctl) {
  __shared__ double s_w[(kPlainMaxTiles / kInvSplit + 2) * kTile];
  __shared__ double s_part[8][kTile];
  const int32_t term = lm_term_chain(ctl);  // requested with the first operands, tested in front of the first barrier
  const int k = blockIdx.x, sp = blockIdx.y, c = threadIdx.x & 31, part = threadIdx.x >> 5;
  const int first = k + 1 + sp;
  const int m = first < nt ? (nt - first + kInvSplit - 1) / kInvSplit : 0;  // tiles i = first + kInvSplit j
  const int own = sp == 0 ? 1 : 0;                                          // slot 0: w_k
  if (m + own == 0) return;
  for (int idx = threadIdx.x; idx < (m + own) * kTile; idx += 256) {
    const int slot = idx >> 5, r = idx & 31;
    const int i = (own && slot == 0) ? k : first + kInvSplit * (slot - own);
    const double* z = A + lt_tile(nt, i) * kTileElems;
    const double* Li = LinvT + (size_t)i * kTileElems + r * kTile;
    double sacc = 0.0;
#pragma unroll 8
    for (int q = 0; q < kTile; ++q) sacc = __builtin_fma(Li[q], z[q], sacc);
    s_w[idx] = sacc;
  }
  // the accumulators of the first kInvPre tiles do not depend on s_w: requested in front of the barrier that publishes it
  double pv[kInvPre][4];
#pragma unroll
  for (int j = 0; j < kInvPre; ++j)
    if (j < m) {
      const double* Pt = Pinv + lt_tile(first + kInvSplit * j, k) * kTileElems;
#pragma unroll
      for (int r = 0; r < 4; ++r) pv[j][r] = Pt[(4 * part + r) * kTile + c];
    }
  if (lm_over_chain(term)) return;
  __syncthreads();
  double sacc = 0.0;
#pragma unroll
  for (int j = 0; j < kInvPre; ++j)
    if (j < m) {
      const double* w = s_w + (j + own) * kTile;
#pragma unroll
      for (int r = 0; r < 4; ++r) sacc += pv[j][r] * w[4 * part + r];
    }
  for (int j = kInvPre; j < m; ++j) {
    const double* Pt = Pinv + lt_tile(first + kInvSplit * j, k) * kTileElems;
    const double* w = s_w + (j + own) * kTile;
#pragma unroll
    for (int r = 4 * part; r < 4 * part + 4; ++r) sacc += Pt[r * kTile + c] * w[r];
  }
  s_part[part][c] = sacc;
  __syncthreads();
  if (part == 0) {
    double v = 0.0;
#pragma unroll
    for (int q = 0; q < 8; ++q) v += s_part[q][c];
    const int g = k * kTile + c;
    const int iy = vec_index(col_slot, g, n);
    if (iy >= 0) atomicAdd(&y[iy], (own ? s_w[c] : 0.0) - v);
  }
}

// ---- host wrappers -----------------------------------------------------------------------------------
void launch_assemble(const AssembleArgs& a, hipStream_t s) {
  const int64_t ntiles = a.tile_list ? (int64_t)a.n_list : (int64_t)(a.nt + 1) * (a.nt + 2) / 2;
  count_launch(kLfAssemble);
  hipLaunchKernelGGL(k_assemble, dim3((unsigned)ntiles), dim3(256), 0, s, a);
}

// factor + forward substitution (steps -1 .. nt-2) and back substitution.
// work: nt*1024 doubles for L^-T of the diagonal tiles followed by nt*32 doubles for z.
static void launch_big(double* A, int nt, int j, int c0, int tk_lo, int tk_hi, hipStream_t s) {
  if (tk_hi < tk_lo) return;
  const int rows = nt - tk_lo + 1, cols = tk_hi - tk_lo + 1;
  hipLaunchKernelGGL(k_big_update, dim3((rows + 1) / 2, (cols + 1) / 2), dim3(256), 0, s, A, nt, j, c0, tk_lo, tk_hi);
}

// layout of the work buffer: L^-T of the diagonal tiles | z | w | one spare tile row | inverse accumulators (per-step path, nt <= 64)
size_t dense_work_doubles(int nt) {
  const size_t t = (size_t)(nt > 0 ? nt : 1);
  size_t n = t * kTileElems + 2 * t * kTile + (t + 1) * kTileElems;
  if (nt <= kPlainMaxTiles) n += (t * (t + 1) / 2) * kTileElems;
  return n;
}
int dense_plain_max_tiles() { return kPlainMaxTiles; }
int dense_inv_rows() { return kInvRows; }
bool dense_level(const DenseOverlap* ov, const LevelPlanDev* lp) { return lp && lp->valid && !(ov && (ov->nb > 0 || ov->no_level)); }
static int dense_panel_width(int nt, const DenseOverlap* ov) {
  return (ov && ov->nb > 0) ? ov->nb : ((nt <= kPlainMaxTiles) ? nt : 8);
}
// the accumulators of the inverse propagation, or NULL when this solve does not use them (outer panels, switched off)
double* dense_pinv(double* work, int nt, const DenseOverlap* ov, const LevelPlanDev* lp) {
  if (nt <= 0 || nt > kPlainMaxTiles || (ov && (ov->no_inverse || ov->nb > 0))) return nullptr;
  if (dense_level(ov, lp) && !lp->use_pinv) return nullptr;
  return work + (size_t)nt * kTileElems + 2 * (size_t)nt * kTile + ((size_t)nt + 1) * kTileElems;
}

// ov (may be NULL): a second stream and events.  With it the update of an outer panel is split: the tile
// columns of the NEXT panel are updated on the main stream (the factorisation needs them next), the columns
// beyond run on the second stream under the next panel's factorisation steps.
void launch_dense_solve(double* A, double* work, int nt, int n, double* y, int* fail, hipStream_t s, DenseOverlap* ov, const LevelPlanDev* lp,
                        const LmCtl* ctl, const DampArgs* damp) {
  if (nt <= 0) return;
  double* LinvT = work;
  double* zbuf = work + (size_t)nt * kTileElems;
  const int panel_waves = (ov ? ov->panel_waves : kPanelWavesDefault) == 1 ? 1 : kWgWaves;
  if (dense_level(ov, lp)) {
    double* Pinv = dense_pinv(work, nt, ov, lp);
    LevelArgs G{A, LinvT, Pinv, nullptr, lp->d_srcs, lp->d_rows, nullptr, fail, nt, g_dbg_flags, ctl, g_chol_trace, panel_waves, damp ? *damp : DampArgs{}, 0};
    const bool list = ov && ov->entry_list;
    bool damped = damp == nullptr;  // the first launch damps (the caller has seen LevelPlanDev::damp_in_launch0)
    for (int l = 0; l < lp->nlevels; ++l) {
      const int grid = lp->h_launch_start[l + 1] - lp->h_launch_start[l];
      if (grid <= 0) continue;
      G.items = lp->d_items + lp->h_launch_start[l];
      G.heads = lp->d_heads + lp->h_launch_start[l];
      count_launch(kLfCholLevel);
      if (!damped) {
        G.nitems = grid;
        const unsigned g2 = (unsigned)(grid + (nt * kTile + kStepThreads - 1) / kStepThreads);
        if (list) hipLaunchKernelGGL((k_chol_level<true, true>), dim3(g2), dim3(kStepThreads), 0, s, G);
        else hipLaunchKernelGGL((k_chol_level<false, true>), dim3(g2), dim3(kStepThreads), 0, s, G);
        damped = true;
        continue;
      }
      if (list) hipLaunchKernelGGL((k_chol_level<true, false>), dim3((unsigned)grid), dim3(kStepThreads), 0, s, G);
      else hipLaunchKernelGGL((k_chol_level<false, false>), dim3((unsigned)grid), dim3(kStepThreads), 0, s, G);
    }
    if (Pinv) {
      count_launch(kLfDenseRest);
      hipLaunchKernelGGL(k_inv_y, dim3(nt, kInvSplit), dim3(256), 0, s, A, LinvT, Pinv, nt, n, y, lp->d_col_slot, ctl);
      return;
    }
    for (int l = 0; l < lp->nlevels; ++l) {
      const int grid = lp->h_back_start[l + 1] - lp->h_back_start[l];
      if (grid <= 0) continue;
      count_launch(kLfDenseRest);
      hipLaunchKernelGGL(k_back_level, dim3((unsigned)grid), dim3(256), 0, s, A, LinvT, lp->d_back_cols + lp->h_back_start[l], lp->d_struct_start,
                         lp->d_struct_rows, nt, n, zbuf, y, lp->d_col_slot, ctl);
    }
    return;
  }
  // Outer panels of NB tile columns.  Inside a panel the plain right-looking steps run on the panel's
  // columns only; the tiles to the right then receive the whole panel in one launch (their load / store is
  // paid once per NB columns).  Up to 64 tile columns the matrix is one panel: exactly the plain algorithm.
  const int NB = dense_panel_width(nt, ov);
  const bool big_kernel = !ov || ov->big;
  const bool overlap = ov && ov->s2 && ov->overlap && big_kernel && NB < nt;
  int npanel = 0;
  bool b_pending = false;  // an update on the second stream has been recorded in ov->evB and not yet waited for
  for (int p0 = 0; p0 < nt; p0 += NB, ++npanel) {
    const int pend = (p0 + NB - 1 < nt - 1) ? p0 + NB - 1 : nt - 1;
    // factor column p0 (its tiles already hold every earlier column); ti in [p0, nt]
    hipLaunchKernelGGL(k_chol_step, dim3(nt - p0 + 1, 1), dim3(kStepThreads), 0, s, A, LinvT, nt, p0 - 1, fail, g_dbg_flags, p0 - 1, p0,
                       kStepNoOwnUpdate, panel_waves, g_chol_trace);
    for (int j = p0; j <= pend - 1; ++j) {  // apply column j to columns (j, pend], factor column j+1; ti in [j+1, nt]
      const int rows = nt - j, cols = pend - j;
      hipLaunchKernelGGL(k_chol_step, dim3(rows, cols), dim3(kStepThreads), 0, s, A, LinvT, nt, j, fail, g_dbg_flags, j, pend, 0, panel_waves, g_chol_trace);
    }
    if (pend >= nt - 1) break;
    // columns (pend, nt-1] receive the panel p0..pend; ti in [pend+1, nt]
    if (!big_kernel) {
      hipLaunchKernelGGL(k_chol_step, dim3(nt - pend, nt - 1 - pend), dim3(kStepThreads), 0, s, A, LinvT, nt, pend, fail, g_dbg_flags, p0, nt - 1,
                         kStepBig, panel_waves, g_chol_trace);
    } else if (!overlap) {
      launch_big(A, nt, pend, p0, pend + 1, nt - 1, s);
    } else {
      const int qend = (pend + NB < nt - 1) ? pend + NB : nt - 1;  // last column of the next panel
      hipEvent_t evF = ov->evF[npanel & 3], evB = ov->evB[npanel & 3];
      (void)hipEventRecord(evF, s);                                  // panel p0..pend is final
      // next panel's columns on the main stream; they were last written by the previous second-stream update
      if (b_pending) (void)hipStreamWaitEvent(s, ov->evB[(npanel - 1) & 3], 0);
      launch_big(A, nt, pend, p0, pend + 1, qend, s);
      // the columns beyond, concurrently with the next panel's steps (disjoint tile columns)
      if (qend < nt - 1) {
        (void)hipStreamWaitEvent(ov->s2, evF, 0);
        launch_big(A, nt, pend, p0, qend + 1, nt - 1, ov->s2);
        (void)hipEventRecord(evB, ov->s2);
        b_pending = true;
      } else {
        b_pending = false;
      }
    }
  }
  if (overlap && npanel > 0) {
    // everything queued on the second stream must be complete before the substitution (and the next assemble)
    for (int k = 0; k < 4; ++k) (void)hipStreamWaitEvent(s, ov->evB[k], 0);
  }
  hipLaunchKernelGGL(k_z_init, dim3((nt * kTile + 255) / 256), dim3(256), 0, s, A, nt, zbuf);
  for (int t1 = nt; t1 > 0; t1 -= kBsG) {
    const int t0 = t1 - kBsG > 0 ? t1 - kBsG : 0;
    hipLaunchKernelGGL(k_backsub_group, dim3(t0 > 0 ? t0 : 1), dim3(256), 0, s, A, LinvT, nt, n, t0, t1, zbuf, y, lp ? lp->d_col_slot : nullptr);
  }
}

}  // namespace mpsfm
