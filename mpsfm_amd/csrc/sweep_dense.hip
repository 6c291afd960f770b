// Track sweep of the DENSE chunks (gfx950) and the reduction of their slabs.
//
// What Ceres does per LM iteration inside pyceres.solve for the problem of reference
// mpsfm/sfm/mapper/bundle_adjustment.py:67-185 — evaluate every residual block and its Jacobian, form J^T J, eliminate the
// landmark blocks (SPARSE_SCHUR) — for one chunk of consecutive (camera-set sorted) landmarks per workgroup.  A dense chunk
// has at most kDenseCams (16) variable cameras, kDensePts (96) landmarks, kObsMax (252) merged records and one record per
// (camera, variable landmark).
//
//   entry  two batches of loads instead of a chain of dependent trips: the control block (term, accepted, radius: vector loads)
//       beside the chunk header, then, from the header alone, the chunk's records; `term` is tested behind these requests
//       and in front of the first global store
//   P0  while the records are in flight: adoption of an accepted candidate, clear the LDS accumulators
//   P1  one thread per record: the loads indexed by the record (landmark, scales, pt_kv, depth triple, camera row) in one batch —
//       pt_kv and the scales stay in registers for P2 —, residuals, analytic Jacobians, robust weights (sweep_common.h);
//       V_p, g_p per landmark and U_c (upper triangle), g_c per camera by ds_add_f64 — the camera accumulators in 4 (up to 8
//       cameras) or 2 copies chosen by the landmark, because neighbouring lanes are the records of one landmark and would
//       otherwise add ~13-fold to one address; W = Jc^T Jp stays in registers
//   P2  one thread per landmark: F = chol(V + D)^-1, F g_p
//   P3a Z = W F^T to LDS (18 doubles per record), W V^-1 g_p per camera
//   P3b S_chunk = M M^T, M the (6 ncam) x (3 npt) matrix of the Z blocks, on the matrix pipe: v_mfma_f64_16x16x4_f64 with a
//       LANDMARK as K index (four landmarks per instruction, one coordinate each).  The 16-row tile pairs (ti <= tj) are
//       dealt to the four waves; a wave sums ITS pairs over all landmarks, so every accumulator is complete in its registers
//       and goes straight to the chunk's SLAB in HBM with plain stores (U_c - Z Z^T on the diagonal blocks) — no LDS staging,
//       no LDS atomics, no global atomics
//   P4  g_c | W V^-1 g_p | diag U of every local camera to the slab, chunk partials (cost, invalid records, max |g_p|)
//
// k_reduce_slabs then sums the slabs per destination (a 6x6 block of S or a camera's vectors) and adds the sums into the
// reduced buffer: 0.7 MB of atomics at C3 instead of 24 MB, and a fixed summation order per destination part.
// LDS: 53.4 KB per workgroup = three workgroups per CU.
#include "sweep_dense_body.h"
#include "ba_launch.h"
#include <algorithm>

namespace mpsfm {

__global__ __launch_bounds__(kThreads, 3) void k_track_sweep_dense(SweepArgs A) {
  __shared__ DenseLds S;
  // One workgroup per chunk.  Persistent workgroups (3 per CU taking chunks from a cost-sorted list through a shared counter) were
  // measured and dropped: the slots stay full, but every chunk then takes longer (wave life 21.5 -> 24.7 us at C3: the sweep is
  // bound by the CU's shared pipes, not by the 22 % of slot time the dispatcher leaves empty) — 0.118 against 0.111 ms.
  // What stays of that list is the ORDER: the dispatcher starts workgroups by ascending blockIdx.x, and workgroup b takes chunk
  // order[b], heaviest first (dense_sweep_cost in common.h), so the chunks that run long start in the first round and the last
  // round holds the light ones.  One scalar load in front of the header (MPSFM_SWEEP_ORDER=0: no table, chunk b + chunk0).
  // (the body requests the control block itself, beside the chunk header: the radius given here is what it uses without one)
  const int cix = A.order ? A.order[blockIdx.x] : (int)blockIdx.x + A.chunk0;
  dense_sweep_chunk<false>(A, cix, A.radius, nullptr, S, A.part);
}

// One wave per destination part: sums the part's slab sources in table order and adds the sum into the (zeroed) reduced buffer.
// kDirect (DirectAsm in common.h): the blocks of S go to the tiles of A instead of Sblk — where an element lands is arithmetic on
// the first columns of the destination's two slots, requested beside the destination and worked out under the sums —, the camera
// vectors also as wv - gc to the right-hand-side row and diag U by column for the panels' damping.
// (256, 8): eight waves per SIMD in either form — the parts of C3 fill the device once at that occupancy, and at seven a second round
// of workgroups repeats the whole chain of dependent loads.
template <bool kDirect>
__global__ __launch_bounds__(256, kDirect ? 8 : 1) void k_reduce_slabs(const RedDest* __restrict__ dests, int ndest, const int32_t* __restrict__ srcs,
                                                      const double* __restrict__ slab, double* Sblk, double* gc, double* wv, double* diagU,
                                                      const LmCtl* ctl, DirectAsm T) {
  if (lm_over(ctl)) return;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= ndest) return;
  RedDest D;
  [[maybe_unused]] RedCols cc{0, 0};
  if constexpr (kDirect) { const RedDestCols X = T.dests[w]; D = X.d; cc = X.c; }
  else D = dests[w];
  bool active;
  if (D.kind == 2) active = lane < 18;
  else if (D.kind == 1) { const int ra = lane / 6, cb = lane - 6 * ra; active = lane < 36 && cb >= ra; }
  else active = lane < 36;
  // the element's place in A and, inside a diagonal tile, its mirror image's (32-bit: the direct form is taken up to 64 tile columns);
  // camera vectors: the system column.  Every destination lies in a tile the factorisation reads (the plan's tile pattern holds every
  // pair of cameras that share a landmark), so no look at the table of live tiles.
  [[maybe_unused]] int32_t o0 = 0, o1 = -1, col = 0;
  if constexpr (kDirect) {
    if (D.kind == 2) {
      col = cc.c0 + lane % 6;
      o0 = (int32_t)lt_tile(T.nt, col >> 5) * 1024 + (col & 31);  // row 0 of the right-hand-side tile
    } else {
      const int a = lane / 6, b = lane - 6 * a;
      const int r = cc.c0 + a, c = cc.c1 + b;  // the stored block is (lower slot, higher slot); a diagonal block holds its upper triangle
      const int R = r > c ? r : c, C = r > c ? c : r;
      const int32_t id = active ? (int32_t)lt_tile(R >> 5, C >> 5) : 0;
      o0 = id * 1024 + (R & 31) * 32 + (C & 31);
      if ((R >> 5) == (C >> 5) && R != C) o1 = id * 1024 + (C & 31) * 32 + (R & 31);
    }
  }
  double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int s = D.s0;
  for (; s + 8 <= D.s1; s += 8) {
    int32_t o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = srcs[s + k];
    if (active) {
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += slab[(size_t)o[k] * 18 + lane];
    }
  }
  for (int k = 0; s < D.s1; ++s, ++k)
    if (active) acc[k & 7] += slab[(size_t)srcs[s] * 18 + lane];
  const double v = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  if (!active || v == 0.0) return;
  if (D.kind == 2) {
    double* base = lane < 6 ? gc : (lane < 12 ? wv : diagU);
    atomicAdd(&base[(size_t)D.dst * 6 + (lane % 6)], v);
    if constexpr (kDirect) {
      if (lane >= 12) atomicAdd(&T.diag_col[col], v);
      else atomicAdd(&T.A[o0], lane < 6 ? -v : v);  // rhs = wv - gc
    }
  } else if constexpr (kDirect) {
    atomicAdd(&T.A[o0], v);
    if (o1 >= 0) atomicAdd(&T.A[o1], v);
  } else {
    atomicAdd(&Sblk[(size_t)D.dst * 36 + lane], v);  // (a diagonal block: diag U travels in the camera vectors)
  }
}

void launch_track_sweep_dense(const SweepArgs& a, int nchunks, hipStream_t s) {
  if (nchunks > 0) { count_launch(kLfTrackSweep); hipLaunchKernelGGL(k_track_sweep_dense, dim3(nchunks), dim3(kThreads), 0, s, a); }
}
void launch_reduce_slabs(const RedDest* dests, int ndest, const int32_t* srcs, const double* slab, double* Sblk, double* gc, double* wv, double* diagU,
                         const LmCtl* ctl, hipStream_t s, const DirectAsm* direct) {
  if (ndest <= 0) return;
  count_launch(kLfReduceSlabs);
  if (direct) hipLaunchKernelGGL(k_reduce_slabs<true>, dim3((ndest + 3) / 4), dim3(256), 0, s, dests, ndest, srcs, slab, Sblk, gc, wv, diagU, ctl, *direct);
  else hipLaunchKernelGGL(k_reduce_slabs<false>, dim3((ndest + 3) / 4), dim3(256), 0, s, dests, ndest, srcs, slab, Sblk, gc, wv, diagU, ctl, DirectAsm{});
}

}  // namespace mpsfm
