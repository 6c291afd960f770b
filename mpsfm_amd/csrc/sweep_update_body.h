// Body of the update sweep (see ba_kernels.hip), shared by k_update_sweep and the single-launch solver of small problems
// (local_lm.hip).
#pragma once
#include "common.h"
#include "sweep_common.h"

namespace mpsfm {

// LDS of one chunk's update sweep: 12 KB, 6.4 KB with the hand-off (no V)
template <bool kHandoff>
struct UpdLdsT {
  double V[kHandoff ? 1 : kPtsMax * 6];
  double g[kPtsMax * 3];   // g_p + W^T y_c (hand-off: W^T y_c alone)
  int32_t slot[kLocalCamsMax];
  double red[5 * (kThreads / 64)];
  uint8_t lpt[kThreads];   // landmark of every record (the first record of a landmark writes its candidate)
  double cand[kDenseCams * 16];  // fused camera update: candidate rows (R, t, K) of the chunk's cameras by local index
};

// Update sweep of chunk `cix` by one workgroup of kThreads threads; yc: the camera steps by slot (HBM, or LDS for kLocal).
//   1  one thread per record: the linearisation again (cheaper than 240 B per record through HBM), V_p and g_p + W^T y_c per landmark:
//      summed along the lanes first (the records of a landmark are neighbouring lanes: DPP segmented scan, as in the track
//      sweep), one LDS add per (16-lane row, landmark) run
//   2  EVERY record solves its landmark's 3x3 system itself (the ~5 records of a landmark repeat ~80 operations) instead of one
//      thread per landmark between two barriers: y_p, the candidate landmark — written by the landmark's first record —, the
//      model cost change and the candidate cost follow in the same registers
// kHandoff: the dense track sweep of the same iteration — same state, same radius — has left the factor F and g_p of every
// variable landmark in A.pt_fac.  Step 1 then only sums W^T y_c (three values through the scan and the LDS adds, no V), and step 2
// starts from the nine doubles of the record's landmark, requested behind the linearisation and in front of the scan and the second
// barrier (beside the record loads they are 12 more registers at the pressure peak, and 0.6 us); F[0] > 0 marks a valid factor.
// Entry: the chunk header and, in the launch chain, `term` of the control block are requested together; the camera list and the
// records follow from the header alone and are in flight while `term` is tested (in front of the first store) and LDS is cleared.
// Behind the first barrier the candidate lanes (fused camera update) and the records request their operands side by side; workgroup
// 0 runs the fused camera update for all cameras at the very end.  118 registers (hand-off and recompute), four workgroups per CU.
template <bool kLocal, bool kHandoff>
__device__ __forceinline__ void update_sweep_chunk(const SweepArgs& A, int cix, double lm_radius, const double* l_tab, const double* l_tab2,
                                                   const double* yc, UpdLdsT<kHandoff>& S, const CamUpdArgs& U, bool fuse) {
  constexpr int NV = kHandoff ? 3 : 9;  // sums per record: [V_p (6),] g (3)
  const int tid = thread_index<kLocal>();
  // ---- entry: two batches of loads instead of a chain of dependent trips ---------------------------------------------------------------
  // batch 0: the chunk header, and behind it (vector loads return in order: the header must not wait for a block that comes all the
  // way from memory) the control block (launch chain only, see lm_term_chain)
  const ChunkHdr H = A.chunks[cix];
  [[maybe_unused]] int32_t term = kLmRunning;
  if constexpr (!kLocal) {
    term = lm_term_chain(A.ctl, A.chunks);
    if constexpr (!kHandoff) lm_radius = lm_radius_chain(A.ctl, A.chunks, lm_radius);  // (the hand-off brings the damped factors)
  }
  const int nrec = H.nrec, npt = H.npt, ncam = H.ncam;
  // batch 1, from the header alone: the camera list and the chunk's records.  Fused camera update: the candidate rows are formed by
  // the LAST lanes of the workgroup (they hold a record only in a chunk of more than kThreads - kDenseCams records), which ask for
  // their camera's slot here as well
  constexpr int kCandTid0 = kThreads - kDenseCams;
  const bool cand_lane = !kLocal && fuse && tid >= kCandTid0 && tid - kCandTid0 < ncam;
  // A lane without a record (camera) keeps its guard but takes no branch: it reads the head of the chunk table, which is always
  // readable, and drops the value.  With a branch around the requests the compiler counts the loads in flight for the path that
  // skips them, and the wait for `term` below becomes a wait for the records.
  const bool has_rec = tid < nrec;
  const int32_t my_slot = *(tid < ncam ? &A.chunk_cams[H.cam0 + tid] : reinterpret_cast<const int32_t*>(A.chunks));
  [[maybe_unused]] int32_t cand_slot = 0;
  if constexpr (!kLocal) cand_slot = *(cand_lane ? &A.chunk_cams[H.cam0 + tid - kCandTid0] : reinterpret_cast<const int32_t*>(A.chunks));
  uint32_t meta = *(has_rec ? &A.rec_meta[H.rec0 + tid] : reinterpret_cast<const uint32_t*>(A.chunks));
  int cam = *(has_rec ? &A.rec_cam[H.rec0 + tid] : reinterpret_cast<const int32_t*>(A.chunks));
  int lpt = 0;
  double2 xy = *(has_rec ? &reinterpret_cast<const double2*>(A.rec_xy)[H.rec0 + tid] : reinterpret_cast<const double2*>(A.chunks));
  // the solve is over (the iteration queued ahead of the news): leave before the first global store
  if constexpr (!kLocal) {
    if (A.ctl != nullptr && lm_over_chain(term)) return;
  }
  if constexpr (!kHandoff) for (int i = tid; i < npt * 6; i += kThreads) S.V[i] = 0.0;
  for (int i = tid; i < npt * 3; i += kThreads) S.g[i] = 0.0;
  if (tid < ncam) S.slot[tid] = my_slot;
  [[maybe_unused]] int cand_cam = 0;  // (lands under the barrier)
  if constexpr (!kLocal) cand_cam = *(cand_lane ? &U.cam_of_slot[cand_slot] : reinterpret_cast<const int32_t*>(A.chunks));
  __syncthreads();
  // (nothing derived from the records is to be computed, and so waited for, in front of the barrier: the clears run under their trip)
  asm volatile("" : "+v"(meta), "+v"(cam));
  if (!has_rec) meta = 0;
  // (the candidate camera's index is waited for here by every lane: a load left pending on the lanes that skip the requests below
  // would make the compiler wait for ALL loads in flight at the first reuse of its register)
  if constexpr (!kLocal) asm volatile("" : "+v"(cand_cam));

  RecUpd L;
  double d = 1.0, m = 0.0, a = 1.0;
  double X[3] = {0, 0, 0}, psc[3] = {0, 0, 0};
  bool ok = true, variable = false;
  double Vg[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) Vg[k] = 0.0;
  double fac[kHandoff ? 9 : 1] = {};  // the landmark's F and g_p
  // batch 2.  The candidate lanes first ask for what their camera's candidate row is made of (pose, scales, step, intrinsics), then
  // every record for what its contents index: landmark, scales, pt_kv and the depth triple.  The two trips run side by side; the
  // candidate rows, which are read behind the second barrier only (record_cost), are formed when both have landed.  The intrinsics
  // come from the camera's row of the table at the linearisation point: k_build_camtab and cam_update_all copy them there from
  // intr[4 intr_idx[i]] and nothing else writes them, so they are the same bits and the intr_idx -> intr trip is saved.
  [[maybe_unused]] double cq[4], ct[3], ccs[6], cy[6], ck[4];
  if constexpr (!kLocal) {
    if (cand_lane) {
      const int i = cand_cam;
#pragma unroll
      for (int k = 0; k < 4; ++k) { cq[k] = U.q[4 * i + k]; ck[k] = A.camtab[(size_t)i * kCamRec + 12 + k]; }
#pragma unroll
      for (int k = 0; k < 3; ++k) ct[k] = U.t[3 * i + k];
#pragma unroll
      for (int k = 0; k < 6; ++k) { ccs[k] = U.cs[6 * i + k]; cy[k] = yc[(size_t)cand_slot * 6 + k]; }
    }
  }
  if (tid < nrec) {
    const int rix = H.rec0 + tid;
    lpt = (meta >> 8) & 0xff;
    if (meta & kRecHasDepth) { d = A.rec_d[rix]; m = A.rec_m[rix]; a = A.rec_a[rix]; }
    const int pix = H.pt0 + lpt;
    variable = A.pt_kv[pix] != 0xffff;
#pragma unroll
    for (int k = 0; k < 3; ++k) { X[k] = A.pts[3 * pix + k]; psc[k] = A.ps[3 * pix + k]; }
  }
  if constexpr (!kLocal) {
    // the candidate row of local camera tid - kCandTid0: the arithmetic of cam_update_all, so that the cost below is evaluated at
    // exactly the pose workgroup 0 writes out
    if (cand_lane) {
      double qn[4], tn[3], s0 = 0.0, s1 = 0.0, s2 = 0.0;
      camera_candidate(cq, ct, ccs, cy, nullptr, qn, tn, s0, s1, s2);
      double* o = &S.cand[(tid - kCandTid0) * 16];
      quat_to_R(qn, o);
      o[9] = tn[0]; o[10] = tn[1]; o[11] = tn[2];
      o[12] = ck[0]; o[13] = ck[1]; o[14] = ck[2]; o[15] = ck[3];
    }
  }
  if (tid < nrec) {
    const int lcam = meta & 0xff;
    linearize_update(camera_row<kLocal>(A.camtab, l_tab, S.slot, cam, lcam), X, psc, meta, xy.x, xy.y, d, m, a, A.loss,
                     lcam != (int)kLcamConst ? yc + (size_t)S.slot[lcam] * 6 : nullptr, L);
    ok = L.ok;
    if constexpr (kHandoff) {
      if (variable) {  // (a constant landmark's slot is never written)
#pragma unroll
        for (int k = 0; k < 9; ++k) fac[k] = A.pt_fac[(size_t)9 * (H.pt0 + lpt) + k];
      }
    }
    if (L.ok && psc[0] != 0.0) {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double j0 = L.Jp[3 * r], j1 = L.Jp[3 * r + 1], j2 = L.Jp[3 * r + 2];
        if constexpr (!kHandoff) { Vg[0] += j0 * j0; Vg[1] += j0 * j1; Vg[2] += j0 * j2; Vg[3] += j1 * j1; Vg[4] += j1 * j2; Vg[5] += j2 * j2; }
        const double rr = kHandoff ? L.mrow[r] : L.r[r] + L.mrow[r];  // (hand-off: J_p^T r is in g_p already)
        Vg[NV - 3] += j0 * rr; Vg[NV - 2] += j1 * rr; Vg[NV - 1] += j2 * rr;
      }
    }
  }
  S.lpt[tid] = tid < nrec ? (uint8_t)lpt : (uint8_t)255;
  {  // all lanes take part: threads beyond the records carry zeros and landmark 0
    seg_step<1>(lpt, Vg); seg_step<2>(lpt, Vg); seg_step<4>(lpt, Vg); seg_step<8>(lpt, Vg);
    const int nlpt = __builtin_amdgcn_update_dpp(-1, lpt, 0x101, 0xf, 0xf, false);  // row_shl:1: the right neighbour's landmark
    if (nlpt != lpt && lpt < npt) {  // last lane of its run inside the row (lane 15 of a row sees -1)
      if constexpr (!kHandoff) {
#pragma unroll
        for (int k = 0; k < 6; ++k) if (Vg[k] != 0.0) atomicAdd(&S.V[lpt * 6 + k], Vg[k]);
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) if (Vg[NV - 3 + k] != 0.0) atomicAdd(&S.g[lpt * 3 + k], Vg[NV - 3 + k]);
    }
  }
  __syncthreads();

  double step_sq = 0.0, xn_sq = 0.0, mcc = 0.0, cand = 0.0;
  if (tid < nrec) {
    const int pix = H.pt0 + lpt;
    double yp[3] = {0, 0, 0}, X2[3] = {X[0], X[1], X[2]};
    const bool first = tid == 0 || S.lpt[tid - 1] != (uint8_t)lpt;
    if (variable) {
      double F[6];
      bool okf;
      double g0 = S.g[lpt * 3], g1 = S.g[lpt * 3 + 1], g2 = S.g[lpt * 3 + 2];
      if constexpr (kHandoff) {
#pragma unroll
        for (int k = 0; k < 6; ++k) F[k] = fac[k];
        okf = F[0] > 0.0;  // the track sweep zeroes the factor of a block it could not factor
        g0 = fac[6] + g0; g1 = fac[7] + g1; g2 = fac[8] + g2;
      } else {
        double V[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) V[k] = S.V[lpt * 6 + k];
        damp_landmark(V, A.min_diag, A.max_diag, lm_radius, sweep_rcp(lm_radius));
        okf = spd3_inv_factor(V, F);  // F = chol(V + D)^-1, the factor the track sweep forms for the same block
      }
      if (!okf) {
        ok = false;  // (every record of the landmark reports it: the count only has to be non-zero)
      } else {
        const double v0 = F[0] * g0, v1 = F[1] * g0 + F[2] * g1, v2 = F[3] * g0 + F[4] * g1 + F[5] * g2;  // F g
        yp[0] = -(F[0] * v0 + F[1] * v1 + F[3] * v2); yp[1] = -(F[2] * v1 + F[4] * v2); yp[2] = -(F[5] * v2);  // -F^T F g
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double dl = psc[k] * yp[k];
          X2[k] = X[k] + dl;
          if (first) { step_sq += dl * dl; xn_sq += X2[k] * X2[k]; }
        }
      }
    }
    if (first) {
#pragma unroll
      for (int k = 0; k < 3; ++k) A.pts2[3 * pix + k] = X2[k];
    }
    if (ok) {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double mm = L.mrow[r] + L.Jp[3 * r] * yp[0] + L.Jp[3 * r + 1] * yp[1] + L.Jp[3 * r + 2] * yp[2];
        mcc -= mm * (L.r[r] + 0.5 * mm);
      }
      bool ok2 = true;
      const int lcam = (int)(meta & 0xff);
      const double* row;
      if (!kLocal && fuse) row = lcam != (int)kLcamConst ? &S.cand[lcam * 16] : A.camtab + (size_t)cam * kCamRec;
      else row = camera_row<kLocal>(kLocal ? A.camtab : A.camtab2, l_tab2, S.slot, cam, lcam);  // (constant cameras have no candidate row of their own)
      cand = record_cost(row, X2, meta, xy.x, xy.y, d, m, a, A.loss, ok2);
      if (!ok2) { ok = false; cand = 0.0; }
    }
  }
  const double r0 = wave_sum(cand), r1 = wave_sum(ok ? 0.0 : 1.0), r2 = wave_sum(mcc), r3 = wave_sum(step_sq),
               r4 = wave_sum(xn_sq);
  const int w = tid >> 6;
  if ((tid & 63) == 0) { S.red[w] = r0; S.red[4 + w] = r1; S.red[8 + w] = r2; S.red[12 + w] = r3; S.red[16 + w] = r4; }
  __syncthreads();
  if (tid < 5) {
    const double* s = &S.red[4 * tid];
    A.part2[(size_t)cix * 8 + tid] = (s[0] + s[1]) + (s[2] + s[3]);
  }
  // Workgroup 0 does what k_cam_update does for all cameras, behind its own chunk: nothing of the chunk is alive here, and the camera
  // loop keeps the constants of libm's sine and cosine in registers (in front of the chunk, where the record loads are in flight, that
  // was the register peak of the whole kernel).  No other workgroup of this launch reads what it writes.
  if constexpr (!kLocal) {
    if (fuse && cix == 0) {
      __syncthreads();  // S.red is read above
      cam_update_all(U, yc, S.red);
    }
  }
}

}  // namespace mpsfm
