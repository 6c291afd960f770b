// The launch wrappers of the bundle-adjustment kernels (ba_kernels.hip, sweep_dense.hip, dense_chol.hip, local_lm.hip): the one
// declaration of each, default arguments included.  The defining files include it too, so a definition that drifts from its
// declaration does not compile.
#pragma once
#include "common.h"
#include "local_lm.h"

namespace mpsfm {
// ---- launches enqueued by the calling thread, per kernel family: counted on the host in the wrappers below; a solve starts them
// from zero and leaves its counts with the handle (code 34 of mpsfm_debug_table) ------------------------------------------------
enum LaunchFamily {
  kLfTrackSweep,   // k_track_sweep_dense, k_track_sweep, k_long_track_sweep
  kLfReduceSlabs,  // k_reduce_slabs
  kLfAssemble,     // k_assemble
  kLfCholLevel,    // k_chol_level
  kLfDenseRest,    // behind the level launches: k_inv_y, k_back_level (the outer-panel path is not counted)
  kLfUpdateSweep,  // k_update_sweep, k_long_update_sweep
  kLfDecide,       // k_lm_reduce_decide, k_lm_decide
  kLfScales,       // k_cam_scales, k_pt_scales, k_build_camtab
  kLfOther,        // the rest of this header
  kLfCount
};
extern thread_local int64_t g_launches[kLfCount];  // dense_chol.hip
inline void count_launch(LaunchFamily f, int n = 1) { g_launches[f] += n; }

// ---- ba_kernels.hip / sweep_dense.hip ----------------------------------------------------------------------------------------
void launch_track_sweep(const SweepArgs&, int nchunks, bool diag_only, hipStream_t);
void launch_update_sweep(const SweepArgs&, int nchunks, hipStream_t, const CamUpdArgs* cu = nullptr);
void launch_track_sweep_dense(const SweepArgs&, int nchunks, hipStream_t);
// direct (may be NULL): the sums go straight into the tiles of the dense solve (DirectAsm in common.h), Sblk is not written
void launch_reduce_slabs(const RedDest* dests, int ndest, const int32_t* srcs, const double* slab, double* Sblk, double* gc, double* wv, double* diagU,
                         const LmCtl* ctl, hipStream_t, const DirectAsm* direct = nullptr);
void launch_cost_records(const CostArgs&, int nblocks, hipStream_t);
void launch_reduce_cols(const double* part, int64_t rows, int stride, int ncols, uint32_t max_mask, double* out, hipStream_t,
                        double* out2 = nullptr, int gmax_slot = -1);
void launch_build_camtab(int nc, const double* q, const double* t, const double* intr, const int32_t* intr_idx,
                         const double* cs, double* camtab, hipStream_t);
void launch_cam_scales(int nc, const int32_t* cam_slot, const double* cmask, const double* diagU, int jacobi, double* cs, hipStream_t);
void launch_pt_scales(int64_t np, const uint16_t* pt_kv, const double* diagV, int jacobi, double* ps, hipStream_t);
void launch_cam_update(int nc, const int32_t* cam_slot, const double* q, const double* t, const double* cs, const double* yc,
                       const double* gc, double* q2, double* t2, double* scal, hipStream_t, const double* intr = nullptr,
                       const int32_t* intr_idx = nullptr, double* camtab2 = nullptr, int* chol_fail = nullptr, const LmCtl* ctl = nullptr);
constexpr int kReduceThreads = 1024;  // the workgroup of k_reduce_cols and k_lm_reduce_decide
void launch_lm_decide(LmCtl* ctl, double* scal, const LmOpts& o, LmCtl* host_copy, hipStream_t, const double* redsc = nullptr);
void launch_zero(double* p, int64_t n, const LmCtl* ctl, hipStream_t);
void launch_lm_reduce_decide(const double* part, const double* part2, int64_t rows, LmCtl* ctl, double* scal, const LmOpts& o, LmCtl* host_copy, hipStream_t);
void launch_lm_prologue(const LmCtl* ctl, double* red, int64_t nred, int nc, int64_t np, double* q, double* t, double* camtab, double* pts, const double* q2,
                        const double* t2, const double* camtab2, const double* pts2, hipStream_t);
void launch_lm_accept(const LmCtl* ctl, int nc, int64_t np, double* q, double* t, double* camtab, double* pts, const double* q2, const double* t2,
                      const double* camtab2, const double* pts2, hipStream_t);
void launch_pts_sqnorm(int64_t np, const uint16_t* pt_kv, const double* pts, double* part, int nblocks, hipStream_t);
void launch_gmax_to_slot(double* redsc, int rank, hipStream_t);
void launch_lm_pack(const double* scal, double* sums, hipStream_t);
void launch_lm_init(LmCtl* ctl, const double* scal, const double* sums, hipStream_t);
void launch_permute_pts(int64_t np, const int32_t* perm, const double* src, double* dst, bool scatter, hipStream_t);
void launch_gmax_from_slots(const double* redsc, double* scal, hipStream_t);

// ---- dense_chol.hip ----------------------------------------------------------------------------------------------------------
extern int g_dbg_flags;  // bits 0-7 dense-solve ablations, bits 8-15 track-sweep ablations (mpsfm_debug_set)
void launch_assemble(const AssembleArgs&, hipStream_t);
// damp (may be NULL; level-scheduled path only): A comes undamped from the direct slab reduction, the first level launch adds the damping
// (DampArgs; the caller has seen LevelPlanDev::damp_in_launch0)
void launch_dense_solve(double* A, double* work, int nt, int n, double* y, int* fail, hipStream_t, DenseOverlap* ov, const LevelPlanDev* lp,
                        const LmCtl* ctl = nullptr, const DampArgs* damp = nullptr);
bool dense_level(const DenseOverlap* ov, const LevelPlanDev* lp);
int dense_plain_max_tiles();
int dense_inv_rows();
size_t dense_work_doubles(int nt);
double* dense_pinv(double* work, int nt, const DenseOverlap* ov, const LevelPlanDev* lp);

// ---- local_lm.hip ------------------------------------------------------------------------------------------------------------
// co-resident workgroups the device offers the kernel (0: cooperative launches unavailable)
int local_lm_max_chunks(int device);
// enqueues the solve; returns a hipError_t as int
int launch_local_lm(const LocalArgs& a, hipStream_t s);

}  // namespace mpsfm
