// The bundle-adjustment handle and what more than one of its files needs: ba_build.hip creates and frees it, ba_comm.hip sums over
// the ranks of a landmark-sharded run, ba_solver.hip solves on it, ba_debug.hip probes it.
#pragma once
#include <cstdint>
#include <memory>
#include <vector>

#include "ba_launch.h"
#include "build_host.h"
#include "common.h"
#include "dev_resources.h"
#include "devbuild.h"

struct mpsfm_ba_handle {
  int device = 0;
  // every device block, event, pinned block and pooled stream below; waits for both streams before they go back.  The
  // pointers of this struct are views into it.
  mpsfm::DeviceBlocks own;
  hipStream_t stream = nullptr;  // from `own`, or the caller's (mpsfm_ba_options::stream): waited for, never released
  void* comm = nullptr;  // ncclComm_t of a landmark-sharded run with use_rccl
  mpsfm::DenseOverlap ov;  // second stream for the dense factorisation in outer panels (MPSFM_CHOL_NB)
  mpsfm::SPattern spat;                    // which blocks of S exist: block skyline or index form (up to kIndexMaxSlots slots), host copies
  mpsfm::BlockSky sky{nullptr, nullptr, nullptr, 0};  // the device copy
  mpsfm::CholPlan plan;                    // camera order, tile elimination tree and launch tables of the dense factorisation (chol_plan.h)
  mpsfm::LevelPlanDev lp;                  // the device copies of the plan's tables
  std::vector<int32_t> nat_slot;    // variable camera in the caller's order -> slot (the accessors of S and y speak the caller's order)
  int n_user = 0;                   // 6 x variable cameras: the reduced dimension the caller sees and the length of the slot-indexed vectors (n counts the
                                    // system's columns incl. the alignment padding)
  mpsfm_ba_options opt{};
  mpsfm::LossParams loss{};
  // sizes
  int nc = 0, np_user = 0;
  int64_t np = 0, np_chunked = 0;   // re-ordered landmarks (all referenced) / those inside chunks
  int64_t nrec = 0, nfixed = 0, nblocks_total = 0, nblocks_reduced = 0;
  double nblocks_global = 0, nblocks_reduced_global = 0, nvarpts_global = 0;
  int ncv = 0, n = 0, nt = 0, nchunks = 0, nlong = 0;
  int n_dense = 0;                  // chunks [0, n_dense) are swept by k_track_sweep_dense, the rest by the general kernel
  double* d_slab = nullptr;         // slabs of the dense chunks
  mpsfm::RedDest* d_red_dests = nullptr;   // slab reduction: destination parts and their sources
  int32_t* d_red_srcs = nullptr;
  int32_t* d_sweep_order = nullptr;        // [n_dense] the chunk the b-th workgroup of k_track_sweep_dense takes: heaviest first (SweepArgs::order)
  int64_t slab_units = 0;                  // 18-double units of d_slab
  mpsfm::RedDestCols* d_red_cols = nullptr;  // direct form of the slab reduction (DirectAsm): where every destination part lands; NULL: the
                                           // handle has a general chunk, a long track, several ranks or no level plan and keeps k_assemble
  double* d_diag_col = nullptr;            // [32 nt] diag U by system column, for the damping in the first level launch
  int n_red_dests = 0;
  int64_t n_red_srcs = 0, n_chunk_cams = 0, n_blk_desc = 0, n_blk_ent_start = 0, n_ents = 0;  // table sizes (diagnostics: mpsfm_debug_table)
  bool built_on_device = false;
  mpsfm::LongHdr* d_lhdr = nullptr;
  double* d_wl = nullptr;
  int64_t red_count = 0, sblk_count = 0;
  std::vector<int32_t> perm;        // re-ordered landmark -> caller's index
  int32_t* d_cam_of_slot = nullptr; // slot -> camera (the fused camera update of k_update_sweep)
  int32_t* d_perm = nullptr;        // device copy, and the landmarks in the caller's order as last uploaded: the state crosses the bus
  double* d_user_pts = nullptr;     // unpermuted and is re-ordered on the device (every landmark referenced: np == np_user)
  std::vector<int32_t> cam_slot_h;
  // device state
  double *d_q = nullptr, *d_t = nullptr, *d_q2 = nullptr, *d_t2 = nullptr, *d_q0 = nullptr, *d_t0 = nullptr;
  double *d_pts = nullptr, *d_pts2 = nullptr, *d_pts0 = nullptr;
  double *d_intr = nullptr, *d_cmask = nullptr, *d_cs = nullptr, *d_camtab = nullptr, *d_camtab2 = nullptr;
  int32_t *d_intr_idx = nullptr, *d_cam_slot = nullptr;
  double *d_ps = nullptr, *d_diagV = nullptr;
  double* d_pt_fac = nullptr;       // [np][9] landmark factors and gradients, track sweep -> update sweep (SweepArgs::pt_fac); NULL: the
                                    // handle has a general chunk or a long track and its update sweep recomputes them
  mpsfm::ChunkHdr* d_chunks = nullptr;
  int32_t *d_chunk_cams = nullptr, *d_blk_ent_start = nullptr;
  uint32_t *d_blk_desc = nullptr, *d_ents = nullptr;
  mpsfm::RecTablesDev rt;           // record and fixed-record tables
  // reduced buffer: Sblk | gc | wv | diagU | scalars
  double* d_red = nullptr;
  double *d_Sblk = nullptr, *d_gc = nullptr, *d_wv = nullptr, *d_diagU = nullptr, *d_redsc = nullptr;
  double *d_part = nullptr, *d_part2 = nullptr, *d_scal = nullptr, *d_costpart = nullptr;
  double* h_scal = nullptr;  // pinned
  mpsfm::LmCtl* d_ctl = nullptr;    // Levenberg-Marquardt control block (device) and the two pinned slots its copies land in
  mpsfm::LmCtl* h_ctl = nullptr;
  hipEvent_t ev2[4] = {nullptr, nullptr, nullptr, nullptr};  // second set of phase events (two iterations are in flight)
  double *d_A = nullptr, *d_yc = nullptr, *d_dwork = nullptr;
  int* d_fail = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  double last_radius = 1e4;
  bool scales_ready = false;
  int64_t last_launches[mpsfm::kLfCount] = {};  // what the last solve enqueued, per kernel family (code 34 of mpsfm_debug_table)
  double split_front_s = 0.0;  // ev0 -> ev1 of the last iteration read (solve_impl: is the front long enough to enqueue the back half behind it?)
  // single-launch solver of small problems (local_lm.hip): two accumulators | barrier words + clocks | per-iteration heads
  bool local_ok = false;
  double* d_local_acc = nullptr;
  int64_t* d_local_sync = nullptr;   // [0]: two 32-bit barrier words, [1..4]: phase clocks
  mpsfm::LmHead* d_local_log = nullptr;
  int local_log_cap = 0;
};

namespace mpsfm {

inline bool sharded(const mpsfm_ba_handle* h) { return h->opt.allreduce != nullptr || h->comm != nullptr; }
// every chunk dense, no long track: the dense sweep can adopt and zero, its landmark factors can be handed on, one workgroup per chunk
inline bool all_dense(const mpsfm_ba_handle* h) { return h->nlong == 0 && h->n_dense > 0 && h->n_dense == h->nchunks; }

// ---- ba_build.hip: handle creation
// What the phases of the table build produce.
struct TableBuild {
  CameraLayout cams;
  CholPlan plan;        // camera order, tile elimination tree and launch tables of the dense factorisation
  SPattern spat;        // which 6x6 blocks of S exist
  DevBuildOut tables;   // .t: the host tables of either build; the rest: the device build's tables
  SlabTables slabs;
  double nblocks_global = 0, nblocks_reduced_global = 0, nvarpts_global = 0;  // totals over the ranks
  bool built_on_device = false;
  bool slab_tables_on_device = false;  // slabs holds diag_block only: DevBuilder::slab_tables forms the reduction tables behind the uploads
};
// The device build where it applies (devbuild.h): its builder, created by build_tables, and the stream its copies run on.
struct DeviceStages {
  hipStream_t stream = nullptr;
  std::unique_ptr<DevBuilder> builder;
};

int check_problem(const mpsfm_ba_problem* P);
// The list of the build's phases.  `opt` gets its chunk caps on the way; `exchange` sums host values over the ranks of a `sharded`
// build (empty: one rank); `dev` NULL: host phases only.
int build_tables(const mpsfm_ba_problem* P, BuildOptions& opt, const SumExchange& exchange, bool sharded, int verbose, const Lap& lap, DeviceStages* dev,
                 TableBuild& out);
void level_plan_flags(const CholPlan& PL, LevelPlanDev& D);

int create_impl(const mpsfm_ba_problem* P, const mpsfm_ba_state* st, const mpsfm_ba_options* o, mpsfm_ba_handle** out);
int upload_state(mpsfm_ba_handle* h, const mpsfm_ba_state* st, bool as_initial);
void free_handle(mpsfm_ba_handle* h);

// ---- ba_comm.hip: RCCL, loaded at run time, and the caller's all-reduce hook
int comm_init_rank(mpsfm_ba_handle* h);  // h->comm from h->opt (use_rccl)
void comm_destroy(void* comm);
// sum `count` doubles over the ranks in place (one rank: nothing): complete on return / enqueued on the handle's stream
int allreduce_host(mpsfm_ba_handle* h, double* buf, int64_t count);
int allreduce_dev(mpsfm_ba_handle* h, double* buf, int64_t count);

// ---- ba_solver.hip: the form of a solve, and the pieces of an iteration that the solve and the probes of ba_debug.hip both enqueue
// What one solve does where the code has a choice: the eight run-time switches combined with the handle's structure, decided in
// solve_form and nowhere else, per solve and per probe call (never kept: tests flip the switches between solves on one handle).
// A probe states the form it wants by overriding fields of the form it read.
struct SolveForm {
  bool sweep_order;     // the dense sweep takes its chunks heaviest first (SweepArgs::order); MPSFM_SWEEP_ORDER=0: in table order
  bool entry_list;      // MPSFM_CHOL_ENTRY=list: the level launches walk item -> source list -> operands instead of launch records
  bool pt_handoff;      // the track sweep hands the landmark factors to the update sweep (d_pt_fac); MPSFM_PT_HANDOFF=0: recomputed
  bool fused_prologue;  // all_dense: the dense sweep adopts an accepted candidate and zeroes the reduced buffer itself (sharded runs
                        // too: the exchange comes behind the slab reduction); MPSFM_FUSE_PROLOGUE=0: k_lm_prologue
  bool fused_cam;       // ... and the update sweep forms the candidate cameras itself (CamUpdArgs); MPSFM_FUSE_CAM=0: k_cam_update
  bool direct;          // ... and, one rank, level-scheduled with inverse accumulators: the slab reduction adds straight into the tiles
                        // of the dense solve, whose first level launch damps (DirectAsm); MPSFM_ASSEMBLE=launch: k_assemble
  bool speculate;       // the host enqueues ahead of an iteration's decision; MPSFM_LM_SPECULATE=0: it waits for every decision
  int force_split;      // MPSFM_LM_SPLIT=0/1: the whole next iteration / only its front half ahead; -1: by the front's measured length
  bool can_split;       // the front half alone may go ahead at all: speculate, one rank, fused_prologue
};
SolveForm solve_form(const mpsfm_ba_handle* h);
SweepArgs sweep_args(mpsfm_ba_handle* h, const SolveForm& f, double radius, const LmCtl* ctl);
// Jacobi column scales from the Jacobian at the current state (Ceres: iteration 0 only)
int prepare_scales(mpsfm_ba_handle* h, const SolveForm& f);
void unit_camtab(mpsfm_ba_handle* h);  // unit camera scales and the camera table at the current state
// the full track sweep in its three launches: dense chunks | reduction of their slabs | general chunks and long tracks, all adding
// into the zeroed reduced buffer (direct: into the tiles of the dense solve); marks (may be NULL): two events recorded between them
int launch_sweeps(mpsfm_ba_handle* h, SweepArgs a, bool direct, hipEvent_t* marks = nullptr);
// one track sweep at the current state: fills the reduced buffer and its scalar tail.  in_loop: as the front of an iteration, where
// the prologue (kernel or f.fused_prologue) zeroes the buffer and single-rank runs reduce the partials with the decision
int run_track_sweep(mpsfm_ba_handle* h, const SolveForm& f, double radius, const LmCtl* ctl, bool in_loop);
void run_assemble(mpsfm_ba_handle* h, double radius, const LmCtl* ctl = nullptr);  // the first launch of run_dense (h->n > 0, not direct)
// f.direct: the track sweep ran in the direct form, A holds the undamped system: no k_assemble, the first level launch damps
int run_dense(mpsfm_ba_handle* h, const SolveForm& f, double radius, const LmCtl* ctl);
// the candidate of a camera step in d_yc: k_cam_update unless f.fused_cam, then the update sweep
void enqueue_update(mpsfm_ba_handle* h, const SolveForm& f, double radius, const LmCtl* ctl);
// the zero fill of the direct form, dealt over the dense sweep's workgroups (SweepArgs::zero_*): camera vectors, y, diag U by column,
// the inverse accumulators the roles write and the live tiles of A
void direct_zero_args(mpsfm_ba_handle* h, SweepArgs& a);

// the single-launch solver's skew hook (mpsfm_debug_local_skew): process-wide like g_dbg_flags, read when a solve is launched
struct LocalSkew { int32_t chunk = 0, mask = 0; int64_t ticks = 0; };
extern LocalSkew g_local_skew;

}  // namespace mpsfm
