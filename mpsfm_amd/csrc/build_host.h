// Host phases of the table build of mpsfm_ba_create (build_host.hip): from the caller's observation lists to the chunked record
// tables, the block pattern of S and the slab reduction tables.  Plain C++ on host threads: no handle, no HIP call, so
// mpsfm_debug_host_build runs them where there is no device.  build_tables() in ba_build.hip is the list of these phases plus the
// device build (devbuild.h), the exchanges over ranks and the uploads.
#pragma once
#include <cstdint>
#include <functional>
#include <vector>

#include "chol_plan.h"
#include "common.h"
#include "host_parts.h"

namespace mpsfm {

// Every MPSFM_* override the build reads, parsed once per build.
struct BuildOptions {
  // false only when the variable is set and equal to 0
  bool dev_build = true, chol_graph = true, sweep_dense = true, chol_inverse = true, chol_envelope = true, local_lm = true;
  bool chol_cuts = true;       // MPSFM_CHOL_CUTS=0: the automatic camera order without the window-separator candidates (chol_plan.h)
  int chol_nd = -2;           // MPSFM_CHOL_ND: -1 caller's order, >= 0 dissection depth; -2: not set
  int slab_tables_host = -1;   // MPSFM_SLAB_TABLES_HOST: 1 host loop, 0 device kernels; -1: not set (by size)
  int chunk_records = 0;       // MPSFM_CHUNK_RECORDS clamped to [16, kObsMax]; 0: not set
  int chunk_pts_by_cams = -1;  // MPSFM_CHUNK_PTS_BY_CAMS as 0 / 1; -1: not set
  int chol_nb = -1, chol_big = -1, chol_overlap = -1, chol_level = -1;  // MPSFM_CHOL_NB (>= 0) / _BIG / _OVERLAP / _LEVEL; -1: not set
  int chol_panel_waves = -1;   // MPSFM_CHOL_PANEL_WAVES: 4 or 1 waves factor a stacked panel; -1: not set
  // derived by set_chunk_caps once the variable cameras are known
  int rec_cap = kObsMax;       // records a DENSE chunk may hold
  int pts_by_cams = 0;         // landmarks of a dense chunk by the size of its camera set (dense_pts_cap)
  static BuildOptions from_environment();
  void set_chunk_caps(bool sharded, int ncv, int64_t n_obs);
  // the tuning / test overrides of the dense factorisation; without MPSFM_CHOL_LEVEL a large reduced system without exploitable
  // structure takes the outer-panel path
  void apply_dense(int nt, const CholPlan& plan, DenseOverlap& ov) const;
};

// sums `count` doubles over the ranks in place, returns 0 or an error code; empty: one rank
typedef std::function<int(double*, int64_t)> SumExchange;
typedef std::function<void(const char*)> Lap;  // build_tables()'s stopwatch (verbose >= 2)
// lap(what) prints `format` (what, milliseconds since the previous lap) when `on`
Lap stopwatch(bool on, const char* format);

// The tables both builds hand to the uploads.  The device build fills the small host members only (chunks, cameras, order, counts).
struct HostTables {
  std::vector<ChunkHdr> chunks;
  std::vector<int32_t> chunk_cams, order;        // order: re-ordered landmark -> caller's index
  HostBuf<int32_t> rec_cam, rec_pt;
  HostBuf<uint32_t> rec_meta;
  HostBuf<double> rec_xy, rec_d, rec_m, rec_a;
  std::vector<int32_t> pt_rec_start;
  std::vector<uint16_t> pt_kv;
  std::vector<int32_t> fx_cam, fx_pt; std::vector<uint32_t> fx_meta; std::vector<double> fx_xy, fx_d, fx_m, fx_a;
  std::vector<uint32_t> blk_desc, ents;          // Schur pairs grouped by destination block, per chunk
  std::vector<int32_t> blk_ent_start;
  std::vector<LongHdr> lhdr;
  int64_t wl_rows = 0;
  int64_t np = 0, np_chunked = 0, n_long = 0, nrec = 0, nfixed = 0, nblk_reduced = 0;  // re-ordered landmarks (all / inside chunks), ...
  double nvarpts = 0;
};

// Which cameras are variable, their slots and the size of the reduced system.
struct CameraLayout {
  std::vector<int32_t> slot;      // camera -> slot; -1: constant or without a block on any rank
  std::vector<int32_t> nat_slot;  // variable camera in the caller's order -> slot
  std::vector<double> cmask;      // [n_cams][6] 1: free coordinate
  int ncv_real = 0;               // variable cameras
  int ncv = 0, n = 0, nt = 0;     // slots, columns (incl. the alignment padding) and tile columns of the reduced system
  bool use_graph = false;         // camera graph (up to kIndexMaxSlots variable cameras): slot order and block index of S from it
};

// Which 6x6 blocks of S exist: the index form (camera graph) or the block skyline.
struct SPattern {
  std::vector<int32_t> sky_index, sky_first;
  std::vector<int64_t> sky_start;
  int64_t nblk = 0;
};

// Slabs of the dense chunks and the tables of their reduction (k_reduce_slabs).
struct SlabTables {
  int n_dense = 0;         // chunks [0, n_dense) are dense
  int64_t slab_units = 0;  // 18-double units of all slabs
  std::vector<RedDest> dests;
  std::vector<int32_t> srcs, diag_block;  // diag_block[slot]: the block of S on that slot's diagonal or -1
  std::vector<int32_t> sweep_order;       // [n_dense] the chunk the b-th workgroup of k_track_sweep_dense takes (dense_sweep_order)
};

struct Rec { int32_t cam; int32_t slot; uint32_t flags; double u, v, d, m, a; };
// The residual blocks of every landmark side by side; every host thread owns a contiguous landmark range.
struct LandmarkGroups {
  struct Part {
    int p0 = 0, p1 = 0, err = 0;
    std::vector<int64_t> pstart;  // block range of every landmark of the part
    HostBuf<Blk> blks;   // recycled, uninitialised blocks (HostBlockCache): a few MB per part
    HostBuf<Rec> recs;   // capacity = the part's blocks (merging only removes); nrecs filled
    size_t nrecs = 0;
    std::vector<Rec> fixed;
    std::vector<int32_t> fixed_pt;
    std::vector<int64_t> nrec_of;  // records per landmark of the range
  };
  std::vector<Part> parts;
};

// -- cameras
void count_camera_blocks(const mpsfm_ba_problem* P, std::vector<double>& cnt);
// slots in the caller's order for the cameras that are not constant and have a block (cnt: blocks per camera over all ranks)
void assign_camera_slots(const mpsfm_ba_problem* P, const std::vector<double>& cnt, const BuildOptions& opt, CameraLayout& cams);
std::vector<int32_t> cam_of_slot_table(const CameraLayout& cams);  // slot -> camera (the fused camera update of k_update_sweep)
// -- blocks grouped by landmark (counting sort per thread part).  check_depths: refuse a depth prior that is not positive
int group_blocks_by_landmark(const mpsfm_ba_problem* P, bool check_depths, LandmarkGroups& G);
// -- camera graph: who shares a variable landmark with whom (caller's slots), and its union over the ranks
void camera_graph_from_groups(const mpsfm_ba_problem* P, const LandmarkGroups& G, const CameraLayout& cams, CamGraph& graph);
int graph_digits(int world);
void pack_graph(const CamGraph& graph, int world, std::vector<double>& packed);
void unpack_graph(const std::vector<double>& packed, int world, CamGraph& graph);
int union_graph_over_ranks(CamGraph& graph, const SumExchange& exchange);
// -- camera order and factorisation plan from the graph; the slots become the plan's
void plan_camera_order(const CamGraph& graph, const BuildOptions& opt, CholPlan& plan, CameraLayout& cams);
void keep_caller_order(CameraLayout& cams);
// -- records, landmark order, chunks, pair tables, long tracks, fixed records: everything of `T` from the groups (released on the way)
int build_record_tables(const mpsfm_ba_problem* P, const CameraLayout& cams, const BuildOptions& opt, LandmarkGroups& G, HostTables& T, const Lap& lap);
// -- block pattern of S: index form from the graph / skyline form from the chunks (with its factorisation plan in the caller's order)
void s_pattern_index(const CameraLayout& cams, const CholPlan& plan, const CamGraph& graph, SPattern& S);
int s_pattern_skyline(const CameraLayout& cams, const HostTables& T, const BuildOptions& opt, const SumExchange& exchange, bool verbose, SPattern& S,
                      CholPlan& plan);
// -- slabs: offsets into the chunk headers, then the reduction tables (tables = false: diag_block only, the device forms the rest)
int assign_slabs(std::vector<ChunkHdr>& chunks, SlabTables& R);
// -- the order in which the dense sweep's workgroups take the chunks: descending dense_sweep_cost (common.h), ties by ascending index
void dense_sweep_order(const std::vector<ChunkHdr>& chunks, int n_dense, std::vector<int32_t>& order);
int slab_reduction_tables(const HostTables& T, const CameraLayout& cams, const CholPlan& plan, const SPattern& S, bool tables, SlabTables& R);

}  // namespace mpsfm
