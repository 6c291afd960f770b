// Device-side table build (build_dev.hip): the stages build_tables() in ba_build.hip runs in place of the host phases of build_host.h.
#pragma once
#include <cstdint>
#include <vector>

#include "build_host.h"
#include "common.h"
#include "dev_resources.h"

namespace mpsfm {

constexpr int MPSFM_DEVBUILD_FALLBACK = 1;  // stage2: the problem needs the host build (long tracks); nothing was produced

// The record and fixed-record tables on the device: built there by the device build, uploaded by the host build.  A view: the blocks
// belong to a DeviceBlocks (the build's output, then the handle).
struct RecTablesDev {
  int32_t *rec_cam = nullptr, *rec_pt = nullptr;
  uint32_t* rec_meta = nullptr;
  double *rec_xy = nullptr, *rec_d = nullptr, *rec_m = nullptr, *rec_a = nullptr;
  int32_t* pt_rec_start = nullptr;
  uint16_t* pt_kv = nullptr;
  // fixed blocks (constant camera and constant landmark)
  int32_t *fx_cam = nullptr, *fx_pt = nullptr;
  uint32_t* fx_meta = nullptr;
  double *fx_xy = nullptr, *fx_d = nullptr, *fx_m = nullptr, *fx_a = nullptr;
};

struct DevBuildOut {
  DeviceBlocks own;  // the device tables below; it waits for the builder's stream
  ChunkHdr* d_chunks = nullptr;
  int32_t* d_chunk_cams = nullptr;
  RecTablesDev rt;
  // host copies of the small tables the rest of build_tables() works on: chunks, chunk_cams, order and the counts
  HostTables t;
};

class DevBuilder {
 public:
  DevBuilder();
  ~DevBuilder();
  DevBuilder(const DevBuilder&) = delete;
  DevBuilder& operator=(const DevBuilder&) = delete;
  // uploads the observation lists, groups the blocks by landmark, returns the blocks per camera, the camera graph over the caller's
  // ("natural") slots and the longest block list of a landmark
  int stage1(const mpsfm_ba_problem* P, hipStream_t stream, const std::vector<int32_t>& nat_slot, int ncv_real, std::vector<double>& cam_counts,
             std::vector<uint64_t>& graph_bits, int graph_words, int64_t* max_blocks_per_landmark);
  // with the final camera slots: landmark order, chunk cut, record arrays.  Returns 0, MPSFM_DEVBUILD_FALLBACK or an error code.
  // rec_cap: records a DENSE chunk may hold (kObsMax, or less for small problems); pts_by_cams: dense_pts_cap by the camera set (BuildOptions)
  int stage2(const std::vector<int32_t>& slot_of_cam, bool dense_on, int rec_cap, int pts_by_cams, DevBuildOut& out);
  // the reduction tables of the dense chunks' slabs (k_reduce_slabs) from device copies of the chunk headers (slab offsets set) and
  // camera lists; d_diag_block[slot]: the block of S on that slot's diagonal or -1.  The two tables are allocated from `own`;
  // stage1 must have run (the builder's stream).
  int slab_tables(const ChunkHdr* d_chunks, int n_dense, const int32_t* d_chunk_cams, const BlockSky& sky, int64_t nsb, int ncv, const int32_t* d_diag_block,
                  DeviceBlocks& own, RedDest** d_dests, int32_t* n_dests, int32_t** d_srcs, int64_t* n_srcs);
  // the order table of the dense sweep (SweepArgs::order: chunks by descending dense_sweep_cost, ties by ascending index) from the
  // device copy of the chunk headers, [n_dense] from `own`; enqueued on the builder's stream (stage1 must have run)
  int sweep_order(const ChunkHdr* d_chunks, int n_dense, DeviceBlocks& own, int32_t** d_order);

 private:
  struct Impl;
  Impl* m;
};

}  // namespace mpsfm
