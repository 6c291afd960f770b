// Creation of a bundle-adjustment handle: the table build (the host phases of build_host.h or the device stages of devbuild.h),
// the uploads, the work buffers and the state.  build_tables() is the list of the build's phases; it knows no handle, so the
// table probe of ba_debug.hip runs the very function mpsfm_ba_create runs.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "ba_handle.h"

namespace mpsfm {

void free_handle(mpsfm_ba_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  // Error returns of the solve (a failing all-reduce hook, a HIP error) and reset_state + destroy leave copies and
  // kernels in flight: h->own waits for both streams before anything goes back to the process-wide caches.
  comm_destroy(h->comm);
  delete h;
}

int check_problem(const mpsfm_ba_problem* P) {
  if (!P) return fail(MPSFM_EINVAL, "problem is NULL");
  if (P->n_cams < 0 || P->n_pts < 0 || P->n_intr < 0 || P->n_obs < 0 || P->n_dobs < 0) return fail(MPSFM_EINVAL, "negative size");
  if (P->n_cams > 0 && (!P->cam_intr_idx || !P->pose_const || !P->cam_intr)) return fail(MPSFM_EINVAL, "camera arrays are NULL");
  if (P->n_pts > 0 && !P->pt_const) return fail(MPSFM_EINVAL, "pt_const is NULL");
  if (P->n_obs > 0 && (!P->obs_cam || !P->obs_pt || !P->obs_xy)) return fail(MPSFM_EINVAL, "observation arrays are NULL");
  if (P->n_dobs > 0 && (!P->dobs_cam || !P->dobs_pt || !P->dobs_depth || !P->dobs_magnitude || !P->dobs_param))
    return fail(MPSFM_EINVAL, "depth observation arrays are NULL");
  if (P->gauge_axis_cam < -1 || P->gauge_axis_cam >= P->n_cams) return fail(MPSFM_EINVAL, "gauge_axis_cam out of range");
  for (int i = 0; i < P->n_cams; ++i)
    if (P->cam_intr_idx[i] < 0 || P->cam_intr_idx[i] >= P->n_intr) return fail(MPSFM_EINVAL, "cam_intr_idx out of range");
  // branch-free sweeps (they vectorise; 7.6 M blocks at C4): an index is in range when it is below the bound as an unsigned number
  auto out_of_range = [](const int32_t* v, int64_t n, int32_t bound) {
    uint32_t bad = 0;
    const uint32_t b = (uint32_t)bound;
    for (int64_t i = 0; i < n; ++i) bad |= (uint32_t)((uint32_t)v[i] >= b);
    return bad != 0;
  };
  if (out_of_range(P->obs_cam, P->n_obs, P->n_cams) || out_of_range(P->obs_pt, P->n_obs, P->n_pts))
    return fail(MPSFM_EINVAL, "observation index out of range");
  if (out_of_range(P->dobs_cam, P->n_dobs, P->n_cams) || out_of_range(P->dobs_pt, P->n_dobs, P->n_pts))
    return fail(MPSFM_EINVAL, "depth observation index out of range");
  for (int t : {P->reproj_loss_type, P->depth_loss_type})
    if (t < MPSFM_LOSS_TRIVIAL || t > MPSFM_LOSS_CAUCHY) return fail(MPSFM_EINVAL, "unknown loss type");
  return 0;
}

void level_plan_flags(const CholPlan& PL, LevelPlanDev& D) { D.valid = PL.nt >= 1 && PL.nlevels >= 1; D.use_pinv = PL.use_pinv; }

// the block pattern of S and the tables of the level-scheduled factorisation (h->spat, h->plan) to the device
static int upload_pattern(mpsfm_ba_handle* h, bool use_graph) {
  const CholPlan& PL = h->plan;
  DeviceBlocks& own = h->own;
  h->sky.ns = h->ncv;
  if (int rc = use_graph ? own.upload(&h->sky.index, h->spat.sky_index) : own.upload(&h->sky.first, h->spat.sky_first, &h->sky.start, h->spat.sky_start))
    return rc;
  std::vector<uint8_t> live((size_t)(PL.nt + 1) * (size_t)(PL.nt + 2) / 2, 0);
  for (int32_t id : PL.asm_tiles) live[(size_t)id] = 1;
  LevelPlanDev& D = h->lp;
  // for the direct form of the front (DirectAsm): the inverse accumulators the roles write, and the columns of the first launch
  std::vector<int32_t> pinv_tiles;
  std::vector<uint8_t> level0((size_t)std::max(PL.nt, 1), 0);
  bool first_is_plain = false;
  {
    std::vector<uint8_t> seen(live.size(), 0);
    for (const CholItem& it : PL.items)
      if (it.type == kItemRole)
        for (uint32_t q = 0; q < it.nsrc; ++q) {
          const int64_t id = lt_tile(PL.rows[(size_t)it.aux + q], it.tk);
          if (!seen[(size_t)id]) { seen[(size_t)id] = 1; pinv_tiles.push_back((int32_t)id); }
        }
    std::sort(pinv_tiles.begin(), pinv_tiles.end());
    for (int l = 0; l + 1 < (int)PL.launch_start.size(); ++l) {
      if (PL.launch_start[(size_t)l + 1] <= PL.launch_start[(size_t)l]) continue;
      first_is_plain = true;  // the first launch that is not empty: panel items without sources only?
      for (int32_t i = PL.launch_start[(size_t)l]; i < PL.launch_start[(size_t)l + 1]; ++i) {
        const CholItem& it = PL.items[(size_t)i];
        if (it.type != kItemPanel || it.nsrc != 0) first_is_plain = false;
        else if (it.ti == it.tk) level0[it.tk] = 1;
      }
      break;
    }
  }
  if (int rc = own.upload(&D.d_items, PL.items, &D.d_heads, PL.heads, &D.d_srcs, PL.srcs, &D.d_rows, PL.rows, &D.d_struct_start, PL.struct_start,
                          &D.d_struct_rows, PL.struct_rows, &D.d_back_cols, PL.back_cols, &D.d_asm_tiles, PL.asm_tiles,
                          &D.d_col_slot, PL.slot_of_col, &D.d_tile_live, live, &D.d_pinv_tiles, pinv_tiles, &D.d_level0, level0))
    return rc;
  D.n_pinv_tiles = (int32_t)pinv_tiles.size(); D.damp_in_launch0 = first_is_plain;
  if (PL.slot_of_col.empty()) D.d_col_slot = nullptr;  // no indirection (the block stays with the handle)
  level_plan_flags(PL, D);
  D.n_asm = (int32_t)PL.asm_tiles.size(); D.nlevels = PL.nlevels;
  D.h_launch_start = PL.launch_start.data(); D.h_back_start = PL.back_start.data();
  return 0;
}

// ---- the table build of mpsfm_ba_create: the phases of build_host.h or the device build (devbuild.h), then the uploads ----------

// the camera graph of the device build's stage 1 in the caller's slots: the device speaks provisional slots (all non-constant
// cameras); cameras without blocks have no slot and no edges
static void graph_from_stage1(const std::vector<uint64_t>& gbits, int words, const std::vector<int32_t>& prov, int nprov, const CameraLayout& cams,
                              CamGraph& graph) {
  graph.init(cams.ncv_real);
  std::vector<int32_t> nat_of_prov((size_t)std::max(nprov, 1), -1);
  for (size_t i = 0; i < cams.slot.size(); ++i) if (prov[i] >= 0) nat_of_prov[(size_t)prov[i]] = cams.slot[i];
  for (int a = 0; a < nprov; ++a) {
    const int na = nat_of_prov[(size_t)a];
    for (int w = 0; w < words; ++w) {
      uint64_t m = gbits[(size_t)a * words + w];
      while (m) {
        const int b = w * 64 + __builtin_ctzll(m);
        m &= m - 1;
        const int nb = nat_of_prov[(size_t)b];
        if (na >= 0 && nb >= 0) graph.set(na, nb);
      }
    }
  }
}

// Pair tables of a device-built handle: a sentinel per dense chunk; the general chunks (landmarks with more than kDenseCams cameras or
// two records of one camera; they come last) get theirs from the host, which needs their record words and landmark tables back
static int pair_tables_of_device_build(hipStream_t stream, const mpsfm_ba_problem* P, const RecTablesDev& rt, HostTables& T, const Lap& lap) {
  std::vector<ChunkHdr>& chunks = T.chunks;
  size_t g0 = 0;
  while (g0 < chunks.size() && chunks[g0].dense) ++g0;
  T.blk_ent_start.assign(g0, 0);
  if (g0 == chunks.size()) return 0;
  const int64_t r0 = chunks[g0].rec0, k0 = chunks[g0].pt0, nrg = T.nrec - r0, nkg = T.np_chunked - k0;
  std::vector<uint32_t> rm((size_t)std::max<int64_t>(nrg, 1));
  std::vector<uint16_t> kvs((size_t)std::max<int64_t>(nkg, 1));
  std::vector<int32_t> prs((size_t)std::max<int64_t>(nkg, 1));
  MPSFM_TRY(hipMemcpyAsync(rm.data(), rt.rec_meta + r0, 4 * (size_t)nrg, hipMemcpyDeviceToHost, stream));
  MPSFM_TRY(hipMemcpyAsync(kvs.data(), rt.pt_kv + k0, 2 * (size_t)nkg, hipMemcpyDeviceToHost, stream));
  MPSFM_TRY(hipMemcpyAsync(prs.data(), rt.pt_rec_start + k0, 4 * (size_t)nkg, hipMemcpyDeviceToHost, stream));
  MPSFM_TRY(hipStreamSynchronize(stream));
  PairScratch ps;
  for (size_t c = g0; c < chunks.size(); ++c) {
    if (chunks[c].dense) return fail(MPSFM_EUNSUPPORTED, "internal: dense chunks must precede the general ones");
    // append_pair_tables indexes by the global record / re-ordered landmark: the copies start at r0 / k0
    append_pair_tables(chunks[c], rm.data() - r0, kvs.data() - k0, prs.data() - k0, T.order.data(), P->pt_const, T.blk_desc, T.ents, T.blk_ent_start, ps);
  }
  if (T.ents.size() > (size_t)INT32_MAX) return fail(MPSFM_EUNSUPPORTED, "too many Schur pairs for 32-bit entry offsets");
  lap("pair tables of the general chunks (host)");
  return 0;
}

static void print_chunk_stats(const std::vector<ChunkHdr>& chunks) {
  double sr = 0, sp = 0, sc = 0, sb = 0, se = 0, sd = 0; int mb = 0, mc = 0;
  for (const ChunkHdr& H : chunks) { sr += H.nrec; sp += H.npt; sc += H.ncam; sb += H.nblk; se += H.nent; sd += H.dense; mb = std::max(mb, H.nblk); mc = std::max(mc, H.ncam); }
  const double n = (double)chunks.size();
  std::fprintf(stderr, "[mpsfm_ba] build: %zu chunks; per chunk: %.1f records, %.1f landmarks, %.1f cameras (max %d), %.1f work items (max %d), %.1f pairs; %.0f %% of the chunks take the dense product\n",
               chunks.size(), sr / n, sp / n, sc / n, mc, sb / n, mb, se / n, 100.0 * sd / n);
  int hist[kDenseCams + 2] = {0};
  for (const ChunkHdr& H : chunks) ++hist[std::min<int>(H.ncam, kDenseCams + 1)];
  std::fprintf(stderr, "[mpsfm_ba] build: chunks by number of variable cameras:");
  for (int c = 0; c <= kDenseCams + 1; ++c) std::fprintf(stderr, " %s%d: %d", c > kDenseCams ? ">" : "", c > kDenseCams ? kDenseCams : c, hist[c]);
  std::fprintf(stderr, "\n");
}

// Everything the solve reads to the device.  `DB`: the device build's output (T is its host part) or, after a host build, empty;
// `devb` forms the slab reduction tables on the device when `R` came without them (R.dests empty, R.diag_block set).
static int upload_tables(mpsfm_ba_handle* h, const mpsfm_ba_problem* P, const CameraLayout& cams, DevBuildOut& DB, SlabTables& R, DevBuilder* devb,
                         bool slab_tables_on_device) {
  HostTables& T = DB.t;
  const int nc = P->n_cams;
  int rc = 0;
  DeviceBlocks& own = h->own;
  std::vector<double> intr(P->cam_intr, P->cam_intr + (size_t)P->n_intr * 4);
  std::vector<int32_t> intr_idx(P->cam_intr_idx, P->cam_intr_idx + nc);
  if ((rc = own.upload(&h->d_intr, intr, &h->d_intr_idx, intr_idx, &h->d_cmask, cams.cmask, &h->d_cam_slot, h->cam_slot_h,
                       &h->d_cam_of_slot, cam_of_slot_table(cams), &h->d_chunks, T.chunks, &h->d_chunk_cams, T.chunk_cams)))
    return rc;
  if (h->np > 0 && h->np == (int64_t)h->np_user) {
    if ((rc = own.upload(&h->d_perm, h->perm))) return rc;
    if ((rc = own.alloc(&h->d_user_pts, (size_t)h->np * 3))) return rc;
  }
  if (h->built_on_device) {  // the device build's tables are where they belong
    h->rt = DB.rt;
    own.adopt(std::move(DB.own));
    own.drop(DB.d_chunks); own.drop(DB.d_chunk_cams);  // the host copies (slab offsets added) are uploaded above; the stream is idle
  } else {  // the host build's record and fixed-record tables
    RecTablesDev& rt = h->rt;
    if ((rc = own.upload(&rt.rec_cam, T.rec_cam, &rt.rec_pt, T.rec_pt, &rt.rec_meta, T.rec_meta, &rt.rec_xy, T.rec_xy, &rt.rec_d, T.rec_d, &rt.rec_m, T.rec_m,
                         &rt.rec_a, T.rec_a, &rt.pt_rec_start, T.pt_rec_start, &rt.pt_kv, T.pt_kv, &rt.fx_cam, T.fx_cam, &rt.fx_pt, T.fx_pt,
                         &rt.fx_meta, T.fx_meta, &rt.fx_xy, T.fx_xy, &rt.fx_d, T.fx_d, &rt.fx_m, T.fx_m, &rt.fx_a, T.fx_a)))
      return rc;
  }
  if ((rc = own.upload(&h->d_lhdr, T.lhdr))) return rc;
  if ((rc = own.alloc(&h->d_wl, (size_t)std::max<int64_t>(T.wl_rows, 1) * 18))) return rc;
  h->n_blk_desc = (int64_t)T.blk_desc.size(); h->n_blk_ent_start = (int64_t)T.blk_ent_start.size(); h->n_ents = (int64_t)T.ents.size();
  if ((rc = own.upload(&h->d_blk_desc, T.blk_desc, &h->d_blk_ent_start, T.blk_ent_start, &h->d_ents, T.ents))) return rc;
  int32_t* d_diag_block = nullptr;
  if (!slab_tables_on_device) {
    if ((rc = own.upload(&h->d_red_dests, R.dests, &h->d_red_srcs, R.srcs, &h->d_sweep_order, R.sweep_order))) return rc;
  } else if ((rc = own.upload(&d_diag_block, R.diag_block))) return rc;
  if ((rc = own.alloc(&h->d_slab, (size_t)std::max<int64_t>(R.slab_units, 1) * 18))) return rc;

  if ((rc = staged_drain())) return rc;
  if (slab_tables_on_device) {
    if ((rc = devb->slab_tables(h->d_chunks, h->n_dense, h->d_chunk_cams, h->sky, h->spat.nblk, h->ncv, d_diag_block, own, &h->d_red_dests, &h->n_red_dests,
                                &h->d_red_srcs, &h->n_red_srcs)))
      return rc;
    if ((rc = devb->sweep_order(h->d_chunks, h->n_dense, own, &h->d_sweep_order))) return rc;
    MPSFM_TRY(hipStreamSynchronize(h->stream));  // d_diag_block goes back to the process-wide cache
    own.drop(d_diag_block);
  }
  return 0;
}

// state, reduced system, dense workspace, scalars, events; the single-launch solver's buffers where it applies
static int alloc_work_buffers(mpsfm_ba_handle* h, const BuildOptions& opt) {
  int rc = 0;
  DeviceBlocks& own = h->own;
  const size_t ncs = (size_t)std::max(h->nc, 1), nps = (size_t)std::max<int64_t>(h->np, 1);
  for (double** p : {&h->d_q, &h->d_q2, &h->d_q0}) if ((rc = own.alloc(p, ncs * 4))) return rc;
  for (double** p : {&h->d_t, &h->d_t2, &h->d_t0}) if ((rc = own.alloc(p, ncs * 3))) return rc;
  for (double** p : {&h->d_pts, &h->d_pts2, &h->d_pts0, &h->d_ps, &h->d_diagV}) if ((rc = own.alloc(p, nps * 3))) return rc;
  // every chunk dense, no long track (fused_prologue's condition in solve_form): the track sweep hands the landmark factors on
  if (all_dense(h)) if ((rc = own.alloc(&h->d_pt_fac, nps * 9))) return rc;
  if ((rc = own.alloc(&h->d_cs, ncs * 6))) return rc;
  if ((rc = own.alloc(&h->d_camtab, ncs * kCamRec))) return rc;
  if ((rc = own.alloc(&h->d_camtab2, ncs * kCamRec))) return rc;
  h->sblk_count = h->spat.nblk * 36;
  h->red_count = h->sblk_count + 3 * (int64_t)h->n_user + SC_COUNT;
  if ((rc = own.alloc(&h->d_red, (size_t)h->red_count))) return rc;
  h->d_Sblk = h->d_red; h->d_gc = h->d_red + h->sblk_count; h->d_wv = h->d_gc + h->n_user; h->d_diagU = h->d_wv + h->n_user;
  h->d_redsc = h->d_diagU + h->n_user;
  if ((rc = own.alloc(&h->d_part, (size_t)std::max(h->nchunks + h->nlong, 1) * 4 * 2))) return rc;  // (second half: the single launch's odd iterations)
  if ((rc = own.alloc(&h->d_part2, (size_t)std::max(h->nchunks + h->nlong, 1) * 8))) return rc;
  if ((rc = own.alloc(&h->d_scal, (size_t)U_COUNT))) return rc;
  if ((rc = own.alloc(&h->d_costpart, (size_t)1024 * 4))) return rc;
  static_assert(sizeof(double) * U_COUNT * 2 <= kPinnedBytes, "pinned scalar block too small");
  MPSFM_TRY(own.pinned((void**)&h->h_scal));
  static_assert(sizeof(LmCtl) * 2 <= kPinnedBytes, "pinned block too small for two control-block copies");
  MPSFM_TRY(own.pinned((void**)&h->h_ctl));
  if ((rc = own.alloc(&h->d_ctl, 1))) return rc;
  for (auto& e : h->ev2) MPSFM_TRY(own.event(&e, true));
  const size_t ntiles = (size_t)(h->nt + 1) * (h->nt + 2) / 2;
  if ((rc = own.alloc(&h->d_A, ntiles * 1024))) return rc;
  if ((rc = own.alloc(&h->d_dwork, dense_work_doubles(h->nt)))) return rc;
  if ((rc = own.alloc(&h->d_yc, (size_t)std::max(h->n_user, 1)))) return rc;
  if ((rc = own.alloc(&h->d_fail, 1))) return rc;
  MPSFM_TRY(hipMemsetAsync(h->d_fail, 0, sizeof(int), h->stream));
  // the inverse accumulators no role writes are zero from here on (LevelPlanDev::d_pinv_tiles)
  if (double* pinv = dense_pinv(h->d_dwork, h->nt, nullptr, nullptr))
    MPSFM_TRY(hipMemsetAsync(pinv, 0, sizeof(double) * (size_t)h->nt * (size_t)(h->nt + 1) / 2 * 1024, h->stream));
  for (auto& e : h->ev) MPSFM_TRY(own.event(&e, true));
  opt.apply_dense(h->nt, h->plan, h->ov);
  if (h->nt > 64 || h->ov.nb > 0) {
    MPSFM_TRY(own.stream(&h->ov.s2));
    for (auto& e : h->ov.evF) MPSFM_TRY(own.event(&e, false));
    for (auto& e : h->ov.evB) MPSFM_TRY(own.event(&e, false));
  }
  // Small problems (local bundle adjustment): the whole trust-region loop in one cooperative launch, one workgroup per chunk
  h->local_ok = false;
  if (opt.local_lm && !sharded(h) && all_dense(h) && h->ncv >= 1 && h->ncv <= kLocalCams &&
      h->n_user == 6 * h->ncv && h->nchunks <= local_lm_max_chunks(h->device)) {
    h->local_log_cap = std::max(h->opt.max_num_iterations, 0) + 2;
    if ((rc = own.alloc(&h->d_local_acc, (size_t)2 * kLocalAccDoubles))) return rc;
    if ((rc = own.alloc(&h->d_local_sync, (size_t)16))) return rc;
    if ((rc = own.alloc(&h->d_local_log, (size_t)h->local_log_cap))) return rc;
    h->local_ok = true;
  }
  MPSFM_TRY(hipMemsetAsync(h->d_ps, 0, nps * 3 * sizeof(double), h->stream));
  MPSFM_TRY(hipMemsetAsync(h->d_yc, 0, (size_t)std::max(h->n_user, 1) * sizeof(double), h->stream));
  MPSFM_TRY(hipStreamSynchronize(h->stream));
  return 0;
}

// ---- where the destinations of the slab reduction land in the tiles of the dense solve (DirectAsm in common.h) ---------------------
// One pass over the block index gives every block of S the first system columns of its two slots; a small kernel then reads them per
// destination part, whichever builder made the destination table (it may exist on the device only).
__global__ __launch_bounds__(256) void k_dest_cols(const RedDest* __restrict__ dests, int ndest, const RedCols* __restrict__ blk_cols,
                                                   const int32_t* __restrict__ col_of_slot, RedDestCols* __restrict__ out) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= ndest) return;
  const RedDest D = dests[w];
  out[w] = RedDestCols{D, D.kind == 2 ? RedCols{col_of_slot[D.dst], 0} : blk_cols[D.dst], {0, 0}};
}
// every chunk dense, no long track, one rank, a level plan (the solve adds the conditions that can change from solve to solve)
static int build_direct_tables(mpsfm_ba_handle* h) {
  if (sharded(h) || !all_dense(h) || !h->lp.valid || !h->lp.damp_in_launch0 || h->n <= 0 || h->n_red_dests <= 0)
    return 0;
  const CholPlan& PL = h->plan;
  std::vector<int32_t> col((size_t)std::max(h->ncv, 1), 0);
  for (int i = 0; i < h->ncv; ++i) col[(size_t)i] = PL.col_of_slot.empty() ? 6 * i : PL.col_of_slot[(size_t)i];
  const BlockSky sky{h->spat.sky_first.data(), h->spat.sky_start.data(), h->spat.sky_index.empty() ? nullptr : h->spat.sky_index.data(), h->ncv};
  std::vector<RedCols> blk_cols((size_t)std::max<int64_t>(h->spat.nblk, 1), RedCols{0, 0});
  for (int j = 0; j < h->ncv; ++j)
    for (int i = sky.index ? 0 : sky.first[j]; i <= j; ++i) {
      if (!sky_has(sky, i, j)) continue;
      const int64_t b = sky_block(sky, i, j);
      if (b < 0 || b >= h->spat.nblk || col[(size_t)i] + 6 > h->n || col[(size_t)j] + 6 > h->n) return fail(MPSFM_EUNSUPPORTED, "internal: block index and plan disagree");
      blk_cols[(size_t)b] = RedCols{col[(size_t)i], col[(size_t)j]};
    }
  RedCols* d_blk_cols = nullptr;
  int32_t* d_col = nullptr;
  DeviceBlocks& own = h->own;
  if (int rc = own.upload(&d_blk_cols, blk_cols, &d_col, col)) return rc;
  if (int rc = staged_drain()) return rc;
  RedDestCols* out = nullptr;
  if (int rc = own.alloc(&out, (size_t)h->n_red_dests)) return rc;
  if (int rc = own.alloc(&h->d_diag_col, (size_t)h->nt * 32)) return rc;
  hipLaunchKernelGGL(k_dest_cols, dim3((h->n_red_dests + 255) / 256), dim3(256), 0, h->stream, h->d_red_dests, h->n_red_dests, d_blk_cols, d_col, out);
  MPSFM_TRY(hipGetLastError());
  MPSFM_TRY(hipStreamSynchronize(h->stream));
  own.drop(d_blk_cols); own.drop(d_col);
  h->d_red_cols = out;
  return 0;
}

// The re-ordered, chunked record tables, the block pattern of S, the factorisation plan and the slab tables: the list of the build's phases.
int build_tables(const mpsfm_ba_problem* P, BuildOptions& opt, const SumExchange& exchange, bool sharded, int verbose, const Lap& lap, DeviceStages* devs,
                 TableBuild& out) {
  const int nc = P->n_cams;
  CameraLayout& cams = out.cams;
  HostTables& T = out.tables.t;  // filled by either build

  // -- Device-side table build (build_dev.hip) where it applies: one rank, at most kIndexMaxSlots non-constant cameras, no
  //    landmark with more blocks than a chunk holds.  Stage 1 runs here (block counts per camera, blocks grouped by landmark,
  //    camera graph); stage 2 then stands in for the host phases.  MPSFM_DEV_BUILD=0: host.
  bool dev = false;
  std::vector<uint64_t> dev_gbits;
  std::vector<int32_t> prov((size_t)std::max(nc, 1), -1);  // provisional slots of the graph stage: the non-constant cameras in order
  int nprov = 0;
  for (int i = 0; i < nc; ++i) if (!P->pose_const[i]) prov[(size_t)i] = nprov++;
  const int dev_words = (nprov + 63) / 64;
  std::vector<double> cnt(nc + 1, 0.0);  // blocks per camera
  if (devs && !sharded && nprov <= kIndexMaxSlots && nc <= 8192 && P->n_obs + P->n_dobs > 0 && opt.dev_build && opt.chol_graph) {
    devs->builder.reset(new DevBuilder());
    int64_t max_blocks = 0;
    if (int rc = devs->builder->stage1(P, devs->stream, prov, nprov, cnt, dev_gbits, dev_words, &max_blocks)) return rc;
    dev = max_blocks <= kObsMax;  // longer block lists may be long tracks: host build
    lap("device stage 1 (upload, group, graph)");
  } else {
    count_camera_blocks(P, cnt);
    if (exchange) if (int rc = exchange(cnt.data(), nc)) return rc;
  }
  assign_camera_slots(P, cnt, opt, cams);
  opt.set_chunk_caps(sharded, cams.ncv, P->n_obs);

  LandmarkGroups groups;
  if (!dev) if (int rc = group_blocks_by_landmark(P, true, groups)) return rc;
  lap("group blocks by landmark (threads)");

  // -- camera order: from the camera graph (summed over the ranks), or the caller's
  CamGraph graph;
  if (cams.use_graph) {
    if (dev) graph_from_stage1(dev_gbits, dev_words, prov, nprov, cams, graph);
    else camera_graph_from_groups(P, groups, cams, graph);
    if (exchange) if (int rc = union_graph_over_ranks(graph, exchange)) return rc;
    lap("camera graph");
    plan_camera_order(graph, opt, out.plan, cams);
    lap("camera order + factorisation plan");
  } else keep_caller_order(cams);

  // -- records, landmark order, chunks, pair tables
  if (dev) {
    const int rc2 = devs->builder->stage2(cams.slot, opt.sweep_dense, opt.rec_cap, opt.pts_by_cams, out.tables);
    if (rc2 < 0) return rc2;
    if (rc2 == MPSFM_DEVBUILD_FALLBACK) {
      // long tracks: the host phases run after all — the grouping first, which was skipped (depths were validated by stage 1)
      dev = false;
      if (int rc = group_blocks_by_landmark(P, false, groups)) return rc;
      lap("device build not applicable: host phases");
    } else {
      if (T.nrec > (int64_t)INT32_MAX) return fail(MPSFM_EUNSUPPORTED, "more than 2^31 records on one device");
      lap("device stage 2 (order, chunks, records)");
      if (int rc = pair_tables_of_device_build(devs->stream, P, out.tables.rt, T, lap)) return rc;
    }
  }
  if (!dev) if (int rc = build_record_tables(P, cams, opt, groups, T, lap)) return rc;
  out.built_on_device = dev;
  {
    double tot[3] = {(double)(P->n_obs + P->n_dobs), (double)T.nblk_reduced, T.nvarpts};
    if (exchange) if (int rc = exchange(tot, 3)) return rc;
    out.nblocks_global = tot[0]; out.nblocks_reduced_global = tot[1]; out.nvarpts_global = tot[2];
  }
  lap("chunks + pair tables");
  if (verbose >= 2 && !T.chunks.empty()) print_chunk_stats(T.chunks);

  // -- which 6x6 blocks of S exist, and the tables of the dense factorisation
  if (cams.use_graph) s_pattern_index(cams, out.plan, graph, out.spat);
  else if (int rc = s_pattern_skyline(cams, T, opt, exchange, verbose >= 2, out.spat, out.plan)) return rc;
  if (verbose >= 2) {
    const CholPlan& PL = out.plan;
    std::fprintf(stderr, "[mpsfm_ba] build: camera order: %s (depth %d), %d slots for %d cameras, %d tile columns in %d levels, %lld tile products, %lld inverse roles, %d blocks of S\n",
                 PL.nd_depth < 0 ? "caller's" : "nested dissection", PL.nd_depth, PL.nslots, PL.ncv, PL.nt, PL.nlevels, (long long)PL.products, (long long)PL.roles, (int)out.spat.nblk);
  }

  // -- slabs of the dense chunks and the tables of their reduction; a device-built handle forms the tables on the device too
  //    (DevBuilder::slab_tables, behind the uploads).  MPSFM_SLAB_TABLES_HOST 1: host loop, 0: device kernels (tests), unset: by
  //    size — below ~500 chunks the host loop is quicker than the launches
  SlabTables& slabs = out.slabs;
  if (int rc = assign_slabs(T.chunks, slabs)) return rc;
  out.slab_tables_on_device = dev && slabs.n_dense > 0 && (opt.slab_tables_host == 0 || (opt.slab_tables_host < 0 && slabs.n_dense >= 512));
  if (int rc = slab_reduction_tables(T, cams, out.plan, out.spat, !out.slab_tables_on_device, slabs)) return rc;
  if (!out.slab_tables_on_device) dense_sweep_order(T.chunks, slabs.n_dense, slabs.sweep_order);  // (otherwise DevBuilder::sweep_order, with the tables)
  lap("slab reduction tables");
  return 0;
}

// The tables of `P` into the handle: build them, keep the plan and the pattern, copy the sizes, upload and allocate.
static int build(mpsfm_ba_handle* h, const mpsfm_ba_problem* P) {
  const Lap lap = stopwatch(h->opt.verbose >= 2, "[mpsfm_ba] build: %-28s %8.2f ms\n");
  h->nc = P->n_cams; h->np_user = P->n_pts;
  h->loss.reproj_type = P->reproj_loss_type; h->loss.reproj_a = P->reproj_loss_scale;
  h->loss.reproj_mag = P->reproj_loss_magnitude; h->loss.depth_type = P->depth_loss_type;
  BuildOptions opt = BuildOptions::from_environment();
  // the exchanges of a landmark-sharded build (block counts, graph union, totals, skyline bisection) sum host values over the ranks
  const SumExchange exchange = sharded(h) ? SumExchange([h](double* buf, int64_t count) { return allreduce_host(h, buf, count); }) : SumExchange();
  DeviceStages devs{h->stream, nullptr};
  TableBuild B;
  if (int rc = build_tables(P, opt, exchange, sharded(h), h->opt.verbose, lap, &devs, B)) return rc;

  h->plan = std::move(B.plan); h->spat = std::move(B.spat);
  const CameraLayout& cams = B.cams;
  HostTables& T = B.tables.t;
  h->n_user = 6 * cams.ncv_real;
  h->cam_slot_h = cams.slot; h->nat_slot = cams.nat_slot;
  h->ncv = cams.ncv; h->n = cams.n; h->nt = cams.nt;
  h->built_on_device = B.built_on_device;
  h->np = T.np; h->np_chunked = T.np_chunked; h->nfixed = T.nfixed; h->nrec = T.nrec;
  h->nchunks = (int)T.chunks.size(); h->nlong = (int)T.lhdr.size();
  h->nblocks_total = P->n_obs + P->n_dobs; h->nblocks_reduced = T.nblk_reduced;
  h->nblocks_global = B.nblocks_global; h->nblocks_reduced_global = B.nblocks_reduced_global; h->nvarpts_global = B.nvarpts_global;
  h->n_dense = B.slabs.n_dense; h->n_red_dests = (int)B.slabs.dests.size();
  h->n_red_srcs = (int64_t)B.slabs.srcs.size(); h->slab_units = B.slabs.slab_units; h->n_chunk_cams = (int64_t)T.chunk_cams.size();
  h->perm.swap(T.order);

  if (int rc = upload_pattern(h, cams.use_graph)) return rc;
  if (int rc = upload_tables(h, P, cams, B.tables, B.slabs, devs.builder.get(), B.slab_tables_on_device)) return rc;
  lap("upload tables");
  if (int rc = alloc_work_buffers(h, opt)) return rc;
  lap("allocate work buffers");
  if (int rc = build_direct_tables(h)) return rc;
  lap("direct assembly tables");
  return 0;
}

int upload_state(mpsfm_ba_handle* h, const mpsfm_ba_state* st, bool as_initial) {
  if (!st || (h->nc > 0 && (!st->cam_quat_xyzw || !st->cam_t)) || (h->np > 0 && !st->pts)) return fail(MPSFM_EINVAL, "state is NULL");
  const Lap lap = stopwatch(h->opt.verbose >= 2, "[mpsfm_ba] state: %-28s %8.2f ms\n");
  // caller memory is pageable: staged copies (see Stager).  The handle's stream is idle between solves.
  MPSFM_TRY(hipStreamSynchronize(h->stream));
  lap("stream idle");
  if (h->nc > 0) {
    if (int rc = staged_h2d(h->d_q, st->cam_quat_xyzw, sizeof(double) * 4 * h->nc)) return rc;
    if (int rc = staged_h2d(h->d_t, st->cam_t, sizeof(double) * 3 * h->nc)) return rc;
  }
  lap("pose copies");
  if (h->d_perm) {  // every landmark is referenced: the caller's array as it is, re-ordered on the device
    if (int rc = staged_h2d(h->d_user_pts, st->pts, sizeof(double) * 3 * h->np)) return rc;
    launch_permute_pts(h->np, h->d_perm, h->d_user_pts, h->d_pts, false, h->stream);
    lap("landmark copy + permute (device)");
  } else {
    std::vector<double> sorted((size_t)h->np * 3);
    parallel_ranges(h->np, 16384, [&](int64_t k0, int64_t k1) {
      for (int64_t k = k0; k < k1; ++k) {
        const double* s = st->pts + 3 * (size_t)h->perm[(size_t)k];
        sorted[3 * (size_t)k] = s[0]; sorted[3 * (size_t)k + 1] = s[1]; sorted[3 * (size_t)k + 2] = s[2];
      }
    });
    lap("permute landmarks");
    if (h->np > 0) if (int rc = staged_h2d(h->d_pts, sorted.data(), sizeof(double) * 3 * h->np)) return rc;
  }
  lap("landmark copy");
  if (as_initial) {
    MPSFM_TRY(hipMemcpyAsync(h->d_q0, h->d_q, sizeof(double) * 4 * h->nc, hipMemcpyDeviceToDevice, h->stream));
    MPSFM_TRY(hipMemcpyAsync(h->d_t0, h->d_t, sizeof(double) * 3 * h->nc, hipMemcpyDeviceToDevice, h->stream));
    if (h->np > 0) MPSFM_TRY(hipMemcpyAsync(h->d_pts0, h->d_pts, sizeof(double) * 3 * h->np, hipMemcpyDeviceToDevice, h->stream));
    MPSFM_TRY(hipStreamSynchronize(h->stream));
    lap("keep initial state");
  }
  h->scales_ready = false;
  return 0;
}

int create_impl(const mpsfm_ba_problem* P, const mpsfm_ba_state* st, const mpsfm_ba_options* o, mpsfm_ba_handle** out) {
  if (!out) return fail(MPSFM_EINVAL, "out is NULL");
  *out = nullptr;
  const auto t_begin = std::chrono::steady_clock::now();
  auto since = [&](const char* what) {
    if (o && o->verbose >= 2)
      std::fprintf(stderr, "[mpsfm_ba] create: %-27s %8.2f ms (cumulative)\n", what,
                   1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count());
  };
  if (int rc = check_problem(P)) return rc;
  if (!o) return fail(MPSFM_EINVAL, "options is NULL");
  since("check_problem");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(MPSFM_ENODEVICE, "no HIP device visible: libmpsfm_hip has no CPU fallback");
  if (o->device < 0 || o->device >= ndev) return fail(MPSFM_EINVAL, "device ordinal out of range");
  if (o->device >= kMaxDevices) return fail(MPSFM_EUNSUPPORTED, "device ordinals beyond 15 are not supported (per-device pools)");
  {
    // the architecture of a device does not change: query it once per process and device
    static std::mutex mu;
    static std::vector<std::string> arch;
    std::lock_guard<std::mutex> lk(mu);
    if ((int)arch.size() < ndev) arch.resize((size_t)ndev);
    if (arch[(size_t)o->device].empty()) {
      hipDeviceProp_t prop;
      MPSFM_TRY(hipGetDeviceProperties(&prop, o->device));
      arch[(size_t)o->device] = prop.gcnArchName;
    }
    if (std::strncmp(arch[(size_t)o->device].c_str(), "gfx950", 6) != 0)
      return fail(MPSFM_ENODEVICE, std::string("device is ") + arch[(size_t)o->device] + ", this library is built for gfx950 only");
  }
  since("device check");
  MPSFM_TRY(hipSetDevice(o->device));
  mpsfm_ba_handle* h = new mpsfm_ba_handle();
  h->device = o->device; h->opt = *o;
  if (o->stream) { h->stream = (hipStream_t)o->stream; h->own.idle_first(h->stream); }
  else if (h->own.stream(&h->stream) != hipSuccess) { delete h; return fail(MPSFM_EHIP, "hipStreamCreate failed"); }
  if (o->use_rccl && o->world_size >= 1) {
    if (int rc = comm_init_rank(h)) { free_handle(h); return rc; }
    since("ncclCommInitRank");
  }
  int rc = build(h, P);
  since("build");
  if (rc == 0 && st) rc = upload_state(h, st, true);
  since("upload_state");
  if (rc) { free_handle(h); return rc; }
  *out = h;
  return 0;
}

}  // namespace mpsfm
