// Host phases of the table build (build_host.h): plain C++ on host threads, no HIP call.
#include "build_host.h"

#include "ba_launch.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iterator>
#include <numeric>

#include <pthread.h>
#include <sched.h>

namespace mpsfm {

Lap stopwatch(bool on, const char* format) {
  return [on, format, t_prev = std::chrono::steady_clock::now()](const char* what) mutable {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, format, what, 1e3 * std::chrono::duration<double>(now - t_prev).count());
    t_prev = now;
  };
}

// ---- host threads and recycled host blocks (host_parts.h) ------------------------------------------------------------------
HostBlockCache& host_cache() { static HostBlockCache c; return c; }

int host_threads() {
  static const int n = [] {
    if (const char* e = std::getenv("MPSFM_HOST_THREADS")) { const int v = std::atoi(e); if (v > 0) return std::min(v, 64); }
    int cpus = 1;
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) cpus = std::max(1, CPU_COUNT(&set));
    if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
      char a[64]; double per = 0.0;
      if (std::fscanf(f, "%63s %lf", a, &per) == 2 && std::strcmp(a, "max") != 0 && per > 0.0)
        cpus = std::min(cpus, std::max(1, (int)(std::atof(a) / per + 0.5)));
      std::fclose(f);
    }
    return std::min(cpus, 32);
  }();
  return n;
}
static std::atomic<HostPool*> g_host_pool{nullptr};
HostPool* host_pool() {
  static std::once_flag once;
  std::call_once(once, [] {
    pthread_atfork(nullptr, nullptr, [] { g_host_pool.store(nullptr); });  // child: the old pool is abandoned, never destroyed
    std::atexit([] { delete g_host_pool.exchange(nullptr); });
  });
  HostPool* p = g_host_pool.load(std::memory_order_acquire);
  if (!p) {
    HostPool* fresh = new HostPool();
    if (g_host_pool.compare_exchange_strong(p, fresh)) p = fresh; else delete fresh;
  }
  return p;
}
bool host_pool_enabled() {
  static const bool use_pool = !(std::getenv("MPSFM_HOST_POOL") && std::atoi(std::getenv("MPSFM_HOST_POOL")) == 0);
  return use_pool;
}

void append_pair_tables(ChunkHdr& H, const uint32_t* rec_meta, const uint16_t* pt_kv, const int32_t* pt_rec_start, const int32_t* order,
                        const uint8_t* pt_const, std::vector<uint32_t>& o_blk_desc, std::vector<uint32_t>& o_ents, std::vector<int32_t>& o_blk_ent_start,
                        PairScratch& S) {
  std::vector<PairEnt>&pe = S.pe, &pe_sorted = S.pe_sorted;
  std::vector<std::pair<int, int>>&blk_order = S.blk_order, &items = S.items;
  std::vector<int32_t>& cnt = S.cnt;
  const int64_t c_first = H.pt0, end_pt = (int64_t)H.pt0 + H.npt;
  pe.clear();
  if (!H.dense) {
    for (int64_t k = c_first; k < end_pt; ++k) {
      const int p = order[k];
      if (pt_const[p]) continue;
      // Schur pairs of this landmark: records rbase .. rbase+kv-1 have variable cameras (slot-sorted)
      const int rbase = pt_rec_start[(size_t)k] - H.rec0;
      const int kv = (int)pt_kv[(size_t)k];
      const uint32_t lpt = (uint32_t)(k - c_first);
      for (int i = 0; i < kv; ++i) {
        const uint32_t li = rec_meta[(size_t)H.rec0 + rbase + i] & 0xff;
        for (int j = i; j < kv; ++j) {
          const uint32_t lj = rec_meta[(size_t)H.rec0 + rbase + j] & 0xff;
          pe.push_back(PairEnt{(uint16_t)(li | (lj << 8)), (uint32_t)(rbase + i) | ((uint32_t)(rbase + j) << 8) | (lpt << 16)});
          // two records of one camera: the diagonal block needs B + B^T
          if (li == lj && i != j)
            pe.push_back(PairEnt{(uint16_t)(li | (lj << 8)), (uint32_t)(rbase + j) | ((uint32_t)(rbase + i) << 8) | (lpt << 16)});
        }
      }
    }
  }
  // group the pairs by destination block (counting sort on li*ncam+lj); heaviest blocks first
  {
    const int nl = std::max(H.ncam, 1);
    cnt.assign((size_t)nl * nl + 1, 0);
    for (const PairEnt& e : pe) cnt[(size_t)(e.key & 0xff) * nl + (e.key >> 8) + 1]++;
    for (size_t q = 1; q < cnt.size(); ++q) cnt[q] += cnt[q - 1];
    pe_sorted.resize(pe.size());
    for (const PairEnt& e : pe) pe_sorted[(size_t)cnt[(size_t)(e.key & 0xff) * nl + (e.key >> 8)]++] = e;
    pe.swap(pe_sorted);
  }
  blk_order.clear();
  for (size_t i = 0; i < pe.size();) {
    size_t j = i;
    while (j < pe.size() && pe[j].key == pe[i].key) ++j;
    blk_order.emplace_back((int)(j - i), (int)i);
    i = j;
  }
  std::stable_sort(blk_order.begin(), blk_order.end(), [](const std::pair<int, int>& x, const std::pair<int, int>& y) { return x.first > y.first; });
  // work items: runs of at most kItemPairs pairs of one block.  Block-major: all items of a block are
  // neighbours, so the flush combines them (one atomic pass per block and round)
  items.clear();
  for (const auto& bo : blk_order)
    for (int q = 0; q < bo.first; q += kItemPairs) items.emplace_back(std::min(kItemPairs, bo.first - q), bo.second + q);
  H.blk0 = (int32_t)o_blk_desc.size();  // thread-local for now
  H.ent0 = (int32_t)o_ents.size();
  H.nent = (int32_t)pe.size();
  H.nblk = (int32_t)items.size();
  for (const auto& it : items) {
    o_blk_desc.push_back(pe[(size_t)it.second].key);
    o_blk_ent_start.push_back((int32_t)(o_ents.size() - (size_t)H.ent0));
    for (int q = 0; q < it.first; ++q) o_ents.push_back(pe[(size_t)(it.second + q)].ent);
  }
  o_blk_ent_start.push_back((int32_t)(o_ents.size() - (size_t)H.ent0));  // per-chunk sentinel
}

// ---- options ------------------------------------------------------------------------------------------------------------------
BuildOptions BuildOptions::from_environment() {
  BuildOptions o;
  auto off = [](const char* name) { const char* e = std::getenv(name); return e && std::atoi(e) == 0; };  // set and equal to 0
  auto read = [](const char* name, int& v) { const char* e = std::getenv(name); if (e) v = std::atoi(e); return e != nullptr; };
  o.dev_build = !off("MPSFM_DEV_BUILD"); o.chol_graph = !off("MPSFM_CHOL_GRAPH"); o.sweep_dense = !off("MPSFM_SWEEP_DENSE");
  o.chol_inverse = !off("MPSFM_CHOL_INVERSE"); o.chol_envelope = !off("MPSFM_CHOL_ENVELOPE"); o.local_lm = !off("MPSFM_LOCAL_LM");
  read("MPSFM_CHOL_ND", o.chol_nd); o.chol_cuts = !off("MPSFM_CHOL_CUTS");
  read("MPSFM_SLAB_TABLES_HOST", o.slab_tables_host);
  if (read("MPSFM_CHUNK_RECORDS", o.chunk_records)) o.chunk_records = std::min(std::max(o.chunk_records, 16), (int)kObsMax);
  if (read("MPSFM_CHUNK_PTS_BY_CAMS", o.chunk_pts_by_cams)) o.chunk_pts_by_cams = o.chunk_pts_by_cams != 0;
  if (read("MPSFM_CHOL_NB", o.chol_nb)) o.chol_nb = std::max(0, o.chol_nb);
  if (read("MPSFM_CHOL_BIG", o.chol_big)) o.chol_big = o.chol_big != 0;
  if (read("MPSFM_CHOL_OVERLAP", o.chol_overlap)) o.chol_overlap = o.chol_overlap != 0;
  if (read("MPSFM_CHOL_LEVEL", o.chol_level)) o.chol_level = o.chol_level != 0;
  if (read("MPSFM_CHOL_PANEL_WAVES", o.chol_panel_waves)) o.chol_panel_waves = o.chol_panel_waves == 1 ? 1 : 4;
  return o;
}
// Records a DENSE chunk may hold.  A very small problem (a local bundle adjustment of a few cameras: a handful of full chunks) is
// cut into ~40 smaller ones: every sweep costs ONE workgroup's latency, which grows with the chunk's landmarks — measured in the
// single launch of local_lm.hip: 3 cameras / 300 landmarks 39 -> 34 us per iteration with 24 chunks instead of 6; beyond ~40
// chunks its grid barriers (~35 ns per workgroup each) take back what the sweep gains.  MPSFM_CHUNK_RECORDS overrides.
// landmarks of a dense chunk by the size of its camera set (dense_pts_cap): small problems, MPSFM_CHUNK_PTS_BY_CAMS overrides
void BuildOptions::set_chunk_caps(bool sharded, int ncv, int64_t n_obs) {
  const bool small = !sharded && ncv >= 1 && ncv <= kLocalCams;
  pts_by_cams = chunk_pts_by_cams >= 0 ? chunk_pts_by_cams : (small ? 1 : 0);
  rec_cap = kObsMax;
  constexpr int64_t kSmallChunks = 40;
  if (chunk_records > 0) rec_cap = chunk_records;
  else if (small && n_obs < kSmallChunks * kObsMax)
    rec_cap = (int)std::min<int64_t>(kObsMax, std::max<int64_t>(64, (n_obs + kSmallChunks - 1) / kSmallChunks));
}
void BuildOptions::apply_dense(int nt, const CholPlan& plan, DenseOverlap& ov) const {
  if (chol_nb >= 0) ov.nb = chol_nb;
  if (chol_big >= 0) ov.big = chol_big != 0;
  if (chol_overlap >= 0) ov.overlap = chol_overlap != 0;
  ov.no_inverse = !chol_inverse;
  if (chol_panel_waves >= 0) ov.panel_waves = chol_panel_waves;
  if (chol_level >= 0) ov.no_level = chol_level == 0;
  // a large reduced system without exploitable structure (every camera shares landmarks with most others): the
  // outer-panel path with its LDS-staged 64x64 trailing update moves fewer bytes per flop than one workgroup per tile
  else if (nt > dense_plain_max_tiles() && (double)plan.products > 0.5 * (double)nt * nt * nt / 6.0) ov.no_level = true;
}

// ---- cameras ------------------------------------------------------------------------------------------------------------------
void count_camera_blocks(const mpsfm_ba_problem* P, std::vector<double>& cnt) {
  for (int64_t i = 0; i < P->n_obs; ++i) cnt[P->obs_cam[i]] += 1.0;
  for (int64_t i = 0; i < P->n_dobs; ++i) cnt[P->dobs_cam[i]] += 1.0;
}
// cameras of the reduced program: not constant and referenced by a residual block (any shard)
void assign_camera_slots(const mpsfm_ba_problem* P, const std::vector<double>& cnt, const BuildOptions& opt, CameraLayout& cams) {
  const int nc = P->n_cams;
  cams.slot.assign(nc, -1);
  cams.cmask.assign((size_t)nc * 6, 0.0);
  cams.ncv = 0;
  for (int i = 0; i < nc; ++i) {
    if (P->pose_const[i] || cnt[i] == 0.0) continue;
    cams.slot[i] = cams.ncv++;
    for (int k = 0; k < 6; ++k) cams.cmask[(size_t)i * 6 + k] = 1.0;
    if (i == P->gauge_axis_cam) cams.cmask[(size_t)i * 6 + 3] = 0.0;
  }
  cams.ncv_real = cams.ncv;
  cams.n = 6 * cams.ncv;
  cams.nt = (cams.n + 31) / 32;
  cams.use_graph = cams.ncv_real > 0 && cams.ncv_real <= kIndexMaxSlots && opt.chol_graph;
}

std::vector<int32_t> cam_of_slot_table(const CameraLayout& cams) {
  std::vector<int32_t> cam_of_slot((size_t)std::max(cams.ncv, 1), 0);
  for (size_t i = 0; i < cams.slot.size(); ++i) if (cams.slot[i] >= 0 && cams.slot[i] < cams.ncv) cam_of_slot[(size_t)cams.slot[i]] = (int32_t)i;
  return cam_of_slot;
}

// ---- blocks grouped by landmark -----------------------------------------------------------------------------------------------
// Phase A (host threads over landmark ranges): the blocks of every landmark side by side (counting sort).
int group_blocks_by_landmark(const mpsfm_ba_problem* P, bool check_depths, LandmarkGroups& G) {
  const int npu = P->n_pts;
  const int mparts = (int)std::max<int64_t>(1, std::min<int64_t>(host_threads(), (P->n_obs + P->n_dobs) / 32768));  // starting threads only pays above ~100 k blocks
  G.parts = std::vector<LandmarkGroups::Part>((size_t)mparts);
  run_parts(mparts, [&](int t, int nparts) {
    LandmarkGroups::Part& M = G.parts[(size_t)t];
    M.p0 = (int)((int64_t)npu * t / nparts); M.p1 = (int)((int64_t)npu * (t + 1) / nparts);
    const int p0 = M.p0, np_loc = M.p1 - M.p0;
    std::vector<int64_t>& pstart = M.pstart;
    pstart.assign((size_t)np_loc + 1, 0);
    for (int64_t i = 0; i < P->n_obs; ++i) { const unsigned q = (unsigned)(P->obs_pt[i] - p0); if (q < (unsigned)np_loc) pstart[q + 1]++; }
    for (int64_t i = 0; i < P->n_dobs; ++i) { const unsigned q = (unsigned)(P->dobs_pt[i] - p0); if (q < (unsigned)np_loc) pstart[q + 1]++; }
    for (int q = 0; q < np_loc; ++q) pstart[q + 1] += pstart[q];
    M.blks.alloc((size_t)pstart[np_loc]);
    std::vector<int64_t> fill(pstart.begin(), pstart.end() - 1);
    for (int64_t i = 0; i < P->n_obs; ++i) {
      const unsigned q = (unsigned)(P->obs_pt[i] - p0);
      if (q >= (unsigned)np_loc) continue;
      M.blks[(size_t)fill[q]++] = Blk{P->obs_cam[i], 0, 0, i};
    }
    for (int64_t i = 0; i < P->n_dobs; ++i) {
      const unsigned q = (unsigned)(P->dobs_pt[i] - p0);
      if (q >= (unsigned)np_loc) continue;
      if (check_depths && !(P->dobs_depth[i] > 0.0)) { M.err = 1; return; }
      M.blks[(size_t)fill[q]++] = Blk{P->dobs_cam[i], 0, 1, i};
    }
  });
  for (const LandmarkGroups::Part& M : G.parts)
    if (M.err == 1) return fail(MPSFM_EINVAL, "depth prior must be positive");
  return 0;
}

// ---- camera graph -------------------------------------------------------------------------------------------------------------
void camera_graph_from_groups(const mpsfm_ba_problem* P, const LandmarkGroups& G, const CameraLayout& cams, CamGraph& graph) {
  const std::vector<int32_t>& slot = cams.slot;
  const int mparts = (int)G.parts.size();
  graph.init(cams.ncv_real);
  std::vector<std::vector<uint64_t>> gb((size_t)mparts);
  run_parts(mparts, [&](int t, int) {
    const LandmarkGroups::Part& M = G.parts[(size_t)t];
    std::vector<uint64_t>& B = gb[(size_t)t];
    B.assign(graph.bits.size(), 0);
    std::vector<int32_t> sl;
    for (int q = 0; q < M.p1 - M.p0; ++q) {
      if (P->pt_const[M.p0 + q]) continue;
      sl.clear();
      for (int64_t r = M.pstart[(size_t)q]; r < M.pstart[(size_t)q + 1]; ++r) {
        const int sc = slot[(size_t)M.blks[(size_t)r].cam];
        if (sc >= 0 && std::find(sl.begin(), sl.end(), sc) == sl.end()) sl.push_back(sc);  // a handful of cameras per landmark
      }
      for (size_t a = 0; a < sl.size(); ++a)
        for (size_t b = a + 1; b < sl.size(); ++b) {
          B[(size_t)sl[a] * graph.words + (sl[b] >> 6)] |= 1ull << (sl[b] & 63);
          B[(size_t)sl[b] * graph.words + (sl[a] >> 6)] |= 1ull << (sl[a] & 63);
        }
    }
  });
  for (const auto& B : gb) for (size_t w = 0; w < B.size(); ++w) graph.bits[w] |= B[w];
}

// The camera graph of a landmark-sharded run is the UNION over the ranks, and the exchange can only SUM doubles: every rank
// packs its adjacency bits as indicator digits in base (world + 1), E digits per double (E chosen so that a sum of `world`
// such numbers stays below 2^53, i.e. exact), the packed vectors are summed, and a digit > 0 means "some rank has the edge".
int graph_digits(int world) {
  int E = 1;
  double cap = 9007199254740992.0 / (world + 1);
  while (cap >= (world + 1) && E < 16) { cap /= (world + 1); ++E; }
  return E;
}
void pack_graph(const CamGraph& graph, int world, std::vector<double>& packed) {
  const int E = graph_digits(world), n = graph.n;
  const int64_t nbits = (int64_t)n * n;
  packed.assign((size_t)((nbits + E - 1) / E), 0.0);
  double pw[16];
  pw[0] = 1.0;
  for (int e = 1; e < 16; ++e) pw[e] = pw[e - 1] * (double)(world + 1);
  for (int a = 0; a < n; ++a) {
    const uint64_t* row = graph.row(a);
    for (int w = 0; w < graph.words; ++w) {
      uint64_t m = row[w];
      while (m) {
        const int64_t q = (int64_t)a * n + (w * 64 + __builtin_ctzll(m));
        m &= m - 1;
        packed[(size_t)(q / E)] += pw[q % E];
      }
    }
  }
}
void unpack_graph(const std::vector<double>& packed, int world, CamGraph& graph) {
  const int E = graph_digits(world), n = graph.n;
  const int64_t nbits = (int64_t)n * n;
  for (size_t w = 0; w < packed.size(); ++w) {
    double v = packed[w];
    for (int e = 0; e < E && v > 0.0; ++e) {
      const double d = std::fmod(v, (double)(world + 1));
      v = std::floor(v / (world + 1));
      const int64_t q = (int64_t)w * E + e;
      if (d > 0.0 && q < nbits) graph.set((int)(q / n), (int)(q % n));
    }
  }
}
// union over the ranks through the sum exchange; the number of ranks comes from the exchange itself (a hook may come without
// world_size)
int union_graph_over_ranks(CamGraph& graph, const SumExchange& exchange) {
  double ones = 1.0;
  if (int rc = exchange(&ones, 1)) return rc;
  const int world = std::max((int)std::llround(ones), 1);
  std::vector<double> packed;
  pack_graph(graph, world, packed);
  if (int rc = exchange(packed.data(), (int64_t)packed.size())) return rc;
  unpack_graph(packed, world, graph);
  return 0;
}

// ---- camera order -------------------------------------------------------------------------------------------------------------
// The camera graph decides the slot order — nested dissection when it shortens the dependent chain of the tile factorisation
// (chol_plan.h) — and which 6x6 blocks of S exist.
void plan_camera_order(const CamGraph& graph, const BuildOptions& opt, CholPlan& plan, CameraLayout& cams) {
  const int forced_depth = opt.chol_nd;
  plan_auto(graph, forced_depth, forced_depth >= -1, opt.chol_cuts, !opt.chol_inverse ? 0 : dense_plain_max_tiles(), dense_inv_rows(), plan,
            [](int n, void (*fn)(void*, int), void* ctx) { run_parts(n, [&](int t, int) { fn(ctx, t); }); });
  cams.nat_slot = plan.slot_of_nat;
  cams.ncv = plan.nslots;                 // a permutation of the variable cameras
  cams.n = plan.n;                        // columns of the reduced system incl. the alignment padding
  cams.nt = (cams.n + 31) / 32;
  for (int32_t& s : cams.slot)
    if (s >= 0) s = plan.slot_of_nat[(size_t)s];
}
// beyond kIndexMaxSlots variable cameras (or MPSFM_CHOL_GRAPH=0): the caller's order and a block skyline
void keep_caller_order(CameraLayout& cams) {
  cams.nat_slot.resize((size_t)cams.ncv_real);
  std::iota(cams.nat_slot.begin(), cams.nat_slot.end(), 0);
}

// ---- records ------------------------------------------------------------------------------------------------------------------
namespace {

struct MergedRecords {
  std::vector<int64_t> prec;  // record range per caller landmark
  HostBuf<Rec> recs;          // uninitialised: value-initialising tens of MB on one thread costs milliseconds
  std::vector<Rec> fixed;     // blocks of a constant camera and a constant landmark
  std::vector<int32_t> fixed_pt;
  int64_t count(int p) const { return prec[(size_t)p + 1] - prec[(size_t)p]; }
};
struct LandmarkOrder {
  std::vector<uint8_t> heavy_flag;  // per caller landmark: goes to a chunk of the general kernel
  std::vector<int32_t> inv;         // caller's landmark -> re-ordered index or -1
};

// Phase B (the same host threads as the grouping): every landmark's blocks ordered by (final) camera slot, a reprojection and a
// depth block of one (camera, landmark) pair merged into one record; fixed blocks (constant camera and constant landmark) are
// kept aside.  Then the parts' records side by side.
int merge_records(const mpsfm_ba_problem* P, const std::vector<int32_t>& slot, LandmarkGroups& G, MergedRecords& R, const Lap& lap) {
  const int npu = P->n_pts, mparts = (int)G.parts.size();
  std::vector<LandmarkGroups::Part>& mp = G.parts;
  auto deff = [&](int cam, int64_t src) {
    double b = 0.0, s = 0.0;
    if (P->shift_logscale) { b = P->shift_logscale[2 * cam]; s = P->shift_logscale[2 * cam + 1]; }
    return P->dobs_depth[src] * std::exp(s) + b;
  };
  run_parts(mparts, [&](int t, int) {
    LandmarkGroups::Part& M = mp[(size_t)t];
    const int p0 = M.p0, np_loc = M.p1 - M.p0;
    Blk* const blks = M.blks.data();
    for (size_t q = 0; q < M.blks.size(); ++q) blks[q].key = slot[(size_t)blks[q].cam] < 0 ? INT32_MAX : slot[(size_t)blks[q].cam];
    M.recs.alloc(M.blks.size());
    M.nrecs = 0;
    M.nrec_of.assign((size_t)np_loc, 0);
    for (int q = 0; q < np_loc; ++q) {
      const int p = p0 + q;
      Blk* const b0 = blks + M.pstart[(size_t)q]; Blk* const b1 = blks + M.pstart[(size_t)q + 1];
      std::sort(b0, b1, [](const Blk& x, const Blk& y) {
        if (x.key != y.key) return x.key < y.key;
        if (x.cam != y.cam) return x.cam < y.cam;
        if (x.kind != y.kind) return x.kind < y.kind;
        return x.src < y.src;
      });
      const size_t before = M.nrecs;
      for (auto it = b0; it != b1;) {
        auto je = it;
        while (je != b1 && je->cam == it->cam) ++je;
        auto mid = it;
        while (mid != je && mid->kind == 0) ++mid;
        const int64_t nr = mid - it, nd = je - mid;
        const bool is_fixed = (slot[it->cam] < 0) && P->pt_const[p];
        for (int64_t k = 0; k < std::max(nr, nd); ++k) {
          Rec r{it->cam, slot[it->cam], 0, 0, 0, 1.0, 0.0, 1.0};
          if (k < nr) { const int64_t s = (it + k)->src; r.flags |= kRecHasReproj; r.u = P->obs_xy[2 * s]; r.v = P->obs_xy[2 * s + 1]; }
          if (k < nd) {
            const int64_t s = (mid + k)->src;
            r.flags |= kRecHasDepth; r.d = deff(it->cam, s); r.m = P->dobs_magnitude[s]; r.a = P->dobs_param[s];
            if (!(r.d > 0.0)) { M.err = 2; return; }
            r.d = std::log(r.d);  // the residual is log Z - log d: the records carry log d (one logarithm less per evaluation)
          }
          if (is_fixed) { M.fixed.push_back(r); M.fixed_pt.push_back(p); }
          else M.recs[M.nrecs++] = r;
        }
        it = je;
      }
      M.nrec_of[(size_t)q] = (int64_t)(M.nrecs - before);
    }
    M.blks.release();
  });
  for (const LandmarkGroups::Part& M : mp)
    if (M.err == 2) return fail(MPSFM_EINVAL, "shifted/scaled depth prior must be positive");
  lap("sort + merge into records (threads)");
  R.prec.assign((size_t)npu + 1, 0);
  std::vector<int64_t> base((size_t)mparts + 1, 0);
  for (int t = 0; t < mparts; ++t) base[(size_t)t + 1] = base[(size_t)t] + (int64_t)mp[(size_t)t].nrecs;
  R.recs.alloc((size_t)base[(size_t)mparts]);
  run_parts(mparts, [&](int t, int) {
    LandmarkGroups::Part& M = mp[(size_t)t];
    std::copy(M.recs.data(), M.recs.data() + M.nrecs, R.recs.data() + base[(size_t)t]);
    int64_t o = base[(size_t)t];
    for (int q = 0; q < M.p1 - M.p0; ++q) { R.prec[(size_t)(M.p0 + q)] = o; o += M.nrec_of[(size_t)q]; }
    M.recs.release();
  });
  R.prec[(size_t)npu] = base[(size_t)mparts];
  for (LandmarkGroups::Part& M : mp) {
    R.fixed.insert(R.fixed.end(), M.fixed.begin(), M.fixed.end());
    R.fixed_pt.insert(R.fixed_pt.end(), M.fixed_pt.begin(), M.fixed_pt.end());
  }
  return 0;
}

// Landmark order: those with records sorted by their camera-slot list; the long tracks behind them, the landmarks of the general
// kernel at the end of the chunked ones; last the rest that are referenced by fixed blocks only.
void order_landmarks(const mpsfm_ba_problem* P, const MergedRecords& R, const BuildOptions& opt, HostTables& T, LandmarkOrder& L, const Lap& lap) {
  const int npu = P->n_pts;
  const std::vector<int64_t>& prec = R.prec;
  const HostBuf<Rec>& recs = R.recs;
  std::vector<int32_t>& order = T.order;
  order.clear(); order.reserve(npu);
  for (int p = 0; p < npu; ++p) if (prec[p + 1] > prec[p]) order.push_back(p);
  {
    // sort key: the first six camera slots of the track (16 bits each; slots beyond 65534 and constant
    // cameras saturate), then the track length, then the landmark index — neighbours in this order share
    // cameras, which keeps the set of S blocks a chunk touches small
    struct Key { uint64_t k1, k2; int32_t p; };
    std::vector<Key> keyed(order.size());
    auto key_less = [](const Key& a, const Key& b) {
      if (a.k1 != b.k1) return a.k1 < b.k1;
      if (a.k2 != b.k2) return a.k2 < b.k2;
      return a.p < b.p;
    };
    // sorted runs per thread, then pairwise merges (the order is total, so the result does not depend on the split)
    const int sparts = (int)std::max<size_t>(1, std::min<size_t>((size_t)host_threads(), order.size() / 8192));
    std::vector<size_t> cut((size_t)sparts + 1);
    for (int t = 0; t <= sparts; ++t) cut[(size_t)t] = order.size() * (size_t)t / (size_t)sparts;
    run_parts(sparts, [&](int t, int) {
      for (size_t q = cut[(size_t)t]; q < cut[(size_t)t + 1]; ++q) {
        const int pnt = order[q];
        const int64_t n_p = prec[pnt + 1] - prec[pnt];
        uint64_t key[2] = {0, 0};
        for (int64_t k = 0; k < 6; ++k) {
          uint64_t sk = 0xffff;
          if (k < n_p && recs[prec[pnt] + k].slot >= 0) sk = (uint64_t)std::min(recs[prec[pnt] + k].slot, 0xfffe);
          key[k / 4] = (key[k / 4] << 16) | sk;
        }
        key[1] = (key[1] << 32) | (uint64_t)std::min<int64_t>(n_p, 0xffffffff);
        keyed[q] = Key{key[0], key[1], pnt};
      }
      std::sort(keyed.begin() + (std::ptrdiff_t)cut[(size_t)t], keyed.begin() + (std::ptrdiff_t)cut[(size_t)t + 1], key_less);
    });
    for (int width = 1; width < sparts; width *= 2) {
      std::vector<int> lefts;
      for (int t = 0; t + width < sparts; t += 2 * width) lefts.push_back(t);
      run_parts((int)lefts.size(), [&](int j, int) {
        const int t = lefts[(size_t)j];
        std::inplace_merge(keyed.begin() + (std::ptrdiff_t)cut[(size_t)t], keyed.begin() + (std::ptrdiff_t)cut[(size_t)(t + width)],
                           keyed.begin() + (std::ptrdiff_t)cut[(size_t)std::min(t + 2 * width, sparts)], key_less);
      });
    }
    for (size_t q = 0; q < order.size(); ++q) order[q] = keyed[q].p;
  }
  lap("sort landmarks by key");
  // landmarks whose track does not fit one chunk are swept by a workgroup of their own
  auto is_long = [&](int p) {
    const int64_t r_p = prec[p + 1] - prec[p];
    if (r_p > kObsMax) return true;
    int distinct = 0, last = -2;
    for (int64_t r = prec[p]; r < prec[p + 1]; ++r)
      if (recs[r].slot >= 0 && recs[r].slot != last) { ++distinct; last = recs[r].slot; }
    return distinct > kLocalCamsMax;
  };
  std::vector<uint8_t> long_flag((size_t)npu + 1, 0);
  parallel_ranges((int64_t)order.size(), 8192, [&](int64_t q0, int64_t q1) {
    for (int64_t q = q0; q < q1; ++q) long_flag[(size_t)order[(size_t)q]] = is_long(order[(size_t)q]) ? 1 : 0;
  });
  auto first_long = std::stable_partition(order.begin(), order.end(), [&](int p) { return !long_flag[(size_t)p]; });
  T.np_chunked = (int64_t)(first_long - order.begin());
  // Landmarks the dense sweep cannot take — more than kDenseCams variable cameras, or two records of one camera for a variable
  // landmark — go behind the others (same relative order), so that they form chunks of their own for the general kernel and
  // every other chunk is dense by construction (the cut below keeps those within kDenseCams cameras / kDensePts landmarks).
  const bool dense_on = opt.sweep_dense;
  L.heavy_flag.assign((size_t)npu + 1, dense_on ? 0 : 1);
  if (dense_on) {
    parallel_ranges(T.np_chunked, 8192, [&](int64_t q0, int64_t q1) {
      for (int64_t q = q0; q < q1; ++q) {
        const int p = order[(size_t)q];
        int distinct = 0, last = -2;
        bool dup = false;
        for (int64_t r = prec[p]; r < prec[p + 1]; ++r) {
          if (recs[r].slot < 0) continue;
          if (recs[r].slot != last) { ++distinct; last = recs[r].slot; }
          else dup = true;  // records are slot-sorted: two of one camera are neighbours
        }
        L.heavy_flag[(size_t)p] = (distinct > kDenseCams || (dup && !P->pt_const[p])) ? 1 : 0;
      }
    });
    std::stable_partition(order.begin(), first_long, [&](int p) { return !L.heavy_flag[(size_t)p]; });
  }
  T.n_long = (int64_t)(order.end() - first_long);
  {
    std::vector<uint8_t> seen((size_t)npu + 1, 0);
    for (int p : order) seen[p] = 1;
    for (int32_t p : R.fixed_pt) if (!seen[p]) { seen[p] = 1; order.push_back(p); }
  }
  T.np = (int64_t)order.size();
  L.inv.assign((size_t)npu + 1, -1);
  for (int64_t k = 0; k < T.np; ++k) L.inv[order[k]] = (int32_t)k;
}

// Chunking, pass 1 (greedy): cut the ordered landmarks into chunks and collect each chunk's sorted camera slots.
// rec_off: first record of every chunked landmark.
void cut_chunks(const MergedRecords& R, const LandmarkOrder& L, const BuildOptions& opt, HostTables& T, std::vector<int64_t>& rec_off) {
  const std::vector<int64_t>& prec = R.prec;
  const HostBuf<Rec>& recs = R.recs;
  const std::vector<int32_t>& order = T.order;
  const std::vector<uint8_t>& heavy_flag = L.heavy_flag;
  const int rec_cap = opt.rec_cap, pts_by_cams = opt.pts_by_cams;
  rec_off.assign((size_t)T.np_chunked + 1, 0);
  for (int64_t k = 0; k < T.np_chunked; ++k) rec_off[(size_t)k + 1] = rec_off[(size_t)k] + (prec[order[k] + 1] - prec[order[k]]);
  // The greedy cut is sequential by nature; the ordered landmarks are therefore split into a FIXED number
  // of segments (independent of the thread count, so the tables are the same on every machine), each cut
  // greedily on its own with a forced chunk boundary at the segment ends.
  struct Seg { std::vector<ChunkHdr> chunks; std::vector<int32_t> cams; };
  const int nseg = (int)std::max<int64_t>(1, std::min<int64_t>(64, T.np_chunked / 4096));
  std::vector<Seg> segs((size_t)nseg);
  auto cut_segment = [&](int sidx) {
    Seg& G = segs[(size_t)sidx];
    const int64_t k0 = T.np_chunked * sidx / nseg, k1 = T.np_chunked * (sidx + 1) / nseg;
    std::vector<int32_t> cur_cams, pc, uni;  // sorted slots of the open chunk
    int64_t c_first = k0, c_nrec = 0;
    auto close_chunk = [&](int64_t end_pt) {
      if (end_pt == c_first) return;
      ChunkHdr H{};
      H.rec0 = (int32_t)rec_off[(size_t)c_first]; H.nrec = (int32_t)(rec_off[(size_t)end_pt] - rec_off[(size_t)c_first]);
      H.pt0 = (int32_t)c_first; H.npt = (int32_t)(end_pt - c_first);
      H.cam0 = (int32_t)G.cams.size(); H.ncam = (int32_t)cur_cams.size();  // segment-local for now
      G.cams.insert(G.cams.end(), cur_cams.begin(), cur_cams.end());
      G.chunks.push_back(H);
      cur_cams.clear(); c_first = end_pt; c_nrec = 0;
    };
    for (int64_t k = k0; k < k1; ++k) {
      const int p = order[k];
      const int64_t r_p = prec[p + 1] - prec[p];
      pc.clear();
      for (int64_t r = prec[p]; r < prec[p + 1]; ++r) if (recs[r].slot >= 0) pc.push_back(recs[r].slot);
      pc.erase(std::unique(pc.begin(), pc.end()), pc.end());  // records are slot-sorted
      const bool subset = std::includes(cur_cams.begin(), cur_cams.end(), pc.begin(), pc.end());
      size_t nuni = cur_cams.size();
      if (!subset) {
        uni.clear();
        std::set_union(cur_cams.begin(), cur_cams.end(), pc.begin(), pc.end(), std::back_inserter(uni));
        nuni = uni.size();
      }
      const bool hv = heavy_flag[(size_t)p] != 0;
      const bool too_big = (c_nrec + r_p > (hv ? kObsMax : rec_cap)) || (k - c_first + 1 > (hv ? kPtsMax : dense_pts_cap((int)nuni, pts_by_cams))) || ((int)nuni > (hv ? kLocalCamsMax : kDenseCams)) ||
                           (hv != (heavy_flag[(size_t)order[(size_t)c_first]] != 0));  // dense and general landmarks never share a chunk
      if (k > c_first && too_big) {
        close_chunk(k);
        cur_cams = pc;
      } else if (!subset) {
        cur_cams.swap(uni);
      }
      c_nrec += r_p;
    }
    close_chunk(k1);
  };
  run_parts(std::min(host_threads(), nseg), [&](int t, int nparts) { for (int sidx = t; sidx < nseg; sidx += nparts) cut_segment(sidx); });
  for (Seg& G : segs) {
    const int32_t cbase = (int32_t)T.chunk_cams.size();
    for (ChunkHdr& H : G.chunks) { H.cam0 += cbase; T.chunks.push_back(H); }
    T.chunk_cams.insert(T.chunk_cams.end(), G.cams.begin(), G.cams.end());
  }
}

// Chunking, pass 2 (host threads over contiguous chunk ranges): records, local camera indices and the block-major Schur pair
// tables of every chunk; then the per-thread pair tables concatenated and the chunk offsets made global.
int fill_chunk_records(const mpsfm_ba_problem* P, const MergedRecords& R, const LandmarkOrder& L, const std::vector<int64_t>& rec_off, HostTables& T,
                       const Lap& lap) {
  const std::vector<int64_t>& prec = R.prec;
  const HostBuf<Rec>& recs = R.recs;
  const std::vector<int32_t>& order = T.order;
  std::vector<ChunkHdr>& chunks = T.chunks;
  T.nrec = rec_off[(size_t)T.np_chunked];
  for (int64_t k = T.np_chunked; k < T.np_chunked + T.n_long; ++k) T.nrec += prec[order[k] + 1] - prec[order[k]];
  if (T.nrec > (int64_t)INT32_MAX) return fail(MPSFM_EUNSUPPORTED, "more than 2^31 records on one device");
  const size_t nr = (size_t)T.nrec;
  T.rec_cam.alloc(nr); T.rec_pt.alloc(nr); T.rec_meta.alloc(nr); T.rec_xy.alloc(2 * nr); T.rec_d.alloc(nr); T.rec_m.alloc(nr); T.rec_a.alloc(nr);
  lap("size record arrays");
  struct ChunkPart {
    std::vector<uint32_t> blk_desc, ents;
    std::vector<int32_t> blk_ent_start;
    int64_t nblk_reduced = 0;
    double nvarpts = 0;
  };
  const int nch = (int)chunks.size();
  const int cparts = std::max(1, std::min(host_threads(), nch / 48));
  std::vector<ChunkPart> cp((size_t)cparts);
  run_parts(cparts, [&](int t, int nparts) {
    ChunkPart& C = cp[(size_t)t];
    PairScratch ps;
    for (int c = (int)((int64_t)nch * t / nparts); c < (int)((int64_t)nch * (t + 1) / nparts); ++c) {
      ChunkHdr& H = chunks[(size_t)c];
      const int32_t* cams = T.chunk_cams.data() + H.cam0;
      const int64_t c_first = H.pt0, end_pt = (int64_t)H.pt0 + H.npt;
      int64_t w = H.rec0;  // next record
      for (int64_t k = c_first; k < end_pt; ++k) {
        const int p = order[k];
        T.pt_rec_start[(size_t)k] = (int32_t)w;
        int kv = 0;
        for (int64_t r = prec[p]; r < prec[p + 1]; ++r, ++w) {
          const Rec& Rc = recs[r];
          uint32_t lcam = kLcamConst;
          if (Rc.slot >= 0) {
            lcam = (uint32_t)(std::lower_bound(cams, cams + H.ncam, Rc.slot) - cams);
            ++kv;
          }
          T.rec_cam[(size_t)w] = Rc.cam; T.rec_pt[(size_t)w] = (int32_t)k;
          T.rec_meta[(size_t)w] = lcam | ((uint32_t)(k - c_first) << 8) | Rc.flags;
          T.rec_xy[2 * (size_t)w] = Rc.u; T.rec_xy[2 * (size_t)w + 1] = Rc.v; T.rec_d[(size_t)w] = Rc.d; T.rec_m[(size_t)w] = Rc.m; T.rec_a[(size_t)w] = Rc.a;
          C.nblk_reduced += ((Rc.flags & kRecHasReproj) ? 1 : 0) + ((Rc.flags & kRecHasDepth) ? 1 : 0);
        }
        if (!P->pt_const[p]) {
          T.pt_kv[(size_t)k] = (uint16_t)kv;
          C.nvarpts += 1;
        }
      }
      // Chunks that form their Schur blocks as one dense product (k_track_sweep) need no pair tables at all.
      H.dense = L.heavy_flag[(size_t)order[(size_t)c_first]] ? 0 : 1;  // by construction: <= kDenseCams cameras, <= kDensePts landmarks, no duplicates
      H.slab0 = 0;
      append_pair_tables(H, T.rec_meta.data(), T.pt_kv.data(), T.pt_rec_start.data(), order.data(), P->pt_const, C.blk_desc, C.ents, C.blk_ent_start, ps);
    }
  });
  lap("chunk records + pairs (threads)");
  // concatenate the per-thread pair tables and make the chunk offsets global
  std::vector<size_t> bbase((size_t)cparts + 1, 0), ebase((size_t)cparts + 1, 0), sbase((size_t)cparts + 1, 0);
  for (int t = 0; t < cparts; ++t) {
    bbase[(size_t)t + 1] = bbase[(size_t)t] + cp[(size_t)t].blk_desc.size();
    ebase[(size_t)t + 1] = ebase[(size_t)t] + cp[(size_t)t].ents.size();
    sbase[(size_t)t + 1] = sbase[(size_t)t] + cp[(size_t)t].blk_ent_start.size();
    T.nblk_reduced += cp[(size_t)t].nblk_reduced; T.nvarpts += cp[(size_t)t].nvarpts;
  }
  if (ebase[(size_t)cparts] > (size_t)INT32_MAX) return fail(MPSFM_EUNSUPPORTED, "too many Schur pairs for 32-bit entry offsets");
  T.blk_desc.resize(bbase[(size_t)cparts]); T.ents.resize(ebase[(size_t)cparts]); T.blk_ent_start.resize(sbase[(size_t)cparts]);
  run_parts(cparts, [&](int t, int nparts) {
    const ChunkPart& C = cp[(size_t)t];
    std::copy(C.blk_desc.begin(), C.blk_desc.end(), T.blk_desc.begin() + (std::ptrdiff_t)bbase[(size_t)t]);
    std::copy(C.ents.begin(), C.ents.end(), T.ents.begin() + (std::ptrdiff_t)ebase[(size_t)t]);
    std::copy(C.blk_ent_start.begin(), C.blk_ent_start.end(), T.blk_ent_start.begin() + (std::ptrdiff_t)sbase[(size_t)t]);
    for (int c = (int)((int64_t)nch * t / nparts); c < (int)((int64_t)nch * (t + 1) / nparts); ++c) {
      chunks[(size_t)c].blk0 += (int32_t)bbase[(size_t)t];
      chunks[(size_t)c].ent0 += (int32_t)ebase[(size_t)t];
    }
  });
  return 0;
}

// The records and headers of the long tracks, behind the chunked records; then pt_rec_start of the landmarks without records.
void fill_long_tracks(const mpsfm_ba_problem* P, const MergedRecords& R, HostTables& T) {
  const std::vector<int32_t>& order = T.order;
  size_t w = T.np_chunked > 0 ? (size_t)(T.pt_rec_start[(size_t)T.np_chunked - 1] + R.count(order[(size_t)T.np_chunked - 1])) : 0;
  for (int64_t k = T.np_chunked; k < T.np_chunked + T.n_long; ++k) {
    const int p = order[k];
    LongHdr L{};
    L.rec0 = (int32_t)w; L.pt = (int32_t)k; L.w0 = T.wl_rows;
    T.pt_rec_start[k] = L.rec0;
    int kv = 0;
    for (int64_t r = R.prec[p]; r < R.prec[p + 1]; ++r, ++w) {
      const Rec& Rc = R.recs[r];
      if (Rc.slot >= 0) ++kv;
      T.rec_cam[w] = Rc.cam; T.rec_pt[w] = (int32_t)k;
      T.rec_meta[w] = (Rc.slot >= 0 ? 0u : kLcamConst) | Rc.flags;
      T.rec_xy[2 * w] = Rc.u; T.rec_xy[2 * w + 1] = Rc.v; T.rec_d[w] = Rc.d; T.rec_m[w] = Rc.m; T.rec_a[w] = Rc.a;
      T.nblk_reduced += ((Rc.flags & kRecHasReproj) ? 1 : 0) + ((Rc.flags & kRecHasDepth) ? 1 : 0);
    }
    L.nrec = (int32_t)w - L.rec0;
    L.kv = P->pt_const[p] ? 0 : kv;
    if (!P->pt_const[p]) { T.pt_kv[k] = (uint16_t)std::min(kv, 0xfffe); T.nvarpts += 1; }
    T.wl_rows += kv;
    T.lhdr.push_back(L);
  }
  for (int64_t k = T.np_chunked + T.n_long; k <= T.np; ++k) T.pt_rec_start[k] = (int32_t)T.nrec;
}

// fixed records (landmark index re-ordered)
void fill_fixed_records(const MergedRecords& R, const LandmarkOrder& L, HostTables& T) {
  const std::vector<Rec>& fixed = R.fixed;
  for (size_t i = 0; i < fixed.size(); ++i) {
    T.fx_cam.push_back(fixed[i].cam); T.fx_pt.push_back(L.inv[R.fixed_pt[i]]); T.fx_meta.push_back(fixed[i].flags);
    T.fx_xy.push_back(fixed[i].u); T.fx_xy.push_back(fixed[i].v); T.fx_d.push_back(fixed[i].d); T.fx_m.push_back(fixed[i].m); T.fx_a.push_back(fixed[i].a);
  }
}

}  // namespace

int build_record_tables(const mpsfm_ba_problem* P, const CameraLayout& cams, const BuildOptions& opt, LandmarkGroups& G, HostTables& T, const Lap& lap) {
  T.chunks.clear(); T.chunk_cams.clear();  // a device build that handed the problem back may have left counts behind
  T.nblk_reduced = 0; T.nvarpts = 0; T.wl_rows = 0;
  MergedRecords R;
  if (int rc = merge_records(P, cams.slot, G, R, lap)) return rc;
  T.nfixed = (int64_t)R.fixed.size();
  lap("merge records");
  LandmarkOrder L;
  order_landmarks(P, R, opt, T, L, lap);
  lap("order landmarks");
  T.pt_rec_start.assign((size_t)T.np + 1, 0);
  T.pt_kv.assign((size_t)T.np + 1, 0xffff);
  std::vector<int64_t> rec_off;
  cut_chunks(R, L, opt, T, rec_off);
  lap("chunk boundaries");
  if (int rc = fill_chunk_records(P, R, L, rec_off, T, lap)) return rc;
  lap("concatenate pair tables");
  fill_long_tracks(P, R, T);
  fill_fixed_records(R, L, T);
  return 0;
}

// ---- block pattern of S -------------------------------------------------------------------------------------------------------
void s_pattern_index(const CameraLayout& cams, const CholPlan& plan, const CamGraph& graph, SPattern& S) {
  const int ns = cams.ncv;
  S.sky_index.assign((size_t)ns * (size_t)ns, -1);
  int32_t nblk = 0;
  for (int sj = 0; sj < ns; ++sj) {
    const int j = plan.nat_of_slot[(size_t)sj];
    if (j < 0) continue;
    for (int si = 0; si <= sj; ++si) {
      const int i = plan.nat_of_slot[(size_t)si];
      if (i < 0) continue;
      if (i == j || graph.get(i, j)) S.sky_index[(size_t)sj * ns + si] = nblk++;
    }
  }
  S.nblk = nblk;
}

// block skyline (DenseEnvelope): which 6x6 blocks of S can be nonzero follows from the static Schur pair tables;
// first_blk[c] = lowest camera slot that shares a landmark with slot c
int s_pattern_skyline(const CameraLayout& cams, const HostTables& T, const BuildOptions& opt, const SumExchange& exchange, bool verbose, SPattern& S,
                      CholPlan& PL) {
  const int ncv = cams.ncv, nt = cams.nt, n = cams.n;
  const std::vector<int32_t>& slot = cams.slot;
  std::vector<int32_t> first_blk((size_t)std::max(ncv, 1));
  for (int c = 0; c < ncv; ++c) first_blk[(size_t)c] = c;
  for (const ChunkHdr& H : T.chunks) {
    const int32_t* cc = T.chunk_cams.data() + H.cam0;
    if (H.dense)  // no pair table: every pair of the chunk's (sorted) cameras may be coupled
      for (int q = 1; q < H.ncam; ++q) first_blk[(size_t)cc[q]] = std::min(first_blk[(size_t)cc[q]], cc[0]);
    for (int b = 0; b < H.nblk; ++b) {
      const uint32_t d = T.blk_desc[(size_t)H.blk0 + (size_t)b];
      const int si = cc[d & 0xff], sj = cc[(d >> 8) & 0xff];
      const int lo = std::min(si, sj), hi = std::max(si, sj);
      first_blk[(size_t)hi] = std::min(first_blk[(size_t)hi], lo);
    }
  }
  for (const LongHdr& L : T.lhdr) {  // a long track couples all its variable cameras
    int lo = INT32_MAX;
    for (int r = 0; r < L.kv; ++r) lo = std::min(lo, slot[T.rec_cam[(size_t)L.rec0 + (size_t)r]]);
    for (int r = 0; r < L.kv; ++r) { int32_t& f = first_blk[(size_t)slot[T.rec_cam[(size_t)L.rec0 + (size_t)r]]]; f = std::min(f, lo); }
  }
  if (!opt.chol_envelope) std::fill(first_blk.begin(), first_blk.end(), 0);  // A/B: treat S as dense
  if (exchange && ncv > 0) {
    // landmark shards see different camera pairs: every rank needs the UNION.  The hook only sums, so the minimum over
    // ranks is found by bisection on indicator sums (the same number of rounds on every rank).
    std::vector<double> lo((size_t)ncv, 0.0), hi((size_t)ncv), ind((size_t)ncv);
    for (int c = 0; c < ncv; ++c) hi[(size_t)c] = (double)c;
    int rounds = 1;
    while ((1 << rounds) < ncv + 1) ++rounds;
    for (int it = 0; it < rounds; ++it) {
      for (int c = 0; c < ncv; ++c) ind[(size_t)c] = first_blk[(size_t)c] <= (int)std::floor(0.5 * (lo[(size_t)c] + hi[(size_t)c])) ? 1.0 : 0.0;
      if (int rc2 = exchange(ind.data(), ncv)) return rc2;
      for (int c = 0; c < ncv; ++c) {
        const double mid = std::floor(0.5 * (lo[(size_t)c] + hi[(size_t)c]));
        if (ind[(size_t)c] > 0.0) hi[(size_t)c] = mid; else lo[(size_t)c] = std::min(mid + 1.0, hi[(size_t)c]);
      }
    }
    for (int c = 0; c < ncv; ++c) first_blk[(size_t)c] = (int32_t)hi[(size_t)c];
  }
  S.sky_first = first_blk;
  S.sky_start.assign((size_t)ncv + 1, 0);
  for (int c = 0; c < ncv; ++c) S.sky_start[(size_t)c + 1] = S.sky_start[(size_t)c] + (c - first_blk[(size_t)c] + 1);
  S.nblk = S.sky_start[(size_t)ncv];
  std::vector<int32_t> first((size_t)nt + 1, 0);
  for (int ti = 0; ti < nt; ++ti) {
    int f = ti;
    for (int r = ti * 32; r < std::min(n, ti * 32 + 32); ++r) f = std::min(f, (6 * first_blk[(size_t)(r / 6)]) / 32);
    first[(size_t)ti] = f;
  }
  first[(size_t)nt] = 0;  // the right-hand-side row
  // the factorisation plan of the skyline in the caller's order: tile (ti, tj) can be nonzero for tj >= first[ti]
  std::vector<uint8_t> pat((size_t)nt * (size_t)nt, 0);
  for (int ti = 0; ti < nt; ++ti)
    for (int tj = first[(size_t)ti]; tj < ti; ++tj) pat[(size_t)ti * nt + tj] = 1;
  PL.ncv = ncv; PL.nslots = ncv; PL.n = n; PL.nd_depth = -1;
  PL.slot_of_nat = cams.nat_slot; PL.nat_of_slot = cams.nat_slot;  // identity, no padding: slot_of_col stays empty (NULL map)
  plan_from_pattern(pat, nt, nt <= dense_plain_max_tiles() && opt.chol_inverse, dense_inv_rows(), PL);
  if (verbose) {
    int64_t inside = 0;
    for (int ti = 0; ti < nt; ++ti) inside += ti - first[(size_t)ti] + 1;
    std::fprintf(stderr, "[mpsfm_ba] build: block skyline %lld of %lld tiles\n", (long long)inside, (long long)nt * (nt + 1) / 2);
  }
  return 0;
}

// ---- slabs of the dense chunks and the tables of their reduction (k_reduce_slabs) ------------------------------------------------
int assign_slabs(std::vector<ChunkHdr>& chunks, SlabTables& R) {
  R.n_dense = 0;
  R.slab_units = 0;
  for (size_t c = 0; c < chunks.size(); ++c) {
    ChunkHdr& H = chunks[c];
    if (!H.dense) continue;
    if ((int)c != R.n_dense) return fail(MPSFM_EUNSUPPORTED, "internal: dense chunks must precede the general ones");
    H.slab0 = (int32_t)R.slab_units;
    R.slab_units += slab_doubles(H.ncam) / 18;
    if (R.slab_units > (int64_t)INT32_MAX) return fail(MPSFM_EUNSUPPORTED, "slabs of the dense chunks exceed 2^31 units");
    R.n_dense = (int)c + 1;
  }
  return 0;
}

// order table of the dense sweep (SweepArgs::order): the dense chunks by descending dense_sweep_cost, ties by ascending index
void dense_sweep_order(const std::vector<ChunkHdr>& chunks, int n_dense, std::vector<int32_t>& order) {
  std::vector<uint64_t> key((size_t)std::max(n_dense, 0));
  for (int c = 0; c < n_dense; ++c) key[(size_t)c] = dense_sweep_order_key(chunks[(size_t)c], c);
  std::sort(key.begin(), key.end());
  order.resize(key.size());
  for (size_t i = 0; i < key.size(); ++i) order[i] = (int32_t)(uint32_t)key[i];
}

// per destination — a block of S or a camera's vectors — the slab positions that contribute, in chunk order; destinations with
// many sources are split into parts
int slab_reduction_tables(const HostTables& T, const CameraLayout& cams, const CholPlan& plan, const SPattern& S, bool tables, SlabTables& R) {
  const int ncv = cams.ncv;
  const bool use_graph = cams.use_graph;
  const int64_t nsb = S.nblk;
  auto host_sky = [&](int si, int sj) -> int64_t {
    return use_graph ? (int64_t)S.sky_index[(size_t)sj * (size_t)ncv + (size_t)si] : S.sky_start[(size_t)sj] + (si - S.sky_first[(size_t)sj]);
  };
  const size_t ndst = (size_t)nsb + (size_t)std::max(ncv, 0);
  // the blocks of S on the diagonal
  std::vector<uint8_t> is_diag((size_t)nsb, 0);
  R.diag_block.assign((size_t)std::max(ncv, 1), -1);
  for (int sl = 0; sl < ncv; ++sl) {
    if (use_graph && plan.nat_of_slot[(size_t)sl] < 0) continue;
    const int64_t b = host_sky(sl, sl);
    if (b >= 0 && b < nsb) { R.diag_block[(size_t)sl] = (int32_t)b; is_diag[(size_t)b] = 1; }
  }
  if (!tables) return 0;
  std::vector<int32_t> cnt(ndst + 1, 0);
  for (int pass = 0; pass < 2; ++pass) {  // count, then place (chunk order within a destination)
    if (pass == 1) {
      for (size_t d = 1; d <= ndst; ++d) cnt[d] += cnt[d - 1];
      R.srcs.resize((size_t)cnt[ndst]);
    }
    for (int c = 0; c < R.n_dense; ++c) {
      const ChunkHdr& H = T.chunks[(size_t)c];
      const int32_t* cc = T.chunk_cams.data() + H.cam0;
      const int nb = H.ncam * (H.ncam + 1) / 2;
      for (int cj = 0; cj < H.ncam; ++cj) {
        for (int ci = 0; ci <= cj; ++ci) {
          const int64_t b = host_sky(cc[ci], cc[cj]);
          if (b < 0) continue;  // two cameras of the chunk that share no landmark anywhere: their product is exactly zero, S has no such block
          if (b >= nsb) return fail(MPSFM_EUNSUPPORTED, "internal: block index beyond S");
          if (pass == 0) cnt[(size_t)b + 1]++;
          else R.srcs[(size_t)cnt[(size_t)b]++] = H.slab0 + 2 * (cj * (cj + 1) / 2 + ci);
        }
        const size_t d = (size_t)nsb + (size_t)cc[cj];
        if (pass == 0) cnt[d + 1]++;
        else R.srcs[(size_t)cnt[d]++] = H.slab0 + 2 * nb + cj;
      }
    }
  }
  // after the placing pass cnt[d] is the END of destination d
  constexpr int kPart = 16;
  for (size_t d = 0; d < ndst; ++d) {
    const int32_t s0 = d == 0 ? 0 : cnt[d - 1], s1 = cnt[d];
    for (int32_t q = s0; q < s1; q += kPart) {
      RedDest D;
      D.kind = d >= (size_t)nsb ? 2 : (is_diag[d] ? 1 : 0);
      D.dst = d >= (size_t)nsb ? (int32_t)(d - (size_t)nsb) : (int32_t)d;
      D.s0 = q; D.s1 = std::min(q + kPart, s1);
      R.dests.push_back(D);
    }
  }
  return 0;
}

}  // namespace mpsfm
