// Host side of libmpsfm_hip: problem upload, chunking of the landmark tracks, the
// Levenberg-Marquardt control loop (Ceres 2.1 TrustRegionMinimizer semantics with the default
// pyceres.SolverOptions() that reference mpsfm/sfm/mapper/bundle_adjustment.py:285-293 uses) and
// the C ABI of include/mpsfm_hip.h.  All arithmetic on problem data runs in the HIP kernels of
// ba_kernels.hip / dense_chol.hip; this file only orders launches and takes the accept/reject
// decisions from a handful of scalars.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include <dlfcn.h>

#include "common.h"
#include "build_host.h"
#include "devbuild.h"
#include "local_lm.h"

namespace mpsfm {

// ---- declarations of the launch wrappers (ba_kernels.hip, dense_chol.hip) ------------------------
void init_tile_tables(hipStream_t);
void launch_track_sweep(const SweepArgs&, int nchunks, bool diag_only, hipStream_t);
void launch_update_sweep(const SweepArgs&, int nchunks, hipStream_t, const CamUpdArgs* cu = nullptr);
void launch_track_sweep_dense(const SweepArgs&, int nchunks, hipStream_t);
void launch_reduce_slabs(const RedDest* dests, int ndest, const int32_t* srcs, const double* slab, double* Sblk, double* gc, double* wv, double* diagU,
                         const LmCtl* ctl, hipStream_t);
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
void launch_assemble(const AssembleArgs&, hipStream_t);
void launch_dense_solve(double* A, double* work, int nt, int n, double* y, int* fail, hipStream_t, DenseOverlap* ov, const LevelPlanDev* lp,
                        const LmCtl* ctl = nullptr);
bool dense_level(const DenseOverlap* ov, const LevelPlanDev* lp);
int dense_plain_max_tiles();
int dense_inv_rows();
size_t dense_work_doubles(int nt);
double* dense_pinv(double* work, int nt, const DenseOverlap* ov, const LevelPlanDev* lp);

thread_local std::string g_err;
extern int g_dbg_flags;  // dense_chol.hip: bits 0-7 dense-solve ablations, bits 8-15 track-sweep ablations
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
// the single-launch solver's skew hook (mpsfm_debug_local_skew): process-wide like g_dbg_flags, read when a solve is launched
static int32_t g_skew_chunk = 0, g_skew_mask = 0;
static int64_t g_skew_ticks = 0;

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return fail(MPSFM_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

// ---- caching device allocator (declared in common.h) ---------------------------------------------------
namespace {
struct DevCache {
  static constexpr size_t kCap = (size_t)6 << 30;       // cached (free) bytes kept per device
  std::mutex mu;
  std::multimap<size_t, void*> free_blocks[16];
  std::unordered_map<void*, std::pair<size_t, int>> live;  // pointer -> (block size, device)
  size_t cached[16] = {};
  static size_t block_size(size_t n) {  // 1/8-of-a-power-of-two granularity: sizes that differ a little share blocks
    n = std::max<size_t>(n, 256);
    size_t p = 256;
    while (p < n) p <<= 1;
    const size_t step = std::max<size_t>(p >> 3, 256);
    return (n + step - 1) / step * step;
  }
  void drop_all(int dev) {
    for (auto& kv : free_blocks[dev]) (void)hipFree(kv.second);
    free_blocks[dev].clear();
    cached[dev] = 0;
  }
  void* alloc(size_t bytes) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    dev = std::min(std::max(dev, 0), 15);
    const size_t bs = block_size(bytes);
    std::lock_guard<std::mutex> lk(mu);
    auto it = free_blocks[dev].lower_bound(bs);
    if (it != free_blocks[dev].end() && it->first <= bs + bs / 4) {
      void* p = it->second;
      const size_t got = it->first;
      free_blocks[dev].erase(it);
      cached[dev] -= got;
      live[p] = {got, dev};
      poison(p, got);
      return p;
    }
    void* p = nullptr;
    if (hipMalloc(&p, bs) != hipSuccess) {
      (void)hipGetLastError();
      drop_all(dev);  // give the cached blocks back and try once more
      if (hipMalloc(&p, bs) != hipSuccess) return nullptr;
    }
    live[p] = {bs, dev};
    poison(p, bs);
    return p;
  }
  // MPSFM_POISON=1 (tests): every block handed out is filled with 0xFF bytes (NaNs / huge indices), so a kernel
  // that reads memory nobody initialised fails loudly instead of finding the zeros a fresh hipMalloc often has
  static void poison(void* p, size_t n) {
    static const bool on = [] { const char* e = std::getenv("MPSFM_POISON"); return e && std::atoi(e) != 0; }();
    if (!on) return;
    (void)hipMemset(p, 0xFF, n);
    (void)hipDeviceSynchronize();
  }
  void release(void* p) {
    if (!p) return;
    std::lock_guard<std::mutex> lk(mu);
    auto it = live.find(p);
    if (it == live.end()) { (void)hipFree(p); return; }
    const size_t bs = it->second.first;
    const int dev = it->second.second;
    live.erase(it);
    if (cached[dev] + bs > kCap) { (void)hipFree(p); return; }
    free_blocks[dev].emplace(bs, p);
    cached[dev] += bs;
  }
};
DevCache& dev_cache() {
  static DevCache* c = new DevCache();  // never destroyed: the HIP runtime may be gone at static-destruction time
  return *c;
}
}  // namespace
void* cached_malloc(size_t bytes) { return dev_cache().alloc(bytes); }
void cached_free(void* p) { dev_cache().release(p); }

// Streams, events and the small pinned scalar block of a handle are recycled the same way: creating and
// destroying them costs more than a whole solve of a small problem.  Per device; never destroyed.
namespace {
struct HandleResources {
  std::mutex mu;
  std::vector<hipStream_t> streams[16];
  std::vector<hipEvent_t> timing_events[16], plain_events[16];
  std::vector<void*> pinned[16];  // blocks of kPinnedBytes
  static constexpr size_t kPinnedBytes = 4096;
  static int dev() { int d = 0; (void)hipGetDevice(&d); return std::min(std::max(d, 0), 15); }
};
HandleResources& pool() { static HandleResources* r = new HandleResources(); return *r; }
}  // namespace
hipError_t pooled_stream(hipStream_t* s) {
  HandleResources& R = pool();
  { std::lock_guard<std::mutex> lk(R.mu); auto& v = R.streams[R.dev()]; if (!v.empty()) { *s = v.back(); v.pop_back(); return hipSuccess; } }
  return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}
void release_stream(hipStream_t s) {
  if (!s) return;
  HandleResources& R = pool();
  std::lock_guard<std::mutex> lk(R.mu);
  R.streams[R.dev()].push_back(s);
}
static hipError_t pooled_event(hipEvent_t* e, bool timing) {
  HandleResources& R = pool();
  {
    std::lock_guard<std::mutex> lk(R.mu);
    auto& v = timing ? R.timing_events[R.dev()] : R.plain_events[R.dev()];
    if (!v.empty()) { *e = v.back(); v.pop_back(); return hipSuccess; }
  }
  return timing ? hipEventCreate(e) : hipEventCreateWithFlags(e, hipEventDisableTiming);
}
static void release_event(hipEvent_t e, bool timing) {
  if (!e) return;
  HandleResources& R = pool();
  std::lock_guard<std::mutex> lk(R.mu);
  (timing ? R.timing_events[R.dev()] : R.plain_events[R.dev()]).push_back(e);
}
static hipError_t pooled_pinned(void** p) {
  HandleResources& R = pool();
  { std::lock_guard<std::mutex> lk(R.mu); auto& v = R.pinned[R.dev()]; if (!v.empty()) { *p = v.back(); v.pop_back(); return hipSuccess; } }
  return hipHostMalloc(p, HandleResources::kPinnedBytes, hipHostMallocDefault);
}
static void release_pinned(void* p) {
  if (!p) return;
  HandleResources& R = pool();
  std::lock_guard<std::mutex> lk(R.mu);
  R.pinned[R.dev()].push_back(p);
}

// ---- RCCL, loaded at run time (no link-time dependency: single-GPU users never touch it) -----------------------------
// The four entry points the landmark-sharded solve needs.  dlopen finds the library already in the process (torch
// ships one) or the system's /opt/rocm copy.
namespace {
struct Rccl {
  typedef struct { char internal[128]; } UniqueId;
  int (*GetUniqueId)(UniqueId*) = nullptr;
  int (*CommInitRank)(void**, int, UniqueId, int) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  bool ok = false;
  std::string why;
  Rccl() {
    void* lib = nullptr;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (lib) break;
    }
    if (!lib) { why = std::string("librccl not found: ") + (dlerror() ? dlerror() : ""); return; }
    GetUniqueId = (int (*)(UniqueId*))dlsym(lib, "ncclGetUniqueId");
    CommInitRank = (int (*)(void**, int, UniqueId, int))dlsym(lib, "ncclCommInitRank");
    AllReduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(lib, "ncclAllReduce");
    CommDestroy = (int (*)(void*))dlsym(lib, "ncclCommDestroy");
    GetErrorString = (const char* (*)(int))dlsym(lib, "ncclGetErrorString");
    ok = GetUniqueId && CommInitRank && AllReduce && CommDestroy;
    if (!ok) why = "librccl lacks ncclGetUniqueId / ncclCommInitRank / ncclAllReduce / ncclCommDestroy";
  }
};
Rccl& rccl() { static Rccl* r = new Rccl(); return *r; }
constexpr int kNcclDouble = 8, kNcclSum = 0;  // ncclFloat64, ncclSum (rccl.h)
}  // namespace

template <typename T>
static int dev_alloc(T** p, size_t count) {
  if (count == 0) count = 1;
  *p = (T*)cached_malloc(count * sizeof(T));
  if (!*p) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  return 0;
}
// Uploads of caller / table memory go through a process-wide pinned staging buffer (two halves, the host copy
// into one overlaps the DMA out of the other).  Handing pageable memory to hipMemcpy directly makes the
// runtime pin and later unpin every source range: measured 17 ms of stall after a 40 MB table upload.
// pageable -> pinned copy of one staging half: a single thread's memcpy (~20 GB/s here) is what bounded the uploads, not the bus;
// a few host threads in parallel (defined behind run_parts)
static void staged_copy(char* dst, const char* src, size_t n);
struct Stager {
  static constexpr size_t kHalf = (size_t)8 << 20;
  std::mutex mu;
  char* buf = nullptr;
  hipStream_t st = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool busy[2] = {false, false};
  int next = 0;
  int init() {
    if (buf) return 0;  // set last: a partly created stager is torn down again and the next call retries
    char* b = nullptr;
    if (hipHostMalloc((void**)&b, 2 * kHalf, hipHostMallocDefault) != hipSuccess) return fail(MPSFM_ENOMEM, "hipHostMalloc (staging) failed");
    const bool ok = hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess &&
                    hipEventCreateWithFlags(&ev[0], hipEventDisableTiming) == hipSuccess &&
                    hipEventCreateWithFlags(&ev[1], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
      for (auto& e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
      if (st) (void)hipStreamDestroy(st);
      st = nullptr;
      (void)hipHostFree(b);
      return fail(MPSFM_EHIP, "creating the staging stream / events failed");
    }
    buf = b;
    return 0;
  }
  // blocking from the caller's point of view only at drain()
  int push(void* dst, const void* src, size_t bytes) {
    const char* s = (const char*)src;
    char* d = (char*)dst;
    while (bytes > 0) {
      const size_t n = std::min(bytes, kHalf);
      const int hf = next;
      next ^= 1;
      if (busy[hf]) { HIP_TRY(hipEventSynchronize(ev[hf])); busy[hf] = false; }
      staged_copy(buf + (size_t)hf * kHalf, s, n);
      HIP_TRY(hipMemcpyAsync(d, buf + (size_t)hf * kHalf, n, hipMemcpyHostToDevice, st));
      HIP_TRY(hipEventRecord(ev[hf], st));
      busy[hf] = true;
      s += n; d += n; bytes -= n;
    }
    return 0;
  }
  int drain() {
    HIP_TRY(hipStreamSynchronize(st));
    busy[0] = busy[1] = false;
    return 0;
  }
};
static Stager g_stagers[16];  // one per device ordinal
static Stager& stager() {
  int dev = 0;
  (void)hipGetDevice(&dev);
  return g_stagers[(size_t)std::min(std::max(dev, 0), 15)];
}

// for the other translation units (int_kernels.hip): queue a staged upload / wait for everything queued
int staged_upload(void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return 0;
  Stager& G = stager();
  std::lock_guard<std::mutex> lk(G.mu);
  if (int rc = G.init()) return rc;
  return G.push(dst, src, bytes);
}
int staged_drain() {
  Stager& G = stager();
  std::lock_guard<std::mutex> lk(G.mu);
  return G.buf ? G.drain() : 0;
}

// staged copy of host memory to the device, complete on return
static int staged_h2d(void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return 0;
  Stager& G = stager();
  std::lock_guard<std::mutex> lk(G.mu);
  if (int rc = G.init()) return rc;
  if (int rc = G.push(dst, src, bytes)) return rc;
  return G.drain();
}

template <typename T>
static int dev_upload(T** p, const std::vector<T>& v) {
  int rc = dev_alloc(p, v.size());
  if (rc) return rc;
  if (v.empty()) return 0;
  Stager& G = stager();
  std::lock_guard<std::mutex> lk(G.mu);
  if ((rc = G.init())) return rc;
  return G.push(*p, v.data(), v.size() * sizeof(T));  // build() drains once after the last table
}
template <typename T>
static int dev_upload(T** p, HostBuf<T>& v) {
  int rc = dev_alloc(p, v.size());
  if (rc) return rc;
  if (v.size() == 0) return 0;
  Stager& G = stager();
  std::lock_guard<std::mutex> lk(G.mu);
  if ((rc = G.init())) return rc;
  return G.push(*p, v.data(), v.size() * sizeof(T));
}
static int drain_uploads() {
  Stager& G = stager();
  std::lock_guard<std::mutex> lk(G.mu);
  return G.buf ? G.drain() : 0;
}

}  // namespace mpsfm

using namespace mpsfm;

struct mpsfm_ba_handle {
  int device = 0;
  hipStream_t stream = nullptr;
  void* comm = nullptr;  // ncclComm_t of a landmark-sharded run with use_rccl
  DenseOverlap ov;  // second stream for the dense factorisation in outer panels (MPSFM_CHOL_NB)
  SPattern spat;                    // which blocks of S exist: block skyline or index form (up to kIndexMaxSlots slots), host copies
  int32_t* d_sky_first = nullptr;
  int64_t* d_sky_start = nullptr;
  int32_t* d_sky_index = nullptr;
  CholPlan plan;                    // camera order, tile elimination tree and launch tables of the dense factorisation (chol_plan.h)
  LevelPlanDev lp;
  CholItem* d_lp_items = nullptr;
  uint8_t* d_lp_live = nullptr;
  int32_t* d_lp_col_slot = nullptr;
  int32_t *d_lp_srcs = nullptr, *d_lp_rows = nullptr, *d_lp_struct_start = nullptr, *d_lp_struct_rows = nullptr, *d_lp_back_cols = nullptr, *d_lp_asm = nullptr;
  std::vector<int32_t> nat_slot;    // variable camera in the caller's order -> slot (the accessors of S and y speak the caller's order)
  int n_user = 0;                   // 6 x variable cameras: the reduced dimension the caller sees and the length of the slot-indexed vectors (n counts the
                                    // system's columns incl. the alignment padding)
  bool own_stream = false;
  mpsfm_ba_options opt{};
  LossParams loss{};
  // sizes
  int nc = 0, np_user = 0;
  int64_t np = 0, np_chunked = 0;   // re-ordered landmarks (all referenced) / those inside chunks
  int64_t nrec = 0, nfixed = 0, nblocks_total = 0, nblocks_reduced = 0;
  double nblocks_global = 0, nblocks_reduced_global = 0, nvarpts_global = 0;
  int ncv = 0, n = 0, nt = 0, nchunks = 0, nlong = 0;
  int n_dense = 0;                  // chunks [0, n_dense) are swept by k_track_sweep_dense, the rest by the general kernel
  double* d_slab = nullptr;         // slabs of the dense chunks
  RedDest* d_red_dests = nullptr;   // slab reduction: destination parts and their sources
  int32_t* d_red_srcs = nullptr;
  int n_red_dests = 0;
  int64_t n_red_srcs = 0, n_chunk_cams = 0, n_blk_desc = 0, n_blk_ent_start = 0, n_ents = 0;  // table sizes (diagnostics: mpsfm_debug_table)
  bool built_on_device = false;
  LongHdr* d_lhdr = nullptr;
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
  ChunkHdr* d_chunks = nullptr;
  int32_t *d_chunk_cams = nullptr, *d_blk_ent_start = nullptr;
  uint32_t *d_blk_desc = nullptr, *d_ents = nullptr;
  RecTablesDev rt;           // record and fixed-record tables
  // reduced buffer: Sblk | gc | wv | diagU | scalars
  double* d_red = nullptr;
  double *d_Sblk = nullptr, *d_gc = nullptr, *d_wv = nullptr, *d_diagU = nullptr, *d_redsc = nullptr;
  double *d_part = nullptr, *d_part2 = nullptr, *d_scal = nullptr, *d_costpart = nullptr;
  double* h_scal = nullptr;  // pinned
  LmCtl* d_ctl = nullptr;    // Levenberg-Marquardt control block (device) and the two pinned slots its copies land in
  LmCtl* h_ctl = nullptr;
  hipEvent_t ev2[4] = {nullptr, nullptr, nullptr, nullptr};  // second set of phase events (two iterations are in flight)
  double *d_A = nullptr, *d_yc = nullptr, *d_dwork = nullptr;
  int* d_fail = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  double last_radius = 1e4;
  bool scales_ready = false;
  // single-launch solver of small problems (local_lm.hip): two accumulators | barrier words + clocks | per-iteration heads
  bool local_ok = false;
  double* d_local_acc = nullptr;
  int64_t* d_local_sync = nullptr;   // [0]: two 32-bit barrier words, [1..4]: phase clocks
  LmHead* d_local_log = nullptr;
  int local_log_cap = 0;
};

namespace mpsfm {

static void free_handle(mpsfm_ba_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  // Error returns of the solve (a failing all-reduce hook, a HIP error) and reset_state + destroy leave copies and
  // kernels in flight: both streams must be idle before the blocks go back to the process-wide cache, where a
  // handle on another stream or host thread may receive them at once.
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->ov.s2) (void)hipStreamSynchronize(h->ov.s2);
  void* ptrs[] = {h->d_q, h->d_t, h->d_q2, h->d_t2, h->d_q0, h->d_t0, h->d_pts, h->d_pts2, h->d_pts0, h->d_intr, h->d_cmask,
                  h->d_cs, h->d_camtab, h->d_camtab2, h->d_intr_idx, h->d_cam_slot, h->d_ps, h->d_diagV, h->d_chunks,
                  h->d_chunk_cams, h->d_blk_ent_start, h->d_blk_desc, h->d_ents, h->d_red, h->d_part, h->d_part2, h->d_scal, h->d_costpart, h->d_A, h->d_yc, h->d_dwork, h->d_fail, h->d_lhdr, h->d_wl, h->d_slab, h->d_red_dests, h->d_red_srcs,
                  h->d_sky_first, h->d_sky_start, h->d_sky_index,
                  h->d_local_acc, h->d_local_sync, h->d_local_log, h->d_perm, h->d_user_pts, h->d_cam_of_slot,
                  h->d_lp_items, h->d_lp_srcs, h->d_lp_rows, h->d_lp_struct_start, h->d_lp_struct_rows, h->d_lp_back_cols, h->d_lp_asm, h->d_lp_live, h->d_lp_col_slot};
  for (void* p : ptrs) cached_free(p);
  h->rt.release();
  if (h->comm) (void)rccl().CommDestroy(h->comm);
  release_pinned(h->h_scal);
  release_pinned(h->h_ctl);
  cached_free(h->d_ctl);
  for (auto& e : h->ev2) release_event(e, true);
  for (auto& e : h->ev) release_event(e, true);
  for (auto& e : h->ov.evF) release_event(e, false);
  for (auto& e : h->ov.evB) release_event(e, false);
  release_stream(h->ov.s2);
  if (h->own_stream) release_stream(h->stream);
  delete h;
}

static int check_problem(const mpsfm_ba_problem* P) {
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

static bool sharded(const mpsfm_ba_handle* h) { return h->opt.allreduce != nullptr || h->comm != nullptr; }
static int rccl_allreduce(mpsfm_ba_handle* h, double* dbuf, int64_t count) {
  const int rc = rccl().AllReduce(dbuf, dbuf, (size_t)count, kNcclDouble, kNcclSum, h->comm, h->stream);
  if (rc != 0) return fail(MPSFM_ECOMM, std::string("ncclAllReduce: ") + (rccl().GetErrorString ? rccl().GetErrorString(rc) : "failed"));
  return 0;
}
static int allreduce_host(mpsfm_ba_handle* h, double* buf, int64_t count) {
  if (count <= 0) return 0;
  if (h->comm) {  // host values travel through a device scratch block
    double* d = (double*)cached_malloc(sizeof(double) * (size_t)count);
    if (!d) return fail(MPSFM_ENOMEM, "hipMalloc failed");
    int rc = 0;
    if (hipMemcpyAsync(d, buf, sizeof(double) * (size_t)count, hipMemcpyHostToDevice, h->stream) != hipSuccess) rc = fail(MPSFM_EHIP, "hipMemcpyAsync failed");
    if (!rc) rc = rccl_allreduce(h, d, count);
    if (!rc && hipMemcpyAsync(buf, d, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, h->stream) != hipSuccess) rc = fail(MPSFM_EHIP, "hipMemcpyAsync failed");
    (void)hipStreamSynchronize(h->stream);
    cached_free(d);
    return rc;
  }
  if (!h->opt.allreduce) return 0;
  if (h->opt.allreduce(h->opt.allreduce_user, buf, count, 0, nullptr)) return fail(MPSFM_ECOMM, "all-reduce hook failed (host buffer)");
  return 0;
}
static int allreduce_dev(mpsfm_ba_handle* h, double* buf, int64_t count) {
  if (count <= 0) return 0;
  if (h->comm) return rccl_allreduce(h, buf, count);
  if (!h->opt.allreduce) return 0;
  if (h->opt.allreduce(h->opt.allreduce_user, buf, count, 1, (void*)h->stream)) return fail(MPSFM_ECOMM, "all-reduce hook failed (device buffer)");
  return 0;
}

static void staged_copy(char* dst, const char* src, size_t n) {
  constexpr size_t kGrain = (size_t)1 << 20;
  static const int max_threads = [] { const char* e = std::getenv("MPSFM_STAGE_THREADS"); return e ? std::max(std::atoi(e), 1) : 6; }();
  const int parts = (int)std::min<size_t>((size_t)std::min(host_threads(), max_threads), n / kGrain);
  if (parts <= 1) { std::memcpy(dst, src, n); return; }
  run_parts(parts, [&](int t, int np) {
    const size_t a = (n * (size_t)t / (size_t)np) & ~(size_t)63, b = t + 1 == np ? n : ((n * (size_t)(t + 1) / (size_t)np) & ~(size_t)63);
    std::memcpy(dst + a, src + a, b - a);
  });
}

static void level_plan_flags(const CholPlan& PL, LevelPlanDev& D) { D.valid = PL.nt >= 1 && PL.nlevels >= 1; D.use_pinv = PL.use_pinv; }
// the ten numbers of mpsfm_ba_dense_plan; `work`: the dense workspace (only compared with NULL)
static void dense_plan_numbers(int ncv, int nt, const CholPlan& P, const DenseOverlap& ov, const LevelPlanDev& lp, double* work, int64_t sblk, int64_t v[10]) {
  const bool level = dense_level(&ov, &lp);
  const bool pinv = level && dense_pinv(work, nt, &ov, &lp) != nullptr;
  const int64_t w[10] = {ncv, nt, level ? P.nlevels : nt, P.nd_depth, pinv ? 1 : 0, (int64_t)P.items.size(), P.products, P.roles, sblk,
                         pinv ? 1 : (level ? P.nlevels : (nt + 3) / 4 + 1)};
  for (int i = 0; i < 10; ++i) v[i] = w[i];
}

// the tables of the level-scheduled factorisation (h->plan) to the device
static int upload_plan(mpsfm_ba_handle* h, int64_t nblk) {
  const CholPlan& PL = h->plan;
  int rc2 = 0;
  if ((rc2 = dev_upload(&h->d_lp_items, PL.items))) return rc2;
  if ((rc2 = dev_upload(&h->d_lp_srcs, PL.srcs))) return rc2;
  if ((rc2 = dev_upload(&h->d_lp_rows, PL.rows))) return rc2;
  if ((rc2 = dev_upload(&h->d_lp_struct_start, PL.struct_start))) return rc2;
  if ((rc2 = dev_upload(&h->d_lp_struct_rows, PL.struct_rows))) return rc2;
  if ((rc2 = dev_upload(&h->d_lp_back_cols, PL.back_cols))) return rc2;
  if ((rc2 = dev_upload(&h->d_lp_asm, PL.asm_tiles))) return rc2;
  if ((rc2 = dev_upload(&h->d_lp_col_slot, PL.slot_of_col))) return rc2;
  {
    std::vector<uint8_t> live((size_t)(PL.nt + 1) * (size_t)(PL.nt + 2) / 2, 0);
    for (int32_t id : PL.asm_tiles) live[(size_t)id] = 1;
    if ((rc2 = dev_upload(&h->d_lp_live, live))) return rc2;
  }
  LevelPlanDev& D = h->lp;
  level_plan_flags(PL, D);
  D.d_items = h->d_lp_items; D.d_srcs = h->d_lp_srcs; D.d_rows = h->d_lp_rows;
  D.d_struct_start = h->d_lp_struct_start; D.d_struct_rows = h->d_lp_struct_rows; D.d_back_cols = h->d_lp_back_cols;
  D.d_asm_tiles = h->d_lp_asm; D.d_tile_live = h->d_lp_live; D.d_col_slot = PL.slot_of_col.empty() ? nullptr : h->d_lp_col_slot; D.n_asm = (int32_t)PL.asm_tiles.size(); D.nlevels = PL.nlevels;
  D.h_launch_start = PL.launch_start.data(); D.h_back_start = PL.back_start.data();
  if (h->opt.verbose >= 2)
    std::fprintf(stderr, "[mpsfm_ba] build: camera order: %s (depth %d), %d slots for %d cameras, %d tile columns in %d levels, %lld tile products, %lld inverse roles, %d blocks of S\n",
                 PL.nd_depth < 0 ? "caller's" : "nested dissection", PL.nd_depth, PL.nslots, PL.ncv, PL.nt, PL.nlevels, (long long)PL.products, (long long)PL.roles, (int)nblk);
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
static int pair_tables_of_device_build(mpsfm_ba_handle* h, const mpsfm_ba_problem* P, const RecTablesDev& rt, HostTables& T, const Lap& lap) {
  std::vector<ChunkHdr>& chunks = T.chunks;
  size_t g0 = 0;
  while (g0 < chunks.size() && chunks[g0].dense) ++g0;
  T.blk_ent_start.assign(g0, 0);
  if (g0 == chunks.size()) return 0;
  const int64_t r0 = chunks[g0].rec0, k0 = chunks[g0].pt0, nrg = T.nrec - r0, nkg = T.np_chunked - k0;
  std::vector<uint32_t> rm((size_t)std::max<int64_t>(nrg, 1));
  std::vector<uint16_t> kvs((size_t)std::max<int64_t>(nkg, 1));
  std::vector<int32_t> prs((size_t)std::max<int64_t>(nkg, 1));
  HIP_TRY(hipMemcpyAsync(rm.data(), rt.rec_meta + r0, 4 * (size_t)nrg, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(kvs.data(), rt.pt_kv + k0, 2 * (size_t)nkg, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(prs.data(), rt.pt_rec_start + k0, 4 * (size_t)nkg, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
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

// the block pattern of S and the tables of the dense factorisation (h->spat, h->plan) to the device
static int upload_pattern(mpsfm_ba_handle* h, bool use_graph) {
  if (use_graph) {
    if (int rc = dev_upload(&h->d_sky_index, h->spat.sky_index)) return rc;
  } else {
    if (int rc = dev_upload(&h->d_sky_first, h->spat.sky_first)) return rc;
    if (int rc = dev_upload(&h->d_sky_start, h->spat.sky_start)) return rc;
  }
  return upload_plan(h, h->spat.nblk);
}

// the record and fixed-record tables of the host build to the device
static int upload_record_tables(HostTables& T, RecTablesDev& rt) {
  int rc = 0;
  if ((rc = dev_upload(&rt.rec_cam, T.rec_cam))) return rc;
  if ((rc = dev_upload(&rt.rec_pt, T.rec_pt))) return rc;
  if ((rc = dev_upload(&rt.rec_meta, T.rec_meta))) return rc;
  if ((rc = dev_upload(&rt.rec_xy, T.rec_xy))) return rc;
  if ((rc = dev_upload(&rt.rec_d, T.rec_d))) return rc;
  if ((rc = dev_upload(&rt.rec_m, T.rec_m))) return rc;
  if ((rc = dev_upload(&rt.rec_a, T.rec_a))) return rc;
  if ((rc = dev_upload(&rt.pt_rec_start, T.pt_rec_start))) return rc;
  if ((rc = dev_upload(&rt.pt_kv, T.pt_kv))) return rc;
  if ((rc = dev_upload(&rt.fx_cam, T.fx_cam))) return rc;
  if ((rc = dev_upload(&rt.fx_pt, T.fx_pt))) return rc;
  if ((rc = dev_upload(&rt.fx_meta, T.fx_meta))) return rc;
  if ((rc = dev_upload(&rt.fx_xy, T.fx_xy))) return rc;
  if ((rc = dev_upload(&rt.fx_d, T.fx_d))) return rc;
  if ((rc = dev_upload(&rt.fx_m, T.fx_m))) return rc;
  return dev_upload(&rt.fx_a, T.fx_a);
}

// Everything the solve reads to the device.  `DB`: the device build's output (T is its host part) or, after a host build, empty;
// `devb` forms the slab reduction tables on the device when `R` came without them (R.dests empty, R.diag_block set).
static int upload_tables(mpsfm_ba_handle* h, const mpsfm_ba_problem* P, const CameraLayout& cams, DevBuildOut& DB, SlabTables& R, DevBuilder* devb,
                         bool slab_tables_on_device) {
  HostTables& T = DB.t;
  const int nc = P->n_cams;
  int rc = 0;
  std::vector<double> intr(P->cam_intr, P->cam_intr + (size_t)P->n_intr * 4);
  std::vector<int32_t> intr_idx(P->cam_intr_idx, P->cam_intr_idx + nc);
  if ((rc = dev_upload(&h->d_intr, intr))) return rc;
  if ((rc = dev_upload(&h->d_intr_idx, intr_idx))) return rc;
  if ((rc = dev_upload(&h->d_cmask, cams.cmask))) return rc;
  if ((rc = dev_upload(&h->d_cam_slot, h->cam_slot_h))) return rc;
  if ((rc = dev_upload(&h->d_cam_of_slot, cam_of_slot_table(cams)))) return rc;
  if ((rc = dev_upload(&h->d_chunks, T.chunks))) return rc;
  if ((rc = dev_upload(&h->d_chunk_cams, T.chunk_cams))) return rc;
  if (h->np > 0 && h->np == (int64_t)h->np_user) {
    if ((rc = dev_upload(&h->d_perm, h->perm))) return rc;
    if ((rc = dev_alloc(&h->d_user_pts, (size_t)h->np * 3))) return rc;
  }
  if (h->built_on_device) {  // the device build's tables are where they belong
    h->rt = DB.rt;
    DB.rt = RecTablesDev{};
    DB.release();  // the device copies of chunks / camera lists: the host copies (slab offsets added) are uploaded above
  } else if ((rc = upload_record_tables(T, h->rt))) return rc;
  if ((rc = dev_upload(&h->d_lhdr, T.lhdr))) return rc;
  if ((rc = dev_alloc(&h->d_wl, (size_t)std::max<int64_t>(T.wl_rows, 1) * 18))) return rc;
  h->n_blk_desc = (int64_t)T.blk_desc.size(); h->n_blk_ent_start = (int64_t)T.blk_ent_start.size(); h->n_ents = (int64_t)T.ents.size();
  if ((rc = dev_upload(&h->d_blk_desc, T.blk_desc))) return rc;
  if ((rc = dev_upload(&h->d_blk_ent_start, T.blk_ent_start))) return rc;
  if ((rc = dev_upload(&h->d_ents, T.ents))) return rc;
  int32_t* d_diag_block = nullptr;
  if (!slab_tables_on_device) {
    if ((rc = dev_upload(&h->d_red_dests, R.dests))) return rc;
    if ((rc = dev_upload(&h->d_red_srcs, R.srcs))) return rc;
  } else if ((rc = dev_upload(&d_diag_block, R.diag_block))) return rc;
  if ((rc = dev_alloc(&h->d_slab, (size_t)std::max<int64_t>(R.slab_units, 1) * 18))) return rc;

  if ((rc = drain_uploads())) { cached_free(d_diag_block); return rc; }
  if (slab_tables_on_device) {
    const BlockSky sky{h->d_sky_first, h->d_sky_start, h->d_sky_index, h->ncv};
    int32_t nd = 0; int64_t ns = 0;
    rc = devb->slab_tables(h->d_chunks, h->n_dense, h->d_chunk_cams, sky, h->spat.nblk, h->ncv, d_diag_block, &h->d_red_dests, &nd, &h->d_red_srcs, &ns);
    HIP_TRY(hipStreamSynchronize(h->stream));  // d_diag_block goes back to the process-wide cache
    cached_free(d_diag_block);
    if (rc) return rc;
    h->n_red_dests = nd; h->n_red_srcs = ns;
  }
  return 0;
}

// state, reduced system, dense workspace, scalars, events; the single-launch solver's buffers where it applies
static int alloc_work_buffers(mpsfm_ba_handle* h, const BuildOptions& opt) {
  int rc = 0;
  const size_t ncs = (size_t)std::max(h->nc, 1), nps = (size_t)std::max<int64_t>(h->np, 1);
  for (double** p : {&h->d_q, &h->d_q2, &h->d_q0}) if ((rc = dev_alloc(p, ncs * 4))) return rc;
  for (double** p : {&h->d_t, &h->d_t2, &h->d_t0}) if ((rc = dev_alloc(p, ncs * 3))) return rc;
  for (double** p : {&h->d_pts, &h->d_pts2, &h->d_pts0, &h->d_ps, &h->d_diagV}) if ((rc = dev_alloc(p, nps * 3))) return rc;
  if ((rc = dev_alloc(&h->d_cs, ncs * 6))) return rc;
  if ((rc = dev_alloc(&h->d_camtab, ncs * kCamRec))) return rc;
  if ((rc = dev_alloc(&h->d_camtab2, ncs * kCamRec))) return rc;
  h->sblk_count = h->spat.nblk * 36;
  h->red_count = h->sblk_count + 3 * (int64_t)h->n_user + SC_COUNT;
  if ((rc = dev_alloc(&h->d_red, (size_t)h->red_count))) return rc;
  h->d_Sblk = h->d_red; h->d_gc = h->d_red + h->sblk_count; h->d_wv = h->d_gc + h->n_user; h->d_diagU = h->d_wv + h->n_user;
  h->d_redsc = h->d_diagU + h->n_user;
  if ((rc = dev_alloc(&h->d_part, (size_t)std::max(h->nchunks + h->nlong, 1) * 4 * 2))) return rc;  // (second half: the single launch's odd iterations)
  if ((rc = dev_alloc(&h->d_part2, (size_t)std::max(h->nchunks + h->nlong, 1) * 8))) return rc;
  if ((rc = dev_alloc(&h->d_scal, (size_t)U_COUNT))) return rc;
  if ((rc = dev_alloc(&h->d_costpart, (size_t)1024 * 4))) return rc;
  static_assert(sizeof(double) * U_COUNT * 2 <= HandleResources::kPinnedBytes, "pinned scalar block too small");
  HIP_TRY(pooled_pinned((void**)&h->h_scal));
  static_assert(sizeof(LmCtl) * 2 <= HandleResources::kPinnedBytes, "pinned block too small for two control-block copies");
  HIP_TRY(pooled_pinned((void**)&h->h_ctl));
  if ((rc = dev_alloc(&h->d_ctl, 1))) return rc;
  for (auto& e : h->ev2) HIP_TRY(pooled_event(&e, true));
  const size_t ntiles = (size_t)(h->nt + 1) * (h->nt + 2) / 2;
  if ((rc = dev_alloc(&h->d_A, ntiles * 1024))) return rc;
  if ((rc = dev_alloc(&h->d_dwork, dense_work_doubles(h->nt)))) return rc;
  if ((rc = dev_alloc(&h->d_yc, (size_t)std::max(h->n_user, 1)))) return rc;
  if ((rc = dev_alloc(&h->d_fail, 1))) return rc;
  HIP_TRY(hipMemsetAsync(h->d_fail, 0, sizeof(int), h->stream));
  for (auto& e : h->ev) HIP_TRY(pooled_event(&e, true));
  opt.apply_dense(h->nt, h->plan, h->ov);
  if (h->nt > 64 || h->ov.nb > 0) {
    HIP_TRY(pooled_stream(&h->ov.s2));
    for (auto& e : h->ov.evF) HIP_TRY(pooled_event(&e, false));
    for (auto& e : h->ov.evB) HIP_TRY(pooled_event(&e, false));
  }
  // Small problems (local bundle adjustment): the whole trust-region loop in one cooperative launch, one workgroup per chunk
  h->local_ok = false;
  if (opt.local_lm && !sharded(h) && h->nlong == 0 && h->nchunks > 0 && h->n_dense == h->nchunks && h->ncv >= 1 && h->ncv <= kLocalCams &&
      h->n_user == 6 * h->ncv && h->nchunks <= local_lm_max_chunks(h->device)) {
    h->local_log_cap = std::max(h->opt.max_num_iterations, 0) + 2;
    if ((rc = dev_alloc(&h->d_local_acc, (size_t)2 * kLocalAccDoubles))) return rc;
    if ((rc = dev_alloc(&h->d_local_sync, (size_t)16))) return rc;
    if ((rc = dev_alloc(&h->d_local_log, (size_t)h->local_log_cap))) return rc;
    h->local_ok = true;
  }
  HIP_TRY(hipMemsetAsync(h->d_ps, 0, nps * 3 * sizeof(double), h->stream));
  HIP_TRY(hipMemsetAsync(h->d_yc, 0, (size_t)std::max(h->n_user, 1) * sizeof(double), h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  init_tile_tables(h->stream);
  return 0;
}

// Build the re-ordered, chunked record tables and upload everything: the list of the build's phases.
static int build(mpsfm_ba_handle* h, const mpsfm_ba_problem* P) {
  const int nc = P->n_cams;
  auto t_prev = std::chrono::steady_clock::now();
  const Lap lap = [&](const char* what) {
    if (h->opt.verbose < 2) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[mpsfm_ba] build: %-28s %8.2f ms\n", what, 1e3 * std::chrono::duration<double>(now - t_prev).count());
    t_prev = now;
  };
  h->nc = nc; h->np_user = P->n_pts;
  h->loss.reproj_type = P->reproj_loss_type; h->loss.reproj_a = P->reproj_loss_scale;
  h->loss.reproj_mag = P->reproj_loss_magnitude; h->loss.depth_type = P->depth_loss_type;
  BuildOptions opt = BuildOptions::from_environment();
  // the exchanges of a landmark-sharded build (block counts, graph union, totals, skyline bisection) sum host values over the ranks
  const SumExchange exchange = sharded(h) ? SumExchange([h](double* buf, int64_t count) { return allreduce_host(h, buf, count); }) : SumExchange();

  // -- Device-side table build (build_dev.hip) where it applies: one rank, at most kIndexMaxSlots non-constant cameras, no
  //    landmark with more blocks than a chunk holds.  Stage 1 runs here (block counts per camera, blocks grouped by landmark,
  //    camera graph); stage 2 then stands in for the host phases.  MPSFM_DEV_BUILD=0: host.
  bool dev = false;
  std::unique_ptr<DevBuilder> devb;
  DevBuildOut DB;
  HostTables& T = DB.t;  // filled by either build
  std::vector<uint64_t> dev_gbits;
  std::vector<int32_t> prov((size_t)std::max(nc, 1), -1);  // provisional slots of the graph stage: the non-constant cameras in order
  int nprov = 0;
  for (int i = 0; i < nc; ++i) if (!P->pose_const[i]) prov[(size_t)i] = nprov++;
  const int dev_words = (nprov + 63) / 64;
  std::vector<double> cnt(nc + 1, 0.0);  // blocks per camera
  if (!sharded(h) && nprov <= kIndexMaxSlots && nc <= 8192 && P->n_obs + P->n_dobs > 0 && opt.dev_build && opt.chol_graph) {
    devb.reset(new DevBuilder());
    int64_t max_blocks = 0;
    if (int rc = devb->stage1(P, h->stream, prov, nprov, cnt, dev_gbits, dev_words, &max_blocks)) return rc;
    dev = max_blocks <= kObsMax;  // longer block lists may be long tracks: host build
    lap("device stage 1 (upload, group, graph)");
  } else {
    count_camera_blocks(P, cnt);
    if (exchange) if (int rc = exchange(cnt.data(), nc)) return rc;
  }
  CameraLayout cams;
  assign_camera_slots(P, cnt, opt, cams);
  h->n_user = 6 * cams.ncv_real;
  opt.set_chunk_caps(sharded(h), cams.ncv, P->n_obs);

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
    plan_camera_order(graph, opt, h->plan, cams);
    lap("camera order + factorisation plan");
  } else keep_caller_order(cams);
  h->cam_slot_h = cams.slot; h->nat_slot = cams.nat_slot;
  h->ncv = cams.ncv; h->n = cams.n; h->nt = cams.nt;

  // -- records, landmark order, chunks, pair tables
  if (dev) {
    const int rc2 = devb->stage2(cams.slot, opt.sweep_dense, opt.rec_cap, opt.pts_by_cams, DB);
    if (rc2 < 0) return rc2;
    if (rc2 == MPSFM_DEVBUILD_FALLBACK) {
      // long tracks: the host phases run after all — the grouping first, which was skipped (depths were validated by stage 1)
      DB.release();
      dev = false;
      if (int rc = group_blocks_by_landmark(P, false, groups)) return rc;
      lap("device build not applicable: host phases");
    } else {
      if (T.nrec > (int64_t)INT32_MAX) return fail(MPSFM_EUNSUPPORTED, "more than 2^31 records on one device");
      lap("device stage 2 (order, chunks, records)");
      if (int rc = pair_tables_of_device_build(h, P, DB.rt, T, lap)) return rc;
    }
  }
  if (!dev) if (int rc = build_record_tables(P, cams, opt, groups, T, lap)) return rc;
  h->built_on_device = dev;
  h->np = T.np; h->np_chunked = T.np_chunked; h->nfixed = T.nfixed; h->nrec = T.nrec;
  h->nchunks = (int)T.chunks.size(); h->nlong = (int)T.lhdr.size();
  h->nblocks_total = P->n_obs + P->n_dobs; h->nblocks_reduced = T.nblk_reduced;
  {
    double tot[3] = {(double)h->nblocks_total, (double)T.nblk_reduced, T.nvarpts};
    if (exchange) if (int rc = exchange(tot, 3)) return rc;
    h->nblocks_global = tot[0]; h->nblocks_reduced_global = tot[1]; h->nvarpts_global = tot[2];
  }
  lap("chunks + pair tables");
  if (h->opt.verbose >= 2 && !T.chunks.empty()) print_chunk_stats(T.chunks);

  // -- which 6x6 blocks of S exist, and the tables of the dense factorisation
  if (cams.use_graph) s_pattern_index(cams, h->plan, graph, h->spat);
  else if (int rc = s_pattern_skyline(cams, T, opt, exchange, h->opt.verbose >= 2, h->spat, h->plan)) return rc;
  if (int rc = upload_pattern(h, cams.use_graph)) return rc;

  // -- slabs of the dense chunks and the tables of their reduction; a device-built handle forms the tables on the device too
  //    (DevBuilder::slab_tables, behind the uploads).  MPSFM_SLAB_TABLES_HOST 1: host loop, 0: device kernels (tests), unset: by
  //    size — below ~500 chunks the host loop is quicker than the launches
  SlabTables slabs;
  if (int rc = assign_slabs(T.chunks, slabs)) return rc;
  h->n_dense = slabs.n_dense;
  const bool slab_tables_on_device = dev && h->n_dense > 0 && (opt.slab_tables_host == 0 || (opt.slab_tables_host < 0 && h->n_dense >= 512));
  if (int rc = slab_reduction_tables(T, cams, h->plan, h->spat, !slab_tables_on_device, slabs)) return rc;
  h->n_red_dests = (int)slabs.dests.size();
  h->n_red_srcs = (int64_t)slabs.srcs.size(); h->n_chunk_cams = (int64_t)T.chunk_cams.size();
  lap("slab reduction tables");

  h->perm.swap(T.order);
  if (int rc = upload_tables(h, P, cams, DB, slabs, devb.get(), slab_tables_on_device)) return rc;
  lap("upload tables");
  if (int rc = alloc_work_buffers(h, opt)) return rc;
  lap("allocate work buffers");
  return 0;
}

static int upload_state(mpsfm_ba_handle* h, const mpsfm_ba_state* st, bool as_initial) {
  if (!st || (h->nc > 0 && (!st->cam_quat_xyzw || !st->cam_t)) || (h->np > 0 && !st->pts)) return fail(MPSFM_EINVAL, "state is NULL");
  auto t_prev = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (h->opt.verbose < 2) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[mpsfm_ba] state: %-28s %8.2f ms\n", what, 1e3 * std::chrono::duration<double>(now - t_prev).count());
    t_prev = now;
  };
  // caller memory is pageable: staged copies (see Stager).  The handle's stream is idle between solves.
  HIP_TRY(hipStreamSynchronize(h->stream));
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
    HIP_TRY(hipMemcpyAsync(h->d_q0, h->d_q, sizeof(double) * 4 * h->nc, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->d_t0, h->d_t, sizeof(double) * 3 * h->nc, hipMemcpyDeviceToDevice, h->stream));
    if (h->np > 0) HIP_TRY(hipMemcpyAsync(h->d_pts0, h->d_pts, sizeof(double) * 3 * h->np, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    lap("keep initial state");
  }
  h->scales_ready = false;
  return 0;
}

static SweepArgs sweep_args(mpsfm_ba_handle* h, double radius, const LmCtl* ctl = nullptr) {
  SweepArgs a{};
  a.ctl = ctl;
  a.chunks = h->d_chunks; a.chunk_cams = h->d_chunk_cams; a.rec_cam = h->rt.rec_cam; a.rec_meta = h->rt.rec_meta;
  a.rec_xy = h->rt.rec_xy; a.rec_d = h->rt.rec_d; a.rec_m = h->rt.rec_m; a.rec_a = h->rt.rec_a;
  a.pt_rec_start = h->rt.pt_rec_start; a.pt_kv = h->rt.pt_kv; a.blk_desc = h->d_blk_desc; a.blk_ent_start = h->d_blk_ent_start; a.ents = h->d_ents;
  a.camtab = h->d_camtab; a.pts = h->d_pts; a.ps = h->d_ps; a.loss = h->loss;
  a.radius = radius; a.min_diag = h->opt.min_lm_diagonal; a.max_diag = h->opt.max_lm_diagonal; a.ncv = h->ncv; a.dbg = (g_dbg_flags >> 8) & 0xff;
  a.lhdr = h->d_lhdr; a.nlong = h->nlong; a.nchunks = h->nchunks; a.cam_slot = h->d_cam_slot; a.wl = h->d_wl;
  a.sky = BlockSky{h->d_sky_first, h->d_sky_start, h->d_sky_index, h->ncv};
  a.Sblk = h->d_Sblk; a.gc = h->d_gc; a.wv = h->d_wv; a.diagU = h->d_diagU; a.part = h->d_part; a.diagV = h->d_diagV;
  a.yc = h->d_yc; a.camtab2 = h->d_camtab2; a.pts2 = h->d_pts2; a.part2 = h->d_part2;
  a.slab = h->d_slab; a.chunk0 = 0;
  return a;
}

// cost of a record list; out[0] reprojection, out[1] depth, out[2] bad count (host values)
static int cost_of_records(mpsfm_ba_handle* h, int64_t nrec, const int32_t* cam, const int32_t* pt, const uint32_t* meta,
                           const double* xy, const double* d, const double* m, const double* a, double* out3) {
  out3[0] = out3[1] = out3[2] = 0.0;
  if (nrec <= 0) return 0;
  const int nb = (int)std::min<int64_t>(1024, (nrec + kThreads - 1) / kThreads);
  CostArgs c{nrec, cam, pt, meta, xy, d, m, a, h->d_camtab, h->d_pts, h->loss, h->d_costpart};
  launch_cost_records(c, nb, h->stream);
  launch_reduce_cols(h->d_costpart, nb, 4, 3, 0u, h->d_scal, h->stream);
  HIP_TRY(hipMemcpyAsync(h->h_scal, h->d_scal, sizeof(double) * 3, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  out3[0] = h->h_scal[0]; out3[1] = h->h_scal[1]; out3[2] = h->h_scal[2];
  return 0;
}

// Jacobi column scales from the Jacobian at the current state (Ceres: iteration 0 only)
static int prepare_scales(mpsfm_ba_handle* h) {
  hipStream_t s = h->stream;
  launch_cam_scales(h->nc, h->d_cam_slot, h->d_cmask, h->d_diagU, 0, h->d_cs, s);
  launch_pt_scales(h->np, h->rt.pt_kv, h->d_diagV, 0, h->d_ps, s);
  launch_build_camtab(h->nc, h->d_q, h->d_t, h->d_intr, h->d_intr_idx, h->d_cs, h->d_camtab, s);
  if (h->opt.jacobi_scaling) {
    HIP_TRY(hipMemsetAsync(h->d_diagU, 0, sizeof(double) * (size_t)std::max(h->n_user, 1), s));
    HIP_TRY(hipMemsetAsync(h->d_diagV, 0, sizeof(double) * 3 * (size_t)std::max<int64_t>(h->np, 1), s));
    SweepArgs a = sweep_args(h, 1.0);
    launch_track_sweep(a, h->nchunks, true, s);
    if (int rc = allreduce_dev(h, h->d_diagU, h->n_user)) return rc;
    launch_cam_scales(h->nc, h->d_cam_slot, h->d_cmask, h->d_diagU, 1, h->d_cs, s);
    launch_pt_scales(h->np, h->rt.pt_kv, h->d_diagV, 1, h->d_ps, s);
    launch_build_camtab(h->nc, h->d_q, h->d_t, h->d_intr, h->d_intr_idx, h->d_cs, h->d_camtab, s);
  }
  HIP_TRY(hipGetLastError());
  h->scales_ready = true;
  return 0;
}

// the full track sweep: dense chunks through their slabs (k_track_sweep_dense + k_reduce_slabs), the others and the long
// tracks through the general kernels (global atomics); all of them add into the zeroed reduced buffer
static void launch_sweeps(mpsfm_ba_handle* h, SweepArgs a, hipStream_t s) {
  launch_track_sweep_dense(a, h->n_dense, s);
  launch_reduce_slabs(h->d_red_dests, h->n_red_dests, h->d_red_srcs, h->d_slab, h->d_Sblk, h->d_gc, h->d_wv, h->d_diagU, a.ctl, s);
  a.chunk0 = h->n_dense;
  launch_track_sweep(a, h->nchunks - h->n_dense, false, s);
}

// one track sweep at the current state: fills the reduced buffer and its scalar tail
// (inside the solve loop the prologue kernel has zeroed the buffer; single-rank runs reduce the partials with the decision)
static int run_track_sweep(mpsfm_ba_handle* h, double radius, const LmCtl* ctl = nullptr, bool in_loop = false, bool adopt = false) {
  hipStream_t s = h->stream;
  if (!in_loop) launch_zero(h->d_red, h->red_count, ctl, s);
  SweepArgs a = sweep_args(h, radius, ctl);
  if (adopt) {
    a.adopt_on = 1; a.adopt_nc = h->nc;
    a.pts_rw = h->d_pts; a.q_rw = h->d_q; a.t_rw = h->d_t; a.camtab_rw = h->d_camtab; a.q2 = h->d_q2; a.t2 = h->d_t2;
    a.red = h->d_red; a.nred = h->red_count;
  }
  launch_sweeps(h, a, s);
  if (h->nchunks + h->nlong > 0 && !(in_loop && !sharded(h)))
    launch_reduce_cols(h->d_part, h->nchunks + h->nlong, 4, 3, 1u << 2, h->d_redsc, s, sharded(h) ? nullptr : h->d_scal + U_X_COST,
                       sharded(h) ? (h->opt.rank > 0 ? h->opt.rank : 0) % kMaxRankSlots : -1);
  else if (sharded(h)) launch_gmax_to_slot(h->d_redsc, h->opt.rank > 0 ? h->opt.rank : 0, s);  // (a rank without chunks: its slot from the zeroed buffer)
  h->last_radius = radius;
  return 0;
}

static int run_dense(mpsfm_ba_handle* h, double radius, const LmCtl* ctl = nullptr) {
  hipStream_t s = h->stream;
  // d_fail is zero here: cleared at creation and re-armed by k_cam_update after every read
  if (h->n > 0) {
    // the level-scheduled factorisation without inverse accumulators only touches the tiles of its plan
    const bool level = dense_level(&h->ov, &h->lp);
    double* pinv = dense_pinv(h->d_dwork, h->nt, &h->ov, &h->lp);
    const bool listed = level && !pinv;
    AssembleArgs as{BlockSky{h->d_sky_first, h->d_sky_start, h->d_sky_index, h->ncv}, h->d_Sblk, h->d_gc, h->d_wv, h->d_diagU, h->ncv, h->n, h->nt, radius,
                    h->opt.min_lm_diagonal, h->opt.max_lm_diagonal, h->d_A, pinv, listed ? h->lp.d_asm_tiles : nullptr, listed ? h->lp.n_asm : 0,
                    h->lp.d_col_slot, h->n_user, (level && pinv) ? h->d_yc : nullptr, (level && pinv) ? h->lp.d_tile_live : nullptr, ctl};
    launch_assemble(as, s);
    launch_dense_solve(h->d_A, h->d_dwork, h->nt, h->n, h->d_yc, h->d_fail, s, &h->ov, &h->lp, ctl);
  }
  return 0;
}

// Small problems (local bundle adjustment): fixed cost, column scales, the trust-region loop and the state norm without a single
// host synchronisation before the end — the loop is ONE cooperative launch (local_lm.hip).  Returns kLocalRefused when the launch
// is not accepted (nothing has changed the state then: the launch chain takes over).
constexpr int kLocalRefused = 1;
static int solve_local(mpsfm_ba_handle* h, mpsfm_ba_summary* sum) {
  hipStream_t s = h->stream;
  const mpsfm_ba_options& o = h->opt;
  launch_cam_scales(h->nc, h->d_cam_slot, h->d_cmask, h->d_diagU, 0, h->d_cs, s);
  launch_build_camtab(h->nc, h->d_q, h->d_t, h->d_intr, h->d_intr_idx, h->d_cs, h->d_camtab, s);
  double* fixed_parts = h->d_scal + 12;  // three free slots of the scalar block
  HIP_TRY(hipMemsetAsync(h->d_scal, 0, sizeof(double) * U_COUNT, s));
  if (h->nfixed > 0) {
    const int nb = (int)std::min<int64_t>(1024, (h->nfixed + kThreads - 1) / kThreads);
    CostArgs c{h->nfixed, h->rt.fx_cam, h->rt.fx_pt, h->rt.fx_meta, h->rt.fx_xy, h->rt.fx_d, h->rt.fx_m, h->rt.fx_a, h->d_camtab, h->d_pts, h->loss, h->d_costpart};
    launch_cost_records(c, nb, s);
    launch_reduce_cols(h->d_costpart, nb, 4, 3, 0u, fixed_parts, s);
  }
  if (int rc = prepare_scales(h)) return rc;
  LmCtl c0;
  std::memset(&c0, 0, sizeof(c0));
  c0.radius = o.initial_trust_region_radius; c0.decrease_factor = 2.0;
  c0.term = kLmRunning; c0.check_gradient = 1;  // x_norm and fixed_cost: filled in by the launch
  h->h_ctl[0] = c0;
  HIP_TRY(hipMemcpyAsync(h->d_ctl, &h->h_ctl[0], sizeof(LmCtl), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(h->d_local_acc, 0, sizeof(double) * 2 * kLocalAccDoubles, s));
  HIP_TRY(hipMemsetAsync(h->d_local_sync, 0, sizeof(int64_t) * 16, s));
  LocalArgs la{};
  la.A = sweep_args(h, 0.0, nullptr);
  la.ctl = h->d_ctl;
  la.o = LmOpts{o.function_tolerance, o.gradient_tolerance, o.parameter_tolerance, o.min_relative_decrease, o.max_trust_region_radius,
                o.min_trust_region_radius, o.max_num_iterations, o.max_num_consecutive_invalid_steps};
  la.log = o.verbose > 0 ? h->d_local_log : nullptr;
  la.acc[0] = h->d_local_acc; la.acc[1] = h->d_local_acc + kLocalAccDoubles;
  la.part[0] = h->d_part; la.part[1] = h->d_part + (size_t)h->nchunks * 4;  // (nlong == 0 here; the chain only ever uses the first half)
  la.bar = reinterpret_cast<int32_t*>(h->d_local_sync); la.clk = reinterpret_cast<long long*>(h->d_local_sync + 1);
  la.ncv = h->ncv; la.nc = h->nc; la.nchunks = h->nchunks;
  la.q = h->d_q; la.t = h->d_t; la.camtab = h->d_camtab; la.pts = h->d_pts; la.cs = h->d_cs; la.fixed_parts = fixed_parts;
  la.skew_chunk = g_skew_chunk; la.skew_mask = g_skew_ticks > 0 ? g_skew_mask : 0; la.skew_ticks = g_skew_ticks;
  if (launch_local_lm(la, s) != (int)hipSuccess) {
    (void)hipGetLastError();
    HIP_TRY(hipStreamSynchronize(s));  // the pinned control block is free again
    return kLocalRefused;
  }
  static_assert(sizeof(int64_t) * 8 <= sizeof(double) * U_COUNT * 2, "the pinned scalar block holds the sync words");
  int64_t* hs = reinterpret_cast<int64_t*>(h->h_scal);
  HIP_TRY(hipMemcpyAsync(&h->h_ctl[0], h->d_ctl, sizeof(LmCtl), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(hs, h->d_local_sync, sizeof(int64_t) * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
  if (reinterpret_cast<const int32_t*>(hs)[1] != 0)
    return fail(MPSFM_EHIP, "single-launch solver: a grid barrier did not complete (workgroups not co-resident?); MPSFM_LOCAL_LM=0 selects the launch chain");
  const LmCtl& last = h->h_ctl[0];
  const double fixed = last.fixed_cost;
  sum->fixed_cost = fixed;
  sum->time_linearize_s = 1e-8 * (double)(hs[1] + hs[2]); sum->time_dense_s = 1e-8 * (double)hs[3]; sum->time_update_s = 1e-8 * (double)(hs[4] + hs[5] + hs[6]);
  if (o.verbose > 0) {
    const int nlog = std::min(last.iter + 1, h->local_log_cap);
    std::vector<LmHead> log((size_t)std::max(nlog, 0));
    if (nlog > 0) HIP_TRY(hipMemcpy(log.data(), h->d_local_log, sizeof(LmHead) * (size_t)nlog, hipMemcpyDeviceToHost));
    for (int i = 0; i < nlog; ++i) {
      const LmHead& l = log[(size_t)i];
      if (l.iter != i + 1 && i != nlog - 1) continue;
      if (l.last_mcc > 0.0 && l.last_cand != DBL_MAX)
        std::fprintf(stderr, "[mpsfm_ba] it %3d cost %.9e cand %.9e rel %.3e radius %.3e |step| %.3e\n", i + 1, l.last_x_cost + fixed, l.last_cand + fixed,
                     l.last_rel, l.radius, l.last_step_norm);
      else
        std::fprintf(stderr, "[mpsfm_ba] it %3d invalid step (chol_fail=%d mcc=%.3e) radius %.3e\n", i + 1, l.last_chol_fail, l.last_mcc, l.radius);
    }
  }
  h->last_radius = last.radius;
  sum->num_jacobian_evals = last.n_jac_evals;
  sum->num_residual_evals = (int64_t)h->nblocks_reduced_global * ((int64_t)last.n_cost_evals + last.n_jac_evals);
  if (last.term == kLmNumericError)
    return fail(MPSFM_ENUMERIC, "the initial point cannot be evaluated (non-finite residual or depth <= 0 in a log-depth block)");
  sum->initial_cost = last.initial_cost;
  sum->fixed_cost = last.fixed_cost;  // (one rank: formed on the device)
  sum->final_cost = last.cur_cost + last.fixed_cost;
  sum->num_iterations = last.iter;
  sum->num_successful_steps = last.n_success;
  sum->num_unsuccessful_steps = last.n_unsuccess;
  sum->termination = last.term;
  sum->final_radius = last.radius;
  sum->trace_len = last.trace_len;
  for (int i = 0; i < last.trace_len; ++i) { sum->trace_cost[i] = last.trace_cost[i]; sum->trace_radius[i] = last.trace_radius[i]; sum->trace_accepted[i] = last.trace_accepted[i]; }
  return 0;
}

static int solve_impl(mpsfm_ba_handle* h, mpsfm_ba_summary* sum) {
  using clk = std::chrono::steady_clock;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const mpsfm_ba_options& o = h->opt;
  std::memset(sum, 0, sizeof(*sum));
  HIP_TRY(hipStreamSynchronize(s));
  const auto t_begin = clk::now();
  sum->num_residual_blocks = (int64_t)h->nblocks_global;
  sum->reduced_dim = h->n_user;
  int64_t n_cost_evals = 0, n_jac_evals = 0;
  if (h->local_ok) {
    const int rc = solve_local(h, sum);
    if (rc != kLocalRefused) {
      sum->time_total_s = std::chrono::duration<double>(clk::now() - t_begin).count();
      return rc;
    }
  }

  auto finish = [&](int rc) {
    sum->num_jacobian_evals = n_jac_evals;
    sum->num_residual_evals = (int64_t)h->nblocks_reduced_global * (n_cost_evals + n_jac_evals);
    sum->time_total_s = std::chrono::duration<double>(clk::now() - t_begin).count();
    return rc;
  };
  // Nothing in front of the loop needs the host — the cost of the fixed blocks and the state norm stay on the device and enter
  // the control block there (k_lm_init); three stream synchronisations less per solve.  Sharded runs sum them over the ranks
  // in one small exchange on the device.
  const bool nothing_to_solve = h->n == 0 && h->nvarpts_global == 0.0;
  const bool async_pre = !nothing_to_solve;
  double fixed = 0.0, x_norm = 0.0;
  // camera table at the initial point (unit scales) for the fixed cost
  launch_cam_scales(h->nc, h->d_cam_slot, h->d_cmask, h->d_diagU, 0, h->d_cs, s);
  launch_build_camtab(h->nc, h->d_q, h->d_t, h->d_intr, h->d_intr_idx, h->d_cs, h->d_camtab, s);
  if (async_pre) {
    HIP_TRY(hipMemsetAsync(h->d_scal, 0, sizeof(double) * U_COUNT, s));
    if (h->nfixed > 0) {
      const int nb = (int)std::min<int64_t>(1024, (h->nfixed + kThreads - 1) / kThreads);
      CostArgs c{h->nfixed, h->rt.fx_cam, h->rt.fx_pt, h->rt.fx_meta, h->rt.fx_xy, h->rt.fx_d, h->rt.fx_m, h->rt.fx_a, h->d_camtab, h->d_pts, h->loss, h->d_costpart};
      launch_cost_records(c, nb, s);
      launch_reduce_cols(h->d_costpart, nb, 4, 3, 0u, h->d_scal + 12, s);
    }
  } else {
    double fx[3];
    if (int rc = cost_of_records(h, h->nfixed, h->rt.fx_cam, h->rt.fx_pt, h->rt.fx_meta, h->rt.fx_xy, h->rt.fx_d, h->rt.fx_m, h->rt.fx_a, fx)) return rc;
    fixed = fx[0] + fx[1];
    if (int rc = allreduce_host(h, &fixed, 1)) return rc;
    sum->fixed_cost = fixed;
  }

  if (nothing_to_solve) {
    double c3[3];
    if (int rc = cost_of_records(h, h->nrec, h->rt.rec_cam, h->rt.rec_pt, h->rt.rec_meta, h->rt.rec_xy, h->rt.rec_d, h->rt.rec_m, h->rt.rec_a, c3)) return rc;
    double c = c3[0] + c3[1];
    if (int rc = allreduce_host(h, &c, 1)) return rc;
    sum->initial_cost = sum->final_cost = c + fixed;
    sum->termination = MPSFM_TERM_NO_VARIABLES;
    return finish(0);
  }

  if (int rc = prepare_scales(h)) return rc;
  if (h->np > 0) HIP_TRY(hipMemcpyAsync(h->d_pts2, h->d_pts, sizeof(double) * 3 * h->np, hipMemcpyDeviceToDevice, s));
  // initial x norm: cameras through a zero-step camera update, landmarks by a reduction
  HIP_TRY(hipMemsetAsync(h->d_yc, 0, sizeof(double) * (size_t)std::max(h->n_user, 1), s));
  if (!async_pre) HIP_TRY(hipMemsetAsync(h->d_scal, 0, sizeof(double) * U_COUNT, s));
  {
    HIP_TRY(hipMemsetAsync(h->d_gc, 0, sizeof(double) * (size_t)std::max(h->n_user, 1), s));
    launch_cam_update(h->nc, h->d_cam_slot, h->d_q, h->d_t, h->d_cs, h->d_yc, h->d_gc, h->d_q2, h->d_t2, h->d_scal, s);
    const int nb = (int)std::min<int64_t>(1024, std::max<int64_t>(1, (h->np + kThreads - 1) / kThreads));
    launch_pts_sqnorm(h->np, h->rt.pt_kv, h->d_pts, h->d_costpart, nb, s);
    launch_reduce_cols(h->d_costpart, nb, 1, 1, 0u, h->d_scal + U_XN_SQ_PTS, s);
    if (!async_pre) {
      HIP_TRY(hipMemcpyAsync(h->h_scal, h->d_scal, sizeof(double) * U_COUNT, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      double v = h->h_scal[U_XN_SQ_PTS];
      if (int rc = allreduce_host(h, &v, 1)) return rc;
      x_norm = std::sqrt(v + h->h_scal[U_XN_SQ_CAMS]);
    }
  }

  // ---- Levenberg-Marquardt loop.  The decisions are taken on the device (k_lm_decide, LmCtl in common.h): the host
  // enqueues iteration i+1 BEFORE it looks at the outcome of iteration i, so the stream never runs dry, and only reads a
  // pinned copy of the control block one iteration late.  When that copy says the solve is over, the one iteration queued
  // ahead returns at once in every kernel.  Every rank of a sharded run sees the same decisions at the same iteration, so
  // all of them enqueue the same sequence of collectives.
  {
    LmCtl c0;
    std::memset(&c0, 0, sizeof(c0));
    c0.radius = o.initial_trust_region_radius; c0.decrease_factor = 2.0; c0.x_norm = x_norm; c0.fixed_cost = fixed;
    c0.term = kLmRunning; c0.check_gradient = 1;
    h->h_ctl[0] = c0;
    HIP_TRY(hipMemcpyAsync(h->d_ctl, &h->h_ctl[0], sizeof(LmCtl), hipMemcpyHostToDevice, s));
    if (async_pre) {  // x_norm and fixed_cost from the device scalars
      double* sums = nullptr;
      if (sharded(h)) {
        sums = h->d_costpart;  // (free again: its reductions are queued in front)
        launch_lm_pack(h->d_scal, sums, s);
        if (int rc = allreduce_dev(h, sums, 3)) return rc;
      }
      launch_lm_init(h->d_ctl, h->d_scal, sums, s);
    }
    else HIP_TRY(hipStreamSynchronize(s));  // the pinned slot is reused below
  }
  const LmOpts lo{o.function_tolerance, o.gradient_tolerance, o.parameter_tolerance, o.min_relative_decrease, o.max_trust_region_radius,
                  o.min_trust_region_radius, o.max_num_iterations, o.max_num_consecutive_invalid_steps};
  const LmCtl* ctl = h->d_ctl;
  const double host_radius = 0.0;  // unused: the kernels read the radius from the control block
  const bool fuse_prologue = [] { const char* e = std::getenv("MPSFM_FUSE_PROLOGUE"); return !(e && std::atoi(e) == 0); }();
  const bool fuse_cam = [] { const char* e = std::getenv("MPSFM_FUSE_CAM"); return !(e && std::atoi(e) == 0); }();
  auto enqueue_iteration = [&](int it) -> int {
    hipEvent_t* ev = (it & 1) ? h->ev2 : h->ev;
    HIP_TRY(hipEventRecord(ev[0], s));
    // all chunks dense: the dense sweep adopts an accepted candidate and zeroes the reduced buffer itself (sharded runs too: the
    // exchange of the reduced buffer comes behind the slab reduction, the camera scalars are the same on every rank)
    const bool fused_prologue = fuse_prologue && h->nlong == 0 && h->n_dense > 0 && h->n_dense == h->nchunks;
    if (!fused_prologue)
      launch_lm_prologue(h->d_ctl, h->d_red, h->red_count, h->nc, h->np, h->d_q, h->d_t, h->d_camtab, h->d_pts, h->d_q2, h->d_t2, h->d_camtab2, h->d_pts2, s);
    if (int rc = run_track_sweep(h, host_radius, ctl, true, fused_prologue)) return rc;
    if (int rc = allreduce_dev(h, h->d_red, h->red_count)) return rc;
    HIP_TRY(hipEventRecord(ev[1], s));
    if (int rc = run_dense(h, host_radius, ctl)) return rc;
    HIP_TRY(hipEventRecord(ev[2], s));
    // all chunks dense and one rank: the update sweep forms the candidate cameras itself (CamUpdArgs)
    const bool fused_cam = fuse_cam && fused_prologue;
    CamUpdArgs cu{1, h->nc, h->d_cam_slot, h->d_cam_of_slot, h->d_q, h->d_t, h->d_cs, h->d_gc, h->d_intr, h->d_intr_idx,
                  h->d_q2, h->d_t2, h->d_camtab2, h->d_scal, h->d_fail};
    if (!fused_cam)
      launch_cam_update(h->nc, h->d_cam_slot, h->d_q, h->d_t, h->d_cs, h->d_yc, h->d_gc, h->d_q2, h->d_t2, h->d_scal, s,
                        h->d_intr, h->d_intr_idx, h->d_camtab2, h->d_fail, ctl);
    {
      SweepArgs a = sweep_args(h, host_radius, ctl);
      launch_update_sweep(a, h->nchunks, s, fused_cam ? &cu : nullptr);
    }
    if (!sharded(h)) {
      launch_lm_reduce_decide(h->d_part, h->d_part2, h->nchunks + h->nlong, h->d_ctl, h->d_scal, lo, &h->h_ctl[it & 1], s);
    } else {
      if (h->nchunks + h->nlong > 0) launch_reduce_cols(h->d_part2, h->nchunks + h->nlong, 8, 5, 0u, h->d_scal, s);
      if (int rc = allreduce_dev(h, h->d_scal, 5)) return rc;
      // the all-reduced scalars of the track sweep: cost and bad count summed, landmark-gradient maximum over the rank slots
      launch_lm_decide(h->d_ctl, h->d_scal, lo, &h->h_ctl[it & 1], s, h->d_redsc);
    }
    HIP_TRY(hipEventRecord(ev[3], s));
    return 0;
  };
  LmCtl last = h->h_ctl[0];
  if (last.term == kLmRunning) {
    if (int rc = enqueue_iteration(1)) return rc;
    const bool speculate = [] { const char* e = std::getenv("MPSFM_LM_SPECULATE"); return !(e && std::atoi(e) == 0); }();  // per solve: tests switch it
    for (int it = 1;; ++it) {
      if (speculate) { if (int rc = enqueue_iteration(it + 1)) return rc; }  // ahead of the news about iteration `it`
      hipEvent_t* ev = (it & 1) ? h->ev2 : h->ev;
      HIP_TRY(hipEventSynchronize(ev[3]));
      HIP_TRY(hipGetLastError());
      float ms;
      HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1])); sum->time_linearize_s += 1e-3 * ms;
      HIP_TRY(hipEventElapsedTime(&ms, ev[1], ev[2])); sum->time_dense_s += 1e-3 * ms;
      HIP_TRY(hipEventElapsedTime(&ms, ev[2], ev[3])); sum->time_update_s += 1e-3 * ms;
      const LmCtl prev = last;
      last = h->h_ctl[it & 1];
      if (o.verbose > 0) {
        if (last.last_mcc > 0.0 && last.last_cand != DBL_MAX)
          std::fprintf(stderr, "[mpsfm_ba] it %3d cost %.9e cand %.9e rel %.3e radius %.3e |step| %.3e\n", it, last.last_x_cost + last.fixed_cost,
                       last.last_cand + last.fixed_cost, last.last_rel, last.radius, last.last_step_norm);
        else
          std::fprintf(stderr, "[mpsfm_ba] it %3d invalid step (chol_fail=%d mcc=%.3e) radius %.3e\n", it, last.last_chol_fail, last.last_mcc, last.radius);
      }
      (void)prev;
      if (last.term != kLmRunning) break;
      if (!speculate) { if (int rc = enqueue_iteration(it + 1)) return rc; }
    }
    // the iteration that ended the solve may have been accepted (iteration or radius limit); the copy is idempotent
    launch_lm_accept(h->d_ctl, h->nc, h->np, h->d_q, h->d_t, h->d_camtab, h->d_pts, h->d_q2, h->d_t2, h->d_camtab2, h->d_pts2, s);
    HIP_TRY(hipStreamSynchronize(s));  // the iteration queued ahead has drained (every kernel of it returned at once)
  }
  h->last_radius = last.radius;
  n_cost_evals = last.n_cost_evals; n_jac_evals = last.n_jac_evals;
  if (last.term == kLmNumericError)
    return finish(fail(MPSFM_ENUMERIC, "the initial point cannot be evaluated (non-finite residual or depth <= 0 in a log-depth block)"));
  sum->initial_cost = last.initial_cost;
  sum->fixed_cost = last.fixed_cost;  // (one rank: formed on the device)
  sum->final_cost = last.cur_cost + last.fixed_cost;
  sum->num_iterations = last.iter;
  sum->num_successful_steps = last.n_success;
  sum->num_unsuccessful_steps = last.n_unsuccess;
  sum->termination = last.term;
  sum->final_radius = last.radius;
  sum->trace_len = last.trace_len;
  for (int i = 0; i < last.trace_len; ++i) { sum->trace_cost[i] = last.trace_cost[i]; sum->trace_radius[i] = last.trace_radius[i]; sum->trace_accepted[i] = last.trace_accepted[i]; }
  return finish(0);
}

static thread_local int g_cu_count = 256;
static int create_impl(const mpsfm_ba_problem* P, const mpsfm_ba_state* st, const mpsfm_ba_options* o, mpsfm_ba_handle** out) {
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
    static std::vector<int> cus;
    std::lock_guard<std::mutex> lk(mu);
    if ((int)arch.size() < ndev) { arch.resize((size_t)ndev); cus.resize((size_t)ndev, 256); }
    if (arch[(size_t)o->device].empty()) {
      hipDeviceProp_t prop;
      HIP_TRY(hipGetDeviceProperties(&prop, o->device));
      arch[(size_t)o->device] = prop.gcnArchName;
      cus[(size_t)o->device] = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    g_cu_count = cus[(size_t)o->device];
    if (std::strncmp(arch[(size_t)o->device].c_str(), "gfx950", 6) != 0)
      return fail(MPSFM_ENODEVICE, std::string("device is ") + arch[(size_t)o->device] + ", this library is built for gfx950 only");
  }
  since("device check");
  HIP_TRY(hipSetDevice(o->device));
  mpsfm_ba_handle* h = new mpsfm_ba_handle();
  h->device = o->device; h->opt = *o;
  if (o->stream) { h->stream = (hipStream_t)o->stream; h->own_stream = false; }
  else {
    if (pooled_stream(&h->stream) != hipSuccess) { delete h; return fail(MPSFM_EHIP, "hipStreamCreate failed"); }
    h->own_stream = true;
  }
  if (o->use_rccl && o->world_size >= 1) {
    Rccl& R = rccl();
    if (!R.ok) { free_handle(h); return fail(MPSFM_ECOMM, "use_rccl: " + R.why); }
    if (o->rank < 0 || o->rank >= o->world_size) { free_handle(h); return fail(MPSFM_EINVAL, "rank out of range"); }
    Rccl::UniqueId id;
    std::memcpy(id.internal, o->comm_id, sizeof(id.internal));
    const int nrc = R.CommInitRank(&h->comm, o->world_size, id, o->rank);
    if (nrc != 0) { h->comm = nullptr; free_handle(h); return fail(MPSFM_ECOMM, std::string("ncclCommInitRank: ") + (R.GetErrorString ? R.GetErrorString(nrc) : "failed")); }
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

// ---- C ABI ---------------------------------------------------------------------------------------
// Test hook (tests/test_host_cpu.py; no device involved): takes and gives back `count` host blocks of `bytes` each through
// the block cache twice; returns how many blocks of the second round were recycled ones of the first (by address).
extern "C" int64_t mpsfm_debug_host_cache(int64_t bytes, int32_t count) {
  std::vector<mpsfm::HostBuf<uint8_t>> first((size_t)count), second((size_t)count);
  std::vector<const void*> seen;
  for (auto& b : first) { b.alloc((size_t)bytes); b[0] = 1; b[(size_t)bytes - 1] = 2; seen.push_back(b.data()); }
  first.clear();
  int64_t reused = 0;
  for (auto& b : second) {
    b.alloc((size_t)bytes);
    b[0] = 3;
    reused += std::find(seen.begin(), seen.end(), (const void*)b.data()) != seen.end() ? 1 : 0;
  }
  return reused;
}

// Test hook (tests/test_host_cpu.py; no device involved): `reps` rounds of an `nparts`-part job through the table build's
// worker pool; returns the number of parts that did not run exactly once.
extern "C" int64_t mpsfm_debug_run_parts(int32_t nparts, int32_t reps) {
  int64_t bad = 0;
  for (int r = 0; r < reps; ++r) {
    std::vector<std::atomic<int>> hits((size_t)std::max(nparts, 1));
    for (auto& x : hits) x.store(0);
    mpsfm::run_parts(nparts, [&](int t, int np) {
      if (np != std::max(nparts, 1) || t < 0 || t >= np) return;
      volatile double acc = 0.0;
      for (int k = 0; k < 2000; ++k) acc = acc + (double)k * 1e-9;  // a little work, so that parts overlap
      hits[(size_t)t].fetch_add(1);
    });
    for (auto& x : hits) bad += x.load() == 1 ? 0 : 1;
  }
  return bad;
}

// Test hook (tests/test_dist_cpu.py; no device involved): the camera-graph union of a landmark-sharded run as the ranks
// compute it — `world` adjacency matrices (n x n bytes each) packed per rank, summed like the all-reduce does, unpacked
// into `out` (n x n bytes).  Returns the digits per double used.
extern "C" int mpsfm_debug_graph_union(const uint8_t* adj, int32_t world, int32_t n, uint8_t* out) {
  std::vector<double> sum;
  for (int r = 0; r < world; ++r) {
    mpsfm::CamGraph g;
    g.init(n);
    for (int a = 0; a < n; ++a)
      for (int b = 0; b < n; ++b)
        if (adj[((size_t)r * n + a) * n + b]) g.set(a, b);
    std::vector<double> packed;
    mpsfm::pack_graph(g, world, packed);
    if (sum.empty()) sum.assign(packed.size(), 0.0);
    for (size_t i = 0; i < packed.size(); ++i) sum[i] += packed[i];
  }
  mpsfm::CamGraph u;
  u.init(n);
  mpsfm::unpack_graph(sum, world, u);
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b) out[(size_t)a * n + b] = u.get(a, b) ? 1 : 0;
  return mpsfm::graph_digits(world);
}

extern "C" {

int mpsfm_abi_version(void) { return MPSFM_ABI_VERSION; }
const char* mpsfm_last_error(void) { return g_err.c_str(); }

int mpsfm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  int good = 0;
  for (int i = 0; i < n; ++i) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, i) == hipSuccess && std::strncmp(p.gcnArchName, "gfx950", 6) == 0) ++good;
  }
  return good;
}

int mpsfm_comm_unique_id(uint8_t id[128]) {
  if (!id) return fail(MPSFM_EINVAL, "id is NULL");
  Rccl& R = rccl();
  if (!R.ok) return fail(MPSFM_ECOMM, R.why);
  Rccl::UniqueId u;
  const int rc = R.GetUniqueId(&u);
  if (rc != 0) return fail(MPSFM_ECOMM, std::string("ncclGetUniqueId: ") + (R.GetErrorString ? R.GetErrorString(rc) : "failed"));
  std::memcpy(id, u.internal, 128);
  return 0;
}

void mpsfm_ba_default_options(mpsfm_ba_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->max_num_iterations = 50;
  o->function_tolerance = 1e-6;
  o->gradient_tolerance = 1e-10;
  o->parameter_tolerance = 1e-8;
  o->initial_trust_region_radius = 1e4;
  o->max_trust_region_radius = 1e16;
  o->min_trust_region_radius = 1e-32;
  o->min_relative_decrease = 1e-3;
  o->min_lm_diagonal = 1e-6;
  o->max_lm_diagonal = 1e32;
  o->max_num_consecutive_invalid_steps = 5;
  o->jacobi_scaling = 1;
}

int mpsfm_ba_create(const mpsfm_ba_problem* problem, const mpsfm_ba_state* initial, const mpsfm_ba_options* options,
                    mpsfm_ba_handle** out) {
  return create_impl(problem, initial, options, out);
}

int mpsfm_ba_set_state(mpsfm_ba_handle* h, const mpsfm_ba_state* state) {
  if (!h) return fail(MPSFM_EINVAL, "handle is NULL");
  if (hipSetDevice(h->device) != hipSuccess) return fail(MPSFM_EHIP, "hipSetDevice failed");
  return upload_state(h, state, false);
}

int mpsfm_ba_reset_state(mpsfm_ba_handle* h) {
  if (!h) return fail(MPSFM_EINVAL, "handle is NULL");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemcpyAsync(h->d_q, h->d_q0, sizeof(double) * 4 * h->nc, hipMemcpyDeviceToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(h->d_t, h->d_t0, sizeof(double) * 3 * h->nc, hipMemcpyDeviceToDevice, h->stream));
  if (h->np > 0) HIP_TRY(hipMemcpyAsync(h->d_pts, h->d_pts0, sizeof(double) * 3 * h->np, hipMemcpyDeviceToDevice, h->stream));
  h->scales_ready = false;
  return 0;
}

int mpsfm_ba_solve_resident(mpsfm_ba_handle* h, mpsfm_ba_summary* summary) {
  if (!h || !summary) return fail(MPSFM_EINVAL, "handle or summary is NULL");
  return solve_impl(h, summary);
}

int mpsfm_ba_get_state(mpsfm_ba_handle* h, mpsfm_ba_state* st) {
  if (!h || !st) return fail(MPSFM_EINVAL, "handle or state is NULL");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));  // copies on the handle's own stream, never the legacy null stream (see solve_impl)
  if (h->nc > 0) {
    HIP_TRY(hipMemcpyAsync(st->cam_quat_xyzw, h->d_q, sizeof(double) * 4 * h->nc, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(st->cam_t, h->d_t, sizeof(double) * 3 * h->nc, hipMemcpyDeviceToHost, h->stream));
  }
  if (h->d_perm) {  // back into the caller's order on the device, one copy straight into the caller's array
    launch_permute_pts(h->np, h->d_perm, h->d_pts, h->d_user_pts, true, h->stream);
    HIP_TRY(hipMemcpyAsync(st->pts, h->d_user_pts, sizeof(double) * 3 * h->np, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
  }
  std::vector<double> sorted((size_t)h->np * 3);
  if (h->np > 0) HIP_TRY(hipMemcpyAsync(sorted.data(), h->d_pts, sizeof(double) * 3 * h->np, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  parallel_ranges(h->np, 16384, [&](int64_t k0, int64_t k1) {
    for (int64_t k = k0; k < k1; ++k) {
      double* d = st->pts + 3 * (size_t)h->perm[(size_t)k];
      d[0] = sorted[3 * (size_t)k]; d[1] = sorted[3 * (size_t)k + 1]; d[2] = sorted[3 * (size_t)k + 2];
    }
  });
  return 0;
}

void mpsfm_ba_destroy(mpsfm_ba_handle* h) { free_handle(h); }

int mpsfm_ba_solve(const mpsfm_ba_problem* problem, mpsfm_ba_state* state, const mpsfm_ba_options* options,
                   mpsfm_ba_summary* summary) {
  if (!state || !summary) return fail(MPSFM_EINVAL, "state or summary is NULL");
  mpsfm_ba_handle* h = nullptr;
  auto t_prev = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (!options || options->verbose < 2) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[mpsfm_ba] one-shot: %-25s %8.2f ms\n", what, 1e3 * std::chrono::duration<double>(now - t_prev).count());
    t_prev = now;
  };
  int rc = create_impl(problem, state, options, &h);
  if (rc) return rc;
  lap("create");
  rc = solve_impl(h, summary);
  lap("solve");
  if (rc == 0) rc = mpsfm_ba_get_state(h, state);
  lap("get_state");
  free_handle(h);
  lap("destroy");
  return rc;
}

int mpsfm_ba_eval_cost(mpsfm_ba_handle* h, double* cost_reproj, double* cost_depth) {
  if (!h) return fail(MPSFM_EINVAL, "handle is NULL");
  HIP_TRY(hipSetDevice(h->device));
  launch_cam_scales(h->nc, h->d_cam_slot, h->d_cmask, h->d_diagU, 0, h->d_cs, h->stream);
  launch_build_camtab(h->nc, h->d_q, h->d_t, h->d_intr, h->d_intr_idx, h->d_cs, h->d_camtab, h->stream);
  h->scales_ready = false;
  double a[3], b[3];
  if (int rc = cost_of_records(h, h->nrec, h->rt.rec_cam, h->rt.rec_pt, h->rt.rec_meta, h->rt.rec_xy, h->rt.rec_d, h->rt.rec_m, h->rt.rec_a, a)) return rc;
  if (int rc = cost_of_records(h, h->nfixed, h->rt.fx_cam, h->rt.fx_pt, h->rt.fx_meta, h->rt.fx_xy, h->rt.fx_d, h->rt.fx_m, h->rt.fx_a, b)) return rc;
  if (cost_reproj) *cost_reproj = a[0] + b[0];
  if (cost_depth) *cost_depth = a[1] + b[1];
  return 0;
}

int mpsfm_ba_dense_plan(mpsfm_ba_handle* h, int64_t info[10]) {
  if (!h || !info) return fail(MPSFM_EINVAL, "handle or info is NULL");
  dense_plan_numbers(h->ncv, h->nt, h->plan, h->ov, h->lp, h->d_dwork, h->spat.nblk, info);
  return 0;
}
int mpsfm_ba_reduced_dim(mpsfm_ba_handle* h) { return h ? h->n_user : MPSFM_EINVAL; }

int mpsfm_ba_sweep_once(mpsfm_ba_handle* h, double radius, float* elapsed_ms) {
  if (!h) return fail(MPSFM_EINVAL, "handle is NULL");
  HIP_TRY(hipSetDevice(h->device));
  if (!h->scales_ready) if (int rc = prepare_scales(h)) return rc;
  HIP_TRY(hipMemsetAsync(h->d_red, 0, sizeof(double) * (size_t)h->red_count, h->stream));
  SweepArgs a = sweep_args(h, radius);
  // the three parts of the sweep between events: dense chunks | reduction of their slabs | general chunks and long tracks
  HIP_TRY(hipEventRecord(h->ev[0], h->stream));
  launch_track_sweep_dense(a, h->n_dense, h->stream);
  HIP_TRY(hipEventRecord(h->ev[1], h->stream));
  launch_reduce_slabs(h->d_red_dests, h->n_red_dests, h->d_red_srcs, h->d_slab, h->d_Sblk, h->d_gc, h->d_wv, h->d_diagU, nullptr, h->stream);
  HIP_TRY(hipEventRecord(h->ev[2], h->stream));
  a.chunk0 = h->n_dense;
  launch_track_sweep(a, h->nchunks - h->n_dense, false, h->stream);
  HIP_TRY(hipEventRecord(h->ev[3], h->stream));
  if (h->nchunks + h->nlong > 0) launch_reduce_cols(h->d_part, h->nchunks + h->nlong, 4, 3, 1u << 2, h->d_redsc, h->stream);
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  h->last_radius = radius;
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, h->ev[0], h->ev[3]));
  if (elapsed_ms) *elapsed_ms = ms;
  return 0;
}

// Diagnostics (scripts/dbg_sweep_trace.py): the first `count` 8-byte words of the landmark-diagonal buffer, where the dense sweep leaves
// its phase stamps under debug flag 128.
int mpsfm_debug_read_trace(mpsfm_ba_handle* h, long long* out, int64_t count) {
  if (!h || !out || count < 0 || count > 3 * std::max<int64_t>(h->np, 1)) return fail(MPSFM_EINVAL, "bad trace request");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemcpyAsync(out, h->d_diagV, sizeof(long long) * (size_t)count, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}

// Diagnostics / tests (tests/test_gpu_devbuild.py): table `which` of the handle copied to `out` (at most `cap` bytes); returns the
// table's size in bytes, or a negative error code.  which: 0 chunk headers, 1 chunk cameras, 2 rec_cam, 3 rec_pt, 4 rec_meta, 5 rec_xy,
// 6 rec_d, 7 rec_m, 8 rec_a, 9 pt_rec_start, 10 pt_kv, 11 fx_cam, 12 fx_pt, 13 fx_meta, 14 fx_xy, 15 fx_d, 16 fx_m, 17 fx_a,
// 18 landmark order (host), 19 reduction destinations, 20 reduction sources, 21 camera slots (host), 22: 1 byte, built on the device?,
// 23 blk_desc, 24 blk_ent_start, 25 ents (pair tables of the general chunks), 27 long-track headers, 28 sky_index, 29 sky_first,
// 30 sky_start (host), 31 cmask, 32 cam_of_slot, 33 the ten numbers of mpsfm_ba_dense_plan
int64_t mpsfm_debug_table(mpsfm_ba_handle* h, int32_t which, void* out, int64_t cap) {
  if (!h) return fail(MPSFM_EINVAL, "handle is NULL");
  const void* src = nullptr;
  int64_t bytes = 0;
  bool host = false;
  const int64_t nr = h->nrec, np1 = h->np + 1, nf = h->nfixed;
  switch (which) {
    case 0: src = h->d_chunks; bytes = (int64_t)sizeof(ChunkHdr) * h->nchunks; break;
    case 1: src = h->d_chunk_cams; bytes = 4 * h->n_chunk_cams; break;
    case 2: src = h->rt.rec_cam; bytes = 4 * nr; break;
    case 3: src = h->rt.rec_pt; bytes = 4 * nr; break;
    case 4: src = h->rt.rec_meta; bytes = 4 * nr; break;
    case 5: src = h->rt.rec_xy; bytes = 16 * nr; break;
    case 6: src = h->rt.rec_d; bytes = 8 * nr; break;
    case 7: src = h->rt.rec_m; bytes = 8 * nr; break;
    case 8: src = h->rt.rec_a; bytes = 8 * nr; break;
    case 9: src = h->rt.pt_rec_start; bytes = 4 * np1; break;
    case 10: src = h->rt.pt_kv; bytes = 2 * np1; break;
    case 11: src = h->rt.fx_cam; bytes = 4 * nf; break;
    case 12: src = h->rt.fx_pt; bytes = 4 * nf; break;
    case 13: src = h->rt.fx_meta; bytes = 4 * nf; break;
    case 14: src = h->rt.fx_xy; bytes = 16 * nf; break;
    case 15: src = h->rt.fx_d; bytes = 8 * nf; break;
    case 16: src = h->rt.fx_m; bytes = 8 * nf; break;
    case 17: src = h->rt.fx_a; bytes = 8 * nf; break;
    case 18: src = h->perm.data(); bytes = 4 * (int64_t)h->perm.size(); host = true; break;
    case 19: src = h->d_red_dests; bytes = (int64_t)sizeof(RedDest) * h->n_red_dests; break;
    case 20: src = h->d_red_srcs; bytes = 4 * h->n_red_srcs; break;
    case 21: src = h->cam_slot_h.data(); bytes = 4 * (int64_t)h->cam_slot_h.size(); host = true; break;
    case 23: src = h->d_blk_desc; bytes = 4 * h->n_blk_desc; break;
    case 24: src = h->d_blk_ent_start; bytes = 4 * h->n_blk_ent_start; break;
    case 25: src = h->d_ents; bytes = 4 * h->n_ents; break;
    case 26: src = h->d_part; bytes = 32 * (int64_t)h->nchunks; break;
    case 22: { static uint8_t flag; flag = h->built_on_device ? 1 : 0; src = &flag; bytes = 1; host = true; break; }
    case 27: src = h->d_lhdr; bytes = (int64_t)sizeof(LongHdr) * h->nlong; break;
    case 28: src = h->spat.sky_index.data(); bytes = 4 * (int64_t)h->spat.sky_index.size(); host = true; break;
    case 29: src = h->spat.sky_first.data(); bytes = 4 * (int64_t)h->spat.sky_first.size(); host = true; break;
    case 30: src = h->spat.sky_start.data(); bytes = 8 * (int64_t)h->spat.sky_start.size(); host = true; break;
    case 31: src = h->d_cmask; bytes = 48 * (int64_t)h->nc; break;
    case 32: src = h->d_cam_of_slot; bytes = 4 * (int64_t)std::max(h->ncv, 1); break;
    case 33: { static thread_local int64_t info[10]; if (int rc = mpsfm_ba_dense_plan(h, info)) return rc; src = info; bytes = 80; host = true; break; }
    default: return fail(MPSFM_EINVAL, "unknown table");
  }
  if (!out || cap < bytes) return bytes;
  if (bytes == 0) return 0;
  if (host) { std::memcpy(out, src, (size_t)bytes); return bytes; }
  if (hipSetDevice(h->device) != hipSuccess) return fail(MPSFM_EHIP, "hipSetDevice failed");
  if (hipMemcpyAsync(out, src, (size_t)bytes, hipMemcpyDeviceToHost, h->stream) != hipSuccess) return fail(MPSFM_EHIP, "copy failed");
  if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(MPSFM_EHIP, "sync failed");
  return bytes;
}

// Diagnostics / tests (tests/test_build_tables_cpu.py; no device involved): the host phases of the table build — the functions
// build() calls, for a single rank — run on `P`, then table `which` copied out: numbering, arguments and return value of
// mpsfm_debug_table (26 is a work buffer and does not exist here).  Rebuilds on every call.
int64_t mpsfm_debug_host_build(const mpsfm_ba_problem* P, int32_t which, void* out, int64_t cap) {
  if (int rc = check_problem(P)) return rc;
  BuildOptions opt = BuildOptions::from_environment();
  const Lap lap = [](const char*) {};
  const SumExchange one_rank;
  std::vector<double> cnt((size_t)P->n_cams + 1, 0.0);
  count_camera_blocks(P, cnt);
  CameraLayout cams;
  assign_camera_slots(P, cnt, opt, cams);
  opt.set_chunk_caps(false, cams.ncv, P->n_obs);
  LandmarkGroups groups;
  if (int rc = group_blocks_by_landmark(P, true, groups)) return rc;
  CamGraph graph;
  CholPlan plan;
  if (cams.use_graph) {
    camera_graph_from_groups(P, groups, cams, graph);
    plan_camera_order(graph, opt, plan, cams);
  } else keep_caller_order(cams);
  HostTables T;
  if (int rc = build_record_tables(P, cams, opt, groups, T, lap)) return rc;
  SPattern S;
  if (cams.use_graph) s_pattern_index(cams, plan, graph, S);
  else if (int rc = s_pattern_skyline(cams, T, opt, one_rank, false, S, plan)) return rc;
  SlabTables slabs;
  if (int rc = assign_slabs(T.chunks, slabs)) return rc;
  if (int rc = slab_reduction_tables(T, cams, plan, S, true, slabs)) return rc;

  const void* src = nullptr;
  int64_t bytes = 0;
  const int64_t nr = T.nrec, nf = T.nfixed;
  std::vector<int32_t> cam_of_slot;
  int64_t info[10];
  const uint8_t on_device = 0;
  auto vec = [&](const auto& v) { src = v.data(); bytes = (int64_t)(sizeof(v[0]) * v.size()); };
  switch (which) {
    case 0: vec(T.chunks); break;
    case 1: vec(T.chunk_cams); break;
    case 2: src = T.rec_cam.data(); bytes = 4 * nr; break;
    case 3: src = T.rec_pt.data(); bytes = 4 * nr; break;
    case 4: src = T.rec_meta.data(); bytes = 4 * nr; break;
    case 5: src = T.rec_xy.data(); bytes = 16 * nr; break;
    case 6: src = T.rec_d.data(); bytes = 8 * nr; break;
    case 7: src = T.rec_m.data(); bytes = 8 * nr; break;
    case 8: src = T.rec_a.data(); bytes = 8 * nr; break;
    case 9: vec(T.pt_rec_start); break;
    case 10: vec(T.pt_kv); break;
    case 11: src = T.fx_cam.data(); bytes = 4 * nf; break;
    case 12: src = T.fx_pt.data(); bytes = 4 * nf; break;
    case 13: src = T.fx_meta.data(); bytes = 4 * nf; break;
    case 14: src = T.fx_xy.data(); bytes = 16 * nf; break;
    case 15: src = T.fx_d.data(); bytes = 8 * nf; break;
    case 16: src = T.fx_m.data(); bytes = 8 * nf; break;
    case 17: src = T.fx_a.data(); bytes = 8 * nf; break;
    case 18: vec(T.order); break;
    case 19: vec(slabs.dests); break;
    case 20: vec(slabs.srcs); break;
    case 21: vec(cams.slot); break;
    case 22: src = &on_device; bytes = 1; break;
    case 23: vec(T.blk_desc); break;
    case 24: vec(T.blk_ent_start); break;
    case 25: vec(T.ents); break;
    case 27: vec(T.lhdr); break;
    case 28: vec(S.sky_index); break;
    case 29: vec(S.sky_first); break;
    case 30: vec(S.sky_start); break;
    case 31: vec(cams.cmask); break;
    case 32: cam_of_slot = cam_of_slot_table(cams); vec(cam_of_slot); break;
    case 33: {
      DenseOverlap ov;
      LevelPlanDev lp;
      opt.apply_dense(cams.nt, plan, ov);
      level_plan_flags(plan, lp);
      double work = 0.0;
      dense_plan_numbers(cams.ncv, cams.nt, plan, ov, lp, &work, S.nblk, info);
      src = info; bytes = 80;
      break;
    }
    default: return fail(MPSFM_EINVAL, "unknown table");
  }
  if (!out || cap < bytes) return bytes;
  if (bytes > 0) std::memcpy(out, src, (size_t)bytes);
  return bytes;
}

int mpsfm_ba_sweep_parts(mpsfm_ba_handle* h, float ms[3], int64_t info[4]) {
  if (!h) return fail(MPSFM_EINVAL, "handle is NULL");
  HIP_TRY(hipSetDevice(h->device));
  if (ms)
    for (int k = 0; k < 3; ++k) HIP_TRY(hipEventElapsedTime(&ms[k], h->ev[k], h->ev[k + 1]));
  if (info) { info[0] = h->n_dense; info[1] = h->nchunks - h->n_dense; info[2] = h->nlong; info[3] = h->n_red_dests; }
  return 0;
}

// phase clocks of the last single-launch solve (local_lm.hip), 100 MHz ticks: sweep, barrier 1, dense + cameras, update, barrier 2,
// decision, iterations, then (debug flag 64 << 8) inside the dense phase: assemble, stacked factorisations, their barrier, trailing
// updates, back substitution (none of these while mpsfm_debug_local_skew is armed: slot 11 then sums the ticks the hook waited);
// returns 0 when the handle does not take that path
int mpsfm_debug_local_clocks(mpsfm_ba_handle* h, int64_t out[12]) {
  if (!h || !h->local_ok) return 0;
  if (hipSetDevice(h->device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) return 0;
  if (hipMemcpy(out, h->d_local_sync + 1, sizeof(int64_t) * 12, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  return 1;
}
// test hook of the single-launch solver: in every solve launched from now on, workgroup `chunk` (negative: counted from the last;
// reduced modulo the grid) waits `ticks` of the 100 MHz wall clock at each phase point of `phase_mask` (bits: P after barrier 0, A
// track sweep, B after barrier 1, D update sweep, E after barrier 2); clock slot 11 of mpsfm_debug_local_clocks sums the wait.
// (0, 0, 0): off.  At most 2 ms per point, far below the grid barrier's bounded spin.
int mpsfm_debug_local_skew(int32_t chunk, int32_t phase_mask, int64_t ticks) {
  if (ticks < 0 || ticks > kSkewMaxTicks) return fail(MPSFM_EINVAL, "skew ticks must lie in [0, 200000] (2 ms at 100 MHz)");
  if (phase_mask & ~kSkewAll) return fail(MPSFM_EINVAL, "skew phase mask: bits 0-4 (P, A, B, D, E)");
  g_skew_chunk = chunk; g_skew_mask = phase_mask; g_skew_ticks = ticks;
  return 0;
}
int mpsfm_ba_dense_solve_once(mpsfm_ba_handle* h, float* elapsed_ms) {
  if (!h) return fail(MPSFM_EINVAL, "handle is NULL");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipEventRecord(h->ev[0], h->stream));
  if (int rc = run_dense(h, h->last_radius)) return rc;
  HIP_TRY(hipEventRecord(h->ev[1], h->stream));
  HIP_TRY(hipMemsetAsync(h->d_fail, 0, sizeof(int), h->stream));  // no k_cam_update follows here to re-arm the flag
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
  if (elapsed_ms) *elapsed_ms = ms;
  return 0;
}

// S and rhs of the last sweep (with the LM damping of its radius), plus the last dense solution
// S and the right-hand side in the CALLER's camera order (6 rows per variable camera), whatever slot order the handle uses.
int mpsfm_ba_get_reduced_system(mpsfm_ba_handle* h, double* S, double* rhs, int32_t n) {
  if (!h) return fail(MPSFM_EINVAL, "handle is NULL");
  if (n != h->n_user) return fail(MPSFM_EINVAL, "n does not match the reduced dimension");
  HIP_TRY(hipSetDevice(h->device));
  std::vector<double> red((size_t)h->red_count);
  HIP_TRY(hipMemcpyAsync(red.data(), h->d_red, sizeof(double) * red.size(), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  const double* Sb = red.data(); const double* gc = Sb + h->sblk_count; const double* wv = gc + h->n_user; const double* dU = wv + h->n_user;
  const mpsfm_ba_options& o = h->opt;
  const BlockSky sky{h->spat.sky_first.data(), h->spat.sky_start.data(), h->spat.sky_index.empty() ? nullptr : h->spat.sky_index.data(), h->ncv};
  for (int R = 0; R < n; ++R)
    for (int C = 0; C < n; ++C) {
      const int br = h->nat_slot[(size_t)(R / 6)], a = R % 6, bc = h->nat_slot[(size_t)(C / 6)], b = C % 6;
      double v;
      const int lo = std::min(br, bc), hi = std::max(br, bc);
      if (!sky_has(sky, lo, hi)) v = 0.0;
      else if (br < bc) v = Sb[sky_block(sky, br, bc) * 36 + a * 6 + b];
      else if (br > bc) v = Sb[sky_block(sky, bc, br) * 36 + b * 6 + a];
      else v = Sb[sky_block(sky, br, br) * 36 + (a <= b ? a * 6 + b : b * 6 + a)];
      if (R == C) v += std::min(std::max(dU[6 * br + a], o.min_lm_diagonal), o.max_lm_diagonal) / h->last_radius;
      if (S) S[(size_t)R * n + C] = v;
    }
  if (rhs) for (int i = 0; i < n; ++i) { const int q = 6 * h->nat_slot[(size_t)(i / 6)] + i % 6; rhs[i] = wv[q] - gc[q]; }
  return 0;
}

int mpsfm_ba_get_dense_solution(mpsfm_ba_handle* h, double* y, int32_t n) {
  if (!h || !y) return fail(MPSFM_EINVAL, "handle or y is NULL");
  if (n != h->n_user) return fail(MPSFM_EINVAL, "n does not match the reduced dimension");
  HIP_TRY(hipSetDevice(h->device));
  std::vector<double> ys((size_t)std::max(h->n_user, 1));
  HIP_TRY(hipMemcpyAsync(ys.data(), h->d_yc, sizeof(double) * (size_t)h->n_user, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (int i = 0; i < n; ++i) y[i] = ys[(size_t)(6 * h->nat_slot[(size_t)(i / 6)] + i % 6)];
  return 0;
}

}  // extern "C"
