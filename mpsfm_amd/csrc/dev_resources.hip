// Process-wide device resources of libmpsfm_hip (dev_resources.h): the caching device allocator, the pools of streams, events
// and pinned blocks, and the pinned staging uploader.  Host code; every object here is per device and never destroyed (the HIP
// runtime may be gone at static-destruction time).
#include "dev_resources.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "../../include/mpsfm_hip_debug.h"
#include "host_parts.h"

namespace mpsfm {

thread_local std::string g_err;

// slot of the current device in the per-device arrays below
static int device_slot() { int d = 0; (void)hipGetDevice(&d); return std::min(std::max(d, 0), 15); }

// ---- caching device allocator --------------------------------------------------------------------------
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
    const int dev = device_slot();
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

// ---- streams, events, pinned blocks --------------------------------------------------------------------
namespace {
struct HandleResources {
  std::mutex mu;
  std::vector<hipStream_t> streams[16];
  std::vector<hipEvent_t> events[2][16];  // [timing]
  std::vector<void*> pinned[16];  // blocks of kPinnedBytes
  int64_t out_streams[16] = {}, out_events[16] = {}, out_pinned[16] = {};  // handed out and not yet given back (mpsfm_debug_resources)
};
HandleResources& pool() { static HandleResources* r = new HandleResources(); return *r; }
// a recycled object of the current device or a fresh one from `make` / an object back to its list
template <typename T, typename F>
hipError_t pool_take(std::vector<T> (&lists)[16], int64_t (&out)[16], T* x, F&& make) {
  std::lock_guard<std::mutex> lk(pool().mu);
  const int dev = device_slot();
  std::vector<T>& v = lists[dev];
  if (!v.empty()) { *x = v.back(); v.pop_back(); }
  else if (hipError_t e = make(x)) return e;
  ++out[dev];
  return hipSuccess;
}
template <typename T>
void pool_give(std::vector<T> (&lists)[16], int64_t (&out)[16], T x) {
  if (!x) return;
  std::lock_guard<std::mutex> lk(pool().mu);
  const int dev = device_slot();
  lists[dev].push_back(x);
  --out[dev];
}
}  // namespace

// ---- the owner (dev_resources.h): the only caller of the allocator and the pools ----------------------------
void* DeviceBlocks::get(size_t bytes) {
  void* p = dev_cache().alloc(bytes);
  if (p) blocks_.push_back(p);
  else ok_ = false;
  return p;
}
void* DeviceBlocks::get_host(size_t bytes) {
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
  hosts_.push_back(p);
  return p;
}
hipError_t DeviceBlocks::pinned(void** p) {
  hipError_t e = pool_take(pool().pinned, pool().out_pinned, p, [](void** q) { return hipHostMalloc(q, kPinnedBytes, hipHostMallocDefault); });
  if (e == hipSuccess) pinned_.push_back(*p);
  return e;
}
hipError_t DeviceBlocks::event(hipEvent_t* ev, bool timing) {
  hipError_t e = pool_take(pool().events[timing], pool().out_events, ev,
                           [timing](hipEvent_t* q) { return timing ? hipEventCreate(q) : hipEventCreateWithFlags(q, hipEventDisableTiming); });
  if (e == hipSuccess) events_[timing].push_back(*ev);
  return e;
}
hipError_t DeviceBlocks::stream(hipStream_t* s) {
  hipError_t e = pool_take(pool().streams, pool().out_streams, s, [](hipStream_t* q) { return hipStreamCreateWithFlags(q, hipStreamNonBlocking); });
  if (e == hipSuccess) { streams_.push_back(*s); idle_.push_back(*s); }
  return e;
}
void DeviceBlocks::adopt(DeviceBlocks&& o) {
  auto take = [](auto& dst, auto& src) { dst.insert(dst.end(), src.begin(), src.end()); src.clear(); };
  take(blocks_, o.blocks_); take(hosts_, o.hosts_); take(pinned_, o.pinned_); take(events_[0], o.events_[0]); take(events_[1], o.events_[1]);
  take(streams_, o.streams_); take(idle_, o.idle_);
  ok_ = ok_ && o.ok_;
}
void DeviceBlocks::drop(void* p) {
  auto it = std::find(blocks_.begin(), blocks_.end(), p);
  if (it == blocks_.end()) return;
  blocks_.erase(it);
  dev_cache().release(p);
}
void DeviceBlocks::reset() {
  for (hipStream_t s : idle_) (void)hipStreamSynchronize(s);
  for (void* p : blocks_) dev_cache().release(p);
  for (void* p : hosts_) (void)hipHostFree(p);
  for (void* p : pinned_) pool_give(pool().pinned, pool().out_pinned, p);
  for (int timing = 0; timing < 2; ++timing)
    for (hipEvent_t e : events_[timing]) pool_give(pool().events[timing], pool().out_events, e);
  for (auto it = streams_.rbegin(); it != streams_.rend(); ++it) pool_give(pool().streams, pool().out_streams, *it);
  blocks_.clear(); hosts_.clear(); pinned_.clear(); events_[0].clear(); events_[1].clear(); streams_.clear(); idle_.clear();
}

// ---- pinned staging uploader ---------------------------------------------------------------------------
namespace {
// pageable -> pinned copy of one staging half: a single thread's memcpy (~20 GB/s here) is what bounded the uploads, not the bus;
// a few host threads in parallel
void staged_copy(char* dst, const char* src, size_t n) {
  constexpr size_t kGrain = (size_t)1 << 20;
  static const int max_threads = [] { const char* e = std::getenv("MPSFM_STAGE_THREADS"); return e ? std::max(std::atoi(e), 1) : 6; }();
  const int parts = (int)std::min<size_t>((size_t)std::min(host_threads(), max_threads), n / kGrain);
  if (parts <= 1) { std::memcpy(dst, src, n); return; }
  run_parts(parts, [&](int t, int np) {
    const size_t a = (n * (size_t)t / (size_t)np) & ~(size_t)63, b = t + 1 == np ? n : ((n * (size_t)(t + 1) / (size_t)np) & ~(size_t)63);
    std::memcpy(dst + a, src + a, b - a);
  });
}
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
      if (busy[hf]) { MPSFM_TRY(hipEventSynchronize(ev[hf])); busy[hf] = false; }
      staged_copy(buf + (size_t)hf * kHalf, s, n);
      MPSFM_TRY(hipMemcpyAsync(d, buf + (size_t)hf * kHalf, n, hipMemcpyHostToDevice, st));
      MPSFM_TRY(hipEventRecord(ev[hf], st));
      busy[hf] = true;
      s += n; d += n; bytes -= n;
    }
    return 0;
  }
  int drain() {
    MPSFM_TRY(hipStreamSynchronize(st));
    busy[0] = busy[1] = false;
    return 0;
  }
};
Stager g_stagers[16];  // one per device ordinal
Stager& stager() { return g_stagers[device_slot()]; }
}  // namespace

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
int staged_h2d(void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return 0;
  if (int rc = staged_upload(dst, src, bytes)) return rc;
  return staged_drain();
}

}  // namespace mpsfm

// Diagnostics / tests: what the current process holds of `device`'s caches — live device blocks and their bytes, and the
// pooled streams, events and pinned blocks handed out and not yet given back.  Equal before and after a balanced call.
extern "C" int mpsfm_debug_resources(int32_t device, int64_t out[5]) {
  using namespace mpsfm;
  if (!out || device < 0 || device > 15) return fail(MPSFM_EINVAL, "mpsfm_debug_resources: out is NULL or the device ordinal is out of range");
  out[0] = out[1] = 0;
  {
    DevCache& C = dev_cache();
    std::lock_guard<std::mutex> lk(C.mu);
    for (const auto& kv : C.live)
      if (kv.second.second == device) { ++out[0]; out[1] += (int64_t)kv.second.first; }
  }
  HandleResources& R = pool();
  std::lock_guard<std::mutex> lk(R.mu);
  out[2] = R.out_streams[device]; out[3] = R.out_events[device]; out[4] = R.out_pinned[device];
  return 0;
}
