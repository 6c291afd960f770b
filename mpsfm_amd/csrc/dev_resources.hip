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
void* cached_malloc(size_t bytes) { return dev_cache().alloc(bytes); }
void cached_free(void* p) { dev_cache().release(p); }

// ---- streams, events, pinned blocks --------------------------------------------------------------------
namespace {
struct HandleResources {
  std::mutex mu;
  std::vector<hipStream_t> streams[16];
  std::vector<hipEvent_t> timing_events[16], plain_events[16];
  std::vector<void*> pinned[16];  // blocks of kPinnedBytes
};
HandleResources& pool() { static HandleResources* r = new HandleResources(); return *r; }
// a recycled object of the current device, if there is one / an object back to its list
template <typename T>
bool pool_take(std::vector<T> (&lists)[16], T* out) {
  HandleResources& R = pool();
  std::lock_guard<std::mutex> lk(R.mu);
  std::vector<T>& v = lists[device_slot()];
  if (v.empty()) return false;
  *out = v.back();
  v.pop_back();
  return true;
}
template <typename T>
void pool_give(std::vector<T> (&lists)[16], T x) {
  if (!x) return;
  HandleResources& R = pool();
  std::lock_guard<std::mutex> lk(R.mu);
  lists[device_slot()].push_back(x);
}
}  // namespace
hipError_t pooled_stream(hipStream_t* s) { return pool_take(pool().streams, s) ? hipSuccess : hipStreamCreateWithFlags(s, hipStreamNonBlocking); }
void release_stream(hipStream_t s) { pool_give(pool().streams, s); }
hipError_t pooled_event(hipEvent_t* e, bool timing) {
  if (pool_take(timing ? pool().timing_events : pool().plain_events, e)) return hipSuccess;
  return timing ? hipEventCreate(e) : hipEventCreateWithFlags(e, hipEventDisableTiming);
}
void release_event(hipEvent_t e, bool timing) { pool_give(timing ? pool().timing_events : pool().plain_events, e); }
hipError_t pooled_pinned(void** p) { return pool_take(pool().pinned, p) ? hipSuccess : hipHostMalloc(p, kPinnedBytes, hipHostMallocDefault); }
void release_pinned(void* p) { pool_give(pool().pinned, p); }

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
