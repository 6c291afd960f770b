// Process-wide device resources (dev_resources.hip) and the error helper every host file shares: the caching device allocator,
// recycled streams / events / pinned blocks, and uploads through the pinned staging buffer.  Host code only and no
// floating-point arithmetic: this header may be included on either side of a header that sets `#pragma clang fp contract`.
#pragma once
#include <cstddef>
#include <string>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/mpsfm_hip.h"

namespace mpsfm {

extern thread_local std::string g_err;  // what mpsfm_last_error returns
inline int fail(int code, const std::string& m) { g_err = m; return code; }
#define MPSFM_TRY(expr)                                                                              \
  do {                                                                                               \
    hipError_t e_ = (expr);                                                                          \
    if (e_ != hipSuccess) return fail(MPSFM_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

// Caching device allocator: hipMalloc / hipFree cost 10-300 us each and a handle makes ~60 of them; freed blocks are kept
// per device (up to a cap) and handed out again — with whatever an earlier owner left in them: every consumer initialises
// what it reads (MPSFM_POISON=1 fills each block with 0xFF to prove it).
// Streams, events and the small pinned scalar blocks of a handle are recycled the same way: creating and destroying them
// costs more than a whole solve of a small problem.  Per device; never destroyed.  Both are reached through DeviceBlocks only.
constexpr size_t kPinnedBytes = 4096;

// Uploads of caller / table memory go through a pinned staging buffer per device (two halves, the host copy into one overlaps
// the DMA out of the other).  Handing pageable memory to hipMemcpy directly makes the runtime pin and later unpin every source
// range: measured 17 ms of stall after a 40 MB table upload.
int staged_upload(void* dst, const void* src, size_t bytes);  // queued: complete after staged_drain()
int staged_drain();                                            // waits for everything queued
int staged_h2d(void* dst, const void* src, size_t bytes);     // queued and drained: complete on return

// The owner of everything a call, a builder or a handle takes from the caches above, and the one place that gives it back
// (DESIGN.md section 4b): the destructor first waits for every stream that may still touch the resources — a block back in
// the process-wide cache is handed to another host thread's handle at once, a released stream must be idle — then releases
// them all, on the current device (a handle makes its device current first).  Move-only.
class DeviceBlocks {
 public:
  DeviceBlocks() = default;
  DeviceBlocks(DeviceBlocks&& o) noexcept { adopt(std::move(o)); }
  DeviceBlocks(const DeviceBlocks&) = delete;
  DeviceBlocks& operator=(const DeviceBlocks&) = delete;
  ~DeviceBlocks() { reset(); }

  // a cached device block of at least one element; nullptr: out of memory (ok() stays false from then on)
  void* get(size_t bytes);
  template <typename T>
  T* alloc(size_t count) { return (T*)get((count ? count : 1) * sizeof(T)); }
  template <typename T>
  int alloc(T** p, size_t count) { return (*p = alloc<T>(count)) ? 0 : fail(MPSFM_ENOMEM, "hipMalloc failed"); }
  bool ok() const { return ok_; }
  // block + queued staged upload of anything with data() and size() (complete after staged_drain()); several (pointer, table)
  // pairs in a row stop at the first failure
  template <typename T, typename C, typename... More>
  int upload(T** p, const C& v, More&&... more) {
    static_assert(sizeof(*v.data()) == sizeof(T), "element type of the table and of its device pointer differ");
    if (int rc = alloc(p, v.size())) return rc;
    if (int rc = staged_upload((void*)*p, v.data(), v.size() * sizeof(T))) return rc;  // (T may be const: a view's field)
    if constexpr (sizeof...(More) > 0) return upload(more...);
    return 0;
  }
  // pinned host memory of any size (read-backs that are plain DMA, not staged copies); nullptr: out of memory
  void* get_host(size_t bytes);
  template <typename T>
  T* host(size_t count) { return (T*)get_host((count ? count : 1) * sizeof(T)); }
  // recycled objects: a pinned block of kPinnedBytes, an event, a non-blocking stream (waited for like an idle_first stream)
  hipError_t pinned(void** p);
  hipError_t event(hipEvent_t* e, bool timing);
  hipError_t stream(hipStream_t* s);
  // a stream somebody else owns that works on these resources: waited for before anything goes back, never released
  void idle_first(hipStream_t s) { if (s) idle_.push_back(s); }

  void adopt(DeviceBlocks&& o);  // everything `o` owns and waits for
  void drop(void* p);            // one device block back early: the caller knows that no stream uses it any more
  void reset();                  // what the destructor does

 private:
  bool ok_ = true;
  std::vector<void*> blocks_, hosts_, pinned_;
  std::vector<hipEvent_t> events_[2];  // [timing]
  std::vector<hipStream_t> streams_, idle_;
};

}  // namespace mpsfm
