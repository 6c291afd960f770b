// Process-wide device resources (dev_resources.hip) and the error helper every host file shares: the caching device allocator,
// recycled streams / events / pinned blocks, and uploads through the pinned staging buffer.  Host code only and no
// floating-point arithmetic: this header may be included on either side of a header that sets `#pragma clang fp contract`.
#pragma once
#include <cstddef>
#include <string>

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
void* cached_malloc(size_t bytes);
void cached_free(void* p);
// Streams, events and the small pinned scalar blocks of a handle are recycled the same way: creating and destroying them
// costs more than a whole solve of a small problem.  Per device; never destroyed.  A released stream must be idle.
hipError_t pooled_stream(hipStream_t* s);  // non-blocking
void release_stream(hipStream_t s);
hipError_t pooled_event(hipEvent_t* e, bool timing);
void release_event(hipEvent_t e, bool timing);
constexpr size_t kPinnedBytes = 4096;
hipError_t pooled_pinned(void** p);  // a block of kPinnedBytes
void release_pinned(void* p);

// Uploads of caller / table memory go through a pinned staging buffer per device (two halves, the host copy into one overlaps
// the DMA out of the other).  Handing pageable memory to hipMemcpy directly makes the runtime pin and later unpin every source
// range: measured 17 ms of stall after a 40 MB table upload.
int staged_upload(void* dst, const void* src, size_t bytes);  // queued: complete after staged_drain()
int staged_drain();                                            // waits for everything queued
int staged_h2d(void* dst, const void* src, size_t bytes);     // queued and drained: complete on return

template <typename T>
int dev_alloc(T** p, size_t count) {
  if (count == 0) count = 1;
  *p = (T*)cached_malloc(count * sizeof(T));
  if (!*p) return fail(MPSFM_ENOMEM, "hipMalloc failed");
  return 0;
}
// block + queued staged upload of anything with data() and size() (complete after staged_drain())
template <typename T, typename C>
int dev_upload(T** p, const C& v) {
  static_assert(sizeof(*v.data()) == sizeof(T), "element type of the table and of its device pointer differ");
  if (int rc = dev_alloc(p, v.size())) return rc;
  return staged_upload(*p, v.data(), v.size() * sizeof(T));
}
// several (pointer, table) pairs in a row; stops at the first failure
template <typename T, typename C, typename... More>
int dev_upload(T** p, const C& v, More&&... more) {
  if (int rc = dev_upload(p, v)) return rc;
  return dev_upload(more...);
}

}  // namespace mpsfm
