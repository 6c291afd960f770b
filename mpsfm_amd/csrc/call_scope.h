// What every stateless entry point shares on the host: the error helper, the device check and the per-call device scope
// (stream, cached blocks, optional event pair).  Host code only and no floating-point arithmetic: this header may be
// included on either side of a header that sets `#pragma clang fp contract`.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>

#include "common.h"
#include "dev_resources.h"

namespace mpsfm {

// host arrays a call refuses when they hold a NaN or an infinity
template <typename T>
inline bool all_finite(const T* a, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(a[i])) return false;
  return true;
}

// the device ordinal of a call: checked, then made current
inline int open_device(int32_t device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(MPSFM_ENODEVICE, "no HIP device visible: libmpsfm_hip has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(MPSFM_EINVAL, "device ordinal out of range");
  if (device >= kMaxDevices) return fail(MPSFM_EUNSUPPORTED, "device ordinals beyond 15 are not supported (per-device pools)");
  MPSFM_TRY(hipSetDevice(device));
  return 0;
}

struct CallScope {
  // Every call works on a non-blocking stream of its own from the pool, never on the legacy null stream: the library is
  // called from several host threads (tests, threaded callers), and null-stream copies / fills issued by one thread while
  // another thread's solve had a deep queue of launches in flight corrupted that solve (MI355X, ROCm 7.2: reproduced with
  // tests/test_gpu_fuzz.py::test_random_problems_concurrently until the last null-stream call was gone).
  hipStream_t st = nullptr;
  double ms = 0.0;  // device time of the segments closed by end()

  CallScope() = default;
  CallScope(const CallScope&) = delete;
  CallScope& operator=(const CallScope&) = delete;
  // the owner waits for the stream, then gives the blocks and the stream back (an early return on a failed call would
  // otherwise free memory that is still in use)
  ~CallScope() {
    own.reset();
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }

  // takes the stream, and the event pair of a call that reports its device time
  int open(bool timed = false) {
    MPSFM_TRY(own.stream(&st));
    if (timed) {
      MPSFM_TRY(hipEventCreate(&ev[0]));
      MPSFM_TRY(hipEventCreate(&ev[1]));
    }
    return 0;
  }

  // a cached block / pinned host memory that lives as long as the scope; nullptr: out of memory
  void* get(size_t bytes) { return own.get(bytes); }
  template <typename T>
  T* alloc(size_t count) { return own.alloc<T>(count); }
  template <typename T>
  T* host(size_t count) { return own.host<T>(count); }
  // block + queued staged upload (complete after staged_drain())
  template <typename T>
  int up(const T** dst, const T* src, size_t count) {
    T* p = alloc<T>(count);
    if (!p) return fail(MPSFM_ENOMEM, "hipMalloc failed");
    *dst = p;
    return staged_upload(p, src, sizeof(T) * count);
  }
  // block + copy on the call's stream; nullptr: out of memory
  template <typename T>
  T* put(const T* host, size_t count) {
    T* p = alloc<T>(count);
    if (p && count && host) (void)hipMemcpyAsync(p, host, count * sizeof(T), hipMemcpyHostToDevice, st);
    return p;
  }
  // device -> caller memory, complete on return
  hipError_t down(void* host, const void* dev, size_t bytes) {
    hipError_t e = hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st);
    return e != hipSuccess ? e : hipStreamSynchronize(st);
  }

  // a timed segment on the stream: begin() .. stop(), read with elapsed() once the stream is idle
  int begin() { MPSFM_TRY(hipEventRecord(ev[0], st)); return 0; }
  int stop() { MPSFM_TRY(hipEventRecord(ev[1], st)); return 0; }
  int elapsed(float* t) { MPSFM_TRY(hipEventElapsedTime(t, ev[0], ev[1])); return 0; }
  // closes a timed segment and adds it to ms: the stream is idle on return
  int end() {
    if (int rc = stop()) return rc;
    MPSFM_TRY(hipStreamSynchronize(st));
    float t = 0.f;
    if (int rc = elapsed(&t)) return rc;
    ms += t;
    return 0;
  }

 private:
  DeviceBlocks own;
  hipEvent_t ev[2] = {nullptr, nullptr};
};

// ---- inputs that are already on the device (the inputs_on_device / stream convention of include/mpsfm_hip.h)
inline int check_device_pointer(const void* p, int32_t device, const char* what) {
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, p) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != device) {
    (void)hipGetLastError();
    return fail(MPSFM_EINVAL, std::string(what) + " is not device memory of the call's device");
  }
  return 0;
}

// the call's stream waits for what the caller's stream has enqueued so far (stream == NULL: the inputs are complete)
inline int wait_for_caller(CallScope& A, void* stream) {
  if (!stream) return 0;
  hipEvent_t e = nullptr;
  MPSFM_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  hipError_t rc = hipEventRecord(e, (hipStream_t)stream);
  if (rc == hipSuccess) rc = hipStreamWaitEvent(A.st, e, 0);
  (void)hipEventDestroy(e);  // released once the recorded work is done
  MPSFM_TRY(rc);
  return 0;
}

}  // namespace mpsfm
