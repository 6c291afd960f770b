// Sums over the ranks of a landmark-sharded bundle adjustment: RCCL, loaded at run time (no link-time dependency: single-GPU
// users never touch it), or the caller's all-reduce hook.
#include <cstring>
#include <string>

#include <dlfcn.h>

#include "ba_handle.h"

namespace mpsfm {

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
  std::string error(const char* call, int rc) const { return std::string(call) + ": " + (GetErrorString ? GetErrorString(rc) : "failed"); }
};
Rccl& rccl() { static Rccl* r = new Rccl(); return *r; }
constexpr int kNcclDouble = 8, kNcclSum = 0;  // ncclFloat64, ncclSum (rccl.h)

int rccl_allreduce(mpsfm_ba_handle* h, double* dbuf, int64_t count) {
  const int rc = rccl().AllReduce(dbuf, dbuf, (size_t)count, kNcclDouble, kNcclSum, h->comm, h->stream);
  if (rc != 0) return fail(MPSFM_ECOMM, rccl().error("ncclAllReduce", rc));
  return 0;
}
}  // namespace

int comm_init_rank(mpsfm_ba_handle* h) {
  const mpsfm_ba_options& o = h->opt;
  Rccl& R = rccl();
  if (!R.ok) return fail(MPSFM_ECOMM, "use_rccl: " + R.why);
  if (o.rank < 0 || o.rank >= o.world_size) return fail(MPSFM_EINVAL, "rank out of range");
  Rccl::UniqueId id;
  std::memcpy(id.internal, o.comm_id, sizeof(id.internal));
  const int nrc = R.CommInitRank(&h->comm, o.world_size, id, o.rank);
  if (nrc != 0) { h->comm = nullptr; return fail(MPSFM_ECOMM, R.error("ncclCommInitRank", nrc)); }
  return 0;
}
void comm_destroy(void* comm) {
  if (comm) (void)rccl().CommDestroy(comm);
}

int allreduce_host(mpsfm_ba_handle* h, double* buf, int64_t count) {
  if (count <= 0) return 0;
  if (h->comm) {  // host values travel through a device scratch block
    DeviceBlocks scratch;  // waits for the stream on every return: `buf` is complete and the block is free to go back
    scratch.idle_first(h->stream);
    double* d = scratch.alloc<double>((size_t)count);
    if (!d) return fail(MPSFM_ENOMEM, "hipMalloc failed");
    int rc = 0;
    if (hipMemcpyAsync(d, buf, sizeof(double) * (size_t)count, hipMemcpyHostToDevice, h->stream) != hipSuccess) rc = fail(MPSFM_EHIP, "hipMemcpyAsync failed");
    if (!rc) rc = rccl_allreduce(h, d, count);
    if (!rc && hipMemcpyAsync(buf, d, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, h->stream) != hipSuccess) rc = fail(MPSFM_EHIP, "hipMemcpyAsync failed");
    return rc;
  }
  if (!h->opt.allreduce) return 0;
  if (h->opt.allreduce(h->opt.allreduce_user, buf, count, 0, nullptr)) return fail(MPSFM_ECOMM, "all-reduce hook failed (host buffer)");
  return 0;
}
int allreduce_dev(mpsfm_ba_handle* h, double* buf, int64_t count) {
  if (count <= 0) return 0;
  if (h->comm) return rccl_allreduce(h, buf, count);
  if (!h->opt.allreduce) return 0;
  if (h->opt.allreduce(h->opt.allreduce_user, buf, count, 1, (void*)h->stream)) return fail(MPSFM_ECOMM, "all-reduce hook failed (device buffer)");
  return 0;
}

}  // namespace mpsfm

extern "C" int mpsfm_comm_unique_id(uint8_t id[128]) {
  using namespace mpsfm;
  if (!id) return fail(MPSFM_EINVAL, "id is NULL");
  Rccl& R = rccl();
  if (!R.ok) return fail(MPSFM_ECOMM, R.why);
  Rccl::UniqueId u;
  const int rc = R.GetUniqueId(&u);
  if (rc != 0) return fail(MPSFM_ECOMM, R.error("ncclGetUniqueId", rc));
  std::memcpy(id, u.internal, 128);
  return 0;
}
