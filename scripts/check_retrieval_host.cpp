// Stand-alone check of the host half of mpsfm_retrieve_topk (csrc/retrieval.hip): the argument checks, the scan of host inputs and
// the empty paths, all of which return before any HIP call, plus one valid call, which is refused (MPSFM_ENODEVICE) on a machine
// without a device and computed with one.  Meant to be built with the host sanitizers and run on a CPU:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         scripts/check_retrieval_host.cpp mpsfm_amd/csrc/retrieval.hip mpsfm_amd/csrc/dev_resources.hip -o check_retrieval_host
//   ./check_retrieval_host
//
// Buffers are exactly as long as the header says, so a read or write past them is the sanitizer's to report.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../include/mpsfm_hip.h"
#include "../mpsfm_amd/csrc/host_parts.h"

// what the two library files linked here expect from files that are not: the error text (ba_solver.hip) and the host thread pool
// behind the staged uploads (build_host.hip), which no retrieval call uses
namespace mpsfm {
int host_threads() { return 1; }
bool host_pool_enabled() { return false; }
HostPool* host_pool() { return nullptr; }
}  // namespace mpsfm
extern "C" const char* mpsfm_last_error(void) { return mpsfm::g_err.c_str(); }

static int failures = 0;
#define EXPECT(what, cond)                                       \
  do {                                                           \
    if (!(cond)) { std::printf("FAILED: %s\n", what); ++failures; } \
  } while (0)

int main() {
  const int64_t nq = 3, nd = 5;
  const int32_t dim = 4, K = 2;
  std::vector<float> q(nq * dim, 0.5f), d(nd * dim, 0.25f);
  std::vector<int32_t> qi(nq, 1), di(nd, 2), idx(nq * K, 7), cnt(nq, 7);
  std::vector<double> val(nq * K, 7.0);
  mpsfm_retrieval_options o;
  mpsfm_retrieval_default_options(&o);
  EXPECT("defaults", o.num_select == 20 && o.use_min_score == 1 && o.min_score == 0.0 && o.column_ranges == 0 && o.inputs_on_device == 0 && !o.stream);
  mpsfm_retrieval_default_options(nullptr);
  o.num_select = K;
  auto call = [&](int64_t a, int64_t b, int32_t dm, const float* x, const float* y, const int32_t* ia, const int32_t* ib,
                  const mpsfm_retrieval_options* opts, int32_t* ii, double* vv, int32_t* cc, mpsfm_retrieval_info* info = nullptr) {
    return mpsfm_retrieve_topk(a, b, dm, x, y, ia, ib, opts, 0, ii, vv, cc, info);
  };
  EXPECT("negative nq", call(-1, nd, dim, q.data(), d.data(), nullptr, nullptr, &o, idx.data(), val.data(), cnt.data()) == MPSFM_EINVAL);
  EXPECT("negative nd", call(nq, -1, dim, q.data(), d.data(), nullptr, nullptr, &o, idx.data(), val.data(), cnt.data()) == MPSFM_EINVAL);
  EXPECT("too many rows", call((1 << 24) + 1, nd, dim, q.data(), d.data(), nullptr, nullptr, &o, idx.data(), val.data(), cnt.data()) == MPSFM_EINVAL);
  EXPECT("dim 0", call(nq, nd, 0, q.data(), d.data(), nullptr, nullptr, &o, idx.data(), val.data(), cnt.data()) == MPSFM_EINVAL);
  EXPECT("dim 65537", call(nq, nd, 65537, q.data(), d.data(), nullptr, nullptr, &o, idx.data(), val.data(), cnt.data()) == MPSFM_EINVAL);
  EXPECT("NULL query", call(nq, nd, dim, nullptr, d.data(), nullptr, nullptr, &o, idx.data(), val.data(), cnt.data()) == MPSFM_EINVAL);
  EXPECT("NULL db", call(nq, nd, dim, q.data(), nullptr, nullptr, nullptr, &o, idx.data(), val.data(), cnt.data()) == MPSFM_EINVAL);
  EXPECT("NULL indices", call(nq, nd, dim, q.data(), d.data(), nullptr, nullptr, &o, nullptr, val.data(), cnt.data()) == MPSFM_EINVAL);
  EXPECT("NULL scores", call(nq, nd, dim, q.data(), d.data(), nullptr, nullptr, &o, idx.data(), nullptr, cnt.data()) == MPSFM_EINVAL);
  EXPECT("NULL counts", call(nq, nd, dim, q.data(), d.data(), nullptr, nullptr, &o, idx.data(), val.data(), nullptr) == MPSFM_EINVAL);
  EXPECT("one id array", call(nq, nd, dim, q.data(), d.data(), qi.data(), nullptr, &o, idx.data(), val.data(), cnt.data()) == MPSFM_EINVAL);
  EXPECT("the other id array", call(nq, nd, dim, q.data(), d.data(), nullptr, di.data(), &o, idx.data(), val.data(), cnt.data()) == MPSFM_EINVAL);
  EXPECT("default num_select exceeds nd", call(nq, nd, dim, q.data(), d.data(), nullptr, nullptr, nullptr, idx.data(), val.data(), cnt.data()) == MPSFM_EINVAL);
  for (int32_t k : {0, -1, 129, 6}) {
    mpsfm_retrieval_options b = o;
    b.num_select = k;
    EXPECT("num_select", call(nq, nd, dim, q.data(), d.data(), nullptr, nullptr, &b, idx.data(), val.data(), cnt.data()) == MPSFM_EINVAL);
  }
  for (double bad : {std::nan(""), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()}) {
    mpsfm_retrieval_options b = o;
    b.min_score = bad;
    EXPECT("min_score", call(nq, nd, dim, q.data(), d.data(), nullptr, nullptr, &b, idx.data(), val.data(), cnt.data()) == MPSFM_EINVAL);
    std::vector<float> x = q, y = d;
    x.back() = (float)bad;  // the last element of each array: the scan reads all of it and no more
    y.back() = (float)bad;
    EXPECT("non-finite query", call(nq, nd, dim, x.data(), d.data(), nullptr, nullptr, &o, idx.data(), val.data(), cnt.data()) == MPSFM_EINVAL);
    EXPECT("non-finite db", call(nq, nd, dim, q.data(), y.data(), nullptr, nullptr, &o, idx.data(), val.data(), cnt.data()) == MPSFM_EINVAL);
    std::vector<int32_t> i5(nd * K);
    std::vector<double> v5(nd * K);
    std::vector<int32_t> c5(nd);
    EXPECT("non-finite query == db", call(nd, nd, dim, y.data(), y.data(), nullptr, nullptr, &o, i5.data(), v5.data(), c5.data()) == MPSFM_EINVAL);
  }
  mpsfm_retrieval_options neg = o;
  neg.column_ranges = -1;
  EXPECT("negative column_ranges", call(nq, nd, dim, q.data(), d.data(), nullptr, nullptr, &neg, idx.data(), val.data(), cnt.data()) == MPSFM_EINVAL);
  // empty sides: no device
  mpsfm_retrieval_info info;
  EXPECT("nd == 0", call(nq, 0, dim, q.data(), nullptr, nullptr, nullptr, &o, idx.data(), val.data(), cnt.data(), &info) == 0);
  bool cleared = info.num_pairs == 0 && info.num_syncs == 0;
  for (int64_t i = 0; i < nq * K; ++i) cleared = cleared && idx[i] == -1 && val[i] == 0.0;
  for (int64_t i = 0; i < nq; ++i) cleared = cleared && cnt[i] == 0;
  EXPECT("nd == 0 clears the outputs", cleared);
  mpsfm_retrieval_options big = o;
  big.num_select = 128;
  std::vector<int32_t> ib(nq * 128);
  std::vector<double> vb(nq * 128);
  EXPECT("nd == 0 at the cap", call(nq, 0, dim, q.data(), nullptr, qi.data(), di.data(), &big, ib.data(), vb.data(), cnt.data()) == 0);
  EXPECT("nq == 0", call(0, nd, dim, nullptr, d.data(), nullptr, nullptr, &o, nullptr, nullptr, nullptr) == 0);
  EXPECT("both empty", call(0, 0, dim, nullptr, nullptr, nullptr, nullptr, &o, nullptr, nullptr, nullptr) == 0);
  // a valid call
  const int rc = call(nq, nd, dim, q.data(), d.data(), qi.data(), di.data(), &o, idx.data(), val.data(), cnt.data(), &info);
  std::printf("valid call: %d (%s)\n", rc, rc == 0 ? "computed" : mpsfm_last_error());
  EXPECT("valid call", rc == 0 || rc == MPSFM_ENODEVICE);
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
