// What the host phases of the table build (build_host.hip) and their callers (ba_build.hip, dev_resources.hip, ba_solver.hip) share: host threads (run_parts on a
// persistent worker pool), recycled host blocks (HostBlockCache / HostBuf) and the pair tables of one chunk.  No device involved.
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "common.h"
#include "dev_resources.h"

namespace mpsfm {

// Large host blocks of the table build come from a process-wide cache: a fresh 40 MB block costs its page faults on first
// touch and an munmap on release (several ms per create at C3); a recycled one costs neither.  Power-of-two buckets from
// 1 MB, at most 512 MB kept (MPSFM_HOST_CACHE_MB).
struct HostBlockCache {
  static constexpr size_t kMinBytes = size_t(1) << 20;
  const size_t kHostCacheBytes = [] {  // MPSFM_HOST_CACHE_MB: how much released host memory is kept for the next build (0: none)
    const char* e = std::getenv("MPSFM_HOST_CACHE_MB");
    return (size_t)((e && std::atoi(e) >= 0) ? std::atoi(e) : 512) << 20;
  }();
  std::mutex mu;
  std::vector<std::pair<size_t, void*>> free_blocks;
  size_t cached = 0;
  static size_t bucket(size_t bytes) { size_t b = kMinBytes; while (b < bytes) b <<= 1; return b; }
  void* take(size_t bytes, size_t& got) {
    if (bytes < kMinBytes) { got = 0; return ::operator new(std::max<size_t>(bytes, 1)); }
    got = bucket(bytes);
    {
      std::lock_guard<std::mutex> lk(mu);
      for (size_t i = 0; i < free_blocks.size(); ++i)
        if (free_blocks[i].first == got) {
          void* p = free_blocks[i].second;
          free_blocks[i] = free_blocks.back(); free_blocks.pop_back();
          cached -= got;
          return p;
        }
    }
    return ::operator new(got);
  }
  void give(void* p, size_t got) {
    if (!p) return;
    if (got) {
      std::lock_guard<std::mutex> lk(mu);
      if (cached + got <= kHostCacheBytes) { free_blocks.emplace_back(got, p); cached += got; return; }
    }
    ::operator delete(p);
  }
  ~HostBlockCache() { for (auto& b : free_blocks) ::operator delete(b.second); }
};
HostBlockCache& host_cache();

// uninitialised host array of trivially copyable elements (std::vector would zero-fill tens of MB on one thread)
template <typename T>
struct HostBuf {
  static_assert(std::is_trivially_copyable<T>::value && std::is_trivially_destructible<T>::value, "HostBuf holds raw storage");
  T* p = nullptr;
  size_t n = 0, got = 0;
  HostBuf() = default;
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  ~HostBuf() { host_cache().give(p, got); }
  void alloc(size_t k) {
    host_cache().give(p, got);
    p = static_cast<T*>(host_cache().take(std::max<size_t>(k, 1) * sizeof(T), got));
    n = k;
  }
  void release() { host_cache().give(p, got); p = nullptr; n = got = 0; }
  size_t size() const { return n; }
  T* data() { return p; }
  const T* data() const { return p; }
  T& operator[](size_t i) { return p[i]; }
  const T& operator[](size_t i) const { return p[i]; }
};

// ---- host threads for the table build (plain std::thread: no OpenMP runtime beside torch's) -------
// CPUs this process may use: scheduler affinity capped by the cgroup quota; MPSFM_HOST_THREADS overrides.
int host_threads();
// Persistent workers for the phases of the table build: creating and joining 15 threads costs ~0.4 ms, and one create runs
// a dozen phases.  One job at a time; a caller that finds the pool busy (another handle being created) starts plain threads
// as before.  Parts are claimed with the job's generation, so a worker that wakes late never touches a newer job; a forked
// child starts over with a pool of its own (the parent's workers do not exist there).
class HostPool {
 public:
  typedef void (*Call)(void* ctx, int part, int nparts);
  // false: the pool is busy, nothing ran
  bool try_run(int nparts, Call call, void* ctx) {
    std::unique_lock<std::mutex> job(job_mu_, std::try_to_lock);
    if (!job.owns_lock()) return false;
    {
      std::lock_guard<std::mutex> lk(mu_);
      if (workers_.empty()) {
        const int nw = std::max(host_threads() - 1, 1);
        for (int i = 0; i < nw; ++i) workers_.emplace_back([this] { work(); });
      }
      call_ = call; ctx_ = ctx; nparts_ = nparts;
      done_.store(0, std::memory_order_relaxed);
      ++gen_;
      state_.store((gen_ << 32) | 1u, std::memory_order_release);  // part 0 is the caller's
    }
    cv_work_.notify_all();
    call(ctx, 0, nparts);
    finish_part();
    claim_loop(gen_, call, ctx, nparts);
    std::unique_lock<std::mutex> lk(mu_);
    cv_done_.wait(lk, [&] { return done_.load(std::memory_order_acquire) == nparts; });
    return true;
  }
  ~HostPool() {
    { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
    cv_work_.notify_all();
    for (auto& w : workers_) w.join();
  }

 private:
  void finish_part() {
    if (done_.fetch_add(1, std::memory_order_acq_rel) + 1 == nparts_) { std::lock_guard<std::mutex> lk(mu_); cv_done_.notify_all(); }
  }
  void claim_loop(uint64_t gen, Call call, void* ctx, int nparts) {
    uint64_t s = state_.load(std::memory_order_acquire);
    while ((s >> 32) == gen && (int)(s & 0xffffffffu) < nparts) {
      if (state_.compare_exchange_weak(s, s + 1, std::memory_order_acq_rel)) {
        call(ctx, (int)(s & 0xffffffffu), nparts);
        finish_part();
        s = state_.load(std::memory_order_acquire);
      }
    }
  }
  void work() {
    uint64_t seen = 0;
    for (;;) {
      Call call; void* ctx; int nparts; uint64_t gen;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_work_.wait(lk, [&] { return stop_ || gen_ != seen; });
        if (stop_) return;
        seen = gen = gen_; call = call_; ctx = ctx_; nparts = nparts_;
      }
      claim_loop(gen, call, ctx, nparts);
    }
  }
  std::mutex job_mu_, mu_;
  std::condition_variable cv_work_, cv_done_;
  std::vector<std::thread> workers_;
  std::atomic<uint64_t> state_{0};
  std::atomic<int> done_{0};
  uint64_t gen_ = 0;
  Call call_ = nullptr; void* ctx_ = nullptr; int nparts_ = 0;
  bool stop_ = false;
};
HostPool* host_pool();
bool host_pool_enabled();  // MPSFM_HOST_POOL=0: plain threads for every job
// f(part, nparts) on nparts threads (the calling thread takes part 0)
template <class F>
void run_parts(int nparts, F&& f) {
  if (nparts <= 1) { f(0, std::max(nparts, 1)); return; }
  typedef typename std::remove_reference<F>::type Fn;
  if (host_pool_enabled() && host_pool()->try_run(nparts, [](void* c, int t, int n) { (*static_cast<Fn*>(c))(t, n); }, const_cast<void*>(static_cast<const void*>(&f)))) return;
  std::vector<std::thread> th;
  th.reserve((size_t)std::max(nparts - 1, 0));
  for (int t = 1; t < nparts; ++t) th.emplace_back([&f, t, nparts] { f(t, nparts); });
  f(0, nparts);
  for (auto& x : th) x.join();
}
// f(begin, end) over [0, n) cut into nearly equal contiguous parts
template <class F>
void parallel_ranges(int64_t n, int64_t min_grain, F&& f) {
  const int parts = (int)std::max<int64_t>(1, std::min<int64_t>(host_threads(), n / std::max<int64_t>(min_grain, 1)));
  if (parts <= 1) { f((int64_t)0, n); return; }
  run_parts(parts, [&](int t, int np) { f(n * t / np, n * (t + 1) / np); });
}

struct Blk { int32_t cam; int32_t key; uint8_t kind; int64_t src; };

// Pair tables of ONE chunk for the general kernel, appended to (blk_desc, ents, blk_ent_start): the Schur pairs of its variable
// landmarks grouped by the 6x6 destination block (counting sort, heaviest blocks first), cut into work items of at most kItemPairs
// pairs; a dense chunk only gets its sentinel.  `rec_meta` is indexed by the global record, `pt_kv` / `pt_rec_start` / `order` by the
// re-ordered landmark.  Shared by the host build and by the device build's general chunks.
struct PairEnt { uint16_t key; uint32_t ent; };
struct PairScratch {
  std::vector<PairEnt> pe, pe_sorted;
  std::vector<std::pair<int, int>> blk_order, items;  // (count, first index into pe)
  std::vector<int32_t> cnt;
};
void append_pair_tables(ChunkHdr& H, const uint32_t* rec_meta, const uint16_t* pt_kv, const int32_t* pt_rec_start, const int32_t* order,
                        const uint8_t* pt_const, std::vector<uint32_t>& o_blk_desc, std::vector<uint32_t>& o_ents, std::vector<int32_t>& o_blk_ent_start,
                        PairScratch& S);

}  // namespace mpsfm
