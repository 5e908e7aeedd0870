// sqlm_host_par.h — host-side helpers of the setup: huge-page arrays, the
// persistent worker pool, run_threads and the phase timers. Plain C++ (no HIP).
#pragma once
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

namespace sqlm {

// Large host arrays on transparent huge pages. The setup's scatter and
// planning passes read 5M-edge arrays at random landmark runs and write the
// page-locked upload buffers; with 4 KiB pages nearly every run costs TLB
// misses. MADV_HUGEPAGE is set before the first touch (the box's THP mode is
// "madvise"); arrays under one huge page use malloc. (SQLM_HOST_HUGE=0: A/B.)
#ifndef SQLM_HOST_HUGE
#define SQLM_HOST_HUGE 1
#endif
constexpr size_t kHugePage = size_t(2) << 20;
inline size_t huge_len(size_t bytes) { return (bytes + kHugePage - 1) & ~(kHugePage - 1); }
// an anonymous mapping of huge_len(bytes), aligned to a huge page, advised; nullptr on failure
inline void *huge_map(size_t bytes) {
  const size_t len = huge_len(bytes);
  void *raw = mmap(nullptr, len + kHugePage, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  if (raw == MAP_FAILED) return nullptr;
  const uintptr_t r = (uintptr_t)raw, a = (r + kHugePage - 1) & ~(uintptr_t)(kHugePage - 1);
  if (a > r) munmap(raw, a - r);
  if (r + kHugePage > a) munmap((void *)(a + len), r + kHugePage - a);
  (void)madvise((void *)a, len, MADV_HUGEPAGE);
  return (void *)a;
}
template <class T>
struct HugeAlloc {
  using value_type = T;
  HugeAlloc() = default;
  template <class U>
  HugeAlloc(const HugeAlloc<U> &) {}
  static bool huge(size_t n) { return SQLM_HOST_HUGE && n * sizeof(T) >= kHugePage; }
  T *allocate(size_t n) {
    void *p = huge(n) ? huge_map(n * sizeof(T)) : std::malloc(std::max<size_t>(n, 1) * sizeof(T));
    if (!p) throw std::bad_alloc();
    return static_cast<T *>(p);
  }
  void deallocate(T *p, size_t n) {
    if (huge(n)) munmap(p, huge_len(n * sizeof(T)));
    else std::free(p);
  }
  template <class U>
  bool operator==(const HugeAlloc<U> &) const { return true; }
  template <class U>
  bool operator!=(const HugeAlloc<U> &) const { return false; }
};
template <class T>
using HVec = std::vector<T, HugeAlloc<T>>;

struct Timer {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double ms() const {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
};

// SQLM_PREP_TIMING=1: host phase times of a setup on stderr, one line per mark
// (the time since the previous mark). fmt takes the phase name and the ms.
struct PhaseTimer {
  const char *fmt;
  const bool on = std::getenv("SQLM_PREP_TIMING") != nullptr;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  explicit PhaseTimer(const char *f) : fmt(f) {}
  void operator()(const char *what) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, fmt, what, std::chrono::duration<double, std::milli>(now - t0).count());
    t0 = now;
  }
};
constexpr const char *kPhasePrepare = "prepare %-12s %8.2f ms\n";
constexpr const char *kPhaseTiles = "  tiles %-14s %8.2f ms\n";  // sub-phases of "tiles"

// Persistent host worker pool for the setup passes (a prepare() runs ~20
// parallel passes; starting and joining 15 threads each time cost ~0.4 ms per
// pass). One caller at a time: a context that finds it busy (another context
// preparing on another thread) falls back to threads of its own.
class HostPool {
 public:
  // never destroyed: a process (or a forked child, whose copy has no worker
  // threads) exits without joining threads that may not exist
  static HostPool &get() {
    static HostPool *p = new HostPool();
    return *p;
  }
  // fn(t) for t = 1 .. nth-1 on the workers while the caller runs fn(0).
  // In a child forked after the pool started (multiprocessing's default start
  // method) the workers do not exist: false, the caller starts plain threads.
  bool try_run(int nth, const std::function<void(int)> &fn) {
    if (getpid() != pid_) return false;
    std::unique_lock<std::mutex> busy(use_, std::try_to_lock);
    if (!busy.owns_lock()) return false;
    {
      std::lock_guard<std::mutex> lk(m_);
      while ((int)th_.size() < nth - 1) {
        const int id = (int)th_.size() + 1;
        th_.emplace_back([this, id] { worker(id); });
      }
      job_ = &fn;
      active_ = nth;
      pending_ = nth - 1;
      ++gen_;
    }
    cv_.notify_all();
    fn(0);
    std::unique_lock<std::mutex> lk(m_);
    done_.wait(lk, [this] { return pending_ == 0; });
    job_ = nullptr;
    return true;
  }
 private:
  HostPool() : pid_(getpid()) {}
  void worker(int id) {
    uint64_t seen = 0;
    std::unique_lock<std::mutex> lk(m_);
    for (;;) {
      cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
      if (stop_) return;
      seen = gen_;
      if (id >= active_) continue;
      const std::function<void(int)> *f = job_;
      lk.unlock();
      (*f)(id);
      lk.lock();
      if (--pending_ == 0) done_.notify_one();
    }
  }
  std::mutex use_, m_;
  std::condition_variable cv_, done_;
  std::vector<std::thread> th_;
  const std::function<void(int)> *job_ = nullptr;
  uint64_t gen_ = 0;
  int active_ = 0, pending_ = 0;
  bool stop_ = false;
  const pid_t pid_;
};

// fn(t) for t = 0 .. nth-1 on nth host threads (t = 0 on the caller's)
template <class F>
void run_threads(int nth, F &&fn) {
  if (nth <= 1) {
    fn(0);
    return;
  }
  const std::function<void(int)> f = [&fn](int t) { fn(t); };
  if (HostPool::get().try_run(nth, f)) return;
  std::vector<std::thread> th;
  for (int t = 1; t < nth; ++t) th.emplace_back(fn, t);
  fn(0);
  for (auto &t : th) t.join();
}

// Items per host thread of a setup pass. Process-wide; only a test program
// lowers it (tools/plan_check.cpp), to run small graphs on many threads.
constexpr int64_t kHostGrain = 131072;
inline int64_t g_host_grain = kHostGrain;

// Host threads for a setup pass over `work` items: one per 128k items (thread
// start-up costs more than small passes save; a local-BA window uses one).
inline int host_threads(int64_t work) {
  const int64_t want = std::max<int64_t>(1, work / g_host_grain);
  return (int)std::max<int64_t>(1, std::min<int64_t>({16, want, (int64_t)std::thread::hardware_concurrency()}));
}

// v <- src[0 .. n) on host threads (the caller's arrays are copied in: ABI)
template <class T, class A>
void par_assign(std::vector<T, A> &v, const T *src, size_t n) {
  v.resize(n);  // same size as the last call: no fill
  const int nth = host_threads((int64_t)n);
  run_threads(nth, [&](int t) {
    const size_t a = n * t / nth, b = n * (t + 1) / nth;
    if (b > a) {
      if (src) std::memcpy(v.data() + a, src + a, (b - a) * sizeof(T));
      else std::memset(static_cast<void *>(v.data() + a), 0, (b - a) * sizeof(T));
    }
  });
}

// v <- n copies of x on host threads
template <class T>
void fill_par(std::vector<T> &v, size_t n, T x) {
  v.resize(n);
  const int nth = host_threads((int64_t)n);
  run_threads(nth, [&](int t) { std::fill(v.begin() + n * t / nth, v.begin() + n * (t + 1) / nth, x); });
}

}  // namespace sqlm
