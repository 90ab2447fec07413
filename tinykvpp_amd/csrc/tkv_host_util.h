// Host-thread helpers of the host format files (tkv_wal_host.cpp, tkv_sst_host.cpp, tkv_runs_host.cpp):
// the thread count, the one fork-join every helper goes through (parallel_tasks), the loops and the sort
// built on it, and the user-key order the memtable and the merge share. Plain C++, no device code.
#pragma once

#include <sched.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

namespace tkv {

inline bool ptr_ok(const void* p) { return p != nullptr; }

// Items from which a loop, a sort or a merge goes to host threads; serial below it.
constexpr std::uint64_t kHostParallelMin = std::uint64_t(1) << 14;

// Host threads for CPU-side work: the CPUs this process may run on, capped by OMP_NUM_THREADS (the
// GPU boxes' per-job CPU share) and 16.
inline unsigned host_threads() {
  unsigned n = 16;
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof(set), &set) == 0) n = std::min<unsigned>(n, static_cast<unsigned>(CPU_COUNT(&set)));
  if (const char* e = std::getenv("OMP_NUM_THREADS")) {
    const long v = std::strtol(e, nullptr, 10);
    if (v > 0) n = std::min<unsigned>(n, static_cast<unsigned>(v));
  }
  return std::max(1u, n);
}

// host_threads() for n items at or past the threshold, else 1.
inline unsigned threads_for(std::uint64_t n) { return n >= kHostParallelMin ? host_threads() : 1u; }

// fn(t) once for every task t in [0, count). threaded: on min(count, host_threads()) threads, the caller
// one of them, each taking the next task from a counter; else on the caller, in order. Returns when every
// task has.
template <class F>
void parallel_tasks(std::uint64_t count, bool threaded, F fn) {
  const unsigned nt = threaded ? static_cast<unsigned>(std::min<std::uint64_t>(count, host_threads())) : 1u;
  if (nt <= 1) {
    for (std::uint64_t t = 0; t < count; ++t) fn(t);
    return;
  }
  std::atomic<std::uint64_t> next{0};
  auto work = [&] {
    for (std::uint64_t t = next++; t < count; t = next++) fn(t);
  };
  std::vector<std::thread> th;
  for (unsigned t = 1; t < nt; ++t) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
}

// fn(i) for i in [0, n): in equal ranges on host threads when n is large (field writes scattered over a
// big image).
template <class F>
void parallel_for(std::uint64_t n, F fn) {
  const unsigned nt = threads_for(n);
  parallel_tasks(nt, nt > 1, [=](std::uint64_t t) {
    const std::uint64_t hi = n * (t + 1) / nt;  // (a local: fn's stores could alias a captured bound)
    for (std::uint64_t i = n * t / nt; i < hi; ++i) fn(i);
  });
}

// fn(t, lo, hi) for the ranges [lo, hi) of [0, n) on host threads: one task per range of at least 32
// items (blocks to parse, entries to copy), so the threshold is 64 items; t < host_threads().
template <class F>
void parallel_ranges(std::uint64_t n, F fn) {
  const unsigned nt = n >= 64 ? static_cast<unsigned>(std::min<std::uint64_t>(host_threads(), n / 32)) : 1u;
  parallel_tasks(nt, nt > 1, [&](std::uint64_t t) { fn(static_cast<unsigned>(t), n * t / nt, n * (t + 1) / nt); });
}

// idx sorted by less, equal elements left in their order: chunks on host threads, then pairwise merges,
// every width behind the one before it.
template <class Less>
void parallel_stable_sort(std::vector<std::uint32_t>& idx, Less less) {
  const std::uint64_t n = idx.size();
  const unsigned nt = threads_for(n);
  if (nt == 1) {
    std::stable_sort(idx.begin(), idx.end(), less);
    return;
  }
  std::vector<std::uint64_t> cut(nt + 1);
  for (unsigned t = 0; t <= nt; ++t) cut[t] = n * t / nt;
  parallel_tasks(nt, true, [&](std::uint64_t t) { std::stable_sort(idx.begin() + cut[t], idx.begin() + cut[t + 1], less); });
  for (unsigned w = 1; w < nt; w *= 2)
    parallel_tasks((nt - w + 2 * w - 1) / (2 * w), true, [&](std::uint64_t k) {
      const unsigned t = static_cast<unsigned>(k) * 2 * w;
      std::inplace_merge(idx.begin() + cut[t], idx.begin() + cut[t + w], idx.begin() + cut[std::min(t + 2 * w, nt)], less);
    });
}

// simd_comparator's order on user keys: unsigned bytes, a prefix first. Negative, 0 or positive.
inline int user_key_cmp(const std::uint8_t* a, std::uint32_t la, const std::uint8_t* b, std::uint32_t lb) {
  const std::uint32_t m = std::min(la, lb);
  const int r = m ? std::memcmp(a, b, m) : 0;
  return r ? r : (la < lb ? -1 : la > lb ? 1 : 0);
}

}  // namespace tkv
