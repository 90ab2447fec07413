// The u64 exclusive scan and the pointer doubling shared by the format device code (WAL encode and
// decode, SSTable flush and scan, memtable replay): the levels of a scan over n entries (kScanBlock
// entries per workgroup, the block sums scanned by the next level) with their host-side plan and the
// launches of the levels above the first, and the doubling rounds that mark a chain of jumps.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "tkv_crc32_device.h"
#include "tkv_device_util.h"

namespace tkv {
namespace {

constexpr unsigned kScanThreads = 256;
constexpr unsigned kScanItems = 4;            // consecutive entries per thread
constexpr std::uint64_t kScanBlock = kScanThreads * kScanItems;  // entries per workgroup of a scan level
constexpr int kScanLevels = 4;                // kScanBlock^4 >= 2^32 entries

// ---- scan levels ------------------------------------------------------------------------------------

// The thread's kScanItems consecutive entries v (entry i0 + k; zero past m) of one workgroup of a scan
// level: their exclusive prefix within the block to arr[i0 + k], the block's sum to bsum[block].
__device__ __forceinline__ void scan_items(const std::uint64_t (&v)[kScanItems], std::uint64_t i0, std::uint64_t m,
                                           std::uint64_t* arr, std::uint64_t* bsum) {
  std::uint64_t s = 0;
#pragma unroll
  for (unsigned k = 0; k < kScanItems; ++k) s += v[k];
  std::uint64_t total;
  std::uint64_t run = dev::block_prefix<std::uint64_t, kScanThreads>(s, &total);
#pragma unroll
  for (unsigned k = 0; k < kScanItems; ++k) {
    const std::uint64_t i = i0 + k;
    if (i < m) arr[i] = run;
    run += v[k];
  }
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// A level above the first: arr[0, m) (the block sums of the level below) in place.
__global__ __launch_bounds__(kScanThreads) void scan_level(std::uint64_t* arr, std::uint64_t m, std::uint64_t* bsum) {
  const std::uint64_t i0 = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
  std::uint64_t v[kScanItems];
#pragma unroll
  for (unsigned k = 0; k < kScanItems; ++k) v[k] = i0 + k < m ? arr[i0 + k] : 0u;
  scan_items(v, i0, m, arr, bsum);
}

__global__ __launch_bounds__(kScanThreads) void scan_add(std::uint64_t* arr, std::uint64_t m, const std::uint64_t* base) {
  const std::uint64_t i = blockIdx.x * static_cast<std::uint64_t>(kScanThreads) + threadIdx.x;
  if (i < m) arr[i] += base[i / kScanBlock];
}

// Entries of the scan levels over n: level k + 1 holds the block sums of level k, the last one a single
// sum. nsum = the entries of the levels above the first.
struct ScanPlan {
  std::uint64_t m[kScanLevels + 1];
  int levels = 0;
  std::uint64_t nsum = 0;
  explicit ScanPlan(std::uint64_t n) {
    m[0] = n;
    while (m[levels] > 1u || levels == 0) {
      m[levels + 1] = (m[levels] + kScanBlock - 1u) / kScanBlock;
      ++levels;
    }
    for (int k = 1; k <= levels; ++k) nsum += m[k];
  }
  // lv[0] = the entries, lv[k] for k >= 1 laid one after the other in sums (nsum entries).
  void place(std::uint64_t* entries, std::uint64_t* sums, std::uint64_t* (&lv)[kScanLevels + 1]) const {
    lv[0] = entries;
    lv[1] = sums;
    for (int k = 2; k <= levels; ++k) lv[k] = lv[k - 1] + m[k - 1];
  }
};

// The levels above the first of a scan whose level 0 has been launched, up to the single total.
inline void scan_up(const ScanPlan& plan, std::uint64_t* const* lv, hipStream_t st) {
  for (int k = 1; k < plan.levels; ++k)
    hipLaunchKernelGGL(scan_level, dim3(static_cast<unsigned>(plan.m[k + 1])), dim3(kScanThreads), 0, st, lv[k], plan.m[k],
                       lv[k + 1]);
}
// The block bases back down to level `lowest`: 0 the entries, 1 for a caller whose own finish kernel adds
// lv[1] to them.
inline void scan_down(const ScanPlan& plan, std::uint64_t* const* lv, hipStream_t st, int lowest = 0) {
  for (int k = plan.levels - 2; k >= lowest; --k)
    hipLaunchKernelGGL(scan_add, dim3(blocks(plan.m[k], kScanThreads)), dim3(kScanThreads), 0, st, lv[k], plan.m[k], lv[k + 1]);
}

// ---- pointer doubling -------------------------------------------------------------------------------

// One doubling round over [0, m): marked positions mark their jump target (< m), the jump composed with
// itself goes to the other buffer (in place it would skip members). (A template, so that only the files
// that run it hold a copy.)
template <class I>
__global__ __launch_bounds__(kScanThreads) void chain_round(const I* in, I* out, I* mark, std::uint64_t m) {
  const std::uint64_t s = blockIdx.x * static_cast<std::uint64_t>(kScanThreads) + threadIdx.x;
  if (s >= m) return;
  const I j = in[s];
  if (mark[s]) mark[j] = 1u;
  out[s] = in[j];
}

// The chain s, J(s), J(J(s)), ... of the position s the caller marked, marked over [0, m) (J maps [0, m)
// into itself and the chain ends in a fixed point): in round k every marked s marks
// J_k[s] and J_{k+1} = J_k o J_k goes to the other of Ja / Jb, so after round k every chain member at
// distance < 2^(k+1) is marked; a mark written and read within one round only adds true members.
template <class I>
void chain_double(const I* J, I* Ja, I* Jb, I* mark, std::uint64_t m, std::uint32_t rounds, hipStream_t st) {
  const I* in = J;
  I* out = Ja;
  for (std::uint32_t r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(chain_round<I>, dim3(blocks(m, kScanThreads)), dim3(kScanThreads), 0, st, in, out, mark, m);
    in = out;
    out = out == Ja ? Jb : Ja;
  }
}

}  // namespace
}  // namespace tkv
