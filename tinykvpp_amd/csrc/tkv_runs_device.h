// What the device code over sorted runs of internal keys shares: the SSTable merge (tkv_sst_merge.hip)
// and the SSTable get (tkv_sst_get.hip). The run table entry the kernels read, the span check every entry
// passes before its key is read, the user key of a checked entry, the comparator over the comparison word
// of tkv_memtable_layout.h ((word, digit), the rest of two keys only on a tie with digit 9), and the pinned
// staging block the host copies its tables to the device from.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "tkv_crc32.h"
#include "tkv_engine.h"
#include "tkv_key_word.h"
#include "tkv_memtable_layout.h"

namespace tkv {
namespace {

constexpr unsigned kMgDigitShift = 40, kMgRunShift = 32;       // the sort entry's second word
constexpr std::uint64_t kMgIdxMask = 0xFFFFFFFFull;
static_assert(TKV_SST_MERGE_MAX_RUNS <= 256, "the run takes 8 bits of the sort entry");

// One run as the kernels see it.
struct MgRun {
  const std::uint8_t* keys;
  std::uint64_t keys_size;
  const std::uint64_t* key_off;
  const std::uint32_t* key_len;
  const std::uint64_t* val_off;  // nullable
  const std::uint32_t* val_len;  // nullable
  std::uint64_t start;           // entries of the runs before it
  std::uint64_t key_bias;        // keys - key_base
  std::uint64_t val_bias;
};

struct MgKey {
  std::uintptr_t addr;
  std::uint32_t ulen;
};

__device__ __forceinline__ const MgRun& run_of(const MgRun* runs, std::uint64_t x) { return runs[(x >> kMgRunShift) & 0xFFu]; }

// The user key of a checked entry.
__device__ __forceinline__ MgKey key_of(const MgRun* runs, std::uint64_t x) {
  const MgRun& r = run_of(runs, x);
  const std::uint64_t i = x & kMgIdxMask;
  return MgKey{reinterpret_cast<std::uintptr_t>(r.keys) + r.key_off[i], r.key_len[i] - kMtMeta};
}

// Two keys equal in their first 8 bytes and both longer: their order by the words behind.
__device__ inline int cmp_rest(MgKey a, MgKey b) {
  for (std::uint32_t o = kMtWordBytes;; o += kMtWordBytes) {
    const std::uint64_t ra = a.ulen - o, rb = b.ulen - o;  // >= 1: the digit in front said the key goes on
    const std::uint64_t wa = load_word(a.addr + o, ra), wb = load_word(b.addr + o, rb);
    if (wa != wb) return wa < wb ? -1 : 1;
    const std::uint32_t da = mt_digit(ra), db = mt_digit(rb);
    if (da != db) return da < db ? -1 : 1;
    if (da < kMtDigitMore) return 0;
  }
}

// The one comparator of the merge's check, partition search, tile merge and ties.
__device__ __forceinline__ int mg_cmp(const MgRun* runs, std::uint64_t wa, std::uint64_t xa, std::uint64_t wb, std::uint64_t xb) {
  if (wa != wb) return wa < wb ? -1 : 1;
  const std::uint32_t da = static_cast<std::uint32_t>(xa >> kMgDigitShift), db = static_cast<std::uint32_t>(xb >> kMgDigitShift);
  if (da != db) return da < db ? -1 : 1;
  if (da < kMtDigitMore) return 0;
  return cmp_rest(key_of(runs, xa), key_of(runs, xb));
}

__device__ __forceinline__ bool span_ok(const MgRun& r, std::uint64_t ko, std::uint32_t kl) {
  return kl >= kMtMeta && kl < kMtMaxIkey && ko <= r.keys_size && kl <= r.keys_size - ko;
}

// Pinned staging of a call's host-built tables (the run table, a tile map): grown by doubling, kept with
// the scratch that owns it; the copies to the device are asynchronous.
struct RunStage {
  void* h = nullptr;
  std::uint64_t cap = 0;
  RunStage() = default;
  RunStage(const RunStage&) = delete;
  RunStage& operator=(const RunStage&) = delete;
  ~RunStage() { (void)hipHostFree(h); }
  int stage(std::uint64_t bytes, const char* msg) {
    if (bytes <= cap) return TKV_OK;
    const std::uint64_t c = std::max<std::uint64_t>(bytes, 2 * cap);
    (void)hipHostFree(h);
    h = nullptr;
    cap = 0;
    if (hipHostMalloc(&h, c, hipHostMallocDefault) != hipSuccess) {
      h = nullptr;
      return set_error(TKV_OUT_OF_MEMORY, msg);
    }
    cap = c;
    return TKV_OK;
  }
};

}  // namespace
}  // namespace tkv
