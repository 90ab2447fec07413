// The key read shared by the memtable replay (tkv_memtable.hip) and the SSTable merge
// (tkv_sst_merge.hip): eight key bytes as the comparison word of tkv_memtable_layout.h, from aligned
// dwords at any source alignment.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "tkv_memtable_layout.h"
#include "tkv_wal_copy.h"

namespace tkv {
namespace {

// Key bytes [addr, addr + min(rem, 8)) big-endian, zero-padded: aligned dwords that hold a byte of them,
// shifted together (v_alignbyte); bytes of those dwords outside the span are masked away.
__device__ __forceinline__ std::uint64_t load_word(std::uintptr_t addr, std::uint64_t rem) {
  const std::uint32_t take = rem < kMtWordBytes ? static_cast<std::uint32_t>(rem) : kMtWordBytes;
  if (take == 0) return 0;
  const std::uintptr_t e = addr + take, a0 = addr & ~static_cast<std::uintptr_t>(3);
  const std::uint32_t sh = static_cast<std::uint32_t>(addr & 3u);
  const std::uint32_t w0 = ld4(a0, addr, e), w1 = ld4(a0 + 4u, addr, e), w2 = ld4(a0 + 8u, addr, e);
  const std::uint32_t lo = __builtin_amdgcn_alignbyte(w1, w0, sh), hi = __builtin_amdgcn_alignbyte(w2, w1, sh);
  std::uint64_t v = (static_cast<std::uint64_t>(hi) << 32) | lo;
  if (take < 8u) v &= (1ull << (8u * take)) - 1ull;
  return __builtin_bswap64(v);
}

}  // namespace
}  // namespace tkv
