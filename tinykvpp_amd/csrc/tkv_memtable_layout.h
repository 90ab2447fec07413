// What the host path (tkv_runs_host.cpp) and the device kernels (tkv_memtable.hip) of the memtable replay
// share (include/tkv_crc32.h "Memtable replay"): the metadata encode_internal_key puts behind a user key
// (sstable_format.cpp:9-25), the comparison word of the sort and the limits.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define TKV_MT_HD __host__ __device__ inline
#else
#define TKV_MT_HD inline
#endif

namespace tkv {

// user_key | u64 seq LE | u64 timestamp LE | u8 tombstone
constexpr std::uint32_t kMtMeta = 17;
constexpr std::uint32_t kMtSeq = 0;    // offsets behind the user key
constexpr std::uint32_t kMtTime = 8;
constexpr std::uint32_t kMtTomb = 16;
// key_len + kMtMeta must stay below this: the flush refuses an internal key of 2^28 bytes or more.
constexpr std::uint32_t kMtMaxIkey = 1u << 28;
constexpr std::uint32_t kMtOpPut = 0, kMtOpDel = 1;

// The comparison word of round r covers key bytes [8 r, 8 r + 8): the bytes big-endian, zero-padded, and
// behind them the digit min(remaining, 9), remaining = key_len - 8 r. Among words with equal bytes the
// digit orders the shorter key first (a < a\0: digits 1 < 2 where padding alone cannot tell), digits
// 0..8 mean the key ends in this word (equal words, equal keys) and 9 that it goes on.
constexpr std::uint32_t kMtWordBytes = 8;
constexpr std::uint32_t kMtDigitBits = 4;
constexpr std::uint32_t kMtDigitMore = 9;
TKV_MT_HD std::uint32_t mt_digit(std::uint64_t remaining) {
  return remaining < kMtDigitMore ? static_cast<std::uint32_t>(remaining) : kMtDigitMore;
}
// Rounds of refinement a key of max_len bytes can need at most: one per word, and one more for a key
// that ends exactly on a word boundary beside a longer one.
TKV_MT_HD std::uint64_t mt_max_rounds(std::uint64_t max_len) { return (max_len + kMtWordBytes - 1) / kMtWordBytes + 1; }

// The 17 metadata bytes of one internal key.
TKV_MT_HD void mt_put_meta(std::uint8_t* d, std::uint64_t seq, std::uint64_t timestamp_ms, std::uint8_t tomb) {
  for (std::uint32_t b = 0; b < 8; ++b) {
    d[kMtSeq + b] = static_cast<std::uint8_t>(seq >> (8 * b));
    d[kMtTime + b] = static_cast<std::uint8_t>(timestamp_ms >> (8 * b));
  }
  d[kMtTomb] = tomb != 0 ? 1 : 0;
}

}  // namespace tkv
