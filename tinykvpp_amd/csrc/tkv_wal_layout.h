// The WAL record wal_entry::encode writes (wal.cpp:19-61), little-endian and packed:
//   u32 record_len | u32 crc32 | u8 op | u64 seq | u8 tombstone | u32 key_len | u32 val_len | key | value
// record_len counts the bytes behind the 8-byte prefix, and crc32 covers exactly those. Plain C++:
// shared by the host walk (tkv_wal_host.cpp) and the device kernels (tkv_wal_*.hip).
#pragma once

#include <cstdint>

namespace tkv {

// Byte offsets of the fields from the record's start.
constexpr std::uint32_t kWalCrc = 4;      // stored CRC-32 of the payload
constexpr std::uint32_t kWalPayload = 8;  // first byte record_len counts and the CRC covers
constexpr std::uint32_t kWalOp = 8;
constexpr std::uint32_t kWalSeq = 9;
constexpr std::uint32_t kWalTomb = 17;
constexpr std::uint32_t kWalKeyLen = 18;
constexpr std::uint32_t kWalValLen = 22;
// wal.hpp:21-27 kMetadataSize: the prefix and the fixed fields, i.e. the offset of the key (u64, so
// sums with record lengths do not wrap).
constexpr std::uint64_t kWalMeta = 26;

}  // namespace tkv
