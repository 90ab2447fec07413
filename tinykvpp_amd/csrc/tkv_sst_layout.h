// The SSTable file image tkv_sst_build[_device] writes (include/tkv_crc32.h "SSTable flush"): the
// arithmetic of sstable_writer::append / get_data_block / get_index / get_footer shared by the host
// path (tkv_formats.cpp) and the device kernels (tkv_sst_build.hip). Plain C++.
#pragma once

#include <cstdint>

#include "tkv_crc32_internal.h"

namespace tkv {

constexpr std::uint32_t kSstHeader = 21;      // varint(20) | the 20-byte data-block header
constexpr std::uint32_t kSstOverhead = 36;    // image bytes beyond the counted size: 8 + 20 + 8
constexpr std::uint32_t kSstEntryCount = 8;   // what append counts per entry beyond key and value (4 per length)
constexpr std::uint32_t kSstMaxLen = 1u << 28;  // a length's varint must fit the 4 bytes counted for it
constexpr std::uint32_t kSstIndexFixed = 16;  // u64 offset | u64 size behind an index entry's key
constexpr std::uint32_t kSstFooter = 20;
constexpr std::uint32_t kSstFooterCrc = 16;
constexpr std::uint32_t kSstCrc = 17;         // TKV_SST_CRC_OFFSET

// Bytes of LEB128(v) (codec::encode_varint).
TKV_HD inline std::uint32_t sst_vlen(std::uint64_t v) {
  std::uint32_t k = 1;
  while (v >= 0x80u) {
    v >>= 7;
    ++k;
  }
  return k;
}

// LEB128(v) to out (at most 10 bytes); returns the count.
TKV_HD inline std::uint32_t sst_put_varint(std::uint8_t* out, std::uint64_t v) {
  std::uint32_t k = 0;
  while (v >= 0x80u) {
    out[k++] = static_cast<std::uint8_t>(v) | 0x80u;
    v >>= 7;
  }
  out[k++] = static_cast<std::uint8_t>(v);
  return k;
}

// What append counts for an entry (sstable_writer.cpp:61,122) and what write_string twice writes.
TKV_HD inline std::uint64_t sst_counted(std::uint32_t kl, std::uint32_t vl) { return std::uint64_t(kSstEntryCount) + kl + vl; }
TKV_HD inline std::uint64_t sst_written(std::uint32_t kl, std::uint32_t vl) {
  return std::uint64_t(sst_vlen(kl)) + kl + sst_vlen(vl) + vl;
}

// The first kSstHeader + vlen(z) bytes of a data-block image with c entries and counted size z (z fits
// u32), CRC field zero; returns their count (at most 26).
TKV_HD inline std::uint32_t sst_block_head(std::uint8_t* out, std::uint32_t c, std::uint32_t z) {
  out[0] = 20;
  for (int b = 0; b < 4; ++b) {
    out[1 + b] = static_cast<std::uint8_t>(c >> (8 * b));
    out[5 + b] = static_cast<std::uint8_t>(z >> (8 * b));
    out[9 + b] = static_cast<std::uint8_t>(z >> (8 * b));
    out[13 + b] = 0;  // compression, three pad bytes
    out[17 + b] = 0;  // crc32_
  }
  return kSstHeader + sst_put_varint(out + kSstHeader, z);
}

// Doubling rounds that mark every member of a chain of at most bmax blocks:
// ceil(log2(bmax + 1)).
inline std::uint32_t sst_rounds(std::uint64_t bmax) {
  std::uint32_t r = 0;
  while ((std::uint64_t(1) << r) < bmax + 1u) ++r;
  return r;
}

}  // namespace tkv
