// The SSTable file image tkv_sst_build[_device] writes (include/tkv_crc32.h "SSTable flush"): the
// arithmetic of sstable_writer::append / get_data_block / get_index / get_footer shared by the host
// path (tkv_sst_host.cpp) and the device kernels (tkv_sst_build.hip), and the checks of the reader
// tkv_sst_scan[_device] ("SSTable scan"; tkv_sst_host.cpp, tkv_sst_scan.hip). Plain C++.
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

// ---- the reader's arithmetic (include/tkv_crc32.h "SSTable scan") -------------------
// Shared by the host scan (tkv_sst_host.cpp) and the device kernels (tkv_sst_scan.hip). Nothing here
// touches memory: a caller packs the (at most 5) bytes it may read into a word, bounded by what is left
// of the region, and gets positions back; every sum is 64-bit.

constexpr std::uint32_t kSstMinFile = 28;     // an index of 8 bytes and the footer
constexpr std::uint32_t kSstMinIndexEntry = 17;  // varint(0) | u64 | u64
constexpr std::uint32_t kSstMinBlock = 22;    // TKV_SST_MIN_IMAGE
constexpr std::uint32_t kSstLenBytes = 4;     // a length's varint: what append counts for it
constexpr std::uint32_t kSstBodyLenBytes = 5; // the body's length prefix: z fits u32

// A LEB128 value whose first bytes are the little-endian bytes of w, of which avail are real: n = its
// byte count, 0 when it does not end within min(avail, maxb) bytes (maxb <= 5). Redundant encodings
// (80 00) are taken at their value.
struct SstVarint {
  std::uint64_t v;
  std::uint32_t n;
};
TKV_HD inline SstVarint sst_varint_word(std::uint64_t w, std::uint64_t avail, std::uint32_t maxb) {
  SstVarint r{0u, 0u};
  const std::uint32_t lim = avail < maxb ? static_cast<std::uint32_t>(avail) : maxb;
  for (std::uint32_t k = 0; k < lim; ++k) {
    const std::uint64_t b = (w >> (8u * k)) & 0xFFu;
    r.v |= (b & 0x7Fu) << (7u * k);
    if (b < 0x80u) {
      r.n = k + 1u;
      return r;
    }
  }
  r.v = 0;
  return r;
}

// The footer's fields against the file: 28 <= file_size <= 2^32 - 1, index_offset + index_size + 20 ==
// file_size, index_size >= 8 (sst.read_index's rules).
TKV_HD inline bool sst_footer_ok(std::uint64_t file_size, std::uint32_t index_offset, std::uint32_t index_size) {
  return file_size >= kSstMinFile && file_size <= 0xFFFFFFFFull && index_size >= 8u &&
         std::uint64_t(index_offset) + index_size + kSstFooter == file_size;
}
TKV_HD inline bool sst_index_count_ok(std::uint64_t B, std::uint64_t index_size) {
  return B <= (index_size - 8u) / kSstMinIndexEntry;
}

// One step of a chain of length-prefixed strings in a region of `end` bytes: the string at position p
// (p < end) is varint(len) | len bytes | `fixed` more bytes, w holds the bytes at p (min(4, end - p) of
// them real). ok: the varint ends within 4 bytes and the whole entry lies inside the region; then n is
// the varint's byte count, len the length and next = p + n + len + fixed <= end.
struct SstLink {
  std::uint64_t next;
  std::uint32_t len, n;
  bool ok;
};
// sst_varint_word(w, avail, 4) without a loop or a branch: the walk of a block takes this step once per
// string, all of it on the scalar unit of a wave whose lanes move together.
TKV_HD inline SstVarint sst_varint4(std::uint32_t w, std::uint64_t avail) {
  const std::uint32_t c0 = w & 0x80u, c1 = w & 0x8000u, c2 = w & 0x800000u, c3 = w & 0x80000000u;
  const std::uint32_t n = !c0 ? 1u : !c1 ? 2u : !c2 ? 3u : !c3 ? 4u : 0u;
  const std::uint32_t v = (w & 0x7Fu) | ((w >> 1) & 0x3F80u) | ((w >> 2) & 0x1FC000u) | ((w >> 3) & 0xFE00000u);
  const bool ok = n != 0u && n <= avail;
  const std::uint32_t bits = 7u * (ok ? n : 1u);
  return SstVarint{ok ? v & (0xFFFFFFFFu >> (32u - bits)) : 0u, ok ? n : 0u};
}

TKV_HD inline SstLink sst_chain_next(std::uint32_t w, std::uint64_t p, std::uint64_t end, std::uint32_t fixed) {
  const SstVarint v = sst_varint4(w, end - p);
  SstLink s{0u, static_cast<std::uint32_t>(v.v), v.n, false};
  if (!v.n) return s;
  s.next = p + v.n + v.v + fixed;
  s.ok = s.next <= end;
  return s;
}

// An index entry's block against the data region [0, index_offset).
TKV_HD inline bool sst_index_block_ok(std::uint64_t off, std::uint64_t size, std::uint64_t index_offset) {
  return size >= kSstMinBlock && off <= index_offset && size <= index_offset - off;
}

// The fixed part of a data-block image of `size` bytes (size >= 22): byte 0, u32 c at 1, u32 z at 5, the
// u32 at 9, byte 13, and the body's length prefix zv (the varint at byte 21, read with size - 21 bytes
// available and at most 5). True: the body is the z bytes at 21 + zv.n and a walk of c entries is bounded.
TKV_HD inline bool sst_block_header_ok(std::uint32_t b0, std::uint32_t c, std::uint32_t z, std::uint32_t z2, std::uint32_t comp,
                                       std::uint64_t size, SstVarint zv) {
  return b0 == 20u && z2 == z && comp == 0u && std::uint64_t(kSstOverhead) + z == size && c >= 1u &&
         8ull * c <= z && zv.n != 0u && zv.v == z;
}

}  // namespace tkv
