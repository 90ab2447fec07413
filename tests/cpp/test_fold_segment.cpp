// Host check of the segment fold (tinykvpp_amd/csrc/tkv_crc32_fold.h, the function crc_packed_body
// runs on the device): for a 64-byte segment, crc_0 of the 40 bytes left in dwords 6-15 equals crc_0
// of the 64 bytes, dwords 0-5 end up zero and no term lands past dword 15. crc_0 is the CRC-32
// register from 0 without the final XOR, computed with frankie::core's table and, independently, bit
// by bit from kCRC32Polynomial. A bit-level model of the identity (stream bit n == bits n + 145,
// n + 183, n + 211, n + 300) must give the same 16 dwords as the dword fold.
//
// Cases: each of the 512 single-bit segments, all-ones, all-zero, 10 000 seeded random segments.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "frankie_crc32.hpp"
#include "tkv_crc32_fold.h"

namespace {

using tkv::fold::kFoldedDwords;
using tkv::fold::kSegDwords;

constexpr auto kTable = frankie::core::generate_crc32_table();

// Register from 0 over n little-endian dwords, no final XOR (Sarwate, frankie's table).
std::uint32_t crc0_table(const std::uint32_t* d, int n) {
  std::uint32_t r = 0;
  for (int i = 0; i < n; ++i)
    for (int b = 0; b < 4; ++b) r = kTable[(r ^ (d[i] >> (8 * b))) & 0xFFu] ^ (r >> 8);
  return r;
}

// The same, one stream bit at a time.
std::uint32_t crc0_bitwise(const std::uint32_t* d, int n) {
  std::uint32_t r = 0;
  for (int i = 0; i < 32 * n; ++i) {
    const std::uint32_t bit = (d[i / 32] >> (i % 32)) & 1u;
    r = ((r ^ bit) & 1u) ? (r >> 1) ^ frankie::core::kCRC32Polynomial : r >> 1;
  }
  return r;
}

// Bit-level model: clears stream bits 0..191 front to back, flipping the four bits each one equals.
// Returns false if a flip would land past bit 511.
bool fold_bits(std::uint32_t (&d)[kSegDwords]) {
  for (int n = 0; n < 32 * kFoldedDwords; ++n) {
    if (!((d[n / 32] >> (n % 32)) & 1u)) continue;
    d[n / 32] ^= 1u << (n % 32);
    for (int s = 0; s < tkv::fold::kFoldTerms; ++s) {
      const int m = n + tkv::fold::kFoldShift[s];
      if (m >= 32 * kSegDwords) return false;
      d[m / 32] ^= 1u << (m % 32);
    }
  }
  return true;
}

int failures = 0;

void check(const std::uint32_t (&seg)[kSegDwords], const char* what, long idx) {
  std::uint32_t f[kSegDwords], m[kSegDwords];
  std::memcpy(f, seg, sizeof f);
  std::memcpy(m, seg, sizeof m);
  tkv::fold::fold_segment(f);
  const bool in_range = fold_bits(m);
  const std::uint32_t want = crc0_table(seg, kSegDwords);
  bool ok = in_range && want == crc0_bitwise(seg, kSegDwords);
  ok = ok && crc0_table(f + kFoldedDwords, tkv::fold::kKeptDwords) == want;  // the 40 bytes the kernel slices
  ok = ok && crc0_bitwise(f, kSegDwords) == want;                            // the whole folded segment
  for (int k = 0; k < kFoldedDwords; ++k) ok = ok && f[k] == 0u;
  ok = ok && std::memcmp(f, m, sizeof f) == 0;
  if (!ok && failures++ < 10) std::printf("FAIL %s %ld\n", what, idx);
}

}  // namespace

int main() {
  static_assert(frankie::core::kCRC32Polynomial == tkv::fold::kFoldPoly, "the fold is for frankie's polynomial");
  std::uint32_t seg[kSegDwords];
  for (int n = 0; n < 32 * kSegDwords; ++n) {
    std::memset(seg, 0, sizeof seg);
    seg[n / 32] = 1u << (n % 32);
    check(seg, "bit", n);
  }
  std::memset(seg, 0xFF, sizeof seg);
  check(seg, "ones", 0);
  std::memset(seg, 0, sizeof seg);
  check(seg, "zeros", 0);
  std::mt19937 rng(20240607u);
  for (long i = 0; i < 10000; ++i) {
    for (auto& w : seg) w = static_cast<std::uint32_t>(rng());
    check(seg, "random", i);
  }
  if (failures) {
    std::printf("%d FAILED\n", failures);
    return 1;
  }
  std::printf("ALL PASSED\n");
  return 0;
}
