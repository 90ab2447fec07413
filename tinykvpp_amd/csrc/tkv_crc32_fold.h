// Shortening a lane's 64-byte segment with a sparse multiple of the CRC-32 polynomial, so that fewer
// of its bytes go through the slicing tables (docs/HISTORY.md §2). Plain C++ that the
// device compiler (crc_packed_body, tkv_crc32_device.h) and a host compiler
// (tests/cpp/test_fold_segment.cpp) both accept.
//
// A segment is 16 little-endian dwords = 512 stream bits: stream bit n is bit n % 32 of dword n / 32
// (dword 0 first in memory) and has polynomial degree 511 - n. crc_0(segment) is the segment
// polynomial mod P, so adding any multiple of P to the segment leaves it unchanged.
//
//   M(x) = x^300 + x^155 + x^117 + x^89 + 1
//
// is a multiple of P = 0x04C11DB7 (CRC-32/ISO-HDLC; the only one of weight <= 5 and degree <= 448).
// Adding x^(211 - n) M(x) clears stream bit n (degree 511 - n = 300 + 211 - n) and flips the bits of
// degree 366 - n, 328 - n, 300 - n and 211 - n: for n <= 211,
//
//   stream bit n  ==  stream bits n + 145, n + 183, n + 211, n + 300   (mod P).
//
// Every target lies behind its source, so folding from the front clears as far as the identity
// reaches. Two groups do it on whole dwords: dwords 0-1 fold into dwords 4-11, then the updated
// dwords 2-5 fold into dwords 6-15 (the last target bit is 191 + 300 = 491 < 512). Dwords 0-5 are
// then zero, leading zeros do not move an init-0 register, and crc_0(segment) = crc_0(dwords 6-15):
// 10 slicing steps instead of 16. The segment's end stays where it was, so what follows the slicing
// (lane shift, Horner step, init injection) is untouched.
//
// CRC-32C has no such multiple (its cheapest, of weight 6 and degree 209, folds 65 bits a pass), so
// the fold is for the 0xEDB88320 tables only.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define TKV_FOLD_HD __host__ __device__ __forceinline__
#define TKV_FOLD_UNROLL _Pragma("unroll")
#else
#define TKV_FOLD_HD inline
#define TKV_FOLD_UNROLL
#endif

namespace tkv {
namespace fold {

constexpr std::uint32_t kFoldPoly = 0xEDB88320u;  // reflected P: the only tables the fold is valid for
constexpr int kFoldTerms = 4;
constexpr int kFoldShift[kFoldTerms] = {145, 183, 211, 300};  // M's degree minus its other exponents
constexpr int kFoldLastBit = 511 - kFoldShift[kFoldTerms - 1];  // 211: last stream bit the identity moves
constexpr int kSegDwords = 16;
constexpr int kFoldedDwords = 6;                        // dwords 0-5 fold away
constexpr int kKeptDwords = kSegDwords - kFoldedDwords;  // dwords 6-15 go through the tables

// (hi << s) | (lo >> (32 - s)) for 0 < s < 32: one v_alignbit_b32.
TKV_FOLD_HD std::uint32_t funnel(std::uint32_t hi, std::uint32_t lo, int s) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(hi, lo, static_cast<std::uint32_t>(32 - s));
#else
  return (hi << s) | (lo >> (32 - s));
#endif
}
TKV_FOLD_HD std::uint32_t fold_xor3(std::uint32_t a, std::uint32_t b, std::uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);  // a ^ b ^ c
#else
  return a ^ b ^ c;
#endif
}

// XOR accumulator that pairs its terms into three-input XORs (`pending` is a compile-time fact once
// the loops around it are unrolled).
struct XorAcc {
  std::uint32_t v, p;
  bool pending;
  TKV_FOLD_HD void add(std::uint32_t t) {
    if (pending) v = fold_xor3(v, p, t);
    else p = t;
    pending = !pending;
  }
  TKV_FOLD_HD std::uint32_t value() const { return pending ? v ^ p : v; }
};

// Adds to `a` what the source dwords [S0, S0 + N) contribute to dword j: for each shift 32 ds + bs, the
// low bits of source j - ds moved up by bs and the high bits of source j - ds - 1 that spill over.
template <int S0, int N>
TKV_FOLD_HD void add_terms(XorAcc& a, const std::uint32_t (&d)[kSegDwords], int j) {
  static_assert(32 * (S0 + N) - 1 <= kFoldLastBit, "the identity holds for stream bits up to 211");
  static_assert(32 * (S0 + N) - 1 + kFoldShift[kFoldTerms - 1] < 32 * kSegDwords, "a term lands past dword 15");
  TKV_FOLD_UNROLL
  for (int s = 0; s < kFoldTerms; ++s) {
    const int ds = kFoldShift[s] / 32, bs = kFoldShift[s] % 32;
    const int k = j - ds;
    const bool hi = k >= S0 && k < S0 + N, lo = k - 1 >= S0 && k - 1 < S0 + N;
    if (hi && lo) a.add(funnel(d[k], d[k - 1], bs));
    else if (hi) a.add(d[k] << bs);
    else if (lo) a.add(d[k - 1] >> (32 - bs));
  }
}
static_assert(kFoldShift[0] % 32 != 0 && kFoldShift[1] % 32 != 0 && kFoldShift[2] % 32 != 0 && kFoldShift[3] % 32 != 0,
              "funnel() needs a bit shift of 1..31");

// The fold in two stages (a caller with several segments interleaves them stage by stage).
// Stage 0: dwords 0-1 into dwords 4-5, the only targets of theirs that are sources again.
constexpr int kGroup0 = 2, kGroup1 = kFoldedDwords - kGroup0;
static_assert(kFoldedDwords - kFoldShift[0] / 32 <= kGroup0, "dwords 2-5 take terms from dwords 0-1 only");
TKV_FOLD_HD void fold_stage0(std::uint32_t (&d)[kSegDwords]) {
  TKV_FOLD_UNROLL
  for (int j = kGroup0; j < kFoldedDwords; ++j) {
    XorAcc a{d[j], 0u, false};
    add_terms<0, kGroup0>(a, d, j);
    d[j] = a.value();
  }
}
// Stage 1: the rest of what dwords 0-1 contribute and all of what the updated dwords 2-5 do, into
// dwords 6-15 (one accumulator per target, so most XORs take three inputs); dwords 0-5 are cleared.
TKV_FOLD_HD void fold_stage1(std::uint32_t (&d)[kSegDwords]) {
  TKV_FOLD_UNROLL
  for (int j = kFoldedDwords; j < kSegDwords; ++j) {
    XorAcc a{d[j], 0u, false};
    add_terms<0, kGroup0>(a, d, j);
    add_terms<kGroup0, kGroup1>(a, d, j);
    d[j] = a.value();
  }
  TKV_FOLD_UNROLL
  for (int k = 0; k < kFoldedDwords; ++k) d[k] = 0u;
}

// The whole fold in place: afterwards d[0..5] = 0 and crc_0(d[6..15]) = crc_0 of the segment before.
TKV_FOLD_HD void fold_segment(std::uint32_t (&d)[kSegDwords]) {
  fold_stage0(d);
  fold_stage1(d);
}

}  // namespace fold
}  // namespace tkv
