// Folds from a wave's LDS window, shared by the WAL verify sweep (tkv_wal_device.hip) and the WAL
// group-commit encoder (tkv_wal_encode.hip): one record per lane (fold_raw), ranges cut into chunks
// over the lanes (fold_ranges), and the GF(2) shifts that combine partial registers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "tkv_crc32_device.h"
#include "tkv_crc32_internal.h"

namespace tkv {
namespace {

constexpr std::uint32_t kLaneFold = 240;        // payloads up to this long are folded by one lane from LDS
constexpr std::uint32_t kChunk = 112;     // bytes per lane of a range fold
// kinds of fold range: the bytes in front of the region's entry (part of the record the chain is in
// when it enters; crc0), a payload wholly inside the region (initial register injected, checked here),
// the head of a payload that goes on past the region (initial register injected; finished by wal_fin_*)
constexpr std::uint32_t kRangeCarry = 0, kRangeWhole = 1, kRangeHead = 2;

// Little-endian u32 at byte b of the window (dword-aligned reads, v_alignbyte).
__device__ __forceinline__ std::uint32_t rd32(const std::uint8_t* win, std::uint32_t b) {
  const std::uint32_t q = b & ~3u;
  const std::uint32_t lo = *reinterpret_cast<const std::uint32_t*>(win + q);
  const std::uint32_t hi = *reinterpret_cast<const std::uint32_t*>(win + q + 4);
  return __builtin_amdgcn_alignbyte(hi, lo, b & 3u);
}

__device__ __forceinline__ std::uint32_t shfl_pos(std::uint32_t v, std::uint32_t src) {
  return static_cast<std::uint32_t>(__shfl(static_cast<int>(v), static_cast<int>(src), 64));
}
__device__ __forceinline__ std::uint64_t shfl_pos(std::uint64_t v, std::uint32_t src) {
  const std::uint32_t lo = shfl_pos(static_cast<std::uint32_t>(v), src);
  const std::uint32_t hi = shfl_pos(static_cast<std::uint32_t>(v >> 32), src);
  return (static_cast<std::uint64_t>(hi) << 32) | lo;
}

using dev::lane_prefix;  // exclusive prefix sum over the 64 lanes (DPP scan) and its total

// CRC-32 (finalized) of the L <= kLaneFold window bytes at s, one record per lane. The record is read
// from s - z, z = 4 nd - L (nd = its dwords), so that it ends on a dword; the z bytes in front are
// zeroed in its first dword (leading zeros leave a zero register at 0). Every lane steps through the
// round's largest dword count, its register frozen after its own nd (selects, no branch: the LDS
// waits stay countable; exec-masked steps measured slower). Dword i is v_alignbyte of two
// dword-aligned window reads. The initial register enters as inj[L] = Shift_L(0xFFFFFFFF)
// (crc_s(D) = Shift_|D|(s) ^ crc_0(D)); slicing-by-4 into the 64 KiB table image (crc32.cpp:9-16
// restated). (Two or three records per lane at once, as independent chains, measured slower.)
// fold_raw is that fold from a zero register (crc0 of the bytes); callers add inj[L] ^ 0xFFFFFFFF.
__device__ __forceinline__ std::uint32_t fold_raw(const std::uint8_t* win, const std::uint32_t* tab, const dev::LaneConstX& kc,
                                                  std::uint32_t s, std::uint32_t L) {
  const std::uint32_t nd = (L + 3u) >> 2;
  const std::uint32_t nmax = dev::wave_max(nd);
  const std::uint32_t z = 4u * nd - L;
  const std::uint32_t b0 = s - z;  // (s >= 8: b0 >= 5)
  const std::uint32_t sh = b0 & 3u;
  const std::uint32_t* w = reinterpret_cast<const std::uint32_t*>(win + (b0 & ~3u));
  std::uint32_t lo = w[1];
  dev::Reg r{0u, 0u};
  dev::slice4(tab, r, __builtin_amdgcn_alignbyte(lo, w[0], sh) & (~0u << (8u * z)), kc);
  if (nd == 0u) r = dev::Reg{0u, 0u};
#pragma unroll 2
  for (std::uint32_t i = 1; i < nmax; ++i) {
    const std::uint32_t hi = w[i + 1u];
    dev::Reg t = r;
    dev::slice4(tab, t, __builtin_amdgcn_alignbyte(hi, lo, sh), kc);
    if (i < nd) r = t;
    lo = hi;
  }
  return r.value();
}

// a*b mod P (reflected, x^0 = bit 31) in few registers: the loop is kept rolled (fully unrolled, the
// shift chain of b is computed ahead and held, which spills the sweep).
__device__ __forceinline__ std::uint32_t mul_lean(std::uint32_t a, std::uint32_t b, std::uint32_t poly) {
  std::uint32_t p = 0;
#pragma unroll 4
  for (int i = 0; i < 32; ++i) {
    p ^= b & (0u - (a >> 31));
    a <<= 1;
    b = (b >> 1) ^ (poly & (0u - (b & 1u)));
  }
  return p;
}

// x^(8n) mod P for n <= 2 kRow (head_shift[h][31] = Shift_h(x^0)), and reg moved past n zero bytes.
__device__ __forceinline__ std::uint32_t x8n(const DeviceTables* t, std::uint32_t n) {
  return n <= static_cast<std::uint32_t>(kRow)
             ? t->head_shift[n][31]
             : dev::multmodp(t->head_shift[n - kRow][31], t->head_shift[kRow][31], t->poly);
}
__device__ __forceinline__ std::uint32_t shift_n(const DeviceTables* t, std::uint32_t reg, std::uint32_t n) {
  return dev::multmodp(x8n(t, n), reg, t->poly);
}

// Fold ranges R[0, nr) of the window (3 words each: x | y << 16 window offsets, kk | kind << 9 |
// record offset << 16, and the result): every range cut into kChunk-byte chunks aligned to its end
// (the front chunk shorter), one chunk per lane (fold_raw from LDS), the chunk j from the end moved past
// the j kChunk bytes behind it by one multiply with K[j] = x^(8 kChunk j), and the chunks of a range
// XORed into its result word (LDS atomics). A range of kind kRangeWhole / kRangeHead starts from the
// initial register (the front chunk adds Shift_L(0xFFFFFFFF)), so its result is the CRC register after
// its bytes; a kRangeCarry range gives crc0. Whole wave; nr <= 64.
__device__ __forceinline__ void fold_ranges(const std::uint8_t* win, const std::uint32_t* tab, const std::uint32_t* inj,
                                            const std::uint32_t* K, std::uint32_t poly, const dev::LaneConstX& kc,
                                            std::uint32_t lane, std::uint32_t* R, std::uint32_t nr) {
  std::uint32_t xi = 0, yi = 0, ci = 0, ki = 0;
  if (lane < nr) {
    const std::uint32_t w0 = R[3 * lane];
    xi = w0 & 0xFFFFu;
    yi = w0 >> 16;
    ci = (yi - xi + kChunk - 1u) / kChunk;
    ki = (R[3 * lane + 1] >> 9) & 3u;
    R[3 * lane + 2] = 0u;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  std::uint32_t total;
  const std::uint32_t pre = lane_prefix(ci, &total);
  for (std::uint32_t base = 0; base < total; base += 64u) {
    const std::uint32_t g = base + lane;
    const bool act = g < total;
    std::uint32_t r = 0;  // the range of chunk g: the last one whose first chunk is at most g
    for (std::uint32_t i = 1; i < nr; ++i) r = g >= static_cast<std::uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(pre), static_cast<int>(i))) ? i : r;
    const std::uint32_t x = shfl_pos(xi, r), y = shfl_pos(yi, r), c = shfl_pos(ci, r), p = shfl_pos(pre, r);
    const std::uint32_t kd = shfl_pos(ki, r);
    const std::uint32_t k = g - p;                 // chunk from the range's front
    const std::uint32_t j = act ? c - 1u - k : 0u;  // chunk from its end
    const std::uint32_t ce = y - j * kChunk;
    const std::uint32_t cs = ce > x + kChunk ? ce - kChunk : x;
    const std::uint32_t L = act ? ce - cs : 0u;
    std::uint32_t v = fold_raw(win, tab, kc, cs, L);
    if (k == 0u && kd != kRangeCarry) v ^= inj[L];
    v = mul_lean(K[j], v, poly);
    if (act) atomicXor(&R[3 * r + 2], v);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

}  // namespace
}  // namespace tkv
