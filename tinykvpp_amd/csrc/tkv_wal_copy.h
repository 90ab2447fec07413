// Device pieces shared by the WAL group-commit encoder (tkv_wal_encode.hip), the batched WAL decode
// (tkv_wal_decode.hip) and the SSTable flush (tkv_sst_build.hip): the copy of byte spans at any source /
// destination alignment into a wave's LDS window and of the window's tile out to memory (one span per
// lane, or one span by the whole wave; loads touch only source granules that hold a byte of the span).
// Includes the u64 scan its users run in front of their copies (tkv_scan.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "tkv_crc32_device.h"
#include "tkv_scan.h"

namespace tkv {
namespace {

constexpr std::uint32_t kShortSpan = 64;      // keys / values up to this long are copied by their record's lane

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- spans into an LDS window -----------------------------------------------------------------------

// The aligned dword / granule at address p when it holds a byte of [s, e), else zero (no load leaves
// the source span rounded out to its granules).
// (Global address space: a generic load could alias the LDS window, and every load of a copy would then
// wait for the window stores in front of it.)
using GlobalU32 = const __attribute__((address_space(1))) std::uint32_t*;
typedef std::uint32_t U32x4 __attribute__((ext_vector_type(4)));
using GlobalU128 = const __attribute__((address_space(1))) U32x4*;
__device__ __forceinline__ std::uint32_t ld4(std::uintptr_t p, std::uintptr_t s, std::uintptr_t e) {
  return (p + 4u > s && p < e) ? *reinterpret_cast<GlobalU32>(p) : 0u;
}
__device__ __forceinline__ uint4 ld16(std::uintptr_t p, std::uintptr_t s, std::uintptr_t e) {
  U32x4 v = {0u, 0u, 0u, 0u};
  if (p + 16u > s && p < e) v = *reinterpret_cast<GlobalU128>(p);
  return make_uint4(v.x, v.y, v.z, v.w);
}

// The bytes of v (window bytes [q, q + 4)) that lie in [d, e).
__device__ __forceinline__ void put4(std::uint8_t* win, std::uint32_t q, std::uint32_t v, std::uint32_t d, std::uint32_t e) {
  if (q >= d && q + 4u <= e) {
    *reinterpret_cast<std::uint32_t*>(win + q) = v;
  } else {
#pragma unroll
    for (std::uint32_t b = 0; b < 4u; ++b)
      if (q + b >= d && q + b < e) win[q + b] = static_cast<std::uint8_t>(v >> (8u * b));
  }
}

// One lane's copy of len source bytes at src to window bytes [d, d + len) (nothing when on is false):
// aligned source dwords, each window dword from two of them (v_alignbyte).
struct LaneSpan {
  std::uint32_t q, d, e, sh;      // next window dword, the span's window bytes, source misalignment
  std::uintptr_t sa, s0, se;      // source address of window dword q rounded down, the source bytes
};
__device__ __forceinline__ LaneSpan lane_span(std::uint32_t d, std::uintptr_t src, std::uint32_t len, bool on) {
  LaneSpan s{};
  if (on) {
    s.q = d & ~3u;
    s.d = d;
    s.e = d + len;
    const std::uintptr_t sp = src - (d - s.q);  // source address of window byte q
    s.sh = static_cast<std::uint32_t>(sp & 3u);
    s.sa = sp & ~static_cast<std::uintptr_t>(3);
    s.s0 = src;
    s.se = src + len;
  }
  return s;
}
// Two such copies side by side (a record's key and value), four window dwords of each per step with the
// step's ten loads issued together.
__device__ __forceinline__ void lane_copy2(std::uint8_t* win, LaneSpan a, LaneSpan b) {
  while (a.q < a.e || b.q < b.e) {
    std::uint32_t wa[5], wb[5];
#pragma unroll
    for (std::uint32_t k = 0; k < 5u; ++k) {
      wa[k] = ld4(a.sa + 4u * k, a.s0, a.se);
      wb[k] = ld4(b.sa + 4u * k, b.s0, b.se);
    }
#pragma unroll
    for (std::uint32_t k = 0; k < 4u; ++k) {
      put4(win, a.q + 4u * k, __builtin_amdgcn_alignbyte(wa[k + 1u], wa[k], a.sh), a.d, a.e);
      put4(win, b.q + 4u * k, __builtin_amdgcn_alignbyte(wb[k + 1u], wb[k], b.sh), b.d, b.e);
    }
    a.q += 16u;
    a.sa += 16u;
    b.q += 16u;
    b.sa += 16u;
  }
}

// The same by the whole wave (wave-uniform arguments), a 16-byte window granule per lane: the two
// source granules that hold its bytes, shifted by the wave-uniform misalignment. A span covers at most
// STEPS steps of 64 granules (it lies in the window); their loads are issued together.
template <std::uint32_t STEPS>
__device__ __forceinline__ void wave_copy(std::uint8_t* win, std::uint32_t d, std::uintptr_t src, std::uint32_t len, std::uint32_t lane) {
  const std::uint32_t e = d + len;
  const std::uint32_t g0 = d & ~15u;
  const std::uintptr_t sp0 = src - (d - g0);  // source address of window byte g0
  const std::uint32_t r = static_cast<std::uint32_t>(sp0 & 15u);
  const std::uint32_t k = r >> 2, sh = r & 3u;
  const std::uintptr_t se = src + len;
  uint4 As[STEPS], Bs[STEPS];
#pragma unroll
  for (std::uint32_t it = 0; it < STEPS; ++it) {
    const std::uint32_t g = g0 + 16u * lane + 1024u * it;
    const std::uintptr_t sa = (sp0 + (g - g0)) & ~static_cast<std::uintptr_t>(15);
    // (past the span's end sa >= se: nothing is loaded)
    As[it] = ld16(sa, src, se);
    Bs[it] = ld16(sa + 16u, src, se);
  }
#pragma unroll
  for (std::uint32_t it = 0; it < STEPS; ++it) {
    const std::uint32_t g = g0 + 16u * lane + 1024u * it;
    if (g >= e) break;
    const uint4 A = As[it], B = Bs[it];
    uint4 v;
    switch (k) {
      case 0:
        v = make_uint4(__builtin_amdgcn_alignbyte(A.y, A.x, sh), __builtin_amdgcn_alignbyte(A.z, A.y, sh),
                       __builtin_amdgcn_alignbyte(A.w, A.z, sh), __builtin_amdgcn_alignbyte(B.x, A.w, sh));
        break;
      case 1:
        v = make_uint4(__builtin_amdgcn_alignbyte(A.z, A.y, sh), __builtin_amdgcn_alignbyte(A.w, A.z, sh),
                       __builtin_amdgcn_alignbyte(B.x, A.w, sh), __builtin_amdgcn_alignbyte(B.y, B.x, sh));
        break;
      case 2:
        v = make_uint4(__builtin_amdgcn_alignbyte(A.w, A.z, sh), __builtin_amdgcn_alignbyte(B.x, A.w, sh),
                       __builtin_amdgcn_alignbyte(B.y, B.x, sh), __builtin_amdgcn_alignbyte(B.z, B.y, sh));
        break;
      default:
        v = make_uint4(__builtin_amdgcn_alignbyte(B.x, A.w, sh), __builtin_amdgcn_alignbyte(B.y, B.x, sh),
                       __builtin_amdgcn_alignbyte(B.z, B.y, sh), __builtin_amdgcn_alignbyte(B.w, B.z, sh));
        break;
    }
    if (g >= d && g + 16u <= e) {
      *reinterpret_cast<uint4*>(win + g) = v;
    } else {
      put4(win, g, v.x, d, e);
      put4(win, g + 4u, v.y, d, e);
      put4(win, g + 8u, v.z, d, e);
      put4(win, g + 12u, v.w, d, e);
    }
  }
}

// A source span of len bytes at src that lies at destination bytes [sx, sx + len), cut to the
// destination bytes [clo, chi) this wave lays out: its window offset (wb = window offset of destination
// byte ts), source address and length (0 when nothing is left).
struct Span {
  std::uint32_t d, len;
  std::uintptr_t src;
};
__device__ __forceinline__ Span clip_span(std::uintptr_t src, std::uint64_t len, std::uint64_t sx, std::uint64_t clo,
                                          std::uint64_t chi, std::uint64_t ts, std::uint32_t wb) {
  const std::uint64_t c0 = sx > clo ? sx : clo;
  const std::uint64_t c1 = sx + len < chi ? sx + len : chi;
  Span s{0u, 0u, src};
  if (c1 > c0) {
    s.len = static_cast<std::uint32_t>(c1 - c0);
    s.src = src + static_cast<std::uintptr_t>(c0 - sx);
    s.d = wb + static_cast<std::uint32_t>(static_cast<std::int32_t>(static_cast<std::int64_t>(c0 - ts)));
  }
  return s;
}

// Long spans of the round's records, one after the other by the whole wave.
template <std::uint32_t STEPS>
__device__ __forceinline__ void wave_spans(std::uint8_t* win, const Span& s, std::uint32_t lane) {
  unsigned long long m = __ballot(s.len > kShortSpan);
  while (m) {
    const std::uint32_t l = static_cast<std::uint32_t>(__ffsll(m)) - 1u;
    m &= m - 1ull;
    const std::uint32_t d = static_cast<std::uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(s.d), static_cast<int>(l)));
    const std::uint32_t len = static_cast<std::uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(s.len), static_cast<int>(l)));
    const std::uintptr_t src = static_cast<std::uintptr_t>(dev::readlane64(static_cast<std::uint64_t>(s.src), l));
    wave_copy<STEPS>(win, d, src, len, lane);
  }
}

// The tile out of the window: the len bytes at dst, which lie at window bytes [o, o + len) of w
// (o = dst & 15, so window granules are the destination's): whole granules with 16-byte stores, the
// (at most two) granules shared with a neighbour or with bytes outside the destination bytewise.
__device__ __forceinline__ void store_tile(const std::uint8_t* w, std::uint8_t* dst, std::uint32_t o, std::uint32_t len,
                                           std::uint32_t lane) {
  const std::uint32_t ng = (o + len + 15u) >> 4;
  std::uint8_t* const g0 = dst - o;
  for (std::uint32_t j = lane; j < ng; j += 64u) {
    const std::uint32_t lo = 16u * j, hi = lo + 16u;  // bytes from g0
    const uint4 v = *reinterpret_cast<const uint4*>(w + lo);
    if (lo >= o && hi <= o + len) {
      *reinterpret_cast<uint4*>(g0 + lo) = v;
    } else {
      const std::uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (std::uint32_t b = 0; b < 16u; ++b)
        if (lo + b >= o && lo + b < o + len) g0[lo + b] = static_cast<std::uint8_t>(wd[b >> 2] >> (8u * (b & 3u)));
    }
  }
}

}  // namespace
}  // namespace tkv
