// The arena emit shared by the batched WAL decode (tkv_wal_decode.hip) and the SSTable scan
// (tkv_sst_scan.hip): n byte spans of an image in HBM gathered back to back into an arena. The arena is
// cut into tiles of kDecTile bytes, tile t, t + W, ... to wave t of W. A wave builds its tile in an LDS
// window, two records per lane and round: spans up to kShortSpan bytes by their lane, longer ones by the
// whole wave (tkv_wal_copy.h: lane_copy2, wave_copy), each clipped to the tile, and stores the tile once
// (store_tile), at any destination alignment. The callers differ in where a record's span lies in the
// image: the Src template argument, a small struct whose operator()(i) gives the address of span i.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "tkv_wal_copy.h"

namespace tkv {
namespace {

constexpr std::uint32_t kDecTile = 4096;             // arena bytes per emit tile
constexpr std::uint32_t kDecWin = 16 + kDecTile;     // the tile behind its destination's offset in its first granule
constexpr unsigned kDecWaves = 8;                    // waves per workgroup: 8 windows, 32.1 KiB of LDS
constexpr unsigned kDecThreads = 64 * kDecWaves;
constexpr unsigned kDecGroupsPerCu = 2;              // resident workgroups the launch is sized for
constexpr std::uint32_t kDecSteps = (kDecWin + 1023u) / 1024u;  // wave_copy steps of a span clipped to a tile
static_assert(kDecTile % 16 == 0 && kDecWin % 16 == 0, "16-byte granules");
static_assert(kDecGroupsPerCu * kDecWaves * kDecWin <= 163840, "LDS");

// Span i = arena bytes [o, o + len) of an arena of `total` bytes, len > 0: for every tile it has a byte
// in, the tile's first record when it holds the tile's first byte and its last record when it holds the
// tile's last byte. One writer per word: the non-empty spans tile the arena.
__device__ __forceinline__ void tile_entries(std::uint32_t* tile, std::uint64_t i, std::uint64_t o, std::uint64_t len,
                                             std::uint64_t total) {
  const std::uint64_t e = o + len < total ? o + len : total;  // (o + len <= total: the scan's own sums)
  for (std::uint64_t t = o / kDecTile; t * kDecTile < e; ++t) {
    if (o <= t * kDecTile) tile[2u * t] = static_cast<std::uint32_t>(i);
    if (e >= (t + 1u) * kDecTile || e == total) tile[2u * t + 1u] = static_cast<std::uint32_t>(i);
  }
}

template <class Src>
struct EmitArgs {
  Src src;                     // where span i lies in the image
  const std::uint64_t* pre;    // the spans of the arena being written: n + 1 offsets, the last one the total
  std::uint8_t* dst;
  std::uint64_t total;
  const std::uint32_t* tile;   // per tile, two words: first and last record with a byte in it
  std::uint64_t ntiles;
  std::uint64_t n;
  std::uint32_t nwaves;
};

// Record i's span as the emit pass reads it, one record per lane: arena offset, length (the scan's:
// a header is not read again) and source address.
struct DecRec {
  std::uint64_t ao;
  std::uint64_t len;
  std::uintptr_t src;
};
template <class Src>
__device__ __forceinline__ DecRec load_rec(const EmitArgs<Src>& a, std::uint64_t i, bool act) {
  DecRec r{0u, 0u, 0};
  if (act) {
    r.ao = a.pre[i];
    r.len = a.pre[i + 1u] - r.ao;
    r.src = a.src(i);
  }
  return r;
}

template <class Src>
__device__ __forceinline__ void emit_tile(const EmitArgs<Src>& a, std::uint8_t* win, std::uint64_t t, uint2 head, std::uint32_t lane) {
  const std::uint64_t ts = t * kDecTile;
  const std::uint64_t te = ts + kDecTile < a.total ? ts + kDecTile : a.total;
  const std::uint64_t first = head.x, last = head.y;
  std::uint8_t* const dst = a.dst + ts;
  const std::uint32_t o = static_cast<std::uint32_t>(reinterpret_cast<std::uintptr_t>(dst) & 15u);  // window granules are the arena's
  for (std::uint64_t rb = first; rb <= last; rb += 128u) {
    const std::uint64_t i0 = rb + lane, i1 = i0 + 64u;
    const DecRec r0 = load_rec(a, i0, i0 <= last && i0 < a.n);
    const DecRec r1 = load_rec(a, i1, i1 <= last && i1 < a.n);
    const Span s0 = clip_span(r0.src, r0.len, r0.ao, ts, te, ts, o);
    const Span s1 = clip_span(r1.src, r1.len, r1.ao, ts, te, ts, o);
    lane_copy2(win, lane_span(s0.d, s0.src, s0.len, s0.len != 0u && s0.len <= kShortSpan),
               lane_span(s1.d, s1.src, s1.len, s1.len != 0u && s1.len <= kShortSpan));
    wave_spans<kDecSteps>(win, s0, lane);
    wave_spans<kDecSteps>(win, s1, lane);
  }
  wave_sync();
  store_tile(win, dst, o, static_cast<std::uint32_t>(te - ts), lane);
  wave_sync();
}

template <class Src>
__global__ __launch_bounds__(kDecThreads) void span_emit(EmitArgs<Src> a) {
  __shared__ __attribute__((aligned(16))) std::uint8_t lds[kDecWaves * kDecWin];
  const std::uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const std::uint32_t lane = threadIdx.x & 63u;
  std::uint8_t* win = lds + wv * kDecWin;
  std::uint64_t t = blockIdx.x * kDecWaves + wv;
  if (t >= a.ntiles) return;
  // a tile's first and last record are read one tile ahead
  uint2 h = *reinterpret_cast<const uint2*>(a.tile + 2u * t);
  for (; t < a.ntiles; t += a.nwaves) {
    const uint2 hn = t + a.nwaves < a.ntiles ? *reinterpret_cast<const uint2*>(a.tile + 2u * (t + a.nwaves)) : make_uint2(1u, 0u);
    emit_tile(a, win, t, h, lane);
    h = hn;
  }
}

// The emit of one copied arena (e.src, e.pre, e.dst, e.total, e.tile, e.n set by the caller) on a device
// of ncu compute units; returns its waves.
template <class Src>
std::uint32_t launch_span_emit(int ncu, EmitArgs<Src> e, hipStream_t st) {
  e.ntiles = (e.total + kDecTile - 1u) / kDecTile;
  const std::uint64_t want = (e.ntiles + kDecWaves - 1u) / kDecWaves;
  const unsigned grid = static_cast<unsigned>(std::min<std::uint64_t>(want, static_cast<std::uint64_t>(ncu) * kDecGroupsPerCu));
  e.nwaves = grid * kDecWaves;
  hipLaunchKernelGGL(span_emit<Src>, dim3(grid), dim3(kDecThreads), 0, st, e);
  return e.nwaves;
}

}  // namespace
}  // namespace tkv
