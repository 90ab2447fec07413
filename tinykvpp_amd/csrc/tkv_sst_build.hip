// SSTable flush on the device (include/tkv_crc32.h "SSTable flush"): the loop of
// sstable_writer::append / is_data_block_complete / get_data_block / record_data_block / get_index /
// get_footer for entries held as key / value arenas with per-entry offsets and lengths, as one call
// that writes the whole file image: data blocks cut by the greedy size rule, the index, the footer,
// every checksum stamped.
//
// sst_sizes / scan_level / scan_add (tkv_scan.h): the counted sizes e_i = 8 + kl + vl and the
//   written sizes w_i = vlen(kl) + kl + vlen(vl) + vl, their u64 exclusive prefix scans S and W, and
//   the flag for a length whose varint would not fit the 4 bytes counted for it.
// sst_next: J[s] = the entry that starts the block after one that starts at s (binary search in S;
//   the sink is n).
// chain_double (tkv_scan.h): the chain 0, J(0), J(J(0)), ... marked by pointer doubling over [0, n] in
//   ceil(log2(Bmax + 1)) rounds, Bmax = min(n, S[n] / T + 1).
// sst_marks + scan: the block of every entry and the first entry of every block; sst_blocks: every
//   block's offset, size, body base; sst_index_sizes + scan: the index entries' offsets.
// sst_publish: {file_size, B, index_offset, index_size, flags} to a pinned block; the host decides
//   invalid / overflow before anything is written for the caller.
// sst_positions: every entry's file offset. sst_tiles: for every 4 KiB tile of the data region the
//   blocks and entries that hold a byte of it, by binary search (entries do not tile the file: headers,
//   slack and padding lie between them, and a tile may hold no entry or no header).
// sst_emit: one wave per tile builds it in a zeroed LDS window (headers one per lane, entries one per
//   lane with their varints, short spans by the lane, long spans by the wave) and stores it once.
// sst_index: the index image and the footer, one wave per index entry.
// One CRC batch over the B block images and the span index || footer[0, 16) (every CRC field was
// written as zero, so the plain CRC is the stamp), then sst_stamp stores the B + 1 fields bytewise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>

#include "tkv_crc32.h"
#include "tkv_crc32_device.h"
#include "tkv_device_util.h"
#include "tkv_engine.h"
#include "tkv_scan.h"
#include "tkv_sst_layout.h"
#include "tkv_wal_copy.h"

namespace tkv {
namespace {

constexpr std::uint32_t kSstTile = 4096;   // file bytes per emit tile
constexpr std::uint32_t kSstPre = 16;      // window bytes in front of the tile's 16-byte granule
constexpr std::uint32_t kSstWin = kSstPre + 16 + kSstTile + 16;
constexpr unsigned kSstWaves = 16;         // waves per emit workgroup
constexpr unsigned kSstThreads = 64 * kSstWaves;
constexpr unsigned kSstHres = 8;           // words of the pinned result block
constexpr std::uint32_t kSstSteps = (kSstWin + 1023u) / 1024u;  // a span lies in the window
enum : int { kFlagLen = 1, kFlagBlock = 2 };
static_assert(kSstTile % 16 == 0 && kSstWin % 16 == 0, "16-byte granules");
static_assert(kSstWaves * kSstWin <= 163840, "LDS");

struct SstArgs {
  const std::uint8_t* keys;
  const std::uint64_t* key_off;
  const std::uint32_t* key_len;
  const std::uint8_t* vals;
  const std::uint64_t* val_off;
  const std::uint32_t* val_len;  // nullable: every value empty
  std::uint64_t n;
  std::uint32_t T;
  std::uint8_t* file;
  // per entry (n + 1 entries each)
  std::uint64_t* S;        // exclusive scan of the counted sizes, S[n] the total; later the entries' file offsets
  std::uint64_t* W;        // exclusive scan of the written sizes
  std::uint32_t* J;        // next block start of a block that starts here
  std::uint32_t* Ja;       // ping-pong buffers of the doubling
  std::uint32_t* Jb;
  std::uint32_t* mark;     // 1: a block starts here
  std::uint64_t* blk;      // exclusive scan of the marks
  // per block (bmax + 1 entries each)
  std::uint32_t* bfirst;   // b_j; [B] = n
  std::uint64_t* boff;     // O_j; [B] = index_offset (the footer's CRC span)
  std::uint32_t* bsize;    // 36 + z_j; [B] = index_size + 16
  std::uint64_t* bbase;    // file offset of the body's byte 0 minus W[b_j]
  std::uint64_t* ioff;     // exclusive scan of the index entry sizes
  std::uint32_t* bcrc;
  std::uint64_t bmax;
  const std::uint64_t* nblk;  // B on the device (the mark scan's total)
  std::uint64_t B, index_offset, index_size;
  std::uint32_t* tile;     // per tile: first block, last block, first entry, entries
  std::uint64_t ntiles;
  std::uint32_t nwaves;
  unsigned long long* flags;
  std::uint64_t* o_off;    // the caller's block arrays, each nullable
  std::uint32_t* o_size;
  std::uint32_t* o_first;
};

__device__ __forceinline__ std::uint32_t entry_vl(const SstArgs& a, std::uint64_t i) { return a.val_len ? a.val_len[i] : 0u; }

// Byte k of LEB128(v) whose length is nv.
__device__ __forceinline__ std::uint8_t varint_byte(std::uint32_t v, std::uint32_t k, std::uint32_t nv) {
  return static_cast<std::uint8_t>(((v >> (7u * k)) & 0x7Fu) | (k + 1u < nv ? 0x80u : 0u));
}

// ---- sizes ------------------------------------------------------------------------------------------

// Level 0 of a size scan: which = 0 the counted sizes to a.S, 1 the written sizes to a.W.
__global__ __launch_bounds__(kScanThreads) void sst_sizes(SstArgs a, int which, std::uint64_t* bsum) {
  const std::uint64_t i0 = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
  std::uint64_t v[kScanItems];
  std::uint32_t bad = 0;
#pragma unroll
  for (unsigned k = 0; k < kScanItems; ++k) {
    const std::uint64_t i = i0 + k;
    v[k] = 0;
    if (i < a.n) {
      const std::uint32_t kl = a.key_len[i], vl = entry_vl(a, i);
      bad |= (kl >= kSstMaxLen || vl >= kSstMaxLen) ? 1u : 0u;
      v[k] = which ? sst_written(kl, vl) : sst_counted(kl, vl);
    }
  }
  scan_items(v, i0, a.n, which ? a.W : a.S, bsum);
  if (bad) atomicOr(a.flags, static_cast<unsigned long long>(kFlagLen));
}

__global__ void sst_publish_sizes(SstArgs a, const std::uint64_t* top, std::uint64_t* h) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    a.S[a.n] = *top;
    h[0] = *top;
    h[1] = *a.flags;
    h[7] = 1;
  }
}

// ---- cut --------------------------------------------------------------------------------------------

// J[s] = the smallest m in (s, n] with S[m] - S[s] >= T, or n: where the block after one that starts at
// s starts (append followed by is_data_block_complete). mark = {0}.
__global__ __launch_bounds__(kScanThreads) void sst_next(SstArgs a) {
  const std::uint64_t s = blockIdx.x * static_cast<std::uint64_t>(kScanThreads) + threadIdx.x;
  if (s > a.n) return;
  a.mark[s] = s == 0 ? 1u : 0u;
  if (s == a.n) {
    a.J[s] = static_cast<std::uint32_t>(a.n);
    return;
  }
  const std::uint64_t want = a.S[s] + a.T;
  std::uint64_t lo = s + 1u, hi = a.n;
  while (lo < hi) {
    const std::uint64_t mid = lo + (hi - lo) / 2u;
    if (a.S[mid] >= want) hi = mid;
    else lo = mid + 1u;
  }
  a.J[s] = static_cast<std::uint32_t>(lo);
}

// Level 0 of the mark scan over [0, n): the blocks in front of every entry.
__global__ __launch_bounds__(kScanThreads) void sst_marks(SstArgs a, std::uint64_t* bsum) {
  const std::uint64_t i0 = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
  std::uint64_t v[kScanItems];
#pragma unroll
  for (unsigned k = 0; k < kScanItems; ++k) v[k] = i0 + k < a.n ? a.mark[i0 + k] : 0u;
  scan_items(v, i0, a.n, a.blk, bsum);
}

// Every block from its first entry: b_j, O_j, 36 + z_j, the body base.
__global__ __launch_bounds__(kScanThreads) void sst_blocks(SstArgs a) {
  const std::uint64_t i = blockIdx.x * static_cast<std::uint64_t>(kScanThreads) + threadIdx.x;
  if (i >= a.n || !a.mark[i]) return;
  const std::uint64_t j = a.blk[i];
  if (j >= a.bmax) return;  // (cannot happen: B <= bmax)
  const std::uint64_t next = a.J[i];
  const std::uint64_t z = a.S[next] - a.S[i];
  const std::uint64_t off = kSstOverhead * j + a.S[i];
  const std::uint64_t size = kSstOverhead + z;
  if (size > 0xFFFFFFFFull) atomicOr(a.flags, static_cast<unsigned long long>(kFlagBlock));
  a.bfirst[j] = static_cast<std::uint32_t>(i);
  a.boff[j] = off;
  a.bsize[j] = static_cast<std::uint32_t>(size);
  a.bbase[j] = off + kSstHeader + sst_vlen(z) - a.W[i];
}

// Level 0 of the index scan over [0, bmax): vlen(kl) + kl + 16 of every block's first entry.
__global__ __launch_bounds__(kScanThreads) void sst_index_sizes(SstArgs a, std::uint64_t* bsum) {
  const std::uint64_t j0 = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
  const std::uint64_t B = *a.nblk;
  std::uint64_t v[kScanItems];
#pragma unroll
  for (unsigned k = 0; k < kScanItems; ++k) {
    v[k] = 0;
    if (j0 + k < B && j0 + k < a.bmax) {
      const std::uint32_t kl = a.key_len[a.bfirst[j0 + k]];
      v[k] = static_cast<std::uint64_t>(sst_vlen(kl)) + kl + kSstIndexFixed;
    }
  }
  scan_items(v, j0, a.bmax, a.ioff, bsum);
}

// The sizes for the host, and entry B of the block arrays: the end of the entries and the footer's span.
__global__ void sst_publish(SstArgs a, const std::uint64_t* idx_top, std::uint64_t* h) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const std::uint64_t B = *a.nblk;
    const std::uint64_t isz = 8u + *idx_top;
    const std::uint64_t ioff = kSstOverhead * B + a.S[a.n];
    if (B <= a.bmax) {
      a.bfirst[B] = static_cast<std::uint32_t>(a.n);
      a.boff[B] = ioff;
      a.bsize[B] = static_cast<std::uint32_t>(isz + kSstFooterCrc);
    }
    h[0] = ioff + isz + kSstFooter;
    h[1] = B;
    h[2] = ioff;
    h[3] = isz;
    h[4] = *a.flags;
    h[7] = 2;
  }
}

// ---- layout -----------------------------------------------------------------------------------------

// Entry i's file offset to S[i] (S itself is no longer needed).
__global__ __launch_bounds__(kScanThreads) void sst_positions(SstArgs a) {
  const std::uint64_t i = blockIdx.x * static_cast<std::uint64_t>(kScanThreads) + threadIdx.x;
  if (i >= a.n) return;
  const std::uint64_t j = a.blk[i] + a.mark[i] - 1u;
  a.S[i] = a.bbase[j] + a.W[i];
}

// Tile t of the data region [0, index_offset): the blocks [jf, jl] and the entries [ef, ef + cnt) that
// hold one of its bytes.
__global__ __launch_bounds__(kScanThreads) void sst_tiles(SstArgs a) {
  const std::uint64_t t = blockIdx.x * static_cast<std::uint64_t>(kScanThreads) + threadIdx.x;
  if (t >= a.ntiles) return;
  const std::uint64_t ts = t * kSstTile;
  const std::uint64_t te = ts + kSstTile < a.index_offset ? ts + kSstTile : a.index_offset;
  // the last block that starts at or before x (boff[0] = 0)
  auto block_of = [&](std::uint64_t x) {
    std::uint64_t lo = 0, hi = a.B;  // the first block that starts behind x
    while (lo < hi) {
      const std::uint64_t mid = lo + (hi - lo) / 2u;
      if (a.boff[mid] > x) hi = mid;
      else lo = mid + 1u;
    }
    return lo - 1u;
  };
  const std::uint64_t jf = block_of(ts), jl = block_of(te - 1u);
  const std::uint64_t e0 = a.bfirst[jf], e1 = a.bfirst[jl + 1u];
  // the first entry that ends behind ts, the entries that start before te
  std::uint64_t lo = e0, hi = e1;
  while (lo < hi) {
    const std::uint64_t mid = lo + (hi - lo) / 2u;
    if (a.S[mid] + sst_written(a.key_len[mid], entry_vl(a, mid)) > ts) hi = mid;
    else lo = mid + 1u;
  }
  const std::uint64_t ef = lo;
  lo = e0;
  hi = e1;
  while (lo < hi) {
    const std::uint64_t mid = lo + (hi - lo) / 2u;
    if (a.S[mid] >= te) hi = mid;
    else lo = mid + 1u;
  }
  a.tile[4u * t] = static_cast<std::uint32_t>(jf);
  a.tile[4u * t + 1u] = static_cast<std::uint32_t>(jl);
  a.tile[4u * t + 2u] = static_cast<std::uint32_t>(ef);
  a.tile[4u * t + 3u] = static_cast<std::uint32_t>(lo > ef ? lo - ef : 0u);
}

// ---- emit -------------------------------------------------------------------------------------------

__device__ __forceinline__ void emit_tile(const SstArgs& a, std::uint8_t* win, std::uint64_t t, std::uint32_t lane) {
  const std::uint64_t ts = t * kSstTile;
  const std::uint64_t te = ts + kSstTile < a.index_offset ? ts + kSstTile : a.index_offset;
  std::uint8_t* const dst = a.file + ts;
  const std::uint32_t o = static_cast<std::uint32_t>(reinterpret_cast<std::uintptr_t>(dst) & 15u);
  const std::uint32_t wb = kSstPre + o;  // window offset of file byte ts: window granules are the file's
  const uint4 head = *reinterpret_cast<const uint4*>(a.tile + 4u * t);
  // slack and padding are whatever no item writes: zero
  for (std::uint32_t k = 16u * lane; k < kSstWin; k += 1024u) *reinterpret_cast<uint4*>(win + k) = make_uint4(0u, 0u, 0u, 0u);
  wave_sync();
  // a window byte for file byte pos when the tile holds it
  auto put = [&](std::uint64_t pos, std::uint8_t v) {
    if (pos >= ts && pos < te) win[wb + static_cast<std::uint32_t>(pos - ts)] = v;
  };
  // block headers, one per lane: varint(20) | header | varint(z)
  for (std::uint64_t jb = head.x; jb <= head.y; jb += 64u) {
    const std::uint64_t j = jb + lane;
    if (j <= head.y) {
      const std::uint64_t off = a.boff[j];
      const std::uint32_t z = a.bsize[j] - kSstOverhead;
      const std::uint32_t nz = sst_vlen(z);
      if (off + kSstHeader + nz > ts && off < te) {
        const std::uint32_t c = a.bfirst[j + 1u] - a.bfirst[j];
        put(off, 20u);
#pragma unroll
        for (std::uint32_t b = 0; b < 4u; ++b) {
          put(off + 1u + b, static_cast<std::uint8_t>(c >> (8u * b)));
          put(off + 5u + b, static_cast<std::uint8_t>(z >> (8u * b)));
          put(off + 9u + b, static_cast<std::uint8_t>(z >> (8u * b)));
        }
#pragma unroll
        for (std::uint32_t k = 0; k < 5u; ++k)
          if (k < nz) put(off + kSstHeader + k, varint_byte(z, k, nz));
      }
    }
  }
  // entries, one per lane: varint(kl) | key | varint(vl) | value
  const std::uint64_t ef = head.z;
  const std::uint32_t cnt = head.w;
  for (std::uint32_t rb = 0; rb < cnt; rb += 64u) {
    const bool act = rb + lane < cnt;
    const std::uint64_t i = ef + rb + lane;
    Span ks{0u, 0u, 0}, vs{0u, 0u, 0};
    if (act) {
      const std::uint64_t fp = a.S[i];
      const std::uint32_t kl = a.key_len[i], vl = entry_vl(a, i);
      const std::uint32_t nk = sst_vlen(kl), nv = sst_vlen(vl);
      const std::uint64_t vp = fp + nk + kl;  // varint(vl)
#pragma unroll
      for (std::uint32_t k = 0; k < 4u; ++k) {
        if (k < nk) put(fp + k, varint_byte(kl, k, nk));
        if (k < nv) put(vp + k, varint_byte(vl, k, nv));
      }
      if (kl) ks = clip_span(reinterpret_cast<std::uintptr_t>(a.keys) + a.key_off[i], kl, fp + nk, ts, te, ts, wb);
      if (vl) vs = clip_span(reinterpret_cast<std::uintptr_t>(a.vals) + a.val_off[i], vl, vp + nv, ts, te, ts, wb);
    }
    lane_copy2(win, lane_span(ks.d, ks.src, ks.len, ks.len != 0u && ks.len <= kShortSpan),
               lane_span(vs.d, vs.src, vs.len, vs.len != 0u && vs.len <= kShortSpan));
    wave_spans<kSstSteps>(win, ks, lane);
    wave_spans<kSstSteps>(win, vs, lane);
  }
  wave_sync();
  store_tile(win + kSstPre, dst, o, static_cast<std::uint32_t>(te - ts), lane);
  wave_sync();
}

__global__ __launch_bounds__(kSstThreads) void sst_emit(SstArgs a) {
  __shared__ __attribute__((aligned(16))) std::uint8_t lds[kSstWaves * kSstWin];
  const std::uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const std::uint32_t lane = threadIdx.x & 63u;
  std::uint8_t* win = lds + wv * kSstWin;
  for (std::uint64_t t = blockIdx.x * kSstWaves + wv; t < a.ntiles; t += a.nwaves) emit_tile(a, win, t, lane);
}

// The index image and the footer (CRC field zero), bytewise: one wave per index entry.
__global__ __launch_bounds__(256) void sst_index(SstArgs a) {
  const std::uint64_t w0 = (blockIdx.x * 256ull + threadIdx.x) >> 6;
  const std::uint64_t nw = (gridDim.x * 256ull) >> 6;
  const std::uint32_t lane = threadIdx.x & 63u;
  std::uint8_t* const idx = a.file + a.index_offset;
  if (w0 == 0) {
    if (lane < 8u) idx[lane] = static_cast<std::uint8_t>(a.B >> (8u * lane));
    if (lane < kSstFooter) {
      const std::uint32_t f[5] = {static_cast<std::uint32_t>(a.index_offset), static_cast<std::uint32_t>(a.index_size), 0u, 0u, 0u};
      std::uint32_t w = 0;
#pragma unroll
      for (std::uint32_t k = 0; k < 5u; ++k) w = (lane >> 2) == k ? f[k] : w;
      idx[a.index_size + lane] = static_cast<std::uint8_t>(w >> (8u * (lane & 3u)));
    }
  }
  for (std::uint64_t j = w0; j < a.B; j += nw) {
    const std::uint64_t i = a.bfirst[j];
    const std::uint32_t kl = a.key_len[i];
    const std::uint32_t nk = sst_vlen(kl);
    std::uint8_t* const d = idx + 8u + a.ioff[j];
    if (lane < nk) d[lane] = varint_byte(kl, lane, nk);
    const std::uint8_t* const src = a.keys + a.key_off[i];
    for (std::uint32_t b = lane; b < kl; b += 64u) d[nk + b] = src[b];
    if (lane < kSstIndexFixed) {
      const std::uint64_t v = lane < 8u ? a.boff[j] : static_cast<std::uint64_t>(a.bsize[j]);
      d[nk + kl + lane] = static_cast<std::uint8_t>(v >> (8u * (lane & 7u)));
    }
  }
}

// The caller's block arrays.
__global__ __launch_bounds__(kScanThreads) void sst_out(SstArgs a) {
  const std::uint64_t j = blockIdx.x * static_cast<std::uint64_t>(kScanThreads) + threadIdx.x;
  if (j >= a.B) return;
  if (a.o_off) a.o_off[j] = a.boff[j];
  if (a.o_size) a.o_size[j] = a.bsize[j];
  if (a.o_first) a.o_first[j] = a.bfirst[j];
}

// The B block stamps and the footer's (entry B) into their fields.
__global__ __launch_bounds__(kScanThreads) void sst_stamp(SstArgs a) {
  const std::uint64_t j = blockIdx.x * static_cast<std::uint64_t>(kScanThreads) + threadIdx.x;
  if (j > a.B) return;
  const std::uint32_t c = a.bcrc[j];
  std::uint8_t* p = j < a.B ? a.file + a.boff[j] + kSstCrc : a.file + a.index_offset + a.index_size + kSstFooterCrc;
  p[0] = static_cast<std::uint8_t>(c);
  p[1] = static_cast<std::uint8_t>(c >> 8);
  p[2] = static_cast<std::uint8_t>(c >> 16);
  p[3] = static_cast<std::uint8_t>(c >> 24);
}

// ---- host side --------------------------------------------------------------------------------------

// Per-device scratch, grown by doubling and kept between calls (guarded by mu).
struct SstScratch : ScratchBase {
  DeviceBuf S, W, J, Ja, Jb, mark, blk;              // per entry
  DeviceBuf sums_a, sums_b;                          // scan levels above the first
  DeviceBuf bfirst, boff, bsize, bbase, ioff, bcrc;  // per block
  DeviceBuf tile;
  unsigned long long*& flags = words;
};

// The calling thread's device builds (tkv_debug_sst_build_last, tkv_debug_sst_build_phases).
thread_local PathStats g_sst;

int build_locked(SstScratch& s, SstArgs a, const SstBuildCall& c, hipStream_t st) {
  const std::uint64_t n = a.n, n1 = a.n + 1u;
  const ScanPlan plan(n);
  if (int rc = s.S.take(n1, &a.S)) return rc;
  if (int rc = s.W.take(n1, &a.W)) return rc;
  std::uint64_t *sums_a = nullptr, *sums_b = nullptr;
  if (int rc = s.sums_a.take(plan.nsum, &sums_a)) return rc;
  if (int rc = s.sums_b.take(plan.nsum, &sums_b)) return rc;
  a.flags = s.flags;
  std::uint64_t *lvS[kScanLevels + 1], *lvW[kScanLevels + 1];
  plan.place(a.S, sums_a, lvS);
  plan.place(a.W, sums_b, lvW);
  const dim3 g0(static_cast<unsigned>(plan.m[1])), tb(kScanThreads);
  const dim3 gn1(blocks(n1, kScanThreads));

  // sizes
  PhaseClock clock(st, g_sst.timing != 0, g_sst.phase);
  clock.mark(0);
  TKV_HIP_RC(hipMemsetAsync(s.flags, 0, sizeof(unsigned long long), st));
  s.h_res[7] = 0;
  hipLaunchKernelGGL(sst_sizes, g0, tb, 0, st, a, 0, lvS[1]);
  scan_up(plan, lvS, st);
  hipLaunchKernelGGL(sst_sizes, g0, tb, 0, st, a, 1, lvW[1]);
  scan_up(plan, lvW, st);
  hipLaunchKernelGGL(sst_publish_sizes, dim3(1), dim3(64), 0, st, a, lvS[plan.levels], s.d_hres);
  clock.mark(1);
  if (int rc = s.wait(st, 7, 1, "SSTable build: the size scan left no result")) return rc;
  if (s.h_res[1] & kFlagLen) return set_error(TKV_INVALID_ARGUMENT, "SSTable build: a key or value length is 2^28 or more");
  const std::uint64_t total = s.h_res[0];
  const std::uint64_t bmax = std::min<std::uint64_t>(n, total / a.T + 1u);
  const std::uint32_t rounds = sst_rounds(bmax);

  // cut
  if (int rc = s.J.take(n1, &a.J)) return rc;
  if (int rc = s.Ja.take(n1, &a.Ja)) return rc;
  if (int rc = s.Jb.take(n1, &a.Jb)) return rc;
  if (int rc = s.mark.take(n1, &a.mark)) return rc;
  if (int rc = s.blk.take(n1, &a.blk)) return rc;
  if (int rc = s.bfirst.take(bmax + 1u, &a.bfirst)) return rc;
  if (int rc = s.boff.take(bmax + 1u, &a.boff)) return rc;
  if (int rc = s.bsize.take(bmax + 1u, &a.bsize)) return rc;
  if (int rc = s.bbase.take(bmax + 1u, &a.bbase)) return rc;
  if (int rc = s.ioff.take(bmax + 1u, &a.ioff)) return rc;
  if (int rc = s.bcrc.take(bmax + 1u, &a.bcrc)) return rc;
  a.bmax = bmax;
  scan_down(plan, lvS, st);
  scan_down(plan, lvW, st);
  hipLaunchKernelGGL(sst_next, gn1, tb, 0, st, a);
  chain_double(a.J, a.Ja, a.Jb, a.mark, n1, rounds, st);
  std::uint64_t* lvM[kScanLevels + 1];
  plan.place(a.blk, sums_a, lvM);  // (the S levels are done with)
  hipLaunchKernelGGL(sst_marks, g0, tb, 0, st, a, lvM[1]);
  scan_up(plan, lvM, st);
  scan_down(plan, lvM, st);
  a.nblk = lvM[plan.levels];
  hipLaunchKernelGGL(sst_blocks, dim3(blocks(n, kScanThreads)), tb, 0, st, a);
  const ScanPlan bplan(bmax);
  std::uint64_t* lvI[kScanLevels + 1];
  bplan.place(a.ioff, sums_b, lvI);  // (the W levels are done with; bmax <= n)
  hipLaunchKernelGGL(sst_index_sizes, dim3(static_cast<unsigned>(bplan.m[1])), tb, 0, st, a, lvI[1]);
  scan_up(bplan, lvI, st);
  scan_down(bplan, lvI, st);
  hipLaunchKernelGGL(sst_publish, dim3(1), dim3(64), 0, st, a, lvI[bplan.levels], s.d_hres);
  clock.mark(2);
  if (int rc = s.wait(st, 7, 2, "SSTable build: the cut left no result")) return rc;
  const std::uint64_t fsize = s.h_res[0], B = s.h_res[1], ioff = s.h_res[2], isz = s.h_res[3];
  if (B == 0 || B > bmax) return set_error(TKV_IO_ERROR, "SSTable build: the cut is inconsistent");
  if (s.h_res[4] & kFlagBlock) return set_error(TKV_INVALID_ARGUMENT, "SSTable build: a data block does not fit u32");
  if (fsize > 0xFFFFFFFFull) return set_error(TKV_INVALID_ARGUMENT, "SSTable build: the file does not fit u32");
  *c.file_size = fsize;
  *c.n_blocks = B;
  *c.index_offset = ioff;
  *c.index_size = isz;
  const bool want_blocks = a.o_off || a.o_size || a.o_first;
  if (fsize > c.cap || (want_blocks && B > c.block_cap))
    return set_error(TKV_BUFFER_OVERFLOW, "SSTable build: the file or the block arrays do not fit");
  if (!a.file) return set_error(TKV_INVALID_ARGUMENT, "null pointer");

  // layout and emit
  a.B = B;
  a.index_offset = ioff;
  a.index_size = isz;
  a.ntiles = (ioff + kSstTile - 1u) / kSstTile;
  if (int rc = s.tile.take(4u * a.ntiles, &a.tile)) return rc;
  hipLaunchKernelGGL(sst_positions, dim3(blocks(n, kScanThreads)), tb, 0, st, a);
  hipLaunchKernelGGL(sst_tiles, dim3(blocks(a.ntiles, kScanThreads)), tb, 0, st, a);
  const std::uint64_t want = (a.ntiles + kSstWaves - 1u) / kSstWaves;
  const unsigned grid = static_cast<unsigned>(std::min<std::uint64_t>(want, 2u * std::max(1, s.ncu)));
  a.nwaves = grid * kSstWaves;
  hipLaunchKernelGGL(sst_emit, dim3(grid), dim3(kSstThreads), 0, st, a);
  hipLaunchKernelGGL(sst_index, dim3(static_cast<unsigned>(std::min<std::uint64_t>((B + 3u) / 4u, 1u << 16))), dim3(256), 0, st, a);
  if (want_blocks) hipLaunchKernelGGL(sst_out, dim3(blocks(B, kScanThreads)), tb, 0, st, a);
  TKV_HIP_RC(hipGetLastError());
  clock.mark(3);
  // stamp: every CRC field is zero, so an image's plain CRC is its stamp
  if (int rc = batch_device_impl(kAlgoCrc32, a.file, a.boff, a.bsize, nullptr, a.bcrc, B + 1u, st)) return rc;
  hipLaunchKernelGGL(sst_stamp, dim3(blocks(B + 1u, kScanThreads)), tb, 0, st, a);
  TKV_HIP_RC(hipGetLastError());
  clock.mark(4);
  TKV_HIP_RC(hipStreamSynchronize(st));
  clock.finish();
  g_sst.last[0] = B;
  g_sst.last[1] = rounds;
  g_sst.last[2] = a.nwaves;
  g_sst.last[3] = fsize;
  return TKV_OK;
}

}  // namespace

int sst_build_device_impl(const SstBuildCall& c, hipStream_t st) {
  g_sst.begin();
  if (!device_tables(kAlgoCrc32)) return TKV_IO_ERROR;
  SstScratch* sp = nullptr;
  if (int rc = per_device_scratch(&sp, kSstHres, 1, false)) return rc;
  SstArgs a{};
  a.keys = c.keys;
  a.key_off = c.key_off;
  a.key_len = c.key_len;
  a.vals = c.vals;
  a.val_off = c.val_off;
  a.val_len = c.val_len;
  a.n = c.n;
  a.T = c.target_block_size;
  a.file = c.file;
  a.o_off = c.block_off;
  a.o_size = c.block_size;
  a.o_first = c.block_first;
  std::lock_guard<std::mutex> lk(sp->mu);
  return build_locked(*sp, a, c, st);
}

}  // namespace tkv

extern "C" {

void tkv_debug_sst_build_geometry(uint64_t out[4]) {
  out[0] = tkv::kSstTile;
  out[1] = tkv::kScanBlock;
  out[2] = 0;  // the partition composes no chunk first: plain doubling over the entries
  out[3] = 0;
}

void tkv_debug_sst_build_last(uint64_t out[4]) { tkv::g_sst.get_last(out); }

int tkv_debug_sst_build_phases(int enable, double out_ms[4]) { return tkv::g_sst.phases(enable, out_ms); }

}  // extern "C"
