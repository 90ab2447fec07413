// WAL group-commit encode on the device: wal_entry::encode
// (/root/reference/src/engine/wal.cpp:19-61) for a whole put batch held as key / value arenas with
// per-record offsets and lengths. Record i is
//   u32 record_len | u32 crc32 | u8 op | u64 seq | u8 tombstone | u32 key_len | u32 val_len | key | value
// (little-endian, packed), record_len = 18 + key_len + val_len, crc32 = CRC-32 of bytes [8, 8 + record_len),
// and the records lie back to back in batch order.
//
// enc_scan / scan_level / scan_add (the levels: tkv_scan.h): record sizes and their u64 exclusive prefix scan over n, kScanBlock records per
// workgroup (DPP prefix per wave, wave totals through LDS), the block sums scanned by the next level,
// up to kScanLevels levels. The host reads {total, overflow flag, long records} from a pinned block
// and decides overflow / invalid before anything is written for the caller.
// enc_finish: the final offsets, the caller's rec_off, for every emit tile the record that holds its
// first byte and the last record that starts in it (so no emit wave searches the offsets) and the list
// of records stamped by read-back.
// enc_emit: the image cut into tiles of kEncTile bytes, tile t, t + W, ... to wave t of W. A tile's record
// range is read two tiles ahead and its first 64 records' inputs one tile ahead. One wave builds its tile in an LDS window:
// headers and short keys / values one record per lane, long spans by the whole wave 16 bytes per lane
// (two source granules and v_alignbyte take the source / destination misalignment out), then folds
// the CRC of every record of record_len <= kLaneFold from the window (fold_raw, the sweep's lane
// fold), writes it into the window and stores the tile with coalesced 16-byte stores; the granules it
// shares with a neighbouring tile or with bytes outside the image go out bytewise, nothing is read
// back. The window reaches kEncOver bytes past the tile and kEncPre in front of it, so such a record
// lies wholly in the window of every tile that holds a byte of its CRC field, wherever it starts.
// Longer records are copied piecewise by the tiles they cross with a zero CRC field; one CRC batch
// over the written image (batch_device_impl) and enc_stamp fill their fields afterwards, in stream
// order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <mutex>

#include "tkv_crc32.h"
#include "tkv_crc32_device.h"
#include "tkv_device_util.h"
#include "tkv_engine.h"
#include "tkv_scan.h"
#include "tkv_wal_copy.h"
#include "tkv_wal_fold.h"
#include "tkv_wal_layout.h"

namespace tkv {
namespace {

constexpr std::uint32_t kEncTile = 4096;      // image bytes per emit tile
constexpr std::uint32_t kEncPre = 16;         // window bytes in front of the tile's 16-byte granule
constexpr std::uint32_t kEncOver = 288;       // window bytes past the tile
constexpr std::uint32_t kEncWin = kEncPre + 16 + kEncTile + kEncOver;
constexpr unsigned kEncWaves = 16;            // waves per workgroup: the 64 KiB tables + 16 windows of LDS
constexpr unsigned kEncThreads = 64 * kEncWaves;
constexpr unsigned kEncHres = 4;              // words of the pinned result block
enum : int { kCntFlag = 0, kCntLong, kCntCursor, kCntWords = 4 };
// a folded record that starts in the tile's last byte ends, and fold_raw's frozen steps read, inside the window
static_assert(kEncPre + 15 + kEncTile - 1 + 8 + kLaneFold + 12 <= kEncWin, "window");
static_assert(kEncPre >= 8 + 8, "a record whose CRC field reaches into the tile starts in the window, fold_raw's s >= 8");
static_assert(kEncTile % 16 == 0 && kEncWin % 16 == 0, "16-byte granules");
static_assert(kLdsSliceWords * 2 + kEncWaves * kEncWin + 4 * (kLaneFold + 1) <= 163840, "LDS");

struct EncArgs {
  const std::uint8_t* keys;
  const std::uint64_t* key_off;
  const std::uint32_t* key_len;
  const std::uint8_t* vals;
  const std::uint64_t* val_off;
  const std::uint32_t* val_len;  // nullable: every value empty
  const std::uint8_t* op;        // nullable: 0
  const std::uint8_t* tomb;      // nullable: 0
  const std::uint64_t* seq;      // nullable: first_seq + i
  std::uint64_t first_seq;
  std::uint64_t n;
  std::uint8_t* img;
  std::uint64_t total;
  std::uint64_t* off;            // scratch: record start offsets
  std::uint64_t* rec_off;        // nullable: the caller's copy
  std::uint32_t* crc;            // nullable: the caller's stamped CRCs
  std::uint32_t* tile_first;     // per tile, two words: the record that holds its first byte, the last one that starts in it
  std::uint64_t ntiles;
  std::uint64_t* l_off;          // records stamped by read-back: offset of byte 8, record_len, index, CRC
  std::uint32_t* l_len;
  std::uint32_t* l_idx;
  std::uint32_t* l_crc;
  unsigned long long* cnt;       // kCntWords device words
  std::uint32_t fused;
  std::uint32_t nwaves;
  const DeviceTables* tabs;
};

// ---- size scan --------------------------------------------------------------------------------------

__device__ __forceinline__ std::uint64_t rec_len64(const EncArgs& a, std::uint64_t i) {
  return 18ull + a.key_len[i] + (a.val_len ? a.val_len[i] : 0u);
}

// Level 0 of the size scan (scan_items): the entries are the record sizes (their exclusive prefix within
// the block to a.off), with the u32 overflow flag and the count of records the emit pass does not stamp.
__global__ __launch_bounds__(kScanThreads) void enc_scan(EncArgs a, std::uint64_t* bsum) {
  const std::uint64_t i0 = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
  std::uint64_t v[kScanItems];
  std::uint32_t nlong = 0, bad = 0;
#pragma unroll
  for (unsigned k = 0; k < kScanItems; ++k) {
    const std::uint64_t i = i0 + k;
    v[k] = 0;
    if (i < a.n) {
      const std::uint64_t rl = rec_len64(a, i);
      v[k] = rl + kWalPayload;
      bad |= rl > 0xFFFFFFFFull ? 1u : 0u;
      nlong += (rl > kLaneFold || !a.fused) ? 1u : 0u;
    }
  }
  scan_items(v, i0, a.n, a.off, bsum);
  if (bad) atomicOr(&a.cnt[kCntFlag], 1ull);
  if (nlong) atomicAdd(&a.cnt[kCntLong], static_cast<unsigned long long>(nlong));
}

__global__ void enc_publish(const std::uint64_t* top, const unsigned long long* cnt, std::uint64_t* h) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    h[0] = *top;
    h[1] = cnt[kCntFlag];
    h[2] = cnt[kCntLong];
    h[3] = 1;
  }
}

__global__ __launch_bounds__(kScanThreads) void enc_finish(EncArgs a, const std::uint64_t* base) {
  const std::uint64_t i = blockIdx.x * static_cast<std::uint64_t>(kScanThreads) + threadIdx.x;
  if (i >= a.n) return;
  const std::uint64_t o = a.off[i] + (base ? base[i / kScanBlock] : 0u);
  a.off[i] = o;
  if (a.rec_off) a.rec_off[i] = o;
  const std::uint64_t rl = rec_len64(a, i);
  const std::uint64_t e = o + rl + kWalPayload;
  for (std::uint64_t t = o / kEncTile; t * kEncTile < e; ++t) {  // one writer per word: records tile the image
    if (o <= t * kEncTile) a.tile_first[2u * t] = static_cast<std::uint32_t>(i);
    if (e >= (t + 1u) * kEncTile || i + 1u == a.n) a.tile_first[2u * t + 1u] = static_cast<std::uint32_t>(i);
  }
  if (rl > kLaneFold || !a.fused) {
    const unsigned long long k = atomicAdd(&a.cnt[kCntCursor], 1ull);
    a.l_off[k] = o + kWalPayload;
    a.l_len[k] = static_cast<std::uint32_t>(rl);
    a.l_idx[k] = static_cast<std::uint32_t>(i);
  }
}

__global__ __launch_bounds__(kScanThreads) void enc_stamp(EncArgs a, std::uint64_t nlong) {
  const std::uint64_t k = blockIdx.x * static_cast<std::uint64_t>(kScanThreads) + threadIdx.x;
  if (k >= nlong) return;
  const std::uint32_t c = a.l_crc[k];
  std::uint8_t* p = a.img + (a.l_off[k] - (kWalPayload - kWalCrc));
  p[0] = static_cast<std::uint8_t>(c);
  p[1] = static_cast<std::uint8_t>(c >> 8);
  p[2] = static_cast<std::uint8_t>(c >> 16);
  p[3] = static_cast<std::uint8_t>(c >> 24);
  if (a.crc) a.crc[a.l_idx[k]] = c;
}

// ---- emit -------------------------------------------------------------------------------------------

// A span lies in the window: at most kWaveSteps steps of wave_copy.
constexpr std::uint32_t kWaveSteps = (kEncWin + 1023u) / 1024u;

// A record's inputs as the emit pass reads them, one record per lane.
struct Rec {
  std::uint64_t ro, seq, ko, vo;
  std::uint32_t kl, vl, op, tomb;
};
__device__ __forceinline__ Rec load_rec(const EncArgs& a, std::uint64_t i, bool act) {
  Rec r{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (act) {
    r.ro = a.off[i];
    r.kl = a.key_len[i];
    r.ko = a.key_off[i];
    if (a.val_len) {
      r.vl = a.val_len[i];
      r.vo = a.val_off[i];
    }
    r.op = a.op ? a.op[i] : 0u;
    r.tomb = a.tomb ? (a.tomb[i] ? 1u : 0u) : 0u;
    r.seq = a.seq ? a.seq[i] : a.first_seq + i;
  }
  return r;
}
// The records of tile t: [x, y] (enc_finish).
__device__ __forceinline__ uint2 tile_head(const EncArgs& a, std::uint64_t t) {
  return *reinterpret_cast<const uint2*>(a.tile_first + 2u * t);
}

// One tile. head and r0 (the tile's first 64 records, one per lane) were loaded a tile ahead.
__device__ __forceinline__ void emit_tile(const EncArgs& a, std::uint8_t* win, const std::uint32_t* tab, const std::uint32_t* inj,
                                          const dev::LaneConstX& kc, std::uint64_t t, uint2 head, const Rec& r0,
                                          std::uint32_t lane) {
  const std::uint64_t ts = t * kEncTile;
  const std::uint64_t te = ts + kEncTile < a.total ? ts + kEncTile : a.total;
  const std::uint64_t first = head.x, last = head.y;
  std::uint8_t* const dst = a.img + ts;
  const std::uint32_t o = static_cast<std::uint32_t>(reinterpret_cast<std::uintptr_t>(dst) & 15u);
  const std::uint32_t wb = kEncPre + o;  // window offset of image byte ts: window granules are the image's
  for (std::uint64_t rb = first; rb <= last; rb += 64u) {
    const std::uint64_t i = rb + lane;
    const bool act = i <= last;
    const Rec r = rb == first ? r0 : load_rec(a, i, act);
    const std::uint64_t ro = act ? r.ro : ts, seq = r.seq, ko = r.ko, vo = r.vo;
    const std::uint32_t kl = r.kl, vl = r.vl, op = r.op, tomb = r.tomb;
    const std::uint32_t rl = 18u + kl + vl;  // fits: the host checked the scan's flag
    const std::uint64_t size = static_cast<std::uint64_t>(rl) + kWalPayload;
    // folded here: short, and a byte of its CRC field lies in the tile (it starts before te)
    const bool fold = act && a.fused && rl <= kLaneFold && ro + kWalPayload > ts;
    const std::uint64_t clo = fold ? ro : (ro > ts ? ro : ts);
    const std::uint64_t chi = fold ? ro + size : (ro + size < te ? ro + size : te);
    // window offset of the record's byte 0 (meaningful when a header byte is laid out)
    const std::uint32_t hw = wb + static_cast<std::uint32_t>(static_cast<std::int32_t>(static_cast<std::int64_t>(ro - ts)));
    if (act) {
      const std::uint32_t hb0 = clo > ro ? static_cast<std::uint32_t>(clo - ro < kWalMeta ? clo - ro : kWalMeta) : 0u;
      const std::uint32_t hb1 = static_cast<std::uint32_t>(chi - ro < kWalMeta ? chi - ro : kWalMeta);
      if (hb0 < hb1) {
        const std::uint32_t h[7] = {rl,
                                    0u,
                                    op | (static_cast<std::uint32_t>(seq) << 8),
                                    static_cast<std::uint32_t>(seq >> 24),
                                    static_cast<std::uint32_t>(seq >> 56) | (tomb << 8) | (kl << 16),
                                    (kl >> 16) | (vl << 16),
                                    vl >> 16};
#pragma unroll
        for (std::uint32_t b = 0; b < kWalMeta; ++b)
          if (b >= hb0 && b < hb1) win[hw + b] = static_cast<std::uint8_t>(h[b >> 2] >> (8u * (b & 3u)));
      }
    }
    Span ks{0u, 0u, 0}, vs{0u, 0u, 0};
    if (act) {
      ks = clip_span(reinterpret_cast<std::uintptr_t>(a.keys) + ko, kl, ro + kWalMeta, clo, chi, ts, wb);
      if (vl) vs = clip_span(reinterpret_cast<std::uintptr_t>(a.vals) + vo, vl, ro + kWalMeta + kl, clo, chi, ts, wb);
    }
    lane_copy2(win, lane_span(ks.d, ks.src, ks.len, ks.len != 0u && ks.len <= kShortSpan),
               lane_span(vs.d, vs.src, vs.len, vs.len != 0u && vs.len <= kShortSpan));
    wave_spans<kWaveSteps>(win, ks, lane);
    wave_spans<kWaveSteps>(win, vs, lane);
    wave_sync();
    // the lane fold (fold_raw plus the initial register's term), its CRC into the window's field
    const std::uint32_t L = fold ? rl : 0u;
    const std::uint32_t c = fold_raw(win, tab, kc, fold ? hw + kWalPayload : kEncPre, L) ^ inj[L] ^ 0xFFFFFFFFu;
    if (fold) {
#pragma unroll
      for (std::uint32_t b = 0; b < 4u; ++b) win[hw + kWalCrc + b] = static_cast<std::uint8_t>(c >> (8u * b));
      if (ro >= ts && a.crc) a.crc[i] = c;
    }
  }
  wave_sync();
  // the tile out of the window: whole granules with 16-byte stores, the (at most two) granules shared
  // with a neighbour or with bytes outside the image bytewise
  const std::uint32_t len = static_cast<std::uint32_t>(te - ts);
  store_tile(win + kEncPre, dst, o, len, lane);
  wave_sync();
}

__global__ __launch_bounds__(kEncThreads) void enc_emit(EncArgs a) {
  // one block with the tables at LDS address 0, so a lookup's v_perm result is its address
  __shared__ __attribute__((aligned(16))) std::uint8_t lds[kLdsSliceWords * 2 + kEncWaves * kEncWin + 4 * (kLaneFold + 1)];
  std::uint32_t* tab = reinterpret_cast<std::uint32_t*>(lds);
  std::uint32_t* inj = reinterpret_cast<std::uint32_t*>(lds + kLdsSliceWords * 2 + kEncWaves * kEncWin);  // Shift_L(0xFFFFFFFF)
  dev::fill_lds_slicing16(a.tabs, tab);
  for (std::uint32_t i = threadIdx.x; i <= kLaneFold; i += blockDim.x) inj[i] = a.tabs->init_shift[i];
  __syncthreads();
  const std::uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const std::uint32_t lane = threadIdx.x & 63u;
  std::uint8_t* win = lds + kLdsSliceWords * 2 + wv * kEncWin;
  const dev::LaneConstX kc = dev::lane_const16(lane);
  // a tile's first and last record are read two tiles ahead and its first 64 records one tile ahead, so
  // their latency lies under the tile in front
  std::uint64_t t = blockIdx.x * kEncWaves + wv;
  if (t >= a.ntiles) return;
  uint2 h = tile_head(a, t);
  Rec r0 = load_rec(a, h.x + lane, h.x + lane <= h.y);
  uint2 hn = t + a.nwaves < a.ntiles ? tile_head(a, t + a.nwaves) : make_uint2(1u, 0u);
  for (; t < a.ntiles; t += a.nwaves) {
    const Rec rn = load_rec(a, static_cast<std::uint64_t>(hn.x) + lane, static_cast<std::uint64_t>(hn.x) + lane <= hn.y);
    const uint2 hnn = t + 2ull * a.nwaves < a.ntiles ? tile_head(a, t + 2ull * a.nwaves) : make_uint2(1u, 0u);
    emit_tile(a, win, tab, inj, kc, t, h, r0, lane);
    h = hn;
    r0 = rn;
    hn = hnn;
  }
}

// ---- host side --------------------------------------------------------------------------------------

// An entry of the read-back list, for its size alone: the list is four arrays of lng.cap entries each.
struct LongRec {
  std::uint32_t off[2], len, idx, crc;
};

// Per-device scratch, grown by doubling and kept between calls (guarded by mu).
struct EncScratch : ScratchBase {
  DeviceBuf off;    // record offsets (u64)
  DeviceBuf sums;   // block sums of every scan level (u64)
  DeviceBuf tiles;  // first and last record of every tile (2 x u32)
  DeviceBuf lng;    // read-back list: off (u64), len, idx, crc (u32)
  unsigned long long*& cnt = words;
};

std::atomic<int> g_enc_fused{1};
// What the calling thread's last device encode did (tkv_debug_wal_encode_last).
thread_local std::uint64_t g_enc_last[4] = {0, 0, 0, 0};

int encode_locked(EncScratch& s, EncArgs a, const WalEncodeCall& c, hipStream_t st) {
  const ScanPlan plan(a.n);
  const int levels = plan.levels;
  std::uint64_t* sums = nullptr;
  if (int rc = s.off.take(a.n, &a.off)) return rc;
  if (int rc = s.sums.take(plan.nsum, &sums)) return rc;
  a.cnt = s.cnt;
  std::uint64_t* lv[kScanLevels + 1];
  plan.place(a.off, sums, lv);
  TKV_HIP_RC(hipMemsetAsync(s.cnt, 0, kCntWords * sizeof(unsigned long long), st));
  s.h_res[3] = 0;
  hipLaunchKernelGGL(enc_scan, dim3(static_cast<unsigned>(plan.m[1])), dim3(kScanThreads), 0, st, a, lv[1]);
  scan_up(plan, lv, st);
  hipLaunchKernelGGL(enc_publish, dim3(1), dim3(64), 0, st, lv[levels], s.cnt, s.d_hres);
  if (int rc = s.wait(st, 3, 1, "WAL encode: the size scan left no result")) return rc;
  const std::uint64_t total = s.h_res[0], nlong = s.h_res[2];
  if (s.h_res[1]) return set_error(TKV_INVALID_ARGUMENT, "WAL encode: 18 + key_len + val_len does not fit u32");
  *c.img_size = total;
  if (total > c.cap) return set_error(TKV_BUFFER_OVERFLOW, "WAL encode: the image does not fit cap");
  if (!a.img) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  a.total = total;
  a.ntiles = (total + kEncTile - 1u) / kEncTile;
  LongRec* lng = nullptr;
  if (int rc = s.tiles.take(2u * a.ntiles, &a.tile_first)) return rc;
  if (int rc = s.lng.take(nlong, &lng)) return rc;
  a.l_off = reinterpret_cast<std::uint64_t*>(lng);
  a.l_len = reinterpret_cast<std::uint32_t*>(a.l_off + s.lng.cap);
  a.l_idx = a.l_len + s.lng.cap;
  a.l_crc = a.l_idx + s.lng.cap;
  scan_down(plan, lv, st, 1);  // (enc_finish adds lv[1] itself)
  hipLaunchKernelGGL(enc_finish, dim3(blocks(a.n, kScanThreads)), dim3(kScanThreads), 0, st, a,
                     levels > 1 ? lv[1] : static_cast<const std::uint64_t*>(nullptr));
  const std::uint64_t want = (a.ntiles + kEncWaves - 1u) / kEncWaves;
  const unsigned grid = static_cast<unsigned>(std::min<std::uint64_t>(want, std::max(1, s.ncu)));
  a.nwaves = grid * kEncWaves;
  hipLaunchKernelGGL(enc_emit, dim3(grid), dim3(kEncThreads), 0, st, a);
  TKV_HIP_RC(hipGetLastError());
  if (nlong) {
    if (int rc = batch_device_impl(kAlgoCrc32, a.img, a.l_off, a.l_len, nullptr, a.l_crc, nlong, st)) return rc;
    hipLaunchKernelGGL(enc_stamp, dim3(blocks(nlong, kScanThreads)), dim3(kScanThreads), 0, st, a, nlong);
    TKV_HIP_RC(hipGetLastError());
  }
  TKV_HIP_RC(hipStreamSynchronize(st));
  g_enc_last[0] = a.n - nlong;
  g_enc_last[1] = nlong;
  g_enc_last[2] = a.nwaves;
  g_enc_last[3] = total;
  return TKV_OK;
}

}  // namespace

int wal_encode_device_impl(const WalEncodeCall& c, hipStream_t st) {
  for (auto& v : g_enc_last) v = 0;
  const DeviceTables* tabs = device_tables(kAlgoCrc32);
  if (!tabs) return TKV_IO_ERROR;
  EncScratch* sp = nullptr;
  if (int rc = per_device_scratch(&sp, kEncHres, kCntWords, false)) return rc;
  EncArgs a{};
  a.keys = c.keys;
  a.key_off = c.key_off;
  a.key_len = c.key_len;
  a.vals = c.vals;
  a.val_off = c.val_off;
  a.val_len = c.val_len;
  a.op = c.op;
  a.tomb = c.tomb;
  a.seq = c.seq;
  a.first_seq = c.first_seq;
  a.n = c.n;
  a.img = c.img;
  a.rec_off = c.rec_off;
  a.crc = c.crc;
  a.fused = g_enc_fused.load() ? 1u : 0u;
  a.tabs = tabs;
  std::lock_guard<std::mutex> lk(sp->mu);
  return encode_locked(*sp, a, c, st);
}

}  // namespace tkv

extern "C" {

void tkv_debug_wal_encode_geometry(uint64_t out[4]) {
  out[0] = tkv::kEncTile;
  out[1] = tkv::kScanBlock;
  out[2] = tkv::kLaneFold;
  out[3] = tkv::kScanLevels;
}

void tkv_debug_wal_encode_last(uint64_t out[4]) {
  for (int i = 0; i < 4; ++i) out[i] = tkv::g_enc_last[i];
}

int tkv_debug_set_wal_encode_fused(int enable) { return tkv::g_enc_fused.exchange(enable ? 1 : 0); }

}  // extern "C"
