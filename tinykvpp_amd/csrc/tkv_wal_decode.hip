// Batched WAL decode on the device (tkv_wal_decode_device, include/tkv_crc32.h): the fields
// wal_entry::decode (the reference's src/engine/wal.cpp:98-127) takes out of a record, for n records of
// an image in HBM whose start offsets are known (tkv_wal_index_device's list), as the columns and key /
// value arenas tkv_wal_encode_device takes. No checksum is computed here: that is tkv_wal_index's and
// tkv_wal_check_records_device's work.
//
// Header pass (load_header, parse_header): one lane per record loads the (at most three) 16-byte granules
// that hold the record's 26 header bytes, realigns them in registers (lane_dwords_n: two selects and
// v_alignbyte) and runs wal_entry::decode's structural checks in 64-bit arithmetic. It runs twice.
// dec_scan: the header pass as level 0 of two u64 exclusive scans over n, keys and values, in one launch
// (scan_items; the levels above and their plan are tkv_scan.h's, as for the encoder), and the
// atomic minimum of the failing indices. The host reads {keys total, values total, first bad} from a
// pinned block and decides corrupted / overflow before anything is written for the caller.
// dec_finish: the header pass again: the fixed-width columns, the final arena offsets, and per copied
// arena and output tile the record whose span holds the tile's first byte and the record whose span holds
// its last byte, so no emit wave searches the offsets. Empty spans hold no byte: they write no table
// entry, so a run of them of any length in front of, behind or across a tile edge is skipped.
// span_emit (tkv_wal_emit.h, shared with the SSTable scan), per copied arena: the arena cut into tiles of
// kDecTile bytes, tile t, t + W, ... to wave t of W. A wave builds its tile in an LDS window and stores it
// once. WalSrc tells it where a record's key or value lies. The kernel needs no CRC tables: its LDS is
// the windows alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>

#include "tkv_crc32.h"
#include "tkv_crc32_device.h"
#include "tkv_device_util.h"
#include "tkv_engine.h"
#include "tkv_scan.h"
#include "tkv_wal_copy.h"
#include "tkv_wal_emit.h"
#include "tkv_wal_layout.h"

namespace tkv {
namespace {

constexpr unsigned kDecHres = 4;                     // words of the pinned result block

struct DecArgs {
  const std::uint8_t* img;
  std::uint64_t size;
  const std::uint64_t* off64;  // exactly one of off64 / off32
  const std::uint32_t* off32;
  std::uint64_t n;
  std::uint32_t key_views, val_views;
  std::uint8_t* op;            // the columns, each nullable
  std::uint8_t* tomb;
  std::uint64_t* seq;
  std::uint64_t* key_off;
  std::uint32_t* key_len;
  std::uint64_t* val_off;
  std::uint32_t* val_len;
  std::uint64_t ktotal, vtotal;
  std::uint64_t* kpre;         // scratch, n + 1 entries: arena offset of every key, then the total
  std::uint64_t* vpre;         // the same for the values
  std::uint32_t* ktile;        // per tile of a copied arena, two words: first and last record with a byte in it
  std::uint32_t* vtile;
  unsigned long long* first_bad;
};

__device__ __forceinline__ std::uint64_t rec_off(const DecArgs& a, std::uint64_t i) {
  return a.off64 ? a.off64[i] : static_cast<std::uint64_t>(a.off32[i]);
}

// ---- header pass ------------------------------------------------------------------------------------

struct Hdr {
  std::uint32_t kl, vl, op, tomb;
  std::uint64_t seq;
  bool ok;
};

// The granules that hold the 26 header bytes of the record at image offset off (two, or three when the
// header starts past byte 6 of its first granule), loaded without a branch: a granule that holds no
// header byte reads the first one again, and a record with fewer than 26 bytes left (never parsed) reads
// the image's first granule. The host has checked that the image holds at least 26 bytes.
struct HdrRaw {
  uint4 g[3];
  std::uint32_t o;       // the header's byte offset in its first granule
  std::uint64_t left;    // image bytes from off on (0 for a record that is not live)
};
__device__ __forceinline__ HdrRaw load_header(const DecArgs& a, std::uint64_t off, bool live) {
  HdrRaw r;
  r.left = live && off < a.size ? a.size - off : 0u;
  const bool fits = r.left >= kWalMeta;
  const std::uintptr_t p = reinterpret_cast<std::uintptr_t>(a.img) + static_cast<std::uintptr_t>(fits ? off : 0u);
  const std::uintptr_t al = p & ~static_cast<std::uintptr_t>(15);
  r.o = static_cast<std::uint32_t>(p & 15u);
  r.g[0] = dev::gload16(al);
  r.g[1] = dev::gload16(fits ? al + 16u : al);
  r.g[2] = dev::gload16(fits && r.o + kWalMeta > 32u ? al + 32u : al);
  return r;
}

// The header's fields and wal_entry::decode's structural checks: at least 26 bytes left (wal.cpp:68),
// record_len + 8 within the image (:83), key and value inside the payload (:118-121). The granules are
// realigned in registers (lane_dwords_n: two selects by the start's dword in its granule, then
// v_alignbyte).
__device__ __forceinline__ Hdr parse_header(const HdrRaw& r) {
  Hdr h{0u, 0u, 0u, 0u, 0u, false};
  uint4 g[3] = {r.g[0], r.g[1], r.o + kWalMeta > 32u ? r.g[2] : make_uint4(0u, 0u, 0u, 0u)};
  std::uint32_t d[12];
  dev::lane_dwords_n<1, 3>(g, r.o, d);
  const std::uint32_t rlen = d[0];
  h.op = d[kWalOp / 4] & 0xFFu;
  h.seq = (static_cast<std::uint64_t>(__builtin_amdgcn_alignbyte(d[4], d[3], kWalSeq % 4)) << 32) |
          __builtin_amdgcn_alignbyte(d[3], d[2], kWalSeq % 4);
  h.tomb = (d[kWalTomb / 4] >> (8u * (kWalTomb % 4))) & 0xFFu;
  h.kl = __builtin_amdgcn_alignbyte(d[kWalKeyLen / 4 + 1], d[kWalKeyLen / 4], kWalKeyLen % 4);
  h.vl = __builtin_amdgcn_alignbyte(d[kWalValLen / 4 + 1], d[kWalValLen / 4], kWalValLen % 4);
  h.ok = r.left >= kWalMeta && static_cast<std::uint64_t>(rlen) + kWalPayload <= r.left &&
         static_cast<std::uint64_t>(h.kl) + h.vl + (kWalMeta - kWalPayload) <= rlen;
  return h;
}

__global__ void dec_init(unsigned long long* first_bad, std::uint64_t n) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *first_bad = n;
}

// Level 0 of both scans: the key and value lengths of the records that pass (0 for one that fails: its
// lengths are never used), their exclusive prefixes within the block to a.kpre / a.vpre. The headers
// are read lane-strided (consecutive lanes read consecutive records, whose granules share cache lines),
// the four records' loads of a thread issued together; the lengths go through LDS to the thread that
// scans them (scan_items takes consecutive entries).
__global__ __launch_bounds__(kScanThreads) void dec_scan(DecArgs a, std::uint64_t* kbsum, std::uint64_t* vbsum) {
  __shared__ __attribute__((aligned(16))) std::uint32_t lk[kScanBlock], lv[kScanBlock];
  const std::uint64_t b0 = blockIdx.x * kScanBlock;
  std::uint64_t off[kScanItems];
#pragma unroll
  for (unsigned k = 0; k < kScanItems; ++k) {
    const std::uint64_t i = b0 + k * kScanThreads + threadIdx.x;
    off[k] = rec_off(a, i < a.n ? i : a.n - 1u);  // (clamped: every load stays inside the array)
  }
  HdrRaw raw[kScanItems];
#pragma unroll
  for (unsigned k = 0; k < kScanItems; ++k) raw[k] = load_header(a, off[k], b0 + k * kScanThreads + threadIdx.x < a.n);
  std::uint64_t bad = ~0ull;
#pragma unroll
  for (unsigned k = 0; k < kScanItems; ++k) {
    const std::uint64_t i = b0 + k * kScanThreads + threadIdx.x;
    const Hdr h = parse_header(raw[k]);
    lk[k * kScanThreads + threadIdx.x] = h.ok ? h.kl : 0u;
    lv[k * kScanThreads + threadIdx.x] = h.ok ? h.vl : 0u;
    if (i < a.n && !h.ok) bad = bad < i ? bad : i;
  }
  __syncthreads();
  const std::uint64_t i0 = b0 + threadIdx.x * kScanItems;
  const uint4 k4 = *reinterpret_cast<const uint4*>(lk + threadIdx.x * kScanItems);
  const uint4 v4 = *reinterpret_cast<const uint4*>(lv + threadIdx.x * kScanItems);
  static_assert(kScanItems == 4, "one uint4 of lengths per thread");
  const std::uint64_t kv[kScanItems] = {k4.x, k4.y, k4.z, k4.w}, vv[kScanItems] = {v4.x, v4.y, v4.z, v4.w};
  scan_items(kv, i0, a.n, a.kpre, kbsum);
  __syncthreads();  // block_prefix's LDS words are used again
  scan_items(vv, i0, a.n, a.vpre, vbsum);
  if (bad != ~0ull) atomicMin(a.first_bad, static_cast<unsigned long long>(bad));
}

__global__ void dec_publish(const std::uint64_t* ktop, const std::uint64_t* vtop, const unsigned long long* first_bad,
                            std::uint64_t* h) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    h[0] = *ktop;
    h[1] = *vtop;
    h[2] = *first_bad;
    h[3] = 1;
  }
}

__global__ __launch_bounds__(kScanThreads) void dec_finish(DecArgs a, const std::uint64_t* kbase, const std::uint64_t* vbase) {
  const std::uint64_t i = blockIdx.x * static_cast<std::uint64_t>(kScanThreads) + threadIdx.x;
  if (i >= a.n) return;
  const std::uint64_t off = rec_off(a, i);
  const Hdr h = parse_header(load_header(a, off, true));  // (every record passed in dec_scan)
  const std::uint64_t ko = a.kpre[i] + (kbase ? kbase[i / kScanBlock] : 0u);
  const std::uint64_t vo = a.vpre[i] + (vbase ? vbase[i / kScanBlock] : 0u);
  a.kpre[i] = ko;
  a.vpre[i] = vo;
  if (i + 1u == a.n) {
    a.kpre[a.n] = a.ktotal;
    a.vpre[a.n] = a.vtotal;
  }
  if (a.op) a.op[i] = static_cast<std::uint8_t>(h.op);
  if (a.tomb) a.tomb[i] = static_cast<std::uint8_t>(h.tomb);
  if (a.seq) a.seq[i] = h.seq;
  if (a.key_len) a.key_len[i] = h.kl;
  if (a.val_len) a.val_len[i] = h.vl;
  if (a.key_off) a.key_off[i] = a.key_views ? off + kWalMeta : ko;
  if (a.val_off) a.val_off[i] = a.val_views ? off + kWalMeta + h.kl : vo;
  if (!a.key_views && h.kl) tile_entries(a.ktile, i, ko, h.kl, a.ktotal);
  if (!a.val_views && h.vl) tile_entries(a.vtile, i, vo, h.vl, a.vtotal);
}

// ---- emit -------------------------------------------------------------------------------------------

// Where record i's span lies in the image for the shared emit (tkv_wal_emit.h): the key behind the
// record's header, the value behind its key.
template <bool VAL>
struct WalSrc {
  const std::uint8_t* img;
  const std::uint64_t* off64;
  const std::uint32_t* off32;
  const std::uint64_t* kpre;   // the key spans: a value lies behind its record's key
  __device__ __forceinline__ std::uintptr_t operator()(std::uint64_t i) const {
    const std::uint64_t off = off64 ? off64[i] : static_cast<std::uint64_t>(off32[i]);
    const std::uint64_t so = off + kWalMeta + (VAL ? kpre[i + 1u] - kpre[i] : 0u);
    return reinterpret_cast<std::uintptr_t>(img) + static_cast<std::uintptr_t>(so);
  }
};

// ---- host side --------------------------------------------------------------------------------------

// Per-device scratch, grown by doubling and kept between calls (guarded by mu).
struct DecScratch : ScratchBase {
  DeviceBuf kpre;   // key arena offsets (u64, n + 1)
  DeviceBuf vpre;   // value arena offsets
  DeviceBuf sums;   // block sums of every scan level, keys then values
  DeviceBuf ktile;  // first and last record of every tile (2 x u32)
  DeviceBuf vtile;
  unsigned long long*& first_bad = words;
};

// What the calling thread's last device decode did (tkv_debug_wal_decode_last).
thread_local std::uint64_t g_dec_last[4] = {0, 0, 0, 0};

// The emit of one copied arena; returns its waves.
template <bool VAL>
std::uint32_t launch_emit(const DecScratch& s, const DecArgs& a, std::uint8_t* dst, std::uint64_t total, hipStream_t st) {
  EmitArgs<WalSrc<VAL>> e{};
  e.src = WalSrc<VAL>{a.img, a.off64, a.off32, a.kpre};
  e.pre = VAL ? a.vpre : a.kpre;
  e.dst = dst;
  e.total = total;
  e.tile = VAL ? a.vtile : a.ktile;
  e.n = a.n;
  return launch_span_emit(s.ncu, e, st);
}

int decode_locked(DecScratch& s, DecArgs a, const WalDecodeCall& c, hipStream_t st) {
  if (a.size < kWalMeta) {  // no record fits (wal.cpp:68); the header pass relies on an image of 26 bytes
    *c.first_bad = 0;
    return set_error(TKV_CORRUPTED, "WAL decode: a record fails wal_entry::decode's structural checks");
  }
  const ScanPlan plan(a.n);
  const int levels = plan.levels;
  std::uint64_t* sums = nullptr;
  if (int rc = s.kpre.take(a.n + 1u, &a.kpre)) return rc;
  if (int rc = s.vpre.take(a.n + 1u, &a.vpre)) return rc;
  if (int rc = s.sums.take(2u * plan.nsum, &sums)) return rc;
  a.first_bad = s.first_bad;
  std::uint64_t *klv[kScanLevels + 1], *vlv[kScanLevels + 1];
  plan.place(a.kpre, sums, klv);
  plan.place(a.vpre, sums + plan.nsum, vlv);
  s.h_res[3] = 0;
  hipLaunchKernelGGL(dec_init, dim3(1), dim3(64), 0, st, s.first_bad, a.n);
  hipLaunchKernelGGL(dec_scan, dim3(static_cast<unsigned>(plan.m[1])), dim3(kScanThreads), 0, st, a, klv[1], vlv[1]);
  scan_up(plan, klv, st);
  scan_up(plan, vlv, st);
  hipLaunchKernelGGL(dec_publish, dim3(1), dim3(64), 0, st, klv[levels], vlv[levels], s.first_bad, s.d_hres);
  if (int rc = s.wait(st, 3, 1, "WAL decode: the header pass left no result")) return rc;
  if (s.h_res[2] < a.n) {
    *c.first_bad = s.h_res[2];
    return set_error(TKV_CORRUPTED, "WAL decode: a record fails wal_entry::decode's structural checks");
  }
  a.ktotal = s.h_res[0];
  a.vtotal = s.h_res[1];
  *c.keys_size = a.ktotal;
  *c.vals_size = a.vtotal;
  const bool kcopy = !a.key_views && a.ktotal != 0, vcopy = !a.val_views && a.vtotal != 0;
  if ((kcopy && a.ktotal > c.keys_cap) || (vcopy && a.vtotal > c.vals_cap))
    return set_error(TKV_BUFFER_OVERFLOW, "WAL decode: an arena does not fit its cap");
  if ((kcopy && !c.keys) || (vcopy && !c.vals)) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  a.ktile = static_cast<std::uint32_t*>(s.ktile.p);  // (an arena left as views keeps an earlier call's table: not read)
  a.vtile = static_cast<std::uint32_t*>(s.vtile.p);
  if (kcopy)
    if (int rc = s.ktile.take(2u * ((a.ktotal + kDecTile - 1u) / kDecTile), &a.ktile)) return rc;
  if (vcopy)
    if (int rc = s.vtile.take(2u * ((a.vtotal + kDecTile - 1u) / kDecTile), &a.vtile)) return rc;
  scan_down(plan, klv, st, 1);  // (dec_finish adds klv[1] and vlv[1] itself)
  scan_down(plan, vlv, st, 1);
  hipLaunchKernelGGL(dec_finish, dim3(blocks(a.n, kScanThreads)), dim3(kScanThreads), 0, st, a,
                     levels > 1 ? klv[1] : static_cast<const std::uint64_t*>(nullptr),
                     levels > 1 ? vlv[1] : static_cast<const std::uint64_t*>(nullptr));
  std::uint32_t kw = 0, vw = 0;
  if (kcopy) kw = launch_emit<false>(s, a, c.keys, a.ktotal, st);
  if (vcopy) vw = launch_emit<true>(s, a, c.vals, a.vtotal, st);
  TKV_HIP_RC(hipGetLastError());
  TKV_HIP_RC(hipStreamSynchronize(st));
  g_dec_last[0] = kw;
  g_dec_last[1] = vw;
  g_dec_last[2] = a.ktotal;
  g_dec_last[3] = a.vtotal;
  return TKV_OK;
}

}  // namespace

int wal_decode_device_impl(const WalDecodeCall& c, hipStream_t st) {
  for (auto& v : g_dec_last) v = 0;
  DecScratch* sp = nullptr;
  if (int rc = per_device_scratch(&sp, kDecHres, 1, true)) return rc;
  DecArgs a{};
  a.img = c.img;
  a.size = c.size;
  a.off64 = c.rec_off64;
  a.off32 = c.rec_off32;
  a.n = c.n;
  a.key_views = (c.flags & TKV_WAL_DECODE_KEY_VIEWS) ? 1u : 0u;
  a.val_views = (c.flags & TKV_WAL_DECODE_VAL_VIEWS) ? 1u : 0u;
  a.op = c.op;
  a.tomb = c.tomb;
  a.seq = c.seq;
  a.key_off = c.key_off;
  a.key_len = c.key_len;
  a.val_off = c.val_off;
  a.val_len = c.val_len;
  std::lock_guard<std::mutex> lk(sp->mu);
  return decode_locked(*sp, a, c, st);
}

}  // namespace tkv

extern "C" {

void tkv_debug_wal_decode_geometry(uint64_t out[4]) {
  out[0] = tkv::kDecTile;
  out[1] = tkv::kScanBlock;
  out[2] = tkv::kShortSpan;
  out[3] = tkv::kScanLevels;
}

void tkv_debug_wal_decode_last(uint64_t out[4]) {
  for (int i = 0; i < 4; ++i) out[i] = tkv::g_dec_last[i];
}

}  // extern "C"
