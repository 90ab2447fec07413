// WAL resynchronisation (tkv_wal_resync_device; the search step of tkv_wal_salvage[_device],
// include/tkv_crc32.h): the smallest position p >= from of an image in HBM at which a
// record passes every check of wal_entry::decode (wal.cpp:63-127), i.e.
//   1. size - p >= 26;  2. record_len + 8 <= size - p;  3. 18 + key_len + val_len <= record_len;
//   4. the CRC-32 of the record_len payload bytes equals the stored field.
// Every byte offset behind a corrupted record is a candidate start, and only the CRC proves one.
//
// The search goes in spans of start offsets from `from`: kRsFirstSpan first (real damage is a sector or
// a torn record), then kRsGrow times longer each, up to kRsMaxSpan. Per span, in stream order:
//   rs_filter  one wave per window of kRsWindow = 4096 start offsets. Windows are cut at 16-byte
//              aligned addresses, so a lane's 64 offsets start on a granule: it loads the 6 granules
//              that hold them and the 25-byte halo (clamped to the image's last granule), forms the
//              three u32 fields at each byte offset with v_alignbyte at compile-time shifts, and applies
//              checks 2 and 3 in 64-bit arithmetic (they imply check 1). The survivors are a 64-bit mask
//              per lane; the wave adds up their count and their payload bytes per window.
//   rs_scan    the exclusive prefix of the window counts (one wave).
//   (host)     reads the per-window counts and bytes, and cuts the windows into batches of bounded
//              payload bytes and candidates, in offset order.
//   rs_emit    per batch: the survivors' (payload offset, record_len, stored CRC), in offset order,
//              each lane's index from the window's base and a wave prefix of the mask popcounts.
//   batch CRC  the irregular batch engine over the list (batch_device_impl: long payloads are split
//              across waves there).
//   rs_pick    the minimum survivor whose CRC equals its stored field (a 64-bit atomic minimum).
//   long ones  a batch's long survivors (record_len above 64 KiB) are set aside by rs_emit<false> and
//              folded behind the short ones, only those in front of the first valid short survivor
//              (rs_emit<true>): one by one as uniform batches of one when they are few, else through the
//              batch engine; then the minimum again (see kRsLongLen).
// The search stops after the batch that holds the first valid candidate, so plausible headers behind
// the answer are never folded, and those in front of it only up to the batch's bound. The masks make
// the result exact for any candidate density: a window may hold 4096 survivors. The one fixed-size
// hand-over is the kRsSingles slots of a batch's long survivors, with the second batch run behind it.
// Loads are whole 16-byte granules that hold at least one byte of the image: the first may begin up to 15
// bytes in front of it and the last end up to 15 bytes behind it (same page), as in the record check.
// Positions are u64 everywhere; 32-bit arithmetic only within a window or a lane's 64 offsets.
//
// Adversarial cost: an image whose damaged range is dense with plausible headers and long record_len
// values costs candidates x payload bytes of CRC work, as a sequential salvage would.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>

#include "tkv_crc32.h"
#include "tkv_crc32_device.h"
#include "tkv_device_util.h"
#include "tkv_engine.h"
#include "tkv_wal_device.h"
#include "tkv_wal_layout.h"

namespace tkv {
namespace {

constexpr std::uint32_t kRsWindow = 4096;                         // start offsets per wave
constexpr std::uint64_t kRsFirstSpan = std::uint64_t(64) << 10;   // start offsets of a search's first span
constexpr std::uint64_t kRsMaxSpan = std::uint64_t(16) << 20;     // and of its largest
constexpr std::uint64_t kRsGrow = 4;
constexpr std::uint32_t kRsMaxWin = static_cast<std::uint32_t>(kRsMaxSpan / kRsWindow) + 1;  // (a span may straddle one more)
// A batch of survivors closes behind the window in which it reaches either bound.
constexpr std::uint64_t kRsBatchBytes = std::uint64_t(32) << 20;
constexpr std::uint64_t kRsBatchCands = std::uint64_t(1) << 18;
// Survivors with a longer record_len are "long". A batch folds its short survivors first and then only the
// long ones in front of the first valid short one: a real record is short, and the larger the image, the
// likelier a random u32 is a record_len that fits it (in a 1 GiB image of small records with random keys
// and values the windows behind one flipped bit hold some 170 long survivors with 67 GB of payload
// between them, behind the answer). Up to kRsSingles long survivors ahead go one by one
// through the uniform engine: the irregular batch engine needs many blocks to spread long ones over the
// device and takes milliseconds for a single long block (tools/crc_long_block_probe.py,
// profiles/wal_salvage/long_block.txt); more than that, through the batch, a second run over the list.
constexpr std::uint32_t kRsLongLen = 64u << 10;
constexpr std::uint32_t kRsSingles = 64;
constexpr unsigned kRsThreads = 256;
constexpr unsigned kRsWaves = kRsThreads / 64;
constexpr int kRsGran = 6;  // 64 start offsets and the 25-byte halo: 89 bytes from a granule's first byte

struct RsArgs {
  std::uintptr_t w0;            // the image's first byte
  std::uint64_t size;
  std::uintptr_t a0;            // window 0's first address (16-byte aligned, at most 15 bytes below lo)
  std::uintptr_t lo, hi;        // the span's start offsets as addresses [lo, hi), hi <= w0 + size - 25
  std::uint32_t nwin;
  unsigned long long* mask;     // [nwin * 64] survivors among each lane's 64 offsets
  std::uint32_t* wcnt;          // [nwin] survivors per window
  unsigned long long* wbytes;   // [nwin] their record_len sum
  std::uint32_t* wbase;         // [nwin] exclusive prefix of wcnt (rs_scan)
  std::uint32_t* wlong;         // [nwin] survivors with record_len > kRsLongLen
};

// The u32 at byte b (compile time) of the lane's realigned dwords.
template <int B>
__device__ __forceinline__ std::uint32_t rs_field(const std::uint32_t (&raw)[4 * kRsGran]) {
  if constexpr (B % 4 == 0) return raw[B / 4];
  else return __builtin_amdgcn_alignbyte(raw[B / 4 + 1], raw[B / 4], B % 4);
}

template <int J>
__device__ __forceinline__ void rs_test(const std::uint32_t (&raw)[4 * kRsGran], std::uint64_t rem0, std::uint64_t& m) {
  const std::uint32_t rl = rs_field<J>(raw);
  // cheap reject first: record_len + 8 within the image fails at almost every offset
  bool ok = static_cast<std::uint64_t>(rl) + (kWalPayload + J) <= rem0;
  const std::uint32_t kl = rs_field<J + kWalKeyLen>(raw), vl = rs_field<J + kWalValLen>(raw);
  ok = ok && static_cast<std::uint64_t>(kl) + vl + (kWalMeta - kWalPayload) <= rl;
  m |= ok ? (1ull << J) : 0ull;
  // The field at byte b serves offsets b, b - 18 and b - 22: scheduled freely, the 64 offsets keep most
  // of the realigned dwords live at once (186 VGPRs); four offsets at a time stay below 128.
  if constexpr (J % 4 == 3) __builtin_amdgcn_sched_barrier(0);
  if constexpr (J + 1 < 64) rs_test<J + 1>(raw, rem0, m);
}

__device__ __forceinline__ std::uint32_t rs_u32(const std::uint8_t* p) {
  return static_cast<std::uint32_t>(p[0]) | (static_cast<std::uint32_t>(p[1]) << 8) | (static_cast<std::uint32_t>(p[2]) << 16) |
         (static_cast<std::uint32_t>(p[3]) << 24);
}

__global__ __launch_bounds__(kRsThreads) void rs_filter(RsArgs a) {
  const std::uint32_t lane = threadIdx.x & 63u;
  const std::uint32_t w = blockIdx.x * kRsWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (w >= a.nwin) return;
  const std::uintptr_t glast = (a.w0 + a.size - 1u) & ~static_cast<std::uintptr_t>(15);  // the image's last granule
  const std::uintptr_t ap0 = a.a0 + static_cast<std::uint64_t>(w) * kRsWindow + 64u * lane;  // the lane's first offset
  std::uint32_t raw[4 * kRsGran];
#pragma unroll
  for (int i = 0; i < kRsGran; ++i) {
    const std::uintptr_t p = ap0 + 16u * i;
    const uint4 g = dev::gload16(p < glast ? p : glast);  // clamped: no load leaves the image's granules
    raw[4 * i + 0] = g.x;
    raw[4 * i + 1] = g.y;
    raw[4 * i + 2] = g.z;
    raw[4 * i + 3] = g.w;
  }
  // Bytes left at the lane's first offset. It wraps for a lane behind the image's end, and the fields
  // of a clamped granule are not the image's: every such offset lies at or behind a.hi and is masked
  // below (an offset in front of a.hi has its 26 header bytes inside the image, so none was clamped).
  const std::uint64_t rem0 = a.w0 + a.size - ap0;
  std::uint64_t m = 0;
  rs_test<0>(raw, rem0, m);
  // the lane's offsets inside [lo, hi)
  const std::uint64_t jlo = a.lo > ap0 ? std::min<std::uint64_t>(a.lo - ap0, 64u) : 0u;
  const std::uint64_t jhi = a.hi > ap0 ? std::min<std::uint64_t>(a.hi - ap0, 64u) : 0u;
  const std::uint64_t below_hi = jhi >= 64u ? ~0ull : (1ull << jhi) - 1ull;
  const std::uint64_t below_lo = jlo >= 64u ? ~0ull : (1ull << jlo) - 1ull;
  m &= below_hi & ~below_lo;
  // The survivors' record_len sum. Survivors are rare, and their bytes are in the cache: byte loads (a
  // survivor has its header inside the image) keep the 64 record_len values out of the registers.
  std::uint64_t bytes = 0;
  std::uint32_t nlong = 0;
  for (std::uint64_t mm = m; mm; mm &= mm - 1u) {
    const std::uint32_t rl = rs_u32(reinterpret_cast<const std::uint8_t*>(ap0 + static_cast<std::uint32_t>(__builtin_ctzll(mm))));
    bytes += rl;
    nlong += rl > kRsLongLen ? 1u : 0u;
  }
  a.mask[static_cast<std::uint64_t>(w) * 64u + lane] = m;
  std::uint32_t cnt_all, long_all;
  std::uint64_t bytes_all;
  (void)dev::lane_prefix<std::uint32_t>(static_cast<std::uint32_t>(__builtin_popcountll(m)), &cnt_all);
  (void)dev::lane_prefix<std::uint32_t>(nlong, &long_all);
  (void)dev::lane_prefix<std::uint64_t>(bytes, &bytes_all);
  if (lane == 0) {
    a.wcnt[w] = cnt_all;
    a.wlong[w] = long_all;
    a.wbytes[w] = bytes_all;
  }
}

// wbase = the exclusive prefix of wcnt, by one wave.
__global__ __launch_bounds__(64) void rs_scan(RsArgs a) {
  std::uint32_t run = 0;
  for (std::uint32_t i0 = 0; i0 < a.nwin; i0 += 64u) {
    const std::uint32_t i = i0 + threadIdx.x;
    std::uint32_t total;
    const std::uint32_t pre = dev::lane_prefix<std::uint32_t>(i < a.nwin ? a.wcnt[i] : 0u, &total);
    if (i < a.nwin) a.wbase[i] = run + pre;
    run += total;
  }
}

struct RsList {
  std::uint64_t* off;     // payload offset in the image (p + 8)
  std::uint32_t* len;     // record_len; 0 while a long survivor is set aside (the batch engine folds nothing for it)
  std::uint32_t* stored;  // the CRC field
  std::uint32_t* crc;     // computed (batch_device_impl; a long survivor's by the uniform engine, or stale)
};

// A batch's result word and what its long survivors come to; the head, or all of it, is copied to the host.
struct RsSingles {
  unsigned long long res;             // smallest valid record start so far, ~0 for none
  unsigned long long long_bytes;      // record_len sum of the batch's long survivors (rs_emit<false>)
  unsigned long long ahead_bytes;     // and of those in front of the limit (rs_emit<true>)
  std::uint32_t n, pad;               // long survivors in front of the limit (the first kRsSingles are listed)
  std::uint64_t off[kRsSingles];      // payload offset
  std::uint32_t len[kRsSingles];      // record_len
  std::uint32_t idx[kRsSingles];      // list entry
};
constexpr std::size_t kRsHead = 32;   // res .. pad

// The survivors of windows [w_first, w_end) in offset order, entry 0 = survivor `first` of the span: payload
// offset, record_len and stored CRC, a long survivor with length 0 (set aside). AHEAD, the second pass
// behind the short survivors' CRCs: the long survivors in front of `limit` get their length back and a
// slot in `single` (an atomic slot each; their order does not matter). A survivor has at least 26 bytes
// inside the image, so its byte loads stay there.
template <bool AHEAD>
__global__ __launch_bounds__(kRsThreads) void rs_emit(RsArgs a, std::uint32_t w_first, std::uint32_t w_end, std::uint32_t first,
                                                      RsList l, RsSingles* single, std::uint64_t limit) {
  const std::uint32_t lane = threadIdx.x & 63u;
  const std::uint32_t w = w_first + blockIdx.x * kRsWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (w >= w_end) return;
  std::uint64_t m = a.mask[static_cast<std::uint64_t>(w) * 64u + lane];
  std::uint32_t total;
  const std::uint32_t pre = dev::lane_prefix<std::uint32_t>(static_cast<std::uint32_t>(__builtin_popcountll(m)), &total);
  if (total == 0) return;
  std::uint64_t idx = static_cast<std::uint64_t>(a.wbase[w] - first) + pre;
  const std::uintptr_t ap0 = a.a0 + static_cast<std::uint64_t>(w) * kRsWindow + 64u * lane;
  for (; m; m &= m - 1u, ++idx) {
    const std::uint32_t j = static_cast<std::uint32_t>(__builtin_ctzll(m));
    const std::uint8_t* p = reinterpret_cast<const std::uint8_t*>(ap0 + j);
    const std::uint64_t pos = static_cast<std::uint64_t>(ap0 + j - a.w0);
    const std::uint32_t rl = rs_u32(p);
    const bool is_long = rl > kRsLongLen;
    if constexpr (AHEAD) {
      // (a short survivor is done with: length 0, so that a second run of the batch over the list, the
      // route of more than kRsSingles long survivors ahead, folds those alone and rs_pick skips the rest)
      if (!is_long) l.len[idx] = 0u;
      if (!is_long || pos >= limit) continue;
      l.len[idx] = rl;
      atomicAdd(&single->ahead_bytes, static_cast<unsigned long long>(rl));
      const std::uint32_t k = atomicAdd(&single->n, 1u);
      if (k < kRsSingles) {
        single->off[k] = pos + kWalPayload;
        single->len[k] = rl;
        single->idx[k] = static_cast<std::uint32_t>(idx);
      }
    } else {
      if (is_long) atomicAdd(&single->long_bytes, static_cast<unsigned long long>(rl));
      l.off[idx] = pos + kWalPayload;
      l.len[idx] = is_long ? 0u : rl;
      l.stored[idx] = rs_u32(p + kWalCrc);
    }
  }
}

// *res (preset to ~0) = the smallest record start of the list whose computed CRC equals its stored one
// (entries set aside, len 0, are not looked at: a survivor's record_len is at least 18).
__global__ __launch_bounds__(kRsThreads) void rs_pick(RsList l, std::uint64_t n, unsigned long long* res) {
  const std::uint64_t i = blockIdx.x * static_cast<std::uint64_t>(kRsThreads) + threadIdx.x;
  if (i < n && l.len[i] != 0u && l.crc[i] == l.stored[i])
    atomicMin(res, static_cast<unsigned long long>(l.off[i] - kWalPayload));
}

// The same over the n <= kRsSingles long survivors listed in `single`, folded one by one.
__global__ __launch_bounds__(64) void rs_pick_singles(RsList l, RsSingles* single, std::uint32_t n) {
  const std::uint32_t k = threadIdx.x;
  if (k >= n) return;
  const std::uint32_t i = single->idx[k];
  if (l.crc[i] == l.stored[i]) atomicMin(&single->res, static_cast<unsigned long long>(single->off[k] - kWalPayload));
}

__global__ __launch_bounds__(kRsThreads) void rs_add_base(std::uint64_t* off, std::uint64_t n, std::uint64_t base) {
  const std::uint64_t i = blockIdx.x * static_cast<std::uint64_t>(kRsThreads) + threadIdx.x;
  if (i < n) off[i] += base;
}

// Per-device scratch, grown by doubling and kept between calls (guarded by mu).
struct RsScratch {
  std::mutex mu;
  std::uint64_t cap_win = 0, cap_list = 0;
  void* win = nullptr;    // per window: mask (64 u64), wbytes (u64), wcnt, wbase, wlong (u32)
  void* list = nullptr;   // per survivor of a batch: off (u64), len, stored, crc (u32)
  RsSingles* res = nullptr;
  std::uint8_t* h = nullptr;  // pinned: RsSingles, wbytes[kRsMaxWin], wcnt[kRsMaxWin], wlong[kRsMaxWin]
  ~RsScratch() {
    (void)hipFree(win);
    (void)hipFree(list);
    (void)hipFree(res);
    (void)hipHostFree(h);
  }
};
constexpr std::uint64_t kRsWinUnit = 64 * 8 + 8 + 4 + 4 + 4, kRsListUnit = 8 + 4 + 4 + 4;

int rs_scratch(RsScratch** out) {
  RsScratch* sp = nullptr;
  if (int rc = per_device(&sp)) return rc;
  std::lock_guard<std::mutex> lk(sp->mu);
  // (each on its own: a failure of the second leaves the first for the next call, not a second copy of it)
  if (!sp->h)
    TKV_HIP_RC(hipHostMalloc(reinterpret_cast<void**>(&sp->h), sizeof(RsSingles) + kRsMaxWin * 16ull, hipHostMallocDefault));
  if (!sp->res) TKV_HIP_RC(hipMalloc(reinterpret_cast<void**>(&sp->res), sizeof(RsSingles)));
  *out = sp;
  return TKV_OK;
}

// What the calling thread's last resync or salvage did (tkv_debug_wal_salvage_last).
thread_local std::uint64_t g_rs_last[6] = {0, 0, 0, 0, 0, 0};

// One span: *found = the smallest valid position among the start offsets [pos, pos + len), ~0 for none.
// Caller holds s.mu; pos + len + 25 <= size.
int rs_span(RsScratch& s, const std::uint8_t* w, std::uint64_t size, std::uint64_t pos, std::uint64_t len, std::uint64_t* found,
            hipStream_t st) {
  *found = ~0ull;
  RsArgs a{};
  a.w0 = reinterpret_cast<std::uintptr_t>(w);
  a.size = size;
  a.lo = a.w0 + pos;
  a.hi = a.lo + len;
  a.a0 = a.lo & ~static_cast<std::uintptr_t>(15);
  a.nwin = static_cast<std::uint32_t>((a.hi - a.a0 + kRsWindow - 1) / kRsWindow);
  if (int e = grow(&s.win, &s.cap_win, a.nwin, kRsWinUnit)) return e;
  a.mask = static_cast<unsigned long long*>(s.win);
  a.wbytes = a.mask + 64 * s.cap_win;
  a.wcnt = reinterpret_cast<std::uint32_t*>(a.wbytes + s.cap_win);
  a.wbase = a.wcnt + s.cap_win;
  a.wlong = a.wbase + s.cap_win;
  hipLaunchKernelGGL(rs_filter, dim3(blocks(a.nwin, kRsWaves)), dim3(kRsThreads), 0, st, a);
  hipLaunchKernelGGL(rs_scan, dim3(1), dim3(64), 0, st, a);
  TKV_HIP_RC(hipGetLastError());
  auto* h_res = reinterpret_cast<RsSingles*>(s.h);
  auto* h_bytes = reinterpret_cast<std::uint64_t*>(h_res + 1);
  auto* h_cnt = reinterpret_cast<std::uint32_t*>(h_bytes + kRsMaxWin);
  auto* h_long = h_cnt + kRsMaxWin;
  TKV_HIP_RC(hipMemcpyAsync(h_bytes, a.wbytes, a.nwin * 8ull, hipMemcpyDeviceToHost, st));
  TKV_HIP_RC(hipMemcpyAsync(h_cnt, a.wcnt, a.nwin * 4ull, hipMemcpyDeviceToHost, st));
  TKV_HIP_RC(hipMemcpyAsync(h_long, a.wlong, a.nwin * 4ull, hipMemcpyDeviceToHost, st));
  TKV_HIP_RC(hipStreamSynchronize(st));
  g_rs_last[1] += 1;
  g_rs_last[2] += len;
  // batches of survivors in offset order, closed behind the window that reaches a bound
  std::uint32_t first = 0;  // survivors in front of the batch
  for (std::uint32_t wi = 0; wi < a.nwin;) {
    const std::uint32_t b0 = wi;
    std::uint64_t cnt = 0, bytes = 0, nlong = 0;
    do {
      cnt += h_cnt[wi];
      bytes += h_bytes[wi];
      nlong += h_long[wi];
      ++wi;
    } while (wi < a.nwin && cnt < kRsBatchCands && bytes < kRsBatchBytes);
    if (cnt == 0) continue;
    const std::uint64_t listed = cnt;  // (cnt and bytes go on as what was folded)
    if (int e = grow(&s.list, &s.cap_list, listed, kRsListUnit)) return e;
    RsList l{};
    l.off = static_cast<std::uint64_t*>(s.list);
    l.len = reinterpret_cast<std::uint32_t*>(l.off + s.cap_list);
    l.stored = l.len + s.cap_list;
    l.crc = l.stored + s.cap_list;
    TKV_HIP_RC(hipMemsetAsync(&s.res->res, 0xFF, sizeof(unsigned long long), st));
    TKV_HIP_RC(hipMemsetAsync(&s.res->long_bytes, 0, kRsHead - sizeof(unsigned long long), st));
    hipLaunchKernelGGL(rs_emit<false>, dim3(blocks(wi - b0, kRsWaves)), dim3(kRsThreads), 0, st, a, b0, wi, first, l, s.res,
                       ~0ull);
    TKV_HIP_RC(hipGetLastError());
    // the short survivors first: a real record is short, and only the long survivors in front of the
    // first valid short one can still be the answer
    if (listed > nlong) {
      if (int rc = batch_device_impl(kAlgoCrc32, w, l.off, l.len, nullptr, l.crc, listed, st)) return rc;
      hipLaunchKernelGGL(rs_pick, dim3(blocks(listed, kRsThreads)), dim3(kRsThreads), 0, st, l, listed, &s.res->res);
      TKV_HIP_RC(hipGetLastError());
    }
    TKV_HIP_RC(hipMemcpyAsync(h_res, s.res, kRsHead, hipMemcpyDeviceToHost, st));
    TKV_HIP_RC(hipStreamSynchronize(st));
    if (nlong) {
      const std::uint64_t limit = h_res->res;
      hipLaunchKernelGGL(rs_emit<true>, dim3(blocks(wi - b0, kRsWaves)), dim3(kRsThreads), 0, st, a, b0, wi, first, l, s.res,
                         limit);
      TKV_HIP_RC(hipGetLastError());
      TKV_HIP_RC(hipMemcpyAsync(h_res, s.res, sizeof(RsSingles), hipMemcpyDeviceToHost, st));
      TKV_HIP_RC(hipStreamSynchronize(st));
      const std::uint32_t ahead = h_res->n;
      cnt = listed - nlong + ahead;
      bytes = bytes - h_res->long_bytes + h_res->ahead_bytes;
      if (ahead != 0 && ahead <= kRsSingles) {
        // few: one by one through the uniform engine, each at the rate of a single span
        for (std::uint32_t k = 0; k < ahead; ++k)
          if (int rc = batch_uniform_impl(kAlgoCrc32, w + h_res->off[k], h_res->len[k], h_res->len[k], nullptr,
                                          l.crc + h_res->idx[k], 1, st))
            return rc;
        hipLaunchKernelGGL(rs_pick_singles, dim3(1), dim3(64), 0, st, l, s.res, ahead);
      } else if (ahead != 0) {
        // many: the batch over the list again, which now holds lengths for the long survivors ahead alone
        if (int rc = batch_device_impl(kAlgoCrc32, w, l.off, l.len, nullptr, l.crc, listed, st)) return rc;
        hipLaunchKernelGGL(rs_pick, dim3(blocks(listed, kRsThreads)), dim3(kRsThreads), 0, st, l, listed, &s.res->res);
      }
      if (ahead != 0) {
        TKV_HIP_RC(hipGetLastError());
        TKV_HIP_RC(hipMemcpyAsync(h_res, s.res, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        TKV_HIP_RC(hipStreamSynchronize(st));
      }
    }
    g_rs_last[3] += cnt;
    g_rs_last[4] += bytes;
    if (h_res->res != ~0ull) {
      *found = h_res->res;
      return TKV_OK;
    }
    first += static_cast<std::uint32_t>(listed);
  }
  return TKV_OK;
}

}  // namespace

int wal_resync_device_impl(const std::uint8_t* d_wal, std::uint64_t size, std::uint64_t from, std::uint64_t* found,
                           hipStream_t st) {
  *found = size;
  g_rs_last[0] += 1;
  if (size < kWalMeta || from > size - kWalMeta) return TKV_NOT_FOUND;  // fewer than 26 bytes left everywhere
  if (!device_tables(kAlgoCrc32)) return TKV_IO_ERROR;  // (creates the device context; left the error text)
  RsScratch* sp = nullptr;
  if (int rc = rs_scratch(&sp)) return rc;
  RsScratch& s = *sp;
  std::lock_guard<std::mutex> lk(s.mu);
  const std::uint64_t end = size - kWalMeta + 1;  // start offsets with 26 bytes left: [0, end)
  std::uint64_t span = kRsFirstSpan;
  for (std::uint64_t pos = from; pos < end; span = std::min(span * kRsGrow, kRsMaxSpan)) {
    const std::uint64_t len = std::min(span, end - pos);
    std::uint64_t p = ~0ull;
    if (int rc = rs_span(s, d_wal, size, pos, len, &p, st)) return rc;
    if (p != ~0ull) {
      *found = p;
      return TKV_OK;
    }
    pos += len;
  }
  return TKV_NOT_FOUND;
}

int wal_salvage_add_base(std::uint64_t* d_off64, std::uint64_t n, std::uint64_t base, hipStream_t st) {
  if (n == 0 || base == 0) return TKV_OK;
  hipLaunchKernelGGL(rs_add_base, dim3(blocks(n, kRsThreads)), dim3(kRsThreads), 0, st, d_off64, n, base);
  TKV_HIP_RC(hipGetLastError());
  return TKV_OK;
}

std::uint64_t* wal_salvage_last() { return g_rs_last; }

}  // namespace tkv

extern "C" void tkv_debug_wal_salvage_geometry(uint64_t out[4]) {
  out[0] = tkv::kRsWindow;
  out[1] = tkv::kRsFirstSpan;
  out[2] = tkv::kRsMaxSpan;
  // The survivor masks hold any density of candidates. The one fixed-size hand-over is a batch's long
  // survivors in front of its first valid short one: up to kRsSingles are folded one by one, more than
  // that by a second run of the batch engine over the list.
  out[3] = tkv::kRsSingles;
}

extern "C" void tkv_debug_wal_salvage_last(uint64_t out[6]) {
  for (int i = 0; i < 6; ++i) out[i] = tkv::g_rs_last[i];
}
