// SSTable merge on the device (include/tkv_crc32.h "SSTable merge"): K sorted runs of
// internal keys, oldest first, into one ascending run in which of all entries with one user key only the
// one from the newest run (and there the last) is left, optionally without tombstones.
//
// mg_check: one lane per input entry, the runs laid one after the other (position = start[r] + i; a lane
//   finds its run by a search over the run table): the span checks, the order check against the entry in
//   front of it in its run, and the 16-byte sort entry {word, digit << 40 | r << 32 | i}: word = user-key
//   bytes [0, 8) big-endian, zero-padded, digit = min(user-key length, 9) (tkv_memtable_layout.h). The
//   smallest bad position goes to a device word by a wave minimum and one atomic minimum. EVERY KERNEL
//   BEHIND THE CHECK READS THAT WORD AND DOES NOTHING WHEN IT IS SET, so the host does not wait for the
//   verdict before it launches them: keys are only ever read through spans the check has passed.
// mg_round: one launch per round merges neighbouring lists pairwise ((0,1), (2,3), ...; an unpaired list
//   is a pair with an empty right side), so lists stay in age order: ceil(log2 K') rounds for K' non-empty
//   runs. Merge path: a workgroup owns kMgTile consecutive outputs of one pair (the map tile -> {pair,
//   diagonal} is built on the host, where every size is known), finds the split of both inputs at its two
//   diagonals by binary searches in global memory, stages both sub-ranges in LDS, and every thread finds
//   its own diagonal there and merges kMgItems outputs serially; the outputs go back through LDS so that
//   neighbouring lanes store neighbouring entries. The comparator (mg_cmp) is (word, digit); only a tie
//   with digit 9 (both keys go on) reads the rest of the two keys where they lie. On equal keys the OLDER
//   side goes first, in the partition search and in the tile alike, so equal keys end up adjacent in age
//   order.
// mg_ties: entry j of the final order dies when entry j + 1 has the same user key, and under the drop flag
//   when its last key byte is non-zero; level 0 of the u64 scan of the survivor flags (tkv_scan.h), the
//   survivors' key and value bytes summed per workgroup beside it. mg_sum adds the workgroups' sums up in
//   one workgroup (one atomic add per wave on a single word took 3.4 ms of 3.9 for 18 M entries: atomics on
//   one address serialise in L2).
// mg_emit: the five columns of the survivors.
// Host synchronisations: two (the verdict with the sizes; the end of the emit).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "tkv_crc32.h"
#include "tkv_crc32_device.h"
#include "tkv_device_util.h"
#include "tkv_engine.h"
#include "tkv_key_word.h"
#include "tkv_memtable_layout.h"
#include "tkv_runs_device.h"
#include "tkv_scan.h"

namespace tkv {
namespace {

constexpr unsigned kMgThreads = 256;
constexpr unsigned kMgItems = 8;                               // outputs a thread merges serially
constexpr std::uint32_t kMgTile = kMgThreads * kMgItems;       // outputs per workgroup: 32 KiB of LDS
constexpr unsigned kMgHres = 8;                                // words of the pinned result block
enum : int { kMsBad = 0, kMsKeys, kMsVals, kMsWords };

// A workgroup's share of a round: the pair's lists in[s0, s1) and in[s1, s2), outputs [d, d + kMgTile) of
// out[s0, s2).
struct MgTile {
  std::uint32_t s0, s1, s2, d;
};

// Sort entries, as two arrays: the comparison word, and digit << 40 | run << 32 | index.
struct MgList {
  std::uint64_t* w;
  std::uint64_t* x;
};

struct MgArgs {
  const MgRun* runs;
  std::uint32_t n_runs;
  std::uint32_t flags;
  std::uint64_t n;
  unsigned long long* st;  // kMsWords device words
  std::uint64_t* cnt;      // exclusive scan of the survivor flags
  std::uint64_t* bytes;    // per workgroup of mg_ties: the survivors' key bytes, value bytes
  std::uint8_t* live;      // 1: the entry at this position survives
  std::uint64_t m;
  std::uint64_t* o_key_off;
  std::uint32_t* o_key_len;
  std::uint64_t* o_val_off;
  std::uint32_t* o_val_len;
  std::uint64_t* o_src;
};

__device__ __forceinline__ bool verdict_bad(const unsigned long long* st) {
  return __hip_atomic_load(st + kMsBad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != ~0ull;
}

// ---- check and sort entries -------------------------------------------------------------------------

__global__ void mg_init(unsigned long long* st) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    st[kMsBad] = ~0ull;
  }
}

__global__ __launch_bounds__(kScanThreads) void mg_check(MgArgs a, MgList l) {
  const std::uint64_t p = blockIdx.x * static_cast<std::uint64_t>(kScanThreads) + threadIdx.x;
  std::uint32_t bad = ~0u;  // (positions stay below 2^32 - 1, and they order as r << 32 | i does)
  if (p < a.n) {
    // the last run that starts at or before p (empty runs share their start with the run behind them)
    std::uint32_t lo = 0, hi = a.n_runs;
    while (lo < hi) {
      const std::uint32_t mid = (lo + hi) >> 1;
      if (a.runs[mid].start <= p) lo = mid + 1u;
      else hi = mid;
    }
    const std::uint32_t rn = lo - 1u;
    const MgRun& r = a.runs[rn];
    const std::uint64_t i = p - r.start;
    const std::uint64_t ko = r.key_off[i];
    const std::uint32_t kl = r.key_len[i];
    bool ok = span_ok(r, ko, kl);
    std::uint64_t w = 0;
    std::uint32_t dg = 0;  // (a bad entry never reaches a key read: its digit says the key ended)
    if (ok) {
      const MgKey k{reinterpret_cast<std::uintptr_t>(r.keys) + ko, kl - kMtMeta};
      w = load_word(k.addr, k.ulen);
      dg = mt_digit(k.ulen);
      if (i > 0) {
        const std::uint64_t pko = r.key_off[i - 1u];
        const std::uint32_t pkl = r.key_len[i - 1u];
        if (span_ok(r, pko, pkl)) {
          const MgKey pk{reinterpret_cast<std::uintptr_t>(r.keys) + pko, pkl - kMtMeta};
          const std::uint64_t pw = load_word(pk.addr, pk.ulen);
          const std::uint32_t pd = mt_digit(pk.ulen);
          const int c = pw != w ? (pw < w ? -1 : 1) : pd != dg ? (pd < dg ? -1 : 1) : dg < kMtDigitMore ? 0 : cmp_rest(pk, k);
          if (c > 0) ok = false;
        }
      }
    }
    if (!ok) bad = static_cast<std::uint32_t>(p);
    l.w[p] = w;
    l.x[p] = (static_cast<std::uint64_t>(dg) << kMgDigitShift) | (static_cast<std::uint64_t>(rn) << kMgRunShift) | i;
  }
  const std::uint32_t wbad = dev::wave_min(bad);
  if ((threadIdx.x & 63u) == 0 && wbad != ~0u) atomicMin(a.st + kMsBad, static_cast<unsigned long long>(wbad));
}

// ---- one merge round --------------------------------------------------------------------------------

// How many of the first d outputs of the pair come from its left list: entries of the left list go in
// front of equal ones of the right list.
__device__ std::uint32_t mg_split(const MgRun* runs, const MgList& in, const MgTile& t, std::uint64_t d) {
  const std::uint64_t na = t.s1 - t.s0, nb = t.s2 - t.s1;
  std::uint64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
  while (lo < hi) {
    const std::uint64_t mid = lo + ((hi - lo) >> 1);
    const std::uint64_t ia = t.s0 + mid, ib = t.s1 + (d - 1u - mid);
    if (mg_cmp(runs, in.w[ia], in.x[ia], in.w[ib], in.x[ib]) <= 0) lo = mid + 1u;
    else hi = mid;
  }
  return static_cast<std::uint32_t>(lo);
}

__global__ __launch_bounds__(kMgThreads) void mg_round(MgArgs a, MgList in, MgList out, const MgTile* tiles) {
  __shared__ std::uint64_t sw[kMgTile];
  __shared__ std::uint64_t sx[kMgTile];
  __shared__ std::uint32_t split[2];
  if (verdict_bad(a.st)) return;
  const MgTile t = tiles[blockIdx.x];
  const std::uint64_t len = static_cast<std::uint64_t>(t.s2) - t.s0;
  const std::uint64_t d0 = t.d, d1 = std::min<std::uint64_t>(d0 + kMgTile, len);
  if (threadIdx.x == 0) split[0] = mg_split(a.runs, in, t, d0);
  if (threadIdx.x == 64) split[1] = mg_split(a.runs, in, t, d1);
  __syncthreads();
  const std::uint64_t i0 = split[0], i1 = split[1];
  const std::uint64_t j0 = d0 - i0, j1 = d1 - i1;
  if (i1 < i0 || j1 < j0 || d1 < d0) return;  // (cannot happen: the lists are sorted, the check saw to it)
  const std::uint32_t ca = static_cast<std::uint32_t>(i1 - i0), cb = static_cast<std::uint32_t>(j1 - j0);
  const std::uint32_t total = ca + cb;  // = d1 - d0 <= kMgTile
  if (total > kMgTile) return;          // (cannot happen)
  for (std::uint32_t k = threadIdx.x; k < total; k += kMgThreads) {
    const std::uint64_t src = k < ca ? t.s0 + i0 + k : t.s1 + j0 + (k - ca);
    sw[k] = in.w[src];
    sx[k] = in.x[src];
  }
  __syncthreads();
  // the thread's own diagonal within the staged ranges: left [0, ca), right [ca, ca + cb)
  const std::uint32_t dd = std::min<std::uint32_t>(threadIdx.x * kMgItems, total);
  std::uint32_t lo = dd > cb ? dd - cb : 0u, hi = dd < ca ? dd : ca;
  while (lo < hi) {
    const std::uint32_t mid = (lo + hi) >> 1;
    const std::uint32_t ib = ca + (dd - 1u - mid);
    if (mg_cmp(a.runs, sw[mid], sx[mid], sw[ib], sx[ib]) <= 0) lo = mid + 1u;
    else hi = mid;
  }
  std::uint32_t ai = lo, bi = dd - lo;
  std::uint64_t rw[kMgItems], rx[kMgItems];
#pragma unroll
  for (unsigned k = 0; k < kMgItems; ++k) {
    rw[k] = 0;
    rx[k] = 0;
    if (dd + k < total) {
      const bool left = bi >= cb || (ai < ca && mg_cmp(a.runs, sw[ai], sx[ai], sw[ca + bi], sx[ca + bi]) <= 0);
      const std::uint32_t from = left ? ai : ca + bi;
      ai += left ? 1u : 0u;
      bi += left ? 0u : 1u;
      rw[k] = sw[from];
      rx[k] = sx[from];
    }
  }
  __syncthreads();
#pragma unroll
  for (unsigned k = 0; k < kMgItems; ++k) {
    if (dd + k < total) {
      sw[dd + k] = rw[k];
      sx[dd + k] = rx[k];
    }
  }
  __syncthreads();
  const std::uint64_t dst = t.s0 + d0;
  for (std::uint32_t k = threadIdx.x; k < total; k += kMgThreads) {
    out.w[dst + k] = sw[k];
    out.x[dst + k] = sx[k];
  }
}

// ---- ties, tombstone drop, survivor scan ------------------------------------------------------------

__global__ __launch_bounds__(kScanThreads) void mg_ties(MgArgs a, MgList l, std::uint64_t* arr, std::uint64_t* bsum) {
  if (verdict_bad(a.st)) return;
  const std::uint64_t j0 = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
  const bool drop = (a.flags & TKV_SST_MERGE_DROP_TOMBSTONES) != 0;
  std::uint64_t v[kScanItems];
  std::uint64_t kb = 0, vb = 0;
#pragma unroll
  for (unsigned q = 0; q < kScanItems; ++q) {
    const std::uint64_t j = j0 + q;
    v[q] = 0;
    if (j < a.n) {
      const std::uint64_t w = l.w[j], x = l.x[j];
      bool live = j + 1u >= a.n || mg_cmp(a.runs, w, x, l.w[j + 1u], l.x[j + 1u]) != 0;
      const MgRun& r = run_of(a.runs, x);
      const std::uint64_t i = x & kMgIdxMask;
      const std::uint32_t kl = r.key_len[i];
      if (live && drop && r.keys[r.key_off[i] + kl - 1u] != 0) live = false;
      a.live[j] = live ? 1 : 0;
      if (live) {
        v[q] = 1;
        kb += kl;
        vb += r.val_len ? r.val_len[i] : 0u;
      }
    }
  }
  scan_items(v, j0, a.n, arr, bsum);
  __shared__ std::uint64_t wsum[2][kScanThreads / 64];
  std::uint64_t wk, wv;
  (void)dev::lane_prefix<std::uint64_t>(kb, &wk);
  (void)dev::lane_prefix<std::uint64_t>(vb, &wv);
  if ((threadIdx.x & 63u) == 0) {
    wsum[0][threadIdx.x >> 6] = wk;
    wsum[1][threadIdx.x >> 6] = wv;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    std::uint64_t t = 0;
#pragma unroll
    for (unsigned k = 0; k < kScanThreads / 64; ++k) t += wsum[threadIdx.x][k];
    a.bytes[2u * blockIdx.x + threadIdx.x] = t;
  }
}

// The sums of mg_ties' nblk workgroups (one workgroup; integer sums: any order gives the same result).
__global__ __launch_bounds__(kScanThreads) void mg_sum(MgArgs a, std::uint64_t nblk) {
  if (verdict_bad(a.st)) return;
  __shared__ std::uint64_t wsum[2][kScanThreads / 64];
  std::uint64_t kb = 0, vb = 0;
  for (std::uint64_t b = threadIdx.x; b < nblk; b += kScanThreads) {
    kb += a.bytes[2u * b];
    vb += a.bytes[2u * b + 1u];
  }
  std::uint64_t wk, wv;
  (void)dev::lane_prefix<std::uint64_t>(kb, &wk);
  (void)dev::lane_prefix<std::uint64_t>(vb, &wv);
  if ((threadIdx.x & 63u) == 0) {
    wsum[0][threadIdx.x >> 6] = wk;
    wsum[1][threadIdx.x >> 6] = wv;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    std::uint64_t t = 0;
#pragma unroll
    for (unsigned k = 0; k < kScanThreads / 64; ++k) t += wsum[threadIdx.x][k];
    a.st[threadIdx.x == 0 ? kMsKeys : kMsVals] = t;
  }
}

__global__ void mg_publish(const unsigned long long* st, const std::uint64_t* count, std::uint64_t* h, std::uint64_t tag) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    h[0] = st[kMsBad];
    h[1] = *count;
    h[2] = st[kMsKeys];
    h[3] = st[kMsVals];
    __threadfence_system();
    h[7] = tag;
  }
}

// ---- emit -------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kScanThreads) void mg_emit(MgArgs a, MgList l) {
  const std::uint64_t j = blockIdx.x * static_cast<std::uint64_t>(kScanThreads) + threadIdx.x;
  if (j >= a.n || !a.live[j]) return;
  const std::uint64_t e = a.cnt[j];
  if (e >= a.m) return;  // (cannot happen: m is the scan's own total)
  const std::uint64_t x = l.x[j];
  const MgRun& r = run_of(a.runs, x);
  const std::uint64_t i = x & kMgIdxMask;
  if (a.o_key_off) a.o_key_off[e] = r.key_bias + r.key_off[i];
  if (a.o_key_len) a.o_key_len[e] = r.key_len[i];
  if (a.o_val_off) a.o_val_off[e] = r.val_bias + (r.val_off ? r.val_off[i] : 0ull);
  if (a.o_val_len) a.o_val_len[e] = r.val_len ? r.val_len[i] : 0u;
  if (a.o_src) a.o_src[e] = x & ((1ull << kMgDigitShift) - 1ull);
}

// ---- host side --------------------------------------------------------------------------------------

// Per-device scratch, grown by doubling and kept between calls (guarded by mu).
struct MgScratch : ScratchBase {
  DeviceBuf w[2], x[2], scan, sums, bytes, live, runs, tiles;
  RunStage hs;  // pinned staging of the run table and the tile map
  unsigned long long*& st = words;
};

// The calling thread's device merges (tkv_debug_sst_merge_last, tkv_debug_sst_merge_phases).
thread_local PathStats g_mg;

template <class T>
int take(DeviceBuf& b, std::uint64_t want, T** out) {
  return tkv::take(b, want, out, g_mg.taken, "sst merge: scratch allocation failed");
}

int merge_locked(MgScratch& s, const SstMergeCall& c, hipStream_t st) {
  const std::uint32_t K = c.n_runs;
  // the run table and the lists of the first round
  std::vector<MgRun> runs(K);
  std::vector<std::uint64_t> cut{0};
  std::uint64_t n = 0;
  for (std::uint32_t r = 0; r < K; ++r) {
    MgRun& q = runs[r];
    q = MgRun{};
    q.start = n;
    if (c.n[r] == 0) continue;
    q.keys = c.keys[r];
    q.keys_size = c.keys_size[r];
    q.key_off = c.key_off[r];
    q.key_len = c.key_len[r];
    q.val_off = c.val_off ? c.val_off[r] : nullptr;
    q.val_len = c.val_len ? c.val_len[r] : nullptr;
    q.key_bias = c.out_key_off ? static_cast<std::uint64_t>(c.keys[r] - c.key_base) : 0u;
    q.val_bias = c.val_bias ? c.val_bias[r] : 0u;
    n += c.n[r];
    cut.push_back(n);
  }
  // the tile map of every round: neighbouring lists pairwise, an unpaired one with an empty right side
  std::vector<MgTile> tiles;
  std::vector<std::uint64_t> first;  // the first tile of every round, and the end
  while (cut.size() > 2) {
    first.push_back(tiles.size());
    std::vector<std::uint64_t> ncut{0};
    for (std::size_t p = 0; p + 1 < cut.size(); p += 2) {
      const std::uint64_t s0 = cut[p], s1 = cut[p + 1], s2 = p + 2 < cut.size() ? cut[p + 2] : s1;
      for (std::uint64_t d = 0; d < s2 - s0; d += kMgTile)
        tiles.push_back(MgTile{static_cast<std::uint32_t>(s0), static_cast<std::uint32_t>(s1), static_cast<std::uint32_t>(s2),
                               static_cast<std::uint32_t>(d)});
      ncut.push_back(s2);
    }
    cut.swap(ncut);
  }
  first.push_back(tiles.size());
  const std::uint64_t rounds = first.size() - 1u;

  MgArgs a{};
  MgList l[2];
  MgTile* d_tiles = nullptr;
  MgRun* d_runs = nullptr;
  for (int k = 0; k < 2; ++k) {
    if (int rc = take(s.w[k], n, &l[k].w)) return rc;
    if (int rc = take(s.x[k], n, &l[k].x)) return rc;
  }
  const ScanPlan plan(n);
  std::uint64_t* sums = nullptr;
  if (int rc = take(s.scan, n, &a.cnt)) return rc;
  if (int rc = take(s.sums, plan.nsum, &sums)) return rc;
  if (int rc = take(s.bytes, 2u * plan.m[1], &a.bytes)) return rc;
  if (int rc = take(s.live, n, &a.live)) return rc;
  if (int rc = take(s.runs, K, &d_runs)) return rc;
  if (int rc = take(s.tiles, std::max<std::uint64_t>(tiles.size(), 1), &d_tiles)) return rc;
  const std::uint64_t rbytes = K * sizeof(MgRun), tbytes = tiles.size() * sizeof(MgTile);
  if (int rc = s.hs.stage(rbytes + tbytes, "sst merge: pinned staging allocation failed")) return rc;
  std::memcpy(s.hs.h, runs.data(), rbytes);
  if (tbytes) std::memcpy(static_cast<std::uint8_t*>(s.hs.h) + rbytes, tiles.data(), tbytes);
  TKV_HIP_RC(hipMemcpyAsync(d_runs, s.hs.h, rbytes, hipMemcpyHostToDevice, st));
  if (tbytes) TKV_HIP_RC(hipMemcpyAsync(d_tiles, static_cast<std::uint8_t*>(s.hs.h) + rbytes, tbytes, hipMemcpyHostToDevice, st));
  a.runs = d_runs;
  a.n_runs = K;
  a.flags = c.flags;
  a.n = n;
  a.st = s.st;
  a.o_key_off = c.out_key_off;
  a.o_key_len = c.out_key_len;
  a.o_val_off = c.out_val_off;
  a.o_val_len = c.out_val_len;
  a.o_src = c.out_src;
  const dim3 tb(kScanThreads);

  // check and sort entries
  PhaseClock clock(st, g_mg.timing != 0, g_mg.phase);
  clock.mark(0);
  s.h_res[7] = 0;
  hipLaunchKernelGGL(mg_init, dim3(1), dim3(64), 0, st, s.st);
  hipLaunchKernelGGL(mg_check, dim3(blocks(n, kScanThreads)), tb, 0, st, a, l[0]);
  clock.mark(1);

  // merge rounds (each does nothing when the check found a bad entry)
  int cur = 0;
  for (std::uint64_t k = 0; k < rounds; ++k) {
    const std::uint64_t nt = first[k + 1] - first[k];
    hipLaunchKernelGGL(mg_round, dim3(static_cast<unsigned>(nt)), dim3(kMgThreads), 0, st, a, l[cur], l[cur ^ 1],
                       static_cast<const MgTile*>(d_tiles + first[k]));
    cur ^= 1;
  }
  clock.mark(2);

  // ties, drop and the survivor scan
  std::uint64_t* lv[kScanLevels + 1];
  plan.place(a.cnt, sums, lv);
  hipLaunchKernelGGL(mg_ties, dim3(static_cast<unsigned>(plan.m[1])), tb, 0, st, a, l[cur], lv[0], lv[1]);
  hipLaunchKernelGGL(mg_sum, dim3(1), tb, 0, st, a, plan.m[1]);
  scan_up(plan, lv, st);
  scan_down(plan, lv, st);
  hipLaunchKernelGGL(mg_publish, dim3(1), dim3(64), 0, st, static_cast<const unsigned long long*>(s.st),
                     static_cast<const std::uint64_t*>(lv[plan.levels]), s.d_hres, std::uint64_t{1});
  clock.mark(3);
  if (int rc = s.wait(st, 7, 1, "sst merge: the scan left no result")) return rc;
  *c.n_entries = *c.keys_bytes = *c.vals_bytes = 0;
  if (s.h_res[0] != ~0ull) {
    const std::uint64_t p = s.h_res[0];
    if (p >= n) return set_error(TKV_IO_ERROR, "sst merge: the check is inconsistent");
    std::uint32_t r = K - 1u;
    while (runs[r].start > p || c.n[r] == 0) --r;  // (the run that holds position p)
    *c.first_bad = (static_cast<std::uint64_t>(r) << 32) | (p - runs[r].start);
    return set_error(TKV_CORRUPTED, "sst merge: a key span is out of bounds or a run is not ascending");
  }
  *c.first_bad = TKV_SST_MERGE_NONE;
  a.m = s.h_res[1];
  if (a.m > n) return set_error(TKV_IO_ERROR, "sst merge: the survivor scan is inconsistent");
  *c.n_entries = a.m;
  *c.keys_bytes = s.h_res[2];
  *c.vals_bytes = s.h_res[3];
  const bool want_cols = a.o_key_off || a.o_key_len || a.o_val_off || a.o_val_len || a.o_src;
  if (want_cols && a.m > c.entry_cap) return set_error(TKV_BUFFER_OVERFLOW, "sst merge: the entries do not fit");

  // emit
  if (want_cols && a.m > 0) {
    hipLaunchKernelGGL(mg_emit, dim3(blocks(n, kScanThreads)), tb, 0, st, a, l[cur]);
    TKV_HIP_RC(hipGetLastError());
  }
  clock.mark(4);
  TKV_HIP_RC(hipStreamSynchronize(st));
  clock.finish();
  g_mg.last[0] = n;
  g_mg.last[1] = rounds;
  g_mg.last[2] = rounds ? first[rounds] - first[rounds - 1u] : 0u;
  g_mg.last[3] = g_mg.taken;
  return TKV_OK;
}

}  // namespace

int sst_merge_device_impl(const SstMergeCall& c, hipStream_t st) {
  g_mg.begin();
  MgScratch* sp = nullptr;
  if (int rc = per_device_scratch(&sp, kMgHres, kMsWords, true)) return rc;
  std::lock_guard<std::mutex> lk(sp->mu);
  return merge_locked(*sp, c, st);
}

}  // namespace tkv

extern "C" {

uint64_t tkv_debug_sst_merge_tile(void) { return tkv::kMgTile; }

void tkv_debug_sst_merge_last(uint64_t out[4]) { tkv::g_mg.get_last(out); }

int tkv_debug_sst_merge_phases(int enable, double out_ms[4]) { return tkv::g_mg.phases(enable, out_ms); }

}  // extern "C"
