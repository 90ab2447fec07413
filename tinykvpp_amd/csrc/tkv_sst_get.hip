// SSTable get on the device (include/tkv_crc32.h "SSTable get"): a batch of user keys
// looked up in K sorted runs of internal keys, oldest first, the newest run that holds a key deciding.
//
// gt_search: one lane per query. The lane checks its query's span, loads the query's comparison word and
//   digit once (tkv_memtable_layout.h), and walks the runs from the highest-numbered one down. In a run of n
//   entries it finds the upper bound of its key in bit_length(n) = ceil(log2(n + 1)) steps, the same count
//   for every lane of the wave: pos = 0; for step = 2^(bits - 1), ..., 2, 1: the entry pos + step - 1 is
//   probed when pos + step <= n, and pos += step when its user key is <= the query. A probe reads the
//   pivot's key_off / key_len, span-checks them (span_ok, tkv_runs_device.h), reads the pivot's word, and
//   goes into cmp_rest only on a (word, digit 9) tie. The last probe a lane accepted is entry pos - 1, so
//   whether it was equal is the hit test; no entry is read twice for it. A lane with a hit is done and
//   idles; a wave leaves the run loop when all its lanes are done. The run table is indexed by the
//   wave-uniform run number (scalar loads). A bad query sets a flag word, a bad probe goes to the verdict
//   word by wave minimum and one atomic minimum, as in the merge. EVERY KERNEL BEHIND THE SEARCH READS
//   BOTH WORDS AND WRITES NOTHING WHEN ONE IS SET. Per query the search leaves {r << 32 | i} and
//   {state << 32 | value length} in scratch.
// gt_lens: level 0 of two u64 scans (tkv_scan.h): FOUND | DELETED << 32 (both counts stay below 2^32) and
//   the FOUND queries' value lengths; the second is out_val_pos and the emit's span table.
// gt_emit: the per-query columns, one lane per query, and the emit's tile table (tile_entries).
// span_emit<GtSrc>: the value gather (tkv_wal_emit.h), the source of span j the hit's value.
// Host synchronisations: two (the verdicts with the sizes; the end of the emit).
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
#include "tkv_wal_emit.h"

namespace tkv {
namespace {

constexpr unsigned kGtThreads = 256;  // queries per workgroup of gt_search
constexpr unsigned kGtHres = 8;       // words of the pinned result block
constexpr std::uint64_t kGtNone = TKV_SST_MERGE_NONE;
constexpr unsigned kGtStateShift = 32;
enum : int { kGsBad = 0, kGsBadQuery, kGsSteps, kGsWords };

// One run as the get's kernels see it: the merge's entry, the value arena and the search's trip count.
struct GtRun {
  MgRun run;
  const std::uint8_t* vals;  // nullable
  std::uint64_t vals_size;
  std::uint32_t n;
  std::uint32_t steps;       // bit_length(n)
};

struct GtArgs {
  const GtRun* runs;
  std::uint32_t n_runs;
  std::uint32_t gather;      // the value span of a FOUND hit is checked
  const std::uint8_t* qkeys;
  std::uint64_t qkeys_size;
  const std::uint64_t* q_off;
  const std::uint32_t* q_len;
  std::uint64_t nq;
  unsigned long long* st;    // kGsWords device words
  std::uint64_t* hit;        // per query: r << 32 | i, kGtNone without a hit
  std::uint64_t* info;       // per query: state << 32 | value length (0 unless FOUND)
  const std::uint64_t* fpre; // exclusive scan of FOUND | DELETED << 32
  std::uint64_t* lpre;       // exclusive scan of the value lengths, nq + 1 entries
  std::uint32_t* tile;       // nullable: the gather's tile table
  std::uint8_t* o_state;
  std::uint64_t* o_src;
  std::uint64_t* o_seq;
  std::uint64_t* o_val_off;
  std::uint32_t* o_val_len;
  std::uint64_t* o_val_pos;
};

__device__ __forceinline__ bool verdict_bad(const unsigned long long* st) {
  return __hip_atomic_load(st + kGsBad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != ~0ull ||
         __hip_atomic_load(st + kGsBadQuery, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull;
}

__global__ void gt_init(unsigned long long* st) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    st[kGsBad] = ~0ull;
    st[kGsBadQuery] = 0;
    st[kGsSteps] = 0;
  }
}

// ---- search -----------------------------------------------------------------------------------------

__global__ __launch_bounds__(kGtThreads) void gt_search(GtArgs a) {
  const std::uint64_t j = blockIdx.x * static_cast<std::uint64_t>(kGtThreads) + threadIdx.x;
  bool done = j >= a.nq, bad_query = false;
  MgKey q{0, 0};
  std::uint64_t qw = 0;
  std::uint32_t qd = 0;
  if (!done) {
    const std::uint64_t qo = a.q_off[j];
    const std::uint32_t ql = a.q_len[j];
    if (qo > a.qkeys_size || ql > a.qkeys_size - qo || ql >= kMtMaxIkey - kMtMeta) {
      bad_query = done = true;
    } else {
      q = MgKey{reinterpret_cast<std::uintptr_t>(a.qkeys) + qo, ql};
      qw = load_word(q.addr, ql);
      qd = mt_digit(ql);
    }
  }
  std::uint32_t bad_r = ~0u, bad_i = ~0u;  // the lane's bad probe (a lane stops at its first)
  std::uint32_t steps = 0, state = TKV_SST_GET_ABSENT, vlen = 0;
  std::uint64_t hit = kGtNone;
  for (std::uint32_t r = a.n_runs; r-- > 0u;) {
    if (__ballot(!done) == 0ull) break;
    const GtRun& g = a.runs[r];  // (r is wave-uniform)
    const std::uint32_t n = g.n;
    if (n == 0u) continue;
    if (!done) steps += g.steps;
    std::uint32_t pos = 0;
    bool eq = false;
    for (std::uint32_t step = 1u << (g.steps - 1u); step != 0u; step >>= 1) {
      const std::uint32_t cand = pos + step;  // <= 2^steps - 1
      if (!done && cand <= n) {
        const std::uint32_t i = cand - 1u;
        const std::uint64_t ko = g.run.key_off[i];
        const std::uint32_t kl = g.run.key_len[i];
        if (!span_ok(g.run, ko, kl)) {
          bad_r = r;
          bad_i = i;
          done = true;
        } else {
          const MgKey k{reinterpret_cast<std::uintptr_t>(g.run.keys) + ko, kl - kMtMeta};
          const std::uint64_t w = load_word(k.addr, k.ulen);
          const std::uint32_t d = mt_digit(k.ulen);
          const int c = w != qw ? (w < qw ? -1 : 1) : d != qd ? (d < qd ? -1 : 1) : d < kMtDigitMore ? 0 : cmp_rest(k, q);
          if (c <= 0) {
            pos = cand;
            eq = c == 0;
          }
        }
      }
    }
    if (!done && eq) {  // (eq: pos >= 1, and entry pos - 1 passed its span check in this search)
      const std::uint32_t i = pos - 1u;
      const bool tomb = g.run.keys[g.run.key_off[i] + g.run.key_len[i] - 1u] != 0;
      hit = (static_cast<std::uint64_t>(r) << 32) | i;
      state = tomb ? TKV_SST_GET_DELETED : TKV_SST_GET_FOUND;
      if (!tomb) {
        vlen = g.run.val_len ? g.run.val_len[i] : 0u;
        const std::uint64_t vo = g.run.val_off ? g.run.val_off[i] : 0ull;
        if (a.gather && (vo > g.vals_size || vlen > g.vals_size - vo)) {
          bad_r = r;
          bad_i = i;
        }
      }
      done = true;
    }
  }
  if (j < a.nq) {
    const bool failed = bad_query || bad_r != ~0u;
    a.hit[j] = failed ? kGtNone : hit;
    a.info[j] = failed ? 0ull : (static_cast<std::uint64_t>(state) << kGtStateShift) | vlen;
  }
  // the verdicts and the debug hook's step count, once per wave and only when there is something to say
  const std::uint32_t wr = dev::wave_min(bad_r);
  const std::uint32_t wi = dev::wave_min(bad_r == wr ? bad_i : ~0u);
  const std::uint32_t ws = dev::wave_max(steps);
  const bool wq = __ballot(bad_query) != 0ull;
  if ((threadIdx.x & 63u) == 0) {
    if (wr != ~0u) atomicMin(a.st + kGsBad, (static_cast<unsigned long long>(wr) << 32) | wi);
    if (wq) atomicMax(a.st + kGsBadQuery, 1ull);
    if (ws > __hip_atomic_load(a.st + kGsSteps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(a.st + kGsSteps, static_cast<unsigned long long>(ws));
  }
}

// ---- scans ------------------------------------------------------------------------------------------

// Level 0 of the scan of the found / deleted flags (which 0) or of the value lengths (which 1).
__global__ __launch_bounds__(kScanThreads) void gt_lens(GtArgs a, int which, std::uint64_t* arr, std::uint64_t* bsum) {
  if (verdict_bad(a.st)) return;
  const std::uint64_t j0 = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
  std::uint64_t v[kScanItems];
#pragma unroll
  for (unsigned k = 0; k < kScanItems; ++k) {
    v[k] = 0;
    if (j0 + k < a.nq) {
      const std::uint64_t inf = a.info[j0 + k];
      const std::uint32_t state = static_cast<std::uint32_t>(inf >> kGtStateShift);
      if (which) v[k] = inf & 0xFFFFFFFFull;
      else v[k] = state == TKV_SST_GET_FOUND ? 1ull : state == TKV_SST_GET_DELETED ? (1ull << 32) : 0ull;
    }
  }
  scan_items(v, j0, a.nq, arr, bsum);
}

__global__ void gt_publish(GtArgs a, const std::uint64_t* flags, const std::uint64_t* bytes, std::uint64_t* h, std::uint64_t tag) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const bool bad = verdict_bad(a.st);
    h[0] = a.st[kGsBad];
    h[1] = a.st[kGsBadQuery];
    h[2] = bad ? 0ull : *flags;
    h[3] = bad ? 0ull : *bytes;
    h[4] = a.st[kGsSteps];
    if (!bad) a.lpre[a.nq] = *bytes;
    __threadfence_system();
    h[7] = tag;
  }
}

// ---- columns and gather -----------------------------------------------------------------------------

__global__ __launch_bounds__(kScanThreads) void gt_emit(GtArgs a) {
  const std::uint64_t j = blockIdx.x * static_cast<std::uint64_t>(kScanThreads) + threadIdx.x;
  if (j >= a.nq || verdict_bad(a.st)) return;
  const std::uint64_t x = a.hit[j], inf = a.info[j];
  const std::uint32_t state = static_cast<std::uint32_t>(inf >> kGtStateShift);
  const std::uint32_t vlen = static_cast<std::uint32_t>(inf);
  std::uint64_t seq = 0, vo = 0;
  if (x != kGtNone) {
    const MgRun& r = a.runs[x >> 32].run;
    const std::uint64_t i = x & kMgIdxMask;
    const std::uint64_t ko = r.key_off[i];
    const std::uint32_t kl = r.key_len[i];
    seq = __builtin_bswap64(load_word(reinterpret_cast<std::uintptr_t>(r.keys) + ko + (kl - kMtMeta) + kMtSeq, 8u));
    if (state == TKV_SST_GET_FOUND) vo = r.val_bias + (r.val_off ? r.val_off[i] : 0ull);
  }
  const std::uint64_t at = a.lpre[j];
  if (a.o_state) a.o_state[j] = static_cast<std::uint8_t>(state);
  if (a.o_src) a.o_src[j] = x;
  if (a.o_seq) a.o_seq[j] = seq;
  if (a.o_val_off) a.o_val_off[j] = vo;
  if (a.o_val_len) a.o_val_len[j] = vlen;
  if (a.o_val_pos) a.o_val_pos[j] = at;
  if (a.tile && vlen) tile_entries(a.tile, j, at, vlen, a.lpre[a.nq]);
}

// Where query j's value lies for the shared emit (only spans with a length are copied: FOUND hits of runs
// with value columns).
struct GtSrc {
  const GtRun* runs;
  const std::uint64_t* hit;
  __device__ __forceinline__ std::uintptr_t operator()(std::uint64_t j) const {
    const std::uint64_t x = hit[j];
    if (x == kGtNone) return 0;
    const GtRun& g = runs[x >> 32];
    return reinterpret_cast<std::uintptr_t>(g.vals) + static_cast<std::uintptr_t>(g.run.val_off ? g.run.val_off[x & kMgIdxMask] : 0ull);
  }
};

// ---- host side --------------------------------------------------------------------------------------

// Per-device scratch, grown by doubling and kept between calls (guarded by mu).
struct GtScratch : ScratchBase {
  DeviceBuf hit, info, fpre, lpre, sums, runs, tile;
  RunStage hs;  // pinned staging of the run table
  unsigned long long*& st = words;
};

// The calling thread's device gets (tkv_debug_sst_get_last, tkv_debug_sst_get_phases).
thread_local PathStats g_gt;
thread_local std::uint64_t g_gt_last[5] = {0, 0, 0, 0, 0};

template <class T>
int take(DeviceBuf& b, std::uint64_t want, T** out) {
  return tkv::take(b, want, out, g_gt.taken, "sst get: scratch allocation failed");
}

std::uint32_t bit_length(std::uint64_t n) {
  std::uint32_t b = 0;
  for (; n; n >>= 1) ++b;
  return b;
}

int get_locked(GtScratch& s, const SstGetCall& c, hipStream_t st) {
  const std::uint32_t K = c.n_runs;
  const std::uint64_t nq = c.nq;
  const bool gather = c.vals != nullptr;
  std::vector<GtRun> runs(std::max<std::uint32_t>(K, 1u));
  for (std::uint32_t r = 0; r < K; ++r) {
    GtRun& g = runs[r];
    g = GtRun{};
    if (c.n[r] == 0) continue;
    g.run.keys = c.keys[r];
    g.run.keys_size = c.keys_size[r];
    g.run.key_off = c.key_off[r];
    g.run.key_len = c.key_len[r];
    g.run.val_off = c.val_off ? c.val_off[r] : nullptr;
    g.run.val_len = c.val_len ? c.val_len[r] : nullptr;  // (never without val_off: the caller's check)
    g.run.val_bias = c.val_bias ? c.val_bias[r] : 0u;
    g.vals = gather ? c.vals[r] : nullptr;
    g.vals_size = gather && c.vals[r] ? c.vals_size[r] : 0u;
    g.n = static_cast<std::uint32_t>(c.n[r]);
    g.steps = bit_length(c.n[r]);
  }

  GtArgs a{};
  GtRun* d_runs = nullptr;
  std::uint64_t *fpre = nullptr, *sums = nullptr;
  const ScanPlan plan(nq);
  if (int rc = take(s.hit, nq, &a.hit)) return rc;
  if (int rc = take(s.info, nq, &a.info)) return rc;
  if (int rc = take(s.fpre, nq, &fpre)) return rc;
  if (int rc = take(s.lpre, nq + 1u, &a.lpre)) return rc;
  if (int rc = take(s.sums, 2u * plan.nsum, &sums)) return rc;
  if (int rc = take(s.runs, runs.size(), &d_runs)) return rc;
  const std::uint64_t rbytes = runs.size() * sizeof(GtRun);
  if (int rc = s.hs.stage(rbytes, "sst get: pinned staging allocation failed")) return rc;
  std::memcpy(s.hs.h, runs.data(), rbytes);
  TKV_HIP_RC(hipMemcpyAsync(d_runs, s.hs.h, rbytes, hipMemcpyHostToDevice, st));
  a.runs = d_runs;
  a.n_runs = K;
  a.gather = gather ? 1u : 0u;
  a.qkeys = c.qkeys;
  a.qkeys_size = c.qkeys_size;
  a.q_off = c.q_off;
  a.q_len = c.q_len;
  a.nq = nq;
  a.st = s.st;
  a.fpre = fpre;
  a.o_state = c.state;
  a.o_src = c.src;
  a.o_seq = c.seq;
  a.o_val_off = c.out_val_off;
  a.o_val_len = c.out_val_len;
  a.o_val_pos = c.out_val_pos;
  const dim3 tb(kScanThreads);

  // search
  PhaseClock clock(st, g_gt.timing != 0, g_gt.phase);
  clock.mark(0);
  s.h_res[7] = 0;
  hipLaunchKernelGGL(gt_init, dim3(1), dim3(64), 0, st, s.st);
  hipLaunchKernelGGL(gt_search, dim3(blocks(nq, kGtThreads)), dim3(kGtThreads), 0, st, a);
  clock.mark(1);

  // the two scans (each level does nothing on a bad verdict)
  std::uint64_t *lvF[kScanLevels + 1], *lvL[kScanLevels + 1];
  plan.place(fpre, sums, lvF);
  plan.place(a.lpre, sums + plan.nsum, lvL);
  const dim3 g0(static_cast<unsigned>(plan.m[1]));
  hipLaunchKernelGGL(gt_lens, g0, tb, 0, st, a, 0, lvF[0], lvF[1]);
  scan_up(plan, lvF, st);
  scan_down(plan, lvF, st);
  hipLaunchKernelGGL(gt_lens, g0, tb, 0, st, a, 1, lvL[0], lvL[1]);
  scan_up(plan, lvL, st);
  scan_down(plan, lvL, st);
  hipLaunchKernelGGL(gt_publish, dim3(1), dim3(64), 0, st, a, static_cast<const std::uint64_t*>(lvF[plan.levels]),
                     static_cast<const std::uint64_t*>(lvL[plan.levels]), s.d_hres, std::uint64_t{1});
  clock.mark(2);
  if (int rc = s.wait(st, 7, 1, "sst get: the scan left no result")) return rc;
  if (s.h_res[1] != 0) return set_error(TKV_INVALID_ARGUMENT, "sst get: a query reaches past qkeys_size or is 2^28 - 17 bytes or longer");
  *c.n_found = *c.vals_bytes = 0;
  *c.first_bad = kGtNone;
  if (s.h_res[0] != ~0ull) {
    *c.first_bad = s.h_res[0];
    return set_error(TKV_CORRUPTED, "sst get: a probed entry's key span or a hit's value span is out of bounds");
  }
  const std::uint64_t found = s.h_res[2] & 0xFFFFFFFFull, deleted = s.h_res[2] >> 32, total = s.h_res[3];
  if (found + deleted > nq) return set_error(TKV_IO_ERROR, "sst get: the scan is inconsistent");
  *c.n_found = found;
  *c.vals_bytes = total;
  if (c.out_vals && total > c.vals_cap) return set_error(TKV_BUFFER_OVERFLOW, "sst get: the values do not fit");

  // columns and gather
  const bool copy = gather && c.out_vals && total > 0;
  const bool want_cols = c.state || c.src || c.seq || c.out_val_off || c.out_val_len || c.out_val_pos;
  if (copy) {
    if (int rc = take(s.tile, 2u * ((total + kDecTile - 1u) / kDecTile), &a.tile)) return rc;
  }
  if (want_cols || copy) {
    hipLaunchKernelGGL(gt_emit, dim3(blocks(nq, kScanThreads)), tb, 0, st, a);
    TKV_HIP_RC(hipGetLastError());
  }
  clock.mark(3);
  if (copy) {
    EmitArgs<GtSrc> e{};
    e.src = GtSrc{d_runs, a.hit};
    e.pre = a.lpre;
    e.dst = c.out_vals;
    e.total = total;
    e.tile = a.tile;
    e.n = nq;
    (void)launch_span_emit(s.ncu, e, st);
    TKV_HIP_RC(hipGetLastError());
  }
  clock.mark(4);
  TKV_HIP_RC(hipStreamSynchronize(st));
  clock.finish();
  g_gt_last[0] = nq;
  g_gt_last[1] = K;
  g_gt_last[2] = s.h_res[4];
  g_gt_last[3] = found;
  g_gt_last[4] = deleted;
  return TKV_OK;
}

}  // namespace

int sst_get_device_impl(const SstGetCall& c, hipStream_t st) {
  g_gt.begin();
  for (auto& v : g_gt_last) v = 0;
  GtScratch* sp = nullptr;
  if (int rc = per_device_scratch(&sp, kGtHres, kGsWords, true)) return rc;
  std::lock_guard<std::mutex> lk(sp->mu);
  return get_locked(*sp, c, st);
}

}  // namespace tkv

extern "C" {

void tkv_debug_sst_get_geometry(uint64_t out[1]) { out[0] = tkv::kGtThreads; }

void tkv_debug_sst_get_last(uint64_t out[5]) {
  for (int i = 0; i < 5; ++i) out[i] = tkv::g_gt_last[i];
}

int tkv_debug_sst_get_phases(int enable, double out_ms[4]) { return tkv::g_gt.phases(enable, out_ms); }

}  // extern "C"
