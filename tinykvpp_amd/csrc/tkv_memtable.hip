// Memtable replay on the device (include/tkv_crc32.h "Memtable replay"): the content a
// skiplist holds after engine::create's replay loop inserted a whole decoded WAL batch, in iteration
// order: one internal key per distinct user key, ascending, the record latest in the batch surviving.
//
// The order is found by most-significant-word refinement, every round a stable LSD radix sort:
// mt_check: one lane per record: the op, length and bounds checks (first_bad by a wave minimum and an
//   atomic minimum, the argument verdict by an atomic OR) and the round's list entry {word, seg | digit,
//   record}: word = key bytes [0, 8) big-endian, zero-padded, digit = min(key_len, 9)
//   (tkv_memtable_layout.h). The OR and the AND of all words are reduced beside it: a bit in which they
//   agree is the same in every entry, and a radix pass whose 8 bits all agree would put every entry into
//   one bucket and is skipped (common prefixes, short keys, few segments).
// mt_pass: one radix pass over the list, 4096 entries per workgroup, entry order = (wave, step, lane).
//   A lane's rank among the equal digits of its step comes from ballots over the digit's bits, the count
//   of the steps before it from a per-wave LDS row only that wave touches, the waves before it from a
//   sum over the rows: no atomics, so the order within a bucket is the entry order and the pass is
//   stable. Mode 0 writes the workgroup's bucket sizes to the digit-major matrix hist[digit][workgroup],
//   whose u64 exclusive scan (scan_level / scan_add, tkv_scan.h) is every bucket's base, mode 1
//   scatters to it; mode 2 does both for a list that fits one workgroup. The scatter first puts the
//   workgroup's entries into bucket order in LDS and stores from there, so that neighbouring lanes store
//   to neighbouring addresses of a bucket.
// mt_ties: the sorted list back into the positions its entries came from (perm), and what the round
//   decided: neighbours equal in segment, word and digit are equal keys when the digit says the key ends
//   here (eqn marks the pair), and form a segment of the next round when it says the key goes on. The
//   flags {enters the next round, starts a segment} are scanned as one u64 (two u32 counts).
// mt_compact: the next round's list, in position order (so that equal keys stay in input order): segment
//   number, the next word of every entry, the positions they will be written back to.
// Rounds end when no entry enters the next one: at most ceil(max key_len / 8) + 1 rounds, each over the
// unresolved entries only. One host synchronisation per round (the list size and the skip mask).
// mt_survivors + scans: position j survives when the key at j + 1 differs (the latest of a run of equal
//   keys: the sort is stable); the survivors' count and the u64 prefix of key_len + 17.
// mt_columns: the caller's columns, the 17 metadata bytes of every entry staged in scratch, and the
//   arena's spans (two per entry: the user key where it lies, the metadata) with their tiles; span_emit
//   (tkv_wal_emit.h) writes the arena, one wave per 4 KiB tile, at any destination alignment.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>

#include "tkv_crc32.h"
#include "tkv_crc32_device.h"
#include "tkv_device_util.h"
#include "tkv_engine.h"
#include "tkv_key_word.h"
#include "tkv_memtable_layout.h"
#include "tkv_scan.h"
#include "tkv_wal_copy.h"
#include "tkv_wal_emit.h"

namespace tkv {
namespace {

constexpr unsigned kMtWaves = 16;                      // waves per workgroup of a radix pass
constexpr unsigned kMtThreads = 64 * kMtWaves;
constexpr unsigned kMtSteps = 4;                       // entries per lane
constexpr std::uint64_t kMtTile = static_cast<std::uint64_t>(kMtThreads) * kMtSteps;  // entries per workgroup
constexpr unsigned kMtBuckets = 256;
constexpr int kMtPasses = 13;                          // digit (4 bits), 8 word bytes, 4 segment bytes
constexpr unsigned kMtHres = 8;                        // words of the pinned result block
constexpr std::uint32_t kMtStage = 24;                 // scratch bytes an entry's 17 metadata bytes are staged in
static_assert(kMtStage >= kMtMeta && kMtStage % 8 == 0, "aligned u64 stores");
enum : unsigned long long { kFlagBounds = 1, kFlagLen = 2 };
enum : int { kStBad = 0, kStFlags, kStOrW, kStAndW, kStOrX, kStAndX, kStWords };
static_assert(kMtThreads >= kMtBuckets, "one thread per bucket");

// A round's list: the comparison word, segment << 4 | digit, the record.
struct List {
  std::uint64_t* kw;
  std::uint64_t* kx;
  std::uint32_t* rec;
};

struct MtArgs {
  const std::uint8_t* keys;
  std::uint64_t keys_size;
  const std::uint64_t* key_off;
  const std::uint32_t* key_len;
  const std::uint64_t* val_off;  // nullable
  const std::uint32_t* val_len;  // nullable: every value empty
  const std::uint8_t* op;        // nullable: every record a put
  const std::uint8_t* tomb;      // nullable: 0
  const std::uint64_t* seq;      // nullable: 0
  std::uint64_t n;
  std::uint64_t ts;
  std::uint32_t* perm;           // the record at every sorted position
  std::uint32_t* eqn;            // 1: the keys at positions j and j + 1 are equal
  unsigned long long* st;        // kStWords device words
  std::uint64_t* cnt;            // exclusive scan of the survivor flags
  std::uint64_t* len;            // exclusive scan of the survivors' key_len + 17
  // the emit
  std::uint32_t* esrc;           // the surviving record of every entry
  std::uint64_t* pre;            // 2 m + 1 span offsets in the arena
  std::uint8_t* meta;            // kMtStage bytes per entry, the first 17 the metadata
  std::uint32_t* tile;
  std::uint64_t m, total;
  std::uint8_t* o_ikeys;         // the caller's outputs, each nullable
  std::uint64_t* o_ikey_off;
  std::uint32_t* o_ikey_len;
  std::uint64_t* o_val_off;
  std::uint32_t* o_val_len;
  std::uint32_t* o_src;
};

// OR (AND) of v over the 64 lanes, wave-uniform: the DPP pattern of dev::wave_max.
template <bool AND>
__device__ __forceinline__ std::uint32_t wave_bits32(std::uint32_t v) {
  constexpr int id = AND ? -1 : 0;
  auto op = [](std::uint32_t x, int y) { return AND ? x & static_cast<std::uint32_t>(y) : x | static_cast<std::uint32_t>(y); };
  v = op(v, __builtin_amdgcn_update_dpp(id, static_cast<int>(v), 0xB1, 0xF, 0xF, false));
  v = op(v, __builtin_amdgcn_update_dpp(id, static_cast<int>(v), 0x4E, 0xF, 0xF, false));
  v = op(v, __builtin_amdgcn_update_dpp(id, static_cast<int>(v), 0x141, 0xF, 0xF, false));
  v = op(v, __builtin_amdgcn_update_dpp(id, static_cast<int>(v), 0x140, 0xF, 0xF, false));
  v = op(v, __builtin_amdgcn_update_dpp(id, static_cast<int>(v), 0x142, 0xA, 0xF, false));
  v = op(v, __builtin_amdgcn_update_dpp(id, static_cast<int>(v), 0x143, 0xC, 0xF, false));
  return static_cast<std::uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), 63));
}
template <bool AND>
__device__ __forceinline__ std::uint64_t wave_bits(std::uint64_t v) {
  return (static_cast<std::uint64_t>(wave_bits32<AND>(static_cast<std::uint32_t>(v >> 32))) << 32) |
         wave_bits32<AND>(static_cast<std::uint32_t>(v));
}

// The wave's entries into the round's OR / AND words (lanes without an entry pass on = false).
__device__ __forceinline__ void fold_bits(unsigned long long* st, bool on, std::uint64_t kw, std::uint64_t kx) {
  const std::uint64_t ow = wave_bits<false>(on ? kw : 0ull), aw = wave_bits<true>(on ? kw : ~0ull);
  const std::uint64_t ox = wave_bits<false>(on ? kx : 0ull), ax = wave_bits<true>(on ? kx : ~0ull);
  if ((threadIdx.x & 63u) == 0) {
    // An OR only gains bits and an AND only loses them, so a word read earlier that this wave would not
    // change is one the atomic would not change either: most waves send none (atomics on one address
    // serialise in L2, and every wave of a list would send four).
    auto seen = [&](int k) { return __hip_atomic_load(st + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    const unsigned long long sow = seen(kStOrW), saw = seen(kStAndW), sox = seen(kStOrX), sax = seen(kStAndX);
    if ((sow | ow) != sow) atomicOr(st + kStOrW, static_cast<unsigned long long>(ow));
    if ((saw & aw) != saw) atomicAnd(st + kStAndW, static_cast<unsigned long long>(aw));
    if ((sox | ox) != sox) atomicOr(st + kStOrX, static_cast<unsigned long long>(ox));
    if ((sax & ax) != sax) atomicAnd(st + kStAndX, static_cast<unsigned long long>(ax));
  }
}

// (load_word, the comparison word's key read: tkv_key_word.h)

// The 8 bits pass p sorts by (p = 0: the digit's 4), and whether they differ anywhere in the list.
__host__ __device__ inline std::uint32_t pass_digit(int p, std::uint64_t kw, std::uint64_t kx) {
  if (p == 0) return static_cast<std::uint32_t>(kx & ((1u << kMtDigitBits) - 1u));
  if (p <= 8) return static_cast<std::uint32_t>((kw >> (8 * (p - 1))) & 0xFFu);
  return static_cast<std::uint32_t>((kx >> (kMtDigitBits + 8 * (p - 9))) & 0xFFu);
}

// ---- check and first word ---------------------------------------------------------------------------

__global__ void mt_init(unsigned long long* st) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    st[kStBad] = ~0ull;
    st[kStFlags] = 0;
    st[kStOrW] = 0;
    st[kStAndW] = ~0ull;
    st[kStOrX] = 0;
    st[kStAndX] = ~0ull;
  }
}

__global__ __launch_bounds__(kScanThreads) void mt_check(MtArgs a, List l) {
  const std::uint64_t i = blockIdx.x * static_cast<std::uint64_t>(kScanThreads) + threadIdx.x;
  const bool act = i < a.n;
  std::uint32_t bad = ~0u;
  unsigned long long flags = 0;
  std::uint64_t kw = 0, kx = 0;
  if (act) {
    const std::uint64_t ko = a.key_off[i];
    const std::uint32_t kl = a.key_len[i];
    if (a.op && a.op[i] > kMtOpDel) bad = static_cast<std::uint32_t>(i);
    if (kl >= kMtMaxIkey - kMtMeta) flags |= kFlagLen;
    if (ko > a.keys_size || kl > a.keys_size - ko) flags |= kFlagBounds;
    if (!flags) kw = load_word(reinterpret_cast<std::uintptr_t>(a.keys) + ko, kl);
    kx = mt_digit(kl);
    l.kw[i] = kw;
    l.kx[i] = kx;
    l.rec[i] = static_cast<std::uint32_t>(i);
  }
  const std::uint32_t wbad = dev::wave_min(bad);
  const std::uint32_t wflags = wave_bits32<false>(static_cast<std::uint32_t>(flags));
  if ((threadIdx.x & 63u) == 0) {
    if (wbad != ~0u) atomicMin(a.st + kStBad, static_cast<unsigned long long>(wbad));
    if (wflags) atomicOr(a.st + kStFlags, static_cast<unsigned long long>(wflags));
  }
  fold_bits(a.st, act, kw, kx);
}

// The round's result for the host, and the OR / AND words cleared for the next list. next = the scan
// total {entries of the next round, its segments << 32}, nullptr after the check.
__global__ void mt_publish(unsigned long long* st, const std::uint64_t* next, std::uint64_t* h, std::uint64_t tag) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    h[0] = st[kStBad];
    h[1] = st[kStFlags];
    h[2] = st[kStOrW] ^ st[kStAndW];
    h[3] = st[kStOrX] ^ st[kStAndX];
    h[4] = next ? *next : 0;
    st[kStOrW] = 0;
    st[kStAndW] = ~0ull;
    st[kStOrX] = 0;
    st[kStAndX] = ~0ull;
    __threadfence_system();
    h[7] = tag;
  }
}

// ---- one radix pass ---------------------------------------------------------------------------------

// MODE 0: the workgroup's bucket sizes to hist[digit * nblk + workgroup]. MODE 1: the scatter, hist now
// holding every bucket's base. MODE 2: both, for a list of one workgroup.
template <int MODE>
__global__ __launch_bounds__(kMtThreads) void mt_pass(List in, List out, std::uint64_t m, int p, std::uint64_t* hist,
                                                      std::uint32_t nblk) {
  __shared__ std::uint32_t cnt[kMtWaves][kMtBuckets];
  __shared__ std::uint64_t gbase[kMtBuckets];
  const std::uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const std::uint32_t lane = threadIdx.x & 63u;
  for (std::uint32_t k = threadIdx.x; k < kMtWaves * kMtBuckets; k += kMtThreads) (&cnt[0][0])[k] = 0u;
  __syncthreads();
  const std::uint64_t base = blockIdx.x * kMtTile + static_cast<std::uint64_t>(wv) * (kMtSteps * 64u);
  const std::uint64_t below = (1ull << lane) - 1ull;
  std::uint32_t dg[kMtSteps], rk[kMtSteps];
  std::uint64_t kw[kMtSteps], kx[kMtSteps];
  std::uint32_t rec[kMtSteps];
#pragma unroll
  for (unsigned s = 0; s < kMtSteps; ++s) {
    const std::uint64_t i = base + s * 64u + lane;
    const bool act = i < m;
    kw[s] = act ? in.kw[i] : 0ull;
    kx[s] = act ? in.kx[i] : 0ull;
    if (MODE != 0) rec[s] = act ? in.rec[i] : 0u;
    const std::uint32_t d = pass_digit(p, kw[s], kx[s]);
    // the lanes of this step with the same digit
    std::uint64_t same = __ballot(act);
#pragma unroll
    for (unsigned b = 0; b < 8u; ++b) {
      const bool bit = (d >> b) & 1u;
      const std::uint64_t bal = __ballot(bit);
      same &= bit ? bal : ~bal;
    }
    const std::uint32_t prior = act ? cnt[wv][d] : 0u;  // this wave's earlier steps
    wave_sync();
    if (act && (same & below) == 0ull) cnt[wv][d] = prior + static_cast<std::uint32_t>(__popcll(same));
    wave_sync();
    dg[s] = d;
    rk[s] = prior + static_cast<std::uint32_t>(__popcll(same & below));
  }
  __syncthreads();
  // bucket t: the waves' counts to their exclusive prefix over the waves, the sum to the matrix
  std::uint32_t sum = 0;
  if (threadIdx.x < kMtBuckets) {
#pragma unroll
    for (unsigned w = 0; w < kMtWaves; ++w) {
      const std::uint32_t c = cnt[w][threadIdx.x];
      cnt[w][threadIdx.x] = sum;
      sum += c;
    }
    if (MODE == 0) hist[static_cast<std::uint64_t>(threadIdx.x) * nblk + blockIdx.x] = sum;
  }
  if constexpr (MODE != 0) {
    // the workgroup's entries in bucket order through LDS, so that neighbouring lanes store to
    // neighbouring addresses of a bucket
    __shared__ std::uint64_t s_kw[kMtTile];
    __shared__ std::uint64_t s_kx[kMtTile];
    __shared__ std::uint32_t s_rec[kMtTile];
    __shared__ std::uint32_t lbase[kMtBuckets];
    std::uint32_t all;
    const std::uint32_t pre = dev::block_prefix<std::uint32_t, kMtThreads>(sum, &all);  // buckets before this one
    if (threadIdx.x < kMtBuckets) {
      lbase[threadIdx.x] = pre;
      gbase[threadIdx.x] = MODE == 2 ? pre : hist[static_cast<std::uint64_t>(threadIdx.x) * nblk + blockIdx.x];
    }
    __syncthreads();
#pragma unroll
    for (unsigned s = 0; s < kMtSteps; ++s) {
      if (base + s * 64u + lane < m) {
        const std::uint32_t lp = lbase[dg[s]] + cnt[wv][dg[s]] + rk[s];
        if (lp < kMtTile) {  // (always: the bucket bases and ranks partition the workgroup's entries)
          s_kw[lp] = kw[s];
          s_kx[lp] = kx[s];
          s_rec[lp] = rec[s];
        }
      }
    }
    __syncthreads();
    const std::uint64_t first = blockIdx.x * kMtTile;
    const std::uint32_t have = static_cast<std::uint32_t>(m - first < kMtTile ? m - first : kMtTile);
    for (std::uint32_t j = threadIdx.x; j < have; j += kMtThreads) {
      const std::uint64_t w = s_kw[j], x = s_kx[j];
      const std::uint32_t d = pass_digit(p, w, x);
      const std::uint64_t dst = gbase[d] + (j - lbase[d]);
      if (dst < m) {  // (always)
        out.kw[dst] = w;
        out.kx[dst] = x;
        out.rec[dst] = s_rec[j];
      }
    }
  }
}

// ---- what a round decided ---------------------------------------------------------------------------

struct Tie {
  bool enter, start, equal_next;
};
// Entry k of the sorted list against its neighbours.
__device__ __forceinline__ Tie tie_of(const List& l, std::uint64_t k, std::uint64_t m) {
  const std::uint64_t w = l.kw[k], x = l.kx[k];
  const bool prev = k > 0 && l.kw[k - 1u] == w && l.kx[k - 1u] == x;
  const bool next = k + 1u < m && l.kw[k + 1u] == w && l.kx[k + 1u] == x;
  const bool more = (x & ((1u << kMtDigitBits) - 1u)) == kMtDigitMore;
  Tie t;
  t.enter = more && (prev || next);
  t.start = t.enter && !prev;
  t.equal_next = next && !more;
  return t;
}

// Level 0 of the scan of {enter, start << 32} over the sorted list, the entries back to their positions
// (apos == nullptr: the list is all positions) and the marks of equal keys.
__global__ __launch_bounds__(kScanThreads) void mt_ties(MtArgs a, List l, const std::uint32_t* apos, std::uint64_t m,
                                                        std::uint64_t* arr, std::uint64_t* bsum) {
  const std::uint64_t k0 = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
  std::uint64_t v[kScanItems];
#pragma unroll
  for (unsigned q = 0; q < kScanItems; ++q) {
    const std::uint64_t k = k0 + q;
    v[q] = 0;
    if (k < m) {
      const Tie t = tie_of(l, k, m);
      const std::uint64_t pos = apos ? apos[k] : k;
      a.perm[pos] = l.rec[k];
      if (t.equal_next) a.eqn[pos] = 1u;
      v[q] = (t.enter ? 1ull : 0ull) | (t.start ? 1ull << 32 : 0ull);
    }
  }
  scan_items(v, k0, m, arr, bsum);
}

// The list of the round that compares key bytes [skip, skip + 8).
__global__ __launch_bounds__(kScanThreads) void mt_compact(MtArgs a, List l, const std::uint32_t* apos, std::uint64_t m,
                                                           const std::uint64_t* arr, std::uint64_t skip, List nl,
                                                           std::uint32_t* napos) {
  const std::uint64_t k = blockIdx.x * static_cast<std::uint64_t>(kScanThreads) + threadIdx.x;
  bool on = false;
  std::uint64_t kw = 0, kx = 0;
  if (k < m) {
    const Tie t = tie_of(l, k, m);
    if (t.enter) {
      on = true;
      const std::uint64_t sc = arr[k];
      const std::uint64_t to = sc & 0xFFFFFFFFull;
      const std::uint64_t seg = (sc >> 32) + (t.start ? 1u : 0u) - 1u;
      const std::uint32_t r = l.rec[k];
      const std::uint64_t rem = a.key_len[r] - skip;  // > 0: the digit said the key goes on
      kw = load_word(reinterpret_cast<std::uintptr_t>(a.keys) + a.key_off[r] + skip, rem);
      kx = (seg << kMtDigitBits) | mt_digit(rem);
      nl.kw[to] = kw;
      nl.kx[to] = kx;
      nl.rec[to] = r;
      napos[to] = apos ? apos[k] : static_cast<std::uint32_t>(k);
    }
  }
  fold_bits(a.st, on, kw, kx);
}

// ---- dedupe -----------------------------------------------------------------------------------------

// Level 0 of a scan over the positions: which = 0 the survivor flags to a.cnt, 1 their key_len + 17 to
// a.len.
__global__ __launch_bounds__(kScanThreads) void mt_survivors(MtArgs a, int which, std::uint64_t* bsum) {
  const std::uint64_t j0 = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
  std::uint64_t v[kScanItems];
#pragma unroll
  for (unsigned q = 0; q < kScanItems; ++q) {
    const std::uint64_t j = j0 + q;
    v[q] = 0;
    if (j < a.n && !a.eqn[j]) v[q] = which ? static_cast<std::uint64_t>(a.key_len[a.perm[j]]) + kMtMeta : 1ull;
  }
  scan_items(v, j0, a.n, which ? a.len : a.cnt, bsum);
}

__global__ void mt_publish_sizes(const std::uint64_t* cnt_top, const std::uint64_t* len_top, std::uint64_t* h,
                                 std::uint64_t tag) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    h[0] = *cnt_top;
    h[1] = *len_top;
    __threadfence_system();
    h[7] = tag;
  }
}

// The columns, the staged metadata and the arena's spans of every survivor.
__global__ __launch_bounds__(kScanThreads) void mt_columns(MtArgs a) {
  const std::uint64_t j = blockIdx.x * static_cast<std::uint64_t>(kScanThreads) + threadIdx.x;
  if (j >= a.n || a.eqn[j]) return;
  const std::uint64_t e = a.cnt[j], off = a.len[j];
  if (e >= a.m) return;  // (cannot happen: m is the scan's own total)
  const std::uint32_t r = a.perm[j];
  const std::uint32_t kl = a.key_len[r];
  const bool del = a.op && a.op[r] == kMtOpDel;
  if (a.o_ikey_off) a.o_ikey_off[e] = off;
  if (a.o_ikey_len) a.o_ikey_len[e] = kl + kMtMeta;
  if (a.o_val_off) a.o_val_off[e] = a.val_off ? a.val_off[r] : 0ull;
  if (a.o_val_len) a.o_val_len[e] = (del || !a.val_len) ? 0u : a.val_len[r];
  if (a.o_src) a.o_src[e] = r;
  if (!a.o_ikeys) return;
  a.esrc[e] = r;
  a.pre[2u * e] = off;
  a.pre[2u * e + 1u] = off + kl;
  if (e + 1u == a.m) a.pre[2u * a.m] = a.total;
  // (little-endian words: three aligned stores, not 17 bytewise ones)
  std::uint64_t* const stage = reinterpret_cast<std::uint64_t*>(a.meta + kMtStage * e);
  stage[0] = a.seq ? a.seq[r] : 0ull;
  stage[1] = a.ts;
  stage[2] = (a.tomb && a.tomb[r] != 0) ? 1ull : 0ull;
  if (kl) tile_entries(a.tile, 2u * e, off, kl, a.total);
  tile_entries(a.tile, 2u * e + 1u, off + kl, kMtMeta, a.total);
}

// Span 2 e is entry e's user key where the caller holds it, span 2 e + 1 its staged metadata.
struct MtSrc {
  const std::uint8_t* keys;
  const std::uint64_t* key_off;
  const std::uint32_t* esrc;
  const std::uint8_t* meta;
  __device__ __forceinline__ std::uintptr_t operator()(std::uint64_t i) const {
    const std::uint64_t e = i >> 1;
    return (i & 1u) ? reinterpret_cast<std::uintptr_t>(meta) + kMtStage * e
                    : reinterpret_cast<std::uintptr_t>(keys) + key_off[esrc[e]];
  }
};

// ---- host side --------------------------------------------------------------------------------------

// Per-device scratch, grown by doubling and kept between calls (guarded by mu).
struct MtScratch : ScratchBase {
  DeviceBuf kw[2], kx[2], rec[2], apos[2];  // the lists (ping-pong) and the positions of their entries
  DeviceBuf perm, eqn, scan, sums_a, sums_b, hist, hsums;
  DeviceBuf pre, meta, tile;
  unsigned long long*& st = words;
};

// The calling thread's device builds (tkv_debug_memtable_last, tkv_debug_memtable_phases).
thread_local PathStats g_mt;
// Which passes the calling thread's last device build launched (tkv_debug_memtable_passes): bit p of [0]
// for a pass one workgroup ran, of [1] for one run as histogram, scan and scatter; [2] the passes run,
// [3] the deepest histogram scan. Written by sort_list only.
thread_local std::uint64_t g_mt_passes[4] = {0, 0, 0, 0};

template <class T>
int take(DeviceBuf& b, std::uint64_t want, T** out) {
  return tkv::take(b, want, out, g_mt.taken, "memtable build: scratch allocation failed");
}

// In-place exclusive scan whose level 0 has been launched: the levels above it, then the bases back down.
void scan_rest(const ScanPlan& plan, std::uint64_t* const* lv, hipStream_t st) {
  scan_up(plan, lv, st);
  scan_down(plan, lv, st);
}

// The stable sort of the m entries of l[cur] by the passes whose bits differ somewhere; returns the list
// that holds the result.
int sort_list(const List* l, int cur, std::uint64_t m, std::uint64_t diffw, std::uint64_t diffx, std::uint64_t* hist,
              std::uint64_t* hsums, hipStream_t st) {
  const std::uint64_t nblk = (m + kMtTile - 1u) / kMtTile;
  for (int p = 0; p < kMtPasses; ++p) {
    if (pass_digit(p, diffw, diffx) == 0u) continue;
    if (nblk == 1) {
      hipLaunchKernelGGL(mt_pass<2>, dim3(1), dim3(kMtThreads), 0, st, l[cur], l[cur ^ 1], m, p, hist, 1u);
      g_mt_passes[0] |= 1ull << p;
    } else {
      const ScanPlan plan(kMtBuckets * nblk);
      g_mt_passes[1] |= 1ull << p;
      g_mt_passes[3] = std::max<std::uint64_t>(g_mt_passes[3], static_cast<std::uint64_t>(plan.levels));
      std::uint64_t* lv[kScanLevels + 1];
      plan.place(hist, hsums, lv);
      const dim3 g(static_cast<unsigned>(nblk)), tb(kMtThreads);
      hipLaunchKernelGGL(mt_pass<0>, g, tb, 0, st, l[cur], l[cur ^ 1], m, p, hist, static_cast<std::uint32_t>(nblk));
      hipLaunchKernelGGL(scan_level, dim3(static_cast<unsigned>(plan.m[1])), dim3(kScanThreads), 0, st, lv[0], plan.m[0], lv[1]);
      scan_rest(plan, lv, st);
      hipLaunchKernelGGL(mt_pass<1>, g, tb, 0, st, l[cur], l[cur ^ 1], m, p, hist, static_cast<std::uint32_t>(nblk));
    }
    ++g_mt_passes[2];
    cur ^= 1;
  }
  return cur;
}

int build_locked(MtScratch& s, MtArgs a, const MemtableCall& c, hipStream_t st) {
  const std::uint64_t n = a.n;
  List l[2];
  std::uint32_t* apos[2];
  for (int k = 0; k < 2; ++k) {
    if (int rc = take(s.kw[k], n, &l[k].kw)) return rc;
    if (int rc = take(s.kx[k], n, &l[k].kx)) return rc;
    if (int rc = take(s.rec[k], n, &l[k].rec)) return rc;
    if (int rc = take(s.apos[k], n, &apos[k])) return rc;
  }
  if (int rc = take(s.perm, n, &a.perm)) return rc;
  if (int rc = take(s.eqn, n, &a.eqn)) return rc;
  const ScanPlan plan(n);
  const std::uint64_t nblk = (n + kMtTile - 1u) / kMtTile;
  const ScanPlan hplan(kMtBuckets * nblk);
  std::uint64_t *scan = nullptr, *sums_a = nullptr, *sums_b = nullptr, *hist = nullptr, *hsums = nullptr;
  if (int rc = take(s.scan, n, &scan)) return rc;
  if (int rc = take(s.sums_a, plan.nsum, &sums_a)) return rc;
  if (int rc = take(s.sums_b, plan.nsum, &sums_b)) return rc;
  if (int rc = take(s.hist, kMtBuckets * nblk, &hist)) return rc;
  if (int rc = take(s.hsums, hplan.nsum, &hsums)) return rc;
  a.st = s.st;
  const dim3 tb(kScanThreads);
  std::uint64_t tag = 0;

  // check and first word
  PhaseClock clock(st, g_mt.timing != 0, g_mt.phase);
  clock.mark(0);
  s.h_res[7] = 0;
  hipLaunchKernelGGL(mt_init, dim3(1), dim3(64), 0, st, s.st);
  TKV_HIP_RC(hipMemsetAsync(a.eqn, 0, n * sizeof(std::uint32_t), st));
  hipLaunchKernelGGL(mt_check, dim3(blocks(n, kScanThreads)), tb, 0, st, a, l[0]);
  hipLaunchKernelGGL(mt_publish, dim3(1), dim3(64), 0, st, s.st, static_cast<const std::uint64_t*>(nullptr), s.d_hres, ++tag);
  if (int rc = s.wait(st, 7, tag, "memtable build: the check left no result")) return rc;
  if (s.h_res[1] & kFlagBounds) return set_error(TKV_INVALID_ARGUMENT, "memtable build: a key reaches past keys_size");
  if (s.h_res[1] & kFlagLen) return set_error(TKV_INVALID_ARGUMENT, "memtable build: an internal key would be 2^28 bytes or more");
  *c.n_entries = 0;
  *c.ikeys_size = 0;
  if (s.h_res[0] < n) {
    *c.first_bad = s.h_res[0];
    return set_error(TKV_CORRUPTED, "memtable build: a record's operation is neither put nor delete");
  }
  *c.first_bad = n;

  // rounds: sort the list, write it back, make the next one
  int cur = 0, ap = -1;  // ap: the apos buffer of the current list, -1 = every position
  std::uint64_t m = n, rounds = 0, second = 0;
  while (m > 0) {
    cur = sort_list(l, cur, m, s.h_res[2], s.h_res[3], hist, hsums, st);
    const ScanPlan rp(m);
    std::uint64_t* lv[kScanLevels + 1];
    rp.place(scan, sums_a, lv);
    const std::uint32_t* pos = ap < 0 ? nullptr : apos[ap];
    const int nap = ap < 0 ? 0 : ap ^ 1;
    hipLaunchKernelGGL(mt_ties, dim3(static_cast<unsigned>(rp.m[1])), tb, 0, st, a, l[cur], pos, m, lv[0], lv[1]);
    scan_rest(rp, lv, st);
    ++rounds;
    hipLaunchKernelGGL(mt_compact, dim3(blocks(m, kScanThreads)), tb, 0, st, a, l[cur], pos, m,
                       static_cast<const std::uint64_t*>(scan), rounds * kMtWordBytes, l[cur ^ 1], apos[nap]);
    hipLaunchKernelGGL(mt_publish, dim3(1), dim3(64), 0, st, s.st, static_cast<const std::uint64_t*>(lv[rp.levels]), s.d_hres,
                       ++tag);
    if (rounds == 1) clock.mark(1);
    if (int rc = s.wait(st, 7, tag, "memtable build: a round left no result")) return rc;
    const std::uint64_t next = s.h_res[4] & 0xFFFFFFFFull;
    if (next > m) return set_error(TKV_IO_ERROR, "memtable build: a round grew its list");
    m = next;
    cur ^= 1;
    ap = nap;
    if (rounds == 1) second = m;
  }
  clock.mark(2);

  // dedupe: the scratch of the lists is free again
  a.cnt = scan;
  a.len = l[0].kw;
  std::uint64_t *lvC[kScanLevels + 1], *lvL[kScanLevels + 1];
  plan.place(a.cnt, sums_a, lvC);
  plan.place(a.len, sums_b, lvL);
  const dim3 g0(static_cast<unsigned>(plan.m[1]));
  hipLaunchKernelGGL(mt_survivors, g0, tb, 0, st, a, 0, lvC[1]);
  scan_rest(plan, lvC, st);
  hipLaunchKernelGGL(mt_survivors, g0, tb, 0, st, a, 1, lvL[1]);
  scan_rest(plan, lvL, st);
  hipLaunchKernelGGL(mt_publish_sizes, dim3(1), dim3(64), 0, st, static_cast<const std::uint64_t*>(lvC[plan.levels]),
                     static_cast<const std::uint64_t*>(lvL[plan.levels]), s.d_hres, ++tag);
  clock.mark(3);
  if (int rc = s.wait(st, 7, tag, "memtable build: the dedupe left no result")) return rc;
  a.m = s.h_res[0];
  a.total = s.h_res[1];
  if (a.m == 0 || a.m > n) return set_error(TKV_IO_ERROR, "memtable build: the dedupe is inconsistent");
  *c.n_entries = a.m;
  *c.ikeys_size = a.total;
  const bool want_cols = a.o_ikey_off || a.o_ikey_len || a.o_val_off || a.o_val_len || a.o_src;
  if ((want_cols && a.m > c.entry_cap) || (a.o_ikeys && a.total > c.ikeys_cap))
    return set_error(TKV_BUFFER_OVERFLOW, "memtable build: the entries or the internal keys do not fit");
  if (a.o_ikeys && a.m > 0x7FFFFFFFull)  // (two spans per entry, u32 span numbers in the tiles)
    return set_error(TKV_INVALID_ARGUMENT, "memtable build: more than 2^31 - 1 entries in one arena");

  // columns and the arena
  if (want_cols || a.o_ikeys) {
    const std::uint64_t ntiles = (a.total + kDecTile - 1u) / kDecTile;
    if (a.o_ikeys) {
      a.esrc = l[0].rec;
      if (int rc = take(s.pre, 2u * a.m + 1u, &a.pre)) return rc;
      if (int rc = take(s.meta, static_cast<std::uint64_t>(kMtStage) * a.m, &a.meta)) return rc;
      if (int rc = take(s.tile, 2u * ntiles, &a.tile)) return rc;
    }
    hipLaunchKernelGGL(mt_columns, dim3(blocks(n, kScanThreads)), tb, 0, st, a);
    if (a.o_ikeys) {
      EmitArgs<MtSrc> e{};
      e.src = MtSrc{a.keys, a.key_off, a.esrc, a.meta};
      e.pre = a.pre;
      e.dst = a.o_ikeys;
      e.total = a.total;
      e.tile = a.tile;
      e.n = 2u * a.m;
      launch_span_emit(s.ncu, e, st);
    }
    TKV_HIP_RC(hipGetLastError());
  }
  clock.mark(4);
  TKV_HIP_RC(hipStreamSynchronize(st));
  clock.finish();
  g_mt.last[0] = a.m;
  g_mt.last[1] = rounds;
  g_mt.last[2] = second;
  g_mt.last[3] = g_mt.taken;
  return TKV_OK;
}

}  // namespace

int memtable_build_device_impl(const MemtableCall& c, hipStream_t st) {
  g_mt.begin();
  for (auto& v : g_mt_passes) v = 0;
  MtScratch* sp = nullptr;
  if (int rc = per_device_scratch(&sp, kMtHres, kStWords, true)) return rc;
  MtArgs a{};
  a.keys = c.keys;
  a.keys_size = c.keys_size;
  a.key_off = c.key_off;
  a.key_len = c.key_len;
  a.val_off = c.val_off;
  a.val_len = c.val_len;
  a.op = c.op;
  a.tomb = c.tomb;
  a.seq = c.seq;
  a.n = c.n;
  a.ts = c.timestamp_ms;
  a.o_ikeys = c.ikeys;
  a.o_ikey_off = c.ikey_off;
  a.o_ikey_len = c.ikey_len;
  a.o_val_off = c.out_val_off;
  a.o_val_len = c.out_val_len;
  a.o_src = c.src;
  std::lock_guard<std::mutex> lk(sp->mu);
  return build_locked(*sp, a, c, st);
}

}  // namespace tkv

extern "C" {

void tkv_debug_memtable_geom(uint64_t out[4]) {
  out[0] = tkv::kMtTile;
  out[1] = tkv::kMtBuckets;
  out[2] = tkv::kMtPasses;
  out[3] = tkv::kDecTile;
}

void tkv_debug_memtable_last(uint64_t out[4]) { tkv::g_mt.get_last(out); }

void tkv_debug_memtable_passes(uint64_t out[4]) {
  for (int i = 0; i < 4; ++i) out[i] = tkv::g_mt_passes[i];
}

int tkv_debug_memtable_phases(int enable, double out_ms[4]) { return tkv::g_mt.phases(enable, out_ms); }

}  // extern "C"
