// SSTable scan on the device (include/tkv_crc32.h "SSTable scan"): the inverse of the
// flush (tkv_sst_build.hip). A file image in HBM is verified and taken apart into the columnar form the
// flush takes: the blocks' offset / size / first entry, every entry's key and value length, and the keys
// and values either copied back to back into arenas or left in the image as views.
//
// Open. scn_open: one thread checks the footer's fields (sst_footer_ok) and B against the index size and
//   publishes them; the host needs B and index_size for the launches below. The index is a chain of
//   length-prefixed strings: scn_next computes J[p] = where the entry that starts at index byte p ends,
//   for every byte p (an entry that fails its checks jumps to the sink index_size + 1, index_size jumps
//   to itself), chain_double (tkv_scan.h, shared with the flush) marks the chain from byte 8 in
//   ceil(log2(B + 2)) rounds, a u64 scan of the marks (tkv_scan.h) ranks the entries, and scn_blocks reads off / size
//   of every marked entry, one thread each. The framing holds when exactly B entries are marked, the
//   sink is not, and every block lies in the data region (scn_index_verdict).
// Checksum. One batch_device_impl call folds the B block images and, as entry B, the footer's span
//   [index_offset, index_offset + index_size + 16); sst_fix turns the blocks' CRCs into stamp values and
//   scn_crc_check compares them with the stored fields. With a broken index only the footer's span is
//   folded: the footer decides between TKV_SST_BAD_FOOTER and TKV_SST_BAD_INDEX.
// Parse. scn_parse, one wave per block: the header checks (sst_block_header_ok), then the body's string
//   chain out of an LDS window of 4 KiB + 3 bytes that starts at the current string: every lane takes the
//   same steps (sst_chain_next on the 4 window bytes at the position), so the walk is serial per block and
//   parallel over blocks. A string that ends behind the window moves the position without loading what
//   it covers; the next window starts at the new position. The first pass writes every block's entry
//   count and key and value bytes (0 for a bad block) and takes the minimum of the bad block indices;
//   three u64 scans over the blocks give block_first and the totals; the host reads them and decides
//   corrupted / overflow. The second pass writes the entry records (key position, value position, lengths)
//   to scratch at block_first[j] + rank, 64 records per store step.
// Emit. Two u64 scans of the lengths give the arena offsets, scn_finish writes the caller's columns and
//   the tile tables, and span_emit (tkv_wal_emit.h, shared with the WAL decode) gathers each copied arena.
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
#include "tkv_wal_emit.h"

namespace tkv {
namespace {

constexpr std::uint32_t kScnBody = 4096;             // body bytes a window is walked for
constexpr std::uint32_t kScnLook = 3;                // varint look-ahead behind them
constexpr std::uint32_t kScnWin = 16 + kScnBody + 16;  // the source's offset in its granule, the bytes, the look-ahead
constexpr unsigned kScnWaves = 8;                    // waves (blocks in flight) per workgroup
constexpr unsigned kScnThreads = 64 * kScnWaves;
constexpr unsigned kScnGroupsPerCu = 2;
constexpr unsigned kScnHres = 8;                     // words of the pinned result block
static_assert(kScnWin % 16 == 0 && 15u + kScnBody + kScnLook <= kScnWin, "window");
static_assert(kScnGroupsPerCu * kScnWaves * kScnWin <= 163840, "LDS");

enum : unsigned long long { kBadIndex = 1, kBadFooterCrc = 2 };

struct ScanArgs {
  const std::uint8_t* file;
  std::uint64_t size;
  std::uint64_t ioff, isz, B;   // the footer's fields and the index's count (after scn_open)
  // per index byte: isz + 2 entries (positions 0 .. isz and the sink isz + 1)
  std::uint32_t* J;
  std::uint32_t* Ja;
  std::uint32_t* Jb;
  std::uint32_t* mark;
  std::uint64_t* rank;          // exclusive scan of the marks over [0, isz)
  const std::uint64_t* nmark;   // its total
  // per block: B + 1 entries (entry B of boff / bsize is the footer's CRC span)
  std::uint64_t* boff;
  std::uint32_t* bsize;
  std::uint32_t* bcrc;
  std::uint64_t* ikey;          // file offset of the index entry's key
  std::uint32_t* ikl;           // its length
  std::uint64_t* bfirst;        // entry counts, then their exclusive scan
  std::uint64_t* bks;           // key bytes of every block, then their exclusive scan
  std::uint64_t* bvs;           // value bytes
  // per entry: n + 1 entries of kpre / vpre
  std::uint64_t* kpos;          // file offset of the key's bytes
  std::uint64_t* vpos;
  std::uint32_t* klen;
  std::uint32_t* vlen;
  std::uint64_t* kpre;          // arena offsets
  std::uint64_t* vpre;
  std::uint32_t* ktile;
  std::uint32_t* vtile;
  std::uint64_t n, ktotal, vtotal;
  std::uint32_t key_views, val_views;
  std::uint32_t nwaves;
  // device words: [0] flags, [1] smallest bad block
  unsigned long long* w;
  // the caller's arrays, each nullable
  std::uint64_t* o_key_off;
  std::uint32_t* o_key_len;
  std::uint64_t* o_val_off;
  std::uint32_t* o_val_len;
  std::uint64_t* o_block_off;
  std::uint32_t* o_block_size;
  std::uint32_t* o_block_first;
};

// Little-endian integers and varint words, bytewise: the image has any alignment.
__device__ __forceinline__ std::uint32_t le32(const std::uint8_t* p) {
  return p[0] | (static_cast<std::uint32_t>(p[1]) << 8) | (static_cast<std::uint32_t>(p[2]) << 16) |
         (static_cast<std::uint32_t>(p[3]) << 24);
}
__device__ __forceinline__ std::uint64_t le64(const std::uint8_t* p) {
  return le32(p) | (static_cast<std::uint64_t>(le32(p + 4)) << 32);
}
// The min(avail, maxb) bytes at p as a word (maxb <= 5): no byte behind p + avail is read.
__device__ __forceinline__ std::uint64_t bytes_word(const std::uint8_t* p, std::uint64_t avail, std::uint32_t maxb) {
  std::uint64_t w = 0;
  if (avail >= 5u && maxb == 5u) {  // the usual case, its loads issued together
#pragma unroll
    for (std::uint32_t k = 0; k < 5u; ++k) w |= static_cast<std::uint64_t>(p[k]) << (8u * k);
    return w;
  }
  for (std::uint32_t k = 0; k < maxb; ++k)
    if (k < avail) w |= static_cast<std::uint64_t>(p[k]) << (8u * k);
  return w;
}

// ---- open -------------------------------------------------------------------------------------------

// The footer's fields and B. The host has checked 28 <= size <= 2^32 - 1.
__global__ void scn_open(ScanArgs a, std::uint64_t* h) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  a.w[0] = 0;
  a.w[1] = ~0ull;
  const std::uint8_t* f = a.file + (a.size - kSstFooter);
  const std::uint32_t ioff = le32(f), isz = le32(f + 4);
  const bool fok = sst_footer_ok(a.size, ioff, isz);
  std::uint64_t B = 0;
  bool bok = false;
  if (fok) {
    B = le64(a.file + ioff);
    bok = sst_index_count_ok(B, isz);
  }
  h[0] = ioff;
  h[1] = isz;
  h[2] = B;
  h[3] = fok ? 1u : 0u;
  h[4] = bok ? 1u : 0u;
  h[7] = 1;
}

// J[p] for every index byte p in [0, isz + 1]: an entry's end, the sink isz + 1 for a position that holds
// no valid entry (and for the count's bytes), isz for isz itself. mark = {8}.
__global__ __launch_bounds__(kScanThreads) void scn_next(ScanArgs a) {
  const std::uint64_t p = blockIdx.x * static_cast<std::uint64_t>(kScanThreads) + threadIdx.x;
  if (p > a.isz + 1u) return;
  const std::uint32_t sink = static_cast<std::uint32_t>(a.isz + 1u);
  a.mark[p] = p == 8u ? 1u : 0u;
  std::uint32_t j = sink;
  if (p == a.isz) {
    j = static_cast<std::uint32_t>(a.isz);
  } else if (p >= 8u && p < a.isz) {
    const std::uint64_t left = a.isz - p;
    const std::uint32_t w = static_cast<std::uint32_t>(bytes_word(a.file + a.ioff + p, left, kSstLenBytes));
    const SstLink s = sst_chain_next(w, p, a.isz, kSstIndexFixed);
    if (s.ok) j = static_cast<std::uint32_t>(s.next);
  }
  a.J[p] = j;
}

// Level 0 of the mark scan over [0, isz): the entries in front of every index byte.
__global__ __launch_bounds__(kScanThreads) void scn_marks(ScanArgs a, std::uint64_t* bsum) {
  const std::uint64_t i0 = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
  std::uint64_t v[kScanItems];
#pragma unroll
  for (unsigned k = 0; k < kScanItems; ++k) v[k] = i0 + k < a.isz ? a.mark[i0 + k] : 0u;
  scan_items(v, i0, a.isz, a.rank, bsum);
}

// Every marked index entry of rank j < B: its key and its block.
__global__ __launch_bounds__(kScanThreads) void scn_blocks(ScanArgs a) {
  const std::uint64_t p = blockIdx.x * static_cast<std::uint64_t>(kScanThreads) + threadIdx.x;
  if (p < 8u || p >= a.isz || !a.mark[p]) return;
  const std::uint64_t j = a.rank[p];
  if (j >= a.B) return;  // more entries than B: scn_index_verdict sees the count
  const std::uint8_t* e = a.file + a.ioff + p;
  const std::uint32_t w = static_cast<std::uint32_t>(bytes_word(e, a.isz - p, kSstLenBytes));
  const SstLink s = sst_chain_next(w, p, a.isz, kSstIndexFixed);  // (ok: a marked position below isz is an entry)
  if (!s.ok) {
    atomicOr(a.w, kBadIndex);
    return;
  }
  const std::uint64_t off = le64(e + s.n + s.len), size = le64(e + s.n + s.len + 8u);
  const bool ok = sst_index_block_ok(off, size, a.ioff);
  if (!ok) atomicOr(a.w, kBadIndex);
  a.boff[j] = ok ? off : 0u;
  a.bsize[j] = ok ? static_cast<std::uint32_t>(size) : 0u;
  a.ikey[j] = a.ioff + p + s.n;
  a.ikl[j] = s.len;
}

__global__ void scn_index_verdict(ScanArgs a, std::uint64_t* h) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const bool ok = *a.nmark == a.B && !a.mark[a.isz + 1u] && !(a.w[0] & kBadIndex);
  if (!ok) a.w[0] |= kBadIndex;
  // the footer's CRC span: entry B of the batch, entry 0 when the index is not to be trusted
  const std::uint64_t k = ok ? a.B : 0u;
  a.boff[k] = a.ioff;
  a.bsize[k] = static_cast<std::uint32_t>(a.isz + kSstFooterCrc);
  h[0] = ok ? 1u : 0u;
  h[7] = 2;
}

// ---- checksum ---------------------------------------------------------------------------------------

// bcrc[0, nb) against the blocks' stored fields, bcrc[nb] against the footer's.
__global__ __launch_bounds__(kScanThreads) void scn_crc_check(ScanArgs a, std::uint64_t nb) {
  const std::uint64_t j = blockIdx.x * static_cast<std::uint64_t>(kScanThreads) + threadIdx.x;
  if (j > nb) return;
  if (j < nb) {
    if (le32(a.file + a.boff[j] + kSstCrc) != a.bcrc[j]) atomicMin(a.w + 1, static_cast<unsigned long long>(j));
  } else if (le32(a.file + a.ioff + a.isz + kSstFooterCrc) != a.bcrc[j]) {
    atomicOr(a.w, kBadFooterCrc);
  }
}

// ---- parse ------------------------------------------------------------------------------------------

// Body bytes [q, q + kScnBody + kScnLook) cut to the body's z bytes into the window: whole source
// granules that hold one of those bytes (ld16 loads no other; the granules' other bytes are the image's:
// at least 22 bytes of header lie in front of a body and the image padding, the index and the footer
// behind it). Returns the window offset of body byte q.
__device__ __forceinline__ std::uint32_t load_window(std::uint8_t* win, const std::uint8_t* body, std::uint64_t q, std::uint64_t z,
                                                     std::uint32_t lane) {
  const std::uint64_t left = z - q;
  const std::uint32_t len = left < kScnBody + kScnLook ? static_cast<std::uint32_t>(left) : kScnBody + kScnLook;
  const std::uintptr_t s = reinterpret_cast<std::uintptr_t>(body) + static_cast<std::uintptr_t>(q);
  const std::uintptr_t e = s + len;
  const std::uintptr_t al = s & ~static_cast<std::uintptr_t>(15);
  const std::uint32_t o = static_cast<std::uint32_t>(s & 15u);
  wave_sync();  // the walk of the window before this one is done
  constexpr std::uint32_t kSteps = (kScnWin + 1023u) / 1024u;
  uint4 v[kSteps];  // the window's loads issued together (ld16 loads nothing at or behind e)
#pragma unroll
  for (std::uint32_t it = 0; it < kSteps; ++it) v[it] = ld16(al + 16u * lane + 1024u * it, s, e);
#pragma unroll
  for (std::uint32_t it = 0; it < kSteps; ++it) {
    const std::uint32_t g = 16u * lane + 1024u * it;
    if (g < o + len) *reinterpret_cast<uint4*>(win + g) = v[it];
  }
  wave_sync();
  return o;
}

// Block j by one wave, every lane in step. WRITE = false: the verdict, the count and the totals.
// WRITE = true (every block has passed): the entry records.
template <bool WRITE>
__device__ __forceinline__ void parse_block(const ScanArgs& a, std::uint8_t* win, std::uint64_t j, std::uint32_t lane) {
  const std::uint64_t off = a.boff[j];
  const std::uint32_t size = a.bsize[j];  // >= 22, off + size <= index_offset
  const std::uint8_t* img = a.file + off;
  const std::uint32_t c = le32(img + 1), z = le32(img + 5);
  const std::uint32_t vavail = size - kSstHeader;
  const SstVarint zv = sst_varint_word(bytes_word(img + kSstHeader, vavail, kSstBodyLenBytes), vavail, kSstBodyLenBytes);
  bool ok = sst_block_header_ok(img[0], c, z, le32(img + 9), img[13], size, zv);
  std::uint64_t sum = 0, ksum = 0, vsum = 0;
  if (ok) {
    const std::uint8_t* body = img + kSstHeader + zv.n;  // z bytes, inside the image: 21 + 5 + z < 36 + z
    const std::uint64_t bpos = off + kSstHeader + zv.n;
    const std::uint64_t first = WRITE ? a.bfirst[j] : 0u;
    const std::uint32_t nstr = 2u * c;  // 8 c <= z < 2^32
    std::uint64_t q = 0, ws = 0, kq = 0, k0 = 0;
    std::uint32_t o = 0, kl = 0, kl0 = 0;
    bool have = false;
    std::uint64_t mk = 0, mv = 0;  // the lane's record of the current 64
    std::uint32_t mkl = 0, mvl = 0;
    for (std::uint32_t r = 0; r < nstr; ++r) {
      if (q >= z) {
        ok = false;
        break;
      }
      if (!have || q >= ws + kScnBody) {  // (q only grows)
        o = load_window(win, body, q, z, lane);
        ws = q;
        have = true;
      }
      const std::uint8_t* b = win + o + static_cast<std::uint32_t>(q - ws);
      const std::uint32_t w = b[0] | (static_cast<std::uint32_t>(b[1]) << 8) | (static_cast<std::uint32_t>(b[2]) << 16) |
                              (static_cast<std::uint32_t>(b[3]) << 24);  // (bytes behind the body are not used)
      const SstLink s = sst_chain_next(w, q, z, 0u);
      if (!s.ok) {
        ok = false;
        break;
      }
      if (!(r & 1u)) {
        kq = q + s.n;
        kl = s.len;
        if (r == 0) {
          k0 = kq;
          kl0 = kl;
        }
      } else {
        sum += sst_counted(kl, s.len);
        ksum += kl;
        vsum += s.len;
        if (WRITE) {
          const std::uint32_t el = r >> 1;
          if ((el & 63u) == lane) {
            mk = bpos + kq;
            mv = bpos + q + s.n;
            mkl = kl;
            mvl = s.len;
          }
          if ((el & 63u) == 63u || el + 1u == c) {
            const std::uint64_t e = first + (el & ~63u) + lane;
            if (lane <= (el & 63u)) {
              a.kpos[e] = mk;
              a.vpos[e] = mv;
              a.klen[e] = mkl;
              a.vlen[e] = mvl;
            }
          }
        }
      }
      q = s.next;
    }
    ok = ok && sum == z;
    if (!WRITE && ok) {
      // the index entry's key is the first entry's
      ok = a.ikl[j] == kl0;
      if (ok) {
        const std::uint8_t* x = a.file + a.ikey[j];
        const std::uint8_t* y = body + k0;
        bool same = true;
        for (std::uint32_t t = lane; t < kl0; t += 64u) same = same && x[t] == y[t];
        ok = __ballot(!same) == 0ull;
      }
    }
  }
  if (!WRITE && lane == 0) {
    // (totals by scans of these, not by atomics: every block would add to the same three words)
    a.bfirst[j] = ok ? c : 0u;
    a.bks[j] = ok ? ksum : 0u;
    a.bvs[j] = ok ? vsum : 0u;
    if (!ok) atomicMin(a.w + 1, static_cast<unsigned long long>(j));
  }
}

template <bool WRITE>
__global__ __launch_bounds__(kScnThreads) void scn_parse(ScanArgs a) {
  __shared__ __attribute__((aligned(16))) std::uint8_t lds[kScnWaves * kScnWin];
  const std::uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const std::uint32_t lane = threadIdx.x & 63u;
  std::uint8_t* win = lds + wv * kScnWin;
  for (std::uint64_t j = blockIdx.x * kScnWaves + wv; j < a.B; j += a.nwaves) parse_block<WRITE>(a, win, j, lane);
}

// The verdict and the totals (the tops of the three block scans; NULL for a table without a block).
__global__ void scn_publish(ScanArgs a, const std::uint64_t* ntop, const std::uint64_t* ktop, const std::uint64_t* vtop,
                            std::uint64_t* h) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  h[0] = a.w[0];
  h[1] = a.w[1];
  h[2] = ntop ? *ntop : 0u;
  h[3] = ktop ? *ktop : 0u;
  h[4] = vtop ? *vtop : 0u;
  h[7] = 3;
}

// Level 0 of a length scan over [0, n): which = 0 the keys to kpre, 1 the values to vpre.
__global__ __launch_bounds__(kScanThreads) void scn_lens(ScanArgs a, int which, std::uint64_t* bsum) {
  const std::uint64_t i0 = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
  const std::uint32_t* len = which ? a.vlen : a.klen;
  std::uint64_t v[kScanItems];
#pragma unroll
  for (unsigned k = 0; k < kScanItems; ++k) v[k] = i0 + k < a.n ? len[i0 + k] : 0u;
  scan_items(v, i0, a.n, which ? a.vpre : a.kpre, bsum);
}

// ---- emit -------------------------------------------------------------------------------------------

// The caller's entry columns and the tile tables of the copied arenas.
__global__ __launch_bounds__(kScanThreads) void scn_finish(ScanArgs a) {
  const std::uint64_t i = blockIdx.x * static_cast<std::uint64_t>(kScanThreads) + threadIdx.x;
  if (i >= a.n) return;
  const std::uint32_t kl = a.klen[i], vl = a.vlen[i];
  const std::uint64_t ko = a.kpre[i], vo = a.vpre[i];
  if (i + 1u == a.n) {
    a.kpre[a.n] = a.ktotal;
    a.vpre[a.n] = a.vtotal;
  }
  if (a.o_key_len) a.o_key_len[i] = kl;
  if (a.o_val_len) a.o_val_len[i] = vl;
  if (a.o_key_off) a.o_key_off[i] = a.key_views ? a.kpos[i] : ko;
  if (a.o_val_off) a.o_val_off[i] = a.val_views ? a.vpos[i] : vo;
  if (a.ktile && kl) tile_entries(a.ktile, i, ko, kl, a.ktotal);
  if (a.vtile && vl) tile_entries(a.vtile, i, vo, vl, a.vtotal);
}

// The caller's block arrays.
__global__ __launch_bounds__(kScanThreads) void scn_out(ScanArgs a) {
  const std::uint64_t j = blockIdx.x * static_cast<std::uint64_t>(kScanThreads) + threadIdx.x;
  if (j >= a.B) return;
  if (a.o_block_off) a.o_block_off[j] = a.boff[j];
  if (a.o_block_size) a.o_block_size[j] = a.bsize[j];
  if (a.o_block_first) a.o_block_first[j] = static_cast<std::uint32_t>(a.bfirst[j]);
}

// Where entry i's span lies in the file for the shared emit.
struct SstSrc {
  const std::uint8_t* file;
  const std::uint64_t* pos;
  __device__ __forceinline__ std::uintptr_t operator()(std::uint64_t i) const {
    return reinterpret_cast<std::uintptr_t>(file) + static_cast<std::uintptr_t>(pos[i]);
  }
};

// ---- host side --------------------------------------------------------------------------------------

// Per-device scratch, grown by doubling and kept between calls (guarded by mu): 24 bytes per index byte,
// 52 per block, 40 per entry, 8 per 4 KiB of a copied arena.
struct ScnScratch : ScratchBase {
  DeviceBuf J, Ja, Jb, mark, rank;                      // per index byte
  DeviceBuf boff, bsize, bcrc, ikey, ikl, bfirst, bks, bvs, bsums;  // per block
  DeviceBuf kpos, vpos, klen, vlen, kpre, vpre;         // per entry
  DeviceBuf sums_a, sums_b, ktile, vtile;
  unsigned long long*& w = words;
};

// The calling thread's device scans (tkv_debug_sst_scan_last, tkv_debug_sst_scan_phases).
thread_local PathStats g_scn;

template <class T>
int take(DeviceBuf& b, std::uint64_t want, T** out) {
  return tkv::take(b, want, out, g_scn.taken, "SSTable scan: scratch allocation failed");
}

int scan_locked(ScnScratch& s, ScanArgs a, const SstScanCall& o, hipStream_t st) {
  const dim3 tb(kScanThreads);
  a.w = s.w;
  PhaseClock clock(st, g_scn.timing != 0, g_scn.phase);
  clock.mark(0);

  // open
  s.h_res[7] = 0;
  hipLaunchKernelGGL(scn_open, dim3(1), dim3(64), 0, st, a, s.d_hres);
  if (int rc = s.wait(st, 7, 1, "SSTable scan: the open left no result")) return rc;
  if (!s.h_res[3]) return sst_scan_corrupted(o, TKV_SST_BAD_FOOTER, "SSTable scan: the footer does not describe this file");
  a.ioff = s.h_res[0];
  a.isz = s.h_res[1];
  a.B = s.h_res[2];
  bool index_ok = s.h_res[4] != 0;
  if (!index_ok) a.B = 0;  // only the footer's span is folded
  const std::uint64_t B = a.B, nidx = a.isz + 2u;
  if (int rc = take(s.boff, B + 1u, &a.boff)) return rc;
  if (int rc = take(s.bsize, B + 1u, &a.bsize)) return rc;
  if (int rc = take(s.bcrc, B + 1u, &a.bcrc)) return rc;
  if (int rc = take(s.ikey, B + 1u, &a.ikey)) return rc;
  if (int rc = take(s.ikl, B + 1u, &a.ikl)) return rc;
  if (int rc = take(s.bfirst, B + 1u, &a.bfirst)) return rc;
  if (int rc = take(s.bks, B + 1u, &a.bks)) return rc;
  if (int rc = take(s.bvs, B + 1u, &a.bvs)) return rc;
  if (int rc = take(s.J, nidx, &a.J)) return rc;
  if (int rc = take(s.Ja, nidx, &a.Ja)) return rc;
  if (int rc = take(s.Jb, nidx, &a.Jb)) return rc;
  if (int rc = take(s.mark, nidx, &a.mark)) return rc;
  if (int rc = take(s.rank, nidx, &a.rank)) return rc;
  const ScanPlan iplan(a.isz);
  std::uint64_t *sums_a = nullptr, *sums_b = nullptr;
  if (int rc = take(s.sums_a, iplan.nsum, &sums_a)) return rc;
  std::uint64_t* lvM[kScanLevels + 1];
  iplan.place(a.rank, sums_a, lvM);
  a.nmark = lvM[iplan.levels];
  const std::uint32_t rounds = sst_rounds(B + 1u);
  hipLaunchKernelGGL(scn_next, dim3(blocks(nidx, kScanThreads)), tb, 0, st, a);
  chain_double(a.J, a.Ja, a.Jb, a.mark, nidx, rounds, st);
  hipLaunchKernelGGL(scn_marks, dim3(static_cast<unsigned>(iplan.m[1])), tb, 0, st, a, lvM[1]);
  scan_up(iplan, lvM, st);
  scan_down(iplan, lvM, st);
  if (index_ok) hipLaunchKernelGGL(scn_blocks, dim3(blocks(a.isz, kScanThreads)), tb, 0, st, a);
  hipLaunchKernelGGL(scn_index_verdict, dim3(1), dim3(64), 0, st, a, s.d_hres);
  clock.mark(1);
  if (int rc = s.wait(st, 7, 2, "SSTable scan: the index pass left no result")) return rc;
  index_ok = index_ok && s.h_res[0] != 0;

  // checksum: the block images and the footer's span in one batch
  const std::uint64_t nb = index_ok ? B : 0u;
  if (int rc = batch_device_impl(kAlgoCrc32, a.file, a.boff, a.bsize, nullptr, a.bcrc, nb + 1u, st)) return rc;
  if (nb) {
    const DeviceTables* tabs = device_tables(kAlgoCrc32);
    if (!tabs) return TKV_IO_ERROR;
    TKV_HIP_RC(launch_sst_fix(const_cast<std::uint8_t*>(a.file), a.boff, a.bsize, a.bcrc, nb, 0, tabs, st));  // store = 0: read only
  }
  hipLaunchKernelGGL(scn_crc_check, dim3(blocks(nb + 1u, kScanThreads)), tb, 0, st, a, nb);
  clock.mark(2);

  // parse: verdicts, counts and totals
  const unsigned pgrid = static_cast<unsigned>(std::max<std::uint64_t>(
      1, std::min<std::uint64_t>((nb + kScnWaves - 1u) / kScnWaves, static_cast<std::uint64_t>(s.ncu) * kScnGroupsPerCu)));
  a.nwaves = pgrid * kScnWaves;
  if (nb) {
    hipLaunchKernelGGL(scn_parse<false>, dim3(pgrid), dim3(kScnThreads), 0, st, a);
    // block_first and the three totals: u64 scans of the blocks' counts and byte sums
    const ScanPlan bplan(nb);
    std::uint64_t* bsums = nullptr;
    if (int rc = take(s.bsums, 3u * bplan.nsum, &bsums)) return rc;
    std::uint64_t *lvB[kScanLevels + 1], *lvK[kScanLevels + 1], *lvV[kScanLevels + 1];
    bplan.place(a.bfirst, bsums, lvB);
    bplan.place(a.bks, bsums + bplan.nsum, lvK);
    bplan.place(a.bvs, bsums + 2u * bplan.nsum, lvV);
    for (std::uint64_t* const* lv : {lvB, lvK, lvV}) {
      hipLaunchKernelGGL(scan_level, dim3(static_cast<unsigned>(bplan.m[1])), tb, 0, st, lv[0], bplan.m[0], lv[1]);
      scan_up(bplan, lv, st);
    }
    scan_down(bplan, lvB, st);
    hipLaunchKernelGGL(scn_publish, dim3(1), dim3(64), 0, st, a, lvB[bplan.levels], lvK[bplan.levels], lvV[bplan.levels], s.d_hres);
  } else {
    const std::uint64_t* none = nullptr;
    hipLaunchKernelGGL(scn_publish, dim3(1), dim3(64), 0, st, a, none, none, none, s.d_hres);
  }
  if (int rc = s.wait(st, 7, 3, "SSTable scan: the parse left no result")) return rc;
  if (s.h_res[0] & kBadFooterCrc) return sst_scan_corrupted(o, TKV_SST_BAD_FOOTER, "SSTable scan: corrupted index or footer");
  if (!index_ok) return sst_scan_corrupted(o, TKV_SST_BAD_INDEX, "SSTable scan: the index framing does not hold");
  if (s.h_res[1] < B) return sst_scan_corrupted(o, s.h_res[1], "SSTable scan: corrupted data block");
  const std::uint64_t n = s.h_res[2];
  a.n = n;
  a.ktotal = s.h_res[3];
  a.vtotal = s.h_res[4];
  *o.n_entries = n;
  *o.n_blocks = B;
  *o.keys_size = a.ktotal;
  *o.vals_size = a.vtotal;
  *o.bad_block = B;
  const bool want_entries = a.o_key_off || a.o_key_len || a.o_val_off || a.o_val_len;
  const bool want_blocks = a.o_block_off || a.o_block_size || a.o_block_first;
  if ((want_entries && n > o.entry_cap) || (want_blocks && B > o.block_cap) || (!a.key_views && a.ktotal > o.keys_cap) ||
      (!a.val_views && a.vtotal > o.vals_cap))
    return set_error(TKV_BUFFER_OVERFLOW, "SSTable scan: an output does not fit its cap");
  const bool kcopy = !a.key_views && o.keys && a.ktotal != 0, vcopy = !a.val_views && o.vals && a.vtotal != 0;
  std::uint32_t kw = 0, vw = 0;
  if (n && (want_entries || want_blocks || kcopy || vcopy)) {
    // the records
    const ScanPlan eplan(n);
    if (int rc = take(s.sums_a, eplan.nsum, &sums_a)) return rc;
    if (int rc = take(s.sums_b, eplan.nsum, &sums_b)) return rc;
    if (int rc = take(s.kpos, n, &a.kpos)) return rc;
    if (int rc = take(s.vpos, n, &a.vpos)) return rc;
    if (int rc = take(s.klen, n, &a.klen)) return rc;
    if (int rc = take(s.vlen, n, &a.vlen)) return rc;
    if (int rc = take(s.kpre, n + 1u, &a.kpre)) return rc;
    if (int rc = take(s.vpre, n + 1u, &a.vpre)) return rc;
    a.ktile = a.vtile = nullptr;
    if (kcopy)
      if (int rc = take(s.ktile, 2u * ((a.ktotal + kDecTile - 1u) / kDecTile), &a.ktile)) return rc;
    if (vcopy)
      if (int rc = take(s.vtile, 2u * ((a.vtotal + kDecTile - 1u) / kDecTile), &a.vtile)) return rc;
    std::uint64_t *lvK[kScanLevels + 1], *lvV[kScanLevels + 1];
    hipLaunchKernelGGL(scn_parse<true>, dim3(pgrid), dim3(kScnThreads), 0, st, a);
    clock.mark(3);
    // emit
    eplan.place(a.kpre, sums_a, lvK);
    eplan.place(a.vpre, sums_b, lvV);
    const dim3 g0(static_cast<unsigned>(eplan.m[1]));
    hipLaunchKernelGGL(scn_lens, g0, tb, 0, st, a, 0, lvK[1]);
    scan_up(eplan, lvK, st);
    scan_down(eplan, lvK, st);
    hipLaunchKernelGGL(scn_lens, g0, tb, 0, st, a, 1, lvV[1]);
    scan_up(eplan, lvV, st);
    scan_down(eplan, lvV, st);
    hipLaunchKernelGGL(scn_finish, dim3(blocks(n, kScanThreads)), tb, 0, st, a);
    if (want_blocks) hipLaunchKernelGGL(scn_out, dim3(blocks(B, kScanThreads)), tb, 0, st, a);
    EmitArgs<SstSrc> e{};
    e.n = n;
    if (kcopy) {
      e.src = SstSrc{a.file, a.kpos};
      e.pre = a.kpre;
      e.dst = o.keys;
      e.total = a.ktotal;
      e.tile = a.ktile;
      kw = launch_span_emit(s.ncu, e, st);
    }
    if (vcopy) {
      e.src = SstSrc{a.file, a.vpos};
      e.pre = a.vpre;
      e.dst = o.vals;
      e.total = a.vtotal;
      e.tile = a.vtile;
      vw = launch_span_emit(s.ncu, e, st);
    }
    TKV_HIP_RC(hipGetLastError());
  } else {
    clock.mark(3);
  }
  clock.mark(4);
  TKV_HIP_RC(hipStreamSynchronize(st));
  clock.finish();
  g_scn.last[0] = B;
  g_scn.last[1] = rounds;
  g_scn.last[2] = a.nwaves;
  g_scn.last[3] = static_cast<std::uint64_t>(kw) + vw;
  return TKV_OK;
}

}  // namespace

int sst_scan_device_impl(const SstScanCall& c, hipStream_t st) {
  g_scn.begin();
  if (!device_tables(kAlgoCrc32)) return TKV_IO_ERROR;
  ScnScratch* sp = nullptr;
  if (int rc = per_device_scratch(&sp, kScnHres, 8, true)) return rc;
  ScanArgs a{};
  a.file = c.file;
  a.size = c.file_size;
  a.key_views = (c.flags & TKV_SST_SCAN_KEY_VIEWS) ? 1u : 0u;
  a.val_views = (c.flags & TKV_SST_SCAN_VAL_VIEWS) ? 1u : 0u;
  a.o_key_off = c.key_off;
  a.o_key_len = c.key_len;
  a.o_val_off = c.val_off;
  a.o_val_len = c.val_len;
  a.o_block_off = c.block_off;
  a.o_block_size = c.block_size;
  a.o_block_first = c.block_first;
  std::lock_guard<std::mutex> lk(sp->mu);
  return scan_locked(*sp, a, c, st);
}

}  // namespace tkv

extern "C" {

void tkv_debug_sst_scan_geometry(uint64_t out[4]) {
  out[0] = tkv::kScnBody;
  out[1] = tkv::kScnLook;
  out[2] = tkv::kDecTile;
  out[3] = tkv::kScanBlock;
}

void tkv_debug_sst_scan_last(uint64_t out[4]) { tkv::g_scn.get_last(out); }

int tkv_debug_sst_scan_phases(int enable, double out_ms[4]) { return tkv::g_scn.phases(enable, out_ms); }

}  // extern "C"
