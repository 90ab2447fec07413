// Record formats around the CRC engine: WAL record verify/stamp (the reference's call sites,
// /root/reference/src/engine/wal.cpp:54-58, 63-130) and SSTable data-block stamping (SURVEY.md §8f
// rank 2, format defined in include/tkv_crc32.h). The host walks lengths and places fields; every
// checksum over record or block bytes runs on the GPU through the engine (tkv_engine.h).
#include <hip/hip_runtime.h>

#include <sched.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "tkv_crc32.h"
#include "tkv_device_util.h"
#include "tkv_engine.h"
#include "tkv_memtable_layout.h"
#include "tkv_sst_layout.h"
#include "tkv_wal_device.h"
#include "tkv_wal_layout.h"

using namespace tkv;

namespace {
bool ptr_ok(const void* p) { return p != nullptr; }

// crc_0 of the 4 little-endian bytes of v followed by z zero bytes: the term that turns the CRC of an
// SSTable image with `v` in its crc32_ field into the CRC with the field read as zero (linearity of
// the CRC over GF(2); the same identity sst_fix applies on the device).
// Shift_(2^k bytes) as byte-sliced linear maps, k < 40: Shift_z(c) is one 4-lookup step per set bit
// of z (about 40 lookups for a 4 KiB image) instead of a bitwise GF(2) multiply per image.
struct PowTables {
  std::uint32_t t[40][4][256];
  PowTables() {
    for (int k = 0; k < 40; ++k)
      for (int j = 0; j < 4; ++j)
        for (std::uint32_t v = 0; v < 256; ++v) t[k][j][v] = shift_bytes(v << (8 * j), std::uint64_t(1) << k, kPoly);
  }
};
const PowTables& pow_tables() {
  static const PowTables* p = new PowTables();
  return *p;
}

std::uint32_t field_term(std::uint32_t v, std::uint64_t z) {
  std::uint32_t c = 0;
  for (int k = 0; k < 4; ++k) {
    c ^= (v >> (8 * k)) & 0xFFu;
    for (int b = 0; b < 8; ++b) c = (c >> 1) ^ ((c & 1u) ? kPoly : 0u);
  }
  const PowTables& pt = pow_tables();
  for (int k = 0; z; ++k, z >>= 1)
    if (z & 1u)
      c = pt.t[k][0][c & 0xFFu] ^ pt.t[k][1][(c >> 8) & 0xFFu] ^ pt.t[k][2][(c >> 16) & 0xFFu] ^ pt.t[k][3][c >> 24];
  return c;
}

// ---- WAL record_len chain (wal.cpp:63-87) ----------------------------------------------------------
struct Chain {
  std::vector<std::uint64_t> pos;  // record starts, in order
  std::vector<std::uint32_t> len;  // their record_len (payload bytes after the 8-byte prefix)
  std::vector<std::uint32_t> crc;  // their stored crc32 (offset 4)
  std::vector<std::uint8_t> kv_ok; // 26 + klen + vlen fits the record (wal.cpp:118-121)
  std::uint64_t end = 0;           // first position after the last record (a record start >= limit)
  bool err = false;                // the chain hit a header that does not fit (wal.cpp:68-70, 82-87)

  void append(const Chain& o, std::size_t from) {
    pos.insert(pos.end(), o.pos.begin() + from, o.pos.end());
    len.insert(len.end(), o.len.begin() + from, o.len.end());
    crc.insert(crc.end(), o.crc.begin() + from, o.crc.end());
    kv_ok.insert(kv_ok.end(), o.kv_ok.begin() + from, o.kv_ok.end());
    end = o.end;
    err = o.err;
  }
};

// Sequential walk from `start` over the records that START before `limit`.
void walk(const std::uint8_t* w, std::uint64_t size, std::uint64_t start, std::uint64_t limit, Chain& c) {
  std::uint64_t p = start;
  while (p < limit) {
    if (size - p < kWalMeta) {
      c.err = true;
      break;
    }
    std::uint32_t rlen, crc, klen, vlen;
    std::memcpy(&rlen, w + p, 4);
    if (static_cast<std::uint64_t>(rlen) + kWalPayload > size - p) {
      c.err = true;
      break;
    }
    std::memcpy(&crc, w + p + kWalCrc, 4);  // the header's other fields share its cache line
    std::memcpy(&klen, w + p + kWalKeyLen, 4);
    std::memcpy(&vlen, w + p + kWalValLen, 4);
    c.pos.push_back(p);
    c.len.push_back(rlen);
    c.crc.push_back(crc);
    c.kv_ok.push_back(kWalMeta + static_cast<std::uint64_t>(klen) + vlen <= kWalPayload + static_cast<std::uint64_t>(rlen));
    p += kWalPayload + static_cast<std::uint64_t>(rlen);
  }
  c.end = p;
}

// Host threads for CPU-side work: the CPUs this process may run on, capped by OMP_NUM_THREADS (the
// GPU boxes' per-job CPU share) and 16.
unsigned host_threads() {
  unsigned n = 16;
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof(set), &set) == 0) n = std::min<unsigned>(n, static_cast<unsigned>(CPU_COUNT(&set)));
  if (const char* e = std::getenv("OMP_NUM_THREADS")) {
    const long v = std::strtol(e, nullptr, 10);
    if (v > 0) n = std::min<unsigned>(n, static_cast<unsigned>(v));
  }
  return std::max(1u, n);
}

// fn(i) for i in [0, n): on host threads when n is large (field writes scattered over a big image).
template <class F>
void parallel_for(std::uint64_t n, F fn) {
  const unsigned nt = n >= (1u << 14) ? host_threads() : 1u;
  if (nt == 1) {
    for (std::uint64_t i = 0; i < n; ++i) fn(i);
    return;
  }
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t)
    th.emplace_back([=] {
      for (std::uint64_t i = n * t / nt; i < n * (t + 1) / nt; ++i) fn(i);
    });
  for (auto& t : th) t.join();
}

// A header the reference encoder would write (wal.cpp:19-61): record_len = 18 + klen + vlen and the
// two flag bytes are 0/1. Used only to choose speculative starting points; never trusted.
bool plausible(const std::uint8_t* w, std::uint64_t size, std::uint64_t p) {
  if (size - p < kWalMeta) return false;
  std::uint32_t rlen, klen, vlen;
  std::memcpy(&rlen, w + p, 4);
  std::memcpy(&klen, w + p + kWalKeyLen, 4);
  std::memcpy(&vlen, w + p + kWalValLen, 4);
  return w[p + kWalOp] <= 1 && w[p + kWalTomb] <= 1 && static_cast<std::uint64_t>(rlen) == 18ull + klen + vlen &&
         static_cast<std::uint64_t>(rlen) + kWalPayload <= size - p;
}

// The chain of the whole image, identical to a sequential walk from 0. Each record start depends on
// the previous one, so one thread walking a large WAL is bound by DRAM latency (one dependent miss
// per record). Here the image is cut into K pieces; the walker of piece k>0 starts at the first
// plausible header at or after the cut (speculation). Stitching is exact: piece k's chain is used
// from the true entry point e_k (where the verified chain of pieces < k crosses the cut) onward only
// if e_k is one of its record starts (chains that share a start coincide from there); otherwise
// piece k is walked again from e_k.
// Records that START in [start, limit); c.end is the first record start >= limit (or where the
// chain broke).
Chain wal_chain(const std::uint8_t* w, std::uint64_t size, std::uint64_t start, std::uint64_t limit) {
  constexpr std::uint64_t kPiece = std::uint64_t(8) << 20;
  const std::uint64_t span = limit > start ? limit - start : 0;
  const unsigned K = static_cast<unsigned>(
      std::min<std::uint64_t>(host_threads(), std::max<std::uint64_t>(1, span / kPiece)));
  std::vector<std::uint64_t> cut(K + 1);
  for (unsigned k = 0; k <= K; ++k) cut[k] = start + span * k / K;
  std::vector<Chain> part(K);
  auto run = [&](unsigned k) {
    Chain local;  // built thread-locally: the Chain headers in `part` share cache lines
    std::uint64_t p = cut[k];
    if (k > 0) {
      while (p < cut[k + 1] && !plausible(w, size, p)) ++p;
      if (p >= cut[k + 1]) {
        local.end = p;
        local.err = true;  // no usable start: forces a re-walk if the chain needs this piece
        part[k] = std::move(local);
        return;
      }
    }
    walk(w, size, p, cut[k + 1], local);
    part[k] = std::move(local);
  };
  if (K == 1) {
    run(0);
    return std::move(part[0]);
  }
  std::vector<std::thread> th;
  for (unsigned k = 0; k < K; ++k) th.emplace_back(run, k);
  for (auto& t : th) t.join();
  Chain c = std::move(part[0]);
  for (unsigned k = 1; k < K && !c.err; ++k) {
    const std::uint64_t e = c.end;  // true entry point into piece k (or beyond it)
    if (e >= cut[k + 1]) continue;  // one record spans piece k entirely
    const auto& pk = part[k].pos;
    const auto it = std::lower_bound(pk.begin(), pk.end(), e);
    if (it != pk.end() && *it == e) {
      c.append(part[k], static_cast<std::size_t>(it - pk.begin()));
    } else {
      Chain r;
      walk(w, size, e, cut[k + 1], r);
      c.append(r, 0);
    }
  }
  return c;
}

Chain wal_chain(const std::uint8_t* w, std::uint64_t size) { return wal_chain(w, size, 0, size); }

int wal_verify_host_walk(const uint8_t* h_wal, uint64_t size, uint64_t* n_good, uint64_t* stop_offset,
                         std::vector<std::uint64_t>* good_pos = nullptr);

// The largest sequence_ (u64 LE at record byte 9) of the records at pos[0, n); 0 for none (engine.cpp:17,46).
std::uint64_t max_sequence_of(const std::uint8_t* w, const std::vector<std::uint64_t>& pos) {
  std::uint64_t mx = 0;
  for (const std::uint64_t p : pos) {
    std::uint64_t seq;
    std::memcpy(&seq, w + p + kWalSeq, 8);
    mx = std::max(mx, seq);
  }
  return mx;
}

// tkv_wal_index_device behind its argument checks: the device index, or the exact host walk when the
// device hands over (*walked, nullable, says which).
int index_device_any(const uint8_t* d_wal, uint64_t size, uint64_t* d_off64, uint32_t* d_off32, uint64_t cap,
                     uint64_t* n_good, uint64_t* stop_offset, uint64_t* max_sequence, hipStream_t st, bool* walked) {
  *n_good = *stop_offset = *max_sequence = 0;
  if (size == 0) return TKV_OK;
  bool host_walk = false;
  if (walked) *walked = false;
  const int rc = wal_index_device_impl(d_wal, size, d_off64, d_off32, cap, n_good, stop_offset, max_sequence,
                                       st, &host_walk);
  if (!host_walk) return rc;
  if (walked) *walked = true;
  // the verify's exact fallback (tkv_wal_verify_device): its walk's positions go to the caller's arrays,
  // the copies on the caller's stream
  std::vector<std::uint8_t> h(size);
  if (hipMemcpyAsync(h.data(), d_wal, size, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return set_error(TKV_IO_ERROR, "WAL image copy to host failed");
  std::vector<std::uint64_t> pos;
  const int rw = wal_verify_host_walk(h.data(), size, n_good, stop_offset, &pos);
  if (rw != TKV_OK && rw != TKV_CORRUPTED) return rw;
  *max_sequence = max_sequence_of(h.data(), pos);
  const std::size_t n = static_cast<std::size_t>(std::min<std::uint64_t>(pos.size(), cap));
  std::vector<std::uint32_t> p32;
  if (n && ptr_ok(d_off32)) p32.assign(pos.begin(), pos.begin() + static_cast<std::ptrdiff_t>(n));
  bool ok = true;
  if (n && ptr_ok(d_off64)) ok = hipMemcpyAsync(d_off64, pos.data(), n * 8, hipMemcpyHostToDevice, st) == hipSuccess;
  if (ok && n && ptr_ok(d_off32)) ok = hipMemcpyAsync(d_off32, p32.data(), n * 4, hipMemcpyHostToDevice, st) == hipSuccess;
  if (hipStreamSynchronize(st) != hipSuccess || !ok) return set_error(TKV_IO_ERROR, "WAL index copy to the device failed");
  return rw;
}

// tkv_wal_salvage_device behind its argument checks. The loop of the salvage program: index the
// sub-image [p, size) (the index kernels unchanged: images at any byte alignment are theirs), make its
// offsets absolute, open a gap at its stop s, resynchronise from s + 1, close the gap there, go on.
int salvage_device_any(const uint8_t* d_wal, uint64_t size, uint64_t* d_off64, uint64_t cap, uint64_t* h_gaps,
                       uint64_t gap_cap, uint64_t max_gaps, uint64_t* n_records, uint64_t* n_gaps, uint64_t* stop_offset,
                       uint64_t* bytes_skipped, uint64_t* max_sequence, hipStream_t st) {
  std::uint64_t* last = wal_salvage_last();
  std::fill(last, last + 6, 0);
  *n_records = *n_gaps = *bytes_skipped = *max_sequence = 0;
  *stop_offset = size;
  std::uint64_t p = 0;
  while (p < size) {
    const std::uint64_t have = std::min(*n_records, cap);
    std::uint64_t ng = 0, stop = 0, mseq = 0;
    bool walked = false;
    last[5] += 1;
    const int rc = index_device_any(d_wal + p, size - p, cap > have ? d_off64 + have : nullptr, nullptr, cap - have, &ng, &stop,
                                    &mseq, st, &walked);
    if (rc != TKV_OK && rc != TKV_CORRUPTED) return rc;
    if (int e = wal_salvage_add_base(d_off64 + have, std::min(ng, cap - have), p, st)) return e;
    *n_records += ng;
    *max_sequence = std::max(*max_sequence, mseq);
    if (rc == TKV_OK) break;
    const std::uint64_t s = p + stop;  // an invalid position
    // no further resynchronisation: the budget is used up, or this sub-image went to the exact host walk
    if (*n_gaps == max_gaps || walked) {
      *stop_offset = s;
      break;
    }
    std::uint64_t q = size;
    const int rr = wal_resync_device_impl(d_wal, size, s + 1, &q, st);
    if (rr != TKV_OK && rr != TKV_NOT_FOUND) return rr;
    if (*n_gaps < gap_cap) {
      h_gaps[2 * *n_gaps] = s;
      h_gaps[2 * *n_gaps + 1] = q;
    }
    *n_gaps += 1;
    *bytes_skipped += q - s;
    p = q;
  }
  if (hipStreamSynchronize(st) != hipSuccess) return set_error(TKV_IO_ERROR, "WAL salvage: stream synchronize failed");
  return *n_gaps == 0 && *stop_offset == size ? TKV_OK : TKV_CORRUPTED;
}

// Per-device buffers of tkv_wal_salvage, as the host-image index keeps its own: the device copy of the
// image and of the offsets, grown by doubling and kept between calls up to kSalvageKeep bytes each, and
// the stream the salvage of a host image runs on (guarded by mu, held for the whole call).
constexpr std::uint64_t kSalvageKeep = std::uint64_t(256) << 20;
struct SalvageHost {
  std::mutex mu;
  void* d_img = nullptr;
  void* d_off = nullptr;
  std::uint64_t cap_img = 0, cap_off = 0;
  hipStream_t st = nullptr;
  ~SalvageHost() {
    (void)hipFree(d_img);
    (void)hipFree(d_off);
    if (st) (void)hipStreamDestroy(st);
  }
};

int sst_check(const std::uint64_t* h_sizes, std::uint64_t n) {
  for (std::uint64_t i = 0; i < n; ++i)
    if (h_sizes[i] < TKV_SST_MIN_IMAGE || h_sizes[i] > 0xFFFFFFFFull)
      return set_error(TKV_INVALID_ARGUMENT, "SSTable block image shorter than 22 bytes or 4 GiB and longer");
  return TKV_OK;
}
}  // namespace

extern "C" {

int tkv_wal_verify(const uint8_t* h_wal, uint64_t size, uint64_t* n_good, uint64_t* stop_offset) {
  if ((size && !ptr_ok(h_wal)) || !ptr_ok(n_good) || !ptr_ok(stop_offset))
    return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  // The image goes to the device once; the chain walk, the CRC batch and the first-corruption
  // search run there (tkv_wal_device.hip). The host walk below is the exact fallback for images the
  // device cannot hold or whose chain the speculative device walk could not settle.
  bool host_walk = false;
  const int rc = wal_verify_host_image_impl(h_wal, size, n_good, stop_offset, &host_walk);
  if (!host_walk) return rc;
  return wal_verify_host_walk(h_wal, size, n_good, stop_offset);
}

int tkv_wal_verify_device(const uint8_t* d_wal, uint64_t size, uint64_t* n_good, uint64_t* stop_offset,
                          void* stream) {
  if ((size && !ptr_ok(d_wal)) || !ptr_ok(n_good) || !ptr_ok(stop_offset))
    return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  if (size == 0) {
    *n_good = *stop_offset = 0;
    return TKV_OK;
  }
  bool host_walk = false;
  const int rc = wal_verify_device_impl(d_wal, size, n_good, stop_offset, static_cast<hipStream_t>(stream), &host_walk);
  if (!host_walk) return rc;
  // exact fallback: the image comes back to the host for the sequential-stitched host walk
  std::vector<std::uint8_t> h(size);
  if (hipMemcpy(h.data(), d_wal, size, hipMemcpyDeviceToHost) != hipSuccess)
    return set_error(TKV_IO_ERROR, "WAL image copy to host failed");
  return wal_verify_host_walk(h.data(), size, n_good, stop_offset);
}

int tkv_wal_index_device(const uint8_t* d_wal, uint64_t size, uint64_t* d_off64, uint32_t* d_off32, uint64_t cap,
                         uint64_t* n_good, uint64_t* stop_offset, uint64_t* max_sequence, void* stream) {
  if ((size && !ptr_ok(d_wal)) || !ptr_ok(n_good) || !ptr_ok(stop_offset) || !ptr_ok(max_sequence))
    return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  if (cap && !ptr_ok(d_off64) && !ptr_ok(d_off32))
    return set_error(TKV_INVALID_ARGUMENT, "cap > 0 without an offsets array");
  if (ptr_ok(d_off32) && size > 0xFFFFFFFFull + 1ull)
    return set_error(TKV_INVALID_ARGUMENT, "image larger than 4 GiB (u32 offsets)");
  return index_device_any(d_wal, size, d_off64, d_off32, cap, n_good, stop_offset, max_sequence,
                          static_cast<hipStream_t>(stream), nullptr);
}

int tkv_wal_index(const uint8_t* h_wal, uint64_t size, uint64_t* h_off64, uint64_t cap, uint64_t* n_good,
                  uint64_t* stop_offset, uint64_t* max_sequence) {
  if ((size && !ptr_ok(h_wal)) || !ptr_ok(n_good) || !ptr_ok(stop_offset) || !ptr_ok(max_sequence))
    return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  if (cap && !ptr_ok(h_off64)) return set_error(TKV_INVALID_ARGUMENT, "cap > 0 without an offsets array");
  *n_good = *stop_offset = *max_sequence = 0;
  if (size == 0) return TKV_OK;
  bool host_walk = false;
  const int rc = wal_index_host_image_impl(h_wal, size, h_off64, cap, n_good, stop_offset, max_sequence, &host_walk);
  if (!host_walk) return rc;
  std::vector<std::uint64_t> pos;
  const int rw = wal_verify_host_walk(h_wal, size, n_good, stop_offset, &pos);
  if (rw != TKV_OK && rw != TKV_CORRUPTED) return rw;
  *max_sequence = max_sequence_of(h_wal, pos);
  const std::size_t n = static_cast<std::size_t>(std::min<std::uint64_t>(pos.size(), cap));
  if (n) std::memcpy(h_off64, pos.data(), n * 8);
  return rw;
}

int tkv_wal_resync_device(const uint8_t* d_wal, uint64_t size, uint64_t from, uint64_t* found, void* stream) {
  if ((size && !ptr_ok(d_wal)) || !ptr_ok(found)) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  if (from > size) return set_error(TKV_INVALID_ARGUMENT, "resync start behind the image's end");
  std::uint64_t* last = wal_salvage_last();
  std::fill(last, last + 6, 0);
  return wal_resync_device_impl(d_wal, size, from, found, static_cast<hipStream_t>(stream));
}

int tkv_wal_salvage_device(const uint8_t* d_wal, uint64_t size, uint64_t* d_off64, uint64_t cap, uint64_t* h_gaps,
                           uint64_t gap_cap, uint64_t max_gaps, uint64_t* n_records, uint64_t* n_gaps,
                           uint64_t* stop_offset, uint64_t* bytes_skipped, uint64_t* max_sequence, void* stream) {
  if ((size && !ptr_ok(d_wal)) || !ptr_ok(n_records) || !ptr_ok(n_gaps) || !ptr_ok(stop_offset) || !ptr_ok(bytes_skipped) ||
      !ptr_ok(max_sequence))
    return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  if (cap && !ptr_ok(d_off64)) return set_error(TKV_INVALID_ARGUMENT, "cap > 0 without an offsets array");
  if (gap_cap && !ptr_ok(h_gaps)) return set_error(TKV_INVALID_ARGUMENT, "gap_cap > 0 without a gaps array");
  if (size == 0) {
    *n_records = *n_gaps = *stop_offset = *bytes_skipped = *max_sequence = 0;
    return TKV_OK;
  }
  return salvage_device_any(d_wal, size, d_off64, cap, h_gaps, gap_cap, max_gaps, n_records, n_gaps, stop_offset,
                            bytes_skipped, max_sequence, static_cast<hipStream_t>(stream));
}

int tkv_wal_salvage(const uint8_t* h_wal, uint64_t size, uint64_t* h_off64, uint64_t cap, uint64_t* h_gaps,
                    uint64_t gap_cap, uint64_t max_gaps, uint64_t* n_records, uint64_t* n_gaps, uint64_t* stop_offset,
                    uint64_t* bytes_skipped, uint64_t* max_sequence) {
  if ((size && !ptr_ok(h_wal)) || !ptr_ok(n_records) || !ptr_ok(n_gaps) || !ptr_ok(stop_offset) || !ptr_ok(bytes_skipped) ||
      !ptr_ok(max_sequence))
    return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  if (cap && !ptr_ok(h_off64)) return set_error(TKV_INVALID_ARGUMENT, "cap > 0 without an offsets array");
  if (gap_cap && !ptr_ok(h_gaps)) return set_error(TKV_INVALID_ARGUMENT, "gap_cap > 0 without a gaps array");
  *n_records = *n_gaps = *stop_offset = *bytes_skipped = *max_sequence = 0;
  if (size == 0) return TKV_OK;
  // the device copy of the image and of the offsets (a good record is at least 26 bytes long)
  const std::uint64_t dcap = std::min<std::uint64_t>(cap, size / kWalMeta);
  SalvageHost* hp = nullptr;
  if (int rc = per_device(&hp)) return rc;
  SalvageHost& h = *hp;
  std::lock_guard<std::mutex> lk(h.mu);
  if (!h.st && hipStreamCreateWithFlags(&h.st, hipStreamNonBlocking) != hipSuccess)
    return set_error(TKV_IO_ERROR, "WAL salvage: no stream");
  if (grow(&h.d_img, &h.cap_img, size, 1) != TKV_OK || grow(&h.d_off, &h.cap_off, dcap, 8) != TKV_OK) {
    // The device cannot hold it: the index's exact host walk, and no resynchronisation.
    (void)hipGetLastError();
    return tkv_wal_index(h_wal, size, h_off64, cap, n_records, stop_offset, max_sequence);
  }
  auto* d_off = static_cast<std::uint64_t*>(h.d_off);
  int rc = wal_host_image_stage_impl(h_wal, size, static_cast<std::uint8_t*>(h.d_img));
  if (rc == TKV_OK)
    rc = salvage_device_any(static_cast<const std::uint8_t*>(h.d_img), size, d_off, dcap, h_gaps, gap_cap, max_gaps, n_records,
                            n_gaps, stop_offset, bytes_skipped, max_sequence, h.st);
  const std::uint64_t n = std::min(*n_records, dcap);
  if ((rc == TKV_OK || rc == TKV_CORRUPTED) && n &&
      (hipMemcpyAsync(h_off64, d_off, n * 8, hipMemcpyDeviceToHost, h.st) != hipSuccess || hipStreamSynchronize(h.st) != hipSuccess))
    rc = set_error(TKV_IO_ERROR, "WAL salvage: offsets copy to the host failed");
  // nothing of the call outlives it; buffers larger than kSalvageKeep are released, as the index's are
  (void)hipStreamSynchronize(h.st);
  if (h.cap_img > kSalvageKeep) {
    (void)hipFree(h.d_img);
    h.d_img = nullptr;
    h.cap_img = 0;
  }
  if (h.cap_off * 8 > kSalvageKeep) {
    (void)hipFree(h.d_off);
    h.d_off = nullptr;
    h.cap_off = 0;
  }
  return rc;
}

}  // extern "C"

namespace {
// The host-walk verify (exact for every image): the record_len chain walked on host threads, the
// CRCs checked on the GPU through the host batch API.
// good_pos, when given, receives the starts of the good records (Chain::pos of the good prefix).
int wal_verify_host_walk(const uint8_t* h_wal, uint64_t size, uint64_t* n_good, uint64_t* stop_offset,
                         std::vector<std::uint64_t>* good_pos) {
  // The record_len chain (wal.cpp:63-87), walked in parallel (wal_chain): records are
  // [u32 record_len][u32 crc][payload of record_len bytes]. Large images go in phases: the CRC
  // batch of phase j runs (GPU, on a helper thread) while the host walks phase j+1.
  const unsigned J = size >= (std::uint64_t(64) << 20) ? 4u : 1u;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return set_error(TKV_IO_ERROR, "hipGetDevice failed");
  std::vector<Chain> phase;
  phase.reserve(J);  // helper threads read phase[j] while later phases are appended
  std::vector<std::vector<std::uint32_t>> got(J);
  std::vector<std::vector<std::uint64_t>> off(J);
  std::vector<int> rcs(J, TKV_OK);
  std::vector<std::thread> crc_th;
  std::uint64_t start = 0;
  for (unsigned j = 0; j < J; ++j) {
    const std::uint64_t limit = j + 1 == J ? size : std::max(start, size * (j + 1) / J);
    phase.push_back(wal_chain(h_wal, size, start, limit));
    const Chain& ch = phase.back();
    const std::size_t nrec = ch.pos.size();
    off[j].resize(nrec);
    got[j].resize(nrec);
    for (std::size_t i = 0; i < nrec; ++i) off[j][i] = ch.pos[i] + kWalPayload;
    if (nrec)
      crc_th.emplace_back([&, j, nrec] {
        if (hipSetDevice(dev) != hipSuccess) {
          rcs[j] = TKV_IO_ERROR;
          return;
        }
        rcs[j] = batch_host_impl(kAlgoCrc32, h_wal, off[j].data(), phase[j].len.data(), nullptr, got[j].data(), nrec);
      });
    start = ch.end;
    if (ch.err || start >= size) break;
  }
  for (auto& t : crc_th) t.join();
  for (unsigned j = 0; j < J; ++j)
    if (rcs[j] != TKV_OK) return set_error(rcs[j], "WAL verify: CRC batch failed");
  Chain ch = std::move(phase[0]);
  for (std::size_t j = 1; j < phase.size(); ++j) ch.append(phase[j], 0);
  std::vector<std::uint32_t> all;
  all.reserve(ch.pos.size());
  for (std::size_t j = 0; j < phase.size(); ++j) all.insert(all.end(), got[j].begin(), got[j].end());
  const std::size_t nrec = ch.pos.size();
  std::uint64_t good = 0;
  // first record whose CRC (wal.cpp:93-96) or key/value bounds (wal.cpp:118-121) fail
  while (good < nrec && all[good] == ch.crc[good] && ch.kv_ok[good]) ++good;
  *n_good = good;
  *stop_offset = good < nrec ? ch.pos[good] : ch.end;
  if (good_pos) good_pos->assign(ch.pos.begin(), ch.pos.begin() + static_cast<std::ptrdiff_t>(good));
  if (good < nrec || ch.err) return set_error(TKV_CORRUPTED, "corrupted WAL record");
  return TKV_OK;
}
}  // namespace

extern "C" {

int tkv_wal_stamp(uint8_t* h_buf, const uint64_t* h_offsets, const uint32_t* h_sizes, uint64_t n) {
  if (n == 0) return TKV_OK;
  if (!ptr_ok(h_buf) || !ptr_ok(h_offsets) || !ptr_ok(h_sizes)) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  std::vector<std::uint64_t> off(n);
  std::vector<std::uint32_t> len(n), crc(n);
  for (std::uint64_t i = 0; i < n; ++i) {
    if (h_sizes[i] < kWalPayload) return set_error(TKV_INVALID_ARGUMENT, "WAL record shorter than its 8-byte prefix");
    off[i] = h_offsets[i] + kWalPayload;  // wal.cpp:54-57: CRC over [8, size)
    len[i] = h_sizes[i] - kWalPayload;
  }
  if (int rc = batch_host_impl(kAlgoCrc32, h_buf, off.data(), len.data(), nullptr, crc.data(), n)) return rc;
  parallel_for(n, [&](std::uint64_t i) { std::memcpy(h_buf + h_offsets[i] + kWalCrc, &crc[i], 4); });  // wal.cpp:58
  return TKV_OK;
}

}  // extern "C"

namespace {
// ---- WAL group-commit encode (wal.cpp:19-61 for a batch) ---------------------------------------------
struct EncodeIn {
  const std::uint8_t* keys;
  const std::uint64_t* key_off;
  const std::uint32_t* key_len;
  const std::uint8_t* vals;
  const std::uint64_t* val_off;
  const std::uint32_t* val_len;
  const std::uint8_t* op;
  const std::uint8_t* tomb;
  const std::uint64_t* seq;
  std::uint64_t first_seq;
  std::uint64_t n;
};

// The argument checks both entry points share (n >= 1).
int encode_check(const EncodeIn& in, const std::uint64_t* img_size) {
  if (in.n > 0xFFFFFFFFull) return set_error(TKV_INVALID_ARGUMENT, "WAL encode: more than 2^32 - 1 records");
  if (!ptr_ok(in.keys) || !ptr_ok(in.key_off) || !ptr_ok(in.key_len) || !ptr_ok(img_size) ||
      (ptr_ok(in.val_len) && (!ptr_ok(in.vals) || !ptr_ok(in.val_off))))
    return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  return TKV_OK;
}

// Record start offsets (n + 1 entries, the last one the total) of a host batch; TKV_INVALID_ARGUMENT when
// a record_len does not fit u32 (no source byte is read).
int encode_offsets(const EncodeIn& in, std::vector<std::uint64_t>& off) {
  off.resize(in.n + 1);
  std::uint64_t run = 0;
  for (std::uint64_t i = 0; i < in.n; ++i) {
    const std::uint64_t rl = 18ull + in.key_len[i] + (in.val_len ? in.val_len[i] : 0u);
    if (rl > 0xFFFFFFFFull) return set_error(TKV_INVALID_ARGUMENT, "WAL encode: 18 + key_len + val_len does not fit u32");
    off[i] = run;
    run += rl + kWalPayload;
  }
  off[in.n] = run;
  return TKV_OK;
}

// Records laid out at img + off[i] with their CRC fields zero (wal.cpp:27-52), on host threads.
void encode_layout(const EncodeIn& in, const std::vector<std::uint64_t>& off, std::uint8_t* img) {
  parallel_for(in.n, [&](std::uint64_t i) {
    std::uint8_t* r = img + off[i];
    const std::uint32_t kl = in.key_len[i], vl = in.val_len ? in.val_len[i] : 0u;
    const std::uint32_t rl = 18u + kl + vl, zero = 0;
    const std::uint64_t seq = in.seq ? in.seq[i] : in.first_seq + i;
    std::memcpy(r, &rl, 4);
    std::memcpy(r + kWalCrc, &zero, 4);
    r[kWalOp] = in.op ? in.op[i] : 0;
    for (int b = 0; b < 8; ++b) r[kWalSeq + b] = static_cast<std::uint8_t>(seq >> (8 * b));
    r[kWalTomb] = in.tomb && in.tomb[i] ? 1 : 0;
    for (int b = 0; b < 4; ++b) r[kWalKeyLen + b] = static_cast<std::uint8_t>(kl >> (8 * b));
    for (int b = 0; b < 4; ++b) r[kWalValLen + b] = static_cast<std::uint8_t>(vl >> (8 * b));
    if (kl) std::memcpy(r + kWalMeta, in.keys + in.key_off[i], kl);
    if (vl) std::memcpy(r + kWalMeta + kl, in.vals + in.val_off[i], vl);
  });
}

// Checks, sizes and the layout of a host batch; *laid is set when the records were written.
int encode_host_layout(const EncodeIn& in, std::uint8_t* h_img, std::uint64_t cap, std::uint64_t* img_size,
                       std::vector<std::uint64_t>& off, bool* laid) {
  *laid = false;
  if (in.n == 0) {
    if (ptr_ok(img_size)) *img_size = 0;
    return TKV_OK;
  }
  if (int rc = encode_check(in, img_size)) return rc;
  if (int rc = encode_offsets(in, off)) return rc;
  *img_size = off[in.n];
  if (off[in.n] > cap) return set_error(TKV_BUFFER_OVERFLOW, "WAL encode: the image does not fit cap");
  if (!ptr_ok(h_img)) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  encode_layout(in, off, h_img);
  *laid = true;
  return TKV_OK;
}
}  // namespace

extern "C" {

int tkv_wal_encode_device(const uint8_t* d_keys, const uint64_t* d_key_off, const uint32_t* d_key_len,
                          const uint8_t* d_vals, const uint64_t* d_val_off, const uint32_t* d_val_len, const uint8_t* d_op,
                          const uint8_t* d_tomb, const uint64_t* d_seq, uint64_t first_seq, uint64_t n, uint8_t* d_img,
                          uint64_t cap, uint64_t* d_rec_off, uint32_t* d_crc, uint64_t* img_size, void* stream) {
  if (n == 0) {
    if (ptr_ok(img_size)) *img_size = 0;
    return TKV_OK;
  }
  const EncodeIn in{d_keys, d_key_off, d_key_len, d_vals, d_val_off, d_val_len, d_op, d_tomb, d_seq, first_seq, n};
  if (int rc = encode_check(in, img_size)) return rc;
  if (cap && !ptr_ok(d_img)) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  return wal_encode_device_impl(d_keys, d_key_off, d_key_len, d_vals, d_val_off, d_val_len, d_op, d_tomb, d_seq, first_seq,
                                n, d_img, cap, d_rec_off, d_crc, img_size, static_cast<hipStream_t>(stream));
}

int tkv_wal_encode(const uint8_t* h_keys, const uint64_t* h_key_off, const uint32_t* h_key_len, const uint8_t* h_vals,
                   const uint64_t* h_val_off, const uint32_t* h_val_len, const uint8_t* h_op, const uint8_t* h_tomb,
                   const uint64_t* h_seq, uint64_t first_seq, uint64_t n, uint8_t* h_img, uint64_t cap,
                   uint64_t* h_rec_off, uint32_t* h_crc, uint64_t* img_size) {
  const EncodeIn in{h_keys, h_key_off, h_key_len, h_vals, h_val_off, h_val_len, h_op, h_tomb, h_seq, first_seq, n};
  std::vector<std::uint64_t> off;
  bool laid = false;
  if (int rc = encode_host_layout(in, h_img, cap, img_size, off, &laid)) return rc;
  if (!laid) return TKV_OK;
  // the stamp of tkv_wal_stamp: CRC over [8, size) of every record on the GPU, then the fields (wal.cpp:54-58)
  std::vector<std::uint64_t> poff(n);
  std::vector<std::uint32_t> len(n), crc(n);
  for (std::uint64_t i = 0; i < n; ++i) {
    poff[i] = off[i] + kWalPayload;
    len[i] = static_cast<std::uint32_t>(off[i + 1] - off[i] - kWalPayload);
  }
  if (int rc = batch_host_impl(kAlgoCrc32, h_img, poff.data(), len.data(), nullptr, crc.data(), n)) return rc;
  parallel_for(n, [&](std::uint64_t i) { std::memcpy(h_img + off[i] + kWalCrc, &crc[i], 4); });
  if (ptr_ok(h_rec_off)) std::memcpy(h_rec_off, off.data(), n * sizeof(std::uint64_t));
  if (ptr_ok(h_crc)) std::memcpy(h_crc, crc.data(), n * sizeof(std::uint32_t));
  return TKV_OK;
}

size_t tkv_debug_wal_encode_layout(const uint8_t* h_keys, const uint64_t* h_key_off, const uint32_t* h_key_len,
                                   const uint8_t* h_vals, const uint64_t* h_val_off, const uint32_t* h_val_len,
                                   const uint8_t* h_op, const uint8_t* h_tomb, const uint64_t* h_seq, uint64_t first_seq,
                                   uint64_t n, uint8_t* h_img, uint64_t cap, uint64_t* img_size) {
  const EncodeIn in{h_keys, h_key_off, h_key_len, h_vals, h_val_off, h_val_len, h_op, h_tomb, h_seq, first_seq, n};
  std::vector<std::uint64_t> off;
  bool laid = false;
  if (encode_host_layout(in, h_img, cap, img_size, off, &laid) != TKV_OK || !laid) return 0;
  return static_cast<size_t>(n);
}

}  // extern "C"

namespace {
// ---- WAL batched decode (wal.cpp:98-127 for a record list) -------------------------------------------

// The argument checks both entry points share; *done is set when the call is finished (n == 0).
int decode_check(const void* img, std::uint64_t size, const void* off64, const void* off32, std::uint64_t n,
                 std::uint32_t flags, std::uint64_t* keys_size, std::uint64_t* vals_size, std::uint64_t* first_bad, bool* done) {
  *done = false;
  if (!ptr_ok(keys_size) || !ptr_ok(vals_size) || !ptr_ok(first_bad)) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  if (flags & ~(TKV_WAL_DECODE_KEY_VIEWS | TKV_WAL_DECODE_VAL_VIEWS))
    return set_error(TKV_INVALID_ARGUMENT, "WAL decode: unknown flag bits");
  if (n > 0xFFFFFFFFull) return set_error(TKV_INVALID_ARGUMENT, "WAL decode: more than 2^32 - 1 records");
  if (n == 0) {
    *keys_size = *vals_size = *first_bad = 0;
    *done = true;
    return TKV_OK;
  }
  if (ptr_ok(off64) == ptr_ok(off32)) return set_error(TKV_INVALID_ARGUMENT, "WAL decode: exactly one offset array");
  if (ptr_ok(off32) && size > 0xFFFFFFFFull + 1ull)
    return set_error(TKV_INVALID_ARGUMENT, "image larger than 4 GiB (u32 offsets)");
  if (!ptr_ok(img)) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  return TKV_OK;
}

// Header fields of the record at h + off when it passes wal_entry::decode's structural checks
// (wal.cpp:68, :83, :118-121; 64-bit arithmetic).
bool decode_header(const std::uint8_t* h, std::uint64_t size, std::uint64_t off, std::uint32_t* kl, std::uint32_t* vl) {
  if (off >= size || size - off < kWalMeta) return false;
  std::uint32_t rlen;
  std::memcpy(&rlen, h + off, 4);
  std::memcpy(kl, h + off + kWalKeyLen, 4);
  std::memcpy(vl, h + off + kWalValLen, 4);
  return static_cast<std::uint64_t>(rlen) + kWalPayload <= size - off &&
         static_cast<std::uint64_t>(*kl) + *vl + (kWalMeta - kWalPayload) <= rlen;
}
}  // namespace

extern "C" {

int tkv_wal_decode_device(const uint8_t* d_img, uint64_t size, const uint64_t* d_rec_off64, const uint32_t* d_rec_off32,
                          uint64_t n, uint32_t flags, uint8_t* d_op, uint8_t* d_tomb, uint64_t* d_seq, uint64_t* d_key_off,
                          uint32_t* d_key_len, uint64_t* d_val_off, uint32_t* d_val_len, uint8_t* d_keys, uint64_t keys_cap,
                          uint8_t* d_vals, uint64_t vals_cap, uint64_t* keys_size, uint64_t* vals_size, uint64_t* first_bad,
                          void* stream) {
  bool done = false;
  if (int rc = decode_check(d_img, size, d_rec_off64, d_rec_off32, n, flags, keys_size, vals_size, first_bad, &done)) return rc;
  if (done) return TKV_OK;
  *keys_size = *vals_size = 0;
  *first_bad = n;
  return wal_decode_device_impl(d_img, size, d_rec_off64, d_rec_off32, n, flags, d_op, d_tomb, d_seq, d_key_off, d_key_len,
                                d_val_off, d_val_len, d_keys, keys_cap, d_vals, vals_cap, keys_size, vals_size, first_bad,
                                static_cast<hipStream_t>(stream));
}

int tkv_wal_decode_host(const uint8_t* h_img, uint64_t size, const uint64_t* h_rec_off64, uint64_t n, uint32_t flags,
                        uint8_t* h_op, uint8_t* h_tomb, uint64_t* h_seq, uint64_t* h_key_off, uint32_t* h_key_len,
                        uint64_t* h_val_off, uint32_t* h_val_len, uint8_t* h_keys, uint64_t keys_cap, uint8_t* h_vals,
                        uint64_t vals_cap, uint64_t* keys_size, uint64_t* vals_size, uint64_t* first_bad) {
  bool done = false;
  if (int rc = decode_check(h_img, size, h_rec_off64, nullptr, n, flags, keys_size, vals_size, first_bad, &done)) return rc;
  if (done) return TKV_OK;
  *keys_size = *vals_size = 0;
  *first_bad = n;
  const bool kviews = flags & TKV_WAL_DECODE_KEY_VIEWS, vviews = flags & TKV_WAL_DECODE_VAL_VIEWS;
  // the header pass: lengths of the records that pass, the smallest failing index per thread's range
  std::vector<std::uint64_t> ko(n + 1), vo(n + 1);
  std::atomic<std::uint64_t> bad{n};
  parallel_for(n, [&](std::uint64_t i) {
    std::uint32_t kl = 0, vl = 0;
    if (!decode_header(h_img, size, h_rec_off64[i], &kl, &vl)) {
      kl = vl = 0;  // (never used as copy lengths)
      std::uint64_t cur = bad.load(std::memory_order_relaxed);
      while (i < cur && !bad.compare_exchange_weak(cur, i, std::memory_order_relaxed)) {
      }
    }
    ko[i + 1] = kl;
    vo[i + 1] = vl;
  });
  if (bad.load() < n) {
    *first_bad = bad.load();
    return set_error(TKV_CORRUPTED, "WAL decode: a record fails wal_entry::decode's structural checks");
  }
  ko[0] = vo[0] = 0;
  for (std::uint64_t i = 0; i < n; ++i) {  // lengths to exclusive prefix sums, the totals last
    ko[i + 1] += ko[i];
    vo[i + 1] += vo[i];
  }
  *keys_size = ko[n];
  *vals_size = vo[n];
  const bool kcopy = !kviews && ko[n] != 0, vcopy = !vviews && vo[n] != 0;
  if ((kcopy && ko[n] > keys_cap) || (vcopy && vo[n] > vals_cap))
    return set_error(TKV_BUFFER_OVERFLOW, "WAL decode: an arena does not fit its cap");
  if ((kcopy && !ptr_ok(h_keys)) || (vcopy && !ptr_ok(h_vals))) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  parallel_for(n, [&](std::uint64_t i) {
    const std::uint64_t off = h_rec_off64[i];
    const std::uint8_t* r = h_img + off;
    const std::uint32_t kl = static_cast<std::uint32_t>(ko[i + 1] - ko[i]), vl = static_cast<std::uint32_t>(vo[i + 1] - vo[i]);
    if (ptr_ok(h_op)) h_op[i] = r[kWalOp];
    if (ptr_ok(h_tomb)) h_tomb[i] = r[kWalTomb];
    if (ptr_ok(h_seq)) std::memcpy(&h_seq[i], r + kWalSeq, 8);
    if (ptr_ok(h_key_len)) h_key_len[i] = kl;
    if (ptr_ok(h_val_len)) h_val_len[i] = vl;
    if (ptr_ok(h_key_off)) h_key_off[i] = kviews ? off + kWalMeta : ko[i];
    if (ptr_ok(h_val_off)) h_val_off[i] = vviews ? off + kWalMeta + kl : vo[i];
    if (kcopy && kl) std::memcpy(h_keys + ko[i], r + kWalMeta, kl);
    if (vcopy && vl) std::memcpy(h_vals + vo[i], r + kWalMeta + kl, vl);
  });
  return TKV_OK;
}


int tkv_sst_stamp_blocks(uint8_t* h_file, const uint64_t* h_offsets, const uint64_t* h_sizes, uint64_t n) {
  if (n == 0) return TKV_OK;
  if (!ptr_ok(h_file) || !ptr_ok(h_offsets) || !ptr_ok(h_sizes)) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  if (int rc = sst_check(h_sizes, n)) return rc;
  std::vector<std::uint32_t> len(n), crc(n);
  parallel_for(n, [&](std::uint64_t i) {
    std::memset(h_file + h_offsets[i] + TKV_SST_CRC_OFFSET, 0, 4);  // the field reads as zero
    len[i] = static_cast<std::uint32_t>(h_sizes[i]);
  });
  if (int rc = batch_host_impl(kAlgoCrc32, h_file, h_offsets, len.data(), nullptr, crc.data(), n)) return rc;
  parallel_for(n, [&](std::uint64_t i) { std::memcpy(h_file + h_offsets[i] + TKV_SST_CRC_OFFSET, &crc[i], 4); });
  return TKV_OK;
}

int tkv_sst_verify_blocks(const uint8_t* h_file, const uint64_t* h_offsets, const uint64_t* h_sizes, uint64_t n,
                          uint64_t* n_bad, uint64_t* first_bad) {
  if (!ptr_ok(n_bad) || !ptr_ok(first_bad)) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  *n_bad = 0;
  *first_bad = n;
  if (n == 0) return TKV_OK;
  if (!ptr_ok(h_file) || !ptr_ok(h_offsets) || !ptr_ok(h_sizes)) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  if (int rc = sst_check(h_sizes, n)) return rc;
  std::vector<std::uint32_t> len(n), got(n);
  for (std::uint64_t i = 0; i < n; ++i) len[i] = static_cast<std::uint32_t>(h_sizes[i]);
  if (int rc = batch_host_impl(kAlgoCrc32, h_file, h_offsets, len.data(), nullptr, got.data(), n)) return rc;
  // stored vs CRC with the field read as zero, on host threads for large files
  const unsigned nt = n >= (1u << 14) ? host_threads() : 1u;
  std::vector<std::uint64_t> bad(nt, 0), first(nt, n);
  auto part = [&](unsigned t) {
    for (std::uint64_t i = n * t / nt; i < n * (t + 1) / nt; ++i) {
      std::uint32_t stored;
      std::memcpy(&stored, h_file + h_offsets[i] + TKV_SST_CRC_OFFSET, 4);
      const std::uint32_t want = got[i] ^ field_term(stored, h_sizes[i] - TKV_SST_CRC_OFFSET - 4);
      if (want != stored) {
        if (bad[t] == 0) first[t] = i;
        ++bad[t];
      }
    }
  };
  pow_tables();
  if (nt == 1) {
    part(0);
  } else {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) th.emplace_back(part, t);
    for (auto& t : th) t.join();
  }
  for (unsigned t = 0; t < nt; ++t) {
    if (bad[t] && *n_bad == 0) *first_bad = first[t];
    *n_bad += bad[t];
  }
  return *n_bad ? set_error(TKV_CORRUPTED, "corrupted SSTable data block") : TKV_OK;
}

int tkv_sst_block_crcs_device(uint8_t* d_file, const uint64_t* d_offsets, const uint32_t* d_sizes, uint32_t* d_out,
                              uint64_t n, int store, void* stream) {
  if (n == 0) return TKV_OK;
  if (!ptr_ok(d_file) || !ptr_ok(d_offsets) || !ptr_ok(d_sizes) || !ptr_ok(d_out))
    return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  if (int rc = batch_device_impl(kAlgoCrc32, d_file, d_offsets, d_sizes, nullptr, d_out, n, stream)) return rc;
  const DeviceTables* tabs = device_tables(kAlgoCrc32);
  if (!tabs) return TKV_IO_ERROR;
  const hipError_t e = launch_sst_fix(d_file, d_offsets, d_sizes, d_out, n, store, tabs, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return set_error(TKV_IO_ERROR, hipGetErrorString(e));
  return TKV_OK;
}

}  // extern "C"

namespace {
// CRC-32 of index image || footer[0, 16): one engine update over the index, chained into a second
// over the footer's fields (the raw register carries across, as crc32::update chaining does).
int footer_crc(const std::uint8_t* h_index, std::uint64_t index_size, const std::uint8_t* h_footer,
               std::uint32_t* crc) {
  if ((index_size && !ptr_ok(h_index)) || !ptr_ok(h_footer)) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  std::uint32_t raw = 0xFFFFFFFFu;
  if (int rc = update_impl(kAlgoCrc32, raw, h_index, index_size, &raw)) return rc;
  if (int rc = update_impl(kAlgoCrc32, raw, h_footer, TKV_SST_FOOTER_CRC_OFFSET, &raw)) return rc;
  *crc = raw ^ 0xFFFFFFFFu;
  return TKV_OK;
}
}  // namespace

extern "C" {

int tkv_sst_stamp_footer(const uint8_t* h_index, uint64_t index_size, uint8_t* h_footer) {
  std::uint32_t crc = 0;
  if (int rc = footer_crc(h_index, index_size, h_footer, &crc)) return rc;
  std::memcpy(h_footer + TKV_SST_FOOTER_CRC_OFFSET, &crc, 4);
  return TKV_OK;
}

int tkv_sst_verify_footer(const uint8_t* h_index, uint64_t index_size, const uint8_t* h_footer) {
  std::uint32_t crc = 0, stored = 0;
  if (int rc = footer_crc(h_index, index_size, h_footer, &crc)) return rc;
  std::memcpy(&stored, h_footer + TKV_SST_FOOTER_CRC_OFFSET, 4);
  return stored == crc ? TKV_OK : set_error(TKV_CORRUPTED, "corrupted SSTable index or footer");
}

}  // extern "C"

namespace {
// ---- SSTable flush (sstable_writer::append ... get_footer for a whole entry list) ---------------------
struct SstIn {
  const std::uint8_t* keys;
  const std::uint64_t* key_off;
  const std::uint32_t* key_len;
  const std::uint8_t* vals;
  const std::uint64_t* val_off;
  const std::uint32_t* val_len;
  std::uint64_t n;
  std::uint32_t T;
};
struct SstOut {
  std::uint8_t* file;
  std::uint64_t cap;
  std::uint64_t* block_off;
  std::uint32_t* block_size;
  std::uint32_t* block_first;
  std::uint64_t block_cap;
  std::uint64_t *file_size, *n_blocks, *index_offset, *index_size;
};
// The cut and the layout of a host entry list.
struct SstPlan {
  std::vector<std::uint64_t> pos;     // file offset of every entry
  std::vector<std::uint32_t> first;   // b_j, B + 1 entries
  std::vector<std::uint64_t> off;     // O_j
  std::vector<std::uint32_t> size;    // 36 + z_j
  std::uint64_t index_offset = 0, index_size = 0, file_size = 0;
};

// The argument checks both entry points share.
int sst_build_check(const SstIn& in, const SstOut& o) {
  if (in.n == 0) return set_error(TKV_INVALID_ARGUMENT, "SSTable build: no entries");
  if (in.n > 0xFFFFFFFFull) return set_error(TKV_INVALID_ARGUMENT, "SSTable build: more than 2^32 - 1 entries");
  if (in.T == 0) return set_error(TKV_INVALID_ARGUMENT, "SSTable build: target_block_size is 0");
  if (!ptr_ok(in.keys) || !ptr_ok(in.key_off) || !ptr_ok(in.key_len) ||
      (ptr_ok(in.val_len) && (!ptr_ok(in.vals) || !ptr_ok(in.val_off))) || !ptr_ok(o.file_size) || !ptr_ok(o.n_blocks) ||
      !ptr_ok(o.index_offset) || !ptr_ok(o.index_size) || (o.cap && !ptr_ok(o.file)))
    return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  return TKV_OK;
}

// Sizes, the greedy cut (append, then is_data_block_complete: size >= target) and every offset; no
// source byte is read.
int sst_build_plan(const SstIn& in, SstPlan& p) {
  for (std::uint64_t i = 0; i < in.n; ++i)
    if (in.key_len[i] >= kSstMaxLen || (in.val_len && in.val_len[i] >= kSstMaxLen))
      return set_error(TKV_INVALID_ARGUMENT, "SSTable build: a key or value length is 2^28 or more");
  p.pos.resize(in.n);
  std::uint64_t file = 0, b = 0;
  while (b < in.n) {
    std::uint64_t z = 0, m = b;
    while (m < in.n && z < in.T) {
      z += sst_counted(in.key_len[m], in.val_len ? in.val_len[m] : 0u);
      ++m;
    }
    if (kSstOverhead + z > 0xFFFFFFFFull) return set_error(TKV_INVALID_ARGUMENT, "SSTable build: a data block does not fit u32");
    std::uint64_t at = file + kSstHeader + sst_vlen(z);
    for (std::uint64_t i = b; i < m; ++i) {
      p.pos[i] = at;
      at += sst_written(in.key_len[i], in.val_len ? in.val_len[i] : 0u);
    }
    p.first.push_back(static_cast<std::uint32_t>(b));
    p.off.push_back(file);
    p.size.push_back(static_cast<std::uint32_t>(kSstOverhead + z));
    file += kSstOverhead + z;
    b = m;
  }
  p.first.push_back(static_cast<std::uint32_t>(in.n));
  p.index_offset = file;
  p.index_size = 8;
  for (std::size_t j = 0; j + 1 < p.first.size(); ++j) {
    const std::uint32_t kl = in.key_len[p.first[j]];
    p.index_size += std::uint64_t(sst_vlen(kl)) + kl + kSstIndexFixed;
  }
  p.file_size = p.index_offset + p.index_size + kSstFooter;
  if (p.file_size > 0xFFFFFFFFull) return set_error(TKV_INVALID_ARGUMENT, "SSTable build: the file does not fit u32");
  return TKV_OK;
}

// The file image with every CRC field zero, entries on host threads.
void sst_build_layout(const SstIn& in, const SstPlan& p, std::uint8_t* f) {
  const std::uint64_t B = p.off.size();
  std::memset(f, 0, p.index_offset);  // slack and padding
  parallel_for(B, [&](std::uint64_t j) {
    std::uint8_t h[32];
    const std::uint32_t nh = sst_block_head(h, p.first[j + 1] - p.first[j], p.size[j] - kSstOverhead);
    std::memcpy(f + p.off[j], h, nh);
  });
  parallel_for(in.n, [&](std::uint64_t i) {
    std::uint8_t* d = f + p.pos[i];
    const std::uint32_t kl = in.key_len[i], vl = in.val_len ? in.val_len[i] : 0u;
    d += sst_put_varint(d, kl);
    if (kl) std::memcpy(d, in.keys + in.key_off[i], kl);
    d += kl;
    d += sst_put_varint(d, vl);
    if (vl) std::memcpy(d, in.vals + in.val_off[i], vl);
  });
  std::uint8_t* d = f + p.index_offset;
  for (int b = 0; b < 8; ++b) *d++ = static_cast<std::uint8_t>(B >> (8 * b));
  for (std::uint64_t j = 0; j < B; ++j) {
    const std::uint64_t i = p.first[j];
    const std::uint32_t kl = in.key_len[i];
    d += sst_put_varint(d, kl);
    if (kl) std::memcpy(d, in.keys + in.key_off[i], kl);
    d += kl;
    const std::uint64_t sz = p.size[j];
    for (int b = 0; b < 8; ++b) *d++ = static_cast<std::uint8_t>(p.off[j] >> (8 * b));
    for (int b = 0; b < 8; ++b) *d++ = static_cast<std::uint8_t>(sz >> (8 * b));
  }
  const std::uint32_t foot[5] = {static_cast<std::uint32_t>(p.index_offset), static_cast<std::uint32_t>(p.index_size), 0u, 0u, 0u};
  for (int k = 0; k < 5; ++k)
    for (int b = 0; b < 4; ++b) *d++ = static_cast<std::uint8_t>(foot[k] >> (8 * b));
}

// Checks, the plan, the sizes, overflow, the layout and the block arrays of a host build.
int sst_build_host_layout(const SstIn& in, const SstOut& o, SstPlan& p) {
  if (int rc = sst_build_check(in, o)) return rc;
  if (int rc = sst_build_plan(in, p)) return rc;
  const std::uint64_t B = p.off.size();
  *o.file_size = p.file_size;
  *o.n_blocks = B;
  *o.index_offset = p.index_offset;
  *o.index_size = p.index_size;
  const bool want_blocks = ptr_ok(o.block_off) || ptr_ok(o.block_size) || ptr_ok(o.block_first);
  if (p.file_size > o.cap || (want_blocks && B > o.block_cap))
    return set_error(TKV_BUFFER_OVERFLOW, "SSTable build: the file or the block arrays do not fit");
  if (!ptr_ok(o.file)) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  sst_build_layout(in, p, o.file);
  if (ptr_ok(o.block_off)) std::memcpy(o.block_off, p.off.data(), B * sizeof(std::uint64_t));
  if (ptr_ok(o.block_size)) std::memcpy(o.block_size, p.size.data(), B * sizeof(std::uint32_t));
  if (ptr_ok(o.block_first)) std::memcpy(o.block_first, p.first.data(), B * sizeof(std::uint32_t));
  return TKV_OK;
}
}  // namespace

extern "C" {

int tkv_sst_build_device(const uint8_t* d_keys, const uint64_t* d_key_off, const uint32_t* d_key_len, const uint8_t* d_vals,
                         const uint64_t* d_val_off, const uint32_t* d_val_len, uint64_t n, uint32_t target_block_size,
                         uint8_t* d_file, uint64_t cap, uint64_t* d_block_off, uint32_t* d_block_size,
                         uint32_t* d_block_first, uint64_t block_cap, uint64_t* file_size, uint64_t* n_blocks,
                         uint64_t* index_offset, uint64_t* index_size, void* stream) {
  const SstIn in{d_keys, d_key_off, d_key_len, d_vals, d_val_off, d_val_len, n, target_block_size};
  const SstOut o{d_file, cap, d_block_off, d_block_size, d_block_first, block_cap, file_size, n_blocks, index_offset, index_size};
  if (int rc = sst_build_check(in, o)) return rc;
  return sst_build_device_impl(d_keys, d_key_off, d_key_len, d_vals, d_val_off, d_val_len, n, target_block_size, d_file, cap,
                               d_block_off, d_block_size, d_block_first, block_cap, file_size, n_blocks, index_offset,
                               index_size, static_cast<hipStream_t>(stream));
}

int tkv_sst_build(const uint8_t* h_keys, const uint64_t* h_key_off, const uint32_t* h_key_len, const uint8_t* h_vals,
                  const uint64_t* h_val_off, const uint32_t* h_val_len, uint64_t n, uint32_t target_block_size,
                  uint8_t* h_file, uint64_t cap, uint64_t* h_block_off, uint32_t* h_block_size, uint32_t* h_block_first,
                  uint64_t block_cap, uint64_t* file_size, uint64_t* n_blocks, uint64_t* index_offset,
                  uint64_t* index_size) {
  const SstIn in{h_keys, h_key_off, h_key_len, h_vals, h_val_off, h_val_len, n, target_block_size};
  const SstOut o{h_file, cap, h_block_off, h_block_size, h_block_first, block_cap, file_size, n_blocks, index_offset, index_size};
  SstPlan p;
  if (int rc = sst_build_host_layout(in, o, p)) return rc;
  // the stamps of tkv_sst_stamp_blocks and tkv_sst_stamp_footer: the fields are zero, so the plain CRC
  // of an image is its stamp
  const std::uint64_t B = p.off.size();
  std::vector<std::uint32_t> crc(B);
  if (int rc = batch_host_impl(kAlgoCrc32, h_file, p.off.data(), p.size.data(), nullptr, crc.data(), B)) return rc;
  parallel_for(B, [&](std::uint64_t j) { std::memcpy(h_file + p.off[j] + TKV_SST_CRC_OFFSET, &crc[j], 4); });
  return tkv_sst_stamp_footer(h_file + p.index_offset, p.index_size, h_file + p.index_offset + p.index_size);
}

int tkv_debug_sst_build_layout(const uint8_t* h_keys, const uint64_t* h_key_off, const uint32_t* h_key_len,
                               const uint8_t* h_vals, const uint64_t* h_val_off, const uint32_t* h_val_len, uint64_t n,
                               uint32_t target_block_size, uint8_t* h_file, uint64_t cap, uint64_t* h_block_off,
                               uint32_t* h_block_size, uint32_t* h_block_first, uint64_t block_cap, uint64_t* file_size,
                               uint64_t* n_blocks, uint64_t* index_offset, uint64_t* index_size) {
  const SstIn in{h_keys, h_key_off, h_key_len, h_vals, h_val_off, h_val_len, n, target_block_size};
  const SstOut o{h_file, cap, h_block_off, h_block_size, h_block_first, block_cap, file_size, n_blocks, index_offset, index_size};
  SstPlan p;
  return sst_build_host_layout(in, o, p);
}

size_t tkv_debug_wal_chain(const uint8_t* h_wal, uint64_t size, uint64_t* out_pos, size_t cap, uint64_t* end,
                           int* err) {
  const Chain c = wal_chain(h_wal, size);
  if (out_pos) std::memcpy(out_pos, c.pos.data(), std::min(cap, c.pos.size()) * sizeof(std::uint64_t));
  if (end) *end = c.end;
  if (err) *err = c.err ? 1 : 0;
  return c.pos.size();
}

}  // extern "C"

namespace {
// ---- SSTable scan (the reader of what tkv_sst_build writes; include/tkv_crc32.h "SSTable scan") --------
struct ScanIn {
  const std::uint8_t* file;
  std::uint64_t size;
  std::uint32_t flags;
};
struct ScanOut {
  std::uint64_t* key_off;
  std::uint32_t* key_len;
  std::uint64_t* val_off;
  std::uint32_t* val_len;
  std::uint64_t entry_cap;
  std::uint8_t* keys;
  std::uint64_t keys_cap;
  std::uint8_t* vals;
  std::uint64_t vals_cap;
  std::uint64_t* block_off;
  std::uint32_t* block_size;
  std::uint32_t* block_first;
  std::uint64_t block_cap;
  std::uint64_t *n_entries, *n_blocks, *keys_size, *vals_size, *bad_block;
};

// The argument checks both entry points share: decided before any device work.
int sst_scan_check(const ScanIn& in, const ScanOut& o) {
  if ((in.size && !ptr_ok(in.file)) || !ptr_ok(o.n_entries) || !ptr_ok(o.n_blocks) || !ptr_ok(o.keys_size) ||
      !ptr_ok(o.vals_size) || !ptr_ok(o.bad_block))
    return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  if (in.flags & ~(TKV_SST_SCAN_KEY_VIEWS | TKV_SST_SCAN_VAL_VIEWS)) return set_error(TKV_INVALID_ARGUMENT, "SSTable scan: unknown flag");
  if (in.size > 0xFFFFFFFFull) return set_error(TKV_INVALID_ARGUMENT, "SSTable scan: the file does not fit u32");
  return TKV_OK;
}

int sst_scan_corrupted(const ScanOut& o, std::uint64_t bad, const char* msg) {
  *o.bad_block = bad;
  *o.n_entries = *o.n_blocks = *o.keys_size = *o.vals_size = 0;
  return set_error(TKV_CORRUPTED, msg);
}

// The min(avail, maxb) bytes at p as a word: no byte behind p + avail is read.
std::uint64_t bytes_word(const std::uint8_t* p, std::uint64_t avail, std::uint32_t maxb) {
  std::uint64_t w = 0;
  for (std::uint32_t k = 0; k < maxb && k < avail; ++k) w |= static_cast<std::uint64_t>(p[k]) << (8u * k);
  return w;
}
std::uint64_t le_bytes(const std::uint8_t* p, int n) {
  std::uint64_t v = 0;
  for (int b = 0; b < n; ++b) v |= static_cast<std::uint64_t>(p[b]) << (8 * b);
  return v;
}

struct ScanBlock {
  std::uint64_t off, size;   // the image
  std::uint64_t ikey;        // file offset of the index entry's key
  std::uint32_t ikl;
};
struct ScanRec {
  std::uint64_t kpos, vpos;  // file offsets of the key's and the value's bytes
  std::uint32_t kl, vl;
};

// Block b's checks (all but the checksum) and its walk: the entry count, or 0 when a check fails (a
// valid block holds at least one entry). rec != nullptr: the c records are written there.
std::uint32_t sst_scan_block(const std::uint8_t* file, const ScanBlock& b, ScanRec* rec) {
  const std::uint8_t* img = file + b.off;
  const std::uint32_t c = static_cast<std::uint32_t>(le_bytes(img + 1, 4)), z = static_cast<std::uint32_t>(le_bytes(img + 5, 4));
  const std::uint64_t vavail = b.size - kSstHeader;
  const SstVarint zv = sst_varint_word(bytes_word(img + kSstHeader, vavail, kSstBodyLenBytes), vavail, kSstBodyLenBytes);
  if (!sst_block_header_ok(img[0], c, z, static_cast<std::uint32_t>(le_bytes(img + 9, 4)), img[13], b.size, zv)) return 0;
  const std::uint8_t* body = img + kSstHeader + zv.n;
  const std::uint64_t bpos = b.off + kSstHeader + zv.n;
  std::uint64_t q = 0, sum = 0, kq = 0;
  std::uint32_t kl = 0;
  for (std::uint32_t r = 0; r < 2u * c; ++r) {
    if (q >= z) return 0;
    const SstLink s = sst_chain_next(static_cast<std::uint32_t>(bytes_word(body + q, z - q, kSstLenBytes)), q, z, 0u);
    if (!s.ok) return 0;
    if (!(r & 1u)) {
      kq = q + s.n;
      kl = s.len;
      if (r == 0 && (kl != b.ikl || (kl && std::memcmp(body + kq, file + b.ikey, kl) != 0))) return 0;
    } else {
      sum += sst_counted(kl, s.len);
      if (rec) rec[r >> 1] = ScanRec{bpos + kq, bpos + q + s.n, kl, s.len};
    }
    q = s.next;
  }
  return sum == z ? c : 0u;
}

// fn(t, lo, hi) for the ranges [lo, hi) of [0, n) on host threads: one task per range of blocks.
template <class F>
void parallel_ranges(std::uint64_t n, F fn) {
  const unsigned nt = n >= 64 ? static_cast<unsigned>(std::min<std::uint64_t>(host_threads(), n / 32)) : 1u;
  if (nt <= 1) {
    fn(0u, std::uint64_t(0), n);
    return;
  }
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t) th.emplace_back([=] { fn(t, n * t / nt, n * (t + 1) / nt); });
  for (auto& t : th) t.join();
}

// The scan of a host image; crc = false skips every checksum comparison (tkv_debug_sst_scan_parse).
int sst_scan_host(const ScanIn& in, const ScanOut& o, bool crc) {
  if (int rc = sst_scan_check(in, o)) return rc;
  const std::uint8_t* f = in.file;
  // footer
  if (in.size < kSstMinFile) return sst_scan_corrupted(o, TKV_SST_BAD_FOOTER, "SSTable scan: the file is shorter than an index and a footer");
  const std::uint8_t* foot = f + (in.size - kSstFooter);
  const std::uint32_t ioff32 = static_cast<std::uint32_t>(le_bytes(foot, 4)), isz32 = static_cast<std::uint32_t>(le_bytes(foot + 4, 4));
  if (!sst_footer_ok(in.size, ioff32, isz32))
    return sst_scan_corrupted(o, TKV_SST_BAD_FOOTER, "SSTable scan: the footer does not describe this file");
  const std::uint64_t ioff = ioff32, isz = isz32;
  if (crc) {
    const int rc = tkv_sst_verify_footer(f + ioff, isz, foot);
    if (rc == TKV_CORRUPTED) return sst_scan_corrupted(o, TKV_SST_BAD_FOOTER, "SSTable scan: corrupted index or footer");
    if (rc) return rc;
  }
  // index
  const std::uint8_t* idx = f + ioff;
  const std::uint64_t B = le_bytes(idx, 8);
  bool iok = sst_index_count_ok(B, isz);
  std::vector<ScanBlock> blk;
  if (iok) {
    blk.resize(B);
    std::uint64_t p = 8;
    for (std::uint64_t j = 0; j < B && iok; ++j) {
      iok = p < isz;
      if (!iok) break;
      const SstLink s = sst_chain_next(static_cast<std::uint32_t>(bytes_word(idx + p, isz - p, kSstLenBytes)), p, isz, kSstIndexFixed);
      iok = s.ok;
      if (!iok) break;
      const std::uint8_t* e = idx + p + s.n + s.len;
      blk[j] = ScanBlock{le_bytes(e, 8), le_bytes(e + 8, 8), ioff + p + s.n, s.len};
      iok = sst_index_block_ok(blk[j].off, blk[j].size, ioff);
      p = s.next;
    }
    iok = iok && p == isz;
  }
  if (!iok) return sst_scan_corrupted(o, TKV_SST_BAD_INDEX, "SSTable scan: the index framing does not hold");
  // blocks: the checksums through tkv_sst_verify_blocks' path, the parse on host threads
  std::uint64_t bad = B;
  if (crc && B) {
    std::vector<std::uint64_t> off(B), size(B);
    for (std::uint64_t j = 0; j < B; ++j) {
      off[j] = blk[j].off;
      size[j] = blk[j].size;
    }
    std::uint64_t n_bad = 0, first_bad = B;
    const int rc = tkv_sst_verify_blocks(f, off.data(), size.data(), B, &n_bad, &first_bad);
    if (rc == TKV_CORRUPTED) bad = first_bad;
    else if (rc) return rc;
  }
  std::vector<std::uint64_t> first(B + 1, 0);
  {
    std::vector<std::uint64_t> tbad(host_threads() + 1u, B);
    parallel_ranges(B, [&](unsigned t, std::uint64_t lo, std::uint64_t hi) {
      for (std::uint64_t j = lo; j < hi; ++j) {
        first[j + 1] = sst_scan_block(f, blk[j], nullptr);
        if (!first[j + 1] && tbad[t] == B) tbad[t] = j;
      }
    });
    for (std::uint64_t v : tbad) bad = std::min(bad, v);
  }
  if (bad < B) return sst_scan_corrupted(o, bad, "SSTable scan: corrupted data block");
  for (std::uint64_t j = 0; j < B; ++j) first[j + 1] += first[j];
  const std::uint64_t n = first[B];
  std::vector<ScanRec> rec(n);
  parallel_ranges(B, [&](unsigned, std::uint64_t lo, std::uint64_t hi) {
    for (std::uint64_t j = lo; j < hi; ++j) (void)sst_scan_block(f, blk[j], rec.data() + first[j]);
  });
  std::vector<std::uint64_t> ko(n + 1, 0), vo(n + 1, 0);
  for (std::uint64_t i = 0; i < n; ++i) {
    ko[i + 1] = ko[i] + rec[i].kl;
    vo[i + 1] = vo[i] + rec[i].vl;
  }
  *o.n_entries = n;
  *o.n_blocks = B;
  *o.keys_size = ko[n];
  *o.vals_size = vo[n];
  *o.bad_block = B;
  const bool kviews = in.flags & TKV_SST_SCAN_KEY_VIEWS, vviews = in.flags & TKV_SST_SCAN_VAL_VIEWS;
  const bool want_entries = ptr_ok(o.key_off) || ptr_ok(o.key_len) || ptr_ok(o.val_off) || ptr_ok(o.val_len);
  const bool want_blocks = ptr_ok(o.block_off) || ptr_ok(o.block_size) || ptr_ok(o.block_first);
  if ((want_entries && n > o.entry_cap) || (want_blocks && B > o.block_cap) || (!kviews && ko[n] > o.keys_cap) ||
      (!vviews && vo[n] > o.vals_cap))
    return set_error(TKV_BUFFER_OVERFLOW, "SSTable scan: an output does not fit its cap");
  const bool kcopy = !kviews && ptr_ok(o.keys), vcopy = !vviews && ptr_ok(o.vals);
  for (std::uint64_t j = 0; j < B; ++j) {
    if (ptr_ok(o.block_off)) o.block_off[j] = blk[j].off;
    if (ptr_ok(o.block_size)) o.block_size[j] = static_cast<std::uint32_t>(blk[j].size);
    if (ptr_ok(o.block_first)) o.block_first[j] = static_cast<std::uint32_t>(first[j]);
  }
  parallel_ranges(n, [&](unsigned, std::uint64_t lo, std::uint64_t hi) {
    for (std::uint64_t i = lo; i < hi; ++i) {
      const ScanRec& r = rec[i];
      if (ptr_ok(o.key_len)) o.key_len[i] = r.kl;
      if (ptr_ok(o.val_len)) o.val_len[i] = r.vl;
      if (ptr_ok(o.key_off)) o.key_off[i] = kviews ? r.kpos : ko[i];
      if (ptr_ok(o.val_off)) o.val_off[i] = vviews ? r.vpos : vo[i];
      if (kcopy && r.kl) std::memcpy(o.keys + ko[i], f + r.kpos, r.kl);
      if (vcopy && r.vl) std::memcpy(o.vals + vo[i], f + r.vpos, r.vl);
    }
  });
  return TKV_OK;
}
}  // namespace

extern "C" {

int tkv_sst_scan_device(const uint8_t* d_file, uint64_t file_size, uint32_t flags, uint64_t* d_key_off, uint32_t* d_key_len,
                        uint64_t* d_val_off, uint32_t* d_val_len, uint64_t entry_cap, uint8_t* d_keys, uint64_t keys_cap,
                        uint8_t* d_vals, uint64_t vals_cap, uint64_t* d_block_off, uint32_t* d_block_size,
                        uint32_t* d_block_first, uint64_t block_cap, uint64_t* n_entries, uint64_t* n_blocks,
                        uint64_t* keys_size, uint64_t* vals_size, uint64_t* bad_block, void* stream) {
  const ScanIn in{d_file, file_size, flags};
  const ScanOut o{d_key_off, d_key_len, d_val_off, d_val_len, entry_cap, d_keys, keys_cap, d_vals, vals_cap, d_block_off,
                  d_block_size, d_block_first, block_cap, n_entries, n_blocks, keys_size, vals_size, bad_block};
  if (int rc = sst_scan_check(in, o)) return rc;
  if (file_size < kSstMinFile) return sst_scan_corrupted(o, TKV_SST_BAD_FOOTER, "SSTable scan: the file is shorter than an index and a footer");
  return sst_scan_device_impl(d_file, file_size, flags, d_key_off, d_key_len, d_val_off, d_val_len, entry_cap, d_keys, keys_cap,
                              d_vals, vals_cap, d_block_off, d_block_size, d_block_first, block_cap, n_entries, n_blocks,
                              keys_size, vals_size, bad_block, static_cast<hipStream_t>(stream));
}

int tkv_sst_scan(const uint8_t* h_file, uint64_t file_size, uint32_t flags, uint64_t* h_key_off, uint32_t* h_key_len,
                 uint64_t* h_val_off, uint32_t* h_val_len, uint64_t entry_cap, uint8_t* h_keys, uint64_t keys_cap,
                 uint8_t* h_vals, uint64_t vals_cap, uint64_t* h_block_off, uint32_t* h_block_size, uint32_t* h_block_first,
                 uint64_t block_cap, uint64_t* n_entries, uint64_t* n_blocks, uint64_t* keys_size, uint64_t* vals_size,
                 uint64_t* bad_block) {
  const ScanIn in{h_file, file_size, flags};
  const ScanOut o{h_key_off, h_key_len, h_val_off, h_val_len, entry_cap, h_keys, keys_cap, h_vals, vals_cap, h_block_off,
                  h_block_size, h_block_first, block_cap, n_entries, n_blocks, keys_size, vals_size, bad_block};
  return sst_scan_host(in, o, true);
}

int tkv_debug_sst_scan_parse(const uint8_t* h_file, uint64_t file_size, uint32_t flags, uint64_t* h_key_off,
                             uint32_t* h_key_len, uint64_t* h_val_off, uint32_t* h_val_len, uint64_t entry_cap,
                             uint8_t* h_keys, uint64_t keys_cap, uint8_t* h_vals, uint64_t vals_cap, uint64_t* h_block_off,
                             uint32_t* h_block_size, uint32_t* h_block_first, uint64_t block_cap, uint64_t* n_entries,
                             uint64_t* n_blocks, uint64_t* keys_size, uint64_t* vals_size, uint64_t* bad_block) {
  const ScanIn in{h_file, file_size, flags};
  const ScanOut o{h_key_off, h_key_len, h_val_off, h_val_len, entry_cap, h_keys, keys_cap, h_vals, vals_cap, h_block_off,
                  h_block_size, h_block_first, block_cap, n_entries, n_blocks, keys_size, vals_size, bad_block};
  return sst_scan_host(in, o, false);
}

}  // extern "C"

namespace {
// ---- memtable replay (engine::create's replay loop into a memtable; include/tkv_crc32.h "Memtable replay") ----

// The checks both entry points make before any work.
int memtable_check(const MemtableCall& c) {
  if (!ptr_ok(c.n_entries) || !ptr_ok(c.ikeys_size) || !ptr_ok(c.first_bad)) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  if (c.n > 0xFFFFFFFFull) return set_error(TKV_INVALID_ARGUMENT, "memtable build: more than 2^32 - 1 records");
  if (c.n && (!ptr_ok(c.key_off) || !ptr_ok(c.key_len) || (c.keys_size && !ptr_ok(c.keys)) ||
              (ptr_ok(c.val_len) && !ptr_ok(c.val_off))))
    return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  return TKV_OK;
}

// idx sorted by less, equal elements left in their order: chunks on host threads, then pairwise merges.
template <class Less>
void parallel_stable_sort(std::vector<std::uint32_t>& idx, Less less) {
  const std::uint64_t n = idx.size();
  const unsigned nt = n >= (1u << 14) ? host_threads() : 1u;
  if (nt == 1) {
    std::stable_sort(idx.begin(), idx.end(), less);
    return;
  }
  std::vector<std::uint64_t> cut(nt + 1);
  for (unsigned t = 0; t <= nt; ++t) cut[t] = n * t / nt;
  {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t)
      th.emplace_back([&, t] { std::stable_sort(idx.begin() + cut[t], idx.begin() + cut[t + 1], less); });
    for (auto& t : th) t.join();
  }
  for (unsigned w = 1; w < nt; w *= 2) {
    std::vector<std::thread> th;
    for (unsigned t = 0; t + w < nt; t += 2 * w)
      th.emplace_back([&, t, w] {
        std::inplace_merge(idx.begin() + cut[t], idx.begin() + cut[t + w], idx.begin() + cut[std::min(t + 2 * w, nt)], less);
      });
    for (auto& t : th) t.join();
  }
}

int memtable_build_host(const MemtableCall& c) {
  if (int rc = memtable_check(c)) return rc;
  const std::uint64_t n = c.n;
  if (n == 0) {
    *c.n_entries = *c.ikeys_size = *c.first_bad = 0;
    return TKV_OK;
  }
  std::uint64_t bad = n;
  for (std::uint64_t i = 0; i < n; ++i) {
    const std::uint64_t ko = c.key_off[i];
    const std::uint32_t kl = c.key_len[i];
    if (ko > c.keys_size || kl > c.keys_size - ko) return set_error(TKV_INVALID_ARGUMENT, "memtable build: a key reaches past keys_size");
    if (kl >= kMtMaxIkey - kMtMeta) return set_error(TKV_INVALID_ARGUMENT, "memtable build: an internal key would be 2^28 bytes or more");
    if (bad == n && ptr_ok(c.op) && c.op[i] > kMtOpDel) bad = i;
  }
  *c.n_entries = 0;
  *c.ikeys_size = 0;
  *c.first_bad = bad;
  if (bad < n) return set_error(TKV_CORRUPTED, "memtable build: a record's operation is neither put nor delete");
  // simd_comparator's order: unsigned bytes, a prefix first
  auto cmp = [&](std::uint32_t x, std::uint32_t y) {
    const std::uint32_t lx = c.key_len[x], ly = c.key_len[y];
    const std::uint32_t m = std::min(lx, ly);
    const int r = m ? std::memcmp(c.keys + c.key_off[x], c.keys + c.key_off[y], m) : 0;
    return r ? r : (lx < ly ? -1 : lx > ly ? 1 : 0);
  };
  std::vector<std::uint32_t> idx(n);
  for (std::uint64_t i = 0; i < n; ++i) idx[i] = static_cast<std::uint32_t>(i);
  parallel_stable_sort(idx, [&](std::uint32_t x, std::uint32_t y) { return cmp(x, y) < 0; });
  // the last of every run of equal keys
  std::vector<std::uint32_t> sv;
  std::vector<std::uint64_t> off;
  std::uint64_t total = 0;
  for (std::uint64_t j = 0; j < n; ++j) {
    if (j + 1 < n && cmp(idx[j], idx[j + 1]) == 0) continue;
    sv.push_back(idx[j]);
    off.push_back(total);
    total += static_cast<std::uint64_t>(c.key_len[idx[j]]) + kMtMeta;
  }
  const std::uint64_t m = sv.size();
  *c.n_entries = m;
  *c.ikeys_size = total;
  const bool want_cols = ptr_ok(c.ikey_off) || ptr_ok(c.ikey_len) || ptr_ok(c.out_val_off) || ptr_ok(c.out_val_len) || ptr_ok(c.src);
  if ((want_cols && m > c.entry_cap) || (ptr_ok(c.ikeys) && total > c.ikeys_cap))
    return set_error(TKV_BUFFER_OVERFLOW, "memtable build: the entries or the internal keys do not fit");
  parallel_for(m, [&](std::uint64_t e) {
    const std::uint32_t r = sv[e];
    const std::uint32_t kl = c.key_len[r];
    const bool del = ptr_ok(c.op) && c.op[r] == kMtOpDel;
    if (ptr_ok(c.ikey_off)) c.ikey_off[e] = off[e];
    if (ptr_ok(c.ikey_len)) c.ikey_len[e] = kl + kMtMeta;
    if (ptr_ok(c.out_val_off)) c.out_val_off[e] = ptr_ok(c.val_off) ? c.val_off[r] : 0u;
    if (ptr_ok(c.out_val_len)) c.out_val_len[e] = (del || !ptr_ok(c.val_len)) ? 0u : c.val_len[r];
    if (ptr_ok(c.src)) c.src[e] = r;
    if (ptr_ok(c.ikeys)) {
      std::uint8_t* d = c.ikeys + off[e];
      if (kl) std::memcpy(d, c.keys + c.key_off[r], kl);
      mt_put_meta(d + kl, ptr_ok(c.seq) ? c.seq[r] : 0u, c.timestamp_ms, ptr_ok(c.tomb) ? c.tomb[r] : std::uint8_t{0});
    }
  });
  return TKV_OK;
}
}  // namespace

extern "C" {

int tkv_memtable_build_device(const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_off, const uint32_t* d_key_len,
                              const uint64_t* d_val_off, const uint32_t* d_val_len, const uint8_t* d_op, const uint8_t* d_tomb,
                              const uint64_t* d_seq, uint64_t n, uint64_t timestamp_ms, uint8_t* d_ikeys, uint64_t ikeys_cap,
                              uint64_t* d_ikey_off, uint32_t* d_ikey_len, uint64_t* d_out_val_off, uint32_t* d_out_val_len,
                              uint32_t* d_src, uint64_t entry_cap, uint64_t* n_entries, uint64_t* ikeys_size,
                              uint64_t* first_bad, void* stream) {
  const MemtableCall c{d_keys, keys_size, d_key_off, d_key_len, d_val_off, d_val_len, d_op, d_tomb, d_seq, n, timestamp_ms,
                       d_ikeys, ikeys_cap, d_ikey_off, d_ikey_len, d_out_val_off, d_out_val_len, d_src, entry_cap,
                       n_entries, ikeys_size, first_bad};
  if (int rc = memtable_check(c)) return rc;
  if (n == 0) {
    *n_entries = *ikeys_size = *first_bad = 0;
    return TKV_OK;
  }
  return memtable_build_device_impl(c, static_cast<hipStream_t>(stream));
}

int tkv_memtable_build(const uint8_t* h_keys, uint64_t keys_size, const uint64_t* h_key_off, const uint32_t* h_key_len,
                       const uint64_t* h_val_off, const uint32_t* h_val_len, const uint8_t* h_op, const uint8_t* h_tomb,
                       const uint64_t* h_seq, uint64_t n, uint64_t timestamp_ms, uint8_t* h_ikeys, uint64_t ikeys_cap,
                       uint64_t* h_ikey_off, uint32_t* h_ikey_len, uint64_t* h_out_val_off, uint32_t* h_out_val_len,
                       uint32_t* h_src, uint64_t entry_cap, uint64_t* n_entries, uint64_t* ikeys_size, uint64_t* first_bad) {
  const MemtableCall c{h_keys, keys_size, h_key_off, h_key_len, h_val_off, h_val_len, h_op, h_tomb, h_seq, n, timestamp_ms,
                       h_ikeys, ikeys_cap, h_ikey_off, h_ikey_len, h_out_val_off, h_out_val_len, h_src, entry_cap,
                       n_entries, ikeys_size, first_bad};
  return memtable_build_host(c);
}

}  // extern "C"

namespace {
// ---- SSTable merge (compaction's k-way merge of sorted runs; include/tkv_crc32.h "SSTable merge") ----

constexpr std::uint64_t kMergeNone = TKV_SST_MERGE_NONE;

// The checks both entry points make before any work; *total = N.
int sst_merge_check(const SstMergeCall& c, std::uint64_t* total) {
  *total = 0;
  if (!ptr_ok(c.n_entries) || !ptr_ok(c.keys_bytes) || !ptr_ok(c.vals_bytes) || !ptr_ok(c.first_bad))
    return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  if (c.n_runs > TKV_SST_MERGE_MAX_RUNS) return set_error(TKV_INVALID_ARGUMENT, "sst merge: more than 64 runs");
  if (c.flags & ~TKV_SST_MERGE_DROP_TOMBSTONES) return set_error(TKV_INVALID_ARGUMENT, "sst merge: unknown flag bits");
  if (c.n_runs == 0) return TKV_OK;
  if (!ptr_ok(c.keys) || !ptr_ok(c.keys_size) || !ptr_ok(c.key_off) || !ptr_ok(c.key_len) || !ptr_ok(c.n))
    return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  std::uint64_t sum = 0;
  for (std::uint32_t r = 0; r < c.n_runs; ++r) {
    if (c.n[r] > 0xFFFFFFFFull) return set_error(TKV_INVALID_ARGUMENT, "sst merge: more than 2^32 - 1 entries in a run");
    sum += c.n[r];
    if (sum > 0xFFFFFFFFull) return set_error(TKV_INVALID_ARGUMENT, "sst merge: more than 2^32 - 1 entries");
    if (ptr_ok(c.val_len) && ptr_ok(c.val_len[r]) && !(ptr_ok(c.val_off) && ptr_ok(c.val_off[r])))
      return set_error(TKV_INVALID_ARGUMENT, "sst merge: val_len without val_off");
    if (c.n[r] == 0) continue;
    if (!ptr_ok(c.keys[r]) || !ptr_ok(c.key_off[r]) || !ptr_ok(c.key_len[r])) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
    if (ptr_ok(c.out_key_off) && (!ptr_ok(c.key_base) || c.key_base > c.keys[r]))
      return set_error(TKV_INVALID_ARGUMENT, "sst merge: key_base is not below every run's keys");
  }
  *total = sum;
  return TKV_OK;
}

// N == 0 (both entry points).
int sst_merge_empty(const SstMergeCall& c) {
  *c.n_entries = *c.keys_bytes = *c.vals_bytes = 0;
  *c.first_bad = kMergeNone;
  return TKV_OK;
}

int sst_merge_host(const SstMergeCall& c) {
  std::uint64_t total = 0;
  if (int rc = sst_merge_check(c, &total)) return rc;
  if (total == 0) return sst_merge_empty(c);
  const std::uint32_t K = c.n_runs;
  auto span_ok = [&](std::uint32_t r, std::uint64_t i) {
    const std::uint64_t ko = c.key_off[r][i];
    const std::uint32_t kl = c.key_len[r][i];
    return kl >= kMtMeta && kl < kMtMaxIkey && ko <= c.keys_size[r] && kl <= c.keys_size[r] - ko;
  };
  // simd_comparator's order on the user keys: unsigned bytes, a prefix first
  auto cmp = [&](std::uint64_t x, std::uint64_t y) {
    const std::uint32_t rx = static_cast<std::uint32_t>(x >> 32), ry = static_cast<std::uint32_t>(y >> 32);
    const std::uint64_t ix = x & 0xFFFFFFFFull, iy = y & 0xFFFFFFFFull;
    const std::uint32_t lx = c.key_len[rx][ix] - kMtMeta, ly = c.key_len[ry][iy] - kMtMeta;
    const std::uint32_t m = std::min(lx, ly);
    const int v = m ? std::memcmp(c.keys[rx] + c.key_off[rx][ix], c.keys[ry] + c.key_off[ry][iy], m) : 0;
    return v ? v : (lx < ly ? -1 : lx > ly ? 1 : 0);
  };
  // validate: every run's smallest bad index on host threads, the runs in order
  std::vector<std::uint64_t> bad(K, kMergeNone);
  {
    std::vector<std::thread> th;
    const unsigned nt = total >= (1u << 14) ? host_threads() : 1u;
    std::atomic<std::uint32_t> next{0};
    auto work = [&] {
      for (std::uint32_t r = next++; r < K; r = next++) {
        bool prev_ok = false;
        for (std::uint64_t i = 0; i < c.n[r]; ++i) {
          const bool ok = span_ok(r, i);
          const std::uint64_t id = (static_cast<std::uint64_t>(r) << 32) | i;
          if (!ok || (prev_ok && cmp(id, id - 1) < 0)) {
            bad[r] = id;
            break;
          }
          prev_ok = ok;
        }
      }
    };
    for (unsigned t = 1; t < std::min<unsigned>(nt, K); ++t) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
  }
  *c.n_entries = *c.keys_bytes = *c.vals_bytes = 0;
  *c.first_bad = *std::min_element(bad.begin(), bad.end());
  if (*c.first_bad != kMergeNone) return set_error(TKV_CORRUPTED, "sst merge: a key span is out of bounds or a run is not ascending");
  // the lists of r << 32 | i, neighbouring lists merged pairwise on host threads, the older side first
  // on equal keys
  std::vector<std::uint64_t> cur(total), nxt(total);
  std::vector<std::uint64_t> cut{0};
  for (std::uint32_t r = 0; r < K; ++r) {
    if (c.n[r] == 0) continue;
    const std::uint64_t at = cut.back();
    for (std::uint64_t i = 0; i < c.n[r]; ++i) cur[at + i] = (static_cast<std::uint64_t>(r) << 32) | i;
    cut.push_back(at + c.n[r]);
  }
  auto less = [&](std::uint64_t x, std::uint64_t y) { return cmp(x, y) < 0; };
  while (cut.size() > 2) {
    std::vector<std::uint64_t> ncut{0};
    std::vector<std::thread> th;
    for (std::size_t p = 0; p + 1 < cut.size(); p += 2) {
      const std::uint64_t s0 = cut[p], s1 = cut[p + 1], s2 = p + 2 < cut.size() ? cut[p + 2] : s1;
      auto job = [&, s0, s1, s2] {
        std::merge(cur.begin() + s0, cur.begin() + s1, cur.begin() + s1, cur.begin() + s2, nxt.begin() + s0, less);
      };
      if (total >= (1u << 14)) th.emplace_back(job);
      else job();
      ncut.push_back(s2);
    }
    for (auto& t : th) t.join();
    cur.swap(nxt);
    cut.swap(ncut);
  }
  // the last of every group of equal keys, without the tombstones under the flag
  const bool drop = (c.flags & TKV_SST_MERGE_DROP_TOMBSTONES) != 0;
  std::vector<std::uint64_t> sv;
  std::uint64_t kb = 0, vb = 0;
  for (std::uint64_t j = 0; j < total; ++j) {
    if (j + 1 < total && cmp(cur[j], cur[j + 1]) == 0) continue;
    const std::uint32_t r = static_cast<std::uint32_t>(cur[j] >> 32);
    const std::uint64_t i = cur[j] & 0xFFFFFFFFull;
    const std::uint32_t kl = c.key_len[r][i];
    if (drop && c.keys[r][c.key_off[r][i] + kl - 1u] != 0) continue;
    sv.push_back(cur[j]);
    kb += kl;
    if (ptr_ok(c.val_len) && ptr_ok(c.val_len[r])) vb += c.val_len[r][i];
  }
  const std::uint64_t m = sv.size();
  *c.n_entries = m;
  *c.keys_bytes = kb;
  *c.vals_bytes = vb;
  const bool want_cols = ptr_ok(c.out_key_off) || ptr_ok(c.out_key_len) || ptr_ok(c.out_val_off) || ptr_ok(c.out_val_len) || ptr_ok(c.out_src);
  if (want_cols && m > c.entry_cap) return set_error(TKV_BUFFER_OVERFLOW, "sst merge: the entries do not fit");
  if (!want_cols) return TKV_OK;
  parallel_for(m, [&](std::uint64_t e) {
    const std::uint32_t r = static_cast<std::uint32_t>(sv[e] >> 32);
    const std::uint64_t i = sv[e] & 0xFFFFFFFFull;
    if (ptr_ok(c.out_key_off)) c.out_key_off[e] = static_cast<std::uint64_t>(c.keys[r] - c.key_base) + c.key_off[r][i];
    if (ptr_ok(c.out_key_len)) c.out_key_len[e] = c.key_len[r][i];
    const std::uint64_t bias = ptr_ok(c.val_bias) ? c.val_bias[r] : 0u;
    if (ptr_ok(c.out_val_off)) c.out_val_off[e] = bias + (ptr_ok(c.val_off) && ptr_ok(c.val_off[r]) ? c.val_off[r][i] : 0u);
    if (ptr_ok(c.out_val_len)) c.out_val_len[e] = ptr_ok(c.val_len) && ptr_ok(c.val_len[r]) ? c.val_len[r][i] : 0u;
    if (ptr_ok(c.out_src)) c.out_src[e] = sv[e];
  });
  return TKV_OK;
}
}  // namespace

extern "C" {

int tkv_sst_merge_device(uint32_t n_runs, const uint8_t* const* d_keys, const uint64_t* keys_size,
                         const uint64_t* const* d_key_off, const uint32_t* const* d_key_len,
                         const uint64_t* const* d_val_off, const uint32_t* const* d_val_len, const uint64_t* n,
                         const uint8_t* d_key_base, const uint64_t* val_bias, uint32_t flags, uint64_t* d_out_key_off,
                         uint32_t* d_out_key_len, uint64_t* d_out_val_off, uint32_t* d_out_val_len, uint64_t* d_out_src,
                         uint64_t entry_cap, uint64_t* n_entries, uint64_t* keys_bytes, uint64_t* vals_bytes,
                         uint64_t* first_bad, void* stream) {
  const SstMergeCall c{n_runs, d_keys, keys_size, d_key_off, d_key_len, d_val_off, d_val_len, n, d_key_base, val_bias, flags,
                       d_out_key_off, d_out_key_len, d_out_val_off, d_out_val_len, d_out_src, entry_cap,
                       n_entries, keys_bytes, vals_bytes, first_bad};
  std::uint64_t total = 0;
  if (int rc = sst_merge_check(c, &total)) return rc;
  if (total == 0) return sst_merge_empty(c);
  return sst_merge_device_impl(c, static_cast<hipStream_t>(stream));
}

int tkv_sst_merge(uint32_t n_runs, const uint8_t* const* h_keys, const uint64_t* keys_size,
                  const uint64_t* const* h_key_off, const uint32_t* const* h_key_len, const uint64_t* const* h_val_off,
                  const uint32_t* const* h_val_len, const uint64_t* n, const uint8_t* h_key_base, const uint64_t* val_bias,
                  uint32_t flags, uint64_t* h_out_key_off, uint32_t* h_out_key_len, uint64_t* h_out_val_off,
                  uint32_t* h_out_val_len, uint64_t* h_out_src, uint64_t entry_cap, uint64_t* n_entries,
                  uint64_t* keys_bytes, uint64_t* vals_bytes, uint64_t* first_bad) {
  const SstMergeCall c{n_runs, h_keys, keys_size, h_key_off, h_key_len, h_val_off, h_val_len, n, h_key_base, val_bias, flags,
                       h_out_key_off, h_out_key_len, h_out_val_off, h_out_val_len, h_out_src, entry_cap,
                       n_entries, keys_bytes, vals_bytes, first_bad};
  return sst_merge_host(c);
}

}  // extern "C"
