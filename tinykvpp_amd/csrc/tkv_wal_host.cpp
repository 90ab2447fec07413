// The WAL record format around the CRC engine (the reference's call sites,
// /root/reference/src/engine/wal.cpp:19-130): the record_len chain walk, verify, index, the salvage
// driver, the batch stamp, the group-commit encode and the batched decode. The host walks lengths and
// places fields; every checksum over record bytes runs on the GPU through the engine (tkv_engine.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "tkv_crc32.h"
#include "tkv_device_util.h"
#include "tkv_engine.h"
#include "tkv_host_util.h"
#include "tkv_wal_device.h"
#include "tkv_wal_layout.h"

using namespace tkv;

namespace {
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
  std::vector<std::thread> th;  // one walker per piece, all at once: the pieces are the speculation
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

// The host-walk verify (exact for every image): the record_len chain walked on host threads, the
// CRCs checked on the GPU through the host batch API.
// good_pos, when given, receives the starts of the good records (Chain::pos of the good prefix).
int wal_verify_host_walk(const uint8_t* h_wal, uint64_t size, uint64_t* n_good, uint64_t* stop_offset,
                         std::vector<std::uint64_t>* good_pos = nullptr) {
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

// ---- WAL group-commit encode (wal.cpp:19-61 for a batch) ---------------------------------------------

// The argument checks both entry points share (n >= 1).
int encode_check(const WalEncodeCall& c) {
  if (c.n > 0xFFFFFFFFull) return set_error(TKV_INVALID_ARGUMENT, "WAL encode: more than 2^32 - 1 records");
  if (!ptr_ok(c.keys) || !ptr_ok(c.key_off) || !ptr_ok(c.key_len) || !ptr_ok(c.img_size) ||
      (ptr_ok(c.val_len) && (!ptr_ok(c.vals) || !ptr_ok(c.val_off))))
    return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  return TKV_OK;
}

// Record start offsets (n + 1 entries, the last one the total) of a host batch; TKV_INVALID_ARGUMENT when
// a record_len does not fit u32 (no source byte is read).
int encode_offsets(const WalEncodeCall& c, std::vector<std::uint64_t>& off) {
  off.resize(c.n + 1);
  std::uint64_t run = 0;
  for (std::uint64_t i = 0; i < c.n; ++i) {
    const std::uint64_t rl = 18ull + c.key_len[i] + (c.val_len ? c.val_len[i] : 0u);
    if (rl > 0xFFFFFFFFull) return set_error(TKV_INVALID_ARGUMENT, "WAL encode: 18 + key_len + val_len does not fit u32");
    off[i] = run;
    run += rl + kWalPayload;
  }
  off[c.n] = run;
  return TKV_OK;
}

// Records laid out at c.img + off[i] with their CRC fields zero (wal.cpp:27-52), on host threads.
void encode_layout(const WalEncodeCall& c, const std::vector<std::uint64_t>& off) {
  parallel_for(c.n, [&](std::uint64_t i) {
    std::uint8_t* r = c.img + off[i];
    const std::uint32_t kl = c.key_len[i], vl = c.val_len ? c.val_len[i] : 0u;
    const std::uint32_t rl = 18u + kl + vl, zero = 0;
    const std::uint64_t seq = c.seq ? c.seq[i] : c.first_seq + i;
    std::memcpy(r, &rl, 4);
    std::memcpy(r + kWalCrc, &zero, 4);
    r[kWalOp] = c.op ? c.op[i] : 0;
    for (int b = 0; b < 8; ++b) r[kWalSeq + b] = static_cast<std::uint8_t>(seq >> (8 * b));
    r[kWalTomb] = c.tomb && c.tomb[i] ? 1 : 0;
    for (int b = 0; b < 4; ++b) r[kWalKeyLen + b] = static_cast<std::uint8_t>(kl >> (8 * b));
    for (int b = 0; b < 4; ++b) r[kWalValLen + b] = static_cast<std::uint8_t>(vl >> (8 * b));
    if (kl) std::memcpy(r + kWalMeta, c.keys + c.key_off[i], kl);
    if (vl) std::memcpy(r + kWalMeta + kl, c.vals + c.val_off[i], vl);
  });
}

// Checks, sizes and the layout of a host batch; *laid is set when the records were written.
int encode_host_layout(const WalEncodeCall& c, std::vector<std::uint64_t>& off, bool* laid) {
  *laid = false;
  if (c.n == 0) {
    if (ptr_ok(c.img_size)) *c.img_size = 0;
    return TKV_OK;
  }
  if (int rc = encode_check(c)) return rc;
  if (int rc = encode_offsets(c, off)) return rc;
  *c.img_size = off[c.n];
  if (off[c.n] > c.cap) return set_error(TKV_BUFFER_OVERFLOW, "WAL encode: the image does not fit cap");
  if (!ptr_ok(c.img)) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  encode_layout(c, off);
  *laid = true;
  return TKV_OK;
}

// ---- WAL batched decode (wal.cpp:98-127 for a record list) -------------------------------------------

// The argument checks both entry points share, and the results' presets; *done is set when the call is
// finished (n == 0).
int decode_check(const WalDecodeCall& c, bool* done) {
  *done = false;
  if (!ptr_ok(c.keys_size) || !ptr_ok(c.vals_size) || !ptr_ok(c.first_bad)) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  if (c.flags & ~(TKV_WAL_DECODE_KEY_VIEWS | TKV_WAL_DECODE_VAL_VIEWS))
    return set_error(TKV_INVALID_ARGUMENT, "WAL decode: unknown flag bits");
  if (c.n > 0xFFFFFFFFull) return set_error(TKV_INVALID_ARGUMENT, "WAL decode: more than 2^32 - 1 records");
  if (c.n == 0) {
    *c.keys_size = *c.vals_size = *c.first_bad = 0;
    *done = true;
    return TKV_OK;
  }
  if (ptr_ok(c.rec_off64) == ptr_ok(c.rec_off32)) return set_error(TKV_INVALID_ARGUMENT, "WAL decode: exactly one offset array");
  if (ptr_ok(c.rec_off32) && c.size > 0xFFFFFFFFull + 1ull)
    return set_error(TKV_INVALID_ARGUMENT, "image larger than 4 GiB (u32 offsets)");
  if (!ptr_ok(c.img)) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  *c.keys_size = *c.vals_size = 0;
  *c.first_bad = c.n;
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

int decode_host(const WalDecodeCall& c) {
  bool done = false;
  if (int rc = decode_check(c, &done)) return rc;
  if (done) return TKV_OK;
  const std::uint64_t n = c.n;
  const bool kviews = c.flags & TKV_WAL_DECODE_KEY_VIEWS, vviews = c.flags & TKV_WAL_DECODE_VAL_VIEWS;
  // the header pass: lengths of the records that pass, the smallest failing index per thread's range
  std::vector<std::uint64_t> ko(n + 1), vo(n + 1);
  std::atomic<std::uint64_t> bad{n};
  parallel_for(n, [&](std::uint64_t i) {
    std::uint32_t kl = 0, vl = 0;
    if (!decode_header(c.img, c.size, c.rec_off64[i], &kl, &vl)) {
      kl = vl = 0;  // (never used as copy lengths)
      std::uint64_t cur = bad.load(std::memory_order_relaxed);
      while (i < cur && !bad.compare_exchange_weak(cur, i, std::memory_order_relaxed)) {
      }
    }
    ko[i + 1] = kl;
    vo[i + 1] = vl;
  });
  if (bad.load() < n) {
    *c.first_bad = bad.load();
    return set_error(TKV_CORRUPTED, "WAL decode: a record fails wal_entry::decode's structural checks");
  }
  ko[0] = vo[0] = 0;
  for (std::uint64_t i = 0; i < n; ++i) {  // lengths to exclusive prefix sums, the totals last
    ko[i + 1] += ko[i];
    vo[i + 1] += vo[i];
  }
  *c.keys_size = ko[n];
  *c.vals_size = vo[n];
  const bool kcopy = !kviews && ko[n] != 0, vcopy = !vviews && vo[n] != 0;
  if ((kcopy && ko[n] > c.keys_cap) || (vcopy && vo[n] > c.vals_cap))
    return set_error(TKV_BUFFER_OVERFLOW, "WAL decode: an arena does not fit its cap");
  if ((kcopy && !ptr_ok(c.keys)) || (vcopy && !ptr_ok(c.vals))) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  parallel_for(n, [&](std::uint64_t i) {
    const std::uint64_t off = c.rec_off64[i];
    const std::uint8_t* r = c.img + off;
    const std::uint32_t kl = static_cast<std::uint32_t>(ko[i + 1] - ko[i]), vl = static_cast<std::uint32_t>(vo[i + 1] - vo[i]);
    if (ptr_ok(c.op)) c.op[i] = r[kWalOp];
    if (ptr_ok(c.tomb)) c.tomb[i] = r[kWalTomb];
    if (ptr_ok(c.seq)) std::memcpy(&c.seq[i], r + kWalSeq, 8);
    if (ptr_ok(c.key_len)) c.key_len[i] = kl;
    if (ptr_ok(c.val_len)) c.val_len[i] = vl;
    if (ptr_ok(c.key_off)) c.key_off[i] = kviews ? off + kWalMeta : ko[i];
    if (ptr_ok(c.val_off)) c.val_off[i] = vviews ? off + kWalMeta + kl : vo[i];
    if (kcopy && kl) std::memcpy(c.keys + ko[i], r + kWalMeta, kl);
    if (vcopy && vl) std::memcpy(c.vals + vo[i], r + kWalMeta + kl, vl);
  });
  return TKV_OK;
}
}  // namespace

extern "C" {

int tkv_wal_verify(const uint8_t* h_wal, uint64_t size, uint64_t* n_good, uint64_t* stop_offset) {
  if ((size && !ptr_ok(h_wal)) || !ptr_ok(n_good) || !ptr_ok(stop_offset))
    return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  // The image goes to the device once; the chain walk, the CRC batch and the first-corruption
  // search run there (tkv_wal_device.hip). The host walk is the exact fallback for images the
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

int tkv_wal_encode_device(const uint8_t* d_keys, const uint64_t* d_key_off, const uint32_t* d_key_len,
                          const uint8_t* d_vals, const uint64_t* d_val_off, const uint32_t* d_val_len, const uint8_t* d_op,
                          const uint8_t* d_tomb, const uint64_t* d_seq, uint64_t first_seq, uint64_t n, uint8_t* d_img,
                          uint64_t cap, uint64_t* d_rec_off, uint32_t* d_crc, uint64_t* img_size, void* stream) {
  const WalEncodeCall c{d_keys, d_key_off, d_key_len, d_vals, d_val_off, d_val_len, d_op, d_tomb, d_seq, first_seq,
                        n, d_img, cap, d_rec_off, d_crc, img_size};
  if (n == 0) {
    if (ptr_ok(img_size)) *img_size = 0;
    return TKV_OK;
  }
  if (int rc = encode_check(c)) return rc;
  if (cap && !ptr_ok(d_img)) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  return wal_encode_device_impl(c, static_cast<hipStream_t>(stream));
}

int tkv_wal_encode(const uint8_t* h_keys, const uint64_t* h_key_off, const uint32_t* h_key_len, const uint8_t* h_vals,
                   const uint64_t* h_val_off, const uint32_t* h_val_len, const uint8_t* h_op, const uint8_t* h_tomb,
                   const uint64_t* h_seq, uint64_t first_seq, uint64_t n, uint8_t* h_img, uint64_t cap,
                   uint64_t* h_rec_off, uint32_t* h_crc, uint64_t* img_size) {
  const WalEncodeCall c{h_keys, h_key_off, h_key_len, h_vals, h_val_off, h_val_len, h_op, h_tomb, h_seq, first_seq,
                        n, h_img, cap, h_rec_off, h_crc, img_size};
  std::vector<std::uint64_t> off;
  bool laid = false;
  if (int rc = encode_host_layout(c, off, &laid)) return rc;
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
  const WalEncodeCall c{h_keys, h_key_off, h_key_len, h_vals, h_val_off, h_val_len, h_op, h_tomb, h_seq, first_seq,
                        n, h_img, cap, nullptr, nullptr, img_size};
  std::vector<std::uint64_t> off;
  bool laid = false;
  if (encode_host_layout(c, off, &laid) != TKV_OK || !laid) return 0;
  return static_cast<size_t>(n);
}

int tkv_wal_decode_device(const uint8_t* d_img, uint64_t size, const uint64_t* d_rec_off64, const uint32_t* d_rec_off32,
                          uint64_t n, uint32_t flags, uint8_t* d_op, uint8_t* d_tomb, uint64_t* d_seq, uint64_t* d_key_off,
                          uint32_t* d_key_len, uint64_t* d_val_off, uint32_t* d_val_len, uint8_t* d_keys, uint64_t keys_cap,
                          uint8_t* d_vals, uint64_t vals_cap, uint64_t* keys_size, uint64_t* vals_size, uint64_t* first_bad,
                          void* stream) {
  const WalDecodeCall c{d_img, size, d_rec_off64, d_rec_off32, n, flags, d_op, d_tomb, d_seq, d_key_off, d_key_len,
                        d_val_off, d_val_len, d_keys, keys_cap, d_vals, vals_cap, keys_size, vals_size, first_bad};
  bool done = false;
  if (int rc = decode_check(c, &done)) return rc;
  if (done) return TKV_OK;
  return wal_decode_device_impl(c, static_cast<hipStream_t>(stream));
}

int tkv_wal_decode_host(const uint8_t* h_img, uint64_t size, const uint64_t* h_rec_off64, uint64_t n, uint32_t flags,
                        uint8_t* h_op, uint8_t* h_tomb, uint64_t* h_seq, uint64_t* h_key_off, uint32_t* h_key_len,
                        uint64_t* h_val_off, uint32_t* h_val_len, uint8_t* h_keys, uint64_t keys_cap, uint8_t* h_vals,
                        uint64_t vals_cap, uint64_t* keys_size, uint64_t* vals_size, uint64_t* first_bad) {
  const WalDecodeCall c{h_img, size, h_rec_off64, nullptr, n, flags, h_op, h_tomb, h_seq, h_key_off, h_key_len,
                        h_val_off, h_val_len, h_keys, keys_cap, h_vals, vals_cap, keys_size, vals_size, first_bad};
  return decode_host(c);
}

size_t tkv_debug_wal_chain(const uint8_t* h_wal, uint64_t size, uint64_t* out_pos, size_t cap, uint64_t* end,
                           int* err) {
  const Chain c = wal_chain(h_wal, size, 0, size);
  if (out_pos) std::memcpy(out_pos, c.pos.data(), std::min(cap, c.pos.size()) * sizeof(std::uint64_t));
  if (end) *end = c.end;
  if (err) *err = c.err ? 1 : 0;
  return c.pos.size();
}

}  // extern "C"
