// The SSTable file format around the CRC engine (format defined in include/tkv_crc32.h; SURVEY.md §8f
// rank 2): data-block and footer stamps, the flush of an entry list into blocks, index and footer, and
// the scan that reads such a file back. The host cuts, places and parses; every checksum over block or
// index bytes runs on the GPU through the engine (tkv_engine.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "tkv_crc32.h"
#include "tkv_device_util.h"
#include "tkv_engine.h"
#include "tkv_host_util.h"
#include "tkv_sst_layout.h"

using namespace tkv;

namespace {
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

int sst_check(const std::uint64_t* h_sizes, std::uint64_t n) {
  for (std::uint64_t i = 0; i < n; ++i)
    if (h_sizes[i] < TKV_SST_MIN_IMAGE || h_sizes[i] > 0xFFFFFFFFull)
      return set_error(TKV_INVALID_ARGUMENT, "SSTable block image shorter than 22 bytes or 4 GiB and longer");
  return TKV_OK;
}

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

// ---- SSTable flush (sstable_writer::append ... get_footer for a whole entry list) ---------------------

// The cut and the layout of a host entry list.
struct SstPlan {
  std::vector<std::uint64_t> pos;     // file offset of every entry
  std::vector<std::uint32_t> first;   // b_j, B + 1 entries
  std::vector<std::uint64_t> off;     // O_j
  std::vector<std::uint32_t> size;    // 36 + z_j
  std::uint64_t index_offset = 0, index_size = 0, file_size = 0;
};

// The argument checks both entry points share.
int sst_build_check(const SstBuildCall& c) {
  if (c.n == 0) return set_error(TKV_INVALID_ARGUMENT, "SSTable build: no entries");
  if (c.n > 0xFFFFFFFFull) return set_error(TKV_INVALID_ARGUMENT, "SSTable build: more than 2^32 - 1 entries");
  if (c.target_block_size == 0) return set_error(TKV_INVALID_ARGUMENT, "SSTable build: target_block_size is 0");
  if (!ptr_ok(c.keys) || !ptr_ok(c.key_off) || !ptr_ok(c.key_len) ||
      (ptr_ok(c.val_len) && (!ptr_ok(c.vals) || !ptr_ok(c.val_off))) || !ptr_ok(c.file_size) || !ptr_ok(c.n_blocks) ||
      !ptr_ok(c.index_offset) || !ptr_ok(c.index_size) || (c.cap && !ptr_ok(c.file)))
    return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  return TKV_OK;
}

// Sizes, the greedy cut (append, then is_data_block_complete: size >= target) and every offset; no
// source byte is read.
int sst_build_plan(const SstBuildCall& c, SstPlan& p) {
  for (std::uint64_t i = 0; i < c.n; ++i)
    if (c.key_len[i] >= kSstMaxLen || (c.val_len && c.val_len[i] >= kSstMaxLen))
      return set_error(TKV_INVALID_ARGUMENT, "SSTable build: a key or value length is 2^28 or more");
  p.pos.resize(c.n);
  std::uint64_t file = 0, b = 0;
  while (b < c.n) {
    std::uint64_t z = 0, m = b;
    while (m < c.n && z < c.target_block_size) {
      z += sst_counted(c.key_len[m], c.val_len ? c.val_len[m] : 0u);
      ++m;
    }
    if (kSstOverhead + z > 0xFFFFFFFFull) return set_error(TKV_INVALID_ARGUMENT, "SSTable build: a data block does not fit u32");
    std::uint64_t at = file + kSstHeader + sst_vlen(z);
    for (std::uint64_t i = b; i < m; ++i) {
      p.pos[i] = at;
      at += sst_written(c.key_len[i], c.val_len ? c.val_len[i] : 0u);
    }
    p.first.push_back(static_cast<std::uint32_t>(b));
    p.off.push_back(file);
    p.size.push_back(static_cast<std::uint32_t>(kSstOverhead + z));
    file += kSstOverhead + z;
    b = m;
  }
  p.first.push_back(static_cast<std::uint32_t>(c.n));
  p.index_offset = file;
  p.index_size = 8;
  for (std::size_t j = 0; j + 1 < p.first.size(); ++j) {
    const std::uint32_t kl = c.key_len[p.first[j]];
    p.index_size += std::uint64_t(sst_vlen(kl)) + kl + kSstIndexFixed;
  }
  p.file_size = p.index_offset + p.index_size + kSstFooter;
  if (p.file_size > 0xFFFFFFFFull) return set_error(TKV_INVALID_ARGUMENT, "SSTable build: the file does not fit u32");
  return TKV_OK;
}

// The file image with every CRC field zero, entries on host threads.
void sst_build_layout(const SstBuildCall& c, const SstPlan& p) {
  std::uint8_t* f = c.file;
  const std::uint64_t B = p.off.size();
  std::memset(f, 0, p.index_offset);  // slack and padding
  parallel_for(B, [&](std::uint64_t j) {
    std::uint8_t h[32];
    const std::uint32_t nh = sst_block_head(h, p.first[j + 1] - p.first[j], p.size[j] - kSstOverhead);
    std::memcpy(f + p.off[j], h, nh);
  });
  parallel_for(c.n, [&](std::uint64_t i) {
    std::uint8_t* d = f + p.pos[i];
    const std::uint32_t kl = c.key_len[i], vl = c.val_len ? c.val_len[i] : 0u;
    d += sst_put_varint(d, kl);
    if (kl) std::memcpy(d, c.keys + c.key_off[i], kl);
    d += kl;
    d += sst_put_varint(d, vl);
    if (vl) std::memcpy(d, c.vals + c.val_off[i], vl);
  });
  std::uint8_t* d = f + p.index_offset;
  for (int b = 0; b < 8; ++b) *d++ = static_cast<std::uint8_t>(B >> (8 * b));
  for (std::uint64_t j = 0; j < B; ++j) {
    const std::uint64_t i = p.first[j];
    const std::uint32_t kl = c.key_len[i];
    d += sst_put_varint(d, kl);
    if (kl) std::memcpy(d, c.keys + c.key_off[i], kl);
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
int sst_build_host_layout(const SstBuildCall& c, SstPlan& p) {
  if (int rc = sst_build_check(c)) return rc;
  if (int rc = sst_build_plan(c, p)) return rc;
  const std::uint64_t B = p.off.size();
  *c.file_size = p.file_size;
  *c.n_blocks = B;
  *c.index_offset = p.index_offset;
  *c.index_size = p.index_size;
  const bool want_blocks = ptr_ok(c.block_off) || ptr_ok(c.block_size) || ptr_ok(c.block_first);
  if (p.file_size > c.cap || (want_blocks && B > c.block_cap))
    return set_error(TKV_BUFFER_OVERFLOW, "SSTable build: the file or the block arrays do not fit");
  if (!ptr_ok(c.file)) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  sst_build_layout(c, p);
  if (ptr_ok(c.block_off)) std::memcpy(c.block_off, p.off.data(), B * sizeof(std::uint64_t));
  if (ptr_ok(c.block_size)) std::memcpy(c.block_size, p.size.data(), B * sizeof(std::uint32_t));
  if (ptr_ok(c.block_first)) std::memcpy(c.block_first, p.first.data(), B * sizeof(std::uint32_t));
  return TKV_OK;
}

// ---- SSTable scan (the reader of what tkv_sst_build writes; include/tkv_crc32.h "SSTable scan") --------

// The argument checks both entry points share: decided before any device work.
int sst_scan_check(const SstScanCall& c) {
  if ((c.file_size && !ptr_ok(c.file)) || !ptr_ok(c.n_entries) || !ptr_ok(c.n_blocks) || !ptr_ok(c.keys_size) ||
      !ptr_ok(c.vals_size) || !ptr_ok(c.bad_block))
    return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  if (c.flags & ~(TKV_SST_SCAN_KEY_VIEWS | TKV_SST_SCAN_VAL_VIEWS)) return set_error(TKV_INVALID_ARGUMENT, "SSTable scan: unknown flag");
  if (c.file_size > 0xFFFFFFFFull) return set_error(TKV_INVALID_ARGUMENT, "SSTable scan: the file does not fit u32");
  return TKV_OK;
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

// The scan of a host image; crc = false skips every checksum comparison (tkv_debug_sst_scan_parse).
int sst_scan_host(const SstScanCall& o, bool crc) {
  if (int rc = sst_scan_check(o)) return rc;
  const std::uint8_t* f = o.file;
  const std::uint64_t fsize = o.file_size;
  // footer
  if (fsize < kSstMinFile) return sst_scan_corrupted(o, TKV_SST_BAD_FOOTER, "SSTable scan: the file is shorter than an index and a footer");
  const std::uint8_t* foot = f + (fsize - kSstFooter);
  const std::uint32_t ioff32 = static_cast<std::uint32_t>(le_bytes(foot, 4)), isz32 = static_cast<std::uint32_t>(le_bytes(foot + 4, 4));
  if (!sst_footer_ok(fsize, ioff32, isz32))
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
  const bool kviews = o.flags & TKV_SST_SCAN_KEY_VIEWS, vviews = o.flags & TKV_SST_SCAN_VAL_VIEWS;
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
  const unsigned nt = threads_for(n);
  std::vector<std::uint64_t> bad(nt, 0), first(nt, n);
  pow_tables();
  parallel_tasks(nt, nt > 1, [&](std::uint64_t t) {
    for (std::uint64_t i = n * t / nt; i < n * (t + 1) / nt; ++i) {
      std::uint32_t stored;
      std::memcpy(&stored, h_file + h_offsets[i] + TKV_SST_CRC_OFFSET, 4);
      const std::uint32_t want = got[i] ^ field_term(stored, h_sizes[i] - TKV_SST_CRC_OFFSET - 4);
      if (want != stored) {
        if (bad[t] == 0) first[t] = i;
        ++bad[t];
      }
    }
  });
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

int tkv_sst_build_device(const uint8_t* d_keys, const uint64_t* d_key_off, const uint32_t* d_key_len, const uint8_t* d_vals,
                         const uint64_t* d_val_off, const uint32_t* d_val_len, uint64_t n, uint32_t target_block_size,
                         uint8_t* d_file, uint64_t cap, uint64_t* d_block_off, uint32_t* d_block_size,
                         uint32_t* d_block_first, uint64_t block_cap, uint64_t* file_size, uint64_t* n_blocks,
                         uint64_t* index_offset, uint64_t* index_size, void* stream) {
  const SstBuildCall c{d_keys, d_key_off, d_key_len, d_vals, d_val_off, d_val_len, n, target_block_size, d_file, cap,
                       d_block_off, d_block_size, d_block_first, block_cap, file_size, n_blocks, index_offset, index_size};
  if (int rc = sst_build_check(c)) return rc;
  return sst_build_device_impl(c, static_cast<hipStream_t>(stream));
}

int tkv_sst_build(const uint8_t* h_keys, const uint64_t* h_key_off, const uint32_t* h_key_len, const uint8_t* h_vals,
                  const uint64_t* h_val_off, const uint32_t* h_val_len, uint64_t n, uint32_t target_block_size,
                  uint8_t* h_file, uint64_t cap, uint64_t* h_block_off, uint32_t* h_block_size, uint32_t* h_block_first,
                  uint64_t block_cap, uint64_t* file_size, uint64_t* n_blocks, uint64_t* index_offset,
                  uint64_t* index_size) {
  const SstBuildCall c{h_keys, h_key_off, h_key_len, h_vals, h_val_off, h_val_len, n, target_block_size, h_file, cap,
                       h_block_off, h_block_size, h_block_first, block_cap, file_size, n_blocks, index_offset, index_size};
  SstPlan p;
  if (int rc = sst_build_host_layout(c, p)) return rc;
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
  const SstBuildCall c{h_keys, h_key_off, h_key_len, h_vals, h_val_off, h_val_len, n, target_block_size, h_file, cap,
                       h_block_off, h_block_size, h_block_first, block_cap, file_size, n_blocks, index_offset, index_size};
  SstPlan p;
  return sst_build_host_layout(c, p);
}

int tkv_sst_scan_device(const uint8_t* d_file, uint64_t file_size, uint32_t flags, uint64_t* d_key_off, uint32_t* d_key_len,
                        uint64_t* d_val_off, uint32_t* d_val_len, uint64_t entry_cap, uint8_t* d_keys, uint64_t keys_cap,
                        uint8_t* d_vals, uint64_t vals_cap, uint64_t* d_block_off, uint32_t* d_block_size,
                        uint32_t* d_block_first, uint64_t block_cap, uint64_t* n_entries, uint64_t* n_blocks,
                        uint64_t* keys_size, uint64_t* vals_size, uint64_t* bad_block, void* stream) {
  const SstScanCall c{d_file, file_size, flags, d_key_off, d_key_len, d_val_off, d_val_len, entry_cap, d_keys, keys_cap, d_vals,
                      vals_cap, d_block_off, d_block_size, d_block_first, block_cap, n_entries, n_blocks, keys_size, vals_size,
                      bad_block};
  if (int rc = sst_scan_check(c)) return rc;
  if (file_size < kSstMinFile) return sst_scan_corrupted(c, TKV_SST_BAD_FOOTER, "SSTable scan: the file is shorter than an index and a footer");
  return sst_scan_device_impl(c, static_cast<hipStream_t>(stream));
}

int tkv_sst_scan(const uint8_t* h_file, uint64_t file_size, uint32_t flags, uint64_t* h_key_off, uint32_t* h_key_len,
                 uint64_t* h_val_off, uint32_t* h_val_len, uint64_t entry_cap, uint8_t* h_keys, uint64_t keys_cap,
                 uint8_t* h_vals, uint64_t vals_cap, uint64_t* h_block_off, uint32_t* h_block_size, uint32_t* h_block_first,
                 uint64_t block_cap, uint64_t* n_entries, uint64_t* n_blocks, uint64_t* keys_size, uint64_t* vals_size,
                 uint64_t* bad_block) {
  const SstScanCall c{h_file, file_size, flags, h_key_off, h_key_len, h_val_off, h_val_len, entry_cap, h_keys, keys_cap, h_vals,
                      vals_cap, h_block_off, h_block_size, h_block_first, block_cap, n_entries, n_blocks, keys_size, vals_size,
                      bad_block};
  return sst_scan_host(c, true);
}

int tkv_debug_sst_scan_parse(const uint8_t* h_file, uint64_t file_size, uint32_t flags, uint64_t* h_key_off,
                             uint32_t* h_key_len, uint64_t* h_val_off, uint32_t* h_val_len, uint64_t entry_cap,
                             uint8_t* h_keys, uint64_t keys_cap, uint8_t* h_vals, uint64_t vals_cap, uint64_t* h_block_off,
                             uint32_t* h_block_size, uint32_t* h_block_first, uint64_t block_cap, uint64_t* n_entries,
                             uint64_t* n_blocks, uint64_t* keys_size, uint64_t* vals_size, uint64_t* bad_block) {
  const SstScanCall c{h_file, file_size, flags, h_key_off, h_key_len, h_val_off, h_val_len, entry_cap, h_keys, keys_cap, h_vals,
                      vals_cap, h_block_off, h_block_size, h_block_first, block_cap, n_entries, n_blocks, keys_size, vals_size,
                      bad_block};
  return sst_scan_host(c, false);
}

}  // extern "C"
