// ThreadSanitizer test of the host runtime's CPU-side threaded code (no GPU needed).
// tinykvpp_amd/csrc/Makefile target `tsan`: the host sources and this test are built with g++
// -fsanitize=thread (ROCm's clang ships no TSan runtime); the gfx950 kernel object is linked
// uninstrumented and never launched here.
//
// Exercised, each from several concurrent callers:
//  * the speculative parallel WAL record_len walk with exact stitching (tkv_debug_wal_chain; the
//    walk of tkv_wal_verify, /root/reference/src/engine/wal.cpp:63-87), on images whose pieces
//    start inside records, cross giant records, and end at a corrupted header;
//  * the multi-device split planner and its host combine step (tkv_debug_multi_plan,
//    tkv_debug_multi_combine; the plan tkv_crc32_batch_host_multi runs on one thread per device);
//  * the host WAL decode (tkv_wal_decode_host) on 40 000 records per caller: the header pass on host
//    threads with its compare-exchange minimum for first_bad (one caller's image has two bad records
//    in different threads' ranges), then the threaded scatter of the columns and the two arenas;
//  * the host WAL encode layout (tkv_debug_wal_encode_layout) of the same batches, records written
//    on host threads into one image;
//  * the host memtable replay (tkv_memtable_build) on 20 000 records per caller: the stable sort as
//    chunks on host threads and pairwise merges, one width behind the other;
//  * the host SSTable merge (tkv_sst_merge) on 4 runs of more than 2^14 entries in all per caller: the
//    per-run validation and the pairwise merge rounds on host threads.
// Results are checked against a sequential walk, a sequential decode and layout written here, the serial
// replay and insertion merge of runs_reference.h, and the test oracle (oracle/crc32_oracle.c, linked into
// this test only). Prints ALL PASSED.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "runs_reference.h"
#include "tkv_crc32.h"

extern "C" {
uint32_t oracle_update(uint32_t raw, const uint8_t* p, size_t n);
}

static int g_fail = 0;
#define CHECK(c)                                                                \
  do {                                                                          \
    if (!(c)) {                                                                 \
      std::fprintf(stderr, "%s:%d CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      __atomic_add_fetch(&g_fail, 1, __ATOMIC_RELAXED);                         \
    }                                                                           \
  } while (0)

namespace {

// One WAL record as wal_entry::encode lays it out (wal.cpp:19-61): u32 record_len | u32 crc |
// u8 op | u64 seq | u8 tombstone | u32 klen | u32 vlen | key | value, record_len = total - 8.
void put_record(std::vector<uint8_t>& w, uint64_t seq, uint32_t klen, uint32_t vlen, std::mt19937_64& rng) {
  const uint32_t rlen = 18 + klen + vlen;
  const size_t p = w.size();
  w.resize(p + 8 + rlen);
  uint8_t* r = w.data() + p;
  std::memcpy(r, &rlen, 4);
  r[8] = static_cast<uint8_t>(seq & 1);
  std::memcpy(r + 9, &seq, 8);
  r[17] = 0;
  std::memcpy(r + 18, &klen, 4);
  std::memcpy(r + 22, &vlen, 4);
  for (uint32_t i = 0; i < klen + vlen; ++i) r[26 + i] = static_cast<uint8_t>(rng());
  const uint32_t crc = oracle_update(0xFFFFFFFFu, r + 8, rlen) ^ 0xFFFFFFFFu;
  std::memcpy(r + 4, &crc, 4);
}

struct Walk {
  std::vector<uint64_t> pos;
  uint64_t end = 0;
  int err = 0;
};

// The reference's walk order (wal.cpp:63-87): a header that does not fit ends the chain.
Walk sequential(const std::vector<uint8_t>& w) {
  Walk s;
  uint64_t p = 0;
  const uint64_t size = w.size();
  while (p < size) {
    if (size - p < 26) {
      s.err = 1;
      break;
    }
    uint32_t rlen;
    std::memcpy(&rlen, w.data() + p, 4);
    if (uint64_t(rlen) + 8 > size - p) {
      s.err = 1;
      break;
    }
    s.pos.push_back(p);
    p += 8 + uint64_t(rlen);
  }
  s.end = p;
  return s;
}

Walk library(const std::vector<uint8_t>& w) {
  Walk g;
  uint64_t end = 0;
  int err = 0;
  const size_t n = tkv_debug_wal_chain(w.data(), w.size(), nullptr, 0, &end, &err);
  g.pos.resize(n);
  tkv_debug_wal_chain(w.data(), w.size(), g.pos.data(), n, &g.end, &g.err);
  return g;
}

std::vector<std::vector<uint8_t>> wal_images() {
  std::mt19937_64 rng(7);
  std::vector<std::vector<uint8_t>> imgs;
  // 1) ~40 MiB of small records: five 8 MiB pieces walked by five threads, stitched.
  {
    std::vector<uint8_t> w;
    uint64_t seq = 0;
    while (w.size() < (40u << 20)) put_record(w, seq++, rng() % 64, rng() % 512, rng);
    imgs.push_back(std::move(w));
  }
  // 2) giant records spanning whole pieces, with small ones between (speculative starts inside
  //    values must be discarded by the stitch).
  {
    std::vector<uint8_t> w;
    uint64_t seq = 0;
    while (w.size() < (48u << 20)) {
      if (seq % 50 == 7) put_record(w, seq++, 16, (9u << 20) + static_cast<uint32_t>(rng() % 4096), rng);
      else put_record(w, seq++, rng() % 32, rng() % 300, rng);
    }
    imgs.push_back(std::move(w));
  }
  // 3) image 1 with a record_len overrunning the image in the middle: the chain ends there.
  {
    std::vector<uint8_t> w = imgs[0];
    const Walk s = sequential(w);
    const uint64_t p = s.pos[s.pos.size() / 2];
    const uint32_t bad = 0xFFFFFF00u;
    std::memcpy(w.data() + p, &bad, 4);
    imgs.push_back(std::move(w));
  }
  // 4) image 2 truncated inside a record (torn tail).
  {
    std::vector<uint8_t> w = imgs[1];
    w.resize(w.size() - 11);
    imgs.push_back(std::move(w));
  }
  return imgs;
}

void check_wal_chains() {
  const auto imgs = wal_images();
  std::vector<Walk> want;
  for (const auto& w : imgs) want.push_back(sequential(w));
  std::vector<std::thread> th;
  for (int t = 0; t < 4; ++t)
    th.emplace_back([&, t] {
      for (int rep = 0; rep < 2; ++rep)
        for (size_t i = 0; i < imgs.size(); ++i) {
          const size_t k = (i + t) % imgs.size();
          const Walk g = library(imgs[k]);
          CHECK(g.pos == want[k].pos);
          CHECK(g.end == want[k].end);
          CHECK(g.err == want[k].err);
        }
    });
  for (auto& x : th) x.join();
}

void check_multi_plans() {
  std::mt19937_64 rng(11);
  std::vector<uint8_t> host(24u << 20);
  for (auto& b : host) b = static_cast<uint8_t>(rng());
  // small blocks with some >= 1 MiB blocks on share boundaries, per-block initial registers
  std::vector<uint64_t> off;
  std::vector<uint32_t> len, init;
  uint64_t p = 5;
  for (int i = 0; i < 400; ++i) {
    uint32_t l = static_cast<uint32_t>(rng() % 20000);
    if (i % 37 == 3) l = (1u << 20) + static_cast<uint32_t>(rng() % (2u << 20));
    if (p + l > host.size()) break;
    off.push_back(p);
    len.push_back(l);
    init.push_back(static_cast<uint32_t>(rng()));
    p += l;
  }
  const uint64_t n = off.size();
  std::vector<uint32_t> want(n);
  for (uint64_t b = 0; b < n; ++b) want[b] = oracle_update(init[b], host.data() + off[b], len[b]) ^ 0xFFFFFFFFu;
  std::vector<std::thread> th;
  for (int t = 0; t < 6; ++t)
    th.emplace_back([&, t] {
      for (int ndev = 1 + t % 3; ndev <= 8; ndev += 3) {
        const size_t k = tkv_debug_multi_plan(ndev, off.data(), len.data(), init.data(), n, nullptr, 0);
        std::vector<uint64_t> rec(6 * k);
        CHECK(tkv_debug_multi_plan(ndev, off.data(), len.data(), init.data(), n, rec.data(), k) == k);
        std::vector<uint32_t> piece(k), got(n);
        for (size_t j = 0; j < k; ++j) {
          const uint64_t* r = &rec[6 * j];
          piece[j] = oracle_update(static_cast<uint32_t>(r[4]), host.data() + r[2], r[3]) ^ 0xFFFFFFFFu;
        }
        CHECK(tkv_debug_multi_combine(TKV_CRC32_POLYNOMIAL, ndev, off.data(), len.data(), init.data(), n,
                                      piece.data(), got.data()) == TKV_OK);
        CHECK(got == want);
      }
    });
  for (auto& x : th) x.join();
}

// ---- tkv_wal_decode_host / tkv_debug_wal_encode_layout (40 000 records: past parallel_for's 16 384) ----
constexpr size_t kRecords = 40000;

struct Image {
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> off;
};

Image record_image(uint64_t seed) {
  std::mt19937_64 rng(seed);
  Image im;
  for (size_t i = 0; i < kRecords; ++i) {
    im.off.push_back(im.bytes.size());
    put_record(im.bytes, rng() >> 2, static_cast<uint32_t>(rng() % 24), static_cast<uint32_t>(rng() % 65), rng);
  }
  return im;
}

struct Columns {
  std::vector<uint8_t> op, tomb, keys, vals;
  std::vector<uint64_t> seq, key_off, val_off;
  std::vector<uint32_t> key_len, val_len;
  uint64_t first_bad = 0;
  bool operator==(const Columns& o) const {
    return op == o.op && tomb == o.tomb && keys == o.keys && vals == o.vals && seq == o.seq && key_off == o.key_off &&
           val_off == o.val_off && key_len == o.key_len && val_len == o.val_len && first_bad == o.first_bad;
  }
};

// wal_entry::decode's structural checks and fields (wal.cpp:68, :83, :98-125), record after record. A bad
// record: first_bad is its index and every column stays empty.
Columns sequential_decode(const Image& im) {
  Columns c;
  const uint64_t size = im.bytes.size();
  const uint8_t* w = im.bytes.data();
  c.first_bad = im.off.size();
  for (size_t i = 0; i < im.off.size(); ++i) {
    const uint64_t p = im.off[i];
    uint32_t rlen = 0, kl = 0, vl = 0;
    bool ok = p < size && size - p >= 26;
    if (ok) {
      std::memcpy(&rlen, w + p, 4);
      std::memcpy(&kl, w + p + 18, 4);
      std::memcpy(&vl, w + p + 22, 4);
      ok = uint64_t(rlen) + 8 <= size - p && 18 + uint64_t(kl) + vl <= rlen;
    }
    if (!ok) {
      Columns bad;
      bad.first_bad = i;
      return bad;
    }
    uint64_t seq;
    std::memcpy(&seq, w + p + 9, 8);
    c.op.push_back(w[p + 8]);
    c.tomb.push_back(w[p + 17]);
    c.seq.push_back(seq);
    c.key_off.push_back(c.keys.size());
    c.val_off.push_back(c.vals.size());
    c.key_len.push_back(kl);
    c.val_len.push_back(vl);
    c.keys.insert(c.keys.end(), w + p + 26, w + p + 26 + kl);
    c.vals.insert(c.vals.end(), w + p + 26 + kl, w + p + 26 + kl + vl);
  }
  return c;
}

// The library's decode into 0xA5-filled outputs; on TKV_CORRUPTED every output must still be 0xA5 and is
// returned empty, as sequential_decode returns it.
Columns library_decode(const Image& im, uint64_t keys_cap, uint64_t vals_cap) {
  const size_t n = im.off.size();
  Columns c;
  c.op.assign(n, 0xA5);
  c.tomb.assign(n, 0xA5);
  c.seq.assign(n, 0xA5A5A5A5A5A5A5A5ull);
  c.key_off.assign(n, 0xA5A5A5A5A5A5A5A5ull);
  c.val_off.assign(n, 0xA5A5A5A5A5A5A5A5ull);
  c.key_len.assign(n, 0xA5A5A5A5u);
  c.val_len.assign(n, 0xA5A5A5A5u);
  c.keys.assign(keys_cap, 0xA5);
  c.vals.assign(vals_cap, 0xA5);
  const Columns filled = c;
  uint64_t ks = 7, vs = 7;
  const int rc = tkv_wal_decode_host(im.bytes.data(), im.bytes.size(), im.off.data(), n, 0, c.op.data(), c.tomb.data(),
                                     c.seq.data(), c.key_off.data(), c.key_len.data(), c.val_off.data(), c.val_len.data(),
                                     c.keys.data(), keys_cap, c.vals.data(), vals_cap, &ks, &vs, &c.first_bad);
  if (rc == TKV_CORRUPTED) {
    const uint64_t bad = c.first_bad;
    c.first_bad = 0;
    CHECK(c == filled);  // nothing written
    CHECK(ks == 0 && vs == 0);
    Columns none;
    none.first_bad = bad;
    return none;
  }
  CHECK(rc == TKV_OK);
  CHECK(ks <= keys_cap && vs <= vals_cap);
  if (ks <= keys_cap) c.keys.resize(ks);
  if (vs <= vals_cap) c.vals.resize(vs);
  return c;
}

std::vector<Image> decode_images() {
  std::vector<Image> ims;
  for (int t = 0; t < 4; ++t) ims.push_back(record_image(100 + t));
  return ims;
}

void check_wal_decode_host() {
  std::vector<Image> ims = decode_images();
  // caller 1: two bad records in different threads' ranges (whatever the thread count: 30 000 lies past
  // the middle, 12 000 in front of it); the smaller index is the answer
  Image& bad = ims[1];
  const uint32_t overrun = 0xFFFFFF00u, huge_key = 0xFFFFFFFFu;
  std::memcpy(bad.bytes.data() + bad.off[30000], &overrun, 4);
  std::memcpy(bad.bytes.data() + bad.off[12000] + 18, &huge_key, 4);
  std::vector<Columns> want;
  for (const auto& im : ims) want.push_back(sequential_decode(im));
  CHECK(want[1].first_bad == 12000 && want[1].op.empty());
  CHECK(want[0].first_bad == kRecords && want[0].op.size() == kRecords);
  std::vector<std::thread> th;
  for (int t = 0; t < 4; ++t)
    th.emplace_back([&, t] {
      for (int rep = 0; rep < 3; ++rep) {
        const Columns got = library_decode(ims[t], 24 * kRecords, 65 * kRecords);
        CHECK(got == want[t]);
      }
    });
  for (auto& x : th) x.join();
}

void check_wal_encode_layout() {
  const std::vector<Image> ims = decode_images();
  std::vector<Columns> cols;
  std::vector<std::vector<uint8_t>> want;  // the image with every CRC field zero (wal.cpp:28)
  for (const auto& im : ims) {
    cols.push_back(sequential_decode(im));
    want.push_back(im.bytes);
    for (const uint64_t p : im.off) std::memset(want.back().data() + p + 4, 0, 4);
  }
  std::vector<std::thread> th;
  for (int t = 0; t < 4; ++t)
    th.emplace_back([&, t] {
      const Columns& c = cols[t];
      for (int rep = 0; rep < 3; ++rep) {
        std::vector<uint8_t> img(want[t].size() + 64, 0xA5);
        uint64_t size = 0;
        const size_t laid = tkv_debug_wal_encode_layout(c.keys.data(), c.key_off.data(), c.key_len.data(), c.vals.data(),
                                                        c.val_off.data(), c.val_len.data(), c.op.data(), c.tomb.data(),
                                                        c.seq.data(), 0, kRecords, img.data(), want[t].size(), &size);
        CHECK(laid == kRecords && size == want[t].size());
        CHECK(std::memcmp(img.data(), want[t].data(), want[t].size()) == 0);
        for (size_t i = want[t].size(); i < img.size(); ++i) CHECK(img[i] == 0xA5);
      }
    });
  for (auto& x : th) x.join();
}

// ---- tkv_memtable_build (20 000 records: the sort's chunks and pairwise merges on host threads) ------
void check_memtable_build() {
  std::vector<mt_ref::Case> cases;
  std::vector<std::vector<uint32_t>> want;  // the surviving records in key order
  for (int t = 0; t < 4; ++t) {
    cases.push_back(mt_ref::make_case(1002 + t, 20000, 20000));  // (1005: keys as overlapping views)
    want.push_back(mt_ref::replay(cases.back()));
  }
  std::vector<std::thread> th;
  for (int t = 0; t < 4; ++t)
    th.emplace_back([&, t] {
      const mt_ref::Case& c = cases[t];
      const uint64_t n = c.klen.size();
      for (int rep = 0; rep < 2; ++rep) {
        std::vector<uint32_t> src(n, 0xA5A5A5A5u);
        std::vector<uint64_t> ikey_off(n);
        uint64_t m = 0, size = 0, bad = 0;
        const int rc = tkv_memtable_build(c.keys.data(), c.keys.size(), c.koff.data(), c.klen.data(), c.voff.data(),
                                          c.vlen.data(), c.op.data(), c.tomb.data(), c.seq.data(), n, c.ts, nullptr, 0,
                                          ikey_off.data(), nullptr, nullptr, nullptr, src.data(), n, &m, &size, &bad);
        CHECK(rc == TKV_OK && bad == n && m == want[t].size());
        src.resize(m);
        CHECK(src == want[t]);
        uint64_t at = 0;
        for (uint64_t j = 0; j < m && j < want[t].size(); ++j) {
          CHECK(ikey_off[j] == at);
          at += c.klen[want[t][j]] + 17;
        }
        CHECK(size == at);
      }
    });
  for (auto& x : th) x.join();
}

// ---- tkv_sst_merge (4 runs, past 2^14 entries: the validation and the pairwise rounds on host threads) ----
void check_sst_merge() {
  std::vector<mg_ref::Case> cases;
  std::vector<std::vector<uint64_t>> want;  // the surviving entries (run << 32 | index) in key order
  // test_sst_merge_host.cpp's case above the threshold and three more of 18 000 to 21 000 entries, two of
  // them with the drop-tombstones flag
  for (const uint64_t seed : {1002, 1012, 1027, 1029}) {
    cases.push_back(mg_ref::make_case(seed, 9000, 4));
    want.push_back(mg_ref::insertion_merge(cases.back()));
  }
  std::vector<std::thread> th;
  for (int t = 0; t < 4; ++t)
    th.emplace_back([&, t] {
      const mg_ref::Case& c = cases[t];
      const mg_ref::Placed p(c);
      uint64_t total = 0;
      for (const uint64_t n : p.n) total += n;
      CHECK(total >= (1u << 14));  // else the merge stays on the calling thread
      for (int rep = 0; rep < 2; ++rep) {
        std::vector<uint64_t> src(total, 0xA5A5A5A5A5A5A5A5ull);
        uint64_t m = 0, kb = 0, vb = 0, bad = 0;
        const int rc = tkv_sst_merge(4, p.pk.data(), p.size.data(), p.pko.data(), p.pkl.data(), p.pvo.data(), p.pvl.data(),
                                     p.n.data(), p.base, p.bias.data(), c.flags, nullptr, nullptr, nullptr, nullptr,
                                     src.data(), total, &m, &kb, &vb, &bad);
        CHECK(rc == TKV_OK && bad == TKV_SST_MERGE_NONE && m == want[t].size());
        src.resize(m);
        CHECK(src == want[t]);
      }
    });
  for (auto& x : th) x.join();
}

}  // namespace

int main() {
  check_wal_chains();
  check_multi_plans();
  check_wal_decode_host();
  check_wal_encode_layout();
  check_memtable_build();
  check_sst_merge();
  if (g_fail) {
    std::printf("%d FAILED\n", g_fail);
    return 1;
  }
  std::printf("ALL PASSED\n");
  return 0;
}
