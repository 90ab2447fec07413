// Stand-alone check of the host parse and copies of the SSTable scan (tkv_debug_sst_scan_parse), built
// with AddressSanitizer and UndefinedBehaviorSanitizer on the host code (Makefile target
// `sanitize-sst-scan`; device code uninstrumented, nothing launched, no GPU needed). Files come from
// tkv_debug_sst_build_layout (the fuzz shapes of tests/sst_build_util.py restated as in
// test_sst_build_host.cpp) and are scanned out of a heap block of exactly file_size bytes, so that a read
// behind the file is the sanitizer's to report; so are their mutations: every byte of the footer and the
// index, and a stride of data bytes, set to values that break lengths, counts and offsets. The verdict,
// the entries and the block arrays are compared with a byte-at-a-time reader that checks every index
// against the file's size itself. The bounds arithmetic under test (tkv_sst_layout.h) is the code the
// device kernels run.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "tkv_crc32.h"

namespace {

struct Rng {
  std::uint64_t s;
  std::uint64_t next() {
    std::uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  std::uint32_t below(std::uint32_t n) { return static_cast<std::uint32_t>(next() % n); }
};

std::uint32_t pick_len(Rng& r, int heavy) {
  const std::uint32_t p = r.below(1000);
  const std::uint32_t cut[3][4] = {{200, 900, 980, 992}, {500, 800, 950, 980}, {50, 950, 990, 996}};
  const std::uint32_t* c = cut[heavy];
  if (p < c[0]) return 0;
  if (p < c[1]) return 1 + r.below(59);
  if (p < c[2]) return 127 + r.below(3);
  if (p < c[3]) return 16383 + r.below(3);
  return r.below(70001);
}

// A built file (CRC fields zero) in a heap block of exactly its size.
struct File {
  std::unique_ptr<std::uint8_t[]> p;
  std::uint64_t size = 0;
};

File build(std::uint32_t seed, std::uint32_t nmax) {
  static const std::uint32_t targets[5] = {1, 64, 100, 4096, 65536};
  Rng r{0x5CA70ull + seed};
  const std::uint32_t target = targets[seed % 5];
  const std::uint32_t n = 1 + r.below(nmax);
  std::vector<std::uint8_t> keys(70001), vals(70001);
  for (auto& b : keys) b = static_cast<std::uint8_t>(r.next());
  for (auto& b : vals) b = static_cast<std::uint8_t>(r.next());
  std::vector<std::uint64_t> koff, voff;
  std::vector<std::uint32_t> klen, vlen;
  for (std::uint32_t i = 0; i < n; ++i) {
    const std::uint32_t kl = pick_len(r, seed % 3), vl = pick_len(r, seed % 3);
    klen.push_back(kl);
    vlen.push_back(vl);
    koff.push_back(r.below(70001 - kl + 1));
    voff.push_back(r.below(70001 - vl + 1));
  }
  std::uint64_t fs = 0, nb = 0, io = 0, is = 0;
  (void)tkv_debug_sst_build_layout(keys.data(), koff.data(), klen.data(), vals.data(), voff.data(), vlen.data(), n, target,
                                   nullptr, 0, nullptr, nullptr, nullptr, 0, &fs, &nb, &io, &is);
  File f;
  f.size = fs;
  f.p.reset(new std::uint8_t[fs]);
  const int rc = tkv_debug_sst_build_layout(keys.data(), koff.data(), klen.data(), vals.data(), voff.data(), vlen.data(), n,
                                            target, f.p.get(), fs, nullptr, nullptr, nullptr, 0, &fs, &nb, &io, &is);
  if (rc != TKV_OK) f.size = 0;
  return f;
}

// ---- the reference reader: one byte at a time, every index checked against n -------------------------
struct Ref {
  bool ok = false;
  std::uint64_t bad = 0;
  std::vector<std::uint8_t> keys, vals;
  std::vector<std::uint32_t> klen, vlen, bsize, bfirst;
  std::vector<std::uint64_t> kpos, vpos, boff;
};

struct Bytes {
  const std::uint8_t* p;
  std::uint64_t n;
  bool oob = false;
  std::uint8_t at(std::uint64_t i) {
    if (i >= n) {
      oob = true;
      return 0;
    }
    return p[i];
  }
  std::uint64_t le(std::uint64_t i, int bytes) {
    std::uint64_t v = 0;
    for (int b = 0; b < bytes; ++b) v |= static_cast<std::uint64_t>(at(i + b)) << (8 * b);
    return v;
  }
};

// The varint at pos that ends within maxb bytes and before end; false otherwise.
bool ref_varint(Bytes& f, std::uint64_t pos, std::uint64_t end, int maxb, std::uint64_t* v, std::uint64_t* next) {
  *v = 0;
  for (int k = 0; k < maxb; ++k) {
    if (pos + k >= end) return false;
    const std::uint8_t b = f.at(pos + k);
    *v |= static_cast<std::uint64_t>(b & 0x7F) << (7 * k);
    if (b < 0x80) {
      *next = pos + k + 1;
      return true;
    }
  }
  return false;
}

Ref reference(const std::uint8_t* p, std::uint64_t n) {
  Ref r;
  Bytes f{p, n};
  r.bad = TKV_SST_BAD_FOOTER;
  if (n < 28 || n > 0xFFFFFFFFull) return r;
  const std::uint64_t ioff = f.le(n - 20, 4), isz = f.le(n - 16, 4);
  if (ioff + isz + 20 != n || isz < 8) return r;
  r.bad = TKV_SST_BAD_INDEX;
  const std::uint64_t B = f.le(ioff, 8), iend = ioff + isz;
  if (B > (isz - 8) / 17) return r;
  std::uint64_t pos = ioff + 8;
  struct Ent {
    std::uint64_t key, kl, off, size;
  };
  std::vector<Ent> idx;
  for (std::uint64_t j = 0; j < B; ++j) {
    std::uint64_t kl, next;
    if (!ref_varint(f, pos, iend, 4, &kl, &next) || next + kl + 16 > iend) return r;
    const std::uint64_t off = f.le(next + kl, 8), size = f.le(next + kl + 8, 8);
    if (size < 22 || off > ioff || size > ioff - off) return r;
    idx.push_back(Ent{next, kl, off, size});
    pos = next + kl + 16;
  }
  if (pos != iend) return r;
  for (std::uint64_t j = 0; j < B; ++j) {
    r.bad = j;
    const Ent& e = idx[j];
    const std::uint64_t c = f.le(e.off + 1, 4), z = f.le(e.off + 5, 4), end = e.off + e.size;
    if (f.at(e.off) != 0x14 || f.le(e.off + 9, 4) != z || f.at(e.off + 13) != 0 || 36 + z != e.size || c < 1 || 8 * c > z) return r;
    std::uint64_t zv, body;
    if (!ref_varint(f, e.off + 21, end, 5, &zv, &body) || zv != z) return r;
    const std::uint64_t bend = body + z;
    std::uint64_t q = body, sum = 0;
    const std::size_t first = r.klen.size();
    for (std::uint64_t i = 0; i < c; ++i) {
      std::uint64_t kl, vl, kp, vp;
      if (!ref_varint(f, q, bend, 4, &kl, &kp) || kp + kl > bend) return r;
      if (!ref_varint(f, kp + kl, bend, 4, &vl, &vp) || vp + vl > bend) return r;
      r.kpos.push_back(kp);
      r.vpos.push_back(vp);
      r.klen.push_back(static_cast<std::uint32_t>(kl));
      r.vlen.push_back(static_cast<std::uint32_t>(vl));
      sum += 8 + kl + vl;
      q = vp + vl;
    }
    if (sum != z || r.klen[first] != e.kl) return r;
    for (std::uint64_t b = 0; b < e.kl; ++b)
      if (f.at(e.key + b) != f.at(r.kpos[first] + b)) return r;
    r.boff.push_back(e.off);
    r.bsize.push_back(static_cast<std::uint32_t>(e.size));
    r.bfirst.push_back(static_cast<std::uint32_t>(first));
  }
  for (std::size_t i = 0; i < r.klen.size(); ++i) {
    for (std::uint32_t b = 0; b < r.klen[i]; ++b) r.keys.push_back(f.at(r.kpos[i] + b));
    for (std::uint32_t b = 0; b < r.vlen[i]; ++b) r.vals.push_back(f.at(r.vpos[i] + b));
  }
  r.bad = B;
  r.ok = !f.oob;
  if (f.oob) std::printf("the reference reader itself left the file\n");
  return r;
}

int fails = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      if (fails < 40) std::printf("FAIL %s:%d %s: %s\n", __FILE__, __LINE__, what, #cond); \
      ++fails;                                                                       \
    }                                                                                \
  } while (0)

// The scan of [p, p + n) (a heap block of exactly n bytes) against the reference.
void check(const std::uint8_t* p, std::uint64_t n, const char* what, bool full) {
  const Ref r = reference(p, n);
  std::uint64_t ne = 7, nb = 7, ks = 7, vs = 7, bad = 7;
  int rc = tkv_debug_sst_scan_parse(p, n, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, nullptr,
                                    nullptr, 0, &ne, &nb, &ks, &vs, &bad);
  if (!r.ok) {
    CHECK(rc == TKV_CORRUPTED);
    CHECK(bad == r.bad && ne == 0 && nb == 0 && ks == 0 && vs == 0);
    return;
  }
  CHECK(rc == TKV_OK || rc == TKV_BUFFER_OVERFLOW);
  CHECK(ne == r.klen.size() && nb == r.boff.size() && ks == r.keys.size() && vs == r.vals.size() && bad == nb);
  if (!full || fails) return;
  // exactly sized outputs: an overrun is the sanitizer's to report
  std::vector<std::uint64_t> koff(ne), voff(ne), boff(nb);
  std::vector<std::uint32_t> klen(ne), vlen(ne), bsize(nb), bfirst(nb);
  std::unique_ptr<std::uint8_t[]> keys(new std::uint8_t[ks]), vals(new std::uint8_t[vs]);
  rc = tkv_debug_sst_scan_parse(p, n, 0, koff.data(), klen.data(), voff.data(), vlen.data(), ne, keys.get(), ks, vals.get(), vs,
                                boff.data(), bsize.data(), bfirst.data(), nb, &ne, &nb, &ks, &vs, &bad);
  CHECK(rc == TKV_OK);
  CHECK(klen == r.klen && vlen == r.vlen && boff == r.boff && bsize == r.bsize && bfirst == r.bfirst);
  CHECK(ks == 0 || std::memcmp(keys.get(), r.keys.data(), ks) == 0);
  CHECK(vs == 0 || std::memcmp(vals.get(), r.vals.data(), vs) == 0);
  std::uint64_t ko = 0, vo = 0;
  for (std::uint64_t i = 0; i < ne; ++i) {
    CHECK(koff[i] == ko && voff[i] == vo);
    ko += klen[i];
    vo += vlen[i];
  }
  // views: the offsets point into the file
  rc = tkv_debug_sst_scan_parse(p, n, TKV_SST_SCAN_KEY_VIEWS | TKV_SST_SCAN_VAL_VIEWS, koff.data(), nullptr, voff.data(), nullptr,
                                ne, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, &ne, &nb, &ks, &vs, &bad);
  CHECK(rc == TKV_OK);
  CHECK(koff == r.kpos && voff == r.vpos);
}

// Mutations of one file, each scanned out of its own exactly sized heap block.
void mutate(const File& f, std::uint32_t seed) {
  const char* what = "mutation";
  Rng r{0xBADull + seed};
  const std::uint64_t n = f.size;
  const std::uint64_t ioff = f.p[n - 20] | (f.p[n - 19] << 8) | (f.p[n - 18] << 16) | (static_cast<std::uint64_t>(f.p[n - 17]) << 24);
  static const std::uint8_t vals[] = {0x00, 0x01, 0x7F, 0x80, 0xFF, 0x14};
  auto one = [&](std::uint64_t pos, std::uint8_t v) {
    if (f.p[pos] == v) return;
    std::unique_ptr<std::uint8_t[]> m(new std::uint8_t[n]);
    std::memcpy(m.get(), f.p.get(), n);
    m[pos] = v;
    check(m.get(), n, what, false);
  };
  // every byte of the index and the footer, and the first 40 bytes of the file (a block header and its
  // first entry), to every value; then random data bytes
  for (std::uint64_t pos = ioff; pos < n; ++pos)
    for (std::uint8_t v : vals) one(pos, v);
  for (std::uint64_t pos = 0; pos < 40 && pos < ioff; ++pos)
    for (std::uint8_t v : vals) one(pos, v);
  for (int k = 0; k < 300 && ioff; ++k) one(r.below(static_cast<std::uint32_t>(ioff)), vals[r.below(6)] ^ static_cast<std::uint8_t>(r.below(2) ? r.next() : 0));
  // truncations: the file's last bytes cut off
  for (std::uint64_t cut = 1; cut <= 30 && cut < n; ++cut) {
    std::unique_ptr<std::uint8_t[]> m(new std::uint8_t[n - cut]);
    std::memcpy(m.get(), f.p.get(), n - cut);
    check(m.get(), n - cut, "truncation", false);
  }
}

}  // namespace

int main() {
  const char* what = "built file";
  int scanned = 0;
  for (std::uint32_t seed = 0; seed < 48; ++seed) {
    const File f = build(seed, seed % 4 ? 3000 : 69);
    CHECK(f.size != 0);
    if (!f.size) continue;
    check(f.p.get(), f.size, what, true);
    ++scanned;
  }
  // small files take every mutation
  for (std::uint32_t seed = 100; seed < 112; ++seed) {
    const File f = build(seed, 12);
    CHECK(f.size != 0);
    if (!f.size) continue;
    check(f.p.get(), f.size, what, true);
    mutate(f, seed);
  }
  // files shorter than a footer, out of exactly sized blocks
  for (std::uint64_t n = 1; n < 28; ++n) {
    std::unique_ptr<std::uint8_t[]> m(new std::uint8_t[n]);
    std::memset(m.get(), 0x14, n);
    check(m.get(), n, "short file", false);
  }
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("ALL PASSED (%d built files)\n", scanned);
  return 0;
}
