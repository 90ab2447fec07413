// Stand-alone check of the host cut and layout of the SSTable flush (tkv_debug_sst_build_layout), built
// with AddressSanitizer and UndefinedBehaviorSanitizer on the host code (Makefile target
// `sanitize-sst`; device code uninstrumented, nothing launched, no GPU needed). The fuzz shapes of
// tests/sst_build_util.py restated here (n <= 3000, T from {1, 64, 100, 4096, 65536}, lengths mixed from
// 0 / 1-59 / 127-129 / 16383-16385 / up to 70 000 bytes) against a byte-at-a-time writer loop, with the
// destination and the block arrays sized exactly so that any overrun is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstring>
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
  // the mixes: empty, 1-59, 127-129, 16383-16385, up to 70 000 (the long ones rare)
  const std::uint32_t cut[3][4] = {{200, 900, 980, 992}, {500, 800, 950, 980}, {50, 950, 990, 996}};
  const std::uint32_t* c = cut[heavy];
  if (p < c[0]) return 0;
  if (p < c[1]) return 1 + r.below(59);
  if (p < c[2]) return 127 + r.below(3);
  if (p < c[3]) return 16383 + r.below(3);
  return r.below(70001);
}

void put_varint(std::vector<std::uint8_t>& out, std::uint64_t v) {
  while (v >= 0x80) {
    out.push_back(static_cast<std::uint8_t>(v | 0x80));
    v >>= 7;
  }
  out.push_back(static_cast<std::uint8_t>(v));
}
void put_le(std::vector<std::uint8_t>& out, std::uint64_t v, int bytes) {
  for (int b = 0; b < bytes; ++b) out.push_back(static_cast<std::uint8_t>(v >> (8 * b)));
}

struct Case {
  std::vector<std::uint8_t> keys, vals;
  std::vector<std::uint64_t> koff, voff;
  std::vector<std::uint32_t> klen, vlen;
  std::uint32_t target;
};

// The writer loop, one byte at a time: append / is_data_block_complete / get_data_block /
// record_data_block / get_index / the footer, every CRC field zero.
struct Expect {
  std::vector<std::uint8_t> file;
  std::vector<std::uint64_t> off;
  std::vector<std::uint32_t> size, first;
  std::uint64_t index_offset = 0, index_size = 0;
};
Expect writer_loop(const Case& c) {
  Expect e;
  std::vector<std::uint8_t> body, index;
  std::vector<std::uint64_t> first_of;
  std::uint64_t counted = 0;
  std::uint32_t count = 0, first = 0;
  const std::size_t n = c.klen.size();
  auto flush = [&](std::uint32_t next_first) {
    const std::uint64_t at = e.file.size();
    e.file.push_back(20);
    put_le(e.file, count, 4);
    put_le(e.file, counted, 4);
    put_le(e.file, counted, 4);
    put_le(e.file, 0, 4);  // compression and padding
    put_le(e.file, 0, 4);  // crc32_
    put_varint(e.file, counted);
    for (std::uint8_t b : body) e.file.push_back(b);
    while (e.file.size() < at + 36 + counted) e.file.push_back(0);
    e.off.push_back(at);
    e.size.push_back(static_cast<std::uint32_t>(36 + counted));
    e.first.push_back(first);
    body.clear();
    counted = 0;
    count = 0;
    first = next_first;
  };
  for (std::size_t i = 0; i < n; ++i) {
    put_varint(body, c.klen[i]);
    for (std::uint32_t b = 0; b < c.klen[i]; ++b) body.push_back(c.keys[c.koff[i] + b]);
    put_varint(body, c.vlen[i]);
    for (std::uint32_t b = 0; b < c.vlen[i]; ++b) body.push_back(c.vals[c.voff[i] + b]);
    counted += 8ull + c.klen[i] + c.vlen[i];
    ++count;
    if (counted >= c.target) flush(static_cast<std::uint32_t>(i + 1));
  }
  if (count) flush(static_cast<std::uint32_t>(n));
  e.index_offset = e.file.size();
  put_le(index, e.off.size(), 8);
  for (std::size_t j = 0; j < e.off.size(); ++j) {
    const std::uint32_t i = e.first[j];
    put_varint(index, c.klen[i]);
    for (std::uint32_t b = 0; b < c.klen[i]; ++b) index.push_back(c.keys[c.koff[i] + b]);
    put_le(index, e.off[j], 8);
    put_le(index, e.size[j], 8);
  }
  e.index_size = index.size();
  for (std::uint8_t b : index) e.file.push_back(b);
  put_le(e.file, e.index_offset, 4);
  put_le(e.file, e.index_size, 4);
  for (int k = 0; k < 3; ++k) put_le(e.file, 0, 4);  // bloom fields, crc32_
  return e;
}

Case make_case(std::uint32_t seed) {
  static const std::uint32_t targets[5] = {1, 64, 100, 4096, 65536};
  Rng r{0x55B0ull + seed};
  Case c;
  c.target = targets[seed % 5];
  const std::uint32_t n = seed % 4 ? 1 + r.below(3000) : 1 + r.below(69);
  // sources lie in one 70 001-byte blob each, at random offsets: they overlap each other and leave gaps
  c.keys.resize(70001);
  c.vals.resize(70001);
  for (auto& b : c.keys) b = static_cast<std::uint8_t>(r.next());
  for (auto& b : c.vals) b = static_cast<std::uint8_t>(r.next());
  for (std::uint32_t i = 0; i < n; ++i) {
    const std::uint32_t kl = pick_len(r, seed % 3), vl = pick_len(r, seed % 3);
    c.klen.push_back(kl);
    c.vlen.push_back(vl);
    c.koff.push_back(r.below(70001 - kl + 1));
    c.voff.push_back(r.below(70001 - vl + 1));
  }
  return c;
}

int fails = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAIL %s:%d seed %u: %s\n", __FILE__, __LINE__, seed, #cond); \
      ++fails;                                                             \
    }                                                                      \
  } while (0)

void run(std::uint32_t seed, bool no_values) {
  Case c = make_case(seed);
  if (no_values) std::fill(c.vlen.begin(), c.vlen.end(), 0u);
  const Expect e = writer_loop(c);
  const std::uint64_t n = c.klen.size(), B = e.off.size();
  std::uint64_t fs = 0, nb = 0, io = 0, is = 0;
  // the sizing call
  int rc = tkv_debug_sst_build_layout(c.keys.data(), c.koff.data(), c.klen.data(), c.vals.data(), c.voff.data(),
                                      no_values ? nullptr : c.vlen.data(), n, c.target, nullptr, 0, nullptr, nullptr, nullptr,
                                      0, &fs, &nb, &io, &is);
  CHECK(rc == TKV_BUFFER_OVERFLOW);
  CHECK(fs == e.file.size() && nb == B && io == e.index_offset && is == e.index_size);
  // exactly sized outputs, at a misaligned start inside an exactly sized heap block
  const std::uint32_t mis = seed % 16;
  std::vector<std::uint8_t> file(mis + e.file.size());
  std::vector<std::uint64_t> boff(B);
  std::vector<std::uint32_t> bsize(B), bfirst(B);
  rc = tkv_debug_sst_build_layout(c.keys.data(), c.koff.data(), c.klen.data(), c.vals.data(), c.voff.data(),
                                  no_values ? nullptr : c.vlen.data(), n, c.target, file.data() + mis, e.file.size(),
                                  boff.data(), bsize.data(), bfirst.data(), B, &fs, &nb, &io, &is);
  CHECK(rc == TKV_OK);
  CHECK(std::memcmp(file.data() + mis, e.file.data(), e.file.size()) == 0);
  CHECK(boff == e.off && bsize == e.size && bfirst == e.first);
  // one byte and one block short
  rc = tkv_debug_sst_build_layout(c.keys.data(), c.koff.data(), c.klen.data(), c.vals.data(), c.voff.data(),
                                  no_values ? nullptr : c.vlen.data(), n, c.target, file.data() + mis, e.file.size() - 1,
                                  boff.data(), bsize.data(), bfirst.data(), B, &fs, &nb, &io, &is);
  CHECK(rc == TKV_BUFFER_OVERFLOW);
  if (B > 1) {
    std::vector<std::uint64_t> small(B - 1, 7);
    rc = tkv_debug_sst_build_layout(c.keys.data(), c.koff.data(), c.klen.data(), c.vals.data(), c.voff.data(),
                                    no_values ? nullptr : c.vlen.data(), n, c.target, file.data() + mis, e.file.size(),
                                    small.data(), nullptr, nullptr, B - 1, &fs, &nb, &io, &is);
    CHECK(rc == TKV_BUFFER_OVERFLOW);
    for (std::uint64_t v : small) CHECK(v == 7);
  }
}

}  // namespace

int main() {
  for (std::uint32_t seed = 0; seed < 64; ++seed) run(seed, seed % 8 == 5);
  // lengths of 2^28 and more over a one-byte arena: invalid, and no source byte is read
  {
    const std::uint32_t seed = 1000;
    const std::uint8_t tiny[1] = {0};
    const std::uint64_t off[2] = {0, 0};
    const std::uint32_t kl[2] = {3, 1u << 28}, vl[2] = {0xFFFFFFFFu, 0};
    std::uint64_t s[4] = {9, 9, 9, 9};
    std::uint8_t out[8] = {0};
    CHECK(tkv_debug_sst_build_layout(tiny, off, kl, tiny, off, nullptr, 2, 4096, out, 8, nullptr, nullptr, nullptr, 0, &s[0], &s[1],
                                     &s[2], &s[3]) == TKV_INVALID_ARGUMENT);
    CHECK(tkv_debug_sst_build_layout(tiny, off, kl, tiny, off, vl, 1, 4096, out, 8, nullptr, nullptr, nullptr, 0, &s[0], &s[1],
                                     &s[2], &s[3]) == TKV_INVALID_ARGUMENT);
    CHECK(s[0] == 9 && s[1] == 9 && s[2] == 9 && s[3] == 9);
  }
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("ALL PASSED\n");
  return 0;
}
