// Stand-alone check of the host memtable replay (tkv_memtable_build), built with AddressSanitizer and
// UndefinedBehaviorSanitizer on the host code (Makefile target `sanitize-memtable`; device code
// uninstrumented, nothing launched, no GPU needed). The fuzz shapes of tests/memtable_util.py restated
// here (n <= 5000 and two cases above the host-thread threshold, key lengths 0-40 over a small alphabet,
// keys as overlapping views into one blob in every fifth case) against a byte-at-a-time insertion sort
// with replacement, every input and output in a heap block of exactly its size so that any overrun is
// the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "runs_reference.h"
#include "tkv_crc32.h"

using namespace mt_ref;  // the cases, compare and the insertion sort with replacement (replay)

namespace {

int failures = 0;
#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      std::printf("FAIL %s: ", #cond);       \
      std::printf(__VA_ARGS__);              \
      std::printf("\n");                     \
      ++failures;                            \
    }                                        \
  } while (0)

void run_case(std::uint64_t seed, std::uint32_t n_min, std::uint32_t n_max) {
  const Case c = make_case(seed, n_min, n_max);
  const std::uint64_t n = c.klen.size();
  const std::vector<std::uint32_t> list = replay(c);
  std::vector<std::uint8_t> want;
  for (std::uint32_t r : list) {
    for (std::uint32_t b = 0; b < c.klen[r]; ++b) want.push_back(c.keys[c.koff[r] + b]);
    for (int b = 0; b < 8; ++b) want.push_back(static_cast<std::uint8_t>(c.seq[r] >> (8 * b)));
    for (int b = 0; b < 8; ++b) want.push_back(static_cast<std::uint8_t>(c.ts >> (8 * b)));
    want.push_back(c.tomb[r] != 0 ? 1 : 0);
  }
  auto keys = exact(c.keys);
  auto koff = exact(c.koff);
  auto klen = exact(c.klen);
  auto voff = exact(c.voff);
  auto vlen = exact(c.vlen);
  auto op = exact(c.op);
  auto tomb = exact(c.tomb);
  auto seq = exact(c.seq);
  std::uint64_t m = 0, size = 0, bad = 0;
  auto call = [&](std::uint8_t* ik, std::uint64_t cap, std::uint64_t* io, std::uint32_t* il, std::uint64_t* ovo,
                  std::uint32_t* ovl, std::uint32_t* src, std::uint64_t ecap) {
    return tkv_memtable_build(keys.get(), c.keys.size(), koff.get(), klen.get(), voff.get(), vlen.get(), op.get(), tomb.get(),
                              seq.get(), n, c.ts, ik, cap, io, il, ovo, ovl, src, ecap, &m, &size, &bad);
  };
  int rc = call(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
  CHECK(rc == TKV_OK && m == list.size() && size == want.size() && bad == n, "seed %llu sizing rc %d m %llu size %llu",
        (unsigned long long)seed, rc, (unsigned long long)m, (unsigned long long)size);
  if (m != list.size() || size != want.size()) return;
  std::unique_ptr<std::uint8_t[]> ik(new std::uint8_t[size]);
  std::unique_ptr<std::uint64_t[]> io(new std::uint64_t[m]), ovo(new std::uint64_t[m]);
  std::unique_ptr<std::uint32_t[]> il(new std::uint32_t[m]), ovl(new std::uint32_t[m]), src(new std::uint32_t[m]);
  // one short: overflow, nothing written (the blocks are exactly one short too)
  if (m > 1) {
    std::unique_ptr<std::uint32_t[]> s1(new std::uint32_t[m - 1]);
    rc = call(nullptr, 0, nullptr, nullptr, nullptr, nullptr, s1.get(), m - 1);
    CHECK(rc == TKV_BUFFER_OVERFLOW && m == list.size(), "seed %llu entry overflow rc %d", (unsigned long long)seed, rc);
  }
  {
    std::unique_ptr<std::uint8_t[]> k1(new std::uint8_t[size - 1]);
    rc = call(k1.get(), size - 1, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
    CHECK(rc == TKV_BUFFER_OVERFLOW && size == want.size(), "seed %llu arena overflow rc %d", (unsigned long long)seed, rc);
  }
  rc = call(ik.get(), size, io.get(), il.get(), ovo.get(), ovl.get(), src.get(), m);
  CHECK(rc == TKV_OK, "seed %llu rc %d: %s", (unsigned long long)seed, rc, tkv_last_error());
  if (rc != TKV_OK) return;
  CHECK(std::memcmp(ik.get(), want.data(), size) == 0, "seed %llu: internal keys differ", (unsigned long long)seed);
  std::uint64_t at = 0;
  for (std::uint64_t j = 0; j < m; ++j) {
    const std::uint32_t r = list[j];
    const std::uint32_t vl = c.op[r] == 1 ? 0u : c.vlen[r];
    CHECK(src[j] == r && io[j] == at && il[j] == c.klen[r] + 17 && ovo[j] == c.voff[r] && ovl[j] == vl,
          "seed %llu entry %llu", (unsigned long long)seed, (unsigned long long)j);
    at += c.klen[r] + 17;
  }
}

void run_errors() {
  const std::uint8_t keys[4] = {'a', 'b', 'c', 'd'};
  const std::uint64_t koff[3] = {0, 1, 2};
  std::uint32_t klen[3] = {1, 1, 2};
  std::uint8_t op[3] = {0, 7, 9};
  std::uint64_t m = 9, size = 9, bad = 9;
  int rc = tkv_memtable_build(keys, 4, koff, klen, nullptr, nullptr, op, nullptr, nullptr, 3, 0, nullptr, 0, nullptr, nullptr,
                              nullptr, nullptr, nullptr, 0, &m, &size, &bad);
  CHECK(rc == TKV_CORRUPTED && bad == 1 && m == 0 && size == 0, "bad op rc %d bad %llu", rc, (unsigned long long)bad);
  klen[2] = 3;  // one past keys_size
  rc = tkv_memtable_build(keys, 4, koff, klen, nullptr, nullptr, nullptr, nullptr, nullptr, 3, 0, nullptr, 0, nullptr, nullptr,
                          nullptr, nullptr, nullptr, 0, &m, &size, &bad);
  CHECK(rc == TKV_INVALID_ARGUMENT, "bounds rc %d", rc);
  rc = tkv_memtable_build(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, nullptr,
                          nullptr, nullptr, nullptr, nullptr, 0, &m, &size, &bad);
  CHECK(rc == TKV_OK && m == 0 && size == 0 && bad == 0, "n == 0 rc %d", rc);
}

}  // namespace

int main() {
  for (std::uint64_t seed = 0; seed < 64; ++seed) run_case(seed, 1, seed % 4 ? 5000 : 80);
  run_case(1001, 1, 1);          // a single record
  run_case(1002, 20000, 30000);  // above the host-thread threshold of the sort (2^14 records)
  run_case(1005, 20000, 30000);  // the same with keys as views
  run_errors();
  if (failures) {
    std::printf("%d FAILED\n", failures);
    return 1;
  }
  std::printf("ALL PASSED\n");
  return 0;
}
