// Stand-alone check of the host SSTable merge (tkv_sst_merge), built with AddressSanitizer and
// UndefinedBehaviorSanitizer on the host code (Makefile target `sanitize-sst-merge`; device code
// uninstrumented, nothing launched, no GPU needed). The fuzz shapes of tests/sst_merge_util.py restated
// here (K in 1..8, runs of 0..3000 entries and two cases above the host-thread threshold, user keys of 0-40
// bytes over a small alphabet, random tombstones and flag) against a byte-at-a-time insertion merge with
// replacement, every input and output in a heap block of exactly its size so that any overrun is the
// sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "runs_reference.h"
#include "tkv_crc32.h"

using namespace mg_ref;  // the cases, compare, the insertion merge with replacement and the placed arrays

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

void run_case(std::uint64_t seed, std::uint32_t n_max, std::uint32_t k_fixed = 0) {
  const Case c = make_case(seed, n_max, k_fixed);
  const std::vector<std::uint64_t> list = insertion_merge(c);
  Placed p(c);
  const std::uint32_t K = static_cast<std::uint32_t>(c.runs.size());
  std::uint64_t m = 9, kb = 9, vb = 9, bad = 9;
  auto call = [&](std::uint64_t* ko, std::uint32_t* kl, std::uint64_t* vo, std::uint32_t* vl, std::uint64_t* src, std::uint64_t cap) {
    return tkv_sst_merge(K, p.pk.data(), p.size.data(), p.pko.data(), p.pkl.data(), p.pvo.data(), p.pvl.data(), p.n.data(), p.base,
                         p.bias.data(), c.flags, ko, kl, vo, vl, src, cap, &m, &kb, &vb, &bad);
  };
  std::uint64_t want_kb = 0, want_vb = 0;
  for (std::uint64_t s : list) {
    want_kb += c.runs[s >> 32].klen[s & 0xFFFFFFFFu];
    want_vb += c.runs[s >> 32].vlen[s & 0xFFFFFFFFu];
  }
  int rc = call(nullptr, nullptr, nullptr, nullptr, nullptr, 0);
  CHECK(rc == TKV_OK && m == list.size() && kb == want_kb && vb == want_vb && bad == TKV_SST_MERGE_NONE,
        "seed %llu sizing rc %d m %llu want %llu", (unsigned long long)seed, rc, (unsigned long long)m, (unsigned long long)list.size());
  if (m != list.size() || m == 0) return;
  if (m > 1) {  // one short: overflow, nothing written (the block is exactly one short too)
    std::unique_ptr<std::uint64_t[]> s1(new std::uint64_t[m - 1]);
    rc = call(nullptr, nullptr, nullptr, nullptr, s1.get(), m - 1);
    CHECK(rc == TKV_BUFFER_OVERFLOW && m == list.size(), "seed %llu overflow rc %d", (unsigned long long)seed, rc);
  }
  std::unique_ptr<std::uint64_t[]> ko(new std::uint64_t[m]), vo(new std::uint64_t[m]), src(new std::uint64_t[m]);
  std::unique_ptr<std::uint32_t[]> kl(new std::uint32_t[m]), vl(new std::uint32_t[m]);
  rc = call(ko.get(), kl.get(), vo.get(), vl.get(), src.get(), m);
  CHECK(rc == TKV_OK, "seed %llu rc %d: %s", (unsigned long long)seed, rc, tkv_last_error());
  if (rc != TKV_OK) return;
  for (std::uint64_t j = 0; j < m; ++j) {
    const std::uint64_t q = list[j] >> 32, i = list[j] & 0xFFFFFFFFu;
    const RunData& d = c.runs[q];
    CHECK(src[j] == list[j] && ko[j] == static_cast<std::uint64_t>(p.pk[q] - p.base) + d.koff[i] && kl[j] == d.klen[i] &&
              vo[j] == p.bias[q] + d.voff[i] && vl[j] == d.vlen[i],
          "seed %llu entry %llu", (unsigned long long)seed, (unsigned long long)j);
  }
}

void run_errors() {
  // run 1: "m", "z", "y": entry 2 is below entry 1
  std::vector<std::uint8_t> k0(2 * 18, 0), k1(3 * 18, 0);
  k0[0] = 'a';
  k0[18] = 'b';
  k1[0] = 'm';
  k1[18] = 'z';
  k1[36] = 'y';
  auto b0 = exact(k0), b1 = exact(k1);
  const std::uint64_t off[3] = {0, 18, 36};
  std::uint32_t len0[2] = {18, 18}, len1[3] = {18, 18, 18};
  const std::uint8_t* pk[2] = {b0.get(), b1.get()};
  const std::uint64_t size[2] = {36, 54}, n[2] = {2, 3};
  const std::uint64_t* pko[2] = {off, off};
  const std::uint32_t* pkl[2] = {len0, len1};
  std::uint64_t m = 9, kb = 9, vb = 9, bad = 9;
  auto call = [&] {
    return tkv_sst_merge(2, pk, size, pko, pkl, nullptr, nullptr, n, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                         0, &m, &kb, &vb, &bad);
  };
  int rc = call();
  CHECK(rc == TKV_CORRUPTED && bad == ((1ull << 32) | 2) && m == 0 && kb == 0 && vb == 0, "order rc %d bad %llx", rc, (unsigned long long)bad);
  len0[1] = 19;  // one past keys_size: the smaller run wins
  rc = call();
  CHECK(rc == TKV_CORRUPTED && bad == 1, "bounds rc %d bad %llx", rc, (unsigned long long)bad);
  len0[1] = 16;  // shorter than the metadata
  rc = call();
  CHECK(rc == TKV_CORRUPTED && bad == 1, "short rc %d bad %llx", rc, (unsigned long long)bad);
  m = kb = vb = bad = 9;
  rc = tkv_sst_merge(65, pk, size, pko, pkl, nullptr, nullptr, n, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                     &m, &kb, &vb, &bad);
  CHECK(rc == TKV_INVALID_ARGUMENT && m == 9 && bad == 9, "65 runs rc %d", rc);
  rc = tkv_sst_merge(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                     nullptr, nullptr, 0, &m, &kb, &vb, &bad);
  CHECK(rc == TKV_OK && m == 0 && kb == 0 && vb == 0 && bad == TKV_SST_MERGE_NONE, "no runs rc %d", rc);
}

}  // namespace

int main() {
  for (std::uint64_t seed = 0; seed < 32; ++seed) run_case(seed, seed % 4 ? 3000 : 60);
  run_case(1001, 1, 1);        // a single run of at most one entry
  run_case(1002, 9000, 4);     // above the host-thread threshold of the merge (2^14 entries)
  run_case(1003, 300, 64);     // the most runs
  run_errors();
  if (failures) {
    std::printf("%d FAILED\n", failures);
    return 1;
  }
  std::printf("ALL PASSED\n");
  return 0;
}
