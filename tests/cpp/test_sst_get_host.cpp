// Stand-alone check of the host SSTable get (tkv_sst_get), built with AddressSanitizer and
// UndefinedBehaviorSanitizer on the host code (Makefile target `sanitize-sst-get`; device code
// uninstrumented, nothing launched, no GPU needed). The merge's fuzz runs (runs_reference.h: K in 1..8 and 64,
// runs of 0..3000 entries, user keys of 0-40 bytes over a small alphabet, random tombstones) looked up with
// every user key of the union, cut and extended copies of them and the same key many times, against a
// byte-at-a-time linear search: runs newest first, in a run the last entry whose user key is equal. Runs,
// queries, values and every output sit in heap blocks of exactly their size, the last key and the last
// value of a run at the very end of their arenas, so that any overrun is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "runs_reference.h"
#include "tkv_crc32.h"

using namespace mg_ref;  // the cases, compare and the placed arrays

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

struct Answer {
  std::uint8_t state = TKV_SST_GET_ABSENT;
  std::uint64_t src = TKV_SST_MERGE_NONE, seq = 0, voff = 0;
  std::uint32_t vlen = 0;
};

// Byte at a time, entry after entry.
Answer linear_get(const Case& c, const Placed& p, const Key& q) {
  Answer a;
  for (std::size_t r = c.runs.size(); r-- > 0;) {
    const RunData& d = c.runs[r];
    std::size_t hit = d.klen.size();
    for (std::size_t i = 0; i < d.klen.size(); ++i)
      if (compare(c.users[r][i], q) == 0) hit = i;
    if (hit == d.klen.size()) continue;
    const std::uint8_t* meta = d.keys.data() + d.koff[hit] + d.klen[hit] - 17;
    a.src = (static_cast<std::uint64_t>(r) << 32) | hit;
    for (int b = 0; b < 8; ++b) a.seq |= static_cast<std::uint64_t>(meta[b]) << (8 * b);
    a.state = meta[16] ? TKV_SST_GET_DELETED : TKV_SST_GET_FOUND;
    if (!meta[16]) {
      a.voff = p.bias[r] + d.voff[hit];
      a.vlen = d.vlen[hit];
    }
    return a;
  }
  return a;
}

void run_case(std::uint64_t seed, std::uint32_t n_max, std::uint32_t k_fixed = 0, std::uint32_t repeat = 1) {
  const Case c = make_case(seed, n_max, k_fixed);
  Placed p(c);
  const std::uint32_t K = static_cast<std::uint32_t>(c.runs.size());
  // the value arenas: exactly the values' bytes, a pattern that names run and byte
  std::vector<std::unique_ptr<std::uint8_t[]>> vals;
  std::vector<const std::uint8_t*> pv;
  std::vector<std::uint64_t> vsize;
  for (std::uint32_t r = 0; r < K; ++r) {
    std::uint64_t total = 0;
    for (std::uint32_t v : c.runs[r].vlen) total += v;
    std::vector<std::uint8_t> bytes(total);
    for (std::uint64_t b = 0; b < total; ++b) bytes[b] = static_cast<std::uint8_t>(r * 37 + b * 11 + 1);
    vals.push_back(exact(bytes));
    pv.push_back(total ? vals.back().get() : nullptr);
    vsize.push_back(total);
  }
  // the queries: every user key, one cut short, one extended; each `repeat` times
  Rng rng{0x6E7000 + seed};
  std::vector<Key> qs;
  for (const auto& us : c.users)
    for (const Key& u : us) {
      for (std::uint32_t k = 0; k < repeat; ++k) qs.push_back(u);
      Key cut(u.begin(), u.begin() + (u.empty() ? 0 : rng.below(static_cast<std::uint32_t>(u.size()))));
      qs.push_back(cut);
      Key ext = u;
      ext.push_back(static_cast<std::uint8_t>(rng.next()));
      qs.push_back(ext);
    }
  qs.push_back(Key{});
  const std::uint64_t nq = qs.size();
  std::vector<std::uint8_t> arena;
  std::vector<std::uint64_t> qoff;
  std::vector<std::uint32_t> qlen;
  for (const Key& q : qs) {
    qoff.push_back(arena.size());
    qlen.push_back(static_cast<std::uint32_t>(q.size()));
    arena.insert(arena.end(), q.begin(), q.end());
  }
  auto qa = exact(arena);
  auto qo = exact(qoff);
  auto ql = exact(qlen);
  std::vector<Answer> want;
  std::uint64_t want_found = 0, want_bytes = 0;
  for (const Key& q : qs) {
    want.push_back(linear_get(c, p, q));
    want_found += want.back().state == TKV_SST_GET_FOUND;
    want_bytes += want.back().vlen;
  }
  std::uint64_t found = 9, bytes = 9, bad = 9;
  auto call = [&](bool gather, std::uint8_t* st, std::uint64_t* src, std::uint64_t* seq, std::uint64_t* vo, std::uint32_t* vl,
                  std::uint64_t* pos, std::uint8_t* out, std::uint64_t cap) {
    return tkv_sst_get(K, p.pk.data(), p.size.data(), p.pko.data(), p.pkl.data(), p.pvo.data(), p.pvl.data(), p.n.data(),
                       gather ? pv.data() : nullptr, gather ? vsize.data() : nullptr, p.bias.data(), arena.empty() ? nullptr : qa.get(),
                       arena.size(), qo.get(), ql.get(), nq, 0, st, src, seq, vo, vl, pos, out, cap, &found, &bytes, &bad);
  };
  int rc = call(false, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
  CHECK(rc == TKV_OK && found == want_found && bytes == want_bytes && bad == TKV_SST_MERGE_NONE,
        "seed %llu sizing rc %d found %llu want %llu", (unsigned long long)seed, rc, (unsigned long long)found, (unsigned long long)want_found);
  if (want_bytes > 0) {  // one byte short: overflow, nothing written (the block is exactly one short too)
    std::unique_ptr<std::uint8_t[]> s1(new std::uint8_t[want_bytes - 1]);
    rc = call(true, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, s1.get(), want_bytes - 1);
    CHECK(rc == TKV_BUFFER_OVERFLOW && bytes == want_bytes, "seed %llu overflow rc %d", (unsigned long long)seed, rc);
  }
  std::unique_ptr<std::uint8_t[]> st(new std::uint8_t[nq]), out(new std::uint8_t[want_bytes]);
  std::unique_ptr<std::uint64_t[]> src(new std::uint64_t[nq]), seq(new std::uint64_t[nq]), vo(new std::uint64_t[nq]), pos(new std::uint64_t[nq]);
  std::unique_ptr<std::uint32_t[]> vl(new std::uint32_t[nq]);
  rc = call(true, st.get(), src.get(), seq.get(), vo.get(), vl.get(), pos.get(), out.get(), want_bytes);
  CHECK(rc == TKV_OK && found == want_found && bytes == want_bytes, "seed %llu rc %d: %s", (unsigned long long)seed, rc, tkv_last_error());
  if (rc != TKV_OK) return;
  std::uint64_t at = 0;
  for (std::uint64_t j = 0; j < nq; ++j) {
    const Answer& a = want[j];
    CHECK(st[j] == a.state && src[j] == a.src && seq[j] == a.seq && vo[j] == a.voff && vl[j] == a.vlen && pos[j] == at,
          "seed %llu query %llu", (unsigned long long)seed, (unsigned long long)j);
    if (a.vlen) {
      const std::uint64_t r = a.src >> 32;
      bool same = true;
      for (std::uint32_t b = 0; b < a.vlen; ++b) same = same && out[at + b] == pv[r][a.voff - p.bias[r] + b];
      CHECK(same, "seed %llu value of query %llu", (unsigned long long)seed, (unsigned long long)j);
    }
    at += a.vlen;
  }
}

void run_errors() {
  // one run: "a", "b", "c" with values "", "xy", "z"; the last key and value end their arenas
  std::vector<std::uint8_t> k(3 * 18, 0), v{'x', 'y', 'z'}, q{'b', 'c', 'a'};
  k[0] = 'a';
  k[18] = 'b';
  k[36] = 'c';
  auto bk = exact(k), bv = exact(v), bq = exact(q);
  const std::uint64_t off[3] = {0, 18, 36}, voff[3] = {0, 0, 2}, qoff[3] = {0, 1, 2};
  std::uint32_t len[3] = {18, 18, 18}, vlen[3] = {0, 2, 1}, qlen[3] = {1, 1, 1};
  const std::uint8_t* pk[1] = {bk.get()};
  const std::uint8_t* pv[1] = {bv.get()};
  const std::uint64_t* pko[1] = {off};
  const std::uint64_t* pvo[1] = {voff};
  const std::uint32_t* pkl[1] = {len};
  const std::uint32_t* pvl[1] = {vlen};
  std::uint64_t size[1] = {54}, vsize[1] = {3}, n[1] = {3};
  std::uint64_t found = 9, bytes = 9, bad = 9;
  std::uint8_t st[3], out[3];
  std::uint64_t qsize = 3, nq = 3;
  auto call = [&] {
    return tkv_sst_get(1, pk, size, pko, pkl, pvo, pvl, n, pv, vsize, nullptr, bq.get(), qsize, qoff, qlen, nq, 0, st, nullptr, nullptr,
                       nullptr, nullptr, nullptr, out, 3, &found, &bytes, &bad);
  };
  int rc = call();
  CHECK(rc == TKV_OK && found == 3 && bytes == 3 && std::memcmp(out, "xyz", 3) == 0 && st[0] == 1 && st[2] == 1, "sound rc %d", rc);
  size[0] = 53;  // the last key reaches one past keys_size: read by the query for "c" (probes 1, then 2)
  rc = call();
  CHECK(rc == TKV_CORRUPTED && bad == 2 && found == 0 && bytes == 0, "bounds rc %d bad %llx", rc, (unsigned long long)bad);
  nq = 1;  // the query for "b" alone probes entry 1 and then 2 as well; the one for "a" (nq = 1 at offset 2) only 1 and 0
  rc = call();
  CHECK(rc == TKV_CORRUPTED && bad == 2, "bounds, b alone rc %d bad %llx", rc, (unsigned long long)bad);
  const std::uint64_t qoff_a[1] = {2};
  rc = tkv_sst_get(1, pk, size, pko, pkl, pvo, pvl, n, pv, vsize, nullptr, bq.get(), qsize, qoff_a, qlen, 1, 0, st, nullptr, nullptr, nullptr,
                   nullptr, nullptr, out, 3, &found, &bytes, &bad);
  CHECK(rc == TKV_OK && found == 1 && bytes == 0 && bad == TKV_SST_MERGE_NONE && st[0] == 1, "unread rc %d", rc);
  size[0] = 54;
  nq = 3;
  vsize[0] = 2;  // the last value reaches one past vals_size
  rc = call();
  CHECK(rc == TKV_CORRUPTED && bad == 2, "value rc %d bad %llx", rc, (unsigned long long)bad);
  vsize[0] = 3;
  qsize = 2;  // the last query reaches past qkeys_size: invalid, whatever the runs
  size[0] = 53;
  found = bytes = bad = 9;
  rc = call();
  CHECK(rc == TKV_INVALID_ARGUMENT && found == 9 && bad == 9, "query rc %d", rc);
  rc = tkv_sst_get(65, pk, size, pko, pkl, pvo, pvl, n, pv, vsize, nullptr, bq.get(), 3, qoff, qlen, 3, 0, st, nullptr, nullptr, nullptr,
                   nullptr, nullptr, out, 3, &found, &bytes, &bad);
  CHECK(rc == TKV_INVALID_ARGUMENT && found == 9, "65 runs rc %d", rc);
  rc = tkv_sst_get(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, bq.get(), 3, qoff, qlen, 3, 0,
                   st, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &found, &bytes, &bad);
  CHECK(rc == TKV_OK && found == 0 && bytes == 0 && bad == TKV_SST_MERGE_NONE && st[0] == 0 && st[1] == 0 && st[2] == 0, "no runs rc %d", rc);
}

}  // namespace

int main() {
  for (std::uint64_t seed = 0; seed < 32; ++seed) run_case(seed, seed % 4 ? 600 : 60);
  run_case(1001, 1, 1);          // a single run of at most one entry
  run_case(1002, 3000, 4);       // above the host-thread threshold of the loops (2^14 queries)
  run_case(1003, 100, 64);       // the most runs
  run_case(1004, 40, 2, 130);    // the same key many times
  run_errors();
  if (failures) {
    std::printf("%d FAILED\n", failures);
    return 1;
  }
  std::printf("ALL PASSED\n");
  return 0;
}
