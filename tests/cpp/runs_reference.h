// Shared by the stand-alone programs that check the host memtable replay and the host SSTable merge
// (test_memtable_host.cpp, test_sst_merge_host.cpp under AddressSanitizer; test_host_threads.cpp under
// ThreadSanitizer): the fuzz cases of tests/memtable_util.py and tests/sst_merge_util.py restated, and
// the serial, byte-at-a-time restatements the library's results are compared with.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "tkv_crc32.h"

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

// A heap block of exactly n elements (never a vector: its capacity may hide an overrun).
template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {
  std::unique_ptr<T[]> p(new T[v.size()]);
  if (!v.empty()) std::memcpy(p.get(), v.data(), v.size() * sizeof(T));
  return p;
}

// ---- memtable replay ---------------------------------------------------------------------------------
namespace mt_ref {

struct Case {
  std::vector<std::uint8_t> keys, op, tomb;
  std::vector<std::uint64_t> koff, voff, seq;
  std::vector<std::uint32_t> klen, vlen;
  std::uint64_t ts;
};

inline Case make_case(std::uint64_t seed, std::uint32_t n_min, std::uint32_t n_max) {
  Rng r{0x3E3E00 + seed};
  Case c;
  const std::uint32_t n = n_min + r.below(n_max - n_min + 1);
  const std::uint8_t alpha_all[7] = {0x00, 0x01, 0x61, 0x62, 0x7F, 0x80, 0xFF};
  const std::uint32_t na = 2 + r.below(6);
  const bool views = seed % 5 == 0;
  std::uint64_t vo = 0;
  c.ts = r.next() >> 16;
  if (views)
    for (std::uint32_t k = 0; k < 64 + n / 4; ++k) c.keys.push_back(alpha_all[r.below(na)]);
  for (std::uint32_t i = 0; i < n; ++i) {
    const std::uint32_t kl = r.below(5) ? r.below(6) : r.below(41);
    if (views) {
      c.koff.push_back(r.below(static_cast<std::uint32_t>(c.keys.size()) - kl + 1));
    } else {
      c.koff.push_back(c.keys.size());
      for (std::uint32_t k = 0; k < kl; ++k) c.keys.push_back(alpha_all[r.below(na)]);
    }
    c.klen.push_back(kl);
    const std::uint32_t vl = r.below(9);
    c.voff.push_back(vo);
    c.vlen.push_back(vl);
    vo += vl;
    c.op.push_back(static_cast<std::uint8_t>(r.below(2)));
    const std::uint8_t tb[6] = {0, 0, 1, 1, 2, 0xFF};
    c.tomb.push_back(tb[r.below(6)]);
    c.seq.push_back(r.next() >> 2);
  }
  return c;
}

// simd_comparator, one byte at a time.
inline int compare(const Case& c, std::uint32_t x, std::uint32_t y) {
  const std::uint32_t lx = c.klen[x], ly = c.klen[y];
  for (std::uint32_t b = 0; b < lx && b < ly; ++b) {
    const std::uint8_t p = c.keys[c.koff[x] + b], q = c.keys[c.koff[y] + b];
    if (p != q) return p < q ? -1 : 1;
  }
  return lx < ly ? -1 : lx > ly ? 1 : 0;
}

// skiplist::insert record after record: the sorted list of record indices, an equal key replaced.
inline std::vector<std::uint32_t> replay(const Case& c) {
  std::vector<std::uint32_t> list;
  for (std::uint32_t i = 0; i < c.klen.size(); ++i) {
    std::size_t lo = 0, hi = list.size();  // the first node whose key is not smaller
    while (lo < hi) {
      const std::size_t mid = (lo + hi) / 2;
      if (compare(c, list[mid], i) < 0) lo = mid + 1;
      else hi = mid;
    }
    if (lo < list.size() && compare(c, list[lo], i) == 0) list[lo] = i;
    else list.insert(list.begin() + static_cast<std::ptrdiff_t>(lo), i);
  }
  return list;
}

}  // namespace mt_ref

// ---- SSTable merge -----------------------------------------------------------------------------------
namespace mg_ref {

using Key = std::vector<std::uint8_t>;

struct RunData {
  std::vector<std::uint8_t> keys;
  std::vector<std::uint64_t> koff, voff;
  std::vector<std::uint32_t> klen, vlen;
};

// unsigned bytes, a prefix first; one byte at a time
inline int compare(const Key& a, const Key& b) {
  for (std::size_t i = 0; i < a.size() && i < b.size(); ++i)
    if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  return a.size() < b.size() ? -1 : a.size() > b.size() ? 1 : 0;
}

struct Case {
  std::vector<RunData> runs;
  std::vector<std::vector<Key>> users;
  std::uint32_t flags;
};

inline Case make_case(std::uint64_t seed, std::uint32_t n_max, std::uint32_t k_fixed) {
  Rng r{0x4D4700 + seed};
  Case c;
  const std::uint32_t K = k_fixed ? k_fixed : 1 + r.below(8);
  const std::uint8_t alpha_all[7] = {0x00, 0x01, 0x61, 0x62, 0x7F, 0x80, 0xFF};
  const std::uint32_t na = 2 + r.below(6);
  c.flags = r.below(2);
  for (std::uint32_t q = 0; q < K; ++q) {
    const std::uint32_t n = r.below(7) ? r.below(n_max + 1) : 0;
    std::vector<Key> us(n);
    for (auto& u : us) {
      const std::uint32_t len = r.below(5) < 3 ? r.below(8) : r.below(41);
      for (std::uint32_t b = 0; b < len; ++b) u.push_back(alpha_all[r.below(na)]);
    }
    std::stable_sort(us.begin(), us.end(), [](const Key& a, const Key& b) { return compare(a, b) < 0; });
    RunData d;
    std::uint64_t vo = 0;
    const std::uint32_t lead = r.below(4);  // junk in front, so that offsets are not multiples of anything
    for (std::uint32_t b = 0; b < lead; ++b) d.keys.push_back(0xEE);
    for (const Key& u : us) {
      d.koff.push_back(d.keys.size());
      d.klen.push_back(static_cast<std::uint32_t>(u.size()) + 17);
      d.keys.insert(d.keys.end(), u.begin(), u.end());
      for (int b = 0; b < 16; ++b) d.keys.push_back(static_cast<std::uint8_t>(r.next()));  // seq, timestamp: any bytes
      const std::uint8_t tb[6] = {0, 0, 0, 1, 2, 0xFF};
      d.keys.push_back(tb[r.below(6)]);
      const std::uint32_t vl = r.below(9);
      d.voff.push_back(vo);
      d.vlen.push_back(vl);
      vo += vl;
    }
    c.runs.push_back(std::move(d));
    c.users.push_back(std::move(us));
  }
  return c;
}

// Entry after entry into a sorted list of r << 32 | i, an equal user key replaced.
inline std::vector<std::uint64_t> insertion_merge(const Case& c) {
  std::vector<std::uint64_t> list;
  auto key = [&](std::uint64_t s) -> const Key& { return c.users[s >> 32][s & 0xFFFFFFFFu]; };
  for (std::uint64_t q = 0; q < c.runs.size(); ++q)
    for (std::uint64_t i = 0; i < c.users[q].size(); ++i) {
      const std::uint64_t s = (q << 32) | i;
      std::size_t lo = 0, hi = list.size();
      while (lo < hi) {
        const std::size_t mid = (lo + hi) / 2;
        if (compare(key(list[mid]), key(s)) < 0) lo = mid + 1;
        else hi = mid;
      }
      if (lo < list.size() && compare(key(list[lo]), key(s)) == 0) list[lo] = s;
      else list.insert(list.begin() + static_cast<std::ptrdiff_t>(lo), s);
    }
  if (c.flags & TKV_SST_MERGE_DROP_TOMBSTONES) {
    std::vector<std::uint64_t> kept;
    for (std::uint64_t s : list) {
      const RunData& d = c.runs[s >> 32];
      const std::uint64_t i = s & 0xFFFFFFFFu;
      if (d.keys[d.koff[i] + d.klen[i] - 1] == 0) kept.push_back(s);
    }
    list.swap(kept);
  }
  return list;
}

// The case's arrays in exact heap blocks and the call's pointer tables.
struct Placed {
  std::vector<std::unique_ptr<std::uint8_t[]>> keys;
  std::vector<std::unique_ptr<std::uint64_t[]>> koff, voff;
  std::vector<std::unique_ptr<std::uint32_t[]>> klen, vlen;
  std::vector<const std::uint8_t*> pk;
  std::vector<const std::uint64_t*> pko, pvo;
  std::vector<const std::uint32_t*> pkl, pvl;
  std::vector<std::uint64_t> size, n, bias;
  const std::uint8_t* base = nullptr;
  explicit Placed(const Case& c) {
    for (const RunData& d : c.runs) {
      keys.push_back(exact(d.keys));
      koff.push_back(exact(d.koff));
      voff.push_back(exact(d.voff));
      klen.push_back(exact(d.klen));
      vlen.push_back(exact(d.vlen));
      const bool any = !d.klen.empty();
      pk.push_back(any ? keys.back().get() : nullptr);
      pko.push_back(any ? koff.back().get() : nullptr);
      pkl.push_back(any ? klen.back().get() : nullptr);
      pvo.push_back(any ? voff.back().get() : nullptr);
      pvl.push_back(any ? vlen.back().get() : nullptr);
      size.push_back(d.keys.size());
      n.push_back(d.klen.size());
      bias.push_back(1000 * keys.size());
      if (any && (!base || keys.back().get() < base)) base = keys.back().get();
    }
  }
};

}  // namespace mg_ref
