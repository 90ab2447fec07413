// Sorted runs of internal keys on the host: the memtable replay (engine::create's replay loop into a
// memtable; include/tkv_crc32.h "Memtable replay"), the SSTable merge (compaction's k-way merge of
// such runs; "SSTable merge") and the SSTable get (engine::get over such runs; "SSTable get"). All order
// entries by user key (user_key_cmp) and let the newest of equal keys win; the device paths are
// tkv_memtable.hip, tkv_sst_merge.hip and tkv_sst_get.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "tkv_crc32.h"
#include "tkv_engine.h"
#include "tkv_host_util.h"
#include "tkv_memtable_layout.h"

using namespace tkv;

namespace {
// ---- memtable replay ---------------------------------------------------------------------------------

// The checks both entry points make before any work.
int memtable_check(const MemtableCall& c) {
  if (!ptr_ok(c.n_entries) || !ptr_ok(c.ikeys_size) || !ptr_ok(c.first_bad)) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  if (c.n > 0xFFFFFFFFull) return set_error(TKV_INVALID_ARGUMENT, "memtable build: more than 2^32 - 1 records");
  if (c.n && (!ptr_ok(c.key_off) || !ptr_ok(c.key_len) || (c.keys_size && !ptr_ok(c.keys)) ||
              (ptr_ok(c.val_len) && !ptr_ok(c.val_off))))
    return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  return TKV_OK;
}

// n == 0 (both entry points).
int memtable_empty(const MemtableCall& c) {
  *c.n_entries = *c.ikeys_size = *c.first_bad = 0;
  return TKV_OK;
}

int memtable_build_host(const MemtableCall& c) {
  if (int rc = memtable_check(c)) return rc;
  const std::uint64_t n = c.n;
  if (n == 0) return memtable_empty(c);
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
  auto cmp = [&](std::uint32_t x, std::uint32_t y) {
    return user_key_cmp(c.keys + c.key_off[x], c.key_len[x], c.keys + c.key_off[y], c.key_len[y]);
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

// ---- SSTable merge -----------------------------------------------------------------------------------

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
  const bool threaded = total >= kHostParallelMin;
  auto span_ok = [&](std::uint32_t r, std::uint64_t i) {
    const std::uint64_t ko = c.key_off[r][i];
    const std::uint32_t kl = c.key_len[r][i];
    return kl >= kMtMeta && kl < kMtMaxIkey && ko <= c.keys_size[r] && kl <= c.keys_size[r] - ko;
  };
  // entries are r << 32 | i; the order is the user keys'
  auto cmp = [&](std::uint64_t x, std::uint64_t y) {
    const std::uint32_t rx = static_cast<std::uint32_t>(x >> 32), ry = static_cast<std::uint32_t>(y >> 32);
    const std::uint64_t ix = x & 0xFFFFFFFFull, iy = y & 0xFFFFFFFFull;
    return user_key_cmp(c.keys[rx] + c.key_off[rx][ix], c.key_len[rx][ix] - kMtMeta, c.keys[ry] + c.key_off[ry][iy],
                        c.key_len[ry][iy] - kMtMeta);
  };
  // validate: every run's smallest bad index, one task per run
  std::vector<std::uint64_t> bad(K, kMergeNone);
  parallel_tasks(K, threaded, [&](std::uint64_t r) {
    bool prev_ok = false;
    for (std::uint64_t i = 0; i < c.n[r]; ++i) {
      const bool ok = span_ok(static_cast<std::uint32_t>(r), i);
      const std::uint64_t id = (r << 32) | i;
      if (!ok || (prev_ok && cmp(id, id - 1) < 0)) {
        bad[r] = id;
        break;
      }
      prev_ok = ok;
    }
  });
  *c.n_entries = *c.keys_bytes = *c.vals_bytes = 0;
  *c.first_bad = *std::min_element(bad.begin(), bad.end());
  if (*c.first_bad != kMergeNone) return set_error(TKV_CORRUPTED, "sst merge: a key span is out of bounds or a run is not ascending");
  // the lists of r << 32 | i, neighbouring lists merged pairwise (one task per pair), the older side
  // first on equal keys
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
    const std::size_t lists = cut.size() - 1;
    std::vector<std::uint64_t> ncut{0};
    for (std::size_t p = 0; p < lists; p += 2) ncut.push_back(cut[std::min(p + 2, lists)]);
    parallel_tasks((lists + 1) / 2, threaded, [&](std::uint64_t k) {
      const std::uint64_t s0 = cut[2 * k], s1 = cut[2 * k + 1], s2 = ncut[k + 1];
      std::merge(cur.begin() + s0, cur.begin() + s1, cur.begin() + s1, cur.begin() + s2, nxt.begin() + s0, less);
    });
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

// ---- SSTable get -------------------------------------------------------------------------------------

// The checks both entry points make before any work.
int sst_get_check(const SstGetCall& c) {
  if (!ptr_ok(c.n_found) || !ptr_ok(c.vals_bytes) || !ptr_ok(c.first_bad)) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  if (c.n_runs > TKV_SST_MERGE_MAX_RUNS) return set_error(TKV_INVALID_ARGUMENT, "sst get: more than 64 runs");
  if (c.flags != 0) return set_error(TKV_INVALID_ARGUMENT, "sst get: unknown flag bits");
  if (c.nq > 0xFFFFFFFFull) return set_error(TKV_INVALID_ARGUMENT, "sst get: more than 2^32 - 1 queries");
  if (c.nq && (!ptr_ok(c.q_off) || !ptr_ok(c.q_len) || (c.qkeys_size && !ptr_ok(c.qkeys))))
    return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  if (ptr_ok(c.vals) && !ptr_ok(c.vals_size)) return set_error(TKV_INVALID_ARGUMENT, "sst get: vals without vals_size");
  if ((ptr_ok(c.out_vals) || ptr_ok(c.out_val_pos)) && !ptr_ok(c.vals))
    return set_error(TKV_INVALID_ARGUMENT, "sst get: out_vals or out_val_pos without vals");
  if (c.n_runs == 0) return TKV_OK;
  if (!ptr_ok(c.keys) || !ptr_ok(c.keys_size) || !ptr_ok(c.key_off) || !ptr_ok(c.key_len) || !ptr_ok(c.n))
    return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  std::uint64_t sum = 0;
  for (std::uint32_t r = 0; r < c.n_runs; ++r) {
    if (c.n[r] > 0xFFFFFFFFull) return set_error(TKV_INVALID_ARGUMENT, "sst get: more than 2^32 - 1 entries in a run");
    sum += c.n[r];
    if (sum > 0xFFFFFFFFull) return set_error(TKV_INVALID_ARGUMENT, "sst get: more than 2^32 - 1 entries");
    if (ptr_ok(c.val_len) && ptr_ok(c.val_len[r]) && !(ptr_ok(c.val_off) && ptr_ok(c.val_off[r])))
      return set_error(TKV_INVALID_ARGUMENT, "sst get: val_len without val_off");
    if (c.n[r] == 0) continue;
    if (!ptr_ok(c.keys[r]) || !ptr_ok(c.key_off[r]) || !ptr_ok(c.key_len[r])) return set_error(TKV_INVALID_ARGUMENT, "null pointer");
  }
  return TKV_OK;
}

// nq == 0 (both entry points).
int sst_get_empty(const SstGetCall& c) {
  *c.n_found = *c.vals_bytes = 0;
  *c.first_bad = kMergeNone;
  return TKV_OK;
}

std::uint32_t bit_length(std::uint64_t n) {
  std::uint32_t b = 0;
  for (; n; n >>= 1) ++b;
  return b;
}

int sst_get_host(const SstGetCall& c) {
  if (int rc = sst_get_check(c)) return rc;
  const std::uint64_t nq = c.nq;
  if (nq == 0) return sst_get_empty(c);
  for (std::uint64_t j = 0; j < nq; ++j) {
    const std::uint64_t qo = c.q_off[j];
    const std::uint32_t ql = c.q_len[j];
    if (qo > c.qkeys_size || ql > c.qkeys_size - qo || ql >= kMtMaxIkey - kMtMeta)
      return set_error(TKV_INVALID_ARGUMENT, "sst get: a query reaches past qkeys_size or is 2^28 - 17 bytes or longer");
  }
  const std::uint32_t K = c.n_runs;
  const bool gather = ptr_ok(c.vals);
  auto val_off = [&](std::uint32_t r) { return ptr_ok(c.val_off) ? c.val_off[r] : nullptr; };
  auto val_len = [&](std::uint32_t r) { return ptr_ok(c.val_len) ? c.val_len[r] : nullptr; };
  // the device search's probe sequence (tkv_sst_get.hip: gt_search), one query after the other: a query
  // stops at its first bad probe, and the smallest bad r << 32 | i over all queries is the verdict
  std::vector<std::uint64_t> hit(nq, kMergeNone), pos(nq + 1, 0);
  std::vector<std::uint32_t> vlen(nq, 0);
  std::vector<std::uint8_t> state(nq, TKV_SST_GET_ABSENT);
  std::vector<std::uint64_t> bad(host_threads(), kMergeNone);
  parallel_ranges(nq, [&](unsigned t, std::uint64_t lo, std::uint64_t hi) {
    std::uint64_t worst = kMergeNone;
    for (std::uint64_t j = lo; j < hi; ++j) {
      const std::uint8_t* q = c.qkeys + c.q_off[j];
      const std::uint32_t ql = c.q_len[j];
      bool done = false;
      for (std::uint32_t r = K; !done && r-- > 0u;) {
        const std::uint64_t n = c.n[r];
        if (n == 0) continue;
        std::uint64_t at = 0;
        bool eq = false;
        for (std::uint64_t step = std::uint64_t{1} << (bit_length(n) - 1u); step != 0 && !done; step >>= 1) {
          const std::uint64_t cand = at + step;
          if (cand > n) continue;
          const std::uint64_t i = cand - 1u;
          const std::uint64_t ko = c.key_off[r][i];
          const std::uint32_t kl = c.key_len[r][i];
          if (!(kl >= kMtMeta && kl < kMtMaxIkey && ko <= c.keys_size[r] && kl <= c.keys_size[r] - ko)) {
            worst = std::min(worst, (static_cast<std::uint64_t>(r) << 32) | i);
            done = true;
            break;
          }
          const int cmp = user_key_cmp(c.keys[r] + ko, kl - kMtMeta, q, ql);
          if (cmp <= 0) {
            at = cand;
            eq = cmp == 0;
          }
        }
        if (done || !eq) continue;
        const std::uint64_t i = at - 1u;
        const bool tomb = c.keys[r][c.key_off[r][i] + c.key_len[r][i] - 1u] != 0;
        done = true;
        if (!tomb) {
          const std::uint32_t vl = val_len(r) ? val_len(r)[i] : 0u;
          const std::uint64_t vo = val_off(r) ? val_off(r)[i] : 0u;
          const std::uint64_t vsize = gather && ptr_ok(c.vals[r]) ? c.vals_size[r] : 0u;
          if (gather && (vo > vsize || vl > vsize - vo)) {
            worst = std::min(worst, (static_cast<std::uint64_t>(r) << 32) | i);
            continue;
          }
          vlen[j] = vl;
        }
        hit[j] = (static_cast<std::uint64_t>(r) << 32) | i;
        state[j] = tomb ? TKV_SST_GET_DELETED : TKV_SST_GET_FOUND;
      }
    }
    bad[t] = worst;
  });
  *c.n_found = *c.vals_bytes = 0;
  *c.first_bad = *std::min_element(bad.begin(), bad.end());
  if (*c.first_bad != kMergeNone) return set_error(TKV_CORRUPTED, "sst get: a probed entry's key span or a hit's value span is out of bounds");
  std::uint64_t found = 0;
  for (std::uint64_t j = 0; j < nq; ++j) {
    found += state[j] == TKV_SST_GET_FOUND;
    pos[j + 1] = pos[j] + vlen[j];
  }
  *c.n_found = found;
  *c.vals_bytes = pos[nq];
  if (ptr_ok(c.out_vals) && pos[nq] > c.vals_cap) return set_error(TKV_BUFFER_OVERFLOW, "sst get: the values do not fit");
  parallel_for(nq, [&](std::uint64_t j) {
    const std::uint32_t r = static_cast<std::uint32_t>(hit[j] >> 32);
    const std::uint64_t i = hit[j] & 0xFFFFFFFFull;
    const bool any = hit[j] != kMergeNone, live = state[j] == TKV_SST_GET_FOUND;
    if (ptr_ok(c.state)) c.state[j] = state[j];
    if (ptr_ok(c.src)) c.src[j] = hit[j];
    if (ptr_ok(c.seq)) {
      std::uint64_t seq = 0;
      if (any) {
        const std::uint8_t* m = c.keys[r] + c.key_off[r][i] + (c.key_len[r][i] - kMtMeta) + kMtSeq;
        for (std::uint32_t b = 0; b < 8; ++b) seq |= static_cast<std::uint64_t>(m[b]) << (8 * b);
      }
      c.seq[j] = seq;
    }
    if (ptr_ok(c.out_val_off)) c.out_val_off[j] = live ? (ptr_ok(c.val_bias) ? c.val_bias[r] : 0u) + (val_off(r) ? val_off(r)[i] : 0u) : 0u;
    if (ptr_ok(c.out_val_len)) c.out_val_len[j] = vlen[j];
    if (ptr_ok(c.out_val_pos)) c.out_val_pos[j] = pos[j];
    if (ptr_ok(c.out_vals) && vlen[j]) std::memcpy(c.out_vals + pos[j], c.vals[r] + val_off(r)[i], vlen[j]);
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
  if (n == 0) return memtable_empty(c);
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

int tkv_sst_get_device(uint32_t n_runs, const uint8_t* const* d_keys, const uint64_t* keys_size, const uint64_t* const* d_key_off,
                       const uint32_t* const* d_key_len, const uint64_t* const* d_val_off, const uint32_t* const* d_val_len,
                       const uint64_t* n, const uint8_t* const* d_vals, const uint64_t* vals_size, const uint64_t* val_bias,
                       const uint8_t* d_qkeys, uint64_t qkeys_size, const uint64_t* d_q_off, const uint32_t* d_q_len, uint64_t nq,
                       uint32_t flags, uint8_t* d_state, uint64_t* d_src, uint64_t* d_seq, uint64_t* d_out_val_off,
                       uint32_t* d_out_val_len, uint64_t* d_out_val_pos, uint8_t* d_out_vals, uint64_t vals_cap,
                       uint64_t* n_found, uint64_t* vals_bytes, uint64_t* first_bad, void* stream) {
  const SstGetCall c{n_runs, d_keys, keys_size, d_key_off, d_key_len, d_val_off, d_val_len, n, d_vals, vals_size, val_bias,
                     d_qkeys, qkeys_size, d_q_off, d_q_len, nq, flags, d_state, d_src, d_seq, d_out_val_off, d_out_val_len,
                     d_out_val_pos, d_out_vals, vals_cap, n_found, vals_bytes, first_bad};
  if (int rc = sst_get_check(c)) return rc;
  if (nq == 0) return sst_get_empty(c);
  return sst_get_device_impl(c, static_cast<hipStream_t>(stream));
}

int tkv_sst_get(uint32_t n_runs, const uint8_t* const* h_keys, const uint64_t* keys_size, const uint64_t* const* h_key_off,
                const uint32_t* const* h_key_len, const uint64_t* const* h_val_off, const uint32_t* const* h_val_len,
                const uint64_t* n, const uint8_t* const* h_vals, const uint64_t* vals_size, const uint64_t* val_bias,
                const uint8_t* h_qkeys, uint64_t qkeys_size, const uint64_t* h_q_off, const uint32_t* h_q_len, uint64_t nq,
                uint32_t flags, uint8_t* h_state, uint64_t* h_src, uint64_t* h_seq, uint64_t* h_out_val_off,
                uint32_t* h_out_val_len, uint64_t* h_out_val_pos, uint8_t* h_out_vals, uint64_t vals_cap, uint64_t* n_found,
                uint64_t* vals_bytes, uint64_t* first_bad) {
  const SstGetCall c{n_runs, h_keys, keys_size, h_key_off, h_key_len, h_val_off, h_val_len, n, h_vals, vals_size, val_bias,
                     h_qkeys, qkeys_size, h_q_off, h_q_len, nq, flags, h_state, h_src, h_seq, h_out_val_off, h_out_val_len,
                     h_out_val_pos, h_out_vals, vals_cap, n_found, vals_bytes, first_bad};
  return sst_get_host(c);
}

}  // extern "C"
