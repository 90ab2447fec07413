// The wave-per-query search of DESIGN.md §6.11, as it was measured for probe_wave_per_query.txt. It is NOT
// part of the library and is not built. To reproduce: paste it into tinykvpp_amd/csrc/tkv_sst_get.hip in
// front of the "scans" section, and in get_locked launch it in place of gt_search with
//   hipLaunchKernelGGL(gt_search_wave, dim3(blocks(nq, kGtThreads / 64u)), dim3(kGtThreads), 0, st, a);
// (a wave per query, four queries a workgroup). It does not report the step count of the debug hook.
// EXPERIMENT (wave per query): 64 pivots per step, the range shrinks 65-fold; a last step over <= 64 entries.
__device__ __forceinline__ int gt_cmp_entry(const MgRun& run, std::uint64_t ko, std::uint32_t kl, MgKey q, std::uint64_t qw, std::uint32_t qd) {
  const MgKey k{reinterpret_cast<std::uintptr_t>(run.keys) + ko, kl - kMtMeta};
  const std::uint64_t w = load_word(k.addr, k.ulen);
  const std::uint32_t d = mt_digit(k.ulen);
  return w != qw ? (w < qw ? -1 : 1) : d != qd ? (d < qd ? -1 : 1) : d < kMtDigitMore ? 0 : cmp_rest(k, q);
}

__global__ __launch_bounds__(kGtThreads) void gt_search_wave(GtArgs a) {
  const std::uint32_t lane = threadIdx.x & 63u;
  const std::uint64_t j = __builtin_amdgcn_readfirstlane(static_cast<std::uint32_t>(blockIdx.x * (kGtThreads / 64u) + (threadIdx.x >> 6)));
  if (j >= a.nq) return;
  const std::uint64_t qo = a.q_off[j];
  const std::uint32_t ql = a.q_len[j];
  if (qo > a.qkeys_size || ql > a.qkeys_size - qo || ql >= kMtMaxIkey - kMtMeta) {
    if (lane == 0) atomicMax(a.st + kGsBadQuery, 1ull);
    return;
  }
  const MgKey q{reinterpret_cast<std::uintptr_t>(a.qkeys) + qo, ql};
  const std::uint64_t qw = load_word(q.addr, ql);
  const std::uint32_t qd = mt_digit(ql);
  std::uint32_t state = TKV_SST_GET_ABSENT, vlen = 0;
  std::uint64_t hit = kGtNone;
  bool bad = false;
  for (std::uint32_t r = a.n_runs; r-- > 0u && hit == kGtNone && !bad;) {
    const GtRun& g = a.runs[r];
    std::uint32_t lo = 0, hi = g.n;
    while (hi > lo && !bad) {
      const std::uint32_t width = hi - lo;
      const bool last = width <= 64u;
      const std::uint32_t idx = last ? lo + lane : lo + static_cast<std::uint32_t>((static_cast<std::uint64_t>(lane + 1u) * width) / 65u);
      bool le = false, ok = true;
      if (!last || lane < width) {
        const std::uint64_t ko = g.run.key_off[idx];
        const std::uint32_t kl = g.run.key_len[idx];
        ok = span_ok(g.run, ko, kl);
        if (ok) le = gt_cmp_entry(g.run, ko, kl, q, qw, qd) <= 0;
      }
      if (__ballot(!ok) != 0ull) {
        bad = true;
        if (!ok) atomicMin(a.st + kGsBad, (static_cast<unsigned long long>(r) << 32) | idx);
        break;
      }
      const std::uint32_t c = static_cast<std::uint32_t>(__popcll(__ballot(le)));
      if (last) {
        lo = hi = lo + c;
      } else {
        const std::uint32_t nlo = c == 0u ? lo : lo + static_cast<std::uint32_t>((static_cast<std::uint64_t>(c) * width) / 65u) + 1u;
        const std::uint32_t nhi = c == 64u ? hi : lo + static_cast<std::uint32_t>((static_cast<std::uint64_t>(c + 1u) * width) / 65u);
        lo = nlo;
        hi = nhi;
      }
    }
    if (!bad && lo > 0u) {
      const std::uint32_t i = lo - 1u;
      const std::uint64_t ko = g.run.key_off[i];
      const std::uint32_t kl = g.run.key_len[i];
      if (span_ok(g.run, ko, kl) && gt_cmp_entry(g.run, ko, kl, q, qw, qd) == 0) {
        const bool tomb = g.run.keys[ko + kl - 1u] != 0;
        hit = (static_cast<std::uint64_t>(r) << 32) | i;
        state = tomb ? TKV_SST_GET_DELETED : TKV_SST_GET_FOUND;
        if (!tomb) {
          vlen = g.run.val_len ? g.run.val_len[i] : 0u;
          const std::uint64_t vo = g.run.val_off ? g.run.val_off[i] : 0ull;
          if (a.gather && (vo > g.vals_size || vlen > g.vals_size - vo)) {
            bad = true;
            if (lane == 0) atomicMin(a.st + kGsBad, hit);
          }
        }
      }
    }
  }
  if (lane == 0) {
    a.hit[j] = bad ? kGtNone : hit;
    a.info[j] = bad ? 0ull : (static_cast<std::uint64_t>(state) << kGtStateShift) | vlen;
  }
}

