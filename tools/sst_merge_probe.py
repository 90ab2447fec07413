#!/usr/bin/env python3
"""Time of the device SSTable merge (not product code): the runs DESIGN.md §6.7-6.9 use (18.2 M small
entries: user keys 4-23 B, values 0-39 B; 400 K Zipf entries: keys 8-63 B, values up to 16 KB), sorted and
deduplicated once by the memtable replay and then dealt out to K = 2, 4 and 8 runs with interleaved key
ranges (entry j goes to run j mod K), and the small entries with every tenth key written again in a newer
run. After untimed warm-ups, K warm calls per leg, in one process, in rotation, each between a pair of
device events on the calls' stream:
  merge    tkv_sst_merge_device of the runs, with its phase times (check, rounds, ties and scan, emit) from
           tkv_debug_sst_merge_phases
  replay   the route the merge replaces: tkv_memtable_build_device over the concatenated columns with the 17
           metadata bytes taken off key_len (it sorts again what is sorted, and writes new internal keys)
and once per shape, with the same clock, sst.compact_device of the runs' files end to end beside its three
stages (scan_device of every file with both view flags, merge_device, flush). Prints one JSON line per
shape and K. The merged order is checked against the deal.

    python tools/sst_merge_probe.py [--k 10] [--warmup 2] [--small-entries N] [--shapes small,zipf,overwrite]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tinykvpp_amd as tk  # noqa: E402
from tinykvpp_amd import memtable, sst  # noqa: E402

VP, U64 = ctypes.c_void_p, ctypes.c_uint64
PHASES = ("check", "rounds", "ties_scan", "emit")


def timed(fn):
    """Milliseconds between device events around one synchronous call on the current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def arena(lens, dev):
    """Random bytes for spans of `lens` bytes back to back from byte 1 (odd addresses): (arena, offsets)."""
    off = np.ones(lens.size, np.int64)
    off[1:] += np.cumsum(lens[:-1].astype(np.int64))
    data = torch.randint(0, 256, (int(lens.sum()) + 17,), dtype=torch.uint8, device=dev)
    return data, torch.from_numpy(off).to(dev)


def sorted_run(klen, vlen, dev):
    """One sorted run without duplicates over random keys of the given lengths: a MemtableRun."""
    keys, koff = arena(klen, dev)
    vals, voff = arena(vlen, dev)
    return memtable.build_device(keys=keys, key_off=koff, key_len=torch.from_numpy(klen.view(np.int32)).to(dev), val_off=voff,
                                 val_len=torch.from_numpy(vlen.view(np.int32)).to(dev), vals=vals, timestamp_ms=7)


def deal(run, k):
    """The run's entries dealt out to k runs over its two arenas: entry j to run j mod k."""
    return [(run.ikeys, run.ikey_off[r::k].contiguous(), run.ikey_len[r::k].contiguous(), run.vals,
             run.val_off[r::k].contiguous(), run.val_len[r::k].contiguous()) for r in range(k)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small-entries", type=int, default=18_199_191)
    ap.add_argument("--zipf-entries", type=int, default=400_000)
    ap.add_argument("--shapes", default="small,zipf,overwrite")
    ap.add_argument("--runs", default="2,4,8")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    tk.set_device(0)
    lib = tk.load_library()
    rng = np.random.default_rng(1)
    n = args.small_entries
    small = (rng.integers(4, 24, n).astype(np.uint32), rng.integers(0, 40, n).astype(np.uint32))
    n2 = args.zipf_entries
    zv = np.minimum(rng.zipf(1.6, n2) * 64, 16_000).astype(np.uint32)
    zipf = (rng.integers(8, 64, n2).astype(np.uint32), zv)
    st = VP(torch.cuda.current_stream().cuda_stream)
    p = lambda t: VP(t.data_ptr()) if t is not None and t.numel() else None  # noqa: E731
    shapes = []
    want = args.shapes.split(",")
    for name, lens in (("small", small), ("zipf", zipf)):
        if name in want or (name == "small" and "overwrite" in want):
            run = sorted_run(*lens, dev)
            if name in want:
                for k in (int(x) for x in args.runs.split(",")):
                    shapes.append((f"{name} K={k}", deal(run, k), "deal"))
            if name == "small" and "overwrite" in want:
                newer = tuple(c[::10].contiguous() if i in (1, 2, 4, 5) else c for i, c in enumerate(deal(run, 1)[0]))
                shapes.append(("small, a tenth written again", [deal(run, 1)[0], newer], "overwrite"))
    for name, runs, kind in shapes:
        k = len(runs)
        total = sum(r[2].numel() for r in runs)
        merged = sst.merge_device(runs)
        m = merged.n_entries
        # the order the deal implies
        j = torch.arange(m, device=dev, dtype=torch.int64)
        if kind == "deal":
            expect = ((j % k) << 32) | (j // k)
        else:
            expect = torch.where(j % 10 == 0, (1 << 32) | (j // 10), j)
        assert m == (total if kind == "deal" else runs[0][2].numel()), (m, total)
        assert torch.equal(merged.src, expect), "the merged order is not the deal's"
        key_base, val_base = merged.key_base, merged.val_base
        vp_arr = lambda vals: (VP * k)(*vals)  # noqa: E731
        a_keys = vp_arr([r[0].data_ptr() for r in runs])
        a_size = (U64 * k)(*[r[0].numel() for r in runs])
        a_cols = [vp_arr([r[c].data_ptr() for r in runs]) for c in (1, 2, 4, 5)]
        a_n = (U64 * k)(*[r[2].numel() for r in runs])
        a_bias = (U64 * k)(*[r[3].data_ptr() - val_base for r in runs])

        def merge():
            out = [U64(0) for _ in range(4)]
            rc = lib.tkv_sst_merge_device(k, a_keys, a_size, *a_cols, a_n, VP(key_base), a_bias, 0, p(merged.key_off),
                                          p(merged.key_len), p(merged.val_off), p(merged.val_len), p(merged.src), m,
                                          *[ctypes.byref(o) for o in out], st)
            ms = (ctypes.c_double * 4)()
            lib.tkv_debug_sst_merge_phases(1, ms)
            return rc, out[0].value, list(ms)

        # the replaced route: one replay over the concatenated columns, user keys only
        cat = [torch.cat([r[c] for r in runs]) for c in (1, 2, 4, 5)]
        cat[1] = cat[1] - 17
        rep = memtable.build_device(keys=runs[0][0], key_off=cat[0], key_len=cat[1], val_off=cat[2], val_len=cat[3], timestamp_ms=7)
        rm, rsize = rep.ikey_len.numel(), rep.ikeys.numel()
        assert rm == m

        def replay():
            out = [U64(0) for _ in range(3)]
            return lib.tkv_memtable_build_device(p(runs[0][0]), runs[0][0].numel(), p(cat[0]), p(cat[1]), p(cat[2]), p(cat[3]),
                                                 None, None, None, total, 7, p(rep.ikeys), rsize, p(rep.ikey_off),
                                                 p(rep.ikey_len), p(rep.val_off), p(rep.val_len), p(rep.src), rm,
                                                 *[ctypes.byref(o) for o in out], st), out[0].value

        lib.tkv_debug_sst_merge_phases(1, None)
        legs = [("merge", merge), ("replay", replay)]
        times = {q: [] for q, _ in legs}
        phases = {q: [] for q in PHASES}
        out = {}
        for r in range(args.warmup + args.k):
            for q, fn in (legs if r % 2 == 0 else legs[::-1]):
                ms, out[q] = timed(fn)
                if r >= args.warmup:
                    times[q].append(ms)
                    if q == "merge":
                        for ph, v in zip(PHASES, out[q][2]):
                            phases[ph].append(v)
        lib.tkv_debug_sst_merge_phases(0, None)
        assert out["merge"][:2] == (0, m) and out["replay"] == (0, m), out
        last = np.zeros(4, np.uint64)
        lib.tkv_debug_sst_merge_last(VP(last.ctypes.data))
        # compaction end to end: the runs as files, then scan -> merge -> flush
        files = [sst.build_device(*r).file for r in runs]
        stage = {}
        for r in range(args.warmup + 3):
            t_scan, tables = timed(lambda: [sst.scan_device(f, key_views=True, val_views=True) for f in files])
            t_merge, mr = timed(lambda: sst.merge_device(tables))
            t_flush, built = timed(lambda: mr.flush())
            t_all, whole = timed(lambda: sst.compact_device(files))
            if r >= args.warmup:
                for q, v in (("scan", t_scan), ("merge_py", t_merge), ("flush", t_flush), ("compact", t_all)):
                    stage.setdefault(q, []).append(v)
            assert whole.size == built.size
            del tables, mr, built, whole
        med = {q: float(np.median(v)) for q, v in times.items()}
        line = {"shape": name, "runs": k, "entries_in": total, "entries_out": m, "rounds": int(last[1]),
                "last_round_tiles": int(last[2]), "scratch_bytes": int(last[3]), "k": args.k}
        for q in times:
            line[q + "_ms"] = round(med[q], 4)
            line[q + "_min_max_ms"] = [round(min(times[q]), 4), round(max(times[q]), 4)]
        for q in PHASES:
            line["phase_" + q + "_ms"] = round(float(np.median(phases[q])), 4)
        line["merge_Mentries_per_s"] = round(total / med["merge"] / 1e3, 1)
        line["replay_over_merge_time"] = round(med["replay"] / med["merge"], 2)
        for q, v in stage.items():
            line[q + "_ms"] = round(float(np.median(v)), 3)
        line["file_bytes_in"] = int(sum(f.numel() for f in files))
        print(json.dumps(line), flush=True)
        del merged, rep, cat, files
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
