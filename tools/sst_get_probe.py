#!/usr/bin/env python3
"""Time of the device SSTable get (not product code): the 18.2 M small entries of DESIGN.md §6.10 (user keys
4-23 B, values 0-39 B), sorted and deduplicated once by the memtable replay, as one run and dealt out to eight
runs with interleaved key ranges (entry j goes to run j mod 8). Query batches of 2^10, 2^16 and 2^20 keys:
uniformly drawn present keys, absent keys (a present key with one byte appended) and one hot key, each with
and without the value gather. After untimed warm-ups, K warm calls per leg between a pair of device events on
the calls' stream, with the phase times (search, scans, columns, gather) from tkv_debug_sst_get_phases. Two
yardsticks on the same data in the same process:
  host     tkv_sst_get on the host's threads (wall clock, 3 calls, with the gather)
  merge    one tkv_sst_merge_device of the same runs: the only device-side way to the same answer without
           the get
Prints one JSON line per dataset, query kind, nq and gather. The states are checked against the draw.

    python tools/sst_get_probe.py [--k 10] [--warmup 2] [--entries N] [--runs 1,8] [--nq 10,16,20]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tinykvpp_amd as tk  # noqa: E402
from tinykvpp_amd import memtable  # noqa: E402

VP, U64 = ctypes.c_void_p, ctypes.c_uint64
PHASES = ("search", "scan", "columns", "gather")


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
    keys, koff = arena(klen, dev)
    vals, voff = arena(vlen, dev)
    return memtable.build_device(keys=keys, key_off=koff, key_len=torch.from_numpy(klen.view(np.int32)).to(dev), val_off=voff,
                                 val_len=torch.from_numpy(vlen.view(np.int32)).to(dev), vals=vals, timestamp_ms=7)


def deal(run, k):
    return [(run.ikeys, run.ikey_off[r::k].contiguous(), run.ikey_len[r::k].contiguous(), run.vals,
             run.val_off[r::k].contiguous(), run.val_len[r::k].contiguous()) for r in range(k)]


def gather_keys(ikeys, off, ln, extra=None):
    """The user keys [off, off + ln) of a host arena back to back (with one byte `extra` behind each):
    (arena, offsets, lengths)."""
    add = 0 if extra is None else 1
    qlen = (ln + add).astype(np.uint32)
    qoff = np.zeros(ln.size, np.uint64)
    qoff[1:] = np.cumsum(qlen[:-1], dtype=np.uint64)
    total = int(qlen.sum())
    out = np.full(total, 0 if extra is None else extra, np.uint8)
    ln = ln.astype(np.int64)
    within = np.arange(int(ln.sum()), dtype=np.int64) - np.repeat(np.cumsum(ln) - ln, ln)  # byte index inside its key
    out[np.repeat(qoff.astype(np.int64), ln) + within] = ikeys[np.repeat(off.astype(np.int64), ln) + within]
    return out, qoff, qlen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--entries", type=int, default=18_199_191)
    ap.add_argument("--runs", default="1,8")
    ap.add_argument("--nq", default="10,16,20")
    ap.add_argument("--host-calls", type=int, default=3)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    tk.set_device(0)
    lib = tk.load_library()
    rng = np.random.default_rng(1)
    n = args.entries
    run = sorted_run(rng.integers(4, 24, n).astype(np.uint32), rng.integers(0, 40, n).astype(np.uint32), dev)
    m = run.ikey_len.numel()
    st = VP(torch.cuda.current_stream().cuda_stream)
    h_ikeys, h_vals = run.ikeys.cpu().numpy(), run.vals.cpu().numpy()
    h_off = run.ikey_off.cpu().numpy().view(np.uint64)
    h_len = run.ikey_len.cpu().numpy().view(np.uint32)
    p = lambda t: VP(t.data_ptr()) if t is not None and t.numel() else None  # noqa: E731
    hp = lambda a: VP(a.ctypes.data) if a is not None and a.size else None  # noqa: E731
    for k in (int(x) for x in args.runs.split(",")):
        runs = deal(run, k)
        host = lambda t, dt: np.ascontiguousarray(t.cpu().numpy().view(dt))  # noqa: E731
        hruns = [(h_ikeys, host(r[1], np.uint64), host(r[2], np.uint32), h_vals, host(r[4], np.uint64), host(r[5], np.uint32))
                 for r in runs]

        def tables(rs, addr, count):
            arr = lambda vals: (VP * k)(*vals)  # noqa: E731
            return ([arr([addr(r[0]) for r in rs]), (U64 * k)(*[count(r[0]) for r in rs])] +
                    [arr([addr(r[c]) for r in rs]) for c in (1, 2, 4, 5)] + [(U64 * k)(*[count(r[2]) for r in rs])],
                    arr([addr(r[3]) for r in rs]), (U64 * k)(*[count(r[3]) for r in rs]), (U64 * k)(*[0] * k))
        d_run, d_vals, d_vsize, bias = tables(runs, lambda t: t.data_ptr(), lambda t: t.numel())
        h_run, hv, hvsize, _ = tables(hruns, lambda a: a.ctypes.data, lambda a: a.size)

        # yardstick 2: one merge of the same runs
        cols = [torch.empty(m, dtype=dt, device=dev) for dt in (torch.int64, torch.int32, torch.int64, torch.int32, torch.int64)]

        def merge():
            out = [U64(0) for _ in range(4)]
            rc = lib.tkv_sst_merge_device(k, *d_run, VP(run.ikeys.data_ptr()), bias, 0, *[p(c) for c in cols], m,
                                          *[ctypes.byref(o) for o in out], st)
            return rc, out[0].value
        t_merge = []
        for r in range(args.warmup + 5):
            ms, got = timed(merge)
            assert got == (0, m), got
            if r >= args.warmup:
                t_merge.append(ms)
        del cols
        torch.cuda.empty_cache()

        for e in (int(x) for x in args.nq.split(",")):
            nq = 1 << e
            pick = rng.integers(0, m, nq)
            kinds = {
                "present": gather_keys(h_ikeys, h_off[pick], h_len[pick] - 17),
                "absent": gather_keys(h_ikeys, h_off[pick], h_len[pick] - 17, extra=0x5A),
                "hot": gather_keys(h_ikeys, np.repeat(h_off[pick[:1]], nq), np.repeat(h_len[pick[:1]] - 17, nq)),
            }
            for kind, (qa, qo, ql) in kinds.items():
                dq = (torch.from_numpy(qa).to(dev), torch.from_numpy(qo.view(np.int64)).to(dev), torch.from_numpy(ql.view(np.int32)).to(dev))
                outs = [torch.empty(nq, dtype=dt, device=dev) for dt in (torch.uint8, torch.int64, torch.int64, torch.int64, torch.int32,
                                                                            torch.int64)]
                res = [U64(0) for _ in range(3)]
                refs = [ctypes.byref(r) for r in res]
                rc = lib.tkv_sst_get_device(k, *d_run, d_vals, d_vsize, bias, p(dq[0]), dq[0].numel(), p(dq[1]), p(dq[2]), nq, 0,
                                            *[None] * 7, 0, *refs, st)
                assert rc == 0, rc
                found, total = res[0].value, res[1].value
                # (a present key with a byte appended can itself be present: a handful in 2^20 draws; the host
                # call below is held to the same states)
                assert (found < 8) if kind == "absent" else (found == nq), (kind, found)
                vals = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
                for gather in (True, False):
                    def get():
                        o = [p(t) for t in outs]
                        if not gather:
                            o[5] = None
                        rc = lib.tkv_sst_get_device(k, *d_run, d_vals if gather else None, d_vsize if gather else None, bias, p(dq[0]),
                                                    dq[0].numel(), p(dq[1]), p(dq[2]), nq, 0, *o, p(vals) if gather else None,
                                                    total if gather else 0, *refs, st)
                        ms = (ctypes.c_double * 4)()
                        lib.tkv_debug_sst_get_phases(1, ms)
                        return rc, res[0].value, res[1].value, list(ms)
                    lib.tkv_debug_sst_get_phases(1, None)
                    times, phases = [], {q: [] for q in PHASES}
                    for r in range(args.warmup + args.k):
                        ms, got = timed(get)
                        assert got[:3] == (0, found, total), got
                        if r >= args.warmup:
                            times.append(ms)
                            for q, v in zip(PHASES, got[3]):
                                phases[q].append(v)
                    lib.tkv_debug_sst_get_phases(0, None)
                    last = np.zeros(5, np.uint64)
                    lib.tkv_debug_sst_get_last(VP(last.ctypes.data))
                    med = float(np.median(times))
                    line = {"runs": k, "entries": m, "queries": kind, "nq": nq, "gather": gather, "found": found,
                            "vals_bytes": total, "steps": int(last[2]), "k": args.k, "get_ms": round(med, 4),
                            "get_min_max_ms": [round(min(times), 4), round(max(times), 4)],
                            "get_Mqueries_per_s": round(nq / med / 1e3, 2)}
                    for q in PHASES:
                        line["phase_" + q + "_ms"] = round(float(np.median(phases[q])), 4)
                    line["merge_ms"] = round(float(np.median(t_merge)), 4)
                    line["merge_over_get_time"] = round(float(np.median(t_merge)) / med, 1)
                    if gather:
                        # yardstick 1: the host call on the host's threads
                        ho = [np.empty(nq, dt) for dt in (np.uint8, np.uint64, np.uint64, np.uint64, np.uint32, np.uint64)]
                        hvals = np.empty(max(total, 1), np.uint8)
                        wall = []
                        for _ in range(args.host_calls):
                            t0 = time.perf_counter()
                            rc = lib.tkv_sst_get(k, *h_run, hv, hvsize, bias, hp(qa), qa.size, hp(qo), hp(ql), nq, 0, *[hp(a) for a in ho],
                                                 hp(hvals), total, *refs)
                            wall.append((time.perf_counter() - t0) * 1e3)
                            assert rc == 0 and (res[0].value, res[1].value) == (found, total)
                        assert np.array_equal(ho[0], outs[0].cpu().numpy()) and np.array_equal(ho[1], outs[1].cpu().numpy().view(np.uint64))
                        assert np.array_equal(hvals[:total], vals[:total].cpu().numpy())
                        line["host_ms"] = round(float(np.median(wall)), 3)
                        line["host_min_max_ms"] = [round(min(wall), 3), round(max(wall), 3)]
                        line["host_over_get_time"] = round(float(np.median(wall)) / med, 1)
                    print(json.dumps(line), flush=True)
                del dq, outs, vals
        del runs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
