#!/usr/bin/env python3
"""Time of the device memtable replay (not product code): the batches decoded from the two WAL images
DESIGN.md §6.3 uses (1 GiB of small records: keys 4-23 B, values 0-39 B, 59 B a record; about 430 MB of
Zipf values), as tkv_wal_decode_device returns them (copied arenas). After untimed warm-ups, K warm calls
per leg, in one process, in rotation, each between a pair of device events on the calls' stream:
  replay   tkv_memtable_build_device of the batch, with its phase times (check and first round, later
           rounds, dedupe, emit) from tkv_debug_memtable_phases
  decode   tkv_wal_decode_device that produced the batch: the stage in front
  flush    tkv_sst_build_device of the run, target_block_size 4096: the stage behind
and, --host-k times (wall clock; it uses no GPU), tkv_memtable_build of the same batch on the host's
threads. Prints one JSON line per shape: median and min-max times, records per second, replay / decode and
replay / flush. The run is checked against the host variant byte for byte.

    python tools/memtable_probe.py [--k 10] [--warmup 2] [--host-k 1]
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
from tinykvpp_amd import memtable, sst  # noqa: E402

VP, U64 = ctypes.c_void_p, ctypes.c_uint64
PHASES = ("first_round", "refine", "dedupe", "emit")


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-k", type=int, default=1)
    ap.add_argument("--small-records", type=int, default=18_199_191, help="records of the small-record image (1 GiB)")
    ap.add_argument("--zipf-records", type=int, default=400_000)
    ap.add_argument("--images", default="small,zipf")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    tk.set_device(0)
    lib = tk.load_library()
    rng = np.random.default_rng(1)
    n = args.small_records
    shapes = [("small records 1 GiB", rng.integers(4, 24, n).astype(np.uint32), rng.integers(0, 40, n).astype(np.uint32))]
    n2 = args.zipf_records
    zv = np.minimum(rng.zipf(1.6, n2) * 64, 16_000).astype(np.uint32)
    zv[-1] = 16
    shapes.append(("zipf 430 MB", rng.integers(8, 64, n2).astype(np.uint32), zv))
    st = VP(torch.cuda.current_stream().cuda_stream)
    p = lambda t: VP(t.data_ptr()) if t.numel() else None  # noqa: E731
    for name, klen, vlen in shapes:
        if name.split()[0] not in args.images.split(","):
            continue
        n = klen.size
        keys, koff = arena(klen, dev)
        vals, voff = arena(vlen, dev)
        img, rec_off, _ = tk.wal.encode_device(keys, koff, torch.from_numpy(klen.view(np.int32)).to(dev), vals, voff,
                                               torch.from_numpy(vlen.view(np.int32)).to(dev), first_seq=1)
        del keys, vals, koff, voff
        b = tk.wal.decode_device(img, rec_off)
        run = memtable.build_device(b, timestamp_ms=7)
        m, isize = run.ikey_len.numel(), run.ikeys.numel()
        table = run.flush()
        torch.cuda.synchronize()

        def replay():
            out = [U64(0) for _ in range(3)]
            rc = lib.tkv_memtable_build_device(p(b.keys), b.keys.numel(), p(b.key_off), p(b.key_len), p(b.val_off),
                                               p(b.val_len), p(b.op), p(b.tomb), p(b.seq), n, 7, p(run.ikeys), isize,
                                               p(run.ikey_off), p(run.ikey_len), p(run.val_off), p(run.val_len), p(run.src), m,
                                               *[ctypes.byref(o) for o in out], st)
            ms = (ctypes.c_double * 4)()
            lib.tkv_debug_memtable_phases(1, ms)
            return rc, out[0].value, list(ms)

        def decode():
            out = [U64(0) for _ in range(3)]
            return lib.tkv_wal_decode_device(p(img), img.numel(), p(rec_off), None, n, 0, p(b.op), p(b.tomb), p(b.seq),
                                             p(b.key_off), p(b.key_len), p(b.val_off), p(b.val_len), p(b.keys), b.keys.numel(),
                                             p(b.vals), b.vals.numel(), *[ctypes.byref(o) for o in out], st)

        def flush():
            sizes = [U64(0) for _ in range(4)]
            return lib.tkv_sst_build_device(p(run.ikeys), p(run.ikey_off), p(run.ikey_len), p(run.vals), p(run.val_off),
                                            p(run.val_len), m, 4096, p(table.file), table.size, p(table.block_off),
                                            p(table.block_size), p(table.block_first), table.n_blocks,
                                            *[ctypes.byref(s) for s in sizes], st)

        lib.tkv_debug_memtable_phases(1, None)
        legs = [("replay", replay), ("decode", decode), ("flush", flush)]
        times = {k: [] for k, _ in legs}
        phases = {k: [] for k in PHASES}
        out = {}
        for r in range(args.warmup + args.k):
            order = legs[r % len(legs):] + legs[:r % len(legs)]
            for k, fn in order:
                ms, out[k] = timed(fn)
                if r >= args.warmup:
                    times[k].append(ms)
                    if k == "replay":
                        for ph, v in zip(PHASES, out[k][2]):
                            phases[ph].append(v)
        lib.tkv_debug_memtable_phases(0, None)
        assert out["replay"][:2] == (0, m) and out["decode"] == 0 and out["flush"] == 0, out
        last = np.zeros(4, np.uint64)
        lib.tkv_debug_memtable_last(VP(last.ctypes.data))
        # the host variant: the same batch on host threads, and the check of the device run against it
        h = [t.cpu().numpy() for t in b]
        host_s = []
        for _ in range(max(1, args.host_k)):
            t0 = time.perf_counter()
            hrun = memtable.build_host_columns(h[7], h[3].view(np.uint64), h[4].view(np.uint32), h[5].view(np.uint64),
                                               h[6].view(np.uint32), h[0], h[1], h[2].view(np.uint64), timestamp_ms=7)
            host_s.append(time.perf_counter() - t0)
        assert np.array_equal(hrun.src, run.src.cpu().numpy().view(np.uint32)), "the device run differs from the host's"
        assert np.array_equal(hrun.ikeys, run.ikeys.cpu().numpy()), "the device internal keys differ from the host's"
        med = {k: float(np.median(v)) for k, v in times.items()}
        pmed = {k: float(np.median(v)) for k, v in phases.items()}
        line = {"shape": name, "records": n, "entries": m, "ikey_bytes": isize, "rounds": int(last[1]),
                "second_round_records": int(last[2]), "scratch_bytes": int(last[3]), "k": args.k}
        for k in times:
            line[k + "_ms"] = round(med[k], 4)
            line[k + "_min_max_ms"] = [round(min(times[k]), 4), round(max(times[k]), 4)]
        for k in PHASES:
            line["phase_" + k + "_ms"] = round(pmed[k], 4)
        line["replay_Mrec_per_s"] = round(n / med["replay"] / 1e3, 1)
        line["replay_over_decode_time"] = round(med["replay"] / med["decode"], 2)
        line["replay_over_flush_time"] = round(med["replay"] / med["flush"], 2)
        line["host_ms"] = round(float(np.median(host_s)) * 1e3, 1)
        line["host_over_replay_time"] = round(line["host_ms"] / med["replay"], 1)
        print(json.dumps(line), flush=True)
        del b, img, run, table, h, hrun
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
