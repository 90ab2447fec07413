#!/usr/bin/env python3
"""Rate of the device SSTable scan (not product code): the two standing shapes of tools/sst_build_probe.py
(18.2 M small entries: keys 4-23 B, values 0-39 B, a 758 MB file; 400 K entries with Zipf values), each
flushed by tkv_sst_build_device with target_block_size 4096 and scanned back. After untimed warm-ups, K
warm calls per leg, in one process, in rotation, each between a pair of device events on the calls'
stream:
  scan_copy   tkv_sst_scan_device with copied arenas, with its phase times (open, checksum, parse, emit)
              from tkv_debug_sst_scan_phases
  scan_views  tkv_sst_scan_device with both views flags
  build       tkv_sst_build_device of the same entries: the yardstick, the same bytes the other way
  block_crcs  tkv_sst_block_crcs_device over the file's blocks: what the checksum phase should cost
Prints one JSON line per shape: median and min-max times, file GB/s, scan / build, views / copy and
checksum / block_crcs. The scanned columns are compared with the flush's inputs.

    python tools/sst_scan_probe.py [--k 20] [--warmup 3]
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
from tinykvpp_amd import sst  # noqa: E402

VP, U64 = ctypes.c_void_p, ctypes.c_uint64
PHASES = ("open", "checksum", "parse", "emit")


def timed(fn):
    """Milliseconds between device events around one synchronous call on the current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def arena(lens, dev):
    """Random bytes for spans of `lens` bytes back to back: (arena, offsets)."""
    off = np.zeros(lens.size, np.int64)
    off[1:] = np.cumsum(lens[:-1].astype(np.int64))
    data = torch.randint(0, 256, (int(lens.sum()) + 16,), dtype=torch.uint8, device=dev)
    return data, torch.from_numpy(off).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small-records", type=int, default=18_199_191)
    ap.add_argument("--zipf-records", type=int, default=400_000)
    ap.add_argument("--target", type=int, default=4096)
    ap.add_argument("--images", default="small,zipf")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    tk.set_device(0)
    lib = tk.load_library()
    rng = np.random.default_rng(1)
    n = args.small_records
    shapes = [("small entries", rng.integers(4, 24, n).astype(np.uint32), rng.integers(0, 40, n).astype(np.uint32))]
    n2 = args.zipf_records
    zv = np.minimum(rng.zipf(1.6, n2) * 64, 16_000).astype(np.uint32)
    zv[-1] = 16
    shapes.append(("zipf values", rng.integers(8, 64, n2).astype(np.uint32), zv))
    st = VP(torch.cuda.current_stream().cuda_stream)
    for name, klen, vlen in shapes:
        if name.split()[0] not in args.images.split(","):
            continue
        n = klen.size
        keys, koff = arena(klen, dev)
        vals, voff = arena(vlen, dev)
        kl_t, vl_t = torch.from_numpy(klen.view(np.int32)).to(dev), torch.from_numpy(vlen.view(np.int32)).to(dev)
        res = sst.build_device(keys, koff, kl_t, vals, voff, vl_t, target_block_size=args.target)
        file, total, B = res.file, res.size, res.n_blocks
        ks, vs = int(klen.sum(dtype=np.uint64)), int(vlen.sum(dtype=np.uint64))
        o_koff, o_voff = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
        o_klen, o_vlen = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        o_keys, o_vals = torch.empty(ks + 16, dtype=torch.uint8, device=dev), torch.empty(vs + 16, dtype=torch.uint8, device=dev)
        o_boff = torch.empty(B, dtype=torch.int64, device=dev)
        o_bsize, o_bfirst = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
        file2 = torch.empty(total, dtype=torch.uint8, device=dev)
        crcs = torch.empty(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        p = lambda t: VP(t.data_ptr())  # noqa: E731

        def scan(flags):
            out = [U64(0) for _ in range(5)]
            rc = lib.tkv_sst_scan_device(p(file), total, flags, p(o_koff), p(o_klen), p(o_voff), p(o_vlen), n, p(o_keys), ks,
                                         p(o_vals), vs, p(o_boff), p(o_bsize), p(o_bfirst), B,
                                         *[ctypes.byref(s) for s in out], st)
            ms = (ctypes.c_double * 4)()
            lib.tkv_debug_sst_scan_phases(1, ms)
            return rc, tuple(s.value for s in out), list(ms)

        def build():
            sizes = [U64(0) for _ in range(4)]
            rc = lib.tkv_sst_build_device(p(keys), p(koff), p(kl_t), p(vals), p(voff), p(vl_t), n, args.target, p(file2),
                                          total, p(res.block_off), p(res.block_size), p(res.block_first), B,
                                          *[ctypes.byref(s) for s in sizes], st)
            return rc, sizes[0].value

        def block_crcs():
            rc = lib.tkv_sst_block_crcs_device(p(file), p(res.block_off), p(res.block_size), p(crcs), B, 0, st)
            torch.cuda.current_stream().synchronize()
            return rc

        lib.tkv_debug_sst_scan_phases(1, None)
        legs = [("scan_copy", lambda: scan(0)), ("scan_views", lambda: scan(3)), ("build", build), ("block_crcs", block_crcs)]
        times = {k: [] for k, _ in legs}
        phases = {k: [] for k in PHASES}
        out = {}
        for r in range(args.warmup + args.k):
            order = legs[r % len(legs):] + legs[:r % len(legs)]
            for k, fn in order:
                ms, out[k] = timed(fn)
                if k == "scan_copy" and r == 0:  # what the copied scan wrote against the flush's inputs
                    assert out[k][:2] == (0, (n, B, ks, vs, B)), out[k]
                    assert torch.equal(o_klen, kl_t) and torch.equal(o_vlen, vl_t) and torch.equal(o_koff, koff)
                    assert torch.equal(o_keys[:ks], keys[:ks]) and torch.equal(o_vals[:vs], vals[:vs])
                    assert torch.equal(o_boff, res.block_off) and torch.equal(o_bfirst, res.block_first)
                if r >= args.warmup:
                    times[k].append(ms)
                    if k == "scan_copy":
                        for ph, v in zip(PHASES, out[k][2]):
                            phases[ph].append(v)
        lib.tkv_debug_sst_scan_phases(0, None)
        assert out["scan_views"][:2] == (0, (n, B, ks, vs, B)) and out["build"] == (0, total) and out["block_crcs"] == 0, out
        last = np.zeros(4, np.uint64)
        lib.tkv_debug_sst_scan_last(VP(last.ctypes.data))
        med = {k: float(np.median(v)) for k, v in times.items()}
        pmed = {k: float(np.median(v)) for k, v in phases.items()}
        line = {"shape": name, "entries": n, "file_bytes": total, "blocks": B, "index_rounds": int(last[1]),
                "parse_waves": int(last[2]), "k": args.k}
        for k in times:
            line[k + "_ms"] = round(med[k], 4)
            line[k + "_min_max_ms"] = [round(min(times[k]), 4), round(max(times[k]), 4)]
        line["scan_copy_GB_per_s"] = round(total / med["scan_copy"] / 1e6, 1)
        line["build_GB_per_s"] = round(total / med["build"] / 1e6, 1)
        for k in PHASES:
            line["phase_" + k + "_ms"] = round(pmed[k], 4)
            line["phase_" + k + "_min_max_ms"] = [round(min(phases[k]), 4), round(max(phases[k]), 4)]
        line["scan_copy_over_build_time"] = round(med["scan_copy"] / med["build"], 3)
        line["scan_views_over_scan_copy_time"] = round(med["scan_views"] / med["scan_copy"], 3)
        line["checksum_over_block_crcs_time"] = round(pmed["checksum"] / med["block_crcs"], 3)
        print(json.dumps(line), flush=True)
        del keys, vals, koff, voff, file, file2, res, crcs, o_keys, o_vals, o_koff, o_voff, o_klen, o_vlen
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
