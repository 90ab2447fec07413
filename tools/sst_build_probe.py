#!/usr/bin/env python3
"""Rate of the device SSTable flush (not product code): the arenas of the two WAL images DESIGN.md §6.3
uses (1 GiB of small records: keys 4-23 B, values 0-39 B, 59 B a record; about 430 MB of Zipf values),
as tkv_wal_decode_device returns them (copied arenas, keys and values back to back). After untimed
warm-ups, K warm calls per leg, in one process, in rotation, each between a pair of device events on the
calls' stream:
  build       tkv_sst_build_device, target_block_size 4096, with its phase times (size scans, block cut,
              emit, stamp) from tkv_debug_sst_build_phases
  encode      tkv_wal_encode_device of the same arenas: the yardstick, the same payload through the same
              scan, tile and window machinery
  block_crcs  tkv_sst_block_crcs_device over the finished file's blocks: what the stamp phase should cost
Prints one JSON line per shape: median and min-max times, file GB/s, emit / encode and stamp / block_crcs.
The built file is verified block by block on the device and through its index and footer on the host.

    python tools/sst_build_probe.py [--k 20] [--warmup 3]
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
PHASES = ("scan", "cut", "emit", "stamp")


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
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small-records", type=int, default=18_199_191, help="records of the small-record image (1 GiB)")
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
    shapes = [("small records 1 GiB", rng.integers(4, 24, n).astype(np.uint32), rng.integers(0, 40, n).astype(np.uint32))]
    n2 = args.zipf_records
    zv = np.minimum(rng.zipf(1.6, n2) * 64, 16_000).astype(np.uint32)
    zv[-1] = 16
    shapes.append(("zipf 430 MB", rng.integers(8, 64, n2).astype(np.uint32), zv))
    st = VP(torch.cuda.current_stream().cuda_stream)
    for name, klen, vlen in shapes:
        if name.split()[0] not in args.images.split(","):
            continue
        n = klen.size
        keys, koff = arena(klen, dev)
        vals, voff = arena(vlen, dev)
        wal_total = int(klen.sum(dtype=np.uint64) + vlen.sum(dtype=np.uint64)) + 26 * n
        img, rec_off, _ = tk.wal.encode_device(keys, koff, torch.from_numpy(klen.view(np.int32)).to(dev), vals, voff,
                                               torch.from_numpy(vlen.view(np.int32)).to(dev), first_seq=1)
        del keys, vals, koff, voff
        b = tk.wal.decode_device(img, rec_off)  # the arenas a recovery holds
        del rec_off
        res = sst.build_device(b.keys, b.key_off, b.key_len, b.vals, b.val_off, b.val_len, target_block_size=args.target)
        file, total, B = res.file, res.size, res.n_blocks
        crcs = torch.empty(B, dtype=torch.int32, device=dev)
        off2 = torch.empty(n, dtype=torch.int64, device=dev)
        crc2 = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        p = lambda t: VP(t.data_ptr())  # noqa: E731

        def build():
            sizes = [U64(0) for _ in range(4)]
            rc = lib.tkv_sst_build_device(p(b.keys), p(b.key_off), p(b.key_len), p(b.vals), p(b.val_off), p(b.val_len), n,
                                          args.target, p(file), total, p(res.block_off), p(res.block_size),
                                          p(res.block_first), B, *[ctypes.byref(s) for s in sizes], st)
            ms = (ctypes.c_double * 4)()
            lib.tkv_debug_sst_build_phases(1, ms)
            return rc, sizes[0].value, list(ms)

        def encode():
            size = U64(0)
            rc = lib.tkv_wal_encode_device(p(b.keys), p(b.key_off), p(b.key_len), p(b.vals), p(b.val_off), p(b.val_len),
                                           p(b.op), p(b.tomb), p(b.seq), 0, n, p(img), wal_total, p(off2), p(crc2),
                                           ctypes.byref(size), st)
            return rc, size.value

        def block_crcs():
            rc = lib.tkv_sst_block_crcs_device(p(file), p(res.block_off), p(res.block_size), p(crcs), B, 0, st)
            torch.cuda.current_stream().synchronize()
            return rc

        lib.tkv_debug_sst_build_phases(1, None)
        legs = [("build", build), ("encode", encode), ("block_crcs", block_crcs)]
        times = {k: [] for k, _ in legs}
        phases = {k: [] for k in PHASES}
        out = {}
        for r in range(args.warmup + args.k):
            order = legs[r % len(legs):] + legs[:r % len(legs)]
            for k, fn in order:
                ms, out[k] = timed(fn)
                if r >= args.warmup:
                    times[k].append(ms)
                    if k == "build":
                        for ph, v in zip(PHASES, out[k][2]):
                            phases[ph].append(v)
        lib.tkv_debug_sst_build_phases(0, None)
        assert out["build"][:2] == (0, total) and out["encode"] == (0, wal_total) and out["block_crcs"] == 0, out
        # the finished file: every block's stored stamp is its CRC, and the index and footer open on the host
        stored = torch.stack([file[res.block_off + 17 + k].to(torch.int64) << (8 * k) for k in range(4)]).sum(0)
        assert torch.equal(stored, crcs.to(torch.int64) & 0xFFFFFFFF), "a stored block stamp differs from its CRC"
        tail = file[res.index_offset:].cpu().numpy().tobytes()
        assert sst.verify_footer(tail[:-20], tail[-20:]) == "ok"
        last = np.zeros(4, np.uint64)
        lib.tkv_debug_sst_build_last(VP(last.ctypes.data))
        med = {k: float(np.median(v)) for k, v in times.items()}
        pmed = {k: float(np.median(v)) for k, v in phases.items()}
        line = {"shape": name, "entries": n, "file_bytes": total, "wal_bytes": wal_total, "blocks": B,
                "rounds": int(last[1]), "emit_waves": int(last[2]), "k": args.k}
        for k in times:
            line[k + "_ms"] = round(med[k], 4)
            line[k + "_min_max_ms"] = [round(min(times[k]), 4), round(max(times[k]), 4)]
        line["build_GB_per_s"] = round(total / med["build"] / 1e6, 1)
        line["encode_GB_per_s"] = round(wal_total / med["encode"] / 1e6, 1)
        for k in PHASES:
            line["phase_" + k + "_ms"] = round(pmed[k], 4)
            line["phase_" + k + "_min_max_ms"] = [round(min(phases[k]), 4), round(max(phases[k]), 4)]
        line["emit_over_encode_time"] = round(pmed["emit"] / med["encode"], 3)
        line["cut_over_emit_time"] = round(pmed["cut"] / pmed["emit"], 3)
        line["stamp_over_block_crcs_time"] = round(pmed["stamp"] / med["block_crcs"], 3)
        print(json.dumps(line), flush=True)
        del b, img, file, res, crcs, off2, crc2
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
