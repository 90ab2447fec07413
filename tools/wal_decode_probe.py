#!/usr/bin/env python3
"""Rate of the device WAL decode (not product code), on the two images DESIGN.md §6.3 uses (1 GiB of small
records: keys 4-23 B, values 0-39 B; about 430 MB of Zipf values), produced in HBM by tkv_wal_encode_device,
with the record offsets that call returns (what tkv_wal_index_device lists). After untimed warm-ups, K
warm calls per leg, in one process, in rotation, each between a pair of device events on the calls' stream:
  copied   tkv_wal_decode_device with copied key and value arenas
  views    the same with both arenas as views (the header pass, the scans and the columns only)
  encode   tkv_wal_encode_device of the decoded batch (copied arenas): the yardstick. The copied decode
           reads the image once and writes about the bytes the encode reads, and folds no CRC.
  copy     a device-to-device copy of the image, for scale
Prints one JSON line per image: median and min-max times, image GB/s per leg and copied / encode (the
times' ratio). The re-encoded image must equal the image decoded.

    python tools/wal_decode_probe.py [--k 20] [--warmup 3]
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
from tools.wal_encode_probe import arena, timed  # noqa: E402

VP, U64 = ctypes.c_void_p, ctypes.c_uint64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small-records", type=int, default=18_199_191, help="records of the small-record image (1 GiB)")
    ap.add_argument("--zipf-records", type=int, default=400_000)
    ap.add_argument("--images", default="small,zipf", help="which images to run (a kernel trace takes one at a time)")
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
    zv[-1] = 16  # a short final record
    shapes.append(("zipf 430 MB", rng.integers(8, 64, n2).astype(np.uint32), zv))
    st = VP(torch.cuda.current_stream().cuda_stream)
    for name, klen, vlen in shapes:
        if name.split()[0] not in args.images.split(","):
            continue
        n = klen.size
        keys, koff = arena(klen, dev)
        vals, voff = arena(vlen, dev)
        total = int(klen.sum(dtype=np.uint64) + vlen.sum(dtype=np.uint64)) + 26 * n
        img, rec_off, _ = tk.wal.encode_device(keys, koff, torch.from_numpy(klen.view(np.int32)).to(dev), vals, voff,
                                               torch.from_numpy(vlen.view(np.int32)).to(dev), first_seq=1)
        assert img.numel() == total
        del keys, vals, koff, voff
        ksz, vsz = int(klen.sum(dtype=np.uint64)), int(vlen.sum(dtype=np.uint64))
        cols = [torch.empty(n, dtype=dt, device=dev) for dt in (torch.uint8, torch.uint8, torch.int64, torch.int64,
                                                                torch.int32, torch.int64, torch.int32)]
        dkeys = torch.empty(ksz, dtype=torch.uint8, device=dev)
        dvals = torch.empty(vsz, dtype=torch.uint8, device=dev)
        other = torch.empty(total, dtype=torch.uint8, device=dev)
        off2 = torch.empty(n, dtype=torch.int64, device=dev)
        crc = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def decode(flags):
            ks, vs, fb = U64(0), U64(0), U64(0)
            rc = lib.tkv_wal_decode_device(VP(img.data_ptr()), total, VP(rec_off.data_ptr()), None, n, flags,
                                           *[VP(c.data_ptr()) for c in cols], VP(dkeys.data_ptr()), ksz,
                                           VP(dvals.data_ptr()), vsz, ctypes.byref(ks), ctypes.byref(vs), ctypes.byref(fb), st)
            last = np.zeros(4, np.uint64)
            lib.tkv_debug_wal_decode_last(VP(last.ctypes.data))
            return rc, ks.value, vs.value, fb.value, int(last[0]), int(last[1])

        def encode():
            size = U64(0)
            op, tomb, seq, ko, kl, vo, vl = cols
            rc = lib.tkv_wal_encode_device(VP(dkeys.data_ptr()), VP(ko.data_ptr()), VP(kl.data_ptr()), VP(dvals.data_ptr()),
                                           VP(vo.data_ptr()), VP(vl.data_ptr()), VP(op.data_ptr()), VP(tomb.data_ptr()),
                                           VP(seq.data_ptr()), 0, n, VP(other.data_ptr()), total, VP(off2.data_ptr()),
                                           VP(crc.data_ptr()), ctypes.byref(size), st)
            return rc, size.value

        def copy():
            other.copy_(img)
            torch.cuda.current_stream().synchronize()

        # `encode` reads the columns of a copied decode: that leg runs right after `copied` in every rotation
        legs = [("views", lambda: decode(3)), ("copied", lambda: decode(0)), ("encode", encode), ("copy", copy)]
        times = {k: [] for k, _ in legs}
        res = {}
        for r in range(args.warmup + args.k):
            for k, fn in legs:
                ms, res[k] = timed(fn)
                if r >= args.warmup:
                    times[k].append(ms)
        assert res["copied"][:4] == (0, ksz, vsz, n) and res["views"][:4] == (0, ksz, vsz, n), res
        assert res["views"][4:] == (0, 0) and res["encode"] == (0, total), res
        decode(0)
        encode()
        assert torch.equal(img, other) and torch.equal(off2, rec_off), "the re-encoded image differs"
        med = {k: float(np.median(v)) for k, v in times.items()}
        line = {"image": name, "bytes": total, "records": n, "k": args.k, "key_bytes": ksz, "value_bytes": vsz,
                "key_emit_waves": res["copied"][4], "value_emit_waves": res["copied"][5]}
        for k in times:
            line[k + "_ms"] = round(med[k], 4)
            line[k + "_GB_per_s"] = round(total / med[k] / 1e6, 1)
            line[k + "_min_max_ms"] = [round(min(times[k]), 4), round(max(times[k]), 4)]
        line["copied_over_encode_time"] = round(med["copied"] / med["encode"], 3)
        line["views_over_copied_time"] = round(med["views"] / med["copied"], 3)
        print(json.dumps(line), flush=True)
        del img, other, dkeys, dvals, cols, rec_off, off2, crc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
