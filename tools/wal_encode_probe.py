#!/usr/bin/env python3
"""Rate of the device WAL encode (not product code): batches that encode to the two images DESIGN.md §6.3
uses (1 GiB of small records: keys 4-23 B, values 0-39 B; about 430 MB of Zipf values), held in HBM as key /
value arenas. After untimed warm-ups, K warm calls per leg, in one process, in rotation, each between a pair
of device events on the calls' stream:
  fused     tkv_wal_encode_device as shipped (records of record_len <= 240 stamped inside the emit pass)
  unfused   the same with tkv_debug_set_wal_encode_fused(0): the emit, then one CRC batch that reads the
            written image back, then the field stores (the two-pass route the fusion replaces)
  copy      a device-to-device copy of img_size bytes (the traffic floor: an encode reads and writes what a
            copy does, plus 16-20 bytes of arrays per record)
  verify    tkv_wal_verify_device of the produced image, for scale
Prints one JSON line per image: median and min-max times, image GB/s per leg, fused / unfused and fused /
copy. The fused and unfused images are compared, and the verify must accept every record.

    python tools/wal_encode_probe.py [--k 20] [--warmup 3]
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

VP, U64 = ctypes.c_void_p, ctypes.c_uint64


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
        kl = torch.from_numpy(klen.view(np.int32)).to(dev)
        vl = torch.from_numpy(vlen.view(np.int32)).to(dev)
        total = int(klen.sum(dtype=np.uint64) + vlen.sum(dtype=np.uint64)) + 26 * n
        img = torch.empty(total, dtype=torch.uint8, device=dev)
        other = torch.empty(total, dtype=torch.uint8, device=dev)
        rec_off = torch.empty(n, dtype=torch.int64, device=dev)
        crc = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def encode(dst, fused):
            prev = lib.tkv_debug_set_wal_encode_fused(fused)
            try:
                size = U64(0)
                rc = lib.tkv_wal_encode_device(VP(keys.data_ptr()), VP(koff.data_ptr()), VP(kl.data_ptr()),
                                               VP(vals.data_ptr()), VP(voff.data_ptr()), VP(vl.data_ptr()), None, None,
                                               None, 1, n, VP(dst.data_ptr()), total, VP(rec_off.data_ptr()),
                                               VP(crc.data_ptr()), ctypes.byref(size), st)
                last = np.zeros(4, np.uint64)
                lib.tkv_debug_wal_encode_last(VP(last.ctypes.data))
                return rc, size.value, int(last[0]), int(last[1])
            finally:
                lib.tkv_debug_set_wal_encode_fused(prev)

        def verify():
            good, stop = U64(0), U64(0)
            rc = lib.tkv_wal_verify_device(VP(img.data_ptr()), total, ctypes.byref(good), ctypes.byref(stop), st)
            return rc, good.value, stop.value

        def copy():
            other.copy_(img)
            torch.cuda.current_stream().synchronize()

        assert encode(img, 1)[:2] == (0, total)  # the image the copy and the verify legs read
        legs = [("fused", lambda: encode(img, 1)), ("unfused", lambda: encode(other, 0)), ("copy", copy), ("verify", verify)]
        times = {k: [] for k, _ in legs}
        res = {}
        for r in range(args.warmup + args.k):
            order = legs[r % len(legs):] + legs[:r % len(legs)]
            for k, fn in order:
                ms, res[k] = timed(fn)
                if r >= args.warmup:
                    times[k].append(ms)
        assert res["fused"][:2] == (0, total) and res["unfused"][:3] == (0, total, 0), res
        assert res["verify"] == (0, n, total), res
        encode(other, 0)
        assert torch.equal(img, other), "fused and unfused images differ"
        med = {k: float(np.median(v)) for k, v in times.items()}
        line = {"image": name, "bytes": total, "records": n, "k": args.k,
                "fused_in_emit": res["fused"][2], "fused_read_back": res["fused"][3]}
        for k in times:
            line[k + "_ms"] = round(med[k], 4)
            line[k + "_GB_per_s"] = round(total / med[k] / 1e6, 1)
            line[k + "_min_max_ms"] = [round(min(times[k]), 4), round(max(times[k]), 4)]
        line["fused_over_unfused_rate"] = round(med["unfused"] / med["fused"], 3)
        line["fused_over_copy_rate"] = round(med["copy"] / med["fused"], 3)
        print(json.dumps(line), flush=True)
        del keys, vals, koff, voff, kl, vl, img, other, rec_off, crc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
