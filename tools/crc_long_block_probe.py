#!/usr/bin/env python3
"""How fast a few long blocks go through the irregular batch engine, the uniform batch and the single-span
update (not product code): n blocks of L bytes at a byte shift, each entry point warmed once and timed as
--k calls between one pair of device events, the three entry points in rotation over --rounds rounds; the
median round is printed with the least and the largest. The salvage search reads its policy for long candidates off
this (tkv_wal_resync.hip, kRsLongLen). Prints one dict per shape.

    python tools/crc_long_block_probe.py [--k 3] [--rounds 5]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tinykvpp_amd as tk  # noqa: E402

VP = ctypes.c_void_p
SHAPES = ((1, 1 << 20, 5), (1, 16 << 20, 5), (1, 64 << 20, 5), (1, 64 << 20, 0), (4, 32 << 20, 5), (1, 200 << 20, 3),
          (64, 100_000, 3))


def timed(fn, k):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    lib = tk.load_library()
    tk.set_device(0)
    torch.cuda.set_device(0)
    buf = torch.randint(0, 256, ((256 << 20) + 64,), dtype=torch.uint8, device="cuda")
    outs = {k: torch.zeros(64, dtype=torch.int32, device="cuda") for k in ("irregular", "uniform", "update")}
    st = VP(torch.cuda.current_stream().cuda_stream)
    for n, L, shift in SHAPES:
        offs = torch.tensor([shift + i * L for i in range(n)], dtype=torch.int64, device="cuda")
        lens = torch.full((n,), L, dtype=torch.int32, device="cuda")
        legs = [
            ("irregular", lambda: lib.tkv_crc32_batch_device(VP(buf.data_ptr()), VP(offs.data_ptr()), VP(lens.data_ptr()), None,
                                                             VP(outs["irregular"].data_ptr()), n, st)),
            ("uniform", lambda: lib.tkv_crc32_batch_uniform_device(VP(buf.data_ptr() + shift), L, L, None,
                                                                   VP(outs["uniform"].data_ptr()), n, st)),
            ("update", lambda: lib.tkv_crc32_update_device(0xFFFFFFFF, VP(buf.data_ptr() + shift), L,
                                                           VP(outs["update"].data_ptr()), st))]
        for _, fn in legs:
            assert fn() == 0
        torch.cuda.synchronize()
        times = {k: [] for k, _ in legs}
        for r in range(args.rounds):
            for name, fn in legs[r % 3:] + legs[:r % 3]:
                times[name].append(timed(fn, args.k))
        line = dict(n=n, L=L, shift=shift, k=args.k, rounds=args.rounds)
        for name, v in times.items():
            line[name + "_ms"] = round(statistics.median(v), 4)
            line[name + "_min_max_ms"] = [round(min(v), 4), round(max(v), 4)]
        line["irregular_GBs"] = round(n * L / line["irregular_ms"] / 1e6, 1)
        line["uniform_GBs"] = round(n * L / line["uniform_ms"] / 1e6, 1)
        first = int(outs["irregular"][0].item()) & 0xFFFFFFFF
        line["same"] = bool(torch.equal(outs["irregular"][:n], outs["uniform"][:n]))
        line["same_update"] = ((int(outs["update"][0].item()) ^ -1) & 0xFFFFFFFF) == first
        print(line, flush=True)


if __name__ == "__main__":
    main()
