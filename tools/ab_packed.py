#!/usr/bin/env python3
"""In-process A/B of packed-kernel variants on the same device buffers (not product code).

    python tools/ab_packed.py abl/libtkv_parent.so abl/libtkv_parent2.so tinykvpp_amd/libtkv_crc32.so \
        [--configs "0,0;4,0;0,1"] [--rounds 8] [--reps 50]

A variant is a library, or a library with one setting of its packed switches "window,order"
(tkv_debug_set_packed_window / tkv_debug_set_packed_order; --configs applies to the last library, which is
also run as it is, with its defaults). All variants run K launches each per round on one stream, the
starting variant rotating round by round; every result array is compared with the first variant's.
Prints one JSON line per workload: per-round GB/s of each variant and, for rounds 1.., the min / median
/ max of its ratio to the first variant (round 0 is warm-up: whoever runs first starts on an idle
device).
"""
import argparse
import ctypes
import json
import os

import numpy as np
import torch

VP = ctypes.c_void_p
U64 = ctypes.c_uint64


def load(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    lib.tkv_crc32_batch_uniform_device.argtypes = [VP, U64, U64, VP, VP, U64, VP]
    lib.tkv_fill_synthetic_uniform.argtypes = [VP, U64, U64, U64, U64, U64, VP]
    assert lib.tkv_set_device(0) == 0
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+")
    ap.add_argument("--configs", default="", help='";"-separated "window,order" settings of the last library')
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", default=None, help="run only workloads whose name contains this")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    libs = [load(p) for p in args.libs]
    variants = [(os.path.basename(p), lib, None) for p, lib in zip(args.libs, libs)]
    for cfg in filter(None, args.configs.split(";")):
        variants.append((f"{os.path.basename(args.libs[-1])}[{cfg}]", libs[-1], tuple(int(x) for x in cfg.split(","))))
    st = torch.cuda.current_stream()
    sp = VP(st.cuda_stream)
    work = [("1M x 4 KiB", 4096, 1 << 20), ("256K x 64 KiB", 65536, 1 << 18), ("512K x 64 KiB", 65536, 1 << 19)]
    work = [w for w in work if not args.only or args.only in w[0]]
    data = torch.empty(max(b * n for _, b, n in work), dtype=torch.uint8, device="cuda")
    outs = [torch.empty(1 << 20, dtype=torch.int32, device="cuda") for _ in variants]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    for name, blen, n in work:
        libs[0].tkv_fill_synthetic_uniform(VP(data.data_ptr()), blen, blen, 0, n, 1, sp)

        def run(v):
            _, lib, cfg = variants[v]
            if cfg is not None:
                prev = (lib.tkv_debug_set_packed_window(cfg[0]), lib.tkv_debug_set_packed_order(cfg[1]))
            try:
                f = lambda: lib.tkv_crc32_batch_uniform_device(VP(data.data_ptr()), blen, blen, None,
                                                               VP(outs[v].data_ptr()), n, sp)
                for _ in range(10):
                    assert f() == 0
                e0.record(st)
                for _ in range(args.reps):
                    f()
                e1.record(st)
                torch.cuda.synchronize()
            finally:
                if cfg is not None:
                    lib.tkv_debug_set_packed_window(prev[0])
                    lib.tkv_debug_set_packed_order(prev[1])
            return blen * n * args.reps / (e0.elapsed_time(e1) * 1e6)

        g = [[] for _ in variants]
        for r in range(args.rounds):
            for i in range(len(variants)):
                v = (i + r) % len(variants)
                g[v].append(run(v))
        same = all(bool(torch.equal(outs[0][:n], o[:n])) for o in outs[1:])
        base = np.array(g[0][1:])
        rec = {"workload": name, "results_identical": same, "variants": {}}
        for (label, _, _), gv in zip(variants, g):
            ratio = np.array(gv[1:]) / base
            rec["variants"][label] = {"GBps": [round(x, 1) for x in gv],
                                      "ratio_to_first_rounds_1..": [round(float(ratio.min()), 4),
                                                                    round(float(np.median(ratio)), 4),
                                                                    round(float(ratio.max()), 4)]}
        print(json.dumps(rec), flush=True)
        assert same


if __name__ == "__main__":
    main()
