#!/usr/bin/env python3
"""In-process A/B of the packed kernel with and without the segment fold (not product code).

    python tools/ab_fold.py [--rounds 8] [--reps 50] [--lib tinykvpp_amd/libtkv_crc32.so]

One library, one set of device buffers: tkv_debug_set_packed_fold(0 / 1) picks crc_packed<*, false> or
crc_packed<*, true> for the same launches, interleaved round by round on one stream; the two result
arrays are compared. Prints one JSON line per workload with the per-round GB/s of each variant and the
median ratio fold/table.
"""
import argparse
import ctypes
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = ctypes.c_void_p
U64 = ctypes.c_uint64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "tinykvpp_amd", "libtkv_crc32.so"))
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    lib = ctypes.CDLL(os.path.abspath(args.lib))
    lib.tkv_crc32_batch_uniform_device.argtypes = [VP, U64, U64, VP, VP, U64, VP]
    lib.tkv_fill_synthetic_uniform.argtypes = [VP, U64, U64, U64, U64, U64, VP]
    assert lib.tkv_set_device(0) == 0
    st = torch.cuda.current_stream()
    sp = VP(st.cuda_stream)
    data = torch.empty(4 << 30, dtype=torch.uint8, device="cuda")
    outs = [torch.empty(1 << 20, dtype=torch.int32, device="cuda") for _ in range(2)]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    for name, blen, n in (("cfg2 1M x 4 KiB", 4096, 1 << 20), ("64K x 64 KiB", 65536, 1 << 16)):
        lib.tkv_fill_synthetic_uniform(VP(data.data_ptr()), blen, blen, 0, n, 1, sp)

        def run(fold):
            prev = lib.tkv_debug_set_packed_fold(fold)
            try:
                f = lambda: lib.tkv_crc32_batch_uniform_device(VP(data.data_ptr()), blen, blen, None,
                                                               VP(outs[fold].data_ptr()), n, sp)
                for _ in range(10):
                    assert f() == 0
                e0.record(st)
                for _ in range(args.reps):
                    f()
                e1.record(st)
                torch.cuda.synchronize()
            finally:
                lib.tkv_debug_set_packed_fold(prev)
            return blen * n * args.reps / (e0.elapsed_time(e1) * 1e6)

        g = [[], []]
        for r in range(args.rounds):
            for fold in ((0, 1) if r % 2 == 0 else (1, 0)):
                g[fold].append(run(fold))
        same = bool(torch.equal(outs[0][:n], outs[1][:n]))
        ratios = np.array(g[1]) / np.array(g[0])
        print(json.dumps({"workload": name, "table_GBps": [round(x, 1) for x in g[0]],
                          "fold_GBps": [round(x, 1) for x in g[1]],
                          "ratios": [round(float(x), 4) for x in ratios],
                          "median_fold_over_table": round(float(np.median(ratios)), 4),
                          "results_identical": same}), flush=True)
        assert same


if __name__ == "__main__":
    main()
