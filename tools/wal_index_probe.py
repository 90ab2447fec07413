#!/usr/bin/env python3
"""Cost of the device WAL record index next to the verify it sits on (not product code): the two images
tools/ab_wal.py builds (1 GiB of small records, the 430 MB Zipf image), resident in HBM. After untimed
warm-ups, K warm calls each of tkv_wal_verify_device and tkv_wal_index_device of this tree's library,
and of tkv_wal_verify_device of another build (--base, e.g. the parent commit's library from
tools/build_at.sh) as the yardstick, in one process, in rotation, each between a pair of device events
on the calls' stream (both calls end in a stream synchronize). Prints one JSON line per image: median
times, the index as a multiple of the verify, this tree's verify against the base's. The index of each
image is compared with the offsets and sequence numbers the image was built from.

    python tools/wal_index_probe.py [--base abl/libtkv_parent.so] [--k 20] [--warmup 3]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ab_wal import image  # noqa: E402

VP, U64 = ctypes.c_void_p, ctypes.c_uint64
P64 = ctypes.POINTER(U64)


def load(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    lib.tkv_wal_verify_device.argtypes = [VP, U64, P64, P64, VP]
    lib.tkv_wal_stamp.argtypes = [VP, VP, VP, U64]
    if hasattr(lib, "tkv_wal_index_device"):
        lib.tkv_wal_index_device.argtypes = [VP, U64, VP, VP, U64, P64, P64, P64, VP]
    assert lib.tkv_set_device(0) == 0
    return lib


def timed(fn):
    """Milliseconds between device events around one synchronous call on the current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", default=None, help="another build of the library: the verify yardstick")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small-records", type=int, default=18_199_191, help="records of the small-record image (1 GiB)")
    ap.add_argument("--zipf-records", type=int, default=400_000)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    tree = load(os.path.join(ROOT, "tinykvpp_amd", "libtkv_crc32.so"))
    base = load(args.base) if args.base else None
    rng = np.random.default_rng(1)
    n = args.small_records
    small = image(n, rng.integers(4, 24, n).astype(np.uint32), rng.integers(0, 40, n).astype(np.uint32), rng)
    n2 = args.zipf_records
    zv = np.minimum(rng.zipf(1.6, n2) * 64, 16_000).astype(np.uint32)
    zv[-1] = 16  # a short final record (a long last payload across a region end)
    zipf = image(n2, rng.integers(8, 64, n2).astype(np.uint32), zv, rng)
    st = VP(torch.cuda.current_stream().cuda_stream)
    for name, (w, offs, sz) in (("small records 1 GiB", small), ("zipf 430 MB", zipf)):
        assert tree.tkv_wal_stamp(VP(w.ctypes.data), VP(offs.ctypes.data), VP(sz.ctypes.data), offs.size) == 0
        seq_max = 0
        for a in range(0, offs.size, 1 << 20):  # the records' sequence_ fields, a million at a time
            at = offs[a:a + (1 << 20)].astype(np.int64)
            seq_max = max(seq_max, int(w[at[:, None] + 9 + np.arange(8)].view("<u8").max()))
        d = torch.from_numpy(w).cuda()
        cap = w.size // 26
        out = torch.empty(cap, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def verify(lib):
            good, stop = U64(0), U64(0)
            rc = lib.tkv_wal_verify_device(VP(d.data_ptr()), w.size, ctypes.byref(good), ctypes.byref(stop), st)
            return rc, good.value, stop.value

        def index():
            good, stop, seq = U64(0), U64(0), U64(0)
            rc = tree.tkv_wal_index_device(VP(d.data_ptr()), w.size, VP(out.data_ptr()), None, cap, ctypes.byref(good),
                                           ctypes.byref(stop), ctypes.byref(seq), st)
            return rc, good.value, stop.value, seq.value

        legs = [("verify", lambda: verify(tree)), ("index", index)]
        if base is not None:
            legs.append(("base_verify", lambda: verify(base)))
        times = {k: [] for k, _ in legs}
        res = {}
        for r in range(args.warmup + args.k):
            order = legs[r % len(legs):] + legs[:r % len(legs)]
            for k, fn in order:
                ms, res[k] = timed(fn)
                if r >= args.warmup:
                    times[k].append(ms)
        want = (0, offs.size, w.size)
        assert res["verify"] == want and res["index"] == want + (seq_max,), (res, want, seq_max)
        if base is not None:
            assert res["base_verify"] == want
        assert np.array_equal(out[:offs.size].cpu().numpy().view(np.uint64), offs), "index differs from the image's offsets"
        med = {k: float(np.median(v)) for k, v in times.items()}
        line = {"image": name, "bytes": int(w.size), "records": int(offs.size), "k": args.k,
                "verify_ms": round(med["verify"], 4), "index_ms": round(med["index"], 4),
                "index_over_verify": round(med["index"] / med["verify"], 3),
                "verify_GB_per_s": round(w.size / med["verify"] / 1e6, 1),
                "index_GB_per_s": round(w.size / med["index"] / 1e6, 1),
                "verify_min_max_ms": [round(min(times["verify"]), 4), round(max(times["verify"]), 4)],
                "index_min_max_ms": [round(min(times["index"]), 4), round(max(times["index"]), 4)]}
        if base is not None:
            line["base_verify_ms"] = round(med["base_verify"], 4)
            line["verify_over_base"] = round(med["verify"] / med["base_verify"], 4)
        print(json.dumps(line), flush=True)
        del d, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
