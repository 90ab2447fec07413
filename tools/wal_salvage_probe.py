#!/usr/bin/env python3
"""Cost of the device WAL salvage next to the index it loops over (not product code): the two images
tools/wal_index_probe.py builds (1 GiB of small records averaging 59 bytes, the 430 MB Zipf image),
resident in HBM. Per image, in one process: tkv_wal_index_device on the clean image (the yardstick),
tkv_wal_salvage_device on the clean image, with one payload bit flipped in the middle record, and with 16
flips spread evenly; the three steps of the one-flip salvage each alone (index to the flip, resync behind
it, index behind it); and, untimed by events, the 16-flip salvage step by step with a host clock and the
search's counters. Then tkv_wal_resync_device over 64 MiB of random bytes that hold no answer, and over the
same bytes with their top bit set (no offset passes the length check: the filter alone), next to a plain
streaming read of the same bytes (a torch sum), as GB/s of start offsets tested.

After untimed warm calls every leg is timed as K calls between one pair of device events on the calls'
stream (every call ends in a stream synchronize), the legs in rotation over --rounds rounds; the median
round is reported, with the least and the largest. Prints one JSON line per image and one for the resync.
The results of every leg are checked against the offsets the image was built from.

    python tools/wal_salvage_probe.py [--k 5] [--rounds 3] [--warmup 2]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ab_wal import image  # noqa: E402

VP, U64 = ctypes.c_void_p, ctypes.c_uint64
P64 = ctypes.POINTER(U64)
NO_LIMIT = (1 << 64) - 1


def load(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    lib.tkv_wal_stamp.argtypes = [VP, VP, VP, U64]
    lib.tkv_wal_index_device.argtypes = [VP, U64, VP, VP, U64, P64, P64, P64, VP]
    lib.tkv_wal_salvage_device.argtypes = [VP, U64, VP, U64, VP, U64, U64, P64, P64, P64, P64, P64, VP]
    lib.tkv_wal_resync_device.argtypes = [VP, U64, U64, P64, VP]
    assert lib.tkv_set_device(0) == 0
    return lib


def timed_k(fn, k):
    """Milliseconds per call of k synchronous calls between one pair of device events; the last result."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / k, out


def rotate(legs, k, rounds, warmup):
    """{name: per-call ms of each round}, {name: last result}."""
    res = {}
    for name, fn in legs:
        for _ in range(warmup):
            res[name] = fn()
    times = {name: [] for name, _ in legs}
    for r in range(rounds):
        for name, fn in legs[r % len(legs):] + legs[:r % len(legs)]:
            ms, res[name] = timed_k(fn, k)
            times[name].append(ms)
    return times, res


def summary(times):
    return {k: {"ms": round(float(np.median(v)), 4), "min_max_ms": [round(min(v), 4), round(max(v), 4)]} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small-records", type=int, default=18_199_191, help="records of the small-record image (1 GiB)")
    ap.add_argument("--zipf-records", type=int, default=400_000)
    ap.add_argument("--noise-mib", type=int, default=64)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    lib = load(os.path.join(ROOT, "tinykvpp_amd", "libtkv_crc32.so"))
    rng = np.random.default_rng(1)
    n = args.small_records
    small = image(n, rng.integers(4, 24, n).astype(np.uint32), rng.integers(0, 40, n).astype(np.uint32), rng)
    n2 = args.zipf_records
    zv = np.minimum(rng.zipf(1.6, n2) * 64, 16_000).astype(np.uint32)
    zv[-1] = 16
    zipf = image(n2, rng.integers(8, 64, n2).astype(np.uint32), zv, rng)
    st = VP(torch.cuda.current_stream().cuda_stream)
    for name, (w, offs, sz) in (("small records 1 GiB", small), ("zipf 430 MB", zipf)):
        assert lib.tkv_wal_stamp(VP(w.ctypes.data), VP(offs.ctypes.data), VP(sz.ctypes.data), offs.size) == 0
        size, nrec = int(w.size), int(offs.size)
        clean = torch.from_numpy(w).cuda()
        mid = nrec // 2
        one, many = clean.clone(), clean.clone()
        one[int(offs[mid]) + 8 + 3] ^= 1
        victims = [(i + 1) * nrec // 17 for i in range(16)]
        for v in victims:
            many[int(offs[v]) + 8 + 3] ^= 1
        cap = size // 26
        out = torch.empty(cap, dtype=torch.int64, device="cuda")
        gaps = np.zeros((64, 2), np.uint64)
        torch.cuda.synchronize()

        def index(d=clean, start=0):
            good, stop, seq = U64(0), U64(0), U64(0)
            rc = lib.tkv_wal_index_device(VP(d.data_ptr() + start), size - start, VP(out.data_ptr()), None, cap,
                                          ctypes.byref(good), ctypes.byref(stop), ctypes.byref(seq), st)
            return rc, good.value, stop.value

        def resync(d, start):
            found = U64(0)
            return lib.tkv_wal_resync_device(VP(d.data_ptr()), size, start, ctypes.byref(found), st), found.value

        def salvage(d):
            o = [U64(0) for _ in range(5)]
            rc = lib.tkv_wal_salvage_device(VP(d.data_ptr()), size, VP(out.data_ptr()), cap, VP(gaps.ctypes.data), 64, NO_LIMIT,
                                            *[ctypes.byref(x) for x in o], st)
            return (rc,) + tuple(x.value for x in o)  # rc, n_records, n_gaps, stop, skipped, max_seq

        legs = [("index_clean", index), ("salvage_clean", lambda: salvage(clean)), ("salvage_one_flip", lambda: salvage(one)),
                ("salvage_16_flips", lambda: salvage(many)),
                # the three steps of the one-flip salvage, each alone
                ("index_to_the_flip", lambda: index(one)), ("resync_behind_the_flip", lambda: resync(one, int(offs[mid]) + 1)),
                ("index_behind_the_flip", lambda: index(one, int(offs[mid + 1])))]
        times, res = rotate(legs, args.k, args.rounds, args.warmup)
        assert res["index_to_the_flip"] == (4, mid, int(offs[mid])) and res["resync_behind_the_flip"] == (0, int(offs[mid + 1]))
        assert res["index_behind_the_flip"] == (0, nrec - mid - 1, size - int(offs[mid + 1]))
        assert res["index_clean"] == (0, nrec, size) and res["salvage_clean"][:4] == (0, nrec, 0, size), res
        assert res["salvage_one_flip"][:5] == (4, nrec - 1, 1, size, int(sz[mid])), res["salvage_one_flip"]
        assert res["salvage_16_flips"][:5] == (4, nrec - 16, 16, size, int(sz[victims].sum())), res["salvage_16_flips"]
        # the 16-flip salvage step by step (host clock around each synchronous call; after the timed legs)
        steps, p = [], 0
        while p < size:
            t0 = time.perf_counter()
            rc, good, stop = index(many, p)
            t1 = time.perf_counter()
            if rc == 0:
                steps.append({"at": p, "index_ms": round((t1 - t0) * 1e3, 3)})
                break
            _, q = resync(many, p + stop + 1)
            t2 = time.perf_counter()
            last = (U64 * 6)()
            lib.tkv_debug_wal_salvage_last(last)
            steps.append({"at": p, "index_ms": round((t1 - t0) * 1e3, 3), "resync_ms": round((t2 - t1) * 1e3, 3),
                          "spans": int(last[1]), "candidates": int(last[3]), "candidate_bytes": int(last[4])})
            p = q
        salvage(many)  # (the legs share `out`: its contents are the last call's)
        assert np.array_equal(out[:nrec - 16].cpu().numpy().view(np.uint64), np.delete(offs, victims)), "salvaged offsets differ"
        assert gaps[:16].tolist() == [[int(offs[v]), int(offs[v + 1])] for v in victims]
        s = summary(times)
        base = s["index_clean"]["ms"]
        line = {"image": name, "bytes": size, "records": nrec, "k": args.k, "rounds": args.rounds, **s,
                "index_GB_per_s": round(size / base / 1e6, 1),
                "salvage_clean_over_index": round(s["salvage_clean"]["ms"] / base, 3),
                "salvage_one_flip_over_index": round(s["salvage_one_flip"]["ms"] / base, 3),
                "salvage_16_flips_over_index": round(s["salvage_16_flips"]["ms"] / base, 3), "steps_16_flips": steps}
        print(json.dumps(line), flush=True)
        del clean, one, many, out
        torch.cuda.empty_cache()
    # resync over random bytes without an answer, next to a streaming read of the same bytes
    nb = args.noise_mib << 20
    noise = torch.from_numpy(rng.integers(0, 256, nb, dtype=np.uint8)).cuda()
    words = noise.view(torch.int64)

    high = noise | 0x80  # every u32 above 2^31: no offset passes the length check, the filter alone runs
    counts = {}

    def resync(d, name):
        found = U64(0)
        rc = lib.tkv_wal_resync_device(VP(d.data_ptr()), nb, 0, ctypes.byref(found), st)
        last = (U64 * 6)()
        lib.tkv_debug_wal_salvage_last(last)
        counts[name] = {"spans": int(last[1]), "offsets_tested": int(last[2]), "candidates": int(last[3]),
                        "candidate_bytes": int(last[4])}
        return rc, found.value

    def stream_read():
        return int(words.sum().item())

    times, res = rotate([("resync_no_answer", lambda: resync(noise, "resync_no_answer")),
                         ("resync_no_candidates", lambda: resync(high, "resync_no_candidates")),
                         ("streaming_read", stream_read)], args.k, args.rounds, args.warmup)
    assert res["resync_no_answer"] == (1, nb) and res["resync_no_candidates"] == (1, nb), res
    assert counts["resync_no_candidates"]["candidates"] == 0
    s = summary(times)
    line = {"image": f"random bytes {args.noise_mib} MiB", "bytes": nb, "k": args.k, "rounds": args.rounds, **s,
            "resync_GB_per_s_of_offsets": round(nb / s["resync_no_answer"]["ms"] / 1e6, 1),
            "resync_no_candidates_GB_per_s_of_offsets": round(nb / s["resync_no_candidates"]["ms"] / 1e6, 1),
            "streaming_read_GB_per_s": round(nb / s["streaming_read"]["ms"] / 1e6, 1), "counts": counts}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
