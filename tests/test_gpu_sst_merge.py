"""The device SSTable merge (tkv_sst_merge_device) against the dict oracle of tests/sst_merge_util.py and the
host call, bit for bit, with canaries on both sides of every output: counts around the workgroup tile, ties
across the partition, the comparator's edges, K up to 64, duplicates, tombstones, sources, outputs, errors,
fuzz, one larger case, the compaction pipelines and threads."""
import ctypes
import threading

import numpy as np
import pytest
import torch

import memtable_util as mu
import sst_merge_util as gu
from sst_build_util import oracle_file
from sst_merge_util import CORRUPTED, NONE, OK, OVERFLOW
from tinykvpp_amd import load_library, memtable, sst

pytestmark = pytest.mark.gpu

T = int(load_library().tkv_debug_sst_merge_tile())
CASES = gu.named_cases(T)


def stream_of(gpu):
    return (ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream),)


def check(gpu, lib, cols, flags=0, **kw):
    return gu.check_merge(lib.tkv_sst_merge_device, cols, flags, device=gpu, tail=stream_of(gpu), also=lib.tkv_sst_merge, **kw)


def last(lib):
    out = (ctypes.c_uint64 * 4)()
    lib.tkv_debug_sst_merge_last(out)
    return list(out)


def rounds_and_tiles(sizes):
    """What tkv_debug_sst_merge_last must report: ceil(log2) of the non-empty runs, and the tiles of the
    last round (one pair over all N entries)."""
    live = sum(1 for n in sizes if n)
    rounds = (live - 1).bit_length() if live else 0
    return rounds, -(-sum(sizes) // T) if rounds else 0


def test_the_tile_is_what_the_cases_assume(lib):
    assert T >= 64 and T % 64 == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_named_cases(gpu, lib, name):
    cols = gu.columns(CASES[name])
    for flags in (0, gu.DROP):
        check(gpu, lib, cols, flags)
    sizes = [len(r) for r in CASES[name]]
    assert last(lib)[:3] == [sum(sizes), *rounds_and_tiles(sizes)]
    assert last(lib)[3] > 0


def test_k5_passes_a_list_through_two_rounds_unpaired(gpu, lib):
    """Five non-empty runs: the fifth list has no partner in rounds 1 and 2 and meets the rest in round 3."""
    rng = np.random.default_rng(40)
    runs = gu.overlapping(rng, [T + 1, 70, 2 * T, 5, T // 2 + 3])
    check(gpu, lib, gu.columns(runs))
    assert last(lib)[1:3] == [3, -(-sum(len(r) for r in runs) // T)]


def test_survivor_of_a_group_across_the_tile_boundary(gpu, lib):
    for name in ("straddle_3_3", "all_equal"):
        runs = CASES[name]
        src = check(gpu, lib, gu.columns(runs))
        users = [k[:-17] for k, _ in runs[1]]
        x = max(set(users), key=users.count)
        assert (1, max(i for i, u in enumerate(users) if u == x)) in src


@pytest.mark.parametrize("misalign", range(16))
def test_every_arena_misalignment(gpu, lib, misalign):
    rng = np.random.default_rng(41)
    runs = gu.overlapping(rng, [90, 130, 60], lo=0, hi=30, alpha=3)
    check(gpu, lib, gu.columns(runs), gu.DROP if misalign % 2 else 0, misalign=misalign)


def test_sources(gpu, lib):
    rng = np.random.default_rng(42)
    runs = gu.overlapping(rng, [T + 9, 300, 200])
    check(gpu, lib, gu.columns(runs, shared=True))                  # two and more runs in one arena
    check(gpu, lib, gu.columns(runs), below=8192, misalign=7)       # the base strictly below every arena
    check(gpu, lib, gu.columns(runs), bias=False)                   # val_bias NULL
    check(gpu, lib, gu.columns(runs, null_vals=(1,)))
    check(gpu, lib, gu.columns(runs, null_vals=(0, 1, 2)))


def test_runs_as_views_from_the_device_scan(gpu, lib):
    rng = np.random.default_rng(43)
    runs = gu.overlapping(rng, [400, 0, 250, 330])
    tables = []
    for run in runs:
        if not run:
            continue
        image = torch.from_numpy(np.frombuffer(oracle_file(run, 512)[0], np.uint8).copy()).to(gpu)
        tables.append(sst.scan_device(image, key_views=True, val_views=True))
        assert tables[-1].keys.data_ptr() == image.data_ptr() and tables[-1].vals.data_ptr() == image.data_ptr()
    live = [r for r in runs if r]
    want = gu.oracle(gu.columns(live))
    got = sst.merge_device(tables)
    assert got.src.cpu().numpy().view(np.uint64).tolist() == [r << 32 | i for r, i in want]
    assert got.entries() == [live[r][i] for r, i in want]
    assert got.key_base == min(t.keys.data_ptr() for t in tables)


@pytest.mark.parametrize("null", gu.OUT_NAMES)
def test_single_null_output(gpu, lib, null):
    rng = np.random.default_rng(44)
    check(gpu, lib, gu.columns(gu.overlapping(rng, [T + 5, 120])), nulls=(null,))


def run_corrupt(gpu, lib, cols, size):
    placed = gu.Placed(cols, gpu)
    outs = gu.Outputs(sum(placed.n), device=gpu)
    res = gu.call(lib.tkv_sst_merge_device, placed, 0, outs, tables=placed.tables(keys_size=size), tail=stream_of(gpu))
    gu.assert_untouched(outs)
    return res


@pytest.mark.parametrize("kind", gu.CORRUPT_KINDS)
def test_corrupted(gpu, lib, kind):
    rng = np.random.default_rng(45)
    base = gu.columns(gu.overlapping(rng, [T + 40, 0, 2 * T + 50, 30], lo=2))
    for r, i in ((0, 0), (2, 0), (2, 2 * T + 49), (2, T - 40), (2, T - 41), (3, 29)):  # run 2 starts at position T + 40
        cols, size = gu.corrupt(base, r, i, kind)
        want = gu.first_bad(cols, size)
        assert want != NONE and want >> 32 == r
        assert run_corrupt(gpu, lib, cols, size) == (CORRUPTED, 0, 0, 0, want)
    cols, size = gu.corrupt(base, 3, 2, kind)
    cols, size = gu.corrupt(cols, 2, 300, kind)
    want = gu.first_bad(cols, size)
    assert want >> 32 == 2
    assert run_corrupt(gpu, lib, cols, size) == (CORRUPTED, 0, 0, 0, want)
    check(gpu, lib, base)  # the same scratch serves a sound call afterwards


def test_overflow_and_exact(gpu, lib):
    rng = np.random.default_rng(46)
    cols = gu.columns(gu.overlapping(rng, [T, 700, 60]))
    src = gu.oracle(cols)
    placed = gu.Placed(cols, gpu)
    want = gu.expected(placed, src)
    m, kb, vb = len(src), int(want["key_len"].sum()), int(want["val_len"].sum())
    for null in ((), ("key_off", "key_len", "val_off", "val_len")):
        outs = gu.Outputs(m - 1, nulls=null, device=gpu)
        assert gu.call(lib.tkv_sst_merge_device, placed, 0, outs, tail=stream_of(gpu)) == (OVERFLOW, m, kb, vb, NONE)
        gu.assert_untouched(outs)


def test_all_tombstones_writes_nothing(gpu, lib):
    placed = gu.Placed(gu.columns(CASES["all_tombstones"]), gpu)
    outs = gu.Outputs(200, device=gpu)
    assert gu.call(lib.tkv_sst_merge_device, placed, gu.DROP, outs, tail=stream_of(gpu)) == (OK, 0, 0, 0, NONE)
    gu.assert_untouched(outs)


def test_empty_inputs(gpu, lib):
    outs = gu.Outputs(4, device=gpu)
    assert gu.call(lib.tkv_sst_merge_device, gu.Placed([], gpu), 0, outs, tail=stream_of(gpu)) == (OK, 0, 0, 0, NONE)
    assert gu.call(lib.tkv_sst_merge_device, gu.Placed(gu.columns([[], []]), gpu), 0, outs, tail=stream_of(gpu)) == (OK, 0, 0, 0, NONE)
    gu.assert_untouched(outs)


@pytest.mark.parametrize("seed", range(gu.FUZZ_SEEDS))
def test_fuzz(gpu, lib, seed):
    runs, drop = gu.fuzz_case(seed)
    check(gpu, lib, gu.columns(runs, shared=seed % 4 == 1), gu.DROP if drop else 0, misalign=seed % 16)


def to_device(gpu, cols):
    """Runs of numpy arrays as tuples of CUDA tensors: what merge_device takes."""
    def dev(x):
        return torch.from_numpy(x if x.dtype == np.uint8 else x.view(x.dtype.str.replace("u", "i"))).to(gpu)
    return [tuple(dev(x) for x in c) for c in cols]


def test_two_calls_agree_bit_for_bit(gpu, lib):
    runs, _ = gu.fuzz_case(3)
    dev = to_device(gpu, gu.columns(runs))
    a, b = sst.merge_device(dev), sst.merge_device(dev)
    for name in ("key_off", "key_len", "val_off", "val_len", "src"):
        assert torch.equal(getattr(a, name), getattr(b, name))


def test_larger_case(gpu, lib):
    """2^20 + 3 entries over 4 runs of distinct 8-byte keys: a tile map of hundreds of tiles in every round and
    a survivor scan of more than one level. The oracle is numpy's: sort by key, then by position in the
    concatenation; the last of every group survives."""
    rng = np.random.default_rng(47)
    total = (1 << 20) + 3
    sizes = [total // 4, total // 4 + 3, total // 4 - 1000, total - 3 * (total // 4) + 997]
    assert sum(sizes) == total
    pool = np.unique(rng.integers(0, 1 << 63, total, dtype=np.uint64))
    cols, words = [], []
    for r, n in enumerate(sizes):
        w = np.sort(pool[rng.choice(pool.size, n, replace=False)])
        raw = np.zeros((n, 25), np.uint8)
        raw[:, :8] = w.astype(">u8").view(np.uint8).reshape(n, 8)
        raw[:, 8] = r
        raw[:, 24] = rng.random(n) < 0.1
        cols.append(gu.Run(raw.reshape(-1), np.arange(n, dtype=np.uint64) * 25, np.full(n, 25, np.uint32), None, None, None))
        words.append(w)
    allw = np.concatenate(words)
    order = np.lexsort((np.arange(total), allw))
    keep = np.ones(total, bool)
    keep[:-1] = allw[order][1:] != allw[order][:-1]
    pos = order[keep]
    start = np.cumsum([0] + sizes[:-1])
    run = np.searchsorted(start, pos, side="right") - 1
    want = (run.astype(np.uint64) << np.uint64(32)) | (pos - start[run]).astype(np.uint64)
    placed = gu.Placed(cols, gpu)
    sizing = gu.Outputs(0, nulls=gu.OUT_NAMES, device=gpu)
    assert gu.call(lib.tkv_sst_merge_device, placed, 0, sizing, tail=stream_of(gpu)) == (OK, want.size, 25 * want.size, 0, NONE)
    outs = gu.Outputs(want.size, device=gpu)
    assert gu.call(lib.tkv_sst_merge_device, placed, 0, outs, tail=stream_of(gpu))[:2] == (OK, want.size)
    assert np.array_equal(outs.get("src", want.size), want) and outs.untouched("src", want.size)
    assert np.array_equal(outs.get("key_off", want.size),
                          np.array(placed.key_addr, np.uint64)[run] - np.uint64(placed.key_base) + (want & np.uint64(0xFFFFFFFF)) * np.uint64(25))
    assert last(lib)[:3] == [total, 2, -(-total // T)]
    host = gu.Outputs(want.size)
    assert gu.call(lib.tkv_sst_merge, gu.Placed(cols), 0, host)[:2] == (OK, want.size)
    assert np.array_equal(host.get("src", want.size), want)


# ---- pipelines ------------------------------------------------------------------------------------------

def batches():
    """Three overlapping record batches (op, seq, key, value, tomb), oldest first."""
    rng = np.random.default_rng(48)
    pool = gu.distinct_keys(rng, 900, lo=0, hi=20, alpha=5)
    out, seq = [], 1
    for b in range(3):
        recs = []
        for j in rng.choice(len(pool), 700).tolist():
            op = int(rng.random() < 0.2)
            recs.append((op, seq, pool[j], b"" if op else b"b%d-%d" % (b, seq), op))
            seq += 1
        out.append(recs)
    return out


def upload(gpu, c):
    def dev(a):
        if a.dtype != np.uint8:
            a = a.view(a.dtype.str.replace("u", "i"))
        return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return {k: dev(v) for k, v in c._asdict().items()}


def flushed(gpu, recs, ts):
    run = memtable.build_device(timestamp_ms=ts, vals=torch.from_numpy(mu.values_arena(recs)).to(gpu), **upload(gpu, mu.columns(recs)))
    return run.flush()


def test_compaction_pipelines(gpu, lib):
    ts = 1_700_000_000_000
    bs = batches()
    files = [flushed(gpu, recs, ts).file for recs in bs]
    every = [r for recs in bs for r in recs]
    want = mu.entries(mu.oracle(mu.columns(every), ts), mu.values_arena(every).tobytes())
    # (a) the compaction of the three files is the flush of one replay over all the records, byte for byte
    compacted = sst.compact_device(files)
    image = compacted.file.cpu().numpy().tobytes()
    assert image == flushed(gpu, every, ts).file.cpu().numpy().tobytes()
    assert image == oracle_file(want, 4096)[0]
    # (b) and scans back to the oracle's entries
    assert sst.scan_device(compacted.file).entries() == want
    # (c) the last level drops the tombstones
    live = [(k, v) for k, v in want if k[-1] == 0]
    assert 0 < len(live) < len(want)
    dropped = sst.compact_device(files, drop_tombstones=True)
    assert dropped.file.cpu().numpy().tobytes() == oracle_file(live, 4096)[0]
    # (d) the host calls give the same files
    host_files = [f.cpu().numpy() for f in files]
    assert sst.compact(host_files).file.tobytes() == image
    assert sst.compact(host_files, drop_tombstones=True, target_block_size=1024).file.tobytes() == oracle_file(live, 1024)[0]


def test_merge_device_rejects_a_bad_run(gpu, lib):
    rng = np.random.default_rng(49)
    cols, _ = gu.corrupt(gu.columns(gu.overlapping(rng, [50, 60])), 1, 33, "order")
    dev = to_device(gpu, cols)
    with pytest.raises(sst.MergeCorrupted) as e:
        sst.merge_device(dev)
    assert (e.value.run, e.value.index) == (1, 33)


# ---- threads and the phase clock --------------------------------------------------------------------------

def test_four_threads_merge_at_once(gpu, lib):
    cases = [gu.fuzz_case(100 + t) for t in range(4)]
    failures = []

    def run(t):
        try:
            torch.cuda.set_device(gpu)
            runs, drop = cases[t]
            for _ in range(3):
                gu.check_merge(lib.tkv_sst_merge_device, gu.columns(runs), gu.DROP if drop else 0, device=gpu, tail=stream_of(gpu))
        except BaseException as e:  # noqa: BLE001
            failures.append((t, repr(e)))
    threads = [threading.Thread(target=run, args=(t,), daemon=True) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(120)
    assert not any(th.is_alive() for th in threads), "a caller is still running after 120 s"
    assert not failures, failures


def test_phase_times_zero_unless_enabled(gpu, lib):
    rng = np.random.default_rng(50)
    cols = gu.columns(gu.overlapping(rng, [3 * T, 2 * T, T]))
    ms = (ctypes.c_double * 4)()
    prev = lib.tkv_debug_sst_merge_phases(0, None)
    try:
        check(gpu, lib, cols)
        lib.tkv_debug_sst_merge_phases(1, ms)
        assert list(ms) == [0.0] * 4
        check(gpu, lib, cols)
        lib.tkv_debug_sst_merge_phases(0, ms)
        assert all(v >= 0.0 for v in ms) and sum(ms) > 0.0
    finally:
        lib.tkv_debug_sst_merge_phases(prev, None)
