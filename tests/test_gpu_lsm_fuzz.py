"""The device LSM pipeline end to end on random record batches (lsm_fuzz_util.case): per batch WAL encode ->
recover -> memtable replay -> flush into a misaligned, canaried slice -> scan with both arenas as views; then
the merge of the scanned tables and the compactions (flat, with the drop flag, nested through an intermediate
file, and a merge that mixes a memtable run with scanned tables), and the scan of the compacted file. Every
stage is checked against its sequential oracle before the next one consumes it, on the seed's stream. Then a
damaged input file, the largest and the smallest seed in turn in grown scratch, and four host threads that
run the whole pipeline at once. Every expected value comes from lsm_fuzz_util.expect, which
test_lsm_fuzz_cpu.py checks against the host paths for the same seeds."""
import ctypes
import threading
import types

import numpy as np
import pytest
import torch

import lsm_fuzz_util as fz
import wal_decode_util as wd
from tinykvpp_amd import load_library, memtable, sst, wal
from wal_encode_util import DeviceBatch
from wal_encode_util import last as encode_last

pytestmark = pytest.mark.gpu

T = int(load_library().tkv_debug_sst_merge_tile())
KEPT = {fz.LARGEST, fz.SMALLEST, fz.DAMAGED, *fz.THREAD_SEEDS}  # seeds more than one test runs
_made = {}


def prepared(seed, oracle):
    """(case, expected) of a seed; made once for the seeds of KEPT."""
    if seed in _made:
        return _made[seed]
    c = fz.case(seed)
    made = c, fz.expect(c, oracle)
    if seed in KEPT:
        _made[seed] = made
    return made


def last(lib, path):
    out = (ctypes.c_uint64 * 4)()
    getattr(lib, f"tkv_debug_{path}_last")(out)
    return list(out)


def host(t):
    return t.cpu().numpy()


def placed(gpu, size, misalign):
    """(buffer of canary bytes, start): buffer[start:start + size] lies ``misalign`` bytes past a 16-byte
    boundary with at least GUARD canary bytes on either side."""
    buf = torch.full((fz.GUARD + 16 + size + fz.GUARD,), fz.CANARY, dtype=torch.uint8, device=gpu)
    return buf, fz.GUARD + (misalign - (buf.data_ptr() + fz.GUARD)) % 16


def file_bytes(table):
    return host(table.file).tobytes()


def same_bytes(got, want, what, starts=None, again=None):
    """Two uint8 arrays are equal; the failure names the sizes, how many bytes differ, the first of them and,
    with ``starts`` (ascending record offsets), the record and the byte inside it of every differing byte (up to
    40); with ``again`` (reads the device tensor a second time) also whether that second copy is the expected one,
    which tells wrong bytes on the device from a wrong copy to the host."""
    if got.size == want.size and np.array_equal(got, want):
        return
    bad = np.flatnonzero(got[:want.size] != want[:got.size])
    msg = f"{what}: {got.size} bytes against {want.size} expected, {bad.size} differ, first at {bad[:8].tolist()}"
    if bad.size and starts is not None:
        r = int(np.searchsorted(starts, bad[0], "right")) - 1
        msg += (f" (record {r} of {len(starts)}, byte {int(bad[0]) - int(starts[r])} of it; got "
                f"{got[bad[:8]].tolist()}, expected {want[bad[:8]].tolist()})")
        rs = np.searchsorted(starts, bad[:40], "right") - 1
        msg += f"; (record, byte) of the differing bytes: {list(zip(rs.tolist(), (bad[:40] - starts[rs].astype(np.int64)).tolist()))}"
    if again is not None:
        second = again()
        msg += f"; a second copy from the device {'equals' if np.array_equal(second, want) else 'differs from'} the expected bytes"
        msg += "" if np.array_equal(second, got) else " and differs from the first copy"
    raise AssertionError(msg)


def batch_stages(gpu, lib, c, e, b, stream):
    """Stages 1-5 for batch b: returns (file tensor, ScannedTable, MemtableRun)."""
    recs = c.batches[b]
    n = len(recs)
    where = f"seed {c.seed} batch {b} ({n} records)"
    kv, vv = bool(c.flags & wd.KEY_VIEWS), bool(c.flags & wd.VAL_VIEWS)
    # 1. the batch as a WAL image
    img, offs, crc = e.wal[b]
    t = DeviceBatch(fz.wal_batch(recs), gpu).t
    image, rec_off, dcrc = wal.encode_device(t["keys"], t["key_off"], t["key_len"], t["vals"], t["val_off"], t["val_len"],
                                             t["op"], t["tomb"], t["seq"], stream=stream)
    same_bytes(host(image), img, f"{where}: encode, image", offs, again=lambda: host(image))
    assert np.array_equal(host(rec_off).view(np.uint64), offs), f"{where}: encode, rec_off"
    assert np.array_equal(host(dcrc).view(np.uint32), crc), f"{where}: encode, crc"
    st = encode_last(lib)
    assert st[0] + st[1] == n and st[3] == img.size, (where, st)
    # 2. recovered with the seed's view flags
    status, batch, stop, mseq = wal.recover_device(image, key_views=kv, val_views=vv, stream=stream)
    assert (status, stop, mseq, batch.op.numel()) == ("ok", img.size, max(r[1] for r in recs), n), f"{where}: recover"
    want = e.decoded[b]
    for name in wd.COLS:
        assert np.array_equal(host(getattr(batch, name)).view(wd.DTYPES[name]), want[name]), f"{where}: recover, {name}"
    for name, views in (("keys", kv), ("vals", vv)):
        if views:
            assert getattr(batch, name) is image, f"{where}: recover, {name} is not the image"
        else:
            assert np.array_equal(host(getattr(batch, name)), want[name]), f"{where}: recover, {name}"
    assert wd.last(lib)[2:] == [want["keys_size"], want["vals_size"]], where
    # 3. replayed
    run = memtable.build_device(batch, timestamp_ms=c.ts[b], stream=stream)
    exp = e.mem[b]
    assert host(run.ikeys).tobytes() == exp.ikeys, f"{where}: replay, ikeys"
    assert np.array_equal(host(run.src).view(np.uint32), exp.src), f"{where}: replay, src"
    assert run.vals is batch.vals and (not vv or run.vals is image), f"{where}: replay, vals"
    assert run.entries() == e.entries[b], f"{where}: replay, entries"
    assert last(lib, "memtable")[0] == exp.src.size, where
    # 4. flushed into a slice at the seed's misalignment
    want_file, blocks, ioff, isz = e.files[b]
    size = len(want_file)
    buf, start = placed(gpu, size, c.misalign)
    table = run.flush(c.target, out=buf[start:start + size], stream=stream)
    h = host(buf)
    assert table.size == size and table.file.data_ptr() % 16 == c.misalign, f"{where}: flush"
    assert h[start:start + size].tobytes() == want_file, f"{where}: flush, file (target {c.target})"
    assert (h[:start] == fz.CANARY).all() and (h[start + size:] == fz.CANARY).all(), f"{where}: flush wrote outside its slice"
    assert host(table.block_off).tolist() == [x[0] for x in blocks], f"{where}: flush, block_off"
    assert host(table.block_size).view(np.uint32).tolist() == [x[1] for x in blocks], f"{where}: flush, block_size"
    assert host(table.block_first).view(np.uint32).tolist() == [x[2] for x in blocks], f"{where}: flush, block_first"
    assert (table.index_offset, table.index_size) == (ioff, isz), f"{where}: flush, index"
    st = last(lib, "sst_build")
    assert (st[0], st[3]) == (len(blocks), size), (where, st)
    # 5. scanned: both arenas are the file
    scanned = sst.scan_device(table.file, key_views=True, val_views=True, stream=stream)
    assert scanned.keys is table.file and scanned.vals is table.file, f"{where}: scan, arenas"
    assert scanned.entries() == e.scans[b], f"{where}: scan, entries"
    assert host(scanned.block_off).tolist() == [x[0] for x in blocks], f"{where}: scan, block_off"
    assert last(lib, "sst_scan")[0] == len(blocks), where
    return table.file, scanned, run


def merged_is(c, e, got, what):
    assert host(got.src).view(np.uint64).tolist() == [r << 32 | i for r, i in e.src], f"seed {c.seed}: {what}, src"
    assert got.entries() == e.model, f"seed {c.seed}: {what}, entries"


def pipeline(gpu, lib, c, e, stream=None):
    """The whole pipeline for a case on ``stream`` (None: the current stream); returns the compacted file."""
    files, tables, runs = [], [], []
    for b in range(c.k):
        f, t, r = batch_stages(gpu, lib, c, e, b, stream)
        files.append(f), tables.append(t), runs.append(r)
    where = f"seed {c.seed} ({c.k} files, target {c.target})"
    # 6. the merge of the scanned tables
    merged = sst.merge_device(tables, stream=stream)
    merged_is(c, e, merged, "merge")
    assert merged.key_base == min(f.data_ptr() for f in files), f"{where}: merge, key_base"
    n_in = sum(len(x) for x in e.entries)
    assert last(lib, "sst_merge")[:3] == [n_in, (c.k - 1).bit_length(), -(-n_in // T)], where
    # 7. the compactions
    compacted = sst.compact_device(files, c.target, stream=stream)
    flat = file_bytes(compacted)
    assert flat == e.flat, f"{where}: compaction"
    dropped = sst.compact_device(files, c.target, drop_tombstones=True, stream=stream)
    assert file_bytes(dropped) == e.dropped, f"{where}: compaction with drop"
    half = c.k // 2
    if e.half is not None:
        mid = sst.compact_device(files[:half], fz.NESTED_TARGET, stream=stream)
        assert file_bytes(mid) == e.half, f"{where}: compaction of the first {half} files"
        nested = sst.compact_device([mid.file] + files[half:], c.target, stream=stream)
        assert file_bytes(nested) == flat, f"{where}: nested compaction"
    j = c.seed % c.k  # a memtable run among scanned tables
    mixed = sst.merge_device(tables[:j] + [runs[j]] + tables[j + 1:], stream=stream)
    merged_is(c, e, mixed, f"merge with run {j} a memtable run")
    assert file_bytes(mixed.flush(c.target, stream=stream)) == flat, f"{where}: flush of the mixed merge"
    # 8. the compacted files scanned back
    back = sst.scan_device(compacted.file, stream=stream).entries()
    assert back == e.model, f"{where}: scan of the compacted file"
    users = [k[:-fz.META] for k, _ in back]
    assert all(a < b for a, b in zip(users, users[1:])), f"{where}: user keys do not ascend strictly"
    assert sst.scan_device(dropped.file, stream=stream).entries() == e.live, f"{where}: scan of the file without tombstones"
    return flat


@pytest.mark.parametrize("seed", fz.SEEDS)
def test_pipeline(gpu, lib, oracle, seed):
    c, e = prepared(seed, oracle)
    pipeline(gpu, lib, c, e, torch.cuda.Stream(gpu) if c.other_stream else None)


# ---- edge batches ---------------------------------------------------------------------------------------------

EDGE_BATCHES = {
    # every value empty: the decode's copied value arena has no byte, and the flush still needs an address
    "no_value_bytes": [(1, 5, b"k2", b"", 1), (1, 6, b"k1", b"", 1), (0, 7, b"", b"", 0), (1, 8, b"k1", b"", 1)],
    # the only key is the empty key: the decode's copied key arena has no byte
    "only_the_empty_key": [(0, 3, b"", b"first", 0), (0, 2, b"", b"second", 0)],
}


@pytest.mark.parametrize("views", [False, True])
@pytest.mark.parametrize("name", sorted(EDGE_BATCHES))
def test_batch_with_an_empty_arena(gpu, lib, oracle, name, views):
    """recover -> replay -> flush -> scan of a batch whose decoded key or value arena holds no byte, with
    copied arenas and with views."""
    c = types.SimpleNamespace(seed=name, k=1, batches=[EDGE_BATCHES[name]], ts=[77], target=4096, misalign=5,
                              flags=3 if views else 0)
    e = fz.expect(c, oracle)
    batch_stages(gpu, lib, c, e, 0, None)


# ---- a damaged input file -------------------------------------------------------------------------------------

def test_damaged_input_file(gpu, lib, oracle):
    """One flipped body bit in a block of the middle file: the compaction names the block, and a compaction of
    the sound files right after it gives the oracle's file (no scratch word is left set)."""
    c, e = prepared(fz.DAMAGED, oracle)
    files = [batch_stages(gpu, lib, c, e, b, None)[0] for b in range(c.k)]
    mid = c.k // 2
    blocks = e.files[mid][1]
    j = len(blocks) // 2
    assert c.k >= 3 and 0 < j < len(blocks) - 1
    off, size, _ = blocks[j]
    bad = files[mid].clone()
    bad[off + 22 + (size - 22) // 2] ^= 0x08
    with pytest.raises(sst.SstCorrupted) as err:
        sst.compact_device(files[:mid] + [bad] + files[mid + 1:], c.target)
    assert err.value.bad_block == j
    assert file_bytes(sst.compact_device(files, c.target)) == e.flat
    assert file_bytes(sst.compact_device(files, c.target, drop_tombstones=True)) == e.dropped


# ---- grown scratch ---------------------------------------------------------------------------------------------

def test_big_small_big(gpu, lib, oracle):
    """The largest seed, the smallest and the largest again in one process: every path's scratch, grown by the
    first, serves the others with stale contents."""
    big, small = prepared(fz.LARGEST, oracle), prepared(fz.SMALLEST, oracle)
    first = pipeline(gpu, lib, *big)
    pipeline(gpu, lib, *small)
    assert pipeline(gpu, lib, *big) == first == big[1].flat


# ---- concurrent callers ----------------------------------------------------------------------------------------

THREADS, ROUNDS = 4, 3


def test_concurrent_callers(gpu, lib, oracle):
    """Four host threads, each on its own stream with its own seed, run the whole pipeline three times over,
    released together: different format paths run at once on one device. The per-device scratch of every path
    is shared under that path's mutex, the `last call` words are thread-local, so every thread must see only
    its own results (batch_stages and pipeline read them after every call)."""
    work = [prepared(s, oracle) for s in fz.THREAD_SEEDS]
    barrier = threading.Barrier(THREADS)
    failures, passes = [], []

    def run(t):
        try:
            torch.cuda.set_device(gpu)
            c, e = work[t]
            stream = torch.cuda.Stream(gpu)
            with torch.cuda.stream(stream):
                barrier.wait(60)
                for rnd in range(ROUNDS):
                    assert pipeline(gpu, lib, c, e, stream) == e.flat
                    passes.append((t, rnd))
        except BaseException as ex:  # noqa: BLE001 - reported by the main thread
            failures.append((t, len([p for p in passes if p[0] == t]), repr(ex)))
            barrier.abort()

    threads = [threading.Thread(target=run, args=(t,), daemon=True) for t in range(THREADS)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(120)
    assert not any(th.is_alive() for th in threads), "a caller is still running after 120 s"
    assert not failures, failures
    assert len(passes) == THREADS * ROUNDS
