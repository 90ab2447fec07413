"""The device memtable replay (tkv_memtable_build_device) against the sequential oracle of
tests/memtable_util.py, byte for byte, with canaries on both sides of every output: launch edges, the
comparator's edges, replacement, sources and destinations, errors, fuzz, the recover -> replay -> flush
pipeline, threads and the phase clock."""
import ctypes
import threading

import numpy as np
import pytest
import torch

import memtable_util as mu
import wal_fuzz_util as fz
from sst_build_util import oracle_file
from tinykvpp_amd import memtable, sst, wal

pytestmark = pytest.mark.gpu

OK, INVALID, CORRUPTED, OVERFLOW = 0, 3, 4, 7


def upload(gpu, c):
    """A Columns of numpy arrays as one of CUDA tensors (None stays None)."""
    def dev(a):
        if a is None:
            return None
        if a.dtype != np.uint8:
            a = a.view(a.dtype.str.replace("u", "i"))
        return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return mu.Columns(*[dev(a) for a in c])


def dptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def last(lib):
    out = (ctypes.c_uint64 * 4)()
    lib.tkv_debug_memtable_last(out)
    return list(out)


def check_build(gpu, lib, c, ts=0, misalign=0, nulls=(), dev_cols=None, want=None, stream=None):
    """The sizing call, then the build into exactly sized canaried outputs; returns the Expected."""
    exp = mu.oracle(c, ts) if want is None else want
    d = upload(gpu, c) if dev_cols is None else dev_cols
    n = c.key_len.size
    st = ctypes.c_void_p(stream.cuda_stream if stream is not None else torch.cuda.current_stream(gpu).cuda_stream)
    sizing = mu.Outputs(0, 0, nulls=mu.OUT_NAMES).to(gpu)
    rc, m, size, bad = mu.call(lib.tkv_memtable_build_device, d, ts, sizing, dptr, stream=st)
    assert (rc, m, size, bad) == (OK, exp.src.size, len(exp.ikeys), n), lib.tkv_last_error()
    outs = mu.Outputs(m, size, misalign=misalign, nulls=nulls).to(gpu)
    res = mu.call(lib.tkv_memtable_build_device, d, ts, outs, dptr, stream=st)
    mu.assert_matches(outs, exp, *res, n)
    return exp


# ---- counts and launch edges ----------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 4096, 4097, 70001])
def test_counts(gpu, lib, n):
    """4096 entries is the longest list one workgroup sorts alone; 70 001 crosses 2^16 and spans several."""
    rng = np.random.default_rng(1000 + n)
    recs = mu._recs(mu.random_keys(rng, n))
    check_build(gpu, lib, mu.columns(recs), ts=n)


def test_n_zero(gpu, lib):
    outs = mu.Outputs(4, 64).to(gpu)
    res = [ctypes.c_uint64(77) for _ in range(3)]
    rc = lib.tkv_memtable_build_device(None, 0, None, None, None, None, None, None, None, 0, 5, outs.ptr("ikeys"), 64,
                                       outs.ptr("ikey_off"), outs.ptr("ikey_len"), outs.ptr("val_off"), outs.ptr("val_len"),
                                       outs.ptr("src"), 4, *[ctypes.byref(r) for r in res], None)
    outs.fetch()
    assert rc == OK and [r.value for r in res] == [0, 0, 0]
    mu.assert_untouched(outs)


# ---- order edges ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(mu.order_cases()))
def test_order_edges(gpu, lib, name):
    check_build(gpu, lib, mu.columns(mu.order_cases()[name]), ts=3)


def test_long_keys_differ_in_last_byte(gpu, lib):
    """130 keys of 1000 bytes that differ in the last byte only: one round per word, no more, and all of
    them enter the second round."""
    c = mu.columns(mu.long_tail_case())
    exp = check_build(gpu, lib, c)
    assert exp.src.size == 130
    m, rounds, second, scratch = last(lib)
    assert m == 130 and scratch > 0
    assert rounds <= (1000 + 7) // 8 + 1
    assert second == mu.shared_first_word(c) == 130


# ---- replacement edges ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(mu.replacement_cases()))
def test_replacement_edges(gpu, lib, name):
    recs = mu.replacement_cases()[name]
    c = mu.columns(recs)
    exp = check_build(gpu, lib, c, ts=1)
    if name == "all_equal":
        assert exp.src.tolist() == [len(recs) - 1]
    if name == "lower_seq_survives":
        assert exp.src.tolist() == [2, 1]
    if name == "del_after_put":
        assert exp.val_len.tolist() == [1, 0] and c.val_len[1] == 13
    if name.startswith("twice_gap_"):
        assert np.all(exp.val_len == 7)  # every survivor is a second copy


def test_null_optional_columns(gpu, lib):
    rng = np.random.default_rng(5)
    c = mu.columns(mu._recs(mu.random_keys(rng, 300, 6)))
    for drop in (("op",), ("tomb",), ("seq",), ("op", "tomb", "seq"), ("val_off", "val_len"), ("val_len",)):
        check_build(gpu, lib, c._replace(**{k: None for k in drop}), ts=9)


# ---- sources and destinations ---------------------------------------------------------------------------

def test_keys_as_views_into_a_wal_image(gpu, lib, oracle):
    """The columns of decode_device under both view flags: keys are unaligned spans of the WAL image."""
    rng = np.random.default_rng(17)
    img, offs, _ = fz.build(rng, oracle, "tiny", 2000)
    image = torch.from_numpy(img).to(gpu)
    b = wal.decode_device(image, torch.from_numpy(offs.astype(np.int64)).to(gpu), key_views=True, val_views=True)
    c = mu.Columns(img, *[t.cpu().numpy().view(dt) for t, dt in ((b.key_off, np.uint64), (b.key_len, np.uint32),
                                                                 (b.val_off, np.uint64), (b.val_len, np.uint32),
                                                                 (b.op, np.uint8), (b.tomb, np.uint8), (b.seq, np.uint64))])
    d = mu.Columns(b.keys, b.key_off, b.key_len, b.val_off, b.val_len, b.op, b.tomb, b.seq)
    check_build(gpu, lib, c, ts=4, dev_cols=d)


def test_overlapping_views(gpu, lib):
    c, _, ts = mu.fuzz_case(5)  # a views case
    assert c.key_off.size > len(set(c.key_off.tolist()))
    check_build(gpu, lib, c, ts)


@pytest.mark.parametrize("misalign", range(16))
def test_arena_misalignment(gpu, lib, misalign):
    rng = np.random.default_rng(40)
    c = mu.columns(mu._recs(mu.random_keys(rng, 700, 90)))  # keys on both sides of the lane / wave copy limit
    check_build(gpu, lib, c, ts=2, misalign=misalign)


@pytest.mark.parametrize("null", mu.OUT_NAMES)
def test_single_null_output(gpu, lib, null):
    rng = np.random.default_rng(41)
    c = mu.columns(mu._recs(mu.random_keys(rng, 500, 10)))
    check_build(gpu, lib, c, ts=2, nulls=(null,))


# ---- errors ---------------------------------------------------------------------------------------------

def run_error(gpu, lib, c, entry_cap=64, ikeys_cap=4096, keys_size=None, nulls=()):
    outs = mu.Outputs(entry_cap, ikeys_cap, nulls=nulls).to(gpu)
    res = mu.call(lib.tkv_memtable_build_device, upload(gpu, c), 0, outs, dptr, keys_size=keys_size,
                  stream=ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream))
    mu.assert_untouched(outs)
    return res


@pytest.mark.parametrize("bad", [(0,), (20,), (39,), (31, 7)])
def test_bad_op(gpu, lib, bad):
    rng = np.random.default_rng(50)
    c = mu.columns(mu._recs(mu.random_keys(rng, 40)))
    for i in bad:
        c.op[i] = 2 + i
    with pytest.raises(mu.BadOp) as e:
        mu.oracle(c)
    assert e.value.index == min(bad)
    assert run_error(gpu, lib, c) == (CORRUPTED, 0, 0, min(bad))


def test_key_past_keys_size(gpu, lib):
    c = mu.columns(mu._recs([b"abc", b"de", b"fghi"]))
    assert run_error(gpu, lib, c, keys_size=c.keys.size - 1)[0] == INVALID
    c.key_off[1] = 2**63  # and an offset that would wrap
    assert run_error(gpu, lib, c)[0] == INVALID


def test_key_too_long_for_the_flush(gpu, lib):
    """key_len = 2^28 - 17 is refused by the check, which reads no key byte: a sizing-only call."""
    c = mu.columns(mu._recs([b"abc", b"de"]))
    c.key_len[1] = 2**28 - 17
    assert run_error(gpu, lib, c, entry_cap=0, ikeys_cap=0, keys_size=2**29, nulls=mu.OUT_NAMES)[0] == INVALID


def test_caps_one_short_and_exact(gpu, lib):
    rng = np.random.default_rng(51)
    c = mu.columns(mu._recs(mu.random_keys(rng, 200, 5)))
    exp = mu.oracle(c)
    m, size = exp.src.size, len(exp.ikeys)
    assert m < 200
    assert run_error(gpu, lib, c, entry_cap=m - 1, ikeys_cap=size) == (OVERFLOW, m, size, 200)
    assert run_error(gpu, lib, c, entry_cap=m, ikeys_cap=size - 1) == (OVERFLOW, m, size, 200)
    # a cap that is short for an array that is NULL does not count
    outs = mu.Outputs(m, size - 1, nulls=("ikeys",)).to(gpu)
    res = mu.call(lib.tkv_memtable_build_device, upload(gpu, c), 0, outs, dptr,
                  stream=ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream))
    mu.assert_matches(outs, exp, *res, 200)
    check_build(gpu, lib, c)  # exact


def test_argument_errors_before_device_work(gpu, lib):
    c = upload(gpu, mu.columns(mu._recs([b"a", b"b"])))
    res = [ctypes.c_uint64(7) for _ in range(3)]
    refs = [ctypes.byref(r) for r in res]
    f = lib.tkv_memtable_build_device
    out = [None, 0, None, None, None, None, None, 0]
    ins = lambda **kw: [dptr(kw.get("keys", c.keys)), 2, dptr(kw.get("key_off", c.key_off)), dptr(kw.get("key_len", c.key_len)),  # noqa: E731
                        dptr(kw.get("val_off", c.val_off)), dptr(c.val_len), None, None, None, kw.get("n", 2), 0]
    assert f(*ins(n=2**32), *out, *refs, None) == INVALID
    assert f(*ins(key_off=None), *out, *refs, None) == INVALID
    assert f(*ins(key_len=None), *out, *refs, None) == INVALID
    assert f(*ins(keys=None), *out, *refs, None) == INVALID
    assert f(*ins(val_off=None), *out, *refs, None) == INVALID
    assert f(*ins(), *out, None, refs[1], refs[2], None) == INVALID
    assert [r.value for r in res] == [7, 7, 7]


# ---- fuzz -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(mu.FUZZ_SEEDS))
def test_fuzz(gpu, lib, seed):
    c, recs, ts = mu.fuzz_case(seed)
    exp = check_build(gpu, lib, c, ts, misalign=seed % 16)
    run = memtable.build_host_columns(c.keys, c.key_off, c.key_len, c.val_off, c.val_len, c.op, c.tomb, c.seq, ts)
    assert run.ikeys.tobytes() == exp.ikeys and np.array_equal(run.src, exp.src)
    assert np.array_equal(run.val_off, exp.val_off) and np.array_equal(run.val_len, exp.val_len)


# ---- pipeline -------------------------------------------------------------------------------------------

def test_recover_replay_flush(gpu, lib, oracle):
    """A WAL image through recover_device, build_device and flush: the file is the oracle writer's over the
    oracle's entries, and scanning it gives the dict's keys in strictly ascending order."""
    rng = np.random.default_rng(31)
    img, offs, _ = fz.build(rng, oracle, "mixed", 3000)
    image = torch.from_numpy(img).to(gpu)
    status, batch, stop, _ = wal.recover_device(image)
    assert status == "ok" and stop == img.size and batch.key_len.numel() == offs.size
    run = memtable.build_device(batch, timestamp_ms=1234567)
    assert run.vals.data_ptr() == batch.vals.data_ptr()
    host = [t.cpu().numpy() for t in batch]
    c = mu.Columns(host[7], host[3].view(np.uint64), host[4].view(np.uint32), host[5].view(np.uint64), host[6].view(np.uint32),
                   host[0], host[1], host[2].view(np.uint64))
    exp = mu.oracle(c, 1234567)
    assert run.ikeys.cpu().numpy().tobytes() == exp.ikeys
    assert np.array_equal(run.src.cpu().numpy().view(np.uint32), exp.src)
    want = mu.entries(exp, host[8].tobytes())
    assert run.entries() == want
    table = run.flush()
    assert table.file.cpu().numpy().tobytes() == oracle_file(want, 4096)[0]
    scanned = sst.scan_device(table.file)
    user = [k[:-mu.META] for k, _ in scanned.entries()]
    assert all(a < b for a, b in zip(user, user[1:]))
    raw = host[7].tobytes()
    assert user == sorted({raw[int(o):int(o) + int(ln)] for o, ln in zip(c.key_off, c.key_len)})
    assert [v for _, v in scanned.entries()] == [v for _, v in want]


def test_format_scratch_grows_and_is_reused(gpu, lib, oracle):
    """The five format paths keep per-device scratch between calls, grown by doubling through one shared
    piece of code. In one process on one device: encode -> decode -> memtable build -> flush -> scan on 3
    records, on 1025 (one more than a scan block: every array regrows and every scan takes a second level),
    and on the 3 again in the grown scratch. Every stage against its sequential oracle, every time."""
    import sst_scan_util as su
    import wal_decode_util as wd
    from wal_encode_util import DeviceBatch, expected, make_batch

    rng = np.random.default_rng(2027)

    def case(n):
        b = make_batch(rng, rng.integers(8, 24, n), rng.integers(0, 41, n))  # random keys of 8+ bytes: distinct
        b["op"] = rng.integers(0, 2, n, dtype=np.uint8)
        return b, DeviceBatch(b, gpu).t, expected(b, oracle)

    small, large = case(3), case(1025)
    for b, t, (img, offs, crc) in (small, large, small):
        n = b["n"]
        image, rec_off, c = wal.encode_device(t["keys"], t["key_off"], t["key_len"], t["vals"], t["val_off"], t["val_len"],
                                              t["op"], t["tomb"], t["seq"])
        assert np.array_equal(image.cpu().numpy(), img)
        assert np.array_equal(rec_off.cpu().numpy().view(np.uint64), offs)
        assert np.array_equal(c.cpu().numpy().view(np.uint32), crc)

        batch = wal.decode_device(image, rec_off)
        dec = wd.expected(img, offs)
        wd.compare({k: getattr(batch, k).cpu().numpy().view(wd.DTYPES[k]) for k in wd.COLS}, batch.keys.cpu().numpy(),
                   batch.vals.cpu().numpy(), dec)

        run = memtable.build_device(batch, timestamp_ms=n)
        exp = mu.oracle(mu.Columns(dec["keys"], dec["key_off"], dec["key_len"], dec["val_off"], dec["val_len"], dec["op"],
                                   dec["tomb"], dec["seq"]), n)
        assert exp.src.size == n == last(lib)[0]
        assert run.ikeys.cpu().numpy().tobytes() == exp.ikeys
        assert np.array_equal(run.src.cpu().numpy().view(np.uint32), exp.src)
        want = mu.entries(exp, dec["vals"].tobytes())
        assert run.entries() == want

        table = run.flush()
        file_bytes, blocks, _, _ = oracle_file(want, 4096)
        assert table.file.cpu().numpy().tobytes() == file_bytes
        assert table.block_off.cpu().tolist() == [x[0] for x in blocks]

        scanned = sst.scan_device(table.file)
        status, _, ents, sblocks = su.oracle_scan(file_bytes)
        assert status == "ok" and ents == want
        assert scanned.entries() == ents
        assert [list(x) for x in zip(scanned.block_off.cpu().tolist(), scanned.block_size.cpu().numpy().view(np.uint32).tolist(),
                                     scanned.block_first.cpu().numpy().view(np.uint32).tolist())] == [list(x) for x in sblocks]


# ---- threads --------------------------------------------------------------------------------------------

def test_four_threads_build_at_once(gpu, lib):
    """Four host threads, each on its own stream with its own input, released together: the per-device
    scratch and the pinned result block are shared under the library's mutex, the `last build` words are
    thread-local."""
    work = []
    for t in range(4):
        c, _, ts = mu.fuzz_case(21 + t)
        work.append((c, ts, mu.oracle(c, ts)))
    barrier = threading.Barrier(4)
    failures, passes = [], []

    def run(t):
        try:
            c, ts, want = work[t]
            stream = torch.cuda.Stream(gpu)
            with torch.cuda.stream(stream):
                d = upload(gpu, c)
                stream.synchronize()
                barrier.wait(60)
                for rnd in range(3):
                    check_build(gpu, lib, c, ts, misalign=(5 * t + rnd) % 16, dev_cols=d, want=want, stream=stream)
                    assert last(lib)[0] == want.src.size
                    passes.append((t, rnd))
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            failures.append((t, repr(e)))
            barrier.abort()

    threads = [threading.Thread(target=run, args=(t,), daemon=True) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(120)
    assert not any(th.is_alive() for th in threads), "a caller is still running after 120 s"
    assert not failures, failures
    assert len(passes) == 12


# ---- phase times ----------------------------------------------------------------------------------------

def test_phase_times_zero_unless_enabled(gpu, lib):
    rng = np.random.default_rng(60)
    c = mu.columns(mu._recs(mu.random_keys(rng, 5000, 12)))
    ms = (ctypes.c_double * 4)()
    prev = lib.tkv_debug_memtable_phases(0, None)
    try:
        check_build(gpu, lib, c)
        lib.tkv_debug_memtable_phases(1, ms)
        assert list(ms) == [0.0] * 4
        check_build(gpu, lib, c)
        lib.tkv_debug_memtable_phases(0, ms)
        assert all(v >= 0.0 for v in ms) and sum(ms) > 0.0
        check_build(gpu, lib, c)
        lib.tkv_debug_memtable_phases(0, ms)
        assert list(ms) == [0.0] * 4
    finally:
        lib.tkv_debug_memtable_phases(prev, None)
