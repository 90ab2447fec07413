"""tkv_wal_decode_host / tkv_wal_decode_device: what can be checked without a GPU. The symbols are
exported and declared, the host decode equals a numpy restatement of wal.cpp:98-125 on the golden
records and on random batches at odd arena alignments, its outputs feed the encode layout back to the
same image, and sizing, overflow, corruption and argument errors leave every output untouched. The same
on 50 000 records, where the header pass, the first_bad minimum and the scatter run on host threads."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import golden
from tinykvpp_amd._lib import BUFFER_OVERFLOW, CORRUPTED, INVALID_ARGUMENT, IO_ERROR, OK, OPTIONAL, SIGNATURES
from wal_decode_util import (COLS, FLAGS, KEY_VIEWS, VAL_VIEWS, HostOut, as_batch, check_host, corrupt, decode_host,
                             expected, first_bad, geometry)
from wal_encode_util import U64, golden_batch, layout_host, make_batch
from wal_encode_util import expected as encoded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tkv_wal_decode_device", "tkv_wal_decode_host", "tkv_debug_wal_decode_geometry", "tkv_debug_wal_decode_last"]


@pytest.fixture(scope="module")
def random_case():
    rng = np.random.default_rng(1201)
    b = make_batch(rng, rng.integers(0, 24, 200), rng.integers(0, 301, 200))
    b["tomb"] = rng.integers(0, 2, 200).astype(np.uint8)
    img, offs, _ = encoded(b)
    return b, img, offs


def test_symbols_and_signatures(lib):
    text = open(os.path.join(ROOT, "include", "tkv_crc32.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), f"libtkv_crc32.so does not export {name}"
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/tkv_crc32.h"
        assert name in SIGNATURES and name in OPTIONAL
        assert len(SIGNATURES[name][1]) == len(m.group(1).split(",")), name
    assert SIGNATURES["tkv_wal_decode_host"][0] is ctypes.c_int and SIGNATURES["tkv_wal_decode_device"][0] is ctypes.c_int
    # the stream and the second offset array
    assert len(SIGNATURES["tkv_wal_decode_device"][1]) == len(SIGNATURES["tkv_wal_decode_host"][1]) + 2
    assert "TKV_WAL_DECODE_KEY_VIEWS 1u" in text and "TKV_WAL_DECODE_VAL_VIEWS 2u" in text


@pytest.mark.parametrize("flags", FLAGS)
def test_golden_records(lib, flags):
    recs = golden("wal.json")["records"]
    raw = [bytes.fromhex(r["hex"]) for r in recs]
    assert len(raw) == 7
    img = np.frombuffer(b"".join(raw), np.uint8).copy()
    offs = np.cumsum([0] + [len(r) for r in raw[:-1]]).astype(np.uint64)
    out, want = check_host(lib, img, offs, flags, kalign=5, valign=11)
    # the expected values against the golden file itself
    assert out.c["op"].tolist() == [r["op"] for r in recs] and out.c["tomb"].tolist() == [r["tombstone"] for r in recs]
    assert out.c["seq"].tolist() == [r["seq"] for r in recs]
    assert out.c["key_len"].tolist() == [len(r["key"]) for r in recs]
    assert out.c["val_len"].tolist() == [len(r["value"]) for r in recs]
    for i, r in enumerate(recs):
        ka = img if flags & KEY_VIEWS else out.arena("keys", want["keys_size"])
        va = img if flags & VAL_VIEWS else out.arena("vals", want["vals_size"])
        ko, vo = int(out.c["key_off"][i]), int(out.c["val_off"][i])
        assert ka[ko:ko + len(r["key"])].tobytes() == r["key"].encode()
        assert va[vo:vo + len(r["value"])].tobytes() == r["value"].encode()


@pytest.mark.parametrize("align", (0, 3, 15))
def test_random_batch(lib, random_case, align):
    b, img, offs = random_case
    for flags in FLAGS:
        out, want = check_host(lib, img, offs, flags, kalign=align, valign=(align * 7 + 1) % 16)
        # the numpy decode against the batch the image was encoded from
        assert np.array_equal(want["key_len"], b["key_len"]) and np.array_equal(want["seq"], b["seq"])
        assert np.array_equal(want["tomb"], b["tomb"]) and np.array_equal(want["op"], b["op"])


@pytest.mark.parametrize("flags", (0, KEY_VIEWS | VAL_VIEWS))
def test_decoded_batch_feeds_the_encode_layout(lib, random_case, flags):
    _, img, offs = random_case
    out, want = check_host(lib, img, offs, flags)
    keys = img if flags & KEY_VIEWS else np.append(out.arena("keys", want["keys_size"]), np.uint8(0))
    vals = img if flags & VAL_VIEWS else np.append(out.arena("vals", want["vals_size"]), np.uint8(0))
    got, size, laid, guard = layout_host(lib, as_batch(out.c, keys, vals))
    zeroed = img.copy()
    zeroed[offs.astype(np.int64)[:, None] + 4 + np.arange(4)] = 0
    assert (got, size) == (offs.size, img.size) and guard
    assert np.array_equal(laid, zeroed)


def test_permuted_offsets_with_a_duplicate(lib, random_case):
    _, img, offs = random_case
    rng = np.random.default_rng(1202)
    p = rng.permutation(offs.size)
    p[17] = p[3]
    for flags in FLAGS:
        check_host(lib, img, offs[p], flags, kalign=9, valign=2)


def test_slack_behind_the_value(lib, random_case):
    """record_len 5 bytes larger than 18 + key_len + val_len: the slack is ignored (wal.cpp:118-125)."""
    b, img, offs = random_case
    at = int(offs[100])
    slack = np.concatenate([img[:int(offs[101])], np.full(5, 0xEE, np.uint8), img[int(offs[101]):]])
    rl = int.from_bytes(slack[at:at + 4].tobytes(), "little") + 5
    slack[at:at + 4] = np.frombuffer(rl.to_bytes(4, "little"), np.uint8)
    o2 = offs.copy()
    o2[101:] += np.uint64(5)
    assert first_bad(slack, o2) == offs.size
    out, want = check_host(lib, slack, o2, 0, kalign=1, valign=6)
    assert np.array_equal(want["val_len"], b["val_len"]) and want["vals_size"] == int(b["val_len"].sum())


def test_delete_only_wal(lib):
    """Every value empty (engine.cpp:39): vals_size == 0 and the value arena may be NULL."""
    rng = np.random.default_rng(1203)
    b = make_batch(rng, rng.integers(1, 24, 60), np.zeros(60, np.int64))
    img, offs, _ = encoded(b)
    want = expected(img, offs)
    out = HostOut(60, want["keys_size"], None)
    assert decode_host(lib, img, offs, 0, out) == (OK, want["keys_size"], 0, 60)
    assert np.array_equal(out.arena("keys", want["keys_size"]), want["keys"]) and not out.c["val_len"].any()
    assert out.guards_ok(want["keys_size"], 0)


def raw_call(lib, device, img, size, off64, off32, n, flags, out, ks, vs, fb):
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    r = lambda v: None if v is None else ctypes.byref(v)  # noqa: E731
    if device:
        return lib.tkv_wal_decode_device(p(img), size, p(off64), p(off32), n, flags, *out.args(), r(ks), r(vs), r(fb), None)
    return lib.tkv_wal_decode_host(p(img), size, p(off64), n, flags, *out.args(), r(ks), r(vs), r(fb))


@pytest.mark.parametrize("device", (False, True))
def test_argument_errors(lib, random_case, device):
    _, img, offs = random_case
    n = offs.size
    o32 = offs.astype(np.uint32)
    out = HostOut(n, 1 << 16, 1 << 16)
    ks, vs, fb = U64(9), U64(9), U64(9)
    call = lambda **kw: raw_call(lib, device, **{**dict(img=img, size=img.size, off64=offs, off32=None, n=n, flags=0,  # noqa: E731
                                                        out=out, ks=ks, vs=vs, fb=fb), **kw})
    assert call(n=1 << 32) == INVALID_ARGUMENT
    assert call(off64=None) == INVALID_ARGUMENT                      # neither offset array
    assert call(flags=4) == INVALID_ARGUMENT and call(flags=1 << 31) == INVALID_ARGUMENT
    assert call(img=None) == INVALID_ARGUMENT
    assert call(ks=None) == INVALID_ARGUMENT and call(vs=None) == INVALID_ARGUMENT and call(fb=None) == INVALID_ARGUMENT
    if device:
        assert call(off32=o32) == INVALID_ARGUMENT                   # both offset arrays
        assert call(off64=None, off32=o32, size=(1 << 32) + 1) == INVALID_ARGUMENT
    assert (ks.value, vs.value, fb.value) == (9, 9, 9)
    assert call(n=0) == OK and (ks.value, vs.value, fb.value) == (0, 0, 0)
    assert out.untouched()


def test_device_call_without_a_gpu_is_an_io_error(lib, random_case):
    """Valid arguments and no usable GPU: TKV_IO_ERROR, never a host decode in its place. (With a GPU the
    device tests cover the call; host pointers are not handed to it.)"""
    if lib.tkv_device_count() > 0:
        return
    _, img, offs = random_case
    out = HostOut(offs.size, 1 << 16, 1 << 16)
    ks, vs, fb = U64(9), U64(9), U64(9)
    assert raw_call(lib, True, img, img.size, offs, None, offs.size, 0, out, ks, vs, fb) == IO_ERROR
    assert out.untouched()


def test_overflow_and_sizing(lib, random_case):
    _, img, offs = random_case
    want = expected(img, offs)
    K, V = want["keys_size"], want["vals_size"]
    for short_k, short_v in ((1, 0), (0, 1)):
        out = HostOut(offs.size, K, V, 3, 8)
        out.kcap -= short_k
        out.vcap -= short_v
        assert decode_host(lib, img, offs, 0, out) == (BUFFER_OVERFLOW, K, V, offs.size)
        assert out.untouched()
    out = HostOut(offs.size, None, None)
    assert decode_host(lib, img, offs, 0, out) == (BUFFER_OVERFLOW, K, V, offs.size) and out.untouched()  # the sizing call
    # a views arena needs no cap
    out = HostOut(offs.size, None, V)
    assert decode_host(lib, img, offs, KEY_VIEWS, out) == (OK, K, V, offs.size)
    out = HostOut(offs.size, None, V)
    out.vcap -= 1
    assert decode_host(lib, img, offs, KEY_VIEWS, out) == (BUFFER_OVERFLOW, K, V, offs.size) and out.untouched()


@pytest.mark.parametrize("kind", ("short", "record_len", "key_len"))
def test_structural_failures(lib, random_case, kind):
    _, img, offs = random_case
    n = offs.size
    for i in (0, n // 2, n - 1):
        bimg, size, boffs = corrupt(kind, img, offs, i)
        assert first_bad(bimg, boffs, size) == i
        for flags in (0, KEY_VIEWS | VAL_VIEWS):
            out = HostOut(n, 1 << 16, 1 << 16, 5, 5)
            assert decode_host(lib, bimg, boffs, flags, out, size=size) == (CORRUPTED, 0, 0, i)
            assert out.untouched()
        if i:  # the prefix decodes
            out = HostOut(i, 1 << 16, 1 << 16)
            assert decode_host(lib, bimg, boffs[:i], 0, out, size=size)[0::3] == (OK, i)


def test_two_bad_records_give_the_smaller_index(lib, random_case):
    _, img, offs = random_case
    bimg, size, boffs = corrupt("record_len", img, offs, 150)
    bimg, size, boffs = corrupt("short", bimg, boffs, 40)
    assert first_bad(bimg, boffs, size) == 40
    out = HostOut(offs.size, 1 << 16, 1 << 16)
    assert decode_host(lib, bimg, boffs, 0, out, size=size) == (CORRUPTED, 0, 0, 40) and out.untouched()


def test_geometry(lib):
    tile, per_wg, lane_max, levels = geometry(lib)
    assert tile > 0 and tile % 16 == 0 and lane_max >= 16
    assert per_wg >= 64 and levels >= 1 and per_wg ** levels >= 1 << 32


def test_python_host_entry(lib, random_case):
    import tinykvpp_amd as tk
    _, img, offs = random_case
    for kv, vv in ((False, False), (True, True)):
        b = tk.wal.decode_batch(img.tobytes(), offs, key_views=kv, val_views=vv)
        want = expected(img, offs, (KEY_VIEWS if kv else 0) | (VAL_VIEWS if vv else 0))
        assert isinstance(b, tk.WalBatch)
        for k in COLS:
            assert np.array_equal(getattr(b, k), want[k]), k
        if not kv:
            assert np.array_equal(b.keys, want["keys"]) and np.array_equal(b.vals, want["vals"])
        else:
            assert np.array_equal(b.keys, img) and np.array_equal(b.vals, img)
    bimg, size, boffs = corrupt("record_len", img, offs, 33)
    with pytest.raises(ValueError, match="record 33"):
        tk.wal.decode_batch(bimg[:size], boffs)


# ---- the threaded branch of the host call (parallel_for goes to host threads at n >= 1 << 14) ---------------

THREADED_N = 50_000


def host_threads():
    """How many threads the library's host loops use: the CPUs this process may run on, capped by
    OMP_NUM_THREADS and 16 (tkv_host_util.h host_threads, restated)."""
    n = min(16, len(os.sched_getaffinity(0)))
    v = os.environ.get("OMP_NUM_THREADS", "")
    if v.strip().lstrip("+").isdigit() and int(v) > 0:
        n = min(n, int(v))
    return max(1, n)


@pytest.fixture(scope="module")
def threaded_case():
    """50 000 records: every per-thread range n t / nt .. n (t + 1) / nt holds thousands of them."""
    if host_threads() < 2:
        pytest.skip("this process may use one CPU: the host loops stay serial")
    rng = np.random.default_rng(1210)
    b = make_batch(rng, rng.integers(0, 24, THREADED_N), rng.integers(0, 65, THREADED_N))
    b["tomb"] = rng.integers(0, 2, THREADED_N).astype(np.uint8)
    img, offs, _ = encoded(b)
    return b, img, offs


@pytest.mark.parametrize("align", (0, 11))
def test_threaded_full_decode(lib, threaded_case, align):
    b, img, offs = threaded_case
    for flags in FLAGS:
        out, want = check_host(lib, img, offs, flags, kalign=align, valign=(align + 6) % 16)
        assert np.array_equal(want["key_len"], b["key_len"]) and np.array_equal(want["seq"], b["seq"])


def test_threaded_permutation_with_a_duplicate(lib, threaded_case):
    _, img, offs = threaded_case
    p = np.random.default_rng(1211).permutation(offs.size)
    p[40_017] = p[3]
    for flags in (0, KEY_VIEWS | VAL_VIEWS):
        check_host(lib, img, offs[p], flags, kalign=9, valign=2)


def test_threaded_bad_records_in_three_ranges(lib, threaded_case):
    """Three bad records in three threads' ranges, the smallest not in the first range: the smallest
    index comes back (the compare-exchange minimum across threads) and nothing is written."""
    _, img, offs = threaded_case
    n, nt = offs.size, host_threads()
    bads = (45_000, 20_000, 33_000) if nt >= 3 else (45_000, 26_000, 33_000)
    assert min(bads) >= n // nt and (nt < 3 or len({b * nt // n for b in bads}) == 3)
    bimg, size, boffs = corrupt("record_len", img, offs, bads[0])
    bimg, size, boffs = corrupt("key_len", bimg, boffs, bads[2])
    bimg, size, boffs = corrupt("short", bimg, boffs, bads[1])
    assert first_bad(bimg, boffs, size) == min(bads)
    for flags in (0, KEY_VIEWS | VAL_VIEWS):
        out = HostOut(n, 1 << 21, 1 << 22, 5, 5)
        assert decode_host(lib, bimg, boffs, flags, out, size=size) == (CORRUPTED, 0, 0, min(bads))
        assert out.untouched()


@pytest.mark.parametrize("where", ("first", "last"))
def test_threaded_only_bad_record_at_an_end(lib, threaded_case, where):
    _, img, offs = threaded_case
    n = offs.size
    i = 0 if where == "first" else n - 1
    bimg, size, boffs = corrupt("record_len", img, offs, i)
    assert first_bad(bimg, boffs, size) == i
    out = HostOut(n, 1 << 21, 1 << 22, 3, 8)
    assert decode_host(lib, bimg, boffs, 0, out, size=size) == (CORRUPTED, 0, 0, i) and out.untouched()


def test_serial_and_threaded_side_by_side(lib, threaded_case):
    """n = 16 383 (one thread) and n = 16 384 (host threads) of the same records."""
    _, img, offs = threaded_case
    for n in ((1 << 14) - 1, 1 << 14):
        for flags in FLAGS:
            check_host(lib, img, offs[:n], flags, kalign=7, valign=1)


def test_threaded_with_three_threads(lib, threaded_case, monkeypatch):
    """An odd thread count: uneven ranges. OMP_NUM_THREADS is only ever lowered."""
    _, img, offs = threaded_case
    if host_threads() > 3:
        monkeypatch.setenv("OMP_NUM_THREADS", "3")
    for flags in FLAGS:
        check_host(lib, img, offs, flags, kalign=13, valign=4)
    bimg, size, boffs = corrupt("record_len", img, offs, 40_000)
    bimg, size, boffs = corrupt("short", bimg, boffs, 17_000)
    out = HostOut(offs.size, 1 << 21, 1 << 22)
    assert decode_host(lib, bimg, boffs, 0, out, size=size) == (CORRUPTED, 0, 0, 17_000) and out.untouched()
