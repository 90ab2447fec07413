"""tkv_wal_encode / tkv_wal_encode_device: what can be checked without a GPU. The symbols are exported
and declared, the host layout step (CRC fields zero) equals a numpy restatement of wal.cpp:19-61 and the
golden records (also at 50 000 records, laid out on host threads), and sizing, overflow and argument
errors are decided before any device work."""
import ctypes
import os
import re

import numpy as np

import tinykvpp_amd as tk
from conftest import golden
from tinykvpp_amd._lib import BUFFER_OVERFLOW, INVALID_ARGUMENT, OK, OPTIONAL, SIGNATURES
from wal_encode_util import U64, expected, geometry, golden_batch, guarded, host_args, make_batch, sentinels_ok

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tkv_wal_encode_device", "tkv_wal_encode", "tkv_debug_wal_encode_layout", "tkv_debug_wal_encode_geometry",
         "tkv_debug_wal_encode_last", "tkv_debug_set_wal_encode_fused"]


def test_symbols_and_signatures(lib):
    text = open(os.path.join(ROOT, "include", "tkv_crc32.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), f"libtkv_crc32.so does not export {name}"
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/tkv_crc32.h"
        assert name in SIGNATURES and name in OPTIONAL
        assert len(SIGNATURES[name][1]) == len(m.group(1).split(",")), name
    assert SIGNATURES["tkv_wal_encode"][0] is ctypes.c_int and SIGNATURES["tkv_wal_encode_device"][0] is ctypes.c_int
    assert len(SIGNATURES["tkv_wal_encode_device"][1]) == len(SIGNATURES["tkv_wal_encode"][1]) + 1  # the stream


def layout(lib, b, cap=None):
    total = int(expected(b)[0].size)
    buf, start = guarded(total, 3)
    size = U64(0)
    got = lib.tkv_debug_wal_encode_layout(*host_args(b), ctypes.c_void_p(buf.ctypes.data + start),
                                          total if cap is None else cap, ctypes.byref(size))
    assert sentinels_ok(buf, start, total)
    return got, size.value, buf[start:start + total].copy()


def test_layout_golden(lib):
    b, raw = golden_batch(golden("wal.json")["records"])
    assert len(raw) == 7
    want = b"".join(r[:4] + b"\0\0\0\0" + r[8:] for r in raw)
    got, size, img = layout(lib, b)
    assert (got, size) == (7, len(want))
    assert img.tobytes() == want
    assert np.array_equal(img, expected(b)[0])


def test_layout_random(lib):
    rng = np.random.default_rng(81)
    b = make_batch(rng, rng.integers(0, 24, 200), rng.integers(0, 301, 200))
    want = expected(b)[0]
    got, size, img = layout(lib, b)
    assert (got, size) == (200, want.size)
    assert np.array_equal(img, want)
    recs = [tk.wal.encode_unstamped(int(b["op"][i]), int(b["seq"][i]),
                                    b["keys"][int(b["key_off"][i]):int(b["key_off"][i]) + int(b["key_len"][i])].tobytes(),
                                    b["vals"][int(b["val_off"][i]):int(b["val_off"][i]) + int(b["val_len"][i])].tobytes(),
                                    int(b["tomb"][i])) for i in range(200)]
    assert img.tobytes() == b"".join(recs)
    # the defaults: no values, op / tombstone 0, seq = first_seq + i
    d = dict(b, val_len=None, op=None, tomb=None, seq=None, first_seq=1 << 40)
    got, size, img = layout(lib, d)
    assert np.array_equal(img, expected(d)[0]) and got == 200
    assert layout(lib, b, cap=want.size - 1)[:2] == (0, want.size)  # too small: nothing laid out, the size reported


def test_sizing_without_gpu(lib):
    rng = np.random.default_rng(82)
    b = make_batch(rng, rng.integers(0, 24, 50), rng.integers(0, 65, 50))
    total = int(expected(b)[0].size)
    size = U64(0)
    assert lib.tkv_wal_encode(*host_args(b), None, 0, None, None, ctypes.byref(size)) == BUFFER_OVERFLOW
    assert size.value == total


def test_record_len_overflow_is_invalid(lib):
    rng = np.random.default_rng(83)
    b = make_batch(rng, [3, 4, 5], [1, 2, 3])
    b["key_len"] = np.array([3, 0xFFFFFFF0, 5], np.uint32)
    b["val_len"] = np.array([1, 0x100, 3], np.uint32)
    buf, start = guarded(4096)
    size = U64(7)
    rc = lib.tkv_wal_encode(*host_args(b), ctypes.c_void_p(buf.ctypes.data + start), 4096, None, None, ctypes.byref(size))
    assert rc == INVALID_ARGUMENT and (buf == 0xA5).all()
    assert lib.tkv_debug_wal_encode_layout(*host_args(b), ctypes.c_void_p(buf.ctypes.data + start), 4096,
                                           ctypes.byref(size)) == 0 and (buf == 0xA5).all()


def test_argument_errors_both_entry_points(lib):
    rng = np.random.default_rng(84)
    b = make_batch(rng, [3, 4], [1, 2])
    buf, start = guarded(256)
    img = ctypes.c_void_p(buf.ctypes.data + start)
    size = U64(0)
    S = ctypes.byref(size)
    good = host_args(b)
    calls = (lambda a, s: lib.tkv_wal_encode(*a, img, 256, None, None, s),
             lambda a, s: lib.tkv_wal_encode_device(*a, img, 256, None, None, s, None))
    for call in calls:
        for k in (0, 1, 2):  # keys, key_off, key_len
            a = list(good)
            a[k] = None
            assert call(a, S) == INVALID_ARGUMENT
        for k in (3, 4):     # vals / val_off with val_len
            a = list(good)
            a[k] = None
            assert call(a, S) == INVALID_ARGUMENT
        assert call(good, None) == INVALID_ARGUMENT  # no img_size
        a = list(good)
        a[10] = 1 << 32
        assert call(a, S) == INVALID_ARGUMENT        # n > 2^32 - 1
        a[10] = 0
        size.value = 9
        assert call(a, S) == OK and size.value == 0   # n = 0 touches nothing else
    assert (buf == 0xA5).all()


def test_geometry(lib):
    tile, per_wg, fold_max, levels = geometry(lib)
    assert tile > 0 and tile % 16 == 0
    assert fold_max >= 240
    assert per_wg >= 64 and levels >= 1 and per_wg ** levels >= 1 << 32
    assert lib.tkv_debug_set_wal_encode_fused(1) == 1  # the default


def test_layout_on_host_threads(lib):
    """The layout at 50 000 records and on either side of 16 384 (parallel_for goes to host threads at
    n >= 1 << 14; with one usable CPU both branches are the serial one): explicit columns, and all the
    defaults (no values, op / tombstone 0, seq = first_seq + i)."""
    rng = np.random.default_rng(85)
    n = 50_000
    b = make_batch(rng, rng.integers(0, 24, n), rng.integers(0, 65, n))
    for m in (n, (1 << 14) - 1, 1 << 14):
        part = dict(b, n=m, **{k: b[k][:m] for k in ("key_off", "key_len", "val_off", "val_len", "op", "tomb", "seq")})
        for d in (part, dict(part, val_len=None, op=None, tomb=None, seq=None, first_seq=1 << 40)):
            want = expected(d)[0]
            got, size, img = layout(lib, d)
            assert (got, size) == (m, want.size)
            bad = np.flatnonzero(img != want)
            assert bad.size == 0, f"n = {m}: the image differs in {bad.size} bytes, first at {bad[0]}"
