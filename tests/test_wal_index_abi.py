"""tkv_wal_index / tkv_wal_index_device: what can be checked without a GPU. Both symbols are exported
with the header's signatures, every argument error is reported before any device work, and an empty
image is TKV_OK with all outputs zero."""
import ctypes
import os
import re

import tinykvpp_amd as tk
from tinykvpp_amd._lib import INVALID_ARGUMENT, OK, SIGNATURES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = ctypes.c_uint64
DUMMY = ctypes.c_void_p(16)  # never dereferenced: the argument checks come first

# C parameter type -> the ctypes type _lib.py must declare for it
CTYPES = {"const uint8_t *": ctypes.c_void_p, "uint64_t": U64, "uint64_t *": (ctypes.c_void_p, ctypes.POINTER(U64)),
          "uint32_t *": ctypes.c_void_p, "void *": ctypes.c_void_p}


def header_params(name):
    text = open(os.path.join(ROOT, "include", "tkv_crc32.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/tkv_crc32.h"
    out = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        out.append(re.sub(r"\s*\w+$", "", p).strip())  # the type: the declarator without its name
    return out


def test_symbols_and_signatures(lib):
    want = {
        "tkv_wal_index_device": ["const uint8_t *", "uint64_t", "uint64_t *", "uint32_t *", "uint64_t", "uint64_t *",
                                 "uint64_t *", "uint64_t *", "void *"],
        "tkv_wal_index": ["const uint8_t *", "uint64_t", "uint64_t *", "uint64_t", "uint64_t *", "uint64_t *",
                          "uint64_t *"],
    }
    for name, params in want.items():
        assert hasattr(lib, name), f"libtkv_crc32.so does not export {name}"
        assert header_params(name) == params
        res, args = SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params)
        for a, p in zip(args, params):
            ok = CTYPES[p]
            assert a in ok if isinstance(ok, tuple) else a is ok, (name, p, a)


def outs():
    return U64(7), U64(7), U64(7)


def test_index_device_argument_errors(lib):
    f = lib.tkv_wal_index_device
    g, s, m = outs()
    G, S, M = ctypes.byref(g), ctypes.byref(s), ctypes.byref(m)
    assert f(DUMMY, 100, DUMMY, None, 4, None, S, M, None) == INVALID_ARGUMENT   # no n_good
    assert f(DUMMY, 100, DUMMY, None, 4, G, None, M, None) == INVALID_ARGUMENT   # no stop_offset
    assert f(DUMMY, 100, DUMMY, None, 4, G, S, None, None) == INVALID_ARGUMENT   # no max_sequence
    assert f(None, 100, DUMMY, None, 4, G, S, M, None) == INVALID_ARGUMENT       # no image
    assert f(DUMMY, 100, None, None, 4, G, S, M, None) == INVALID_ARGUMENT       # cap > 0, no offsets array
    assert f(DUMMY, (1 << 32) + 1, None, DUMMY, 4, G, S, M, None) == INVALID_ARGUMENT  # u32 offsets over 4 GiB
    assert f(DUMMY, (1 << 32) + 1, DUMMY, DUMMY, 4, G, S, M, None) == INVALID_ARGUMENT
    assert b"4 GiB" in lib.tkv_last_error()
    assert (g.value, s.value, m.value) == (7, 7, 7)  # results untouched by a rejected call


def test_index_host_argument_errors(lib):
    f = lib.tkv_wal_index
    g, s, m = outs()
    G, S, M = ctypes.byref(g), ctypes.byref(s), ctypes.byref(m)
    assert f(DUMMY, 100, DUMMY, 4, None, S, M) == INVALID_ARGUMENT
    assert f(DUMMY, 100, DUMMY, 4, G, None, M) == INVALID_ARGUMENT
    assert f(DUMMY, 100, DUMMY, 4, G, S, None) == INVALID_ARGUMENT
    assert f(None, 100, DUMMY, 4, G, S, M) == INVALID_ARGUMENT
    assert f(DUMMY, 100, None, 4, G, S, M) == INVALID_ARGUMENT  # cap > 0, no offsets array


def test_empty_image_is_ok_and_zero(lib):
    for call in (lambda G, S, M: lib.tkv_wal_index_device(None, 0, None, None, 0, G, S, M, None),
                 lambda G, S, M: lib.tkv_wal_index_device(DUMMY, 0, DUMMY, DUMMY, 9, G, S, M, None),
                 lambda G, S, M: lib.tkv_wal_index(None, 0, None, 0, G, S, M),
                 lambda G, S, M: lib.tkv_wal_index(DUMMY, 0, DUMMY, 9, G, S, M)):
        g, s, m = outs()
        assert call(ctypes.byref(g), ctypes.byref(s), ctypes.byref(m)) == OK
        assert (g.value, s.value, m.value) == (0, 0, 0)
    status, offs, stop, seq = tk.wal.index(b"")
    assert (status, offs.size, stop, seq) == ("ok", 0, 0, 0)
