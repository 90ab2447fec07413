"""tkv_sst_build / tkv_sst_build_device: what can be checked without a GPU. The symbols are exported and
declared; the host cut and layout (tkv_debug_sst_build_layout, CRC fields zero) equal the sequential
writer-loop oracle on the golden fixture, 64 fuzz seeds and the cut's and the varints' edges; nothing
outside the destination is touched at any destination alignment; and every argument, sizing and
overflow decision of the host call is made before any GPU use, with the outputs untouched."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

from conftest import golden
from sst_build_util import FUZZ_SEEDS, arenas, call_layout, edge_cases, fuzz_case, oracle_file, unstamped
from tinykvpp_amd import sst
from tinykvpp_amd._lib import BUFFER_OVERFLOW, INVALID_ARGUMENT, OK, OPTIONAL, SIGNATURES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tkv_sst_build_device", "tkv_sst_build", "tkv_debug_sst_build_layout", "tkv_debug_sst_build_geometry",
         "tkv_debug_sst_build_last", "tkv_debug_sst_build_phases"]
GUARD = 64


def test_symbols_and_signatures(lib):
    text = open(os.path.join(ROOT, "include", "tkv_crc32.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), f"libtkv_crc32.so does not export {name}"
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/tkv_crc32.h"
        assert name in SIGNATURES and name in OPTIONAL
        assert len(SIGNATURES[name][1]) == len(m.group(1).split(",")), name
    for name in NAMES[:3]:
        assert SIGNATURES[name][0] is ctypes.c_int
    assert len(SIGNATURES["tkv_sst_build_device"][1]) == len(SIGNATURES["tkv_sst_build"][1]) + 1  # the stream
    assert SIGNATURES["tkv_debug_sst_build_layout"][1] == SIGNATURES["tkv_sst_build"][1]
    geo = (ctypes.c_uint64 * 4)()
    lib.tkv_debug_sst_build_geometry(geo)
    assert geo[0] == 4096 and geo[1] == 1024 and geo[3] == 0
    last = (ctypes.c_uint64 * 4)()
    lib.tkv_debug_sst_build_last(last)
    ms = (ctypes.c_double * 4)(1, 1, 1, 1)
    assert lib.tkv_debug_sst_build_phases(0, ms) == 0 and list(ms) == [0, 0, 0, 0]  # timing is off by default


def check_layout(lib, entries, target, misalign=0, cols=None):
    """The debug layout of ``entries`` at destination misalignment ``misalign`` against the oracle."""
    want, blocks, ioff, isz = oracle_file(entries, target)
    want0 = unstamped(want, blocks)
    cols = arenas(entries) if cols is None else cols
    buf = np.full(GUARD + 16 + len(want) + GUARD, 0xEE, np.uint8)
    start = GUARD + (-(buf.ctypes.data + GUARD) % 16) + misalign
    rc, sizes, (boff, bsize, bfirst) = call_layout(lib, "tkv_debug_sst_build_layout", cols, target,
                                                   buf.ctypes.data + start, len(want), block_cap=len(blocks))
    assert rc == OK
    assert sizes == (len(want), len(blocks), ioff, isz)
    got = buf[start:start + len(want)].tobytes()
    if got != want0:
        bad = next(i for i in range(len(want)) if got[i] != want0[i])
        raise AssertionError(f"file differs from the oracle first at byte {bad} of {len(want)}")
    assert (buf[:start] == 0xEE).all() and (buf[start + len(want):] == 0xEE).all(), "a guard byte changed"
    assert [(int(o), int(s), int(f)) for o, s, f in zip(boff, bsize, bfirst)] == blocks
    return want


def test_golden_fixture(lib, oracle):
    """The fixture is what both constructions give (the writer-loop oracle; the image encoders of
    tinykvpp_amd.sst stamped by the C oracle), and the layout reproduces it with zero CRC fields."""
    doc = golden("sst_build.json")
    assert 3 <= len(doc["cases"]) <= 4
    for c in doc["cases"]:
        entries = [(bytes.fromhex(k), bytes.fromhex(v)) for k, v in c["entries"]]
        target = c["target_block_size"]
        want = bytes.fromhex(c["file"])
        assert oracle_file(entries, target)[0] == want, c["name"]
        # the image encoders, block by block as the index lists them
        idx = sst.read_index(want)
        first = [b[2] for b in oracle_file(entries, target)[1]] + [len(entries)]
        for j, (key, off, size) in enumerate(idx):
            img = bytearray(sst.encode_data_block_image(entries[first[j]:first[j + 1]]))
            struct.pack_into("<I", img, sst.CRC_OFFSET, oracle.sst_stamp(bytes(img)))
            assert want[off:off + size] == bytes(img) and key == entries[first[j]][0], c["name"]
        index = sst.encode_index_image(idx)
        ioff = len(want) - sst.FOOTER_SIZE - len(index)
        foot = sst.encode_footer(ioff, len(index))
        crc = oracle.crc(index + foot[:sst.FOOTER_CRC_OFFSET])
        assert want[ioff:] == index + foot[:sst.FOOTER_CRC_OFFSET] + struct.pack("<I", crc), c["name"]
        assert check_layout(lib, entries, target) == want


@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_layout_fuzz(lib, seed):
    entries, target = fuzz_case(seed)
    rng = np.random.default_rng(seed)
    check_layout(lib, entries, target, misalign=seed % 16, cols=arenas(entries, rng, gaps=seed % 2 == 1))


@pytest.mark.parametrize("name", sorted(edge_cases()))
def test_layout_edges(lib, name):
    entries, target = edge_cases()[name]
    want = check_layout(lib, entries, target)
    if name.startswith("z_"):
        z = int(name[2:])
        assert struct.unpack_from("<I", want, 5)[0] == z
        assert len(oracle_file(entries, target)[1]) == 2
    if name == "exact_T":
        assert [b[2] for b in oracle_file(entries, target)[1]] == [0, 2, 4]
    if name == "T_minus_1":
        assert [b[2] for b in oracle_file(entries, target)[1]] == [0, 3]


def test_layout_many_entries_on_host_threads(lib):
    """Enough entries and blocks that the layout runs on host threads."""
    rng = np.random.default_rng(5)
    blob = rng.integers(0, 256, 4096, dtype=np.uint8).tobytes()
    entries = [(blob[i % 4000:i % 4000 + 9 + i % 5], blob[(7 * i) % 4000:(7 * i) % 4000 + i % 40]) for i in range(40000)]
    check_layout(lib, entries, 64)


@pytest.mark.parametrize("misalign", range(16))
def test_guard_bytes_at_every_destination_alignment(lib, misalign):
    entries, target = fuzz_case(4 + misalign % 3)
    check_layout(lib, entries[:50], target, misalign=misalign)


# ---- argument, sizing and overflow decisions: no GPU is used (this file runs without one) ------------

def untouched(sizes, arrays):
    return all(s == 0xDEADBEEF for s in sizes) and all((a == a.dtype.type(0xA5A5A5A5A5A5A5A5 & (2 ** (8 * a.itemsize) - 1))).all()
                                                       for a in arrays)


@pytest.mark.parametrize("fn", ["tkv_sst_build", "tkv_debug_sst_build_layout"])
def test_invalid_arguments_touch_nothing(lib, fn):
    entries = [(b"key-%d" % i, b"value") for i in range(10)]
    cols = arenas(entries)
    want = oracle_file(entries, 64)[0]
    buf = np.full(len(want) + 32, 0xEE, np.uint8)

    def call(c, target=64, cap=len(want)):
        rc, sizes, arrays = call_layout(lib, fn, c, target, buf.ctypes.data, cap)
        assert (buf == 0xEE).all()
        return rc, sizes, arrays

    empty = tuple(a[:0] if i % 3 else a for i, a in enumerate(cols))
    for c, target in ((empty, 64),                                     # n == 0
                      (cols, 0),                                       # target_block_size == 0
                      ((None,) + cols[1:], 64), (cols[:1] + (None,) + cols[2:], 64),
                      (cols[:2] + (None,) + cols[3:], 64),             # keys, key_off, key_len
                      (cols[:3] + (None,) + cols[4:], 64), (cols[:4] + (None, cols[5]), 64)):  # vals, val_off with val_len
        if c[2] is None:  # call_layout takes n from key_len
            p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731
            s4 = [ctypes.c_uint64(0xDEADBEEF) for _ in range(4)]
            rc = getattr(lib, fn)(p(c[0]), p(c[1]), None, p(c[3]), p(c[4]), p(c[5]), 10, target, ctypes.c_void_p(buf.ctypes.data),
                                  len(want), None, None, None, 0, *[ctypes.byref(s) for s in s4])
            assert rc == INVALID_ARGUMENT and all(s.value == 0xDEADBEEF for s in s4) and (buf == 0xEE).all()
            continue
        rc, sizes, arrays = call(c, target)
        assert rc == INVALID_ARGUMENT and untouched(sizes, arrays), (target, [a is None for a in c])
    # a NULL size output, and n beyond u32 (decided before any array is read: the arrays hold 10 entries)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    s4 = [ctypes.c_uint64(0xDEADBEEF) for _ in range(4)]
    for k in range(4):
        outs = [ctypes.byref(s) for s in s4]
        outs[k] = None
        rc = getattr(lib, fn)(*[p(a) for a in cols], 10, 64, p(buf), len(want), None, None, None, 0, *outs)
        assert rc == INVALID_ARGUMENT and all(s.value == 0xDEADBEEF for s in s4) and (buf == 0xEE).all()
    rc = getattr(lib, fn)(*[p(a) for a in cols], 2 ** 32, 64, p(buf), len(want), None, None, None, 0,
                          *[ctypes.byref(s) for s in s4])
    assert rc == INVALID_ARGUMENT and all(s.value == 0xDEADBEEF for s in s4) and (buf == 0xEE).all()
    # val_len == NULL is not an error: every value is empty
    if fn == "tkv_debug_sst_build_layout":
        keys_only, blocks = oracle_file([(k, b"") for k, _ in entries], 64)[:2]
        rc, sizes, _ = call_layout(lib, fn, cols[:3] + (None, None, None), 64, buf.ctypes.data, len(buf))
        assert rc == OK and buf[:sizes[0]].tobytes() == unstamped(keys_only, blocks)


@pytest.mark.parametrize("fn", ["tkv_sst_build", "tkv_debug_sst_build_layout"])
def test_lengths_of_2_28_are_invalid_and_no_source_byte_is_read(lib, fn):
    """A length >= 2^28 over a one-byte arena: were a source byte read, the call would run off the arena."""
    tiny = np.zeros(1, np.uint8)
    buf = np.full(64, 0xEE, np.uint8)
    for klen, vlen in ((2 ** 28, 0), (0, 2 ** 28), (2 ** 32 - 1, 3), (5, 2 ** 31)):
        cols = (tiny, np.zeros(3, np.uint64), np.array([0, klen, 0], np.uint32),
                tiny, np.zeros(3, np.uint64), np.array([0, vlen, 0], np.uint32))
        rc, sizes, arrays = call_layout(lib, fn, cols, 4096, buf.ctypes.data, 64)
        assert rc == INVALID_ARGUMENT and untouched(sizes, arrays) and (buf == 0xEE).all()
    # 2^28 - 1 is a valid length: the sizing call accepts it (and still reads no source byte)
    cols = (tiny, np.zeros(1, np.uint64), np.array([2 ** 28 - 1], np.uint32), tiny, np.zeros(1, np.uint64), np.zeros(1, np.uint32))
    rc, sizes, _ = call_layout(lib, fn, cols, 4096, None, 0, with_blocks=False)
    z = 8 + 2 ** 28 - 1
    assert rc == BUFFER_OVERFLOW and sizes == (36 + z + 8 + 4 + 2 ** 28 - 1 + 16 + 20, 1, 36 + z, 8 + 4 + 2 ** 28 - 1 + 16)


@pytest.mark.parametrize("fn", ["tkv_sst_build", "tkv_debug_sst_build_layout"])
def test_block_and_file_beyond_u32_are_invalid(lib, fn):
    """Many entries sharing one (never read) source span: with T = 2^32 - 1 a block's 36 + z_j passes
    u32; with a smaller T every block fits but the file does not."""
    tiny = np.zeros(1, np.uint8)
    n, ln = 40, 2 ** 27
    cols = (tiny, np.zeros(n, np.uint64), np.full(n, ln, np.uint32), tiny, np.zeros(n, np.uint64), np.zeros(n, np.uint32))
    buf = np.full(64, 0xEE, np.uint8)
    for target in (2 ** 32 - 1, 2 ** 30):
        rc, sizes, arrays = call_layout(lib, fn, cols, target, buf.ctypes.data, 2 ** 40)
        assert rc == INVALID_ARGUMENT and untouched(sizes, arrays) and (buf == 0xEE).all()
    # 31 such entries: z = 31 * (2^27 + 8) < 2^32 - 36 in one block, but index and footer push the file past u32
    m = 31
    c31 = tuple(a[:m] if a.size == n else a for a in cols)
    rc, sizes, arrays = call_layout(lib, fn, c31, 2 ** 32 - 1, buf.ctypes.data, 2 ** 40)
    z = m * (ln + 8)
    assert 36 + z <= 2 ** 32 - 1 < 36 + z + 8 + 4 + ln + 16 + 20
    assert rc == INVALID_ARGUMENT and untouched(sizes, arrays) and (buf == 0xEE).all()


@pytest.mark.parametrize("fn", ["tkv_sst_build", "tkv_debug_sst_build_layout"])
def test_sizing_and_overflow(lib, fn):
    entries, target = fuzz_case(2)
    want, blocks, ioff, isz = oracle_file(entries, target)
    cols = arenas(entries)
    full = (len(want), len(blocks), ioff, isz)
    # the sizing call
    rc, sizes, _ = call_layout(lib, fn, cols, target, None, 0, with_blocks=False)
    assert rc == BUFFER_OVERFLOW and sizes == full
    buf = np.full(len(want) + 32, 0xEE, np.uint8)
    # one byte short, one block short: the sizes are reported and nothing is written
    for cap, bcap in ((len(want) - 1, len(blocks)), (len(want), len(blocks) - 1)):
        rc, sizes, arrays = call_layout(lib, fn, cols, target, buf.ctypes.data, cap, block_cap=bcap)
        assert rc == BUFFER_OVERFLOW and sizes == full
        assert (buf == 0xEE).all() and untouched((), arrays)
    # too few block entries do not matter when no block array is asked for; exact caps succeed
    if fn == "tkv_debug_sst_build_layout":
        rc, sizes, _ = call_layout(lib, fn, cols, target, buf.ctypes.data, len(want), block_cap=0, with_blocks=False)
        assert rc == OK and sizes == full and buf[:len(want)].tobytes() == unstamped(want, blocks)
        rc, sizes, arrays = call_layout(lib, fn, cols, target, buf.ctypes.data, len(want), block_cap=len(blocks))
        assert rc == OK and [int(x) for x in arrays[2][:len(blocks)]] == [b[2] for b in blocks]
        assert (buf[len(want):] == 0xEE).all()


def test_read_index_round_trip_and_corruption():
    entries, target = fuzz_case(7)
    want, blocks, ioff, isz = oracle_file(entries, target)
    idx = sst.read_index(want)
    assert [(o, s) for _, o, s in idx] == [(o, s) for o, s, _ in blocks]
    assert [k for k, _, _ in idx] == [entries[f][0] for _, _, f in blocks]
    assert sst.read_index(np.frombuffer(want, np.uint8)) == idx
    for pos in (ioff, ioff + 9, len(want) - 20, len(want) - 13, len(want) - 1):
        bad = bytearray(want)
        bad[pos] ^= 0x10
        with pytest.raises(ValueError):
            sst.read_index(bytes(bad))
    with pytest.raises(ValueError):
        sst.read_index(want[:-1])
