"""The device memtable replay (tkv_memtable_build_device) where the rest of the suite does not take it: the
rounds past the first on lists of more than one workgroup, each radix pass standing alone across
workgroups, the segment passes, stability within a bucket that spans a dozen workgroups, four rounds in a
row (the position lists back in their first buffer) and scans of three levels. Every list is built in
numpy (memtable_util.rounds_cases: every byte misalignment of the key offsets, mixed op, tomb and seq) and
goes through test_gpu_memtable.check_build: the sizing call, then the build into exactly sized canaried
outputs, byte for byte against memtable_util.np_oracle, which tests/test_memtable_oracle_cpu.py holds to
the dict replay. Afterwards tkv_debug_memtable_last and tkv_debug_memtable_passes say whether the path a
list was written for ran: against the numbers stated with each case, and against memtable_util.np_rounds,
the refinement restated from the design text.

Not reached: pass 12 (more than 2^24 segments: at least 2^25 + 2 records), lists of more than 2^24 entries
in rounds 2 and later, more than one GPU."""
import ctypes

import numpy as np
import pytest
import torch

import memtable_util as mu
from test_gpu_memtable import check_build, last, upload

pytestmark = pytest.mark.gpu

SEG = 0x1E00   # passes 9-12: the segment's bytes
WORD = 0x1FE   # passes 1-8: the word's bytes


@pytest.fixture(scope="module")
def geom(lib):
    """(T, B): entries per workgroup of a radix pass and of a scan level."""
    g, e = (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 4)()
    lib.tkv_debug_memtable_geom(g)
    lib.tkv_debug_wal_encode_geometry(e)
    assert (g[1], g[2]) == (256, 13)
    return int(g[0]), int(e[1])


def passes(lib):
    out = (ctypes.c_uint64 * 4)()
    lib.tkv_debug_memtable_passes(out)
    return list(out)


def run(gpu, lib, geom, name):
    """One of rounds_cases through check_build; returns (what make() gave, Columns, Expected, last, passes)
    with the build held to np_rounds: survivors, rounds, the second round's size and all four pass words."""
    make, ts = mu.rounds_cases(*geom)[name]
    made = make()
    c = made if isinstance(made, mu.Columns) else made[0]
    assert set((c.key_off[c.key_len > 0] & 3).tolist()) == {0, 1, 2, 3}
    want = mu.np_oracle(c, ts)
    check_build(gpu, lib, c, ts, misalign=ts % 16, want=want)
    did, ran = last(lib), passes(lib)
    sizes, one, many, count, levels = mu.np_rounds(c, *geom)
    assert did[:3] == [want.src.size, len(sizes), sizes[1] if len(sizes) > 1 else 0]
    assert ran == [one, many, count, levels]
    return made, c, want, did, ran


# ---- a. one pass standing, across workgroups ------------------------------------------------------------

@pytest.mark.parametrize("p", range(9))
def test_one_pass_across_workgroups(gpu, lib, geom, p):
    """2 T + 1 records, three workgroups, the last with one entry, and at most 256 distinct keys: every
    survivor is decided by the scatter's stability across workgroups."""
    _, c, want, did, ran = run(gpu, lib, geom, f"one_pass_{p}")
    assert c.key_len.size == 2 * geom[0] + 1 and want.src.size == (9 if p == 0 else 256)
    assert ran[:3] == [0, 1 << p, 1] and did[1] == 1


def test_digit_pass_alone_in_two_rounds(gpu, lib, geom):
    """Keys of 0-12 zero bytes: pass 0 alone in round 1, and again in a second round of more than T entries
    (written back through a position list)."""
    _, c, want, did, ran = run(gpu, lib, geom, "one_pass_0_len12")
    assert want.src.size == 13 and did[1] == 2 and did[2] == np.count_nonzero(c.key_len > 8) > geom[0]
    assert ran[:3] == [0, 1, 2]


# ---- b. few keys, many workgroups -----------------------------------------------------------------------

def test_few_keys_over_a_dozen_workgroups(gpu, lib, geom):
    """12 T + 5 records over six keys (empty, k, k\\0, 9 bytes, 17 and 20 bytes equal in their first 16):
    the survivors are the last copies, three rounds, each of several workgroups."""
    (_, which), c, want, did, ran = run(gpu, lib, geom, "few_keys")
    assert c.key_len.size == 12 * geom[0] + 5
    by_key = sorted(range(len(mu.FEW_KEYS)), key=lambda i: mu.FEW_KEYS[i])
    assert want.src.tolist() == [int(np.flatnonzero(which == i)[-1]) for i in by_key]
    assert did[1] == 3 and ran[0] == 0 and ran[1] & 1 and ran[1] & WORD


# ---- c. segment passes ----------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", mu.SEGMENT_SHAPES)
def test_segment_passes(gpu, lib, geom, shape):
    """S heads x e tails enter round 2 as S segments from positions scattered through the log: pass 9 runs,
    pass 10 exactly above 256 segments, pass 11 exactly above 65 536; 257 x 2 is the one-workgroup
    counterpart."""
    heads, each = mu.segment_shape(shape, geom[0])
    _, c, want, did, ran = run(gpu, lib, geom, f"segments_{shape}")
    assert did[1] == 2 and did[2] == heads * each == mu.np_shared_first_word(c)
    bits = SEG & (0x200 | (0x400 if heads > 256 else 0) | (0x800 if heads > 65536 else 0))
    if shape == "257x2":
        assert heads * each <= geom[0] and ran[0] & SEG == bits and ran[1] & SEG == 0
    else:
        assert heads * each > geom[0] and ran[1] & SEG == bits


# ---- d. four rounds, each across workgroups -------------------------------------------------------------

def test_four_rounds_across_workgroups(gpu, lib, geom):
    """A tree of 32-byte keys whose lists stay above T through round 4 (the position lists are back in their
    first buffer there), keys that end at 8, 16 and 24 bytes beside longer ones, 33-byte keys for a fifth
    round of one byte, and exact copies far apart in the log."""
    (_, far), c, want, did, ran = run(gpu, lib, geom, "tree")
    longest = int(c.key_len.max())
    assert far >= 200 and want.src.size < c.key_len.size - 250
    assert did[1] == 5 <= (longest + 7) // 8 + 1
    assert ran[1] & SEG and ran[1] & WORD


# ---- e. three scan levels in the rounds -----------------------------------------------------------------

def test_three_scan_levels_in_two_rounds(gpu, lib, geom):
    """B^2 + 2 records that all enter round 2: the tie scan of both rounds and the survivor scans take a
    third level, and round 2 has B^2 / 2 + 1 segments (three segment bytes)."""
    n = geom[1] ** 2 + 2
    assert mu.scan_levels(n, geom[1]) == 3 and mu.scan_levels(n - 2, geom[1]) == 2
    _, c, want, did, ran = run(gpu, lib, geom, "two_tails")
    assert c.key_len.size == n and did[1] == 2 and did[2] == n
    assert ran[0] == 0 and ran[1] & SEG == 0xE00


# ---- f. three levels of the histogram scan --------------------------------------------------------------

@pytest.fixture(scope="module")
def four_byte(gpu, geom):
    """The one large list, T^2 + 1 records, with its oracle and its upload: built once."""
    free = torch.cuda.mem_get_info(gpu)[0]
    if free < 4 << 30:
        pytest.skip(f"{free >> 20} MiB of device memory free: the list of T^2 + 1 records needs 4 GiB")
    make, ts = mu.rounds_cases(*geom)["four_byte"]
    c = make()
    return c, ts, mu.np_oracle(c, ts), upload(gpu, c)


def test_three_levels_of_the_histogram_scan(gpu, lib, geom, four_byte):
    """T^2 + 1 four-byte keys from T^2 / 4 values: the smallest list whose histogram (256 x (T + 1)) has more
    than B^2 entries. One round of the four passes over the key's bytes."""
    c, ts, want, dev = four_byte
    tile, block = geom
    assert c.key_len.size == tile * tile + 1 and mu.scan_levels(256 * (tile + 1), block) == 3 > mu.scan_levels(256 * tile, block)
    assert set((c.key_off & 3).tolist()) == {0, 1, 2, 3}
    check_build(gpu, lib, c, ts, misalign=3, dev_cols=dev, want=want)
    assert last(lib)[:3] == [want.src.size, 1, 0]
    assert passes(lib) == [0, 0x1E0, 4, 3]
