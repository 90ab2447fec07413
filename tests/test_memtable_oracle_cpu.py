"""The vectorised memtable oracle (memtable_util.np_oracle) against the dict replay (memtable_util.oracle)
on every list the suite has and on the numpy-built lists of tests/test_gpu_memtable_rounds.py at a few
thousand records, the facts those lists are built for, and the host replay (tkv_memtable_build) against
np_oracle on the full-size lists of up to 150 000 records, with canaried outputs. No GPU."""
import ctypes

import numpy as np
import pytest

import memtable_util as mu

OK = 0
SMALL_TILE, SMALL_BLOCK = 64, 32
HOST_LIMIT = 150_000  # records: the segment lists of 65 537 x 2 with their round-1 keys are 147 458


def assert_same(got, want):
    assert got.ikeys == want.ikeys
    for name in mu.OUT_NAMES[1:]:
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name


def named():
    cases = {f"order_{k}": v for k, v in mu.order_cases().items()}
    cases.update({f"replace_{k}": v for k, v in mu.replacement_cases().items()})
    cases["long_tail"] = mu.long_tail_case()
    return cases


def columns_of(made):
    return made if isinstance(made, mu.Columns) else made[0]


@pytest.mark.parametrize("seed", range(mu.FUZZ_SEEDS))
def test_np_oracle_on_fuzz(seed):
    c, _, ts = mu.fuzz_case(seed)
    assert_same(mu.np_oracle(c, ts), mu.oracle(c, ts))
    assert mu.np_shared_first_word(c) == mu.shared_first_word(c)


@pytest.mark.parametrize("name", sorted(named()))
def test_np_oracle_on_named_cases(name):
    c = mu.columns(named()[name])
    assert_same(mu.np_oracle(c, 77), mu.oracle(c, 77))
    assert mu.np_shared_first_word(c) == mu.shared_first_word(c)


def test_np_oracle_optional_columns_and_bad_op():
    c, _, ts = mu.fuzz_case(9)
    for drop in (("op",), ("tomb",), ("seq",), ("op", "tomb", "seq"), ("val_off", "val_len"), ("val_len",)):
        d = c._replace(**{k: None for k in drop})
        assert_same(mu.np_oracle(d, ts), mu.oracle(d, ts))
    assert_same(mu.np_oracle(c, ts, words=9), mu.oracle(c, ts))  # more words than the longest key needs
    c.op[[700, 31]] = 5
    with pytest.raises(mu.BadOp) as e:
        mu.np_oracle(c)
    assert e.value.index == 31


@pytest.mark.parametrize("name", sorted(mu.rounds_cases(SMALL_TILE, SMALL_BLOCK, small=True)))
def test_np_oracle_on_rounds_cases_small(name):
    make, ts = mu.rounds_cases(SMALL_TILE, SMALL_BLOCK, small=True)[name]
    c = columns_of(make())
    assert c.key_len.size <= 5000
    assert_same(mu.np_oracle(c, ts), mu.oracle(c, ts))
    assert mu.np_shared_first_word(c) == mu.shared_first_word(c)
    sizes = mu.np_rounds(c, SMALL_TILE, SMALL_BLOCK)[0]
    assert sizes[0] == c.key_len.size and (sizes[1] if len(sizes) > 1 else 0) == mu.shared_first_word(c)
    assert len(sizes) <= (int(c.key_len.max()) + 7) // 8 + 1


def geometry(lib):
    g, e = (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 4)()
    lib.tkv_debug_memtable_geom(g)
    lib.tkv_debug_wal_encode_geometry(e)
    return int(g[0]), int(e[1])


def test_rounds_cases_are_what_they_are_for(lib):
    """The full-size lists (all but the two largest) against the sort's geometry: every byte misalignment of
    key_off, mixed columns, and per list the rounds, list sizes and passes it was built to reach."""
    tile, block = geometry(lib)
    assert block * block // 2 + 1 > 65536 * 8  # two_tails: its segments fill three segment bytes
    assert 256 * (tile + 1) > block * block >= 256 * tile  # four_byte: the smallest histogram of three levels
    cases = mu.rounds_cases(tile, block)
    for name, (make, _) in cases.items():
        if name in ("two_tails", "four_byte"):
            continue
        made = make()
        c = columns_of(made)
        n = c.key_len.size
        assert set((c.key_off[c.key_len > 0] & 3).tolist()) == {0, 1, 2, 3}, name
        assert set(c.op.tolist()) == {0, 1} and len(set(c.tomb.tolist())) == 4 and np.unique(c.seq).size > n // 2, name
        sizes, one, many, passes, levels = mu.np_rounds(c, tile, block)
        assert levels == (0 if n <= tile else mu.scan_levels(256 * -(-n // tile), block)) <= 2, name
        if name.startswith("one_pass_") and name != "one_pass_0_len12":
            p = int(name.split("_")[2])
            assert n == 2 * tile + 1 and (sizes, one, many, passes) == ([n], 0, 1 << p, 1), name
            assert mu.np_oracle(c).src.size == (9 if p == 0 else 256), name
        elif name == "one_pass_0_len12":
            assert sizes == [n, int(np.count_nonzero(c.key_len > 8))] and sizes[1] > tile, name
            assert (one, many, passes) == (0, 1, 2), name
        elif name == "few_keys":
            assert n == 12 * tile + 5 and len(sizes) == 3 and min(sizes) > tile and one == 0, name
        elif name.startswith("segments_"):
            heads, each = mu.segment_shape(name[len("segments_"):], tile)
            assert sizes == [n, heads * each] and mu.np_shared_first_word(c) == heads * each, name
            where = one if heads * each <= tile else many
            assert (heads * each <= tile) == (name == "segments_257x2"), name
            assert [bool(where >> b & 1) for b in (9, 10, 11, 12)] == [True, heads > 256, heads > 65536, False], name
            assert n >= sizes[1] + 128 and n <= HOST_LIMIT, name
        elif name == "tree":
            assert len(sizes) == 5 and min(sizes[:4]) > tile and 0 < sizes[4] <= tile, name
            assert int(c.key_len.max()) == 33 and made[1] >= 200, name
            assert {8, 16, 24, 32, 33} == set(c.key_len.tolist()), name
            assert many & 0x1E00 and many & 0x1FE, name
    assert set(cases) == {f"one_pass_{p}" for p in range(9)} | {f"segments_{s}" for s in mu.SEGMENT_SHAPES} | \
        {"one_pass_0_len12", "few_keys", "tree", "two_tails", "four_byte"}


@pytest.mark.parametrize("name", sorted(mu.rounds_cases(SMALL_TILE, SMALL_BLOCK)))
def test_host_variant_against_np_oracle(lib, name):
    """tkv_memtable_build on the full-size lists, called as tests/test_memtable_abi.py calls it. The two
    largest (two_tails at block^2 + 2 and four_byte at tile^2 + 1 records) run at the small geometry."""
    tile, block = geometry(lib)
    full = name not in ("two_tails", "four_byte")
    make, ts = mu.rounds_cases(tile, block)[name] if full else mu.rounds_cases(SMALL_TILE, SMALL_BLOCK)[name]
    c = columns_of(make())
    n = c.key_len.size
    assert n <= HOST_LIMIT
    exp = mu.np_oracle(c, ts)
    sizing = mu.Outputs(0, 0, nulls=mu.OUT_NAMES)
    assert mu.call(lib.tkv_memtable_build, c, ts, sizing, mu.np_ptr) == (OK, exp.src.size, len(exp.ikeys), n)
    outs = mu.Outputs(exp.src.size, len(exp.ikeys), misalign=ts % 16)
    mu.assert_matches(outs, exp, *mu.call(lib.tkv_memtable_build, c, ts, outs, mu.np_ptr), n)
