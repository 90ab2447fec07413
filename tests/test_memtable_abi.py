"""The host memtable replay (tkv_memtable_build: host threads, no GPU) against the sequential oracle of
tests/memtable_util.py on every named case and the fuzz seeds, its sizing / overflow / argument behaviour
with canaried outputs, the committed fixture, and the Python wrappers over it."""
import ctypes
import json
import os

import numpy as np
import pytest

import memtable_util as mu
from tinykvpp_amd import memtable

OK, INVALID, CORRUPTED, OVERFLOW = 0, 3, 4, 7
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "memtable.json")


def check_build(lib, c, ts=0, misalign=0, nulls=()):
    exp = mu.oracle(c, ts)
    n = c.key_len.size
    sizing = mu.Outputs(0, 0, nulls=mu.OUT_NAMES)
    assert mu.call(lib.tkv_memtable_build, c, ts, sizing, mu.np_ptr) == (OK, exp.src.size, len(exp.ikeys), n)
    outs = mu.Outputs(exp.src.size, len(exp.ikeys), misalign=misalign, nulls=nulls)
    mu.assert_matches(outs, exp, *mu.call(lib.tkv_memtable_build, c, ts, outs, mu.np_ptr), n)
    return exp


def named_cases():
    cases = dict(mu.order_cases())
    cases.update(mu.replacement_cases())
    cases["long_tail"] = mu.long_tail_case()
    return cases


@pytest.mark.parametrize("name", sorted(named_cases()))
def test_named_cases(lib, name):
    check_build(lib, mu.columns(named_cases()[name]), ts=77)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 4097, 70001])
def test_counts(lib, n):
    """70 001 records run the sort on host threads (chunks and merges)."""
    rng = np.random.default_rng(1000 + n)
    check_build(lib, mu.columns(mu._recs(mu.random_keys(rng, n))), ts=n)


@pytest.mark.parametrize("seed", range(mu.FUZZ_SEEDS))
def test_fuzz(lib, seed):
    c, _, ts = mu.fuzz_case(seed)
    check_build(lib, c, ts, misalign=seed % 16)


def test_fuzz_covers_what_it_is_for():
    cases = [mu.fuzz_case(s) for s in range(mu.FUZZ_SEEDS)]
    assert sum(1 for s in range(mu.FUZZ_SEEDS) if s % 5 == 0) >= 12
    dup = sum(1 for c, _, _ in cases if mu.oracle(c._replace(op=None)).src.size < c.key_len.size)
    assert dup >= 48
    assert sum(mu.shared_first_word(c) > 0 for c, _, _ in cases) >= 32
    assert any(c.key_len.max() == 40 for c, _, _ in cases) and any(c.key_len.min() == 0 for c, _, _ in cases)


def test_order_statement_of_the_contract(lib):
    keys = [b"\x80", b"a\x01", b"a\x00\x00", b"a\x00", b"a", b""]
    exp = check_build(lib, mu.columns(mu._recs(keys)))
    assert [keys[i] for i in exp.src] == [b"", b"a", b"a\x00", b"a\x00\x00", b"a\x01", b"\x80"]


def test_null_optional_columns(lib):
    rng = np.random.default_rng(5)
    c = mu.columns(mu._recs(mu.random_keys(rng, 300, 6)))
    for drop in (("op",), ("tomb",), ("seq",), ("op", "tomb", "seq"), ("val_off", "val_len"), ("val_len",)):
        check_build(lib, c._replace(**{k: None for k in drop}), ts=9)


@pytest.mark.parametrize("null", mu.OUT_NAMES)
def test_single_null_output(lib, null):
    rng = np.random.default_rng(41)
    check_build(lib, mu.columns(mu._recs(mu.random_keys(rng, 500, 10))), ts=2, nulls=(null,))


def run_error(lib, c, entry_cap=64, ikeys_cap=4096, keys_size=None, nulls=()):
    outs = mu.Outputs(entry_cap, ikeys_cap, nulls=nulls)
    res = mu.call(lib.tkv_memtable_build, c, 0, outs, mu.np_ptr, keys_size=keys_size)
    mu.assert_untouched(outs)
    return res


@pytest.mark.parametrize("bad", [(0,), (20,), (39,), (31, 7)])
def test_bad_op(lib, bad):
    rng = np.random.default_rng(50)
    c = mu.columns(mu._recs(mu.random_keys(rng, 40)))
    for i in bad:
        c.op[i] = 2 + i
    assert run_error(lib, c) == (CORRUPTED, 0, 0, min(bad))


def test_invalid_arguments(lib):
    c = mu.columns(mu._recs([b"abc", b"de", b"fghi"]))
    assert run_error(lib, c, keys_size=c.keys.size - 1)[0] == INVALID
    c.key_off[1] = 2**63
    assert run_error(lib, c)[0] == INVALID
    c = mu.columns(mu._recs([b"abc", b"de"]))
    c.key_len[1] = 2**28 - 17
    assert run_error(lib, c, keys_size=2**29)[0] == INVALID
    c.key_len[1] = 2
    c.op[0] = 9  # an argument error wins over a bad op
    c.key_off[1] = 4
    assert run_error(lib, c)[0] == INVALID
    c = mu.columns(mu._recs([b"a", b"b"]))
    assert run_error(lib, c._replace(val_off=None))[0] == INVALID
    assert run_error(lib, c._replace(key_off=None), nulls=())[0] == INVALID
    res = [ctypes.c_uint64(7) for _ in range(3)]
    p = mu.np_ptr
    args = [p(c.keys), 2, p(c.key_off), p(c.key_len), None, None, None, None, None]
    tail = [0, None, 0, None, None, None, None, None, 0]
    assert lib.tkv_memtable_build(*args, 2**32, *tail, *[ctypes.byref(r) for r in res]) == INVALID
    assert lib.tkv_memtable_build(*args, 2, *tail, None, ctypes.byref(res[1]), ctypes.byref(res[2])) == INVALID
    assert [r.value for r in res] == [7, 7, 7]
    assert lib.tkv_memtable_build(None, 0, None, None, None, None, None, None, None, 0, *tail,
                                  *[ctypes.byref(r) for r in res]) == OK
    assert [r.value for r in res] == [0, 0, 0]


def test_caps_one_short_and_exact(lib):
    rng = np.random.default_rng(51)
    c = mu.columns(mu._recs(mu.random_keys(rng, 200, 5)))
    exp = mu.oracle(c)
    m, size = exp.src.size, len(exp.ikeys)
    assert run_error(lib, c, entry_cap=m - 1, ikeys_cap=size) == (OVERFLOW, m, size, 200)
    assert run_error(lib, c, entry_cap=m, ikeys_cap=size - 1) == (OVERFLOW, m, size, 200)
    check_build(lib, c)


def test_python_wrapper_and_flush_input(lib):
    recs = mu.replacement_cases()["del_after_put"] + mu.replacement_cases()["tomb_bytes"]
    run = memtable.build(recs, timestamp_ms=5)
    exp = mu.oracle(mu.columns(recs), 5)
    assert run.ikeys.tobytes() == exp.ikeys and np.array_equal(run.src, exp.src)
    assert run.entries() == mu.entries(exp, mu.values_arena(recs).tobytes())
    with pytest.raises(memtable.BadOperation) as e:
        memtable.build([(0, 1, b"a", b"", 0), (3, 2, b"b", b"", 0)])
    assert e.value.index == 1
    empty = memtable.build([])
    assert empty.ikey_len.size == 0 and empty.ikeys.size == 0


def test_golden_fixture(lib):
    with open(GOLDEN) as f:
        g = json.load(f)
    recs = [(r["op"], r["seq"], bytes.fromhex(r["key"]), bytes.fromhex(r["value"]), r["tomb"]) for r in g["records"]]
    c = mu.columns(recs)
    exp = check_build(lib, c, ts=g["timestamp_ms"])
    assert exp.ikeys.hex() == g["ikeys"] and exp.src.tolist() == g["src"]
    assert exp.val_len.tolist() == g["val_len"] and exp.ikey_off.tolist() == g["ikey_off"]
