"""tkv_sst_merge (the host k-way merge, no GPU) against the dict oracle of tests/sst_merge_util.py: the named
cases of the device tests at a reduced tile, fuzz seeds, every argument error, every kind of bad run, sizing
and overflow with canaries, nullable outputs, empty inputs; the argument errors of tkv_sst_merge_device and
its answer without a GPU; the Python wrappers on numpy arrays."""
import ctypes
import json
import os

import numpy as np
import pytest

import memtable_util as mu
import sst_merge_util as gu
from sst_merge_util import CORRUPTED, INVALID, IO_ERROR, NONE, OK, OVERFLOW
from tinykvpp_amd import sst

T_SMALL = 16  # stands for the device tile in the named cases: the host merge has none
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sst_merge.json")
CASES = gu.named_cases(T_SMALL)


def golden_runs(runs):
    return [[(bytes.fromhex(e["ikey"]), bytes.fromhex(e["value"])) for e in run] for run in runs]


def test_oracle_agrees_with_the_replay_oracle():
    """Valid runs whose internal keys carry one timestamp: the merge oracle's survivors are the memtable
    oracle's over the concatenated records (same user keys, src = the concatenation's index)."""
    for seed in range(6):
        runs, _ = gu.fuzz_case(seed, n_max=300)
        recs, start, at = [], [], 0
        for run in runs:
            start.append(at)
            at += len(run)
            for k, v in run:
                recs.append((0, int.from_bytes(k[-17:-9], "little"), k[:-17], v, k[-1]))
        src = gu.oracle(gu.columns(runs))
        if not recs:
            assert src == []
            continue
        exp = mu.oracle(mu.columns(recs), 0)
        assert [start[r] + i for r, i in src] == exp.src.tolist()
        assert [runs[r][i][0][:-17] for r, i in src] == [recs[j][2] for j in exp.src]


@pytest.mark.parametrize("name", sorted(CASES))
def test_named_cases(lib, name):
    cols = gu.columns(CASES[name])
    for flags in (0, gu.DROP):
        gu.check_merge(lib.tkv_sst_merge, cols, flags)


def test_named_cases_say_what_they_claim():
    t = T_SMALL
    src = gu.oracle(gu.columns(CASES["identical"]))
    assert len(src) == t + 3 and all(r == 1 for r, _ in src)
    assert gu.oracle(gu.columns(CASES["all_equal"])) == [(1, t)]
    for name in ("straddle_3_3", "straddle_5_4", "straddle_1_7"):
        a, b = (int(v) for v in name.split("_")[1:])
        runs = CASES[name]
        users = [[k[:-17] for k, _ in run] for run in runs]
        x = next(u for u in users[1] if users[1].count(u) == b and users[0].count(u) == a)
        # the group of x lies at outputs [T - a, T + b) of the last round: across the tile boundary
        assert sum(u < x for run in users for u in run) == t - a
        last = max(i for i, u in enumerate(users[1]) if u == x)
        assert (1, last) in gu.oracle(gu.columns(runs))
    assert gu.oracle(gu.columns(CASES["all_tombstones"]), True) == []
    assert [r for r, _ in gu.oracle(gu.columns(CASES["metadata_no_part"]))] == [1, 1]
    got = gu.oracle(gu.columns(CASES["tomb_byte_2"]), True)
    assert all(r == 0 for r, _ in got) and len(got) == 5


@pytest.mark.parametrize("seed", range(gu.FUZZ_SEEDS))
def test_fuzz(lib, seed):
    runs, drop = gu.fuzz_case(seed, n_max=600)
    gu.check_merge(lib.tkv_sst_merge, gu.columns(runs, shared=seed % 4 == 1), gu.DROP if drop else 0, misalign=seed % 16)


def test_above_the_host_thread_threshold(lib):
    rng = np.random.default_rng(3)
    runs = gu.overlapping(rng, [9000, 7000, 0, 6000], lo=6, hi=10)
    gu.check_merge(lib.tkv_sst_merge, gu.columns(runs), gu.DROP)


def test_sources(lib):
    rng = np.random.default_rng(4)
    runs = gu.overlapping(rng, [150, 90, 200])
    gu.check_merge(lib.tkv_sst_merge, gu.columns(runs, shared=True))
    gu.check_merge(lib.tkv_sst_merge, gu.columns(runs), below=4096, misalign=5)
    gu.check_merge(lib.tkv_sst_merge, gu.columns(runs), bias=False)
    gu.check_merge(lib.tkv_sst_merge, gu.columns(runs, null_vals=(1,)))
    gu.check_merge(lib.tkv_sst_merge, gu.columns(runs, null_vals=(0, 1, 2)))
    gu.check_merge(lib.tkv_sst_merge, gu.file_columns(lib, runs), misalign=3)


@pytest.mark.parametrize("null", gu.OUT_NAMES)
def test_single_null_output(lib, null):
    rng = np.random.default_rng(5)
    gu.check_merge(lib.tkv_sst_merge, gu.columns(gu.overlapping(rng, [100, 120])), nulls=(null,))


def test_golden_fixture(lib):
    with open(GOLDEN) as f:
        g = json.load(f)
    assert len(g["cases"]) >= 5
    for case in g["cases"]:
        cols = gu.columns(golden_runs(case["runs"]))
        src = gu.check_merge(lib.tkv_sst_merge, cols, gu.DROP if case["drop_tombstones"] else 0)
        assert [list(s) for s in src] == case["src"], case["name"]
    bad = gu.Placed(gu.columns(golden_runs(g["bad_order"]["runs"])))
    outs = gu.Outputs(8)
    r, i = g["bad_order"]["first_bad"]
    assert gu.call(lib.tkv_sst_merge, bad, 0, outs) == (CORRUPTED, 0, 0, 0, r << 32 | i)
    gu.assert_untouched(outs)


def run_corrupt(fn, cols, size, device=None, tail=()):
    placed = gu.Placed(cols, device)
    outs = gu.Outputs(sum(placed.n), device=device)
    res = gu.call(fn, placed, 0, outs, tables=placed.tables(keys_size=size), tail=tail)
    gu.assert_untouched(outs)
    return res


@pytest.mark.parametrize("kind", gu.CORRUPT_KINDS)
def test_corrupted(lib, kind):
    rng = np.random.default_rng(6)
    base = gu.columns(gu.overlapping(rng, [40, 0, 50, 30], lo=2))
    for r, i in ((0, 0), (2, 0), (2, 49), (2, 17), (3, 29)):
        cols, size = gu.corrupt(base, r, i, kind)
        want = gu.first_bad(cols, size)
        assert want != NONE and want >> 32 == r
        assert run_corrupt(lib.tkv_sst_merge, cols, size) == (CORRUPTED, 0, 0, 0, want)
    # two bad runs: the smaller r << 32 | i
    cols, size = gu.corrupt(base, 3, 2, kind)
    cols, size = gu.corrupt(cols, 2, 30, kind)
    want = gu.first_bad(cols, size)
    assert want >> 32 == 2
    assert run_corrupt(lib.tkv_sst_merge, cols, size) == (CORRUPTED, 0, 0, 0, want)


def test_keys_size_is_the_bound(lib):
    cols = gu.columns([gu.make_run([b"a", b"b"], 0)])
    assert run_corrupt(lib.tkv_sst_merge, cols, [cols[0].keys.size - 1]) == (CORRUPTED, 0, 0, 0, 1)


def test_equal_neighbours_are_not_an_order_error(lib):
    gu.check_merge(lib.tkv_sst_merge, gu.columns([gu.make_run([b"a", b"a", b"b", b"b", b"b"], 0)]))


def invalid_rows(placed):
    """(name, kwargs of gu.call) of every TKV_INVALID_ARGUMENT row that keeps the four scalar outputs."""
    t = placed.tables

    def without(j, r=None):
        tb = t()
        if r is None:
            tb[j] = None
        else:
            tb[j][r] = None
        return tb
    rows = [("too_many_runs", dict(k=gu.MAX_RUNS + 1)), ("unknown_flag", dict(flags=2)), ("unknown_flag_high", dict(flags=1 << 31))]
    for j, name in ((0, "d_keys"), (1, "keys_size"), (2, "d_key_off"), (3, "d_key_len"), (6, "n")):
        rows.append((f"null_{name}", dict(tables=without(j))))
    for j, name in ((0, "d_keys"), (2, "d_key_off"), (3, "d_key_len")):
        rows.append((f"null_{name}_element", dict(tables=without(j, 1))))
    rows.append(("val_len_without_val_off", dict(tables=without(4, 0))))
    rows.append(("val_len_without_val_off_array", dict(tables=without(4))))
    tb = t()
    tb[6][1] = 2**32
    rows.append(("run_too_long", dict(tables=tb)))
    tb = t()
    tb[6][0] = tb[6][1] = 2**31
    rows.append(("total_too_long", dict(tables=tb)))
    rows.append(("key_base_above", dict(key_base=min(placed.key_addr) + 1)))
    rows.append(("key_base_null", dict(key_base=0, null_base=True)))
    return rows


def check_invalid(fn, tail=()):
    rng = np.random.default_rng(8)
    placed = gu.Placed(gu.columns(gu.overlapping(rng, [5, 6])))
    for name, kw in invalid_rows(placed):
        outs = gu.Outputs(16)
        flags = kw.pop("flags", 0)
        if kw.pop("null_base", False):
            res = [ctypes.c_uint64(0xDEADBEEF) for _ in range(4)]
            t = placed.tables()
            rc = fn(2, *t[:7], None, t[7], 0, *[outs.ptr(x) for x in gu.OUT_NAMES], 16, *[ctypes.byref(r) for r in res], *tail)
            got = (rc,) + tuple(r.value for r in res)
        else:
            got = gu.call(fn, placed, flags, outs, tail=tail, **kw)
        assert got == (INVALID,) + (0xDEADBEEF,) * 4, name
        gu.assert_untouched(outs)
    # NULL among the four scalar outputs
    t = placed.tables()
    for hole in range(4):
        res = [ctypes.c_uint64(7) for _ in range(4)]
        refs = [None if q == hole else ctypes.byref(r) for q, r in enumerate(res)]
        assert fn(2, *t[:7], ctypes.c_void_p(placed.key_base), t[7], 0, None, None, None, None, None, 0, *refs, *tail) == INVALID
        assert all(r.value == 7 for r in res)
    # the key base is only looked at when out_key_off is written
    outs = gu.Outputs(16, nulls=("key_off",))
    if not tail:
        assert gu.call(fn, placed, 0, outs, key_base=min(placed.key_addr) + 1)[0] == OK


def test_invalid_arguments(lib):
    check_invalid(lib.tkv_sst_merge)


def test_device_call_checks_arguments_before_any_device_work(lib):
    """The same rows through tkv_sst_merge_device on host pointers that are never dereferenced; with sound
    arguments and no GPU it is an I/O error, never the host merge."""
    import torch
    check_invalid(lib.tkv_sst_merge_device, tail=(None,))
    res = [ctypes.c_uint64(5) for _ in range(4)]
    refs = [ctypes.byref(r) for r in res]
    assert lib.tkv_sst_merge_device(0, *[None] * 9, 0, *[None] * 5, 0, *refs, None) == OK
    assert [r.value for r in res] == [0, 0, 0, NONE]
    if not torch.cuda.is_available():
        placed = gu.Placed(gu.columns([gu.make_run([b"a"], 0)]))
        outs = gu.Outputs(4)
        assert gu.call(lib.tkv_sst_merge_device, placed, 0, outs, tail=(None,))[0] == IO_ERROR
        gu.assert_untouched(outs)


def test_sizing_overflow_and_exact(lib):
    rng = np.random.default_rng(9)
    cols = gu.columns(gu.overlapping(rng, [80, 70, 60]))
    src = gu.oracle(cols)
    placed = gu.Placed(cols)
    m = len(src)
    want = gu.expected(placed, src)
    kb, vb = int(want["key_len"].sum()), int(want["val_len"].sum())
    for null in ((), ("key_off", "key_len", "val_off", "val_len")):
        outs = gu.Outputs(m - 1, nulls=null)
        assert gu.call(lib.tkv_sst_merge, placed, 0, outs) == (OVERFLOW, m, kb, vb, NONE)
        gu.assert_untouched(outs)
    outs = gu.Outputs(m + 3)
    assert gu.call(lib.tkv_sst_merge, placed, 0, outs)[:2] == (OK, m)
    assert outs.untouched("src", m) and np.array_equal(outs.get("src", m), want["src"])


def test_empty_inputs(lib):
    outs = gu.Outputs(4)
    assert gu.call(lib.tkv_sst_merge, gu.Placed([]), 0, outs) == (OK, 0, 0, 0, NONE)
    empty = gu.columns([[], [], []])
    assert gu.call(lib.tkv_sst_merge, gu.Placed(empty), gu.DROP, outs) == (OK, 0, 0, 0, NONE)
    gu.assert_untouched(outs)
    # n_runs == 0 with every per-run array NULL
    res = [ctypes.c_uint64(5) for _ in range(4)]
    assert lib.tkv_sst_merge(0, *[None] * 9, 0, *[None] * 5, 0, *[ctypes.byref(r) for r in res]) == OK
    assert [r.value for r in res] == [0, 0, 0, NONE]
    rng = np.random.default_rng(10)
    gu.check_merge(lib.tkv_sst_merge, gu.columns([[]] + gu.overlapping(rng, [30]) + [[], []] + gu.overlapping(rng, [20]) + [[]]))


def test_all_tombstones_writes_nothing(lib):
    cols = gu.columns(CASES["all_tombstones"])
    placed = gu.Placed(cols)
    outs = gu.Outputs(200)
    assert gu.call(lib.tkv_sst_merge, placed, gu.DROP, outs) == (OK, 0, 0, 0, NONE)
    gu.assert_untouched(outs)


def test_python_wrapper(lib):
    rng = np.random.default_rng(11)
    runs = gu.overlapping(rng, [60, 0, 45])
    cols = gu.columns(runs)
    src = gu.oracle(cols)
    got = sst.merge([tuple(c) for c in cols])
    assert got.n_entries == len(src)
    assert got.src.tolist() == [r << 32 | i for r, i in src]
    assert got.entries() == [runs[r][i] for r, i in src]
    dropped = sst.merge([tuple(c) for c in gu.columns(CASES["tomb_mixed"])], drop_tombstones=True)
    want = gu.oracle(gu.columns(CASES["tomb_mixed"]), True)
    assert dropped.entries() == [CASES["tomb_mixed"][r][i] for r, i in want]
    nothing = sst.merge([tuple(c) for c in gu.columns(CASES["all_tombstones"])], drop_tombstones=True)
    assert nothing.n_entries == 0 and nothing.entries() == []
    with pytest.raises(ValueError, match="nothing survives"):
        nothing.flush()
    bad, _ = gu.corrupt(cols, 2, 7, "order")
    with pytest.raises(sst.MergeCorrupted) as e:
        sst.merge([tuple(c) for c in bad])
    assert (e.value.run, e.value.index) == (2, 7)
    with pytest.raises(ValueError):
        sst.merge([tuple(cols[0])] * 65)
