"""tkv_sst_get (the host batched point lookup, no GPU) against the dict oracle of tests/sst_get_util.py: the
named cases, the comparator's and the search's edges, fuzz seeds, every argument error and each verdict's
precedence, sizing and overflow with canaries, nullable outputs, empty inputs, bad spans a search reads and
ones it does not; the argument errors of tkv_sst_get_device and its answer without a GPU; the Python wrappers
on numpy arrays."""
import ctypes
import json
import os

import numpy as np
import pytest

import sst_get_util as tu
import sst_merge_util as gu
from sst_get_util import ABSENT, DELETED, FOUND
from sst_merge_util import CORRUPTED, INVALID, IO_ERROR, NONE, OK, OVERFLOW
from tinykvpp_amd import _lib, sst

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sst_get.json")
CASES = tu.named_cases()
COMPARATOR = tu.comparator_cases()
DUPLICATES = tu.duplicate_cases()


def test_symbols_and_argtypes(lib):
    for name in ("tkv_sst_get", "tkv_sst_get_device", "tkv_debug_sst_get_geometry", "tkv_debug_sst_get_last",
                 "tkv_debug_sst_get_phases"):
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name][1], name
    assert len(lib.tkv_sst_get.argtypes) == 28 and len(lib.tkv_sst_get_device.argtypes) == 29
    assert (sst.GET_ABSENT, sst.GET_FOUND, sst.GET_DELETED) == (ABSENT, FOUND, DELETED) == (0, 1, 2)
    out = (ctypes.c_uint64 * 1)()
    lib.tkv_debug_sst_get_geometry(out)
    assert out[0] >= 64 and out[0] % 64 == 0


def test_oracle_agrees_with_the_merge_oracle():
    """The get oracle's hit for every user key of the union is the merge oracle's survivor of that key."""
    for seed in range(6):
        runs, qs = tu.fuzz_case(seed, n_max=300)
        cols = gu.columns(runs)
        users = tu.users_of(runs)
        src = gu.oracle(cols)
        got = tu.oracle(cols, users)
        assert [(a[1], a[2]) for a in got] == src
        assert all(a[0] == ABSENT for a in tu.oracle(cols, [q for q in qs if q not in set(users)]))


def test_search_model_agrees_with_the_oracle():
    """The contract's probe sequence finds the dict oracle's hits on ascending runs."""
    for seed in range(8):
        runs, qs = tu.fuzz_case(seed, n_max=200)
        cols = gu.columns(runs)
        bad, hits, _ = tu.search_model(cols, qs)
        assert bad == NONE
        assert hits == [None if a[1] is None else (a[1], a[2]) for a in tu.oracle(cols, qs)]


@pytest.mark.parametrize("name", sorted(CASES))
def test_named_cases(lib, name):
    runs, qs = CASES[name]
    tu.check_get(lib.tkv_sst_get, gu.columns(runs), qs)
    tu.check_get(lib.tkv_sst_get, gu.columns(runs), qs, gather=False)


def test_named_cases_say_what_they_claim():
    def states(name):
        runs, qs = CASES[name]
        return [a[0] for a in tu.oracle(gu.columns(runs), qs)]
    assert states("tomb_over_put") == [DELETED, FOUND, DELETED, FOUND, DELETED, ABSENT]
    assert states("put_over_tomb") == [DELETED, FOUND, DELETED, FOUND, DELETED]
    assert states("dup_tomb_last") == [DELETED] and states("dup_put_last") == [FOUND]
    assert states("tomb_byte_ff") == [DELETED, FOUND]
    runs, qs = CASES["seq_no_part"]
    assert tu.oracle(gu.columns(runs), qs)[0][1:] == (1, 0, 0, b"new")
    runs, qs = CASES["dups_in_run"]
    assert [a[2] for a in tu.oracle(gu.columns(runs), qs)] == [0, 3, 5, None]


@pytest.mark.parametrize("name", sorted(COMPARATOR))
def test_comparator_edges(lib, name):
    runs, qs = COMPARATOR[name]
    tu.check_get(lib.tkv_sst_get, gu.columns(runs), qs, misalign=3, qmisalign=5)


@pytest.mark.parametrize("g", (2, 64, 65, 300))
def test_duplicates_highest_index_is_the_hit(lib, g):
    for name in sorted(DUPLICATES):
        if not name.startswith(f"dup_{g}_"):
            continue
        runs, qs = DUPLICATES[name]
        ans = tu.check_get(lib.tkv_sst_get, gu.columns(runs), qs)
        lead = int(name.split("_")[-1])
        assert ans[0][:3] == (FOUND, 0, lead + g - 1)


@pytest.mark.parametrize("n", sorted({1, 2, 3, 63, 64, 65} | {(1 << k) + d for k in range(1, 13) for d in (-1, 0, 1)}))
def test_search_edges(lib, n):
    keys = [b"k%06d" % (2 * i) for i in range(n)]
    runs = [tu.valued_run(keys, 0, sizes=(0, 1, 5))]
    tu.check_get(lib.tkv_sst_get, gu.columns(runs), tu.edge_queries(runs))


@pytest.mark.parametrize("seed", range(tu.FUZZ_SEEDS))
def test_fuzz(lib, seed):
    runs, qs = tu.fuzz_case(seed)
    tu.check_get(lib.tkv_sst_get, gu.columns(runs, shared=seed % 4 == 1, null_vals=(0,) if seed % 5 == 2 else ()), qs,
                 misalign=seed % 16, qmisalign=(seed * 7) % 16, phase=(seed * 3) % 16, gather=seed % 3 != 0)


def test_above_the_host_thread_threshold(lib):
    rng = np.random.default_rng(3)
    runs = gu.overlapping(rng, [9000, 7000, 0, 6000], lo=6, hi=10)
    qs = tu.users_of(runs)
    qs = (qs + [k + b"!" for k in qs])[:20000]
    tu.check_get(lib.tkv_sst_get, gu.columns(runs), qs)


@pytest.mark.parametrize("null", tu.COLS + ("vals",))
def test_single_null_output(lib, null):
    rng = np.random.default_rng(5)
    runs = gu.overlapping(rng, [100, 120])
    tu.check_get(lib.tkv_sst_get, gu.columns(runs), tu.users_of(runs)[:90] + [b"none"], nulls=(null,))


def test_golden_fixture(lib):
    with open(GOLDEN) as f:
        g = json.load(f)
    assert len(g["cases"]) >= 10
    for case in g["cases"]:
        runs = [[(bytes.fromhex(e["ikey"]), bytes.fromhex(e["value"])) for e in run] for run in case["runs"]]
        qs = [bytes.fromhex(q) for q in case["queries"]]
        want = [(a["state"], *(a["src"] or (None, None)), a["seq"], bytes.fromhex(a["value"])) for a in case["answers"]]
        assert tu.check_get(lib.tkv_sst_get, gu.columns(runs), qs) == want, case["name"]
        assert b"".join(a[4] for a in want).hex() == case["vals"]


# ---- errors ---------------------------------------------------------------------------------------------

def base_case():
    rng = np.random.default_rng(6)
    runs = gu.overlapping(rng, [40, 0, 50, 30], lo=2)
    return gu.columns(runs), tu.users_of(runs)


def run_call(fn, cols, qs, keys_size=None, vals_size=None, gather=True, tail=(), outs=None, device=None, **kw):
    placed = gu.Placed(cols, device)
    q = tu.Queries(qs, device)
    outs = tu.Outputs(len(qs), 1 << 16, device=device) if outs is None else outs
    got = tu.call(fn, placed, q, outs, gather, tail=tail, tables=placed.tables(keys_size=keys_size), vals_size=vals_size, **kw)
    return got, outs


@pytest.mark.parametrize("kind", [k for k in gu.CORRUPT_KINDS if k != "order"])
def test_corrupted_probed_entry(lib, kind):
    """A bad span on an entry some search reads: TKV_CORRUPTED, the smallest such r << 32 | i, nothing
    written. Entry 2^(b - 1) - 1 of a run is the first probe of every query that reaches the run."""
    base, qs = base_case()
    for r, i in ((3, 15), (2, 31), (0, 31), (3, 0)):
        cols, size = gu.corrupt(base, r, i, kind)
        want, _, _ = tu.search_model(cols, qs, size)
        assert want != NONE and (r != 3 or want == (r << 32 | i))
        got, outs = run_call(lib.tkv_sst_get, cols, qs, size)
        assert got == (CORRUPTED, 0, 0, want)
        tu.assert_untouched(outs)


@pytest.mark.parametrize("kind", [k for k in gu.CORRUPT_KINDS if k != "order"])
def test_corrupted_unprobed_entry_is_not_read(lib, kind):
    """The same bad span where no search of the batch goes: TKV_OK and the sound answers."""
    base, _ = base_case()
    qs = [b"\xff\xff\xff\xff\xff\xff\xff\xff\xff\xff\xff\xff\xff"]  # above every key: the probes are 2^k - 1 ... n - 1
    cols, size = gu.corrupt(base, 3, 3, kind)
    assert tu.search_model(cols, qs, size)[0] == NONE
    got, outs = run_call(lib.tkv_sst_get, cols, qs, size)
    assert got == (OK, 0, 0, NONE)
    assert outs.get("state", 1)[0] == ABSENT


def test_two_bad_entries_report_the_smallest_read(lib):
    base, qs = base_case()
    cols, size = gu.corrupt(base, 3, 15, "short")
    cols, _ = gu.corrupt(cols, 0, 31, "huge")
    # every query stops at (3, 15), its first probe: (0, 31) is never read
    assert run_call(lib.tkv_sst_get, cols, qs, size)[0] == (CORRUPTED, 0, 0, 3 << 32 | 15)
    # (3, 7) is read by the queries that go left at (3, 15), (2, 31) by every query that run 3 does not
    # answer: both are read, the smaller one is reported
    only, size = gu.corrupt(base, 3, 7, "short")
    assert tu.search_model(only, qs, size)[0] == (3 << 32 | 7)
    cols, _ = gu.corrupt(only, 2, 31, "huge")
    assert tu.search_model(cols, qs, size)[0] == (2 << 32 | 31)
    assert run_call(lib.tkv_sst_get, cols, qs, size)[0] == (CORRUPTED, 0, 0, 2 << 32 | 31)


def test_value_span_of_a_hit_is_checked_with_the_gather_only(lib):
    base, qs = base_case()
    ans = tu.oracle(base, qs)
    j = next(j for j, a in enumerate(ans) if a[0] == FOUND and a[1] == 2)
    r, i = ans[j][1], ans[j][2]
    vsize = [c.vals.size for c in base]
    for what in ("off", "len", "size"):
        cols = [c._replace(val_off=c.val_off.copy(), val_len=c.val_len.copy()) for c in base]
        vs = list(vsize)
        if what == "off":
            cols[r].val_off[i] = vsize[r]
        elif what == "len":
            cols[r].val_len[i] = vsize[r] + 1 - int(cols[r].val_off[i])
        else:
            vs[r] = int(cols[r].val_off[i]) + int(cols[r].val_len[i]) - 1
        assert tu.search_model(cols, qs, vals_size=vs)[0] == (r << 32 | i)
        got, outs = run_call(lib.tkv_sst_get, cols, qs, vals_size=vs)
        assert got == (CORRUPTED, 0, 0, r << 32 | i), what
        tu.assert_untouched(outs)
        # without the gather the span is reported as it stands and no value is read
        outs = tu.Outputs(len(qs), 0, nulls=("vals", "val_pos"))
        got, _ = run_call(lib.tkv_sst_get, cols, qs, vals_size=vs, gather=False, outs=outs)
        assert got[0] == OK and got[3] == NONE
        assert int(outs.get("val_len", len(qs))[j]) == int(cols[r].val_len[i])
        # ... and a batch that does not hit the entry does not trip over it (a smaller arena cuts others too)
        others = [q for k, q in enumerate(qs) if k != j]
        assert what == "size" or run_call(lib.tkv_sst_get, cols, others, vals_size=vs)[0][0] == OK


def test_keys_size_is_the_bound(lib):
    cols = gu.columns([gu.make_run([b"a", b"b"], 0)])
    got, _ = run_call(lib.tkv_sst_get, cols, [b"b"], [cols[0].keys.size - 1])
    assert got == (CORRUPTED, 0, 0, 1)


def bad_query_args(q, kind):
    a = q.args()
    if kind == "past_end":
        a[1] = q.size - 1
    return a


def test_bad_queries_are_invalid_and_go_before_corrupted(lib):
    base, qs = base_case()
    cols, size = gu.corrupt(base, 3, 15, "short")
    placed = gu.Placed(cols)
    # the last query's span reaches past qkeys_size
    q = tu.Queries(qs)
    outs = tu.Outputs(len(qs), 1 << 16)
    got = tu.call(lib.tkv_sst_get, placed, q, outs, tables=placed.tables(keys_size=size), qargs=bad_query_args(q, "past_end"))
    assert got == (INVALID, 0xDEADBEEF, 0xDEADBEEF, 0xDEADBEEF)
    tu.assert_untouched(outs)
    # an offset that wraps, and a length of 2^28 - 17
    for off, ln in ((2**64 - 2, 4), (0, 2**28 - 17)):
        q = tu.Queries(qs)
        o = np.frombuffer((ctypes.c_uint64 * q.nq).from_address(q.off_addr), np.uint64)
        n = np.frombuffer((ctypes.c_uint32 * q.nq).from_address(q.len_addr), np.uint32)
        o[5], n[5] = off, ln
        a = q.args()
        a[1] = 2**30 if ln > 100 else q.size  # (a bound past the length: the length alone is the error)
        got = tu.call(lib.tkv_sst_get, placed, q, outs, tables=placed.tables(keys_size=size), qargs=a)
        assert got == (INVALID, 0xDEADBEEF, 0xDEADBEEF, 0xDEADBEEF), (off, ln)
        tu.assert_untouched(outs)
    # the same runs with sound queries: corrupted
    assert run_call(lib.tkv_sst_get, cols, qs, size)[0] == (CORRUPTED, 0, 0, 3 << 32 | 15)


def check_invalid(fn, tail=()):
    cols, qs = base_case()
    placed = gu.Placed(cols)
    q = tu.Queries(qs)
    outs = tu.Outputs(len(qs), 1 << 16)
    vp = ctypes.c_void_p

    def go(tables=None, k=None, gather=True, flags=0, qargs=None, res=None, outs_=None, vals=True):
        t = placed.tables() if tables is None else tables
        res = [ctypes.c_uint64(0xDEADBEEF) for _ in range(3)] if res is None else res
        kk = placed.k
        v = (vp * kk)(*[a or None for a in placed.val_addr]) if gather else None
        vs = (ctypes.c_uint64 * kk)(*[c.vals.size for c in cols]) if gather and vals else None
        o = outs if outs_ is None else outs_
        refs = [None if r is None else ctypes.byref(r) for r in res]
        rc = fn(kk if k is None else k, *t[:7], v, vs, t[7], *(q.args() if qargs is None else qargs), flags,
                *[o.ptr(name) for name in tu.COLS], o.ptr("vals"), o.vals_cap, *refs, *tail)
        o.fetch()
        tu.assert_untouched(o)
        assert all(r is None or r.value == 0xDEADBEEF for r in res)
        return rc

    assert go(k=65) == INVALID
    assert go(flags=1) == INVALID and go(flags=0x80000000) == INVALID
    for j in range(3):
        res = [ctypes.c_uint64(0xDEADBEEF) for _ in range(3)]
        res[j] = None
        assert go(res=res) == INVALID
    for j in (0, 1, 2, 3, 6):  # d_keys, keys_size, d_key_off, d_key_len, n
        t = placed.tables()
        t[j] = None
        assert go(tables=t) == INVALID, j
    for j in (0, 2, 3):  # a NULL element for a run with entries
        t = placed.tables()
        t[j][2] = None
        assert go(tables=t) == INVALID, j
    t = placed.tables()
    t[4][0] = None  # val_len[0] without val_off[0]
    assert go(tables=t) == INVALID
    t = placed.tables()
    t[6][1] = 2**32
    assert go(tables=t) == INVALID
    t = placed.tables()
    t[6][0] = t[6][2] = 2**31
    assert go(tables=t) == INVALID
    a = q.args()
    for j in (2, 3):  # q_off, q_len
        b = list(a)
        b[j] = None
        assert go(qargs=b) == INVALID
    b = list(a)
    b[0] = None  # qkeys with a size
    assert go(qargs=b) == INVALID
    b = list(a)
    b[4] = 2**32
    assert go(qargs=b) == INVALID
    assert go(vals=False) == INVALID  # d_vals without vals_size
    assert go(gather=False) == INVALID  # out_vals and out_val_pos without d_vals
    assert go(gather=False, outs_=tu.Outputs(len(qs), 0, nulls=("vals",))) == INVALID  # out_val_pos alone
    assert go(gather=False, outs_=tu.Outputs(len(qs), 16, nulls=("val_pos",))) == INVALID  # out_vals alone


def test_invalid_arguments(lib):
    check_invalid(lib.tkv_sst_get)


def test_device_call_checks_arguments_before_any_device_work(lib):
    """The same rows through tkv_sst_get_device on host pointers that are never dereferenced; nq == 0 is
    answered without a device; with sound arguments and no GPU it is an I/O error, never the host get."""
    import torch
    check_invalid(lib.tkv_sst_get_device, tail=(None,))
    res = [ctypes.c_uint64(5) for _ in range(3)]
    refs = [ctypes.byref(r) for r in res]
    assert lib.tkv_sst_get_device(0, *[None] * 11, 0, None, None, 0, 0, *[None] * 7, 0, *refs, None) == OK
    assert [r.value for r in res] == [0, 0, NONE]
    if not torch.cuda.is_available():
        (rc, *_), outs = run_call(lib.tkv_sst_get_device, gu.columns([gu.make_run([b"a"], 0)]), [b"a"], tail=(None,))
        assert rc == IO_ERROR
        tu.assert_untouched(outs)


def test_sizing_overflow_and_exact(lib):
    rng = np.random.default_rng(9)
    runs = [tu.valued_run(gu.distinct_keys(rng, 80), 0, sizes=(3, 0, 17, 100)), tu.valued_run(gu.distinct_keys(rng, 60), 1, sizes=(9,))]
    cols = gu.columns(runs)
    qs = tu.users_of(runs) + [b"nope"]
    _, vals, found = tu.expected(gu.Placed(cols), tu.oracle(cols, qs))
    total = len(vals)
    assert total > 100 and found == len(qs) - 1
    # the sizing call: every output NULL, cap 0
    got, outs = run_call(lib.tkv_sst_get, cols, qs, outs=tu.Outputs(0, 0, nulls=tu.COLS + ("vals",)))
    assert got == (OK, found, total, NONE)
    for cap in (0, 1, total - 1):
        got, outs = run_call(lib.tkv_sst_get, cols, qs, outs=tu.Outputs(len(qs), cap))
        assert got == (OVERFLOW, found, total, NONE), cap
        tu.assert_untouched(outs)
    # a cap too small without d_out_vals is no overflow: the columns are written
    outs = tu.Outputs(len(qs), 0, nulls=("vals",))
    got, _ = run_call(lib.tkv_sst_get, cols, qs, outs=outs)
    assert got == (OK, found, total, NONE) and not outs.untouched("state")
    for phase in (0, 1, 15):
        outs = tu.Outputs(len(qs), total, phase=phase)
        got, _ = run_call(lib.tkv_sst_get, cols, qs, outs=outs)
        assert got == (OK, found, total, NONE) and outs.get("vals", total) == vals and outs.untouched("vals", total)


def test_empty_inputs(lib):
    cols, qs = base_case()
    # nq == 0: sizes 0, nothing else touched
    got, outs = run_call(lib.tkv_sst_get, cols, [], outs=tu.Outputs(4, 16))
    assert got == (OK, 0, 0, NONE)
    tu.assert_untouched(outs)
    # no runs, and only empty runs: every query absent
    for runs in ([], [[], [], []]):
        ans = tu.check_get(lib.tkv_sst_get, gu.columns(runs), qs[:70])
        assert all(a[0] == ABSENT for a in ans)
    got, outs = run_call(lib.tkv_sst_get, gu.columns([]), qs[:3])
    assert got == (OK, 0, 0, NONE)
    assert outs.get("src", 3).tolist() == [NONE] * 3 and outs.get("seq", 3).tolist() == [0] * 3
    # n_runs == 0 with NULL run tables
    res = [ctypes.c_uint64(5) for _ in range(3)]
    q = tu.Queries([b"a"])
    st = np.full(1, 9, np.uint8)
    rc = lib.tkv_sst_get(0, *[None] * 10, *q.args(), 0, st.ctypes.data, *[None] * 6, 0, *[ctypes.byref(r) for r in res])
    assert rc == OK and [r.value for r in res] == [0, 0, NONE] and st[0] == ABSENT


def test_all_absent_and_all_deleted_write_no_value(lib):
    ks = [b"k%03d" % i for i in range(100)]
    runs = [gu.make_run(ks, 0), gu.make_run(ks, 1, tomb=1)]
    ans = tu.check_get(lib.tkv_sst_get, gu.columns(runs), ks)
    assert all(a[0] == DELETED for a in ans)
    ans = tu.check_get(lib.tkv_sst_get, gu.columns(runs), [k + b"x" for k in ks])
    assert all(a[0] == ABSENT for a in ans)


def test_the_same_key_many_times(lib):
    runs = [tu.valued_run([b"a", b"hot", b"z"], 0, sizes=(70, 33, 5))]
    ans = tu.check_get(lib.tkv_sst_get, gu.columns(runs), [b"hot"] * 130 + [b"a", b"nope", b"hot"])
    assert sum(len(a[4]) for a in ans) == 131 * 33 + 70


def test_shared_arenas_and_bias(lib):
    rng = np.random.default_rng(10)
    runs = gu.overlapping(rng, [60, 45, 70])
    qs = tu.users_of(runs)
    tu.check_get(lib.tkv_sst_get, gu.columns(runs, shared=True), qs)
    tu.check_get(lib.tkv_sst_get, gu.columns(runs), qs, bias=False)
    tu.check_get(lib.tkv_sst_get, gu.columns(runs, null_vals=(1,)), qs)


def test_python_wrapper(lib):
    rng = np.random.default_rng(11)
    runs = gu.overlapping(rng, [60, 0, 45])
    runs[2] = gu.make_run([k[:-17] for k, _ in runs[2]], 2, tomb=[i % 3 == 0 for i in range(45)])
    cols = gu.columns(runs)
    qs = tu.users_of(runs) + [b"", b"absent-key"]
    want = tu.oracle(cols, qs)
    tuples = [(c.keys, c.key_off, c.key_len, c.vals, c.val_off, c.val_len) for c in cols]
    for form in (tuples, [dict(zip(("keys", "key_off", "key_len", "vals", "val_off", "val_len"), t)) for t in tuples]):
        res = sst.get(form, qs)
        assert res.n_found == sum(a[0] == FOUND for a in want) and res.vals_bytes == sum(len(a[4]) for a in want)
        assert list(res.items()) == [(a[0], a[4] if a[0] == FOUND else None) for a in want]
        assert res.src.tolist() == [NONE if a[1] is None else a[1] << 32 | a[2] for a in want]
        assert res.seq.tolist() == [a[3] for a in want]
    res = sst.get(tuples, qs, values=False)
    assert res.vals is None and res.val_pos is None and res.vals_bytes == sum(len(a[4]) for a in want)
    assert [s for s, _ in res.items()] == [a[0] for a in want]
    # an (arena, off, len) triple, and a merged run as the only run: the same answers
    arena, off, ln = gu._arena(qs)
    assert list(sst.get(tuples, (arena, off, ln)).items()) == list(sst.get(tuples, qs).items())
    merged = sst.merge(tuples)
    assert list(sst.get([merged], qs).items()) == list(sst.get(tuples, qs).items())
    assert list(sst.get([sst.merge(tuples[:2]), tuples[2]], qs).items()) == list(sst.get(tuples, qs).items())
    bare = [t[:3] + (None, None, None) for t in tuples]  # a merge without a value arena: a value bound of 0
    no_vals = sst.get([sst.merge(bare[:2]), bare[2]], qs)
    assert no_vals.vals_bytes == 0 and [s for s, _ in no_vals.items()] == [a[0] for a in want]
    assert list(sst.get(tuples, []).items()) == []
    bad = [t if r != 2 else (t[0], t[1], np.where(np.arange(45) == 31, 3, t[2]).astype(np.uint32), *t[3:]) for r, t in enumerate(tuples)]
    with pytest.raises(sst.GetCorrupted) as e:
        sst.get(bad, qs)
    assert (e.value.run, e.value.index) == (2, 31)
