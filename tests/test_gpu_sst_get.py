"""The device SSTable get (tkv_sst_get_device) against the dict oracle of tests/sst_get_util.py and the host
call, with canaries on both sides of every output: the search's and the comparator's edges, duplicates,
runs, launch edges, alignments, the value gather, errors, the equivalence with the merge, the pipeline,
threads and the debug hooks."""
import ctypes
import json
import os
import threading

import numpy as np
import pytest
import torch

import memtable_util as mu
import sst_get_util as tu
import sst_merge_util as gu
from sst_build_util import oracle_file
from sst_get_util import ABSENT, DELETED, FOUND
from sst_merge_util import CORRUPTED, INVALID, NONE, OK, OVERFLOW
from tinykvpp_amd import load_library, memtable, sst, wal

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sst_get.json")
COMPARATOR = tu.comparator_cases()
DUPLICATES = tu.duplicate_cases()
TILE = 4096  # bytes per tile of the shared arena emit


def geometry(lib):
    out = (ctypes.c_uint64 * 1)()
    lib.tkv_debug_sst_get_geometry(out)
    return int(out[0])


W = geometry(load_library())


def stream_of(gpu):
    return (ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream),)


def check(gpu, lib, cols, qs, **kw):
    return tu.check_get(lib.tkv_sst_get_device, cols, qs, device=gpu, tail=stream_of(gpu), also=lib.tkv_sst_get, **kw)


def last(lib):
    out = (ctypes.c_uint64 * 5)()
    lib.tkv_debug_sst_get_last(out)
    return list(out)


def run_call(gpu, lib, cols, qs, keys_size=None, vals_size=None, gather=True, outs=None, **kw):
    placed = gu.Placed(cols, gpu)
    q = tu.Queries(qs, gpu)
    outs = tu.Outputs(len(qs), 1 << 16, device=gpu) if outs is None else outs
    got = tu.call(lib.tkv_sst_get_device, placed, q, outs, gather, tail=stream_of(gpu), tables=placed.tables(keys_size=keys_size),
                  vals_size=vals_size, **kw)
    return got, outs


def test_golden_fixture(gpu, lib):
    with open(GOLDEN) as f:
        g = json.load(f)
    for case in g["cases"]:
        runs = [[(bytes.fromhex(e["ikey"]), bytes.fromhex(e["value"])) for e in run] for run in case["runs"]]
        qs = [bytes.fromhex(q) for q in case["queries"]]
        want = [(a["state"], *(a["src"] or (None, None)), a["seq"], bytes.fromhex(a["value"])) for a in case["answers"]]
        assert check(gpu, lib, gu.columns(runs), qs) == want, case["name"]


# ---- search edges -----------------------------------------------------------------------------------------

SIZES = sorted({1, 2, 3, 63, 64, 65} | {(1 << k) + d for k in range(1, 13) for d in (-1, 0, 1)})


@pytest.mark.parametrize("n", SIZES)
def test_search_edges_every_run_size(gpu, lib, n):
    """A run of n entries, n = 1 .. 2^12 + 1 around every power of two: every present key, a key below the
    first, one above the last and one between each pair of neighbours (2 n + 1 queries)."""
    runs = [tu.valued_run([b"k%06d" % (2 * i) for i in range(n)], 0, sizes=(0, 1, 5))]
    qs = tu.edge_queries(runs)
    assert len(qs) == 2 * n + 1
    ans = check(gpu, lib, gu.columns(runs), qs)
    assert [a[2] for a in ans[:n]] == list(range(n)) and all(a[0] == ABSENT for a in ans[n:])
    assert last(lib)[:3] == [len(qs), 1, n.bit_length()]


@pytest.mark.parametrize("name", sorted(COMPARATOR))
def test_comparator_edges(gpu, lib, name):
    runs, qs = COMPARATOR[name]
    check(gpu, lib, gu.columns(runs), qs, misalign=3, qmisalign=5)


@pytest.mark.parametrize("g", (2, 64, 65, 300))
def test_duplicates_highest_index_is_the_hit(gpu, lib, g):
    for name in sorted(DUPLICATES):
        if not name.startswith(f"dup_{g}_"):
            continue
        runs, qs = DUPLICATES[name]
        ans = check(gpu, lib, gu.columns(runs), qs)
        assert ans[0][:3] == (FOUND, 0, int(name.split("_")[-1]) + g - 1)


# ---- runs -------------------------------------------------------------------------------------------------

def k_case(rng, sizes, tombs=()):
    pool = gu.distinct_keys(rng, max(sizes) + sum(sizes) // 3 + 1)
    runs = []
    for r, n in enumerate(sizes):
        ks = sorted(pool[j] for j in rng.choice(len(pool), n, replace=False))
        runs.append(tu.valued_run(ks, r, sizes=(3, 0, 20), tomb=rng.choice(np.array([0, 0, 1, 0xFF]), n).tolist() if r in tombs else 0))
    return runs, pool


@pytest.mark.parametrize("sizes", ([300], [200, 150], [0, 120, 0, 77, 300], [0] * 5),
                         ids=("k1", "k2", "k5_some_empty", "k5_all_empty"))
def test_k_runs(gpu, lib, sizes):
    rng = np.random.default_rng(60)
    runs, pool = k_case(rng, sizes, tombs=(1, 3))
    check(gpu, lib, gu.columns(runs), pool + [b""])


def test_k64(gpu, lib):
    rng = np.random.default_rng(61)
    sizes = [int(x) for x in np.where(rng.random(64) < 0.3, 0, rng.integers(1, 120, 64))]
    runs, pool = k_case(rng, sizes, tombs=range(0, 64, 3))
    ans = check(gpu, lib, gu.columns(runs), pool)
    assert len({a[1] for a in ans if a[1] is not None}) > 20  # the hits come from many runs


def test_tombstone_over_value_and_the_inverse(gpu, lib):
    ks = [b"k%03d" % i for i in range(100)]
    ans = check(gpu, lib, gu.columns([tu.valued_run(ks, 0, sizes=(4,)), gu.make_run(ks[::2], 1, tomb=1)]), ks)
    assert [a[0] for a in ans] == [DELETED, FOUND] * 50
    ans = check(gpu, lib, gu.columns([gu.make_run(ks, 0, tomb=0xFF), tu.valued_run(ks[::2], 1, sizes=(4,))]), ks)
    assert [a[0] for a in ans] == [FOUND, DELETED] * 50


def test_one_wave_finishes_in_different_runs(gpu, lib):
    """64 queries of one wave: query j is answered by run j % 5 (runs of different sizes), every eighth by
    none. The step count of the hook is that of a lane that went through all five."""
    sizes = [40, 7, 130, 1, 64]
    keys = [[b"r%d-%04d" % (r, i) for i in range(n)] for r, n in enumerate(sizes)]
    runs = [tu.valued_run(ks, r, sizes=(2,)) for r, ks in enumerate(keys)]
    qs = [b"zz-none" if j % 8 == 7 else keys[j % 5][(j * 3) % sizes[j % 5]] for j in range(64)]
    ans = check(gpu, lib, gu.columns(runs), qs)
    assert {a[1] for a in ans} == {0, 1, 2, 3, 4, None}
    assert last(lib) == [64, 5, tu.steps_of(sizes), 56, 0]


def test_step_count_of_the_longest_lane(gpu, lib):
    """Runs of 1000, 0, 17 and 300 entries. A batch answered by the newest run makes bit_length(300) steps;
    one query that only run 0 answers makes the steps of all three."""
    sizes = [1000, 0, 17, 300]
    keys = [[b"r%d-%04d" % (r, i) for i in range(n)] for r, n in enumerate(sizes)]
    cols = gu.columns([gu.make_run(ks, r) for r, ks in enumerate(keys)])
    check(gpu, lib, cols, keys[3][::7])
    assert last(lib)[:3] == [len(keys[3][::7]), 4, tu.steps_of([300])]
    check(gpu, lib, cols, keys[3][::7] + [keys[2][5]])
    assert last(lib)[2] == tu.steps_of([300, 17])
    check(gpu, lib, cols, keys[3][::7] + [keys[0][999]] + keys[2][:3])
    assert last(lib)[2:] == [tu.steps_of([300, 17, 1000]), len(keys[3][::7]) + 4, 0]
    assert tu.search_model(cols, [keys[0][999]])[2] == tu.steps_of(sizes)


# ---- launch edges -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("nq", sorted({1, 63, 64, 65, W - 1, W, W + 1, 3 * W + 1}))
def test_query_counts(gpu, lib, nq):
    rng = np.random.default_rng(62)
    runs, pool = k_case(rng, [500, 300], tombs=(1,))
    qs = [pool[j] for j in rng.integers(0, len(pool), nq)]
    check(gpu, lib, gu.columns(runs), qs)
    assert last(lib)[0] == nq


def test_no_queries(gpu, lib):
    rng = np.random.default_rng(63)
    runs, _ = k_case(rng, [50], ())
    got, outs = run_call(gpu, lib, gu.columns(runs), [], outs=tu.Outputs(4, 16, device=gpu))
    assert got == (OK, 0, 0, NONE)
    tu.assert_untouched(outs)


# ---- alignment --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("phase", range(16))
def test_every_arena_and_query_phase(gpu, lib, phase):
    rng = np.random.default_rng(64)
    runs = gu.overlapping(rng, [90, 70], lo=0, hi=30)
    qs = tu.users_of(runs)
    qs += [q + b"\x00" for q in qs[:30]]
    check(gpu, lib, gu.columns(runs), qs, misalign=phase, qmisalign=0, phase=phase)
    check(gpu, lib, gu.columns(runs, shared=True), qs, misalign=5, qmisalign=phase, phase=(phase * 7) % 16)


def test_runs_as_views_from_the_device_scan_of_a_misaligned_file(gpu, lib):
    rng = np.random.default_rng(65)
    runs = [r for r in gu.overlapping(rng, [400, 250, 330]) if r]
    tables = []
    for k, run in enumerate(runs):
        image = np.frombuffer(oracle_file(run, 512)[0], np.uint8)
        buf = torch.zeros(image.size + 16, dtype=torch.uint8, device=gpu)
        view = buf[3 + 4 * k:3 + 4 * k + image.size]
        view.copy_(torch.from_numpy(image.copy()))
        tables.append(sst.scan_device(view, key_views=True, val_views=True))
        assert tables[-1].keys.data_ptr() % 16 == 3 + 4 * k
    qs = tu.users_of(runs) + [b"", b"\xff" * 9]
    want = tu.oracle(gu.columns(runs), qs)
    res = sst.get_device(tables, qs)
    assert list(res.items()) == [(a[0], a[4] if a[0] == FOUND else None) for a in want]
    assert res.src.cpu().numpy().view(np.uint64).tolist() == [NONE if a[1] is None else a[1] << 32 | a[2] for a in want]
    assert res.seq.cpu().numpy().view(np.uint64).tolist() == [a[3] for a in want]


def test_queries_as_views_into_a_wal_image(gpu, lib):
    """The query arena is a WAL image recovered with key views: offsets into the image, no key copied."""
    rng = np.random.default_rng(66)
    runs = gu.overlapping(rng, [300, 200], lo=1, hi=24)
    users = tu.users_of(runs)
    asked = [users[j] for j in rng.permutation(len(users))[:150]] + [b"not-there-%d" % j for j in range(20)]
    img, _ = wal.encode_batch(asked, [b"v"] * len(asked), first_seq=1)
    image = torch.zeros(len(img) + 7, dtype=torch.uint8, device=gpu)[7:]
    image.copy_(torch.from_numpy(np.frombuffer(img, np.uint8).copy()))
    status, batch, _, _ = wal.recover_device(image, key_views=True)
    assert status == "ok" and batch.keys is image
    cols = gu.columns(runs)
    tuples = [tuple(None if a is None else torch.from_numpy(a.view(a.dtype.str.replace("u", "i")) if a.itemsize > 1 else a).to(gpu)
                    for a in (c.keys, c.key_off, c.key_len, c.vals, c.val_off, c.val_len)) for c in cols]
    res = sst.get_device(tuples, (batch.keys, batch.key_off, batch.key_len))
    want = tu.oracle(cols, asked)
    assert list(res.items()) == [(a[0], a[4] if a[0] == FOUND else None) for a in want]


# ---- gather -----------------------------------------------------------------------------------------------

VALUE_SIZES = (0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 9000)


def test_value_sizes_and_every_destination_phase(gpu, lib):
    ks = [b"v%02d" % i for i in range(len(VALUE_SIZES))]
    runs = [tu.valued_run(ks, 0, sizes=VALUE_SIZES)]
    cols = gu.columns(runs)
    placed = gu.Placed(cols, gpu, 9)
    rng = np.random.default_rng(67)
    for phase in range(16):
        qs = [ks[j] for j in rng.permutation(len(ks))] + [b"none"]
        tu.check_get(lib.tkv_sst_get_device, cols, qs, device=gpu, phase=phase, tail=stream_of(gpu), placed=placed)


@pytest.mark.parametrize("total", (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1))
def test_totals_around_the_emit_tiles(gpu, lib, total):
    sizes = [total // 3, 0, total // 3, total - 2 * (total // 3)]
    ks = [b"t%d" % i for i in range(4)]
    ans = check(gpu, lib, gu.columns([tu.valued_run(ks, 0, sizes=sizes)]), ks + [b"none"], phase=total % 16)
    assert sum(len(a[4]) for a in ans) == total


def test_the_same_key_130_times(gpu, lib):
    runs = [tu.valued_run([b"a", b"hot", b"z"], 0, sizes=(70, 33, 5)), tu.valued_run([b"big"], 1, sizes=(5000,))]
    ans = check(gpu, lib, gu.columns(runs), [b"hot"] * 130 + [b"a", b"nope", b"hot"] + [b"big"] * 3, phase=11)
    assert sum(len(a[4]) for a in ans) == 131 * 33 + 70 + 3 * 5000


def test_all_absent_all_deleted_and_no_gather(gpu, lib):
    ks = [b"k%03d" % i for i in range(300)]
    runs = [tu.valued_run(ks, 0, sizes=(9,)), gu.make_run(ks, 1, tomb=1)]
    assert all(a[0] == DELETED for a in check(gpu, lib, gu.columns(runs), ks))
    assert last(lib)[3:] == [0, 300]
    assert all(a[0] == ABSENT for a in check(gpu, lib, gu.columns(runs), [k + b"x" for k in ks]))
    assert last(lib)[3:] == [0, 0]
    # vals_bytes without the gather: d_vals NULL, the lengths and the total still reported
    ans = check(gpu, lib, gu.columns(runs[:1]), ks + [b"none"], gather=False)
    assert sum(len(a[4]) for a in ans) == 300 * 9


@pytest.mark.parametrize("null", tu.COLS + ("vals",))
def test_single_null_output(gpu, lib, null):
    rng = np.random.default_rng(68)
    runs, pool = k_case(rng, [100, 120], tombs=(1,))
    check(gpu, lib, gu.columns(runs), pool[:150], nulls=(null,))


# ---- errors -----------------------------------------------------------------------------------------------

def base_case():
    rng = np.random.default_rng(6)
    runs = gu.overlapping(rng, [40, 0, 50, 30], lo=2)
    return gu.columns(runs), tu.users_of(runs)


def test_overflow_and_exact(gpu, lib):
    rng = np.random.default_rng(69)
    runs = [tu.valued_run(gu.distinct_keys(rng, 80), 0, sizes=(3, 0, 17, 100))]
    cols = gu.columns(runs)
    qs = tu.users_of(runs) + [b"nope"]
    _, vals, found = tu.expected(gu.Placed(cols), tu.oracle(cols, qs))
    for cap in (0, len(vals) - 1):
        got, outs = run_call(gpu, lib, cols, qs, outs=tu.Outputs(len(qs), cap, device=gpu))
        assert got == (OVERFLOW, found, len(vals), NONE)
        tu.assert_untouched(outs)
    outs = tu.Outputs(len(qs), len(vals), device=gpu, phase=5)
    got, _ = run_call(gpu, lib, cols, qs, outs=outs)
    assert got == (OK, found, len(vals), NONE) and outs.get("vals", len(vals)) == vals and outs.untouched("vals", len(vals))


@pytest.mark.parametrize("kind", [k for k in gu.CORRUPT_KINDS if k != "order"])
def test_corrupted(gpu, lib, kind):
    """A bad span on a probed entry: TKV_CORRUPTED with the model's (and the host call's) first_bad and no
    output touched; the same span where no search goes: TKV_OK."""
    base, qs = base_case()
    for r, i in ((3, 15), (2, 31), (0, 31), (3, 0)):
        cols, size = gu.corrupt(base, r, i, kind)
        want = tu.search_model(cols, qs, size)[0]
        assert want != NONE
        got, outs = run_call(gpu, lib, cols, qs, size)
        assert got == (CORRUPTED, 0, 0, want), (r, i)
        tu.assert_untouched(outs)
    cols, size = gu.corrupt(base, 3, 3, kind)
    above = [b"\xff" * 13]
    assert tu.search_model(cols, above, size)[0] == NONE
    got, outs = run_call(gpu, lib, cols, above, size)
    assert got == (OK, 0, 0, NONE) and outs.get("state", 1)[0] == ABSENT


def test_two_bad_entries_report_the_smallest_read(gpu, lib):
    base, qs = base_case()
    cols, size = gu.corrupt(base, 3, 7, "short")
    cols, _ = gu.corrupt(cols, 2, 31, "huge")
    assert tu.search_model(cols, qs, size)[0] == (2 << 32 | 31)
    got, outs = run_call(gpu, lib, cols, qs, size)
    assert got == (CORRUPTED, 0, 0, 2 << 32 | 31)
    tu.assert_untouched(outs)


def test_value_span_of_a_hit(gpu, lib):
    base, qs = base_case()
    ans = tu.oracle(base, qs)
    j = next(j for j, a in enumerate(ans) if a[0] == FOUND and a[1] == 2)
    r, i = ans[j][1], ans[j][2]
    cols = [c._replace(val_off=c.val_off.copy(), val_len=c.val_len.copy()) for c in base]
    cols[r].val_len[i] = cols[r].vals.size + 1 - int(cols[r].val_off[i])
    got, outs = run_call(gpu, lib, cols, qs)
    assert got == (CORRUPTED, 0, 0, r << 32 | i)
    tu.assert_untouched(outs)
    got, _ = run_call(gpu, lib, cols, qs, gather=False, outs=tu.Outputs(len(qs), 0, nulls=("vals", "val_pos"), device=gpu))
    assert got[0] == OK and got[3] == NONE
    assert run_call(gpu, lib, cols, [q for k, q in enumerate(qs) if k != j])[0][0] == OK


def test_bad_queries_go_before_corrupted(gpu, lib):
    base, qs = base_case()
    cols, size = gu.corrupt(base, 3, 15, "short")
    placed = gu.Placed(cols, gpu)
    outs = tu.Outputs(len(qs), 1 << 16, device=gpu)
    q = tu.Queries(qs, gpu)
    a = q.args()
    a[1] = q.size - 1  # the last query reaches past qkeys_size
    got = tu.call(lib.tkv_sst_get_device, placed, q, outs, tables=placed.tables(keys_size=size), qargs=a, tail=stream_of(gpu))
    assert got == (INVALID, 0xDEADBEEF, 0xDEADBEEF, 0xDEADBEEF)
    tu.assert_untouched(outs)
    for off, ln, bound in ((2**64 - 2, 4, None), (0, 2**28 - 17, 2**30)):
        q = tu.Queries(qs, gpu)
        q.keep[1][5], q.keep[2][5] = off - 2**64 if off >= 2**63 else off, ln
        a = q.args()
        a[1] = q.size if bound is None else bound
        got = tu.call(lib.tkv_sst_get_device, placed, q, outs, tables=placed.tables(keys_size=size), qargs=a, tail=stream_of(gpu))
        assert got == (INVALID, 0xDEADBEEF, 0xDEADBEEF, 0xDEADBEEF), (off, ln)
        tu.assert_untouched(outs)
    assert run_call(gpu, lib, cols, qs, size)[0] == (CORRUPTED, 0, 0, 3 << 32 | 15)


# ---- equivalence, pipeline, threads -----------------------------------------------------------------------

def to_device(gpu, cols):
    def dev(a):
        if a is None:
            return None
        return torch.from_numpy(a.view(a.dtype.str.replace("u", "i")) if a.itemsize > 1 else a).to(gpu)
    return [tuple(dev(a) for a in (c.keys, c.key_off, c.key_len, c.vals, c.val_off, c.val_len)) for c in cols]


@pytest.mark.parametrize("seed", range(16))
def test_get_equals_the_lookup_in_the_merge(gpu, lib, seed):
    """Every user key of the union and as many absent keys: src, value span and tombstone are those of the
    key's entry in merge_device's output (no drop flag), and a key the merge does not hold is absent."""
    runs, qs = tu.fuzz_case(seed)
    dev = to_device(gpu, gu.columns(runs))
    merged = sst.merge_device(dev)
    res = sst.get_device(dev, qs)
    by_user = {}
    src = merged.src.cpu().numpy().view(np.uint64)
    vo, vl = merged.val_off.cpu().numpy().view(np.uint64), merged.val_len.cpu().numpy().view(np.uint32)
    for j, (k, _) in enumerate(merged.entries()):
        by_user[k[:-17]] = (int(src[j]), int(vo[j]), int(vl[j]), k[-1] != 0)
    state = res.state.cpu().numpy()
    got_src, got_vo, got_vl = (t.cpu().numpy().view(dt) for t, dt in ((res.src, np.uint64), (res.val_off, np.uint64), (res.val_len, np.uint32)))
    assert len(by_user) == merged.n_entries
    for j, q in enumerate(qs):
        if q not in by_user:
            assert (state[j], got_src[j], got_vo[j], got_vl[j]) == (ABSENT, NONE, 0, 0), j
            continue
        s, o, ln, tomb = by_user[q]
        assert got_src[j] == s and state[j] == (DELETED if tomb else FOUND), j
        assert (got_vo[j], got_vl[j]) == ((0, 0) if tomb else (o, ln)), j
    assert sum(1 for q in qs if q in by_user) == len(by_user)


def test_get_device_over_a_merged_run(gpu, lib):
    """A MergedRun as a run of its own (offsets from its two bases, bounded by the key arenas and by the
    value arenas), alone and under a newer run, with and without value arenas in the merge."""
    rng = np.random.default_rng(72)
    runs = gu.overlapping(rng, [200, 150, 90])
    runs[1] = gu.make_run([k[:-17] for k, _ in runs[1]], 1, tomb=[i % 4 == 0 for i in range(150)])
    qs = tu.users_of(runs) + [b"", b"absent-key"]
    cols = gu.columns(runs)
    dev = to_device(gpu, cols)
    want = [(a[0], a[4] if a[0] == FOUND else None) for a in tu.oracle(cols, qs)]
    merged = sst.merge_device(dev[:2])
    assert list(sst.get_device([merged], qs).items()) == [(a[0], a[4] if a[0] == FOUND else None) for a in tu.oracle(cols[:2], qs)]
    assert list(sst.get_device([merged, dev[2]], qs).items()) == want
    seq = sst.get_device([merged, dev[2]], qs).seq.cpu().numpy().view(np.uint64).tolist()
    assert seq == [a[3] for a in tu.oracle(cols, qs)]
    bare = [t[:3] + (None, None, None) for t in dev]
    no_vals = sst.get_device([sst.merge_device(bare[:2]), bare[2]], qs)
    assert no_vals.vals_bytes == 0 and [s for s, _ in no_vals.items()] == [s for s, _ in want]
    assert list(sst.get_device([sst.merge_device(bare[:2]), bare[2]], qs, values=False).items()) == [(s, None) for s, _ in want]


def upload(gpu, c):
    def dev(a):
        if a.dtype != np.uint8:
            a = a.view(a.dtype.str.replace("u", "i"))
        return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return {k: dev(v) for k, v in c._asdict().items()}


def test_pipeline(gpu, lib):
    """WAL -> recover -> replay -> flush -> scan_device(views) as run 0, a second replayed batch as run 1:
    the get of every key ever written is a dict replay of the records; the same queries against the
    compaction of both give the same states and values."""
    rng = np.random.default_rng(70)
    pool = gu.distinct_keys(rng, 500, lo=0, hi=20, alpha=5)
    batches, seq = [], 1
    for b in range(2):
        recs = []
        for j in rng.choice(len(pool), 600).tolist():
            op = int(rng.random() < 0.25)
            recs.append((op, seq, pool[j], b"" if op else b"b%d-%d" % (b, seq) * int(rng.integers(1, 9)), op))
            seq += 1
        batches.append(recs)
    model = {}
    for recs in batches:
        for op, s, k, v, _ in recs:
            model[k] = (DELETED, None) if op else (FOUND, v)
    ts = 1_700_000_000_000
    r0 = batches[0]
    img, _ = wal.encode_batch([r[2] for r in r0], [r[3] for r in r0], seqs=[r[1] for r in r0], ops=[r[0] for r in r0],
                              tombstones=[r[4] for r in r0])
    image = torch.from_numpy(np.frombuffer(img, np.uint8).copy()).to(gpu)
    status, batch, _, _ = wal.recover_device(image, key_views=True, val_views=True)
    assert status == "ok"
    table = memtable.build_device(batch, timestamp_ms=ts).flush(1024)
    run0 = sst.scan_device(table.file, key_views=True, val_views=True)
    r1 = batches[1]
    run1 = memtable.build_device(timestamp_ms=ts + 1, vals=torch.from_numpy(mu.values_arena(r1)).to(gpu), **upload(gpu, mu.columns(r1)))
    qs = pool + [b"never-written"]
    want = [model.get(q, (ABSENT, None)) for q in qs]
    assert {s for s, _ in want} == {ABSENT, FOUND, DELETED}
    res = sst.get_device([run0, run1], qs)
    assert list(res.items()) == want
    compacted = sst.compact_device([table.file, run1.flush(512).file])
    again = sst.get_device([sst.scan_device(compacted.file, key_views=True, val_views=True)], qs)
    assert list(again.items()) == want


def test_four_threads_get_at_once(gpu, lib):
    cases = [tu.fuzz_case(100 + t) for t in range(4)]
    failures = []

    def run(t):
        try:
            torch.cuda.set_device(gpu)
            runs, qs = cases[t]
            for _ in range(3):
                tu.check_get(lib.tkv_sst_get_device, gu.columns(runs), qs, device=gpu, tail=stream_of(gpu), phase=t)
        except BaseException as e:  # noqa: BLE001
            failures.append((t, repr(e)))
    threads = [threading.Thread(target=run, args=(t,), daemon=True) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(120)
    assert not any(th.is_alive() for th in threads), "a caller is still running after 120 s"
    assert not failures, failures


def test_phase_times_zero_unless_enabled(gpu, lib):
    rng = np.random.default_rng(71)
    runs, pool = k_case(rng, [2000, 1000], ())
    ms = (ctypes.c_double * 4)()
    prev = lib.tkv_debug_sst_get_phases(0, None)
    try:
        check(gpu, lib, gu.columns(runs), pool)
        lib.tkv_debug_sst_get_phases(1, ms)
        assert list(ms) == [0.0] * 4
        check(gpu, lib, gu.columns(runs), pool)
        lib.tkv_debug_sst_get_phases(0, ms)
        assert all(v >= 0.0 for v in ms) and sum(ms) > 0.0
    finally:
        lib.tkv_debug_sst_get_phases(prev, None)
