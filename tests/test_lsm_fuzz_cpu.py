"""The LSM fuzz cases (lsm_fuzz_util.case) without a GPU: the host replay (tkv_memtable_build) of every batch
and the host merge (tkv_sst_merge) of the batches' file images, flat, with the drop flag and nested, against
the helper's dict model for every seed the GPU test runs, and the counts that prove the seed range holds
every situation the fuzz exists for. tkv_sst_build and tkv_sst_scan stamp and verify on the GPU and stay out
of this file: the files are the writer oracle's, taken apart by the host parse."""
import numpy as np
import pytest

import lsm_fuzz_util as fz
import sst_merge_util as gu
from tinykvpp_amd import load_library, memtable, sst

T = int(load_library().tkv_debug_sst_merge_tile())


@pytest.fixture(scope="module")
def cases():
    """case(seed) for every seed, made once for this module."""
    made = {}

    def get(seed):
        if seed not in made:
            made[seed] = fz.case(seed)
        return made[seed]
    return get


def test_coverage(cases):
    """The seed range holds every situation often enough, no seed is degenerate, and the seeds the GPU tests
    name are what they are named for."""
    cs = [cases(s) for s in fz.SEEDS]
    cov = fz.coverage(cs, T)
    print("coverage over", len(cs), "seeds:", cov)
    assert len(cs) == 32
    assert fz.SCAN_BLOCK < T and min(fz.COUNTS) < fz.SCAN_BLOCK < 1100 < T < 2100
    for name, floor in (("five_runs", 8), ("entries_over_tile", 8), ("batch_over_tile", 8), ("pool_40_batch_1000", 4),
                        ("nested", 8), ("big_value_survives", 4), ("seq_descends", 6), ("other_stream", 8),
                        ("ts_descends", 4), ("cross_batch_duplicates", 8), ("tombstone_survives", 8)):
        assert cov[name] >= floor, (name, cov)
    assert cov["seq_descends"] < 32 and cov["ts_descends"] < 32 and cov["other_stream"] < 32
    assert {c.target for c in cs} == set(fz.TARGETS)
    assert {c.flags for c in cs} == {0, 1, 2, 3}
    assert {c.misalign for c in cs} >= {0, 15}
    for c in cs:  # no degenerate seed: two or more batches with a record, distinct timestamps, a put survives
        assert 2 <= c.k <= 8 and all(c.counts) and len(set(c.ts)) == c.k and sum(c.counts) <= 8 * 3000
        seqs = [r[1] for recs in c.batches for r in recs]
        assert len(set(seqs)) == len(seqs)
        assert (c.batches[-1][0][1] < c.batches[0][0][1]) == c.seq_descends
        assert (c.ts[-1] < c.ts[0]) == c.ts_descends
    size = {c.seed: fz.work(c) for c in cs}
    assert size[fz.LARGEST] == max(size.values()) and size[fz.SMALLEST] == min(size.values()), size
    d = cases(fz.DAMAGED)
    assert d.k >= 3 and d.counts[d.k // 2] >= 1000 and d.target <= 512
    assert len(set(fz.THREAD_SEEDS)) == 4
    for s in fz.THREAD_SEEDS:
        assert cases(s).k >= 3 and sum(cases(s).counts) < 6000
    assert len({cases(s).target for s in fz.THREAD_SEEDS}) >= 3


def merged_entries(cols, drop=False):
    got = sst.merge(cols, drop_tombstones=drop)
    return got, got.entries()


@pytest.mark.parametrize("seed", fz.SEEDS)
def test_host_paths_of_every_case(lib, cases, seed):
    c = cases(seed)
    e = fz.expect(c)
    # the host replay of every batch
    for recs, ts, exp, ents in zip(c.batches, c.ts, e.mem, e.entries):
        run = memtable.build(recs, timestamp_ms=ts)
        assert run.ikeys.tobytes() == exp.ikeys and np.array_equal(run.src, exp.src)
        assert run.entries() == ents
    assert any(k[-1] == 0 for k, _ in e.model) and e.live
    # the host merge of the batches' files: flat, with drop
    cols = gu.file_columns(lib, e.entries, c.target)
    assert [gu.run_entries(col) for col in cols] == e.entries
    want_src = gu.oracle(cols)
    assert want_src == e.src
    got, ents = merged_entries(cols)
    assert got.src.tolist() == [r << 32 | i for r, i in want_src]
    assert ents == e.model
    assert [e.entries[r][i] for r, i in want_src] == e.model
    got, ents = merged_entries(cols, drop=True)
    assert got.src.tolist() == [r << 32 | i for r, i in gu.oracle(cols, drop=True)]
    assert ents == e.live == [x for x in e.model if x[0][-1] == 0]
    # nested: the first half compacted into a file of its own, which is then the oldest run
    half = c.k // 2
    if half >= 2:
        _, first = merged_entries(cols[:half])
        assert first == fz.model(e.entries[:half])
        mid = gu.file_columns(lib, [first], fz.NESTED_TARGET)
        assert mid[0].keys.tobytes() == e.half
        for drop, want in ((False, e.model), (True, e.live)):
            assert merged_entries(mid + cols[half:], drop)[1] == want
