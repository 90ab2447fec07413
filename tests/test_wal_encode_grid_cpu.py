"""The batches of tests/test_gpu_wal_encode_grid.py without a GPU: each grid builder holds every case it
promises (counted from the built batch, so a builder that loses coverage fails here), and the host
layout (tkv_debug_wal_encode_layout, CRC fields zero) of each equals the numpy restatement of
wal.cpp:19-61 with intact sentinels."""
import numpy as np
import pytest

from wal_encode_util import (FUSED_LENS, KEY_LONG, SPAN_SHORT, VAL_LONG, arena_at, expected, fused_grid_batch,
                             fused_pairs, geometry, layout_host, loop_pattern, make_batch, span_cases, span_coverage,
                             span_grid_batch, tiled, tiled_expected)


def layout_equals(lib, b, want):
    got, size, img, guard = layout_host(lib, b)
    assert (got, size) == (b["n"], want.size)
    assert guard, "bytes outside the destination were written"
    bad = np.flatnonzero(img != want)
    assert bad.size == 0, f"layout differs at {bad[:8]}"


def test_arena_at():
    rng = np.random.default_rng(940)
    lens = rng.integers(0, 300, 500)
    res = rng.integers(0, 16, 500)
    res[0] = 0
    data, off = arena_at(rng, lens, res)
    o = off.astype(np.int64)
    assert np.array_equal(o % 16, res) and o[0] == 16
    gap = o[1:] - (o[:-1] + lens[:-1])
    assert gap.min() >= 0 and gap.max() <= 15 and int(o[-1] + lens[-1]) <= data.size
    assert arena_at(rng, lens, res, first_at_zero=True)[1][0] == 0
    # through make_batch, and the callers without residues keep the arena of odd offsets
    b = make_batch(rng, lens, lens[::-1], key_res=res, val_res=res[::-1])
    assert np.array_equal(b["key_off"] % 16, res) and np.array_equal(b["val_off"] % 16, res[::-1])
    assert make_batch(rng, [3, 4], [5, 6])["key_off"][0] == 1


def test_fused_length_grid_is_complete(lib):
    b = fused_grid_batch(np.random.default_rng(941))
    want, offs, _ = expected(b)
    assert want.size < 1 << 20
    for img_res in (0, 5):  # wherever the image lies
        assert fused_pairs(b, offs, img_res).size == len(FUSED_LENS) * 16 == 225 * 16
    rl = 18 + b["key_len"].astype(np.int64) + b["val_len"].astype(np.int64)
    t = b["target"]
    assert np.count_nonzero(t) == 225 * 16 and (rl[~t] <= 33).all() and (b["val_len"][~t] == 0).all()
    for kind in (0, 1, 2):  # every length all key, all value and split
        assert np.array_equal(np.unique(rl[b["kind"] == kind]), np.arange(18, 243))
    assert (b["val_len"][b["kind"] == 0] == 0).all() and (b["key_len"][b["kind"] == 1] == 0).all()
    # bodies on both sides of the border between the lane copy and the wave copy, keys and values
    for ln in (b["key_len"][t], b["val_len"][t]):
        assert {63, 64, 65, 66} <= set(ln.tolist()) and ln.max() == 224
    layout_equals(lib, b, want)


@pytest.mark.parametrize("which,longer", [("val", VAL_LONG), ("key", KEY_LONG)])
def test_span_alignment_grid_is_complete(lib, which, longer):
    b = span_grid_batch(np.random.default_rng(942), SPAN_SHORT + longer, which)
    want, offs, _ = expected(b)
    assert want.size < (12 << 20 if which == "val" else 3 << 20)
    for src_res, img_res in ((0, 0), (7, 12)):
        cases = span_cases(b, offs, which, src_res, img_res)
        assert cases.shape[0] == 256 * len(SPAN_SHORT + longer)
        pairs, triples = span_coverage(cases)
        assert sorted(pairs) == sorted(SPAN_SHORT + longer)
        assert all(v == 256 for v in pairs.values()), pairs
        assert triples == 4096
    t = b["target"]
    short = b["key_len"] if which == "val" else b["val_len"]
    assert short[t].max() <= 15 and (b["key_len"][~t] <= 15).all() and (b["val_len"][~t] == 0).all()
    layout_equals(lib, b, want)


def test_loop_pattern_and_tiling(lib):
    tile = geometry(lib)[0]
    for seed, size, mids in ((943, 1 << 20, (1, 4)), (944, 1 << 20, (80, 121))):
        b = loop_pattern(np.random.default_rng(seed), size, tile, mids=mids)
        want, offs, _ = expected(b)
        assert want.size % 2 == 1 and size <= want.size < size + (1 << 18)
        sz = 26 + b["key_len"].astype(np.int64) + b["val_len"].astype(np.int64)
        o = offs.astype(np.int64)
        assert np.count_nonzero(sz == 248) >= 1 and np.count_nonzero(sz == 249) >= 1  # record_len 240 and 241
        assert np.count_nonzero(sz > 2 * tile) >= 3
        assert (b["key_len"] > 2 * tile).any() and (b["val_len"] > 2 * tile).any()
        assert np.count_nonzero((b["val_len"] >= 100) & (b["val_len"] <= 3000)) >= 100
        starts = np.bincount(o // tile, minlength=want.size // tile + 1)  # records that start in each tile
        assert starts.max() > 64 and starts.min() == 0
        if mids == (1, 4):  # all of it within any few tiles: runs past the lanes, mid-size values between them
            run = (sz <= 40).astype(np.int64)
            edges = np.flatnonzero(np.diff(np.concatenate([[0], run, [0]])))
            runs = edges[1::2] - edges[0::2]
            assert runs.size >= 100 and np.median(runs) > 64
            assert np.diff(o[edges[0::2]]).max() < 6 * tile
        layout_equals(lib, b, want)
        if mids == (1, 4):
            reps = 3
            tb = tiled(b, reps)
            timg, toffs, _ = tiled_expected((want, offs, np.zeros(b["n"], np.uint32)), reps)
            assert tb["n"] == reps * b["n"] and np.array_equal(expected(tb)[1], toffs)
            assert len({(k * want.size) % 16 for k in range(16)}) == 16  # an odd size: every residue
            layout_equals(lib, tb, timg)
