"""tkv_wal_decode_device on the GPU over whole grids of cases: every (source, destination) alignment of
a wave-copied span as key and as value, tile edges and runs of empty spans, the emit wave's tile loop run
several times, the second scan level, offsets past 4 GiB on both sides, and a small decode behind a large
one. Expected values are wal_decode_util.expected on images from wal_encode_util.expected; every byte and
record is compared and every arena lies between 0xA5 sentinels."""
import numpy as np
import pytest

from wal_decode_util import (GRID_LONG, GRID_SHORT, KEY_VIEWS, VAL_VIEWS, DevOut, check_device, decode_device, dev_offsets,
                             expected, geometry, grid_coverage, grid_lens, last, tiled_want)
from wal_encode_util import geometry as enc_geometry
from wal_encode_util import loop_pattern, make_batch, tiled_expected
from wal_encode_util import expected as encoded

pytestmark = pytest.mark.gpu


def upload(gpu, img):
    import torch
    return torch.from_numpy(img).to(gpu)


@pytest.mark.parametrize("which", ("key", "val"))
def test_span_alignment_grid(gpu, lib, oracle, which):
    """Spans of 65..80 bytes and a few long ones at every (source residue, destination residue) mod 16,
    as key and as value: wave_copy's switch and shift, its head and tail granules, one to five steps, a
    span cut by one or two tile edges. The residues are those of the real pointers."""
    rng = np.random.default_rng(1401 if which == "key" else 1402)
    lengths = GRID_SHORT + GRID_LONG
    klen, vlen, target = grid_lens(rng, lengths, which)
    b = make_batch(rng, klen, vlen)
    img, offs, _ = encoded(b, oracle)
    image = upload(gpu, img)
    for align in (0, 9):
        out, want = check_device(lib, gpu, image, img, offs, 0, kalign=align, valign=align)
        ares = (out.kbuf.data_ptr() + out.kstart if which == "key" else out.vbuf.data_ptr() + out.vstart) % 16
        cover = grid_coverage(want, offs, target, which, image.data_ptr() % 16, ares)
        assert sorted(cover) == sorted(lengths) and all(v == 256 for v in cover.values()), cover
    check_device(lib, gpu, image, img, offs, VAL_VIEWS if which == "key" else KEY_VIEWS, kalign=3, valign=3)


def edge_lens(tile):
    """Span lengths of one arena: a span that ends exactly at a tile end, one that starts there, one longer
    than two tiles, 300 one-byte spans in one tile, a run of 5000 empty spans at a tile edge (the span in
    front ends at the tile's last byte) and one in the middle of a tile."""
    lens = [tile - 10, 10, 5, 2 * tile + 100]         # ends at tile 1's end; starts at tile 1; crosses tiles 1..3
    lens += [1] * 300 + [70]
    pos = sum(lens)
    lens += [(-pos) % tile or tile]                    # ends exactly at a tile end
    lens += [0] * 5000 + [33]                          # the run lies on the tile edge
    lens += [0] * 5000 + [9, 0, 0, 200, 0]             # a run inside a tile, and empty spans at the very end
    return np.array(lens, np.int64)


@pytest.mark.parametrize("which", ("key", "val"))
def test_tile_edges_and_empty_runs(gpu, lib, oracle, which):
    tile = geometry(lib)[0]
    rng = np.random.default_rng(1403)
    a = edge_lens(tile)
    other = rng.integers(0, 20, a.size)
    b = make_batch(rng, *((a, other) if which == "key" else (other, a)))
    img, offs, _ = encoded(b, oracle)
    image = upload(gpu, img)
    for align in (0, 13):
        check_device(lib, gpu, image, img, offs, 0, kalign=align, valign=16 - align)
    # empty spans in front of everything
    p = np.r_[np.flatnonzero(a == 0)[:200], np.arange(a.size)]
    check_device(lib, gpu, image, img, offs[p], 0, kalign=5, valign=5)


def test_one_byte_arena(gpu, lib, oracle):
    rng = np.random.default_rng(1404)
    klen = np.zeros(200, np.int64)
    klen[137] = 1
    b = make_batch(rng, klen, rng.integers(0, 90, 200))
    img, offs, _ = encoded(b, oracle)
    for align in (0, 15):
        out, want = check_device(lib, gpu, upload(gpu, img), img, offs, 0, kalign=align, valign=1)
        assert want["keys_size"] == 1 and last(lib)[0] > 0


@pytest.fixture(scope="module")
def loop_case(gpu, oracle, lib):
    b = loop_pattern(np.random.default_rng(1405), 1 << 20, enc_geometry(lib)[0], mids=(40, 60))
    exp = encoded(b, oracle)
    return b, exp, expected(exp[0], exp[1])


def sweeps(lib, want, factor):
    """Repetitions of the loop pattern for its value arena to be `factor` sweeps of the largest launch
    (at most 32 waves per CU), and that many arena bytes."""
    import torch
    need = factor * torch.cuda.get_device_properties(0).multi_processor_count * 32 * geometry(lib)[0]
    return need // want["vals_size"] + 2, need


def test_wave_tile_loop(gpu, lib, loop_case):
    """A value arena of more than three sweeps of the launch, so every emit wave goes round its tile loop
    at least three times, over tiles with more than 128 span starts, mid-size spans, no span start at all
    and one span."""
    b, exp, want = loop_case
    reps, need = sweeps(lib, want, 3)
    img, offs, _ = tiled_expected(exp, reps)
    tw = tiled_want(want, exp[0].size, reps)
    assert tw["vals_size"] > need
    check_device(lib, gpu, upload(gpu, img), img, offs, 0, kalign=7, valign=7, want=tw)
    st = last(lib)
    assert st[0] > 0 and 3 * st[1] * geometry(lib)[0] < tw["vals_size"], st


def test_small_after_large(gpu, lib, oracle, loop_case):
    """The kept scratch (offsets, tile tables, first-bad word) after a large decode: a small batch and a
    single record decode as on a fresh device."""
    b, exp, want = loop_case
    reps = sweeps(lib, want, 1)[0]
    img, offs, _ = tiled_expected(exp, reps)
    check_device(lib, gpu, upload(gpu, img), img, offs, 0, kalign=3, valign=3, want=tiled_want(want, exp[0].size, reps))
    rng = np.random.default_rng(1406)
    for klen, vlen in ((rng.integers(0, 24, 1000), rng.integers(0, 65, 1000)), ([9], [30]), ([7], [300]), ([0], [0])):
        s = make_batch(rng, klen, vlen)
        simg, soffs, _ = encoded(s, oracle)
        check_device(lib, gpu, upload(gpu, simg), simg, soffs, 0, kalign=3, valign=3)


def test_second_scan_level(gpu, lib, oracle):
    """n = (records per scan workgroup)^2 + 5 one-byte keys with empty values: the second scan level
    carries into a third."""
    per = geometry(lib)[1]
    n = per * per + 5
    rng = np.random.default_rng(1407)
    b = make_batch(rng, np.ones(n, np.int64), np.zeros(n, np.int64))
    img, offs, _ = encoded(b, oracle)
    out, want = check_device(lib, gpu, upload(gpu, img), img, offs, 0, kalign=1, valign=0)
    assert want["keys_size"] == n and want["vals_size"] == 0
    assert int(out.cols()["key_off"][-1]) == n - 1


def test_offsets_past_4_gib(gpu, lib, oracle):
    """Source positions and arena offsets past 2^32, built and checked on the device: two records with
    values of 2^31 + 7 and 2^31 + 1000 bytes (a value_len is a u32 and record_len = 18 + key_len + value_len
    another, so no single value reaches 2^32: the first value offset behind the two is the one past 2^32),
    and 300 small records behind them, past the image's 4 GiB mark, with u64 offsets."""
    import torch
    free = torch.cuda.mem_get_info()[0]
    if free < 16 << 30:
        pytest.skip(f"{free >> 30} GiB of device memory free, the test needs 16 GiB")
    rng = np.random.default_rng(1408)
    V = ((1 << 31) + 7, (1 << 31) + 1000)
    K = (5, 3)
    sb = make_batch(rng, rng.integers(0, 24, 300), rng.integers(0, 200, 300))
    simg, soffs, _ = encoded(sb, oracle)
    starts = [0, 26 + K[0] + V[0]]
    base = starts[1] + 26 + K[1] + V[1]
    total = base + simg.size
    image = torch.empty(total, dtype=torch.uint8, device=gpu)
    for lo in range(0, base, 1 << 30):  # the giant values: random bytes, a slab at a time
        hi = min(base, lo + (1 << 30))
        image[lo:hi] = torch.randint(0, 256, (hi - lo,), dtype=torch.uint8, device=gpu)
    for s, k, v in zip(starts, K, V):
        hdr = np.zeros(26, np.uint8)
        hdr[0:4] = np.frombuffer((18 + k + v).to_bytes(4, "little"), np.uint8)
        hdr[8], hdr[17] = 1, 1
        hdr[9:17] = np.frombuffer((0x1122334455667788 + s).to_bytes(8, "little"), np.uint8)
        hdr[18:22] = np.frombuffer(k.to_bytes(4, "little"), np.uint8)
        hdr[22:26] = np.frombuffer(v.to_bytes(4, "little"), np.uint8)
        image[s:s + 26] = torch.from_numpy(hdr).to(gpu)
    image[base:] = torch.from_numpy(simg).to(gpu)
    offs = np.r_[np.array(starts, np.uint64), soffs + np.uint64(base)]
    assert int(offs[2]) > 1 << 32
    small = expected(simg, soffs)
    ks, vs = sum(K) + small["keys_size"], sum(V) + small["vals_size"]
    out = DevOut(gpu, offs.size, ks, vs, 5, 11)
    assert decode_device(lib, image, dev_offsets(gpu, offs), 0, out) == (0, ks, vs, offs.size)
    assert out.guards_ok(ks, vs), "bytes outside a destination were written"
    c = out.cols()
    assert c["val_off"].tolist()[:3] == [0, V[0], V[0] + V[1]] and int(c["val_off"][2]) > 1 << 32
    assert c["key_off"].tolist()[:3] == [0, K[0], K[0] + K[1]]
    assert c["key_len"].tolist()[:2] == list(K) and c["val_len"].tolist()[:2] == list(V)
    assert c["seq"].tolist()[:2] == [0x1122334455667788 + s for s in starts] and c["op"].tolist()[:2] == [1, 1]
    for k in ("op", "tomb", "seq", "key_len", "val_len"):
        assert np.array_equal(c[k][2:], small[k]), k
    assert np.array_equal(c["val_off"][2:], small["val_off"] + np.uint64(sum(V)))
    keys, vals = out.arena("keys", ks), out.arena("vals", vs)
    assert torch.equal(keys[:K[0]], image[26:26 + K[0]]) and torch.equal(keys[K[0]:sum(K)], image[starts[1] + 26:starts[1] + 26 + K[1]])
    assert np.array_equal(keys[sum(K):].cpu().numpy(), small["keys"])
    assert np.array_equal(vals[sum(V):].cpu().numpy(), small["vals"])
    at = 0
    for s, k, v in zip(starts, K, V):  # the giant values, a slab at a time
        for lo in range(0, v, 1 << 30):
            hi = min(v, lo + (1 << 30))
            assert torch.equal(vals[at + lo:at + hi], image[s + 26 + k + lo:s + 26 + k + hi]), (s, lo)
        at += v
    # the same records as views: offsets into the image past 2^32
    vout = DevOut(gpu, offs.size, None, None)
    assert decode_device(lib, image, dev_offsets(gpu, offs), KEY_VIEWS | VAL_VIEWS, vout) == (0, ks, vs, offs.size)
    vc = vout.cols()
    assert np.array_equal(vc["key_off"], offs + np.uint64(26))
    assert np.array_equal(vc["val_off"], offs + np.uint64(26) + c["key_len"].astype(np.uint64))
    del image, out, vout, keys, vals
    torch.cuda.empty_cache()
