"""tkv_wal_encode_device / tkv_wal_encode on the GPU over whole grids of cases: every fused record
length at every start residue, every (source, destination, end) alignment of a wave-copied span, the
emit wave's tile loop run several times over real spans, images and arena offsets past 4 GiB, the host
entry, and a small batch behind a large one. Every expected image is the numpy restatement of
wal.cpp:19-61 with CRCs from the test oracle (wal_encode_util.expected), every destination lies between
two 64-byte sentinels, and every residue is taken from the real pointers. The batches are those of
tests/test_wal_encode_grid_cpu.py, which proves their coverage without a GPU."""
import numpy as np
import pytest

import tinykvpp_amd as tk
from test_gpu_wal_encode import check, long_batch, small_batch
from tinykvpp_amd._lib import OK
from wal_encode_util import (FUSED_LENS, KEY_LONG, SENT, SPAN_SHORT, VAL_LONG, DeviceBatch, encode_host,
                             encode_on_device, expected, fused_grid_batch, fused_pairs, geometry, last, loop_pattern,
                             make_batch, span_cases, span_coverage, span_grid_batch, tiled, tiled_expected)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fused_case(gpu, oracle):
    b = fused_grid_batch(np.random.default_rng(921))
    return DeviceBatch(b, gpu), expected(b, oracle)


@pytest.fixture(scope="module")
def val_case(gpu, oracle):
    b = span_grid_batch(np.random.default_rng(922), SPAN_SHORT + VAL_LONG, "val")
    return DeviceBatch(b, gpu), expected(b, oracle)


@pytest.fixture(scope="module")
def key_case(gpu, oracle):
    b = span_grid_batch(np.random.default_rng(923), SPAN_SHORT + KEY_LONG, "key")
    return DeviceBatch(b, gpu), expected(b, oracle)


@pytest.fixture(scope="module")
def loop_case(gpu, oracle, lib):
    b = loop_pattern(np.random.default_rng(924), 1 << 20, geometry(lib)[0])
    return b, expected(b, oracle)


@pytest.fixture(scope="module")
def small_case(gpu, oracle):
    b = small_batch(np.random.default_rng(925), 1000)
    return DeviceBatch(b, gpu), expected(b, oracle)


def check_on(lib, db, exp, align):
    """The encode of db at image address = align (mod 16) against exp, sentinels, rec_off and crc in
    full: (image as numpy, the image's address)."""
    want, offs, crc = exp
    buf, start, goff, gcrc = encode_on_device(lib, db, want.size, align)
    addr = buf.data_ptr() + start
    h = buf.cpu().numpy()
    assert (h[start - SENT:start] == 0xA5).all() and (h[start + want.size:start + want.size + SENT] == 0xA5).all(), \
        "bytes outside the destination were written"
    img = h[start:start + want.size]
    bad = np.flatnonzero(img != want)
    if bad.size:
        r = int(np.searchsorted(offs, bad[0], "right")) - 1
        at = int(bad[0])
        raise AssertionError(f"image differs in {bad.size} bytes, first at {at}: record {r} (key_len "
                             f"{db.b['key_len'][r]}, val_len {db.b['val_len'][r]}) byte {at - int(offs[r])}, "
                             f"expected {want[at:at + 8].tobytes().hex()} got {img[at:at + 8].tobytes().hex()}")
    assert np.array_equal(goff.cpu().numpy().view(np.uint64), offs)
    got = gcrc.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, crc), f"crc differs for records {np.flatnonzero(got != crc)[:8]}"
    st = last(lib)
    assert st[0] + st[1] == db.b["n"] and st[3] == want.size
    return img, addr


def unfused(lib, db, exp, align, fused_img):
    prev = lib.tkv_debug_set_wal_encode_fused(0)
    try:
        img, _ = check_on(lib, db, exp, align)
        assert last(lib)[:2] == [0, db.b["n"]]
    finally:
        lib.tkv_debug_set_wal_encode_fused(prev)
    assert np.array_equal(img, fused_img)


def test_fused_length_grid(lib, fused_case):
    """Every record_len 18..242 at every address of its first byte mod 16 (fold_raw's b0 & 3, its masked
    first dword and the window dwords it reads; inj[L]), the body all key, all value and split."""
    db, exp = fused_case
    b = db.b
    rl = 18 + b["key_len"].astype(np.int64) + b["val_len"].astype(np.int64)
    nlong = int(np.count_nonzero(rl > 240))
    assert nlong == 32 and set(rl[rl > 240].tolist()) == {241, 242}
    for align in (0, 11):
        img, addr = check_on(lib, db, exp, align)
        assert addr % 16 == align
        assert fused_pairs(b, exp[1], addr % 16).size == len(FUSED_LENS) * 16
        assert last(lib)[:2] == [b["n"] - nlong, nlong]  # the emit pass stamped all up to 240, the rest read back
    unfused(lib, db, exp, 11, img)


def span_grid(lib, db, exp, which, lengths, align):
    img, addr = check_on(lib, db, exp, align)
    arena = db.t["vals" if which == "val" else "keys"]
    pairs, triples = span_coverage(span_cases(db.b, exp[1], which, arena.data_ptr() % 16, addr % 16))
    assert sorted(pairs) == sorted(lengths) and all(v == 256 for v in pairs.values()) and triples == 4096
    return img


def test_long_span_alignment_grid(lib, val_case):
    """Values of 65..80 bytes at every (source, destination) residue: every (relative, destination, end)
    triple of wave_copy (its switch, sh, and the head and tail granules through put4); the longer
    lengths at all 256 pairs: one to five steps of the unroll, the longest cut by one or two tile edges."""
    db, exp = val_case
    img = span_grid(lib, db, exp, "val", SPAN_SHORT + VAL_LONG, 9)
    unfused(lib, db, exp, 9, img)


def test_long_key_alignment_grid(lib, key_case):
    """The same with the long span as the key (ks of emit_tile) and a value of 0..15 bytes behind it."""
    db, exp = key_case
    img = span_grid(lib, db, exp, "key", SPAN_SHORT + KEY_LONG, 2)
    unfused(lib, db, exp, 2, img)


def sweeps(lib, factor):
    """Image bytes for every emit wave to run its tile loop `factor` times: (tile, bytes)."""
    import torch
    tile = geometry(lib)[0]
    return tile, factor * torch.cuda.get_device_properties(0).multi_processor_count * 16 * tile


def test_wave_tile_loop(gpu, lib, loop_case):
    """An image of more than three sweeps of the grid, so every wave goes round its loop (t += nwaves, the
    h / hn / hnn and r0 / rn prefetch rotation) at least three times, over tiles with more than 64
    records, mid-size values, no record start at all, and one record."""
    b, exp = loop_case
    tile, need = sweeps(lib, 3)
    reps = need // exp[0].size + 2
    tb = tiled(b, reps)
    want, offs, crc = tiled_expected(exp, reps)
    db = DeviceBatch(tb, gpu)
    check_on(lib, db, (want, offs, crc), 7)
    st = last(lib)
    assert 3 * st[2] * tile < want.size, (st, tile, want.size)
    assert st[1] == int(np.count_nonzero(18 + tb["key_len"].astype(np.int64) + tb["val_len"] > 240))


def test_image_past_4_gib(gpu, lib, oracle):
    """An image of more than 2^32 + 2^27 bytes: u64 offsets in the size scan, enc_finish, the tile heads,
    the read-back list and the emit pass. Compared on the device against the pattern's expected image."""
    import torch
    free = torch.cuda.mem_get_info()[0]
    if free < 16 << 30:
        pytest.skip(f"{free >> 30} GiB of device memory free, the test needs 16 GiB")
    tile = geometry(lib)[0]
    b = loop_pattern(np.random.default_rng(926), 1 << 20, tile, mids=(80, 121))
    pimg, poffs, pcrc = expected(b, oracle)
    P = pimg.size
    reps = ((1 << 32) + (1 << 27)) // P + 1
    total = reps * P
    assert total > (1 << 32) + (1 << 27) and P % 2 == 1
    tb = tiled(b, reps)
    n = tb["n"]
    assert n < 8_000_000
    db = DeviceBatch(tb, gpu)
    buf, start, goff, gcrc = encode_on_device(lib, db, total, 13)
    st = last(lib)
    assert st[0] + st[1] == n and st[3] == total
    assert bool((buf[start - SENT:start] == 0xA5).all()) and bool((buf[start + total:start + total + SENT] == 0xA5).all())
    image = buf[start:start + total]
    row = torch.from_numpy(pimg).to(gpu)
    slab = max(1, (256 << 20) // P)
    for k0 in range(0, reps, slab):
        k1 = min(reps, k0 + slab)
        diff = image[k0 * P:k1 * P].view(k1 - k0, P) != row
        if bool(diff.any()):
            at = int(diff.view(-1).nonzero()[0]) + k0 * P
            raise AssertionError(f"image differs at {at} (repetition {at // P}, pattern byte {at % P}): expected "
                                 f"{pimg[at % P:at % P + 8].tobytes().hex()} got {image[at:at + 8].cpu().numpy().tobytes().hex()}")
        del diff
    base = torch.arange(reps, dtype=torch.int64, device=gpu) * P
    woff = (base[:, None] + torch.from_numpy(poffs.view(np.int64)).to(gpu)[None, :]).reshape(-1)
    assert int(woff[-1]) > 1 << 32 and torch.equal(goff, woff)
    assert torch.equal(gcrc, torch.from_numpy(pcrc.view(np.int32)).to(gpu).repeat(reps))
    del woff, row
    assert tk.wal.verify_device(image) == ("ok", n, total)
    del image, buf, db
    torch.cuda.empty_cache()


def test_arena_offsets_past_4_gib(gpu, lib, oracle):
    """key_off / val_off of 2^32 and more: the arenas' bytes lie at the end of two device buffers of
    4 GiB + their size."""
    import torch
    rng = np.random.default_rng(927)
    n = 2000
    klen, vlen = rng.integers(0, 24, n), rng.integers(0, 65, n)
    lk, lv = rng.choice(n, 300, replace=False), rng.choice(n, 500, replace=False)
    klen[lk], vlen[lv] = rng.integers(65, 3001, 300), rng.integers(65, 3001, 500)
    b = make_batch(rng, klen, vlen)
    exp = expected(b, oracle)
    db = DeviceBatch(b, gpu)
    for name, off in (("keys", "key_off"), ("vals", "val_off")):
        size = b[name].size
        big = torch.empty((1 << 32) + size, dtype=torch.uint8, device=gpu)
        big[1 << 32:] = db.t[name]
        db.t[name] = big
        db.t[off] = db.t[off] + (1 << 32)
        assert int(db.t[off].min()) >= 1 << 32
    check_on(lib, db, exp, 4)
    del db
    torch.cuda.empty_cache()


def test_host_entry_against_oracle(gpu, lib, oracle, fused_case, key_case):
    """tkv_wal_encode (host layout, one CRC batch on the GPU, the fields stamped on the host) on the
    grids and on the giant records."""
    cases = [(fused_case[0].b, fused_case[1]), (key_case[0].b, key_case[1])]
    lb = long_batch(np.random.default_rng(928), geometry(lib)[0])
    cases.append((lb, expected(lb, oracle)))
    for b, (want, offs, crc) in cases:
        rc, size, img, guard, goff, gcrc = encode_host(lib, b, align=5, total=want.size)
        assert rc == OK and size == want.size
        assert guard, "bytes outside the destination were written"
        bad = np.flatnonzero(img != want)
        assert bad.size == 0, f"image differs at {bad[:8]} (first record {np.searchsorted(offs, bad[0], 'right') - 1})"
        assert np.array_equal(goff, offs) and np.array_equal(gcrc, crc)


def test_small_after_large(gpu, lib, oracle, loop_case, small_case):
    """The kept scratch (tile heads, read-back list, counters) after a large image: the 1000-record small
    batch and a batch of one record encode as on a fresh device."""
    b, exp = loop_case
    reps = sweeps(lib, 1)[1] // exp[0].size + 2
    db = DeviceBatch(tiled(b, reps), gpu)
    check_on(lib, db, tiled_expected(exp, reps), 3)
    assert last(lib)[1] > 1000
    sdb, (want, offs, crc) = small_case
    check(lib, sdb, want, offs, crc, align=3, fused_all=True)
    for klen, vlen, nlong in (([9], [30], 0), ([7], [300], 1)):
        one = make_batch(np.random.default_rng(929), klen, vlen)
        check_on(lib, DeviceBatch(one, gpu), expected(one, oracle), 3)
        assert last(lib)[:2] == [1 - nlong, nlong]
