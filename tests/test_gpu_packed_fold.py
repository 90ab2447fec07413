"""The packed kernel's segment fold (crc_packed<*, true>, tkv_crc32_fold.h) against the oracle.

Every case runs through tk.crc32_batch_uniform with tkv_debug_set_packed_fold on and off; both must
equal the oracle, so they equal each other. A uniform batch reaches crc_packed when its blocks are a
multiple of 4 KiB, back to back, 16-byte aligned and at least as many as the grid has waves (256
workgroups x 16 waves = 4096); smaller batches of the same shapes take the other uniform kernels, which
the switch must leave alone.
"""
import numpy as np
import pytest

import tinykvpp_amd as tk

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROW = 4096
WAVES = 4096


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def both_ways(lib, run):
    """run() with the fold on, then off; the switch is put back afterwards."""
    prev = lib.tkv_debug_set_packed_fold(1)
    try:
        on = run()
        lib.tkv_debug_set_packed_fold(0)
        off = run()
    finally:
        lib.tkv_debug_set_packed_fold(prev)
    return on, off


def check_uniform(lib, gpu, oracle, host, blen, n, init=None, offset=0, algo="crc32"):
    d = torch.from_numpy(host).to(gpu)
    ini = None if init is None else torch.from_numpy(init.view(np.int32)).to(gpu)
    offs = offset + np.arange(n, dtype=np.int64) * blen
    if algo == "crc32":
        want = oracle.batch(host, offs, np.full(n, blen), init)
    else:
        assert init is None
        want = np.array([oracle.crc_c(host[int(o):int(o) + blen].tobytes()) for o in offs], np.uint32)
    on, off = both_ways(lib, lambda: u32(tk.crc32_batch_uniform(d, blen, n, init_raw=ini, offset=offset, algo=algo)))
    assert np.array_equal(on, want), ("fold on", blen, n)
    assert np.array_equal(off, want), ("fold off", blen, n)


def random_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def test_switch_returns_previous(lib):
    prev = lib.tkv_debug_set_packed_fold(0)
    assert lib.tkv_debug_set_packed_fold(1) == 0
    assert lib.tkv_debug_set_packed_fold(prev) == 1


def basis_blocks(lane, bit, extra):
    """One 4 KiB block per (lane, bit): zero except that stream bit of that lane's segment; then
    `extra` - 1 all-0xFF blocks and one all-zero block."""
    k = lane.size
    host = np.zeros((k + extra) * ROW, np.uint8)
    host[np.arange(k) * ROW + lane * 64 + bit // 8] = (1 << (bit % 8)).astype(np.uint8)
    host[k * ROW:(k + extra - 1) * ROW] = 0xFF
    return host


def test_basis_batch(lib, gpu, oracle):
    """4096 blocks, block i zero except stream bit i % 512 of lane (7 i) % 64's segment: every stream
    bit's fold path and every lane-shift column (bit b always meets lane (7 b) % 64, 512 distinct
    pairs eight times over). Then 62 all-0xFF blocks and one all-zero block."""
    i = np.arange(4096)
    lane, bit = (7 * i) % 64, i % 512
    assert set(lane.tolist()) == set(range(64)) and set(bit.tolist()) == set(range(512))
    check_uniform(lib, gpu, oracle, basis_blocks(lane, bit, 63), ROW, 4096 + 63)


def test_basis_batch_rotated_lanes(lib, gpu, oracle):
    """The same with lane (7 i + i // 512) % 64: every stream bit in eight different lanes, 4096
    distinct (lane, bit) pairs."""
    i = np.arange(4096)
    lane, bit = (7 * i + i // 512) % 64, i % 512
    assert len(set(zip(lane.tolist(), bit.tolist()))) == 4096
    check_uniform(lib, gpu, oracle, basis_blocks(lane, bit, 63), ROW, 4096 + 63)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, WAVES - 1, WAVES, WAVES + 1, 3 * WAVES + 5])
def test_wave_range_edges(lib, gpu, oracle, n):
    """Random 4 KiB blocks. From 4096 blocks on the batch is crc_packed's: waves with 1 row (the tail
    body), 2 rows (one interleaved pair) and 3-4 rows, and the partial 64-result store; below, the
    other uniform kernels."""
    check_uniform(lib, gpu, oracle, random_bytes(n, n * ROW), ROW, n)


@pytest.mark.parametrize("blen", [2 * ROW, 3 * ROW, 16 * ROW])
@pytest.mark.parametrize("n", [1, 5, 257])
def test_several_rows_per_block(lib, gpu, oracle, blen, n):
    check_uniform(lib, gpu, oracle, random_bytes(blen + n, n * blen), blen, n)


@pytest.mark.parametrize("blen,n", [(2 * ROW, 6000), (3 * ROW, WAVES + 5)])
def test_several_rows_per_block_packed(lib, gpu, oracle, blen, n):
    """Enough blocks for crc_packed<false, *>: the Horner step over a block's rows and the skewed
    partition (waves of one workgroup with different block counts)."""
    check_uniform(lib, gpu, oracle, random_bytes(blen + n, n * blen), blen, n)


@pytest.mark.parametrize("blen,n", [(ROW, 1000), (2 * ROW, 1000), (ROW, WAVES + 1), (2 * ROW, WAVES + 3)])
def test_per_block_init(lib, gpu, oracle, blen, n):
    init = np.random.default_rng(n).integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    check_uniform(lib, gpu, oracle, random_bytes(blen * 3 + n, n * blen), blen, n, init=init)


@pytest.mark.parametrize("blen,n", [(ROW, 1000), (16 * ROW, 1000), (ROW, WAVES + 4), (2 * ROW, WAVES + 4)])
def test_crc32c_keeps_the_table_path(lib, gpu, oracle, blen, n):
    """CRC-32C has no such multiple: with the switch on its batches still take crc_packed<*, false>."""
    check_uniform(lib, gpu, oracle, random_bytes(blen + 7 * n, n * blen), blen, n, algo="crc32c")


@pytest.mark.parametrize("n", [1000, WAVES + 4])
def test_data_offset(lib, gpu, oracle, n):
    host = random_bytes(16 + n, 16 + n * ROW)
    check_uniform(lib, gpu, oracle, host, ROW, n, offset=16)
