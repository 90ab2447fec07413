"""crc_packed on 4 KiB blocks: kept result registers and the chunk-strided block order.

Two switches pick, inside one library, how a packed batch of 4 KiB blocks is walked:
tkv_debug_set_packed_window (result registers a wave keeps before it stores any) and
tkv_debug_set_packed_order (chunks of C = 16 blocks dealt out round-robin, 0 = one range per wave). Every case
runs the same batch with the new settings and with both off (the kernel as it was); the two result
arrays must be equal, and the blocks at the seams of the order (a wave's first and last block of a chunk,
of a 64-result register, of its share of the remainder; the batch's first and last) must equal the
oracle's CRC of the generator's bytes.

W is the grid's wave count, 16 x the device's CUs. Blocks come from one device buffer of synthetic 4 KiB
blocks (block i = the generator's block i), filled once and never written again.
"""
import ctypes

import numpy as np
import pytest

import tinykvpp_amd as tk

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROW = 4096
SEED = 1
OLD = (0, 0)  # window, order: the kernel before the switches existed
C = 16        # kPackedChunk


def u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def waves(gpu):
    return 16 * torch.cuda.get_device_properties(gpu).multi_processor_count


@pytest.fixture(scope="module")
def blocks(gpu, waves):
    """193 W + 7 synthetic 4 KiB blocks (a wave with 193 blocks fills three registers and starts a fourth)."""
    n = 193 * waves + 7
    d = torch.empty(n * ROW, dtype=torch.uint8, device=gpu)
    tk.fill_synthetic_uniform(d, ROW, n, first_block=0, seed=SEED)
    torch.cuda.synchronize()
    return d


class Settings:
    def __init__(self, lib, window, order):
        self.lib, self.new = lib, (window, order)

    def __enter__(self):
        lib, (w, o) = self.lib, self.new
        self.prev = (lib.tkv_debug_set_packed_window(w), lib.tkv_debug_set_packed_order(o))

    def __exit__(self, *exc):
        lib, (w, o) = self.lib, self.prev
        lib.tkv_debug_set_packed_window(w)
        lib.tkv_debug_set_packed_order(o)


def seam_blocks(n, W, C):
    """Batch indices at the seams of the order for a few waves (crc_packed_body's block_of restated)."""
    rounds = n // (W * C) if C else 0
    done = rounds * W * C
    rest = n - done
    picks = {0, n - 1}
    for w in (0, 1, W // 2, W - 1):
        for c in (0, 3, 4, rounds - 1):
            if 0 <= c < rounds:
                first = (c * W + w) * C
                picks |= {first, first + C - 1}
        t0, t1 = done + w * rest // W, done + (w + 1) * rest // W
        if t1 > t0:
            picks |= {t0, t0 + min(63, t1 - t0 - 1), t1 - 1}
    return sorted(picks)


def oracle_blocks(oracle, idx, init=None, algo="crc32", uniform_init=None):
    want = np.zeros(len(idx), np.uint32)
    for k, b in enumerate(idx):
        if init is None and uniform_init is None and algo == "crc32":
            want[k] = oracle.synthetic(SEED, b, 1, ROW)[0]
            continue
        data = oracle.fill(SEED, b, 0, ROW).tobytes()
        if algo == "crc32c":
            want[k] = oracle.crc_c(data)
        else:
            start = int(init[b]) if init is not None else uniform_init
            want[k] = oracle.update(start, data) ^ 0xFFFFFFFF
    return want


def check(lib, oracle, blocks, W, n, new, init=None, algo="crc32", uniform_init=None, out=None):
    """The first n blocks with settings `new` and with OLD: equal arrays, seam blocks equal the oracle."""
    ini = None if init is None else torch.from_numpy(init.view(np.int32)).to(blocks.device)

    def run():
        if uniform_init is None:
            r = tk.crc32_batch_uniform(blocks, ROW, n, init_raw=ini, algo=algo, out=out)
        else:
            r = torch.empty(n, dtype=torch.int32, device=blocks.device) if out is None else out
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            rc = lib.tkv_debug_batch_uniform_init_device(ctypes.c_void_p(blocks.data_ptr()), ROW, ROW, uniform_init,
                                                         ctypes.c_void_p(r.data_ptr()), n, st)
            assert rc == 0
        return r.clone()

    with Settings(lib, *new):
        got_new = run()
    with Settings(lib, *OLD):
        got_old = run()
    assert torch.equal(got_new, got_old), ("new settings differ from old", new, n)
    idx = sorted(set(seam_blocks(n, W, C if new[1] else 0)) | set(seam_blocks(n, W, 0)))
    want = oracle_blocks(oracle, idx, init=init, algo=algo, uniform_init=uniform_init)
    got = u32(got_new[torch.tensor(idx, device=got_new.device)])
    bad = [(b, hex(g), hex(w)) for b, g, w in zip(idx, got, want) if g != w]
    assert not bad, (new, n, bad[:8])
    return got_new


def test_switches_return_previous(lib):
    for setter, other, default in ((lib.tkv_debug_set_packed_window, 2, 4), (lib.tkv_debug_set_packed_order, 0, 1)):
        prev = setter(other)
        assert prev == default
        assert setter(prev) == other
    # a window outside 0..4 is clamped
    assert lib.tkv_debug_set_packed_window(9) == 4 and lib.tkv_debug_set_packed_window(4) == 4


@pytest.mark.parametrize("n_of_w", [lambda W: W, lambda W: W + 1, lambda W: 2 * W - 1, lambda W: 3 * W + 17],
                         ids=["W", "W+1", "2W-1", "3W+17"])
def test_small_batches(lib, oracle, blocks, waves, n_of_w):
    """The smallest packed batch, its neighbours and an uneven split: fewer than W * C blocks, so every
    block is remainder; all of them against the oracle."""
    n = n_of_w(waves)
    got = check(lib, oracle, blocks, waves, n, (4, 1))
    assert np.array_equal(u32(got), oracle.synthetic(SEED, 0, n, ROW))


@pytest.mark.parametrize("window", [0, 4])
@pytest.mark.parametrize("n_of_w", [lambda W: W * C - 1, lambda W: W * C, lambda W: W * C + 1,
                                    lambda W: 2 * W * C + W // 2 + 3], ids=["WC-1", "WC", "WC+1", "2WC+W/2+3"])
def test_rounds_and_remainder(lib, oracle, blocks, waves, window, n_of_w):
    """No whole round, exactly one, one and a single block over (one wave with one more block), and two
    rounds with a remainder that only every other wave shares."""
    check(lib, oracle, blocks, waves, n_of_w(waves), (window, 1))


@pytest.mark.parametrize("order", [0, 1])
def test_window_overflow(lib, oracle, blocks, waves, order):
    """Window 1 and 65 blocks per wave: the smallest batch in which a wave fills its window and stores a
    register inside the row loop, against window 0."""
    check(lib, oracle, blocks, waves, 65 * waves, (1, order))


@pytest.mark.parametrize("window,per_wave", [(2, 129), (3, 193), (4, 193), (4, 130)])
def test_held_registers(lib, oracle, blocks, waves, window, per_wave):
    """Windows of two and three registers overflowing (the oldest held register goes out), and a window
    of four holding two and three full registers to the end."""
    check(lib, oracle, blocks, waves, per_wave * waves + 5, (window, 1))


def test_per_block_init(lib, oracle, blocks, waves):
    """Per-block initial registers, read at the block's batch index."""
    n = waves * C + 3 * waves + 17
    init = np.random.default_rng(n).integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    check(lib, oracle, blocks, waves, n, (4, 1), init=init)


@pytest.mark.parametrize("reg", [0, 0x12345678])
def test_uniform_init_register(lib, oracle, blocks, waves, reg):
    """A uniform initial register other than 0xFFFFFFFF."""
    check(lib, oracle, blocks, waves, C * waves + 3 * waves + 17, (4, 1), uniform_init=reg)


def test_crc32c_table_kernel(lib, oracle, blocks, waves):
    """CRC-32C takes the table-only kernel; the switches apply to it as well."""
    check(lib, oracle, blocks, waves, waves * C + waves // 2 + 3, (4, 1), algo="crc32c")


def test_out_view_at_odd_element(lib, oracle, blocks, waves):
    """`out` starting 3 elements into an allocation: the 64-result stores start at no 256-byte boundary."""
    n = 2 * waves * C + waves // 2 + 3
    backing = torch.full((n + 8,), 0x5A5A5A5A, dtype=torch.int32, device=blocks.device)
    check(lib, oracle, blocks, waves, n, (4, 1), out=backing[3:3 + n])
    assert bool((backing[:3] == 0x5A5A5A5A).all()) and bool((backing[3 + n:] == 0x5A5A5A5A).all())


def test_64k_blocks_unchanged(lib, gpu, oracle, waves):
    """64 KiB blocks at n = W + 3: the multi-row kernel takes neither switch."""
    blen, n = 16 * ROW, waves + 3
    d = torch.empty(n * blen, dtype=torch.uint8, device=gpu)
    tk.fill_synthetic_uniform(d, blen, n, first_block=0, seed=SEED)
    with Settings(lib, 4, 1):
        new = tk.crc32_batch_uniform(d, blen, n).clone()
    with Settings(lib, *OLD):
        old = tk.crc32_batch_uniform(d, blen, n).clone()
    assert torch.equal(new, old)
    idx = sorted({0, 1, 63, 64, waves // 2, waves - 1, waves, n - 1})
    want = np.array([oracle.synthetic(SEED, b, 1, blen)[0] for b in idx], np.uint32)
    assert np.array_equal(u32(new)[idx], want)
