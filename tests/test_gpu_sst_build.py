"""tkv_sst_build_device on the GPU against the sequential writer-loop oracle (tests/sst_build_util.py):
the whole file byte for byte at the scan-block, wave and doubling-round edges, the varint and tile
edges, overlapping sources, sizing / overflow / invalid arguments with canaried outputs, the fuzz seeds,
the round trips through the verify calls, recover-then-flush from a WAL image, and concurrent callers."""
import ctypes
import math
import struct
import threading
import zlib

import numpy as np
import pytest
import torch

import wal_fuzz_util as fz
from sst_build_util import FUZZ_SEEDS, arenas, edge_cases, fuzz_case, oracle_file
from tinykvpp_amd import sst, wal
from tinykvpp_amd._lib import BUFFER_OVERFLOW, INVALID_ARGUMENT, OK

pytestmark = pytest.mark.gpu
CANARY = 0xC7


def upload(gpu, cols):
    """The numpy arenas as CUDA tensors in the dtypes wal.decode_device returns."""
    keys, koff, klen, vals, voff, vlen = cols
    t = lambda a, dt: torch.from_numpy(a.view(dt)).to(gpu)  # noqa: E731
    return (t(keys, np.uint8), t(koff, np.int64), t(klen, np.int32), t(vals, np.uint8), t(voff, np.int64), t(vlen, np.int32))


def first_diff(got, want):
    if len(got) != len(want):
        return f"sizes differ: {len(got)} != {len(want)}"
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    bad = np.flatnonzero(a != b)
    return f"{bad.size} bytes differ, the first at {int(bad[0])} of {len(want)} (tile {int(bad[0]) // 4096})"


def rounds_expected(entries, target):
    total = sum(8 + len(k) + len(v) for k, v in entries)
    bmax = min(len(entries), total // target + 1)
    return math.ceil(math.log2(bmax + 1))


def check_build(gpu, lib, entries, target, misalign=0, dev_cols=None, want=None):
    """build_device of ``entries`` at destination misalignment ``misalign`` equals the oracle: the file,
    the sizes, the block arrays, the canaries on both sides, and what the call says it did."""
    want, blocks, ioff, isz = oracle_file(entries, target) if want is None else want
    d = upload(gpu, arenas(entries)) if dev_cols is None else dev_cols
    buf = torch.full((64 + len(want) + 64,), CANARY, dtype=torch.uint8, device=gpu)
    start = 16 + (-(buf.data_ptr() + 16) % 16) + misalign
    res = sst.build_device(*d, target_block_size=target, out=buf[start:start + len(want)])
    last = (ctypes.c_uint64 * 4)()
    lib.tkv_debug_sst_build_last(last)
    host = buf.cpu().numpy()
    got = host[start:start + len(want)].tobytes()
    assert (res.size, res.index_offset, res.index_size) == (len(want), ioff, isz)
    assert got == want, first_diff(got, want)
    assert (host[:start] == CANARY).all() and (host[start + len(want):] == CANARY).all(), "a canary byte changed"
    assert res.file.data_ptr() == buf.data_ptr() + start
    assert res.block_off.cpu().tolist() == [b[0] for b in blocks]
    assert res.block_size.cpu().numpy().view(np.uint32).tolist() == [b[1] for b in blocks]
    assert res.block_first.cpu().numpy().view(np.uint32).tolist() == [b[2] for b in blocks]
    assert last[0] == len(blocks) and last[3] == len(want) and last[2] >= 16
    assert last[1] == rounds_expected(entries, target), "doubling rounds"
    return res, want


def small_entries(n, seed=0):
    rng = np.random.default_rng(1000 + seed)
    blob = rng.integers(0, 256, 4096, dtype=np.uint8).tobytes()
    kl, vl = rng.integers(0, 24, n), rng.integers(0, 41, n)
    ko, vo = rng.integers(0, 4000, n), rng.integers(0, 4000, n)
    return [(blob[ko[i]:ko[i] + kl[i]], blob[vo[i]:vo[i] + vl[i]]) for i in range(n)]


# ---- parity of the whole file --------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1023, 1024, 1025, 4097])
@pytest.mark.parametrize("target", [1, 4096, 1 << 30])
def test_parity_scan_and_wave_edges(gpu, lib, n, target):
    res, _ = check_build(gpu, lib, small_entries(n, n), target, misalign=n % 16)
    if target == 1:
        assert res.n_blocks == n
    if target == 1 << 30:
        assert res.n_blocks == 1


def test_parity_third_scan_level_empty_entries(gpu, lib):
    """1024 * 1024 + 1 empty entries with T = 4096: three scan levels, 512 entries per block."""
    n = 1024 * 1024 + 1
    z = np.zeros(n, np.int64)
    one = torch.zeros(1, dtype=torch.uint8, device=gpu)
    cols = (one, torch.from_numpy(z).to(gpu), torch.zeros(n, dtype=torch.int32, device=gpu)) * 2
    # the oracle's file without a million Python appends: 2048 identical full blocks and one of one entry
    full, _, _, _ = oracle_file([(b"", b"")] * 512, 4096)
    tail, _, _, _ = oracle_file([(b"", b"")], 4096)
    bsz = 36 + 4096
    assert len(full) == bsz + 8 + 1 + 16 + 20 and len(tail) == 44 + 8 + 1 + 16 + 20
    B = 2049
    data = full[:bsz] * 2048 + tail[:44]
    idx = struct.pack("<Q", B) + b"".join(b"\0" + struct.pack("<QQ", j * bsz, bsz if j < 2048 else 44) for j in range(B))
    foot = struct.pack("<IIII", len(data), len(idx), 0, 0)
    want = data + idx + foot + struct.pack("<I", zlib.crc32(idx + foot))
    blocks = [(j * bsz, bsz if j < 2048 else 44, j * 512) for j in range(B)]
    res = sst.build_device(*cols, target_block_size=4096)
    got = res.file.cpu().numpy().tobytes()
    assert got == want, first_diff(got, want)
    assert res.block_first.cpu().tolist() == [b[2] for b in blocks] and res.block_off.cpu().tolist() == [b[0] for b in blocks]
    last = (ctypes.c_uint64 * 4)()
    lib.tkv_debug_sst_build_last(last)
    assert list(last)[:2] == [B, math.ceil(math.log2(min(n, 8 * n // 4096 + 1) + 1))]
    assert len(want) > 8 << 20


# ---- chain lengths around the doubling rounds -----------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 65537])
def test_chain_lengths_every_entry_a_block(gpu, lib, n):
    res, _ = check_build(gpu, lib, small_entries(n, 77 + n) if n < 1000 else [(b"k", b"")] * n, 1)
    assert res.n_blocks == n


def test_chain_uniform_entries_never_merge(gpu, lib):
    """Uniform 41-byte entries (counted 49): a chain from any other start never meets the true one."""
    entries = [(b"0123456789abcdef", b"v" * 25)] * 50_000
    res, _ = check_build(gpu, lib, entries, 4096)
    assert res.n_blocks == math.ceil(50_000 / 84)  # 84 * 49 = 4116 >= 4096 > 83 * 49


# ---- varint edges ---------------------------------------------------------------------------------------

VLENS = [0, 1, 127, 128, 16383, 16384, 2097151, 2097152]


def test_varint_edges_of_key_and_value_lengths(gpu, lib):
    rng = np.random.default_rng(3)
    blob = rng.integers(0, 256, 2097152, dtype=np.uint8).tobytes()
    entries = [(blob[:kl], blob[-vl:] if vl else b"") for kl, vl in zip(VLENS, VLENS[::-1])]
    entries += [(blob[5:5 + kl], blob[9:9 + vl]) for kl in VLENS[:6] for vl in VLENS[:6]]
    check_build(gpu, lib, entries, 4096, misalign=3)
    check_build(gpu, lib, entries, 1 << 30, misalign=11)


@pytest.mark.parametrize("name", sorted(edge_cases()))
def test_cut_and_block_size_varint_edges(gpu, lib, name):
    entries, target = edge_cases()[name]
    check_build(gpu, lib, entries, target)


# ---- tile edges -----------------------------------------------------------------------------------------

def test_header_varint_and_slack_across_a_tile_boundary(gpu, lib):
    """Block 0 = a leading entry of key length L and a 4004-byte value, closed exactly by T: block 1's
    header starts at 4056 + L, so over L = 0..63 the 24 zero bytes that end block 0 (11 of slack, 13 of
    padding), block 1's 21-byte header, its varint(z) and the varints of its first entries each straddle
    file byte 4096 at every phase."""
    rest = small_entries(30, 5)
    for L in range(64):
        entries = [(b"L" * L, b""), (b"", b"F" * 4004)] + rest
        target = 16 + L + 4004
        res, want = check_build(gpu, lib, entries, target, misalign=L % 16)
        assert res.block_off.cpu().tolist()[1] == 4056 + L


def test_tiles_without_entries_and_tiles_of_headers(gpu, lib):
    """T = 65536 with empty keys and values: three quarters of every body is slack, whole tiles hold no
    entry and most hold no header. T = 1 with empty entries: 44-byte blocks, about 93 headers per tile."""
    check_build(gpu, lib, [(b"", b"")] * 20_000, 65536, misalign=5)
    check_build(gpu, lib, [(b"", b"")] * 3000, 1, misalign=9)


def test_one_mib_value_between_small_entries(gpu, lib):
    rng = np.random.default_rng(8)
    big = rng.integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    entries = small_entries(100, 1)[:90] + [(b"big", big)] + small_entries(100, 2)
    check_build(gpu, lib, entries, 4096, misalign=7)


@pytest.mark.parametrize("misalign", range(16))
def test_destination_misalignment(gpu, lib, misalign):
    entries, target = fuzz_case(6)
    check_build(gpu, lib, entries[:400], target, misalign=misalign)


# ---- sources --------------------------------------------------------------------------------------------

def test_overlapping_and_gapped_sources(gpu, lib):
    """Every entry shares one key; the values overlap one another inside a small arena with gaps."""
    rng = np.random.default_rng(12)
    arena = rng.integers(0, 256, 700, dtype=np.uint8)
    n = 3000
    klen = np.full(n, 17, np.uint32)
    koff = np.full(n, 5, np.uint64)
    vlen = rng.integers(0, 200, n).astype(np.uint32)
    voff = rng.integers(0, 500, n).astype(np.uint64)
    a = arena.tobytes()
    entries = [(a[5:22], a[int(o):int(o) + int(ln)]) for o, ln in zip(voff, vlen)]
    check_build(gpu, lib, entries, 4096, dev_cols=upload(gpu, (arena, koff, klen, arena, voff, vlen)), misalign=13)
    # no value column: every value is empty
    want = oracle_file([(k, b"") for k, _ in entries], 100)
    d = upload(gpu, (arena, koff, klen, arena, voff, vlen))
    res = sst.build_device(d[0], d[1], d[2], target_block_size=100)
    assert res.file.cpu().numpy().tobytes() == want[0]


# ---- sizing and errors ----------------------------------------------------------------------------------

def raw_call(lib, d, n, target, file, cap, arrays, bcap, stream=None):
    sizes = [ctypes.c_uint64(0xDEADBEEF) for _ in range(4)]
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib.tkv_sst_build_device(*[p(t) for t in d], n, target, p(file), cap, *[p(a) for a in arrays], bcap,
                                  *[ctypes.byref(s) for s in sizes], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, tuple(s.value for s in sizes)


def test_sizing_overflow_and_exact_caps(gpu, lib):
    entries, target = fuzz_case(2)
    want, blocks, ioff, isz = oracle_file(entries, target)
    full = (len(want), len(blocks), ioff, isz)
    d = upload(gpu, arenas(entries))
    n, B = len(entries), len(blocks)
    assert raw_call(lib, d, n, target, None, 0, (None, None, None), 0) == (BUFFER_OVERFLOW, full)  # the sizing call
    file = torch.full((len(want) + 64,), CANARY, dtype=torch.uint8, device=gpu)
    arrays = (torch.full((B,), -7, dtype=torch.int64, device=gpu), torch.full((B,), -7, dtype=torch.int32, device=gpu),
              torch.full((B,), -7, dtype=torch.int32, device=gpu))
    for cap, bcap in ((len(want) - 1, B), (len(want), B - 1)):
        assert raw_call(lib, d, n, target, file, cap, arrays, bcap) == (BUFFER_OVERFLOW, full)
        torch.cuda.synchronize()
        assert bool((file == CANARY).all()) and all(bool((a == -7).all()) for a in arrays)
    # too few block entries do not matter when no block array is asked for
    assert raw_call(lib, d, n, target, file, len(want), (None, None, None), 0) == (OK, full)
    assert file[:len(want)].cpu().numpy().tobytes() == want and bool((file[len(want):] == CANARY).all())
    file.fill_(CANARY)
    assert raw_call(lib, d, n, target, file, len(want), arrays, B) == (OK, full)  # exact caps
    assert file[:len(want)].cpu().numpy().tobytes() == want and bool((file[len(want):] == CANARY).all())
    assert arrays[2].cpu().tolist() == [b[2] for b in blocks]


def test_invalid_arguments_write_nothing(gpu, lib):
    entries = small_entries(50, 3)
    d = upload(gpu, arenas(entries))
    file = torch.full((1 << 16,), CANARY, dtype=torch.uint8, device=gpu)
    arrays = tuple(torch.full((64,), -7, dtype=dt, device=gpu) for dt in (torch.int64, torch.int32, torch.int32))
    untouched = (0xDEADBEEF,) * 4

    def clean():
        torch.cuda.synchronize()
        return bool((file == CANARY).all()) and all(bool((a == -7).all()) for a in arrays)
    for dd, n, target in ((d, 0, 64), (d, 1 << 32, 64), (d, 50, 0), ((None,) + d[1:], 50, 64), (d[:1] + (None,) + d[2:], 50, 64),
                          (d[:2] + (None,) + d[3:], 50, 64), (d[:3] + (None,) + d[4:], 50, 64), (d[:4] + (None, d[5]), 50, 64)):
        assert raw_call(lib, dd, n, target, file, file.numel(), arrays, 64) == (INVALID_ARGUMENT, untouched)
        assert clean()
    assert raw_call(lib, d, 50, 64, None, 1 << 16, arrays, 64) == (INVALID_ARGUMENT, untouched) and clean()
    # lengths of 2^28 and more over a tiny arena: decided on the device from the lengths alone
    tiny = torch.zeros(1, dtype=torch.uint8, device=gpu)
    off = torch.zeros(3, dtype=torch.int64, device=gpu)
    zero = torch.zeros(3, dtype=torch.int32, device=gpu)
    for bad in (1 << 28, (1 << 32) - 1, 1 << 31):
        ln = torch.from_numpy(np.array([0, bad, 0], np.uint32).view(np.int32)).to(gpu)
        for dd in ((tiny, off, ln, tiny, off, zero), (tiny, off, zero, tiny, off, ln)):
            assert raw_call(lib, dd, 3, 4096, file, file.numel(), arrays, 64) == (INVALID_ARGUMENT, untouched) and clean()
    # a block and a file beyond u32, from entries that share one (never read) span
    n, ln = 40, 1 << 27
    big = (tiny, torch.zeros(n, dtype=torch.int64, device=gpu), torch.full((n,), ln, dtype=torch.int32, device=gpu),
           tiny, torch.zeros(n, dtype=torch.int64, device=gpu), torch.zeros(n, dtype=torch.int32, device=gpu))
    for m, target in ((40, (1 << 32) - 1), (40, 1 << 30), (31, (1 << 32) - 1)):
        assert raw_call(lib, big, m, target, file, 1 << 40, arrays, 64) == (INVALID_ARGUMENT, untouched) and clean()


# ---- fuzz -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_fuzz(gpu, lib, seed):
    entries, target = fuzz_case(seed)
    rng = np.random.default_rng(seed)
    cols = arenas(entries, rng, gaps=seed % 2 == 1)
    check_build(gpu, lib, entries, target, misalign=seed % 16, dev_cols=upload(gpu, cols))


# ---- round trips ----------------------------------------------------------------------------------------

def test_round_trips_and_flipped_bits(gpu, lib):
    entries, target = fuzz_case(9)
    res, want = check_build(gpu, lib, entries, target)
    file = res.file.cpu().numpy().copy()
    idx = sst.read_index(file)
    offs, sizes = [o for _, o, _ in idx], [s for _, _, s in idx]
    assert offs == res.block_off.cpu().tolist() and sizes == res.block_size.cpu().tolist()
    assert [k for k, _, _ in idx] == [entries[f][0] for f in res.block_first.cpu().tolist()]
    assert sst.verify_blocks(file, offs, sizes) == ("ok", 0, len(idx))
    ioff, isz = res.index_offset, res.index_size
    assert sst.verify_footer(file[ioff:ioff + isz], file[ioff + isz:].tobytes()) == "ok"
    crcs = sst.block_crcs_device(res.file, res.block_off, res.block_size).cpu().numpy().view(np.uint32)
    stored = np.array([int.from_bytes(want[o + 17:o + 21], "little") for o in offs], np.uint32)
    assert np.array_equal(crcs, stored)
    # one flipped bit in a block, in the index, in the footer
    j = len(idx) // 2
    bad = file.copy()
    bad[offs[j] + sizes[j] // 2] ^= 4
    assert sst.verify_blocks(bad, offs, sizes) == ("corrupted", 1, j)
    bad = file.copy()
    bad[ioff + isz // 2] ^= 1
    assert sst.verify_footer(bad[ioff:ioff + isz], bad[ioff + isz:].tobytes()) == "corrupted"
    with pytest.raises(ValueError):
        sst.read_index(bad)
    bad = file.copy()
    bad[ioff + isz + 9] ^= 0x80
    assert sst.verify_footer(bad[ioff:ioff + isz], bad[ioff + isz:].tobytes()) == "corrupted"
    with pytest.raises(ValueError):
        sst.read_index(bad)


def test_host_build_equals_the_oracle(gpu, lib):
    entries, target = fuzz_case(13)
    want, blocks, ioff, isz = oracle_file(entries, target)
    res = sst.build(entries, target)
    assert res.file.tobytes() == want and (res.index_offset, res.index_size) == (ioff, isz)
    assert [(int(o), int(s), int(f)) for o, s, f in zip(res.block_off, res.block_size, res.block_first)] == blocks
    res = sst.build(arenas(entries, np.random.default_rng(1), gaps=True), target)
    assert res.file.tobytes() == want


def test_phase_times_only_when_enabled(gpu, lib):
    """tkv_debug_sst_build_phases: four phase times of this thread's last build while enabled, zeros after
    a build with the timing off."""
    entries, target = fuzz_case(3)
    ms = (ctypes.c_double * 4)()
    assert lib.tkv_debug_sst_build_phases(1, None) == 0
    try:
        check_build(gpu, lib, entries, target)
        assert lib.tkv_debug_sst_build_phases(1, ms) == 1 and all(v > 0 for v in ms), list(ms)
    finally:
        lib.tkv_debug_sst_build_phases(0, None)
    check_build(gpu, lib, entries, target)
    assert lib.tkv_debug_sst_build_phases(0, ms) == 0 and list(ms) == [0, 0, 0, 0]


# ---- recover, then flush --------------------------------------------------------------------------------

def test_recover_then_flush_from_the_wal_image(gpu, lib, oracle):
    """A WAL image through index_device and decode_device with both view flags, then build_device reading
    keys and values straight out of the image."""
    rng = np.random.default_rng(31)
    img, offs, _ = fz.build(rng, oracle, "mixed", 3000)
    image = torch.from_numpy(img).to(gpu)
    status, rec_off, stop, _ = wal.index_device(image)
    assert status == "ok" and rec_off.numel() == offs.size and stop == img.size
    b = wal.decode_device(image, rec_off, key_views=True, val_views=True)
    assert b.keys.data_ptr() == image.data_ptr() and b.vals.data_ptr() == image.data_ptr()
    raw = img.tobytes()
    entries = []
    for o in offs.astype(np.int64).tolist():
        kl, vl = int.from_bytes(raw[o + 18:o + 22], "little"), int.from_bytes(raw[o + 22:o + 26], "little")
        entries.append((raw[o + 26:o + 26 + kl], raw[o + 26 + kl:o + 26 + kl + vl]))
    check_build(gpu, lib, entries, 4096, dev_cols=(b.keys, b.key_off, b.key_len, b.vals, b.val_off, b.val_len))


# ---- threads --------------------------------------------------------------------------------------------

def test_four_threads_build_at_once(gpu, lib):
    """Four host threads, each on its own stream with its own input, released together: the per-device
    scratch and the pinned result block are shared under the library's mutex, the `last build` words are
    thread-local."""
    work = []
    for t in range(4):
        entries, target = fuzz_case(20 + t)
        work.append((entries, target, oracle_file(entries, target)))
    barrier = threading.Barrier(4)
    failures, passes = [], []

    def run(t):
        try:
            entries, target, want = work[t]
            stream = torch.cuda.Stream(gpu)
            with torch.cuda.stream(stream):
                d = upload(gpu, arenas(entries))
                stream.synchronize()
                barrier.wait(60)
                for rnd in range(3):
                    check_build(gpu, lib, entries, target, misalign=(5 * t + rnd) % 16, dev_cols=d, want=want)
                    passes.append((t, rnd))
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            failures.append((t, repr(e)))
            barrier.abort()

    threads = [threading.Thread(target=run, args=(t,), daemon=True) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(120)
    assert not any(th.is_alive() for th in threads), "a caller is still running after 120 s"
    assert not failures, failures
    assert len(passes) == 12
