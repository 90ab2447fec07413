"""tkv_sst_scan_device on the GPU against the sequential reader oracle (tests/sst_scan_util.py): round trips
through build_device, the byte-for-byte rebuild, the parse window's and the index chain's edges at every
file misalignment, views against copies, every catalogue mutation and every single-bit flip of a small
file with canaried outputs, sizing and overflow, the empty table, the WAL pipeline, the host variant and
concurrent callers."""
import ctypes
import math
import threading

import numpy as np
import pytest
import torch

import sst_scan_util as su
import wal_fuzz_util as fz
from sst_build_util import FUZZ_SEEDS, arenas, edge_cases, fuzz_case, oracle_file
from tinykvpp_amd import sst, wal
from tinykvpp_amd._lib import BUFFER_OVERFLOW, CORRUPTED, OK

pytestmark = pytest.mark.gpu
CANARY = 0xC7
WINDOW = 4096  # tkv_debug_sst_scan_geometry()[0]


def upload(gpu, cols):
    keys, koff, klen, vals, voff, vlen = cols
    t = lambda a, dt: torch.from_numpy(a.view(dt)).to(gpu)  # noqa: E731
    return (t(keys, np.uint8), t(koff, np.int64), t(klen, np.int32), t(vals, np.uint8), t(voff, np.int64), t(vlen, np.int32))


def dev_file(gpu, file_bytes, misalign=0):
    """The file on the device at byte misalignment ``misalign`` of a 16-byte granule, canaries around it."""
    n = len(file_bytes)
    buf = torch.full((48 + n + 48,), CANARY, dtype=torch.uint8, device=gpu)
    start = 16 + (-(buf.data_ptr() + 16) % 16) + misalign
    buf[start:start + n] = torch.from_numpy(np.frombuffer(file_bytes, np.uint8).copy()).to(gpu)
    return buf[start:start + n]


def u32(t):
    return t.cpu().numpy().view(np.uint32).tolist()


def check_scan(gpu, file_bytes, misalign=0, key_views=False, val_views=False, want=None):
    """scan_device of the file equals the oracle's entries and blocks."""
    status, _, ents, blocks = su.oracle_scan(file_bytes) if want is None else want
    assert status == "ok"
    f = dev_file(gpu, file_bytes, misalign)
    res = sst.scan_device(f, key_views=key_views, val_views=val_views)
    assert (res.n_entries, res.n_blocks) == (len(ents), len(blocks))
    assert res.entries() == ents
    assert [list(x) for x in zip(res.block_off.cpu().tolist(), u32(res.block_size), u32(res.block_first))] == \
        [list(b) for b in blocks]
    if key_views:
        assert res.keys.data_ptr() == f.data_ptr()
    else:
        assert res.key_off.cpu().tolist() == np.cumsum([0] + [len(k) for k, _ in ents])[:-1].tolist()
    if val_views:
        assert res.vals.data_ptr() == f.data_ptr()
    else:
        assert res.val_off.cpu().tolist() == np.cumsum([0] + [len(v) for _, v in ents])[:-1].tolist()
    return res


def small_entries(n, seed=0):
    rng = np.random.default_rng(1000 + seed)
    blob = rng.integers(0, 256, 4096, dtype=np.uint8).tobytes()
    kl, vl = rng.integers(0, 24, n), rng.integers(0, 41, n)
    ko, vo = rng.integers(0, 4000, n), rng.integers(0, 4000, n)
    return [(blob[ko[i]:ko[i] + kl[i]], blob[vo[i]:vo[i] + vl[i]]) for i in range(n)]


def round_trip(gpu, entries, target, misalign=0):
    """build_device -> scan_device gives the entries and the flush's block arrays back; scan_device ->
    build_device reproduces the file byte for byte."""
    built = sst.build_device(*upload(gpu, arenas(entries)), target_block_size=target)
    f = dev_file(gpu, built.file.cpu().numpy().tobytes(), misalign)
    res = sst.scan_device(f)
    assert res.n_entries == len(entries) and res.entries() == entries
    assert res.block_off.tolist() == built.block_off.tolist()
    assert u32(res.block_size) == u32(built.block_size) and u32(res.block_first) == u32(built.block_first)
    again = sst.build_device(res.keys, res.key_off, res.key_len, res.vals, res.val_off, res.val_len, target_block_size=target)
    assert torch.equal(again.file, built.file)
    # and out of the image itself
    v = sst.scan_device(f, key_views=True, val_views=True)
    again = sst.build_device(v.keys, v.key_off, v.key_len, v.vals, v.val_off, v.val_len, target_block_size=target)
    assert torch.equal(again.file, built.file)
    return res


# ---- round trips -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1023, 1025, 4097])
@pytest.mark.parametrize("target", [1, 4096, 1 << 30])
def test_round_trip_scan_and_wave_edges(gpu, n, target):
    res = round_trip(gpu, small_entries(n, n), target, misalign=n % 16)
    if target == 1:
        assert res.n_blocks == n
    if target == 1 << 30:
        assert res.n_blocks == 1


@pytest.mark.parametrize("name", sorted(edge_cases()))
def test_round_trip_edge_cases(gpu, name):
    entries, target = edge_cases()[name]
    round_trip(gpu, entries, target, misalign=len(name) % 16)


@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_round_trip_fuzz(gpu, seed):
    entries, target = fuzz_case(seed)
    round_trip(gpu, entries, target, misalign=seed % 16)


def test_phase_times_only_when_enabled(gpu, lib):
    """tkv_debug_sst_scan_phases: four phase times of this thread's last scan while enabled, zeros after a
    scan with the timing off. Copied arenas and every output: each phase (open and index, checksum, parse,
    emit) holds a launch."""
    entries, target = fuzz_case(3)
    file_bytes = oracle_file(entries, target)[0]
    want = su.oracle_scan(file_bytes)
    ms = (ctypes.c_double * 4)()
    assert lib.tkv_debug_sst_scan_phases(1, None) == 0
    try:
        check_scan(gpu, file_bytes, want=want)
        assert lib.tkv_debug_sst_scan_phases(1, ms) == 1 and all(v > 0 for v in ms), list(ms)
    finally:
        lib.tkv_debug_sst_scan_phases(0, None)
    check_scan(gpu, file_bytes, want=want)
    assert lib.tkv_debug_sst_scan_phases(0, ms) == 0 and list(ms) == [0, 0, 0, 0]


# ---- the parse window -------------------------------------------------------------------------------------

def test_geometry(lib):
    g = (ctypes.c_uint64 * 4)()
    lib.tkv_debug_sst_scan_geometry(g)
    assert g[0] == WINDOW and g[1] == 3 and g[2] == 4096


@pytest.mark.parametrize("start", range(WINDOW - 5, WINDOW + 3))
def test_varint_and_string_end_at_the_window_boundary(gpu, start):
    """Entry 1's 4-byte key length starts at body byte ``start``: it straddles the window boundary at each
    of its byte positions, and entry 0's value ends on the boundary, one byte before and one behind it."""
    a = start - 4  # varint(a) is 2 bytes, the empty value's is 2 (redundant)
    body = su.varint(a) + b"k" * a + su.varint(0, 1) + su.varint(5, 3) + b"hello" + su.varint(2, 3) + b"yo" + \
        su.varint(1) + b"z" + su.varint(0)
    assert body.index(su.varint(5, 3)) == start
    z = (8 + a) + (8 + 5 + 2) + (8 + 1)
    img = su.block_image([], c=3, z=z, body=body)
    file = su.make_file(img, su.index_image([(b"k" * a, 0, len(img))]))
    want = su.oracle_scan(file)
    assert want[2] == [(b"k" * a, b""), (b"hello", b"yo"), (b"z", b"")]
    for mis in range(16):
        check_scan(gpu, file, mis, want=want)


def test_string_skipping_more_than_two_windows(gpu):
    big = bytes(range(256)) * 50  # 12 800 bytes
    blocks = [[(b"a", big), (b"b", b"1"), (big, b""), (b"c", big[:5000])], [(b"d", b"")]]
    file = su.file_of_blocks(blocks)
    want = su.oracle_scan(file)
    for mis in range(16):
        check_scan(gpu, file, mis, want=want)


def test_block_of_more_than_two_windows_of_empty_entries(gpu):
    file = su.file_of_blocks([[(b"", b"")] * 5000, [(b"", b"")]])
    want = su.oracle_scan(file)
    assert len(want[2]) == 5001
    for mis in range(16):
        check_scan(gpu, file, mis, want=want)


def test_lengths_on_the_varint_edges_as_entries_and_index_keys(gpu):
    lens = (0, 127, 128, 16383, 16384)
    blocks = [[(bytes([65 + i]) * kl, bytes([97 + i]) * vl) for vl in lens] for i, kl in enumerate(lens)]
    file = su.file_of_blocks(blocks)
    want = su.oracle_scan(file)
    for mis in range(16):
        check_scan(gpu, file, mis, want=want)
    check_scan(gpu, file, 3, key_views=True, val_views=True, want=want)


# ---- the index chain --------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 2, 3, 5, 6, 7, 13, 14, 15, 29, 30, 31, 61, 62, 63, 1021, 1022, 1023, 1025])
def test_index_chain_rounds(gpu, lib, B):
    """B blocks of one entry each: the chain is marked in ceil(log2(B + 2)) doubling rounds, on both sides
    of every B at which another round is taken."""
    entries = [(b"k%05d" % i, b"v" * (i % 7)) for i in range(B)]
    file, blocks, _, _ = oracle_file(entries, 1)
    assert len(blocks) == B
    check_scan(gpu, file, B % 16)
    last = (ctypes.c_uint64 * 4)()
    lib.tkv_debug_sst_scan_last(last)
    assert last[0] == B and last[1] == math.ceil(math.log2(B + 2))


def test_index_out_of_file_order_with_gaps(gpu):
    file, expect = su.mutations()["out_of_order_with_gaps_ok"]
    want = su.oracle_scan(file)
    assert [b[0] for b in want[3]] != sorted(b[0] for b in want[3])
    for mis in range(16):
        check_scan(gpu, file, mis, want=want)


# ---- raw calls with canaried outputs ----------------------------------------------------------------------

class DevOutputs:
    """Canaried device outputs sized for n entries, nb blocks and ks / vs arena bytes, the arenas at byte
    misalignment ``mis`` with canaries on both sides."""

    def __init__(self, gpu, n, nb, ks, vs, mis=0):
        can = lambda nbytes: torch.full((nbytes,), CANARY, dtype=torch.uint8, device=gpu)  # noqa: E731
        self.key_off, self.val_off = can(8 * (n + 1)), can(8 * (n + 1))
        self.key_len, self.val_len = can(4 * (n + 1)), can(4 * (n + 1))
        self.block_off, self.block_size, self.block_first = can(8 * (nb + 1)), can(4 * (nb + 1)), can(4 * (nb + 1))
        self.kbuf, self.vbuf = can(32 + ks + 48), can(32 + vs + 48)
        self.kstart = 16 + (-(self.kbuf.data_ptr() + 16) % 16) + mis
        self.vstart = 16 + (-(self.vbuf.data_ptr() + 16) % 16) + (mis * 7 + 3) % 16
        self.caps = (n, nb, ks, vs)

    def all(self):
        return (self.key_off, self.key_len, self.val_off, self.val_len, self.block_off, self.block_size, self.block_first,
                self.kbuf, self.vbuf)

    def untouched(self):
        return all(bool((t == CANARY).all()) for t in self.all())


def raw_scan(lib, f, flags=0, out=None, caps=None, skip=()):
    res = [ctypes.c_uint64(0x5EED) for _ in range(5)]
    p = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + o)  # noqa: E731
    if out is None:
        args = [None, None, None, None, 0, None, 0, None, 0, None, None, None, 0]
    else:
        n, nb, ks, vs = out.caps if caps is None else caps
        args = [p(out.key_off), p(out.key_len), p(out.val_off), p(out.val_len), n, p(out.kbuf, out.kstart), ks,
                p(out.vbuf, out.vstart), vs, p(out.block_off), p(out.block_size), p(out.block_first), nb]
        for k in skip:
            args[k] = None
    rc = lib.tkv_sst_scan_device(ctypes.c_void_p(f.data_ptr()) if f.numel() else None, f.numel(), flags, *args,
                                 *[ctypes.byref(r) for r in res], None)
    torch.cuda.synchronize()
    return rc, tuple(r.value for r in res)


def read_outputs(out, n, nb, ks, vs):
    col = lambda t, dt, m: t.cpu().numpy().view(dt)[:m].tolist()  # noqa: E731
    return dict(key_off=col(out.key_off, np.uint64, n), key_len=col(out.key_len, np.uint32, n),
                val_off=col(out.val_off, np.uint64, n), val_len=col(out.val_len, np.uint32, n),
                block_off=col(out.block_off, np.uint64, nb), block_size=col(out.block_size, np.uint32, nb),
                block_first=col(out.block_first, np.uint32, nb),
                keys=out.kbuf.cpu().numpy()[out.kstart:out.kstart + ks].tobytes(),
                vals=out.vbuf.cpu().numpy()[out.vstart:out.vstart + vs].tobytes())


@pytest.fixture(scope="module")
def mixed_file():
    entries, target = fuzz_case(7)
    file = oracle_file(entries, target)[0]
    return file, su.oracle_scan(file)


def test_arena_destinations_at_every_misalignment(gpu, lib, mixed_file):
    file, (_, _, ents, blocks) = mixed_file
    f = dev_file(gpu, file, 5)
    n, nb = len(ents), len(blocks)
    ks, vs = sum(len(k) for k, _ in ents), sum(len(v) for _, v in ents)
    for mis in range(16):
        out = DevOutputs(gpu, n, nb, ks, vs, mis)
        rc, sizes = raw_scan(lib, f, 0, out)
        assert rc == OK and sizes == (n, nb, ks, vs, nb)
        got = read_outputs(out, n, nb, ks, vs)
        assert got["keys"] == b"".join(k for k, _ in ents) and got["vals"] == b"".join(v for _, v in ents)
        assert got["key_len"] == [len(k) for k, _ in ents] and got["val_len"] == [len(v) for _, v in ents]
        kb, vb = out.kbuf.cpu().numpy(), out.vbuf.cpu().numpy()
        assert (kb[:out.kstart] == CANARY).all() and (kb[out.kstart + ks:] == CANARY).all()
        assert (vb[:out.vstart] == CANARY).all() and (vb[out.vstart + vs:] == CANARY).all()
        for t, width, m in ((out.key_off, 8, n), (out.val_len, 4, n), (out.block_first, 4, nb), (out.block_off, 8, nb)):
            assert (t.cpu().numpy()[width * m:] == CANARY).all()


@pytest.mark.parametrize("flags", [su.KEY_VIEWS, su.VAL_VIEWS, su.KEY_VIEWS | su.VAL_VIEWS])
def test_views_against_copies(gpu, lib, mixed_file, flags):
    file, want = mixed_file
    check_scan(gpu, file, 9, key_views=bool(flags & su.KEY_VIEWS), val_views=bool(flags & su.VAL_VIEWS), want=want)
    # a views arena is not written and has no cap
    ents, blocks = want[2], want[3]
    n, nb = len(ents), len(blocks)
    ks, vs = sum(len(k) for k, _ in ents), sum(len(v) for _, v in ents)
    out = DevOutputs(gpu, n, nb, ks, vs)
    caps = (n, nb, 0 if flags & su.KEY_VIEWS else ks, 0 if flags & su.VAL_VIEWS else vs)
    rc, sizes = raw_scan(lib, dev_file(gpu, file, 2), flags, out, caps=caps)
    assert rc == OK and sizes == (n, nb, ks, vs, nb)
    if flags & su.KEY_VIEWS:
        assert bool((out.kbuf == CANARY).all())
    if flags & su.VAL_VIEWS:
        assert bool((out.vbuf == CANARY).all())


def test_nullable_arrays(gpu, lib, mixed_file):
    file, (_, _, ents, blocks) = mixed_file
    f = dev_file(gpu, file, 1)
    n, nb = len(ents), len(blocks)
    ks, vs = sum(len(k) for k, _ in ents), sum(len(v) for _, v in ents)
    full = DevOutputs(gpu, n, nb, ks, vs)
    assert raw_scan(lib, f, 0, full)[0] == OK
    want = read_outputs(full, n, nb, ks, vs)
    names = ("key_off", "key_len", "val_off", "val_len", None, "keys", None, "vals", None, "block_off", "block_size", "block_first")
    for skip in ((0, 2), (1, 3), (5,), (7,), (9, 10), (11,), (0, 1, 2, 3), (9, 10, 11), (0, 1, 2, 3, 5, 7)):
        out = DevOutputs(gpu, n, nb, ks, vs)
        rc, sizes = raw_scan(lib, f, 0, out, skip=skip)
        assert rc == OK and sizes == (n, nb, ks, vs, nb), skip
        got = read_outputs(out, n, nb, ks, vs)
        for k, name in enumerate(names):
            if name is None:
                continue
            if k in skip:
                t = {"keys": out.kbuf, "vals": out.vbuf}.get(name, getattr(out, name, None))
                assert bool((t == CANARY).all()), (skip, name)
            else:
                assert got[name] == want[name], (skip, name)


# ---- corrupted files --------------------------------------------------------------------------------------

MUT = su.mutations()


@pytest.mark.parametrize("name", sorted(MUT))
def test_every_catalogue_mutation(gpu, lib, name):
    file, expect = MUT[name]
    status, bad, ents, blocks = su.oracle_scan(file)
    if status == "ok":
        assert expect == "ok"
        check_scan(gpu, file, len(name) % 16)
        return
    assert bad == expect
    out = DevOutputs(gpu, 64, 8, 4096, 4096)
    for mis in (0, len(name) % 16):
        rc, sizes = raw_scan(lib, dev_file(gpu, file, mis), 0, out)
        assert rc == CORRUPTED and sizes == (0, 0, 0, 0, bad)
    assert out.untouched()


def test_two_bad_blocks_report_the_smaller(gpu, lib):
    blocks = [[(b"k%03d" % (3 * j + i), b"v" * j) for i in range(3)] for j in range(40)]
    file = bytearray(su.file_of_blocks(blocks))
    _, _, _, bl = su.oracle_scan(bytes(file))
    file[bl[31][0] + 30] ^= 1      # a checksum failure
    file[bl[17][0] + 1] ^= 2       # a structural one (c), its stamp then fails too
    file[bl[25][0] + 25] ^= 4
    assert su.oracle_scan(bytes(file))[:2] == ("corrupted", 17)
    rc, sizes = raw_scan(lib, dev_file(gpu, bytes(file), 7))
    assert rc == CORRUPTED and sizes == (0, 0, 0, 0, 17)


def test_every_single_bit_flip_of_a_small_file(gpu, lib):
    file = MUT["base"][0]
    assert 600 <= len(file) <= 800
    rng = np.random.default_rng(0xB17)
    bits = rng.integers(0, 8, len(file))
    out = DevOutputs(gpu, 16, 8, 1024, 1024)
    f = dev_file(gpu, file, 11)
    orig = f.clone()
    wrong = []
    for pos in range(len(file)):
        mutated = bytearray(file)
        mutated[pos] ^= 1 << int(bits[pos])
        status, bad, _, _ = su.oracle_scan(bytes(mutated))
        assert status == "corrupted"
        f[pos] = mutated[pos]
        rc, sizes = raw_scan(lib, f, 0, out)
        f[pos] = orig[pos]
        if rc != CORRUPTED or sizes != (0, 0, 0, 0, bad):
            wrong.append((pos, int(bits[pos]), rc, sizes, bad))
    assert not wrong, wrong[:10]
    assert out.untouched()


# ---- sizing, overflow, empty ------------------------------------------------------------------------------

def test_sizing_and_each_overflow_kind(gpu, lib, mixed_file):
    file, (_, _, ents, blocks) = mixed_file
    f = dev_file(gpu, file, 4)
    n, nb = len(ents), len(blocks)
    ks, vs = sum(len(k) for k, _ in ents), sum(len(v) for _, v in ents)
    rc, sizes = raw_scan(lib, f)
    assert rc == BUFFER_OVERFLOW and sizes == (n, nb, ks, vs, nb)
    for caps in ((n - 1, nb, ks, vs), (n, nb - 1, ks, vs), (n, nb, ks - 1, vs), (n, nb, ks, vs - 1)):
        out = DevOutputs(gpu, n, nb, ks, vs)
        rc, sizes = raw_scan(lib, f, 0, out, caps=caps)
        assert rc == BUFFER_OVERFLOW and sizes == (n, nb, ks, vs, nb), caps
        assert out.untouched(), caps


def test_empty_table(gpu, lib):
    for name in ("empty_table_ok", "empty_table_with_data_ok"):
        file = MUT[name][0]
        out = DevOutputs(gpu, 4, 4, 16, 16)
        rc, sizes = raw_scan(lib, dev_file(gpu, file, 3), 0, out)
        assert rc == OK and sizes == (0, 0, 0, 0, 0)
        assert out.untouched()
        res = sst.scan_device(dev_file(gpu, file))
        assert res.n_entries == 0 and res.n_blocks == 0 and res.entries() == []


def test_corrupted_file_raises_with_the_bad_block(gpu):
    for name, want in (("footer_crc", "footer"), ("index_trailing_byte", "index"), ("c_one_less", 2)):
        with pytest.raises(sst.SstCorrupted) as e:
            sst.scan_device(dev_file(gpu, MUT[name][0]))
        assert e.value.bad_block == want


# ---- pipeline, host variant, threads ----------------------------------------------------------------------

def test_wal_recover_flush_scan(gpu, oracle):
    rng = np.random.default_rng(32)
    img, offs, _ = fz.build(rng, oracle, "mixed", 3000)
    image = torch.from_numpy(img).to(gpu)
    status, b, stop, _ = wal.recover_device(image, key_views=True, val_views=True)
    assert status == "ok" and stop == img.size
    raw = img.tobytes()
    entries = []
    for o in offs.astype(np.int64).tolist():
        kl, vl = int.from_bytes(raw[o + 18:o + 22], "little"), int.from_bytes(raw[o + 22:o + 26], "little")
        entries.append((raw[o + 26:o + 26 + kl], raw[o + 26 + kl:o + 26 + kl + vl]))
    built = sst.build_device(b.keys, b.key_off, b.key_len, b.vals, b.val_off, b.val_len, target_block_size=4096)
    res = sst.scan_device(built.file)
    assert res.entries() == entries
    assert res.block_off.tolist() == built.block_off.tolist() and u32(res.block_first) == u32(built.block_first)


@pytest.mark.parametrize("name", ["edge:uniform", "edge:one_larger_than_T", "fuzz:3", "fuzz:10", "mut:out_of_order_with_gaps_ok"])
def test_host_variant(gpu, name):
    kind, key = name.split(":")
    if kind == "mut":
        file = MUT[key][0]
    else:
        entries, target = edge_cases()[key] if kind == "edge" else fuzz_case(int(key))
        file = oracle_file(entries, target)[0]
    _, _, ents, blocks = su.oracle_scan(file)
    for kv, vv in ((False, False), (True, True)):
        res = sst.scan(file, key_views=kv, val_views=vv)
        assert res.entries() == ents
        assert [list(x) for x in zip(res.block_off.tolist(), res.block_size.tolist(), res.block_first.tolist())] == \
            [list(b) for b in blocks]


def test_host_variant_verdicts(gpu):
    for name in ("footer_crc", "block_crc", "two_bad_blocks", "index_key_one_byte", "B_one_less"):
        file, expect = MUT[name]
        with pytest.raises(sst.SstCorrupted) as e:
            sst.scan(file)
        assert e.value.bad_block == {su.BAD_FOOTER: "footer", su.BAD_INDEX: "index"}.get(expect, expect)


def test_four_threads_scan_at_once(gpu):
    work = []
    for t in range(4):
        entries, target = fuzz_case(20 + t)
        file = oracle_file(entries, target)[0]
        work.append((file, su.oracle_scan(file)))
    barrier = threading.Barrier(4)
    failures, passes = [], []

    def run(t):
        try:
            file, want = work[t]
            stream = torch.cuda.Stream(gpu)
            with torch.cuda.stream(stream):
                f = dev_file(gpu, file, 3 * t)
                stream.synchronize()
                barrier.wait(60)
                for rnd in range(3):
                    res = sst.scan_device(f, key_views=bool(rnd & 1), stream=stream)
                    assert res.entries() == want[2]
                    assert u32(res.block_first) == [b[2] for b in want[3]]
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
