"""tkv_wal_encode_device / tkv_wal_encode on the GPU: every image is compared byte for byte with a numpy
restatement of wal.cpp:19-61 whose CRCs come from the test oracle (never from the library under test),
with 64-byte sentinels in front of and behind every destination."""
import ctypes

import numpy as np
import pytest

import tinykvpp_amd as tk
from conftest import golden
from tinykvpp_amd._lib import BUFFER_OVERFLOW, INVALID_ARGUMENT, OK
from wal_encode_util import (DeviceBatch, encode_host, expected, geometry, golden_batch, last, make_batch)

pytestmark = pytest.mark.gpu


def small_batch(rng, n, kmin=0):
    """Keys kmin-23 B, values 0-64 B, with the 26-byte record and records with one side empty."""
    klen, vlen = rng.integers(kmin, 24, n), rng.integers(0, 65, n)
    if kmin == 0:
        klen[:3], vlen[:3] = (0, 0, 5), (0, 7, 0)
    return make_batch(rng, klen, vlen)


def long_batch(rng, tile):
    """record_len 241, 4096, 2 tile + 5, 65537 and 1 MiB + 3 as long key, long value and both long, each
    between short records."""
    klen, vlen = [], []
    for rl in (241, 4096, 2 * tile + 5, 65537, (1 << 20) + 3):
        body = rl - 18
        for k, v in ((body, 0), (0, body), (body // 3, body - body // 3)):
            klen += [int(rng.integers(0, 24)), k, int(rng.integers(0, 24))]
            vlen += [int(rng.integers(0, 65)), v, int(rng.integers(0, 65))]
    return make_batch(rng, klen, vlen)


def check(lib, db, want, offs, crc, align=0, fused_all=False):
    rc, size, img, guard, goff, gcrc = db.encode(lib, want.size, align=align)
    assert rc == OK and size == want.size
    assert guard, "bytes outside the destination were written"
    bad = np.flatnonzero(img != want)
    assert bad.size == 0, f"image differs at {bad[:8]} (first record {np.searchsorted(offs, bad[0], 'right') - 1})"
    assert np.array_equal(goff, offs)
    assert np.array_equal(gcrc, crc)
    st = last(lib)
    assert st[0] + st[1] == db.b["n"] and st[3] == want.size
    if fused_all:
        assert st[1] == 0 and st[0] == db.b["n"]
    return img


@pytest.fixture(scope="module")
def small_case(gpu, oracle):
    b = small_batch(np.random.default_rng(901), 1000)
    return DeviceBatch(b, gpu), expected(b, oracle)


@pytest.fixture(scope="module")
def long_case(gpu, oracle, lib):
    b = long_batch(np.random.default_rng(902), geometry(lib)[0])
    return DeviceBatch(b, gpu), expected(b, oracle)


def test_golden_records(gpu, lib, oracle):
    recs = golden("wal.json")["records"]
    b, raw = golden_batch(recs)
    want = np.frombuffer(b"".join(raw), np.uint8)
    offs = np.cumsum([0] + [len(r) for r in raw[:-1]]).astype(np.uint64)
    crc = np.array([r["crc"] for r in recs], np.uint32)
    check(lib, DeviceBatch(b, gpu), want, offs, crc, align=5, fused_all=True)
    rc, size, img, guard, goff, gcrc = encode_host(lib, b, align=5)
    assert rc == OK and size == want.size and guard
    assert img.tobytes() == want.tobytes()
    assert np.array_equal(goff, offs) and np.array_equal(gcrc, crc)


@pytest.mark.parametrize("align", [0, 1, 7, 13])
def test_random_small_batch(lib, small_case, align):
    db, (want, offs, crc) = small_case
    check(lib, db, want, offs, crc, align=align, fused_all=True)


def test_defaults(gpu, lib, oracle):
    rng = np.random.default_rng(903)
    b = small_batch(rng, 300)
    for d in (dict(b, op=None, tomb=None, seq=None, first_seq=1 << 40),
              dict(b, val_len=None),
              dict(b, key_off=np.full(300, b["key_off"][7], np.uint64), key_len=np.full(300, 11, np.uint32))):
        want, offs, crc = expected(d, oracle)
        check(lib, DeviceBatch(d, gpu), want, offs, crc, align=3, fused_all=True)


def test_tile_edges(gpu, lib, oracle):
    """Every header byte, the CRC field and the first payload bytes of a record across a tile edge.
    One first record that puts the second at T - d is itself longer than a tile, so it is stamped by the
    read-back route (the encoder carries no CRC across tiles): there the emit pass must stamp all the
    others (out[0] == n - 1, out[1] == 1). The same edge offsets are then run with a lead-in of short
    records in place of the one long one, where the emit pass must stamp everything (out[1] == 0,
    out[0] == n)."""
    T = geometry(lib)[0]
    rng = np.random.default_rng(904)
    cases = []
    for d in range(34):  # the second record starts at T - d
        first = T - d - 26
        cases.append(([first // 2, 9, 200, 4], [first - first // 2, 20, 22, 3]))  # then record_len 240 and a short one
    cases.append(([T - 26 - 100, 5, 3], [100, 6, 0]))           # a record ends exactly at T
    cases.append(([T - 1 - 26 - 7, 100, 2], [7, 122, 9]))       # record_len 240 starts at T - 1
    for klen, vlen in cases:
        b = make_batch(rng, klen, vlen)
        want, offs, crc = expected(b, oracle)
        assert T < want.size <= 3 * T
        rc, size, img, guard, goff, gcrc = DeviceBatch(b, gpu).encode(lib, want.size, align=9)
        assert rc == OK and guard and np.array_equal(img, want), (klen, vlen)
        assert np.array_equal(goff, offs) and np.array_equal(gcrc, crc)
        assert last(lib)[:2] == [b["n"] - 1, 1]
    m = (T - 100) // 246          # records of 246 bytes in front of the edge, behind a lead-in of s0 bytes
    for d in list(range(34)) + [-1]:  # the record after them starts at T - d (d = -1: record_len 240 at T + 1 ...)
        s0 = T - d - 246 * m
        lead = [s0] if s0 <= 248 else [100, s0 - 100]
        klen = [5] * len(lead) + [20] * m + [9, 100, 4]
        vlen = [s - 26 - 5 for s in lead] + [200] * m + [20, 122, 3]  # ... record_len 240 and a short one behind
        fill = (2 * T + 40 - (T - d + 55 + 248 + 33)) // 246 + 1      # and on into a third tile
        klen += [20] * fill + [7]
        vlen += [200] * fill + [0]
        b = make_batch(rng, klen, vlen)
        want, offs, crc = expected(b, oracle)
        assert int(offs[len(lead) + m]) == T - d and 2 * T < want.size <= 3 * T
        check(lib, DeviceBatch(b, gpu), want, offs, crc, align=d % 16, fused_all=True)
    # a record that ends exactly at T, and a record_len 240 record that starts at T - 1, among short ones
    for cut, nxt in ((T, (9, 20)), (T - 1, (100, 122))):
        s0 = cut - 246 * m
        lead = [s0] if s0 <= 248 else [100, s0 - 100]
        b = make_batch(rng, [5] * len(lead) + [20] * m + [nxt[0], 3], [s - 31 for s in lead] + [200] * m + [nxt[1], 0])
        want, offs, crc = expected(b, oracle)
        assert int(offs[len(lead) + m]) == cut
        check(lib, DeviceBatch(b, gpu), want, offs, crc, align=1, fused_all=True)


def test_long_records(lib, long_case):
    db, (want, offs, crc) = long_case
    check(lib, db, want, offs, crc, align=11)
    assert last(lib)[1] == 15


def test_scan_levels(gpu, lib, oracle):
    _, B, _, levels = geometry(lib)
    ns = [B - 1, B, B + 1] + [B ** k + 1 for k in range(2, levels) if B ** k <= 1 << 22]
    rng = np.random.default_rng(905)
    for n in ns:
        klen, vlen = np.zeros(n, np.int64), np.zeros(n, np.int64)
        some = rng.integers(0, n, 64)
        klen[some], vlen[some] = rng.integers(0, 24, 64), rng.integers(1, 42, 64)
        b = make_batch(rng, klen, vlen, plain=True)
        want, offs, crc = expected(b, oracle)
        assert want.size < 64 << 20
        check(lib, DeviceBatch(b, gpu), want, offs, crc, align=2, fused_all=True)


def test_route_switch(lib, small_case, long_case):
    for db, (want, offs, crc) in (small_case, long_case):
        fused = check(lib, db, want, offs, crc, align=6)
        prev = lib.tkv_debug_set_wal_encode_fused(0)
        try:
            unfused = check(lib, db, want, offs, crc, align=6)
            assert last(lib)[:2] == [0, db.b["n"]]
        finally:
            lib.tkv_debug_set_wal_encode_fused(prev)
        assert np.array_equal(fused, unfused)


def test_overflow_and_invalid(gpu, lib, small_case):
    db, (want, offs, crc) = small_case
    rc, size, img, guard, goff, gcrc = db.encode(lib, want.size, cap=want.size - 1)
    assert rc == BUFFER_OVERFLOW and size == want.size
    assert guard and (img == 0xA5).all() and (goff == 0xA5A5A5A5A5A5A5A5).all() and (gcrc == 0xA5A5A5A5).all()
    assert last(lib) == [0, 0, 0, 0]
    assert db.encode(lib, want.size, cap=want.size)[0] == OK
    b = dict(db.b)
    b["key_len"], b["val_len"] = b["key_len"].copy(), b["val_len"].copy()
    b["key_len"][500], b["val_len"][500] = 0xFFFFFFF0, 0x100
    rc, size, img, guard, goff, gcrc = DeviceBatch(b, gpu).encode(lib, want.size)
    assert rc == INVALID_ARGUMENT
    assert guard and (img == 0xA5).all() and (goff == 0xA5A5A5A5A5A5A5A5).all() and (gcrc == 0xA5A5A5A5).all()


def test_round_trip_through_the_read_side(gpu, lib, oracle):
    import torch
    rng = np.random.default_rng(906)
    small = small_batch(rng, 20000)
    zv = np.minimum(rng.zipf(1.6, 2000) * 64, 16000)
    zv[-1] = 30  # the image ends with a short record
    zipf = make_batch(rng, rng.integers(4, 24, 2000), zv)
    for b in (small, zipf):
        n = b["n"]
        db = DeviceBatch(b, gpu)
        image, rec_off, crc = tk.wal.encode_device(db.t["keys"], db.t["key_off"], db.t["key_len"], db.t["vals"],
                                                   db.t["val_off"], db.t["val_len"], db.t["op"], db.t["tomb"], db.t["seq"])
        total = image.numel()
        want, want_off, want_crc = expected(b, oracle)
        assert total < 20 << 20 and total == int(want.size)
        bad = np.flatnonzero(image.cpu().numpy() != want)
        assert bad.size == 0, f"image differs at {bad[:8]} (first record {np.searchsorted(want_off, bad[0], 'right') - 1})"
        assert np.array_equal(rec_off.cpu().numpy().view(np.uint64), want_off)
        assert np.array_equal(crc.cpu().numpy().view(np.uint32), want_crc)
        assert tk.wal.verify_device(image) == ("ok", n, total)
        status, offs, stop, mseq = tk.wal.index_device(image, offsets32=True)
        assert (status, stop, mseq) == ("ok", total, int(b["seq"].max()))
        assert torch.equal(offs.to(torch.int64), rec_off)
        first_bad, got = tk.wal.check_records_device(image, offs, max_payload=64)
        assert int(first_bad.item()) == n
        assert torch.equal(got, crc)


def test_side_stream(gpu, lib, small_case):
    import torch
    db, (want, offs, crc) = small_case
    st = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(st):
        t = {k: (None if v is None else v.clone()) for k, v in db.t.items()}  # the inputs produced on the stream
        image, rec_off, got = tk.wal.encode_device(t["keys"], t["key_off"], t["key_len"], t["vals"], t["val_off"],
                                                   t["val_len"], t["op"], t["tomb"], t["seq"], stream=st)
    st.synchronize()
    assert np.array_equal(image.cpu().numpy(), want)
    assert np.array_equal(rec_off.cpu().numpy().view(np.uint64), offs)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), crc)
    small = torch.empty(want.size - 1, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError, match=str(want.size)):
        tk.wal.encode_device(db.t["keys"], db.t["key_off"], db.t["key_len"], db.t["vals"], db.t["val_off"],
                             db.t["val_len"], out=small)


def list_batch(keys, vals, ops=None, tombs=None, seqs=None, first_seq=0):
    """Lists of bytes as a batch of arrays (the arenas back to back), for expected()."""
    klen, vlen = np.array([len(k) for k in keys], np.uint32), np.array([len(v) for v in vals], np.uint32)
    arr = lambda x, dt: None if x is None else np.array(x, dt)  # noqa: E731
    return dict(n=len(keys), keys=np.frombuffer(b"".join(keys) + b"\0", np.uint8),
                key_off=(np.cumsum(klen, dtype=np.uint64) - klen), key_len=klen,
                vals=np.frombuffer(b"".join(vals) + b"\0", np.uint8),
                val_off=(np.cumsum(vlen, dtype=np.uint64) - vlen), val_len=vlen,
                op=arr(ops, np.uint8), tomb=arr(tombs, np.uint8), seq=arr(seqs, np.uint64), first_seq=first_seq)


def test_python_host_path(gpu, lib, oracle):
    recs = golden("wal.json")["records"]
    raw = [bytes.fromhex(r["hex"]) for r in recs]
    keys = [x[26:26 + int.from_bytes(x[18:22], "little")] for x in raw]
    vals = [x[26 + len(k):] for x, k in zip(raw, keys)]
    image, offs = tk.wal.encode_batch(keys, vals, seqs=[r["seq"] for r in recs], ops=[r["op"] for r in recs],
                                      tombstones=[r["tombstone"] for r in recs])
    assert image == b"".join(raw)
    assert offs.tolist() == np.cumsum([0] + [len(r) for r in raw[:-1]]).tolist()
    rng = np.random.default_rng(907)
    n = 500
    keys = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(0, 24, n)]
    vals = [rng.integers(0, 256, int(v), dtype=np.uint8).tobytes() for v in rng.integers(0, 400, n)]
    ops, tombs = rng.integers(0, 2, n).tolist(), rng.integers(0, 2, n).tolist()
    seqs = rng.integers(0, 1 << 62, n).tolist()
    want = b"".join(tk.wal.stamp([tk.wal.encode_unstamped(o, s, k, v, t)
                                  for o, s, k, v, t in zip(ops, seqs, keys, vals, tombs)]))
    image, offs = tk.wal.encode_batch(keys, vals, seqs=seqs, ops=ops, tombstones=tombs)
    assert image == want
    exp, exp_off, _ = expected(list_batch(keys, vals, ops, tombs, seqs), oracle)
    assert image == exp.tobytes() and np.array_equal(offs, exp_off)
    want = b"".join(tk.wal.stamp([tk.wal.encode_unstamped(0, 77 + i, k, v, 0) for i, (k, v) in enumerate(zip(keys, vals))]))
    image, offs = tk.wal.encode_batch(keys, vals, first_seq=77)
    assert image == want
    exp, exp_off, _ = expected(list_batch(keys, vals, first_seq=77), oracle)
    assert image == exp.tobytes() and np.array_equal(offs, exp_off)


def test_host_entry_on_host_threads(gpu, lib, oracle):
    """tkv_wal_encode at 50 000 records: the layout and the CRC fields are written on host threads
    (n >= 1 << 14); image, rec_off and crc against the numpy encode."""
    rng = np.random.default_rng(908)
    b = small_batch(rng, 50_000)
    want, offs, crc = expected(b, oracle)
    rc, size, img, guard, goff, gcrc = encode_host(lib, b, align=7)
    assert rc == OK and size == want.size and guard
    bad = np.flatnonzero(img != want)
    assert bad.size == 0, f"image differs at {bad[:8]} (first record {np.searchsorted(offs, bad[0], 'right') - 1})"
    assert np.array_equal(goff, offs) and np.array_equal(gcrc, crc)
