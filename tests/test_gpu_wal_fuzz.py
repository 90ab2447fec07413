"""The device WAL pipeline end to end on random mutated images (wal_fuzz_util.case): verify and index,
then the record check and the decode on the lists the index wrote (they stay on the device), the encode
of the decoded batch back to the image, and the recovery wrappers; and the same pipeline from four host
threads at once. Every expected value comes from the helper's sequential decode and the numpy
restatements (test_wal_fuzz_cpu.py checks that decode against the C oracle for the same seeds); the one
comparison with the input itself is the closed loop, whose target is image[:stop]."""
import ctypes
import threading

import numpy as np
import pytest
import torch

import tinykvpp_amd as tk
import wal_fuzz_util as fz
from test_gpu_wal_index import SENT32, SENT64, index_raw
from tinykvpp_amd._lib import CORRUPTED, OK
from wal_decode_util import COLS, FLAGS, KEY_VIEWS, VAL_VIEWS, DevOut, check_device, decode_device, expected, first_bad
from wal_decode_util import last as decode_last
from wal_encode_util import SENT, U64
from wal_encode_util import last as encode_last

pytestmark = pytest.mark.gpu

MAX_PAYLOAD = (36, 64, 100, 1024)


def upload(gpu, c):
    """The case's buffer on the device; the image is the view at its shift."""
    return torch.from_numpy(c.buf).to(gpu)[c.shift:]


def index_and_check(c, image, cap):
    """tkv_wal_index_device, both widths at once, against the case: the verdict, the offsets, the
    untouched tail and max_sequence. Returns the two device buffers."""
    got, o64, o32, seq, bufs = index_raw(image, c.size, cap, tensors=True)
    assert got == c.verdict, (got, c.verdict)
    k = min(c.n_good, cap)
    assert np.array_equal(o64[:k].view(np.uint64), c.starts[:k])
    assert np.array_equal(o32[:k].view(np.uint32), c.starts[:k].astype(np.uint32))
    assert (o64[k:] == SENT64).all() and (o32[k:] == SENT32).all(), "an entry at or past min(n_good, cap) was written"
    assert seq == c.max_seq
    return bufs


def check_records(oracle, c, image, dlist, starts, max_payload, stream=None):
    """tkv_wal_check_records_device on a device list that holds `starts`: first_bad and every CRC."""
    want_crc, ok = fz.records_expected(oracle, c.img, c.size, starts)
    bad = np.flatnonzero(~ok)
    fb, crc = tk.wal.check_records_device(image, dlist, max_payload=max_payload, stream=stream)
    (torch.cuda.current_stream() if stream is None else stream).synchronize()
    assert int(fb.item()) == (int(bad[0]) if bad.size else len(starts)), (int(fb.item()), bad[:4], max_payload)
    diff = np.flatnonzero(crc.cpu().numpy().view(np.uint32) != want_crc)
    assert diff.size == 0, f"{diff.size} CRCs differ, first {diff[:5]} (max_payload {max_payload})"


def encode_decoded(lib, gpu, out, image, flags, n, total, align, stream=None):
    """tkv_wal_encode_device of a decoded batch (out: the DevOut of a decode with `flags`; a views arena
    is the image) into a guarded buffer: (rc, img_size, image bytes, guards intact, rec_off, crc)."""
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    keys = image.data_ptr() if flags & KEY_VIEWS else out.kbuf.data_ptr() + out.kstart
    vals = image.data_ptr() if flags & VAL_VIEWS else out.vbuf.data_ptr() + out.vstart
    buf = torch.full((SENT + 32 + total + SENT,), 0xA5, dtype=torch.uint8, device=gpu)
    start = SENT + (align - (buf.data_ptr() + SENT)) % 16
    off = torch.full((n,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=gpu)
    crc = torch.full((n,), -0x5A5A5A5B, dtype=torch.int32, device=gpu)
    torch.cuda.synchronize()
    size = U64(0)
    c = out.c
    rc = lib.tkv_wal_encode_device(ctypes.c_void_p(keys), p(c["key_off"]), p(c["key_len"]), ctypes.c_void_p(vals),
                                   p(c["val_off"]), p(c["val_len"]), p(c["op"]), p(c["tomb"]), p(c["seq"]), 0, n,
                                   ctypes.c_void_p(buf.data_ptr() + start), total, p(off), p(crc), ctypes.byref(size), stream)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    guards = bool((h[:start] == 0xA5).all() and (h[start + total:] == 0xA5).all())
    return rc, size.value, h[start:start + total], guards, off.cpu().numpy().view(np.uint64), crc.cpu().numpy().view(np.uint32)


def closed_loop(lib, gpu, c, image, out, flags, align, stream=None):
    """The decoded good prefix encoded again reproduces image[:stop] byte for byte between sentinels, its
    offsets the good starts, its CRCs the stored fields."""
    rc, size, img, guards, off, crc = encode_decoded(lib, gpu, out, image, flags, c.n_good, c.stop, align, stream)
    assert (rc, size) == (OK, c.stop), (rc, size, c.stop)
    assert guards, "bytes outside the destination were written"
    bad = np.flatnonzero(img != c.img[:c.stop])
    assert bad.size == 0, f"image differs at {bad[:8]} (first record {np.searchsorted(c.starts, bad[0], 'right') - 1})"
    stored = c.img[c.starts.astype(np.int64)[:, None] + 4 + np.arange(4)].copy().view("<u4").reshape(-1)
    assert np.array_equal(off, c.starts) and np.array_equal(crc, stored)
    if c.n_good:  # (a call without records returns before it records anything)
        st = encode_last(lib)
        assert st[0] + st[1] == c.n_good and st[3] == c.stop, st


def same_batch(batch, want, to_numpy):
    for k in COLS + ("keys", "vals"):
        got = to_numpy(getattr(batch, k))
        assert np.array_equal(got.view(want[k].dtype), want[k]), k


@pytest.mark.parametrize("seed", fz.SEEDS)
def test_pipeline(gpu, lib, oracle, seed):
    c = fz.case(seed, oracle)
    rng = np.random.default_rng(515_000 + seed)
    image = upload(gpu, c)
    n = c.n_good
    # 1. verify and index
    assert tk.wal.verify_device(image, c.size) == c.verdict
    if seed % 4 == 3 and n:
        index_and_check(c, image, int(rng.integers(0, n)))  # a cap below the good prefix
    o64, o32 = index_and_check(c, image, c.size // fz.META)
    # 2. the record check on the u32 list the index wrote, and on the structural chain past `stop`
    check_records(oracle, c, image, o32[:n], c.starts, int(rng.choice(MAX_PAYLOAD)))
    if c.chain_goes_on or c.chain_broke:  # (a chain that broke: one more start, whose length check fails)
        full = np.append(c.chain, np.uint64(c.chain_end)) if c.chain_broke else c.chain
        dfull = torch.from_numpy(full.astype(np.uint32).view(np.int32)).to(gpu)
        check_records(oracle, c, image, dfull, full, int(rng.choice(MAX_PAYLOAD)))
    # 3. decode on the list the index wrote: a random flag combination, and what the closed loop needs
    outs = {}
    for flags in dict.fromkeys([int(rng.choice(FLAGS)), 0, KEY_VIEWS | VAL_VIEWS]):
        u32 = bool(rng.integers(0, 2))
        dlist = (o32 if u32 else o64)[:n]
        ka, va = int(rng.integers(0, 16)), int(rng.integers(0, 16))
        if n:
            outs[flags], _ = check_device(lib, gpu, image, c.img, c.starts, flags, kalign=ka, valign=va, doffs=dlist)
        else:
            outs[flags] = DevOut(gpu, 0, 16, 16, ka, va)
            assert decode_device(lib, image, dlist, flags, outs[flags]) == (OK, 0, 0, 0) and outs[flags].untouched()
    if c.kind == "val_len_restamped":  # the full chain: the victim passes the record check's CRC and fails here
        assert first_bad(c.img, c.chain, c.size) == n < c.chain.size
        out = DevOut(gpu, c.chain.size, 1 << 16, 1 << 16, 5, 11)
        dfull = torch.from_numpy(c.chain.view(np.int64)).to(gpu)
        assert decode_device(lib, image, dfull, 0, out) == (CORRUPTED, 0, 0, n)
        assert out.untouched() and decode_last(lib) == [0, 0, 0, 0]
    # 4. the closed loop, where the good prefix is what the reference encoder writes
    if c.ref_shape:
        for flags in (0, KEY_VIEWS | VAL_VIEWS):
            closed_loop(lib, gpu, c, image, outs[flags], flags, int(rng.integers(0, 16)))
    # 5. the recovery wrappers
    status, batch, stop, mseq = tk.wal.recover_device(image)
    assert (status, batch.op.numel(), stop, mseq) == (c.status, n, c.stop, c.max_seq)
    same_batch(batch, c.want, lambda t: t.cpu().numpy())
    status, vb, stop, mseq = tk.wal.recover_device(image, key_views=True, val_views=True)
    assert (status, stop, mseq) == (c.status, c.stop, c.max_seq) and vb.keys is image and vb.vals is image
    views = expected(c.img, c.starts, KEY_VIEWS | VAL_VIEWS)
    for k in COLS:
        assert np.array_equal(getattr(vb, k).cpu().numpy().view(views[k].dtype), views[k]), k
    status, hb, stop, mseq = tk.wal.recover(c.img)
    assert (status, hb.op.size, stop, mseq) == (c.status, n, c.stop, c.max_seq)
    same_batch(hb, c.want, lambda a: a)


# ---- concurrent callers --------------------------------------------------------------------------------------

THREADS, ROUNDS = 4, 6


def thread_cases(oracle, t):
    """A thread's own three cases: clean with at least 16 384 records, corrupted, values made of records."""
    clean = fz.case(9000 + 3 * t, oracle, profile=("tiny", "empties", "lane_wave", "tiny")[t], count=20_000, kind=0)
    bad = fz.case(9100 + 16 * (t + 2) + t, oracle, profile=("mixed", "tiny", "fold_edge", "lane_wave")[t], count=5000,
                  kind=(1, 2, 3, 4)[t])
    decoys = fz.case(9300 + 3 * t, oracle, profile="decoys", count=300, kind=0)
    assert clean.verdict == ("ok", 20_000, clean.size) and clean.n_good >= fz.HOST_THREADS_MIN
    assert bad.status == "corrupted" and 0 < bad.n_good < bad.count
    assert decoys.verdict == ("ok", 300, decoys.size)
    return clean, bad, decoys


def test_concurrent_callers(gpu, lib, oracle):
    """Four host threads, each on its own stream with its own images, run index -> record check -> decode
    -> encode six times over, released together: the per-device scratch, the pinned result block and
    the first_bad word are shared under the library's mutex, the `last call` words are thread-local, so
    every thread must see only its own results."""
    work = []
    for t in range(THREADS):
        cs = thread_cases(oracle, t)
        work.append([(c, expected(c.img, c.starts, 0)) for c in cs])
    barrier = threading.Barrier(THREADS)
    failures, passes = [], []

    def run(t):
        try:
            stream = torch.cuda.Stream(gpu)
            with torch.cuda.stream(stream):
                images = [upload(gpu, c) for c, _ in work[t]]
                stream.synchronize()
                barrier.wait(60)
                for rnd in range(ROUNDS):
                    for (c, want), image in zip(work[t], images):
                        o64, o32 = index_and_check(c, image, c.size // fz.META)
                        check_records(oracle, c, image, o32[:c.n_good], c.starts, MAX_PAYLOAD[(rnd + t) % 4], stream)
                        out, _ = check_device(lib, gpu, image, c.img, c.starts, 0, kalign=(t + rnd) % 16, valign=(3 * t + rnd) % 16,
                                              doffs=(o32 if rnd % 2 else o64)[:c.n_good], stream=stream.cuda_stream, want=want)
                        # (check_device read tkv_debug_wal_decode_last right after its call: this thread's totals)
                        if c.ref_shape:
                            closed_loop(lib, gpu, c, image, out, 0, (5 * t + rnd) % 16, stream.cuda_stream)
                        passes.append((t, rnd, c.seed))
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            failures.append((t, repr(e)))
            barrier.abort()

    threads = [threading.Thread(target=run, args=(t,), daemon=True) for t in range(THREADS)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(120)
    assert not any(th.is_alive() for th in threads), "a caller is still running after 120 s"
    assert not failures, failures
    assert len(passes) == THREADS * ROUNDS * 3 and all(c.ref_shape for cs in work for c, _ in cs)
