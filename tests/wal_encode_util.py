"""Helpers of the WAL encode tests: batches as arenas at arbitrary offsets, the expected image restated
in numpy (wal.cpp:19-61 layout, CRCs from the test oracle), and the C calls."""
import ctypes

import numpy as np

U64 = ctypes.c_uint64
SENT = 64  # sentinel bytes in front of and behind every destination


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def arena(rng, lens, gaps=True):
    """(arena, offsets): spans of `lens` bytes of random data at odd offsets, with gaps of 0-6 bytes."""
    lens = np.asarray(lens, np.uint64)
    gap = rng.integers(0, 7, lens.size).astype(np.uint64) if gaps else np.zeros(lens.size, np.uint64)
    step = lens + gap
    off = np.zeros(lens.size, np.uint64)
    off[1:] = np.cumsum(step[:-1])
    off += np.uint64(1 if gaps else 0)
    data = rng.integers(0, 256, int(step.sum()) + 17, dtype=np.uint8)
    return data, off


def make_batch(rng, klen, vlen, plain=False):
    """A batch with random op / tombstone (0, 1, 0x80) / seq; plain: the defaults (NULL arrays) instead."""
    klen, vlen = np.asarray(klen, np.uint32), np.asarray(vlen, np.uint32)
    n = klen.size
    keys, koff = arena(rng, klen)
    vals, voff = arena(rng, vlen)
    b = dict(n=n, keys=keys, key_off=koff, key_len=klen, vals=vals, val_off=voff, val_len=vlen, op=None, tomb=None,
             seq=None, first_seq=0)
    if not plain:
        b["op"] = rng.integers(0, 256, n, dtype=np.uint8)
        b["tomb"] = rng.choice(np.array([0, 1, 0x80], np.uint8), n)
        b["seq"] = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    return b


def _spread(lens):
    """For spans of `lens` bytes laid back to back: (span of byte j, j's index inside its span)."""
    lens = lens.astype(np.int64)
    starts = np.cumsum(lens) - lens
    which = np.repeat(np.arange(lens.size), lens)
    return which, np.arange(int(lens.sum())) - starts[which]


def expected(b, oracle=None):
    """(image, offsets, crc) of batch b; without an oracle the CRC fields stay zero (crc = None)."""
    n = b["n"]
    klen = b["key_len"].astype(np.uint64)
    vlen = b["val_len"].astype(np.uint64) if b["val_len"] is not None else np.zeros(n, np.uint64)
    size = 26 + klen + vlen
    offs = np.zeros(n, np.uint64)
    offs[1:] = np.cumsum(size[:-1])
    img = np.zeros(int(size.sum()), np.uint8)
    hdr = np.zeros((n, 26), np.uint8)
    hdr[:, 0:4] = (size - 8).astype("<u4").view(np.uint8).reshape(-1, 4)
    if b["op"] is not None:
        hdr[:, 8] = b["op"]
    seq = b["seq"] if b["seq"] is not None else (np.uint64(b["first_seq"]) + np.arange(n, dtype=np.uint64))
    hdr[:, 9:17] = seq.astype("<u8").view(np.uint8).reshape(-1, 8)
    if b["tomb"] is not None:
        hdr[:, 17] = b["tomb"] != 0
    hdr[:, 18:22] = klen.astype("<u4").view(np.uint8).reshape(-1, 4)
    hdr[:, 22:26] = vlen.astype("<u4").view(np.uint8).reshape(-1, 4)
    o = offs.astype(np.int64)
    img[o[:, None] + np.arange(26)] = hdr
    w, j = _spread(klen)
    img[o[w] + 26 + j] = b["keys"][b["key_off"].astype(np.int64)[w] + j]
    if b["val_len"] is not None:
        w, j = _spread(vlen)
        img[o[w] + 26 + klen.astype(np.int64)[w] + j] = b["vals"][b["val_off"].astype(np.int64)[w] + j]
    if oracle is None:
        return img, offs, None
    crc = oracle.batch(img, offs + 8, (size - 8).astype(np.uint32))
    img[o[:, None] + 4 + np.arange(4)] = crc.astype("<u4").view(np.uint8).reshape(-1, 4)
    return img, offs, crc


def host_args(b):
    return [_ptr(b["keys"]), _ptr(b["key_off"]), _ptr(b["key_len"]), _ptr(b["vals"]), _ptr(b["val_off"]),
            _ptr(b["val_len"]), _ptr(b["op"]), _ptr(b["tomb"]), _ptr(b["seq"]), int(b["first_seq"]), int(b["n"])]


def guarded(total, align=0):
    """(buffer, start): a host buffer of 0xA5 bytes whose byte `start` lies `align` bytes past a 16-byte
    boundary, with at least SENT bytes on either side of [start, start + total)."""
    buf = np.full(SENT + 32 + total + SENT, 0xA5, np.uint8)
    start = SENT + (align - (buf.ctypes.data + SENT)) % 16
    return buf, start


def sentinels_ok(buf, start, total):
    return bool((buf[start - SENT:start] == 0xA5).all() and (buf[start + total:start + total + SENT] == 0xA5).all())


def encode_host(lib, b, cap=None, align=0, total=None):
    """tkv_wal_encode into a guarded host buffer: (rc, img_size, image, sentinels intact, rec_off, crc)."""
    total = int(expected(b)[0].size) if total is None else total
    cap = total if cap is None else cap
    buf, start = guarded(total, align)
    off, crc = np.full(b["n"], 0xA5A5A5A5A5A5A5A5, np.uint64), np.full(b["n"], 0xA5A5A5A5, np.uint32)
    size = U64(0)
    rc = lib.tkv_wal_encode(*host_args(b), ctypes.c_void_p(buf.ctypes.data + start), cap, _ptr(off), _ptr(crc),
                            ctypes.byref(size))
    return rc, size.value, buf[start:start + total].copy(), sentinels_ok(buf, start, total), off, crc


class DeviceBatch:
    """Batch b uploaded once; encode() runs tkv_wal_encode_device into a fresh guarded device buffer."""

    def __init__(self, b, dev):
        import torch
        self.b, self.dev, self.torch = b, dev, torch
        self.t = {k: (None if b[k] is None else torch.from_numpy(b[k].view(np.int64) if b[k].dtype == np.uint64 else
                                                                 b[k].view(np.int32) if b[k].dtype == np.uint32 else
                                                                 b[k]).to(dev))
                  for k in ("keys", "key_off", "key_len", "vals", "val_off", "val_len", "op", "tomb", "seq")}

    def args(self):
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
        t = self.t
        return [p(t["keys"]), p(t["key_off"]), p(t["key_len"]), p(t["vals"]), p(t["val_off"]), p(t["val_len"]),
                p(t["op"]), p(t["tomb"]), p(t["seq"]), int(self.b["first_seq"]), int(self.b["n"])]

    def encode(self, lib, total, cap=None, align=0, stream=None):
        """(rc, img_size, image, sentinels intact, rec_off, crc), the arrays as numpy."""
        torch = self.torch
        n = self.b["n"]
        cap = total if cap is None else cap
        buf = torch.full((SENT + 32 + total + SENT,), 0xA5, dtype=torch.uint8, device=self.dev)
        start = SENT + (align - (buf.data_ptr() + SENT)) % 16
        off = torch.full((n,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=self.dev)
        crc = torch.full((n,), -0x5A5A5A5B, dtype=torch.int32, device=self.dev)
        torch.cuda.synchronize()
        size = U64(0)
        rc = lib.tkv_wal_encode_device(*self.args(), ctypes.c_void_p(buf.data_ptr() + start), cap,
                                       ctypes.c_void_p(off.data_ptr()), ctypes.c_void_p(crc.data_ptr()),
                                       ctypes.byref(size), stream)
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        return (rc, size.value, h[start:start + total].copy(), sentinels_ok(h, start, total),
                off.cpu().numpy().view(np.uint64), crc.cpu().numpy().view(np.uint32))


def last(lib):
    out = np.zeros(4, np.uint64)
    lib.tkv_debug_wal_encode_last(ctypes.c_void_p(out.ctypes.data))
    return [int(v) for v in out]


def geometry(lib):
    out = np.zeros(4, np.uint64)
    lib.tkv_debug_wal_encode_geometry(ctypes.c_void_p(out.ctypes.data))
    return [int(v) for v in out]


def golden_batch(records):
    """The golden records of tests/golden/wal.json as a batch (keys and values cut from their hex)."""
    raw = [bytes.fromhex(r["hex"]) for r in records]
    klen = np.array([int.from_bytes(x[18:22], "little") for x in raw], np.uint32)
    vlen = np.array([int.from_bytes(x[22:26], "little") for x in raw], np.uint32)
    keys = [x[26:26 + int(k)] for x, k in zip(raw, klen)]
    vals = [x[26 + int(k):26 + int(k) + int(v)] for x, k, v in zip(raw, klen, vlen)]

    def pack(chunks):
        off, out = [], b"\x11"
        for c in chunks:
            off.append(len(out))
            out += c + b"\x22\x33"
        return np.frombuffer(out, np.uint8).copy(), np.array(off, np.uint64)
    karena, koff = pack(keys)
    varena, voff = pack(vals)
    return dict(n=len(raw), keys=karena, key_off=koff, key_len=klen, vals=varena, val_off=voff, val_len=vlen,
                op=np.array([r["op"] for r in records], np.uint8),
                tomb=np.array([r["tombstone"] for r in records], np.uint8),
                seq=np.array([r["seq"] for r in records], np.uint64), first_seq=0), raw
