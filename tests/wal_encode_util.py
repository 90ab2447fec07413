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


def arena_at(rng, lens, residues, first_at_zero=False):
    """(arena, offsets) as arena(), but span i starts at an arena offset = residues[i] (mod 16): the
    gap in front of it is the 0-15 bytes of random filler that get it there. The first span is not at
    byte 0 unless first_at_zero (and residues[0] == 0)."""
    lens = np.asarray(lens, np.int64)
    res = np.asarray(residues, np.int64) % 16
    assert lens.size == res.size
    gap = np.zeros(lens.size, np.int64)
    if lens.size:
        gap[0] = res[0] if (res[0] or first_at_zero) else 16
        gap[1:] = (res[1:] - res[:-1] - lens[:-1]) % 16  # the span before ends at res + len (mod 16)
    off = np.cumsum(gap + lens) - lens
    assert np.array_equal(off % 16, res)
    data = rng.integers(0, 256, int((gap + lens).sum()) + 17, dtype=np.uint8)
    return data, off.astype(np.uint64)


def make_batch(rng, klen, vlen, plain=False, key_res=None, val_res=None):
    """A batch with random op / tombstone (0, 1, 0x80) / seq; plain: the defaults (NULL arrays) instead.
    key_res / val_res: the arena offset of every key / value modulo 16 (arena_at)."""
    klen, vlen = np.asarray(klen, np.uint32), np.asarray(vlen, np.uint32)
    n = klen.size
    keys, koff = arena(rng, klen) if key_res is None else arena_at(rng, klen, key_res)
    vals, voff = arena(rng, vlen) if val_res is None else arena_at(rng, vlen, val_res)
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

    def run(self, lib, total, cap=None, align=0, stream=None):
        """The call into a fresh guarded device buffer whose byte `start` lies `align` bytes past a 16-byte
        boundary: (rc, img_size, buffer, start, rec_off, crc), the last four on the device."""
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
        return rc, size.value, buf, start, off, crc

    def encode(self, lib, total, cap=None, align=0, stream=None):
        """(rc, img_size, image, sentinels intact, rec_off, crc), the arrays as numpy."""
        rc, size, buf, start, off, crc = self.run(lib, total, cap, align, stream)
        h = buf.cpu().numpy()
        return (rc, size, h[start:start + total].copy(), sentinels_ok(h, start, total),
                off.cpu().numpy().view(np.uint64), crc.cpu().numpy().view(np.uint32))


def encode_on_device(lib, db, total, align=0):
    """DeviceBatch.encode's call with the results left on the device: (guard buffer, start, rec_off, crc);
    the image is buffer[start:start + total] between its two sentinels."""
    rc, size, buf, start, off, crc = db.run(lib, total, align=align)
    assert rc == 0 and size == total, (rc, size, total)
    assert (buf.data_ptr() + start) % 16 == align % 16
    return buf, start, off, crc


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


def layout_host(lib, b, align=3):
    """tkv_debug_wal_encode_layout (the host layout, CRC fields zero) into a guarded buffer:
    (records laid out, img_size, image, sentinels intact)."""
    total = int(expected(b)[0].size)
    buf, start = guarded(total, align)
    size = U64(0)
    got = lib.tkv_debug_wal_encode_layout(*host_args(b), ctypes.c_void_p(buf.ctypes.data + start), total,
                                          ctypes.byref(size))
    return got, size.value, buf[start:start + total].copy(), sentinels_ok(buf, start, total)


# ---- grids: batches that hold every case of a kernel path, and the counts that prove it ---------------
# A record's image address modulo 16 is set by a filler in front of it: a record with an empty value and
# a key of 0-15 bytes (26-41 bytes, record_len 18-33) moves the next start to any residue. The builders
# lay the residues out against image offset 0 and arena offset 0; with the real pointers the residues
# are rotated, which leaves a full grid full (the counters below take the pointers' residues).

FUSED_LENS = range(18, 243)  # record_len: 18..240 folded by the emit pass, 241 and 242 read back
SPAN_SHORT = tuple(range(65, 81))  # with all (source, destination) residues: every wave_copy triple
VAL_LONG = (127, 128, 129, 131, 255, 256, 257, 511, 1000, 1023, 1024, 1025, 1040, 2047, 2048, 2049, 3000, 4095, 4096,
            4097, 4400)
KEY_LONG = (200, 1024, 4097)


def fused_grid_batch(rng):
    """A target record for every (record_len in FUSED_LENS, image offset of its first byte mod 16), in
    random order, each behind its filler. The body (record_len - 18 bytes) is all key (kind 0), all value
    (kind 1) or split at random (kind 2), rotating over the residues. b["target"] marks the targets,
    b["kind"] their kinds (-1: filler)."""
    cells = [(rl, r) for rl in FUSED_LENS for r in range(16)]
    klen, vlen, target, kind = [], [], [], []
    pos = 0
    for j in rng.permutation(len(cells)):
        rl, r = cells[j]
        f = (r - pos - 26) % 16
        klen.append(f), vlen.append(0), target.append(False), kind.append(-1)
        pos += 26 + f
        body, kd = rl - 18, (rl + r) % 3
        k = body if kd == 0 else 0 if kd == 1 else int(rng.integers(0, body + 1))
        klen.append(k), vlen.append(body - k), target.append(True), kind.append(kd)
        pos += 8 + rl
    n = len(klen)
    b = make_batch(rng, klen, vlen, key_res=rng.integers(0, 16, n), val_res=rng.integers(0, 16, n))
    b["target"], b["kind"] = np.array(target), np.array(kind)
    return b


def fused_pairs(b, offs, img_res=0):
    """The distinct (record_len, address of the first byte mod 16) of b's targets, as record_len * 16 +
    residue, for an image at an address = img_res (mod 16)."""
    t = b["target"]
    rl = 18 + b["key_len"].astype(np.int64) + b["val_len"].astype(np.int64)
    return np.unique(rl[t] * 16 + (offs.astype(np.int64)[t] + img_res) % 16)


def span_grid_batch(rng, lengths, which):
    """A target record for every (length in lengths, source residue, destination residue) of its long
    span, in random order. which == "val": the value is the long span and the key (0-15 bytes) the filler
    that puts it at its residue. which == "key": the key is the long span, behind a filler record, with
    a value of 0-15 bytes behind it. The residues are those of the arena offset and of the image offset
    of the span's first byte."""
    cells = [(ln, s, d) for ln in lengths for s in range(16) for d in range(16)]
    klen, vlen, kres, vres, target = [], [], [], [], []
    pos = 0
    for j in rng.permutation(len(cells)):
        ln, s, d = cells[j]
        other = int(rng.integers(0, 16))
        if which == "val":
            k = (d - pos - 26) % 16
            klen.append(k), vlen.append(ln), kres.append(other), vres.append(s), target.append(True)
            pos += 26 + k + ln
        else:
            f = (d - 26 - pos - 26) % 16
            klen.append(f), vlen.append(0), kres.append(other), vres.append(0), target.append(False)
            v = int(rng.integers(0, 16))
            klen.append(ln), vlen.append(v), kres.append(s), vres.append(other), target.append(True)
            pos += 26 + f + 26 + ln + v
    b = make_batch(rng, klen, vlen, key_res=kres, val_res=vres)
    b["target"] = np.array(target)
    return b


def span_cases(b, offs, which, src_res=0, img_res=0):
    """(length, relative, destination, end) of every target's long span: what selects wave_copy's path,
    (source - destination) mod 16, destination mod 16 and end mod 16, for an arena at an address =
    src_res and an image at an address = img_res (mod 16). One row per target."""
    t = b["target"]
    kl = b["key_len"].astype(np.int64)[t]
    o = offs.astype(np.int64)[t]
    if which == "val":
        ln, src, dst = b["val_len"].astype(np.int64)[t], b["val_off"].astype(np.int64)[t], o + 26 + kl
    else:
        ln, src, dst = kl, b["key_off"].astype(np.int64)[t], o + 26
    src, dst = (src + src_res) % 16, (dst + img_res) % 16
    return np.stack([ln, (src - dst) % 16, dst, (dst + ln) % 16], 1)


def span_coverage(cases, short=SPAN_SHORT):
    """({length: distinct (relative, destination) pairs}, distinct (relative, destination, end) triples
    among the lengths of `short`)."""
    pairs = {int(ln): int(np.unique(cases[cases[:, 0] == ln][:, 1] * 16 + cases[cases[:, 0] == ln][:, 2]).size)
             for ln in np.unique(cases[:, 0])}
    s = cases[np.isin(cases[:, 0], short)]
    return pairs, int(np.unique(s[:, 1] * 256 + s[:, 2] * 16 + s[:, 3]).size)


def loop_pattern(rng, size, tile, mids=(1, 4), giants=4):
    """A batch of about `size` bytes (odd) for tiling: groups of a run of 65-100 records of 26-40 bytes
    (more records than lanes start in a tile), mids[0]..mids[1]-1 records with values of 100-3000 bytes, a
    record_len 240 and a record_len 241 record; `giants` of the groups also hold a record longer than two
    tiles (tiles in which no record starts), its value and its key long in turn. op, tomb and seq are
    explicit."""
    klen, vlen = [], []
    pos, groups = 0, 0
    est = 83 * 33 + (mids[0] + mids[1] - 1) * 790 + 500
    every = max(1, size // est // max(1, giants))
    while pos < size:
        m = int(rng.integers(65, 101))
        body = rng.integers(0, 15, m)
        k = (rng.random(m) * (body + 1)).astype(np.int64)
        nm = int(rng.integers(mids[0], mids[1]))
        k2, v2 = rng.integers(4, 24, nm), rng.integers(100, 3001, nm)
        ks = [k, k2, [10, 9]]
        vs = [body - k, v2, [212, 214]]
        if groups % every == every // 2 and groups // every < giants:
            big, short = 2 * tile + int(rng.integers(1, tile)), int(rng.integers(0, 24))
            ks.append([big if (groups // every) % 2 else short])  # a long value, then a long key, in turn
            vs.append([short if (groups // every) % 2 else big])
        ks, vs = np.concatenate(ks).astype(np.int64), np.concatenate(vs).astype(np.int64)
        p = rng.permutation(ks.size - m)  # the run stays a run; what follows it is shuffled
        ks[m:], vs[m:] = ks[m:][p], vs[m:][p]
        klen.append(ks), vlen.append(vs)
        pos += int((26 + ks + vs).sum())
        groups += 1
    if pos % 2 == 0:
        klen.append(np.array([1])), vlen.append(np.array([0]))
    return make_batch(rng, np.concatenate(klen), np.concatenate(vlen))


def tiled(b, reps):
    """b's records `reps` times over: the per-record arrays repeated (op, tomb and seq too, so every
    repetition is byte for byte the same), the arenas shared. b's image has an odd size, so every
    repetition lies at another residue mod 16 and another phase of the emit tile."""
    assert b["op"] is not None and b["tomb"] is not None and b["seq"] is not None
    assert int((26 + b["key_len"].astype(np.int64) + b["val_len"].astype(np.int64)).sum()) % 2 == 1
    t = dict(b, n=b["n"] * reps)
    for k in ("key_off", "key_len", "val_off", "val_len", "op", "tomb", "seq"):
        t[k] = np.tile(b[k], reps)
    return t


def tiled_expected(exp, reps):
    """expected() of tiled(b, reps) from exp = expected(b, oracle)."""
    img, offs, crc = exp
    base = np.arange(reps, dtype=np.uint64) * np.uint64(img.size)
    return np.tile(img, reps), (base[:, None] + offs[None, :]).reshape(-1), np.tile(crc, reps)
