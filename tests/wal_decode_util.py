"""Helpers of the WAL decode tests: wal_entry::decode's field extraction and structural checks
(wal.cpp:63-87 without the checksum, :98-125) restated in numpy, guarded outputs on the host and on the
device, and the C calls. Test images come from wal_encode_util.expected (the numpy encode)."""
import ctypes

import numpy as np

from wal_encode_util import SENT, U64, _spread, guarded, sentinels_ok

KEY_VIEWS, VAL_VIEWS = 1, 2
FLAGS = (0, KEY_VIEWS, VAL_VIEWS, KEY_VIEWS | VAL_VIEWS)
COLS = ("op", "tomb", "seq", "key_off", "key_len", "val_off", "val_len")
DTYPES = dict(op=np.uint8, tomb=np.uint8, seq=np.uint64, key_off=np.uint64, key_len=np.uint32, val_off=np.uint64,
              val_len=np.uint32)
FILL = dict(op=0xA5, tomb=0xA5, seq=0xA5A5A5A5A5A5A5A5, key_off=0xA5A5A5A5A5A5A5A5, key_len=0xA5A5A5A5,
            val_off=0xA5A5A5A5A5A5A5A5, val_len=0xA5A5A5A5)


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _le(hdr, lo, hi, dt):
    return np.ascontiguousarray(hdr[:, lo:hi]).view(dt).reshape(-1)


def first_bad(img, offs, size=None):
    """Index of the first record that fails wal_entry::decode's structural checks (len(offs) when none):
    fewer than 26 bytes left (wal.cpp:68), record_len + 8 past the end (:83), 18 + key_len + val_len >
    record_len (:118-121). Python integers: no wrap."""
    size = img.size if size is None else size
    for i, o in enumerate(int(x) for x in offs):
        left = size - o if o < size else 0
        if left < 26:
            return i
        rl = int.from_bytes(img[o:o + 4].tobytes(), "little")
        kl = int.from_bytes(img[o + 18:o + 22].tobytes(), "little")
        vl = int.from_bytes(img[o + 22:o + 26].tobytes(), "little")
        if rl + 8 > left or 18 + kl + vl > rl:
            return i
    return len(offs)


def expected(img, offs, flags=0):
    """The decode of the (good) records at offs: dict of the seven columns, keys, vals (None for a views
    arena), keys_size, vals_size. wal.cpp:98-125: operation_ byte 8, sequence_ u64 at 9, tombstone_ byte
    17, key_len / value_len u32 at 18 / 22, key_ behind the header, value_ behind the key."""
    o = np.asarray(offs, np.uint64).astype(np.int64)
    n = o.size
    hdr = img[o[:, None] + np.arange(26)] if n else np.zeros((0, 26), np.uint8)
    kl, vl = _le(hdr, 18, 22, "<u4"), _le(hdr, 22, 26, "<u4")
    e = dict(op=hdr[:, 8].copy(), tomb=hdr[:, 17].copy(), seq=_le(hdr, 9, 17, "<u8").astype(np.uint64),
             key_len=kl.astype(np.uint32), val_len=vl.astype(np.uint32))
    kpre = np.cumsum(kl.astype(np.uint64)) - kl
    vpre = np.cumsum(vl.astype(np.uint64)) - vl
    e["key_off"] = (o + 26).astype(np.uint64) if flags & KEY_VIEWS else kpre.astype(np.uint64)
    e["val_off"] = (o + 26 + kl.astype(np.int64)).astype(np.uint64) if flags & VAL_VIEWS else vpre.astype(np.uint64)
    w, j = _spread(kl)
    e["keys"] = None if flags & KEY_VIEWS else img[o[w] + 26 + j]
    w, j = _spread(vl)
    e["vals"] = None if flags & VAL_VIEWS else img[o[w] + 26 + kl.astype(np.int64)[w] + j]
    e["keys_size"], e["vals_size"] = int(kl.sum(dtype=np.uint64)), int(vl.sum(dtype=np.uint64))
    return e


class HostOut:
    """Guarded host outputs: the columns filled with 0xA5 patterns, each arena of `cap` bytes at a given
    alignment between two sentinels (None: a NULL arena)."""

    def __init__(self, n, kcap, vcap, kalign=0, valign=0, cols=COLS):
        self.n = n
        self.c = {k: (np.full(n, FILL[k], DTYPES[k]) if k in cols else None) for k in COLS}
        self.kcap, self.vcap = kcap, vcap
        self.kbuf, self.kstart = guarded(kcap, kalign) if kcap is not None else (None, 0)
        self.vbuf, self.vstart = guarded(vcap, valign) if vcap is not None else (None, 0)

    def args(self):
        kp = None if self.kbuf is None else ctypes.c_void_p(self.kbuf.ctypes.data + self.kstart)
        vp = None if self.vbuf is None else ctypes.c_void_p(self.vbuf.ctypes.data + self.vstart)
        return [_ptr(self.c[k]) for k in COLS] + [kp, self.kcap or 0, vp, self.vcap or 0]

    def untouched(self):
        return (all(c is None or bool((c == FILL[k]).all()) for k, c in self.c.items()) and
                (self.kbuf is None or bool((self.kbuf == 0xA5).all())) and
                (self.vbuf is None or bool((self.vbuf == 0xA5).all())))

    def arena(self, which, size):
        buf, start = (self.kbuf, self.kstart) if which == "keys" else (self.vbuf, self.vstart)
        return buf[start:start + size]

    def guards_ok(self, ks, vs):
        return ((self.kbuf is None or sentinels_ok(self.kbuf, self.kstart, ks) and
                 bool((self.kbuf[self.kstart + ks:] == 0xA5).all())) and
                (self.vbuf is None or sentinels_ok(self.vbuf, self.vstart, vs) and
                 bool((self.vbuf[self.vstart + vs:] == 0xA5).all())))


def decode_host(lib, img, offs, flags, out, size=None, n=None):
    """tkv_wal_decode_host into out: (rc, keys_size, vals_size, first_bad)."""
    offs = np.ascontiguousarray(offs, np.uint64)
    ks, vs, fb = U64(7), U64(7), U64(7)
    rc = lib.tkv_wal_decode_host(_ptr(img), img.size if size is None else size, _ptr(offs), offs.size if n is None else n,
                                 flags, *out.args(), ctypes.byref(ks), ctypes.byref(vs), ctypes.byref(fb))
    return rc, ks.value, vs.value, fb.value


def compare(got_cols, keys, vals, want):
    """All columns and arenas against expected(): raises with the first difference."""
    for k in COLS:
        if got_cols[k] is not None:
            bad = np.flatnonzero(got_cols[k] != want[k])
            assert bad.size == 0, f"{k} differs for {bad.size} records, first {bad[0]}: got {got_cols[k][bad[0]]} want {want[k][bad[0]]}"
    for name, got in (("keys", keys), ("vals", vals)):
        if want[name] is not None:
            assert got.size == want[name].size, (name, got.size, want[name].size)
            bad = np.flatnonzero(got != want[name])
            assert bad.size == 0, f"{name} arena differs in {bad.size} bytes, first at {bad[0]}"


def check_host(lib, img, offs, flags, kalign=0, valign=0):
    """A full decode on the host against expected(), sentinels included; returns (out, want)."""
    want = expected(img, offs, flags)
    kcap = None if flags & KEY_VIEWS else want["keys_size"]
    vcap = None if flags & VAL_VIEWS else want["vals_size"]
    out = HostOut(len(offs), kcap, vcap, kalign, valign)
    rc, ks, vs, fb = decode_host(lib, img, offs, flags, out)
    assert (rc, ks, vs, fb) == (0, want["keys_size"], want["vals_size"], len(offs)), (rc, ks, vs, fb)
    assert out.guards_ok(ks, vs), "bytes outside a destination were written"
    compare(out.c, None if kcap is None else out.arena("keys", ks), None if vcap is None else out.arena("vals", vs), want)
    return out, want


def as_batch(cols, keys, vals):
    """Decoded columns and arenas as a wal_encode_util batch."""
    return dict(n=cols["op"].size, keys=keys, key_off=cols["key_off"], key_len=cols["key_len"], vals=vals,
                val_off=cols["val_off"], val_len=cols["val_len"], op=cols["op"], tomb=cols["tomb"], seq=cols["seq"],
                first_seq=0)


def geometry(lib):
    out = np.zeros(4, np.uint64)
    lib.tkv_debug_wal_decode_geometry(ctypes.c_void_p(out.ctypes.data))
    return [int(v) for v in out]


def last(lib):
    out = np.zeros(4, np.uint64)
    lib.tkv_debug_wal_decode_last(ctypes.c_void_p(out.ctypes.data))
    return [int(v) for v in out]


# ---- the device -------------------------------------------------------------------------------------------

TORCH_DT = dict(op="uint8", tomb="uint8", seq="int64", key_off="int64", key_len="int32", val_off="int64", val_len="int32")
TORCH_FILL = dict(op=0xA5, tomb=0xA5, seq=-0x5A5A5A5A5A5A5A5B, key_off=-0x5A5A5A5A5A5A5A5B, key_len=-0x5A5A5A5B,
                  val_off=-0x5A5A5A5A5A5A5A5B, val_len=-0x5A5A5A5B)


class DevOut:
    """HostOut on the device."""

    def __init__(self, dev, n, kcap, vcap, kalign=0, valign=0):
        import torch
        self.torch, self.n = torch, n
        self.c = {k: torch.full((n,), TORCH_FILL[k], dtype=getattr(torch, TORCH_DT[k]), device=dev) for k in COLS}
        self.kcap, self.vcap = kcap, vcap
        self.kbuf, self.kstart = self._guarded(dev, kcap, kalign) if kcap is not None else (None, 0)
        self.vbuf, self.vstart = self._guarded(dev, vcap, valign) if vcap is not None else (None, 0)

    def _guarded(self, dev, total, align):
        buf = self.torch.full((SENT + 32 + total + SENT,), 0xA5, dtype=self.torch.uint8, device=dev)
        return buf, SENT + (align - (buf.data_ptr() + SENT)) % 16

    def args(self):
        kp = None if self.kbuf is None else ctypes.c_void_p(self.kbuf.data_ptr() + self.kstart)
        vp = None if self.vbuf is None else ctypes.c_void_p(self.vbuf.data_ptr() + self.vstart)
        return [ctypes.c_void_p(self.c[k].data_ptr()) if self.n else None for k in COLS] + [kp, self.kcap or 0, vp,
                                                                                             self.vcap or 0]

    def untouched(self):
        return (all(bool((c == TORCH_FILL[k]).all()) for k, c in self.c.items()) and
                (self.kbuf is None or bool((self.kbuf == 0xA5).all())) and
                (self.vbuf is None or bool((self.vbuf == 0xA5).all())))

    def cols(self):
        return {k: c.cpu().numpy().view(DTYPES[k]) for k, c in self.c.items()}

    def arena(self, which, size):
        buf, start = (self.kbuf, self.kstart) if which == "keys" else (self.vbuf, self.vstart)
        return buf[start:start + size]

    def guards_ok(self, ks, vs):
        ok = True
        for buf, start, sz in ((self.kbuf, self.kstart, ks), (self.vbuf, self.vstart, vs)):
            if buf is not None:
                ok = ok and bool((buf[:start] == 0xA5).all()) and bool((buf[start + sz:] == 0xA5).all())
        return ok


def dev_offsets(dev, offs, u32=False):
    import torch
    offs = np.ascontiguousarray(offs, np.uint64)
    return torch.from_numpy(offs.astype(np.uint32).view(np.int32) if u32 else offs.view(np.int64)).to(dev)


def decode_device(lib, image, doffs, flags, out, size=None, stream=None):
    """tkv_wal_decode_device (image and doffs device tensors, doffs int64 or int32) into out:
    (rc, keys_size, vals_size, first_bad)."""
    import torch
    ks, vs, fb = U64(7), U64(7), U64(7)
    p = ctypes.c_void_p(doffs.data_ptr()) if doffs.numel() else None
    o64, o32 = (p, None) if doffs.dtype == torch.int64 else (None, p)
    torch.cuda.synchronize()
    rc = lib.tkv_wal_decode_device(ctypes.c_void_p(image.data_ptr()), image.numel() if size is None else size, o64, o32,
                                   doffs.numel(), flags, *out.args(), ctypes.byref(ks), ctypes.byref(vs), ctypes.byref(fb),
                                   stream)
    torch.cuda.synchronize()
    return rc, ks.value, vs.value, fb.value


def check_device(lib, dev, image, img, offs, flags, kalign=0, valign=0, u32=False, stream=None, want=None, doffs=None):
    """A full decode on the device of image (= img on the host) against expected(), every column and
    arena byte and the sentinels; returns (out, want). doffs: a device list that holds offs already
    (int64 or int32), read in place instead of an upload of offs."""
    want = expected(img, offs, flags) if want is None else want
    kcap = None if flags & KEY_VIEWS else want["keys_size"]
    vcap = None if flags & VAL_VIEWS else want["vals_size"]
    out = DevOut(dev, len(offs), kcap, vcap, kalign, valign)
    if kcap is not None:
        assert (out.kbuf.data_ptr() + out.kstart) % 16 == kalign % 16
    doffs = dev_offsets(dev, offs, u32) if doffs is None else doffs
    assert doffs.numel() == len(offs)
    rc, ks, vs, fb = decode_device(lib, image, doffs, flags, out, stream=stream)
    assert (rc, ks, vs, fb) == (0, want["keys_size"], want["vals_size"], len(offs)), (rc, ks, vs, fb)
    assert out.guards_ok(ks, vs), "bytes outside a destination were written"
    compare(out.cols(), None if kcap is None else out.arena("keys", ks).cpu().numpy(),
            None if vcap is None else out.arena("vals", vs).cpu().numpy(), want)
    st = last(lib)
    assert st[2:] == [ks, vs] and (st[0] > 0) == bool(kcap) and (st[1] > 0) == bool(vcap), st
    return out, want


# ---- batches that hold every case of a path, and the counts that prove it ---------------------------------

def corrupt(kind, img, offs, i):
    """(image, size, offsets) with record i failing one structural check."""
    img, offs = img.copy(), offs.copy()
    size = img.size
    if kind == "short":          # fewer than 26 bytes left at the offset
        offs[i] = size - 25
    elif kind == "record_len":   # record_len + 8 past size
        at = int(offs[i])
        img[at:at + 4] = np.frombuffer((size - at - 8 + 1).to_bytes(4, "little"), np.uint8)
    else:                        # key_len = 0xFFFFFFFF (18 + key_len + val_len wraps in u32) in a record at the image end
        rec = img[int(offs[-1]):].copy()
        rec[18:22] = 0xFF
        offs[i] = size
        img = np.concatenate([img, rec])
        size = img.size
    return img, size, offs


GRID_SHORT = tuple(range(65, 81))
GRID_LONG = (127, 1024, 4095, 4096, 4097, 8200)


def grid_lens(rng, lengths, which):
    """(key_len, val_len, target) of a batch with a target record for every (length, source residue,
    destination residue) of its long span, in random order, each behind a filler record. which == "key":
    the target's key is the span; the filler's key length (0-15) moves the key arena position and the
    image position, its value length (0-15) the image position alone. which == "val": the roles are
    swapped. Source residue: image offset of the span's first byte mod 16; destination residue: its
    arena offset mod 16."""
    cells = [(ln, s, d) for ln in lengths for s in range(16) for d in range(16)]
    klen, vlen, target = [], [], []
    pos = apos = 0  # image offset of the next record, arena offset of the next span
    for j in rng.permutation(len(cells)):
        ln, s, d = cells[j]
        other = int(rng.integers(0, 16))  # the target's other span
        f_arena = (d - apos) % 16
        if which == "key":
            f_img = (s - (pos + 26 + f_arena + 26)) % 16
            klen += [f_arena, ln]
            vlen += [f_img, other]
        else:
            f_img = (s - (pos + 26 + f_arena + 26 + other)) % 16
            klen += [f_img, other]
            vlen += [f_arena, ln]
        target += [False, True]
        pos += 26 + f_arena + f_img + 26 + ln + other
        apos += f_arena + ln
    return np.array(klen), np.array(vlen), np.array(target)


def grid_coverage(want, offs, target, which, img_res=0, arena_res=0):
    """{length: distinct (source, destination) residue pairs} of the targets' long spans, for an image at
    an address = img_res and an arena at an address = arena_res (mod 16)."""
    o = offs.astype(np.int64)[target]
    kl = want["key_len"].astype(np.int64)[target]
    if which == "key":
        ln, src, dst = kl, o + 26, want["key_off"].astype(np.int64)[target]
    else:
        ln, src, dst = want["val_len"].astype(np.int64)[target], o + 26 + kl, want["val_off"].astype(np.int64)[target]
    pair = ((src + img_res) % 16) * 16 + (dst + arena_res) % 16
    return {int(v): int(np.unique(pair[ln == v]).size) for v in np.unique(ln)}


def tiled_want(want, img_size, reps):
    """expected() of the image of wal_encode_util.tiled(b, reps) with all its offsets, copied arenas,
    from want = expected() of one repetition."""
    t = {k: np.tile(want[k], reps) for k in ("op", "tomb", "seq", "key_len", "val_len")}
    n = want["op"].size
    rep = np.repeat(np.arange(reps, dtype=np.uint64), n)
    t["key_off"] = np.tile(want["key_off"], reps) + rep * np.uint64(want["keys_size"])
    t["val_off"] = np.tile(want["val_off"], reps) + rep * np.uint64(want["vals_size"])
    t["keys"], t["vals"] = np.tile(want["keys"], reps), np.tile(want["vals"], reps)
    t["keys_size"], t["vals_size"] = want["keys_size"] * reps, want["vals_size"] * reps
    return t
