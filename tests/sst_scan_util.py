"""Sequential oracle of the SSTable scan (tkv_sst_scan[_device]) and the mutation catalogue its tests share.

``oracle_scan`` restates the reader's contract (include/tkv_crc32.h "SSTable scan") one byte at a time:
footer, index, then every block, in that order of precedence. It has its own varint reader and struct
unpacking, checks stamps with zlib.crc32 and does not use tinykvpp_amd.sst.

``block_image`` / ``make_file`` write files by hand, field by field, so that a test can break exactly one
rule and stamp the result again: then the structural check is what fails and not the checksum.
``mutations`` is the catalogue: one named file per check of the contract.
"""
import ctypes
import struct
import zlib

import numpy as np

BAD_FOOTER = 2**64 - 1
BAD_INDEX = 2**64 - 2
KEY_VIEWS, VAL_VIEWS = 1, 2


def varint(v, pad=0):
    """LEB128(v); ``pad`` extra bytes make a redundant encoding (80 00 for v = 0, pad = 1)."""
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    for _ in range(pad):
        out[-1] |= 0x80
        out.append(0)
    return bytes(out)


def read_varint(buf, pos, end, maxb):
    """(value, next position) of the varint at pos that ends within maxb bytes and before end, or None."""
    v = 0
    for k in range(maxb):
        if pos + k >= end:
            return None
        b = buf[pos + k]
        v |= (b & 0x7F) << (7 * k)
        if b < 0x80:
            return v, pos + k + 1
    return None


def _block(buf, off, size, ikey, check_crc):
    """The entries [(key, value)] of the image [off, off + size) or None when a check fails."""
    img = buf[off:off + size]
    if img[0] != 0x14:
        return None
    c, z, z2, comp = struct.unpack_from("<IIIB", img, 1)
    stored = struct.unpack_from("<I", img, 17)[0]
    if z2 != z or comp != 0 or 36 + z != size or c < 1 or 8 * c > z:
        return None
    zv = read_varint(img, 21, size, 5)
    if zv is None or zv[0] != z:
        return None
    if check_crc and zlib.crc32(img[:17] + b"\0\0\0\0" + img[21:]) != stored:
        return None
    body = img[zv[1]:zv[1] + z]
    assert len(body) == z
    pos, total, out = 0, 0, []
    for _ in range(c):
        strings = []
        for _ in range(2):
            lv = read_varint(body, pos, z, 4)
            if lv is None or lv[1] + lv[0] > z:
                return None
            strings.append(body[lv[1]:lv[1] + lv[0]])
            pos = lv[1] + lv[0]
        total += 8 + len(strings[0]) + len(strings[1])
        out.append((strings[0], strings[1]))
    if total != z or out[0][0] != ikey:
        return None
    return out


def oracle_scan(file_bytes, check_crc=True):
    """(status, bad_block, entries, blocks): status "ok" or "corrupted"; bad_block BAD_FOOTER, BAD_INDEX,
    the smallest bad block's number, or the block count when ok; entries [(key, value)] in index order
    and blocks [(offset, size, first_entry)] (both empty when corrupted)."""
    buf = bytes(file_bytes)
    n = len(buf)
    if n < 28 or n > 2**32 - 1:
        return "corrupted", BAD_FOOTER, [], []
    ioff, isz, _, _, crc = struct.unpack("<IIIII", buf[-20:])
    if ioff + isz + 20 != n or isz < 8:
        return "corrupted", BAD_FOOTER, [], []
    if check_crc and zlib.crc32(buf[ioff:ioff + isz + 16]) != crc:
        return "corrupted", BAD_FOOTER, [], []
    idx = buf[ioff:ioff + isz]
    (count,) = struct.unpack_from("<Q", idx, 0)
    if count > (isz - 8) // 17:
        return "corrupted", BAD_INDEX, [], []
    pos, index = 8, []
    for _ in range(count):
        lv = read_varint(idx, pos, isz, 4)
        if lv is None or lv[1] + lv[0] + 16 > isz:
            return "corrupted", BAD_INDEX, [], []
        key = idx[lv[1]:lv[1] + lv[0]]
        off, size = struct.unpack_from("<QQ", idx, lv[1] + lv[0])
        if size < 22 or off + size > ioff:
            return "corrupted", BAD_INDEX, [], []
        index.append((key, off, size))
        pos = lv[1] + lv[0] + 16
    if pos != isz:
        return "corrupted", BAD_INDEX, [], []
    entries, blocks = [], []
    for j, (key, off, size) in enumerate(index):
        got = _block(buf, off, size, key, check_crc)
        if got is None:
            return "corrupted", j, [], []
        blocks.append((off, size, len(entries)))
        entries += got
    return "ok", len(index), entries, blocks


# ---- files written by hand ----------------------------------------------------------------------------

def entry_bytes(key, value, kpad=0, vpad=0):
    return varint(len(key), kpad) + key + varint(len(value), vpad) + value


def block_image(entries, c=None, z=None, z2=None, b0=0x14, comp=0, zvar=None, body=None, size=None, fill=0):
    """A stamped data-block image. By default what the writer makes of ``entries``; every field can be
    overridden. ``body`` replaces the written entries, ``fill`` is the slack and padding byte."""
    counted = sum(8 + len(k) + len(v) for k, v in entries)
    z = counted if z is None else z
    c = len(entries) if c is None else c
    body = b"".join(entry_bytes(k, v) for k, v in entries) if body is None else body
    head = bytes([b0]) + struct.pack("<IIIB3xI", c & 0xFFFFFFFF, z, z if z2 is None else z2, comp, 0)
    img = bytearray(head + (varint(z) if zvar is None else zvar) + body)
    size = 36 + z if size is None else size
    img = bytearray(bytes(img[:size]).ljust(size, bytes([fill])))
    return stamp_block(img)


def stamp_block(img):
    img = bytearray(img)
    img[17:21] = b"\0\0\0\0"
    struct.pack_into("<I", img, 17, zlib.crc32(bytes(img)))
    return bytes(img)


def index_image(entries, count=None, kpad=0):
    """entries: [(key, offset, size)] or raw bytes items (taken as they are)."""
    out = bytearray(struct.pack("<Q", len(entries) if count is None else count))
    for e in entries:
        out += e if isinstance(e, (bytes, bytearray)) else varint(len(e[0]), kpad) + e[0] + struct.pack("<QQ", e[1], e[2])
    return bytes(out)


def make_file(data, index, ioff=None, isz=None):
    """data region || index || footer, the footer stamped over what its own fields describe (when they
    describe a span of the file)."""
    ioff = len(data) if ioff is None else ioff
    isz = len(index) if isz is None else isz
    buf = bytearray(data + index + struct.pack("<IIIII", ioff & 0xFFFFFFFF, isz & 0xFFFFFFFF, 0, 0, 0))
    return restamp_footer(buf)


def restamp_footer(buf):
    buf = bytearray(buf)
    ioff, isz = struct.unpack_from("<II", buf, len(buf) - 20)
    if ioff + isz + 16 <= len(buf):
        struct.pack_into("<I", buf, len(buf) - 4, zlib.crc32(bytes(buf[ioff:ioff + isz + 16])))
    return bytes(buf)


def file_of_blocks(block_entries, **kw):
    """A file of the blocks [[(key, value), ...], ...] back to back, indexed in order."""
    data, idx = bytearray(), []
    for ents in block_entries:
        img = block_image(ents, **kw)
        idx.append((ents[0][0], len(data), len(img)))
        data += img
    return make_file(bytes(data), index_image(idx))


BASE_BLOCKS = [
    [(b"apple", b"red"), (b"apricot", b"")],
    [(b"banana", b"yellow" * 30), (b"", b"x")],
    [(b"cherry", b"dark red"), (b"citron", b"y" * 130), (b"cranberry", b"tart")],
]


def mutations():
    """{name: (file bytes, expected bad_block or "ok")}: one file per check of the contract, each stamped
    again after the change so that the named check is the one that fails."""
    imgs = [block_image(e) for e in BASE_BLOCKS]
    offs = [sum(len(i) for i in imgs[:j]) for j in range(3)]
    data = b"".join(imgs)
    idx = [(e[0][0], offs[j], len(imgs[j])) for j, e in enumerate(BASE_BLOCKS)]
    base_index = index_image(idx)
    m = {}

    def with_block(j, img):
        """Block j replaced by an image of the same size."""
        assert len(img) == len(imgs[j])
        d = bytearray(data)
        d[offs[j]:offs[j] + len(img)] = img
        return make_file(bytes(d), base_index)

    def with_index(index, **kw):
        return make_file(data, index, **kw)

    m["base"] = (make_file(data, base_index), "ok")
    # footer
    m["footer_sum_plus_1"] = (with_index(base_index, ioff=len(data) + 1), BAD_FOOTER)
    m["footer_sum_minus_1"] = (with_index(base_index, isz=len(base_index) - 1), BAD_FOOTER)
    m["index_size_7"] = (make_file(data, b"\0" * 7), BAD_FOOTER)
    bad_crc = bytearray(m["base"][0])
    bad_crc[-1] ^= 0x40
    m["footer_crc"] = (bytes(bad_crc), BAD_FOOTER)
    bloom = bytearray(m["base"][0])
    struct.pack_into("<II", bloom, len(bloom) - 12, 77, 99)
    m["bloom_fields_free"] = (restamp_footer(bloom), "ok")
    m["short_file_27"] = (b"\0" * 27, BAD_FOOTER)
    # index
    m["B_too_large"] = (with_index(index_image(idx, count=(len(base_index) - 8) // 17 + 1)), BAD_INDEX)
    m["B_one_more"] = (with_index(index_image(idx, count=4)), BAD_INDEX)
    m["B_one_less"] = (with_index(index_image(idx, count=2)), BAD_INDEX)
    raw = lambda e, lenbytes: lenbytes + e[0] + struct.pack("<QQ", e[1], e[2])  # noqa: E731
    m["index_varint_5"] = (with_index(index_image([raw(idx[0], varint(len(idx[0][0]), 4)), idx[1], idx[2]])), BAD_INDEX)
    m["index_varint_4_redundant_ok"] = (with_index(index_image([raw(idx[0], varint(len(idx[0][0]), 3)), idx[1], idx[2]])), "ok")
    m["index_entry_past_index"] = (with_index(index_image([idx[0], idx[1], raw(idx[2], varint(len(idx[2][0]) + 1))])), BAD_INDEX)
    m["index_block_past_data"] = (with_index(index_image([idx[0], idx[1], (idx[2][0], idx[2][1], idx[2][2] + 1)])), BAD_INDEX)
    m["index_block_off_huge"] = (with_index(index_image([idx[0], (idx[1][0], 2**64 - 8, 44), idx[2]])), BAD_INDEX)
    m["index_block_size_21"] = (with_index(index_image([idx[0], (idx[1][0], idx[1][1], 21), idx[2]])), BAD_INDEX)
    m["index_trailing_byte"] = (with_index(base_index + b"\0"), BAD_INDEX)
    m["index_truncated"] = (with_index(base_index[:-1]), BAD_INDEX)
    # block headers (block 1, so that the smallest bad index is not trivially 0)
    e1 = BASE_BLOCKS[1]
    z1 = sum(8 + len(k) + len(v) for k, v in e1)
    m["byte0_not_0x14"] = (with_block(1, block_image(e1, b0=0x15)), 1)
    m["u32_at_9_not_z"] = (with_block(1, block_image(e1, z2=z1 + 1)), 1)
    m["compression_1"] = (with_block(1, block_image(e1, comp=1)), 1)
    m["size_not_36_plus_z"] = (with_block(1, block_image(e1, z=z1 - 1, size=36 + z1)), 1)
    m["c_0"] = (with_block(1, block_image(e1, c=0)), 1)
    m["8c_over_z"] = (with_block(1, block_image(e1, c=z1 // 8 + 1)), 1)
    m["body_varint_not_z"] = (with_block(1, block_image(e1, zvar=varint(z1 - 1))), 1)
    m["body_varint_6_bytes"] = (with_block(1, block_image(e1, zvar=varint(z1, 6 - len(varint(z1))))), 1)
    m["body_varint_5_redundant_ok"] = (with_block(1, block_image(e1, zvar=varint(z1, 5 - len(varint(z1))))), "ok")
    m["c_one_more"] = (with_block(2, block_image(BASE_BLOCKS[2], c=4)), 2)
    m["c_one_less"] = (with_block(2, block_image(BASE_BLOCKS[2], c=2)), 2)
    m["block_crc"] = (make_file(data[:offs[2] + 30] + bytes([data[offs[2] + 30] ^ 1]) + data[offs[2] + 31:], base_index), 2)
    m["pad_byte_covered_by_crc_only"] = (with_block(0, stamp_block(imgs[0][:14] + b"\x07" + imgs[0][15:])), "ok")
    m["slack_not_inspected"] = (with_block(1, block_image(e1, fill=0xEE)), "ok")
    # the walk: one block of z = 64 written by hand
    z = 64
    past = varint(3) + b"abc" + varint(z - 5 + 1)            # the value ends one byte behind the body
    m["string_past_body"] = (with_one(past, c=1, z=z, key=b"abc"), 0)
    exact = varint(3) + b"abc" + varint(z - 5)                # ends on the body's end, the sum is off
    m["string_to_body_end_sum_off"] = (with_one(exact, c=1, z=z, key=b"abc"), 0)
    m["entry_varint_5"] = (with_one(varint(3, 4) + b"abc" + varint(z - 11) + b"v" * (z - 11), c=1, z=z, key=b"abc"), 0)
    # entry 1 fills the body up to its last byte, which starts entry 2's key length (0x80: to be continued)
    m["varint_cut_by_body_end"] = (with_one(varint(3) + b"abc" + varint(z - 6) + b"v" * (z - 6) + b"\x80", c=2, z=z, key=b"abc"), 0)
    m["sum_not_z"] = (with_one(entry_bytes(b"abc", b"v" * (z - 12)), c=1, z=z, key=b"abc"), 0)
    m["redundant_varints_ok"] = (with_one(varint(3, 1) + b"abc" + varint(z - 11, 2) + b"v" * (z - 11), c=1, z=z, key=b"abc"), "ok")
    m["empty_key_value_80_00_ok"] = (with_one(varint(0, 1) + varint(0, 1), c=1, z=8, key=b""), "ok")
    # the index entry's key
    m["index_key_longer"] = (with_index(index_image([idx[0], (idx[1][0] + b"s", idx[1][1], idx[1][2]), idx[2]])), 1)
    m["index_key_shorter"] = (with_index(index_image([idx[0], (idx[1][0][:-1], idx[1][1], idx[1][2]), idx[2]])), 1)
    m["index_key_one_byte"] = (with_index(index_image([idx[0], idx[1], (b"cherrz", idx[2][1], idx[2][2])])), 2)
    # two bad blocks: the smaller index is reported
    two = bytearray(data)
    two[offs[2]:offs[2] + len(imgs[2])] = block_image(BASE_BLOCKS[2], c=2)
    two[offs[0] + 40] ^= 0x10
    m["two_bad_blocks"] = (make_file(bytes(two), base_index), 0)
    # layout freedom: out of order, gaps, and the empty table
    gap = b"\xAB" * 5
    d2 = gap + imgs[2] + gap + imgs[0] + imgs[1] + gap
    o2, o0 = 5, 10 + len(imgs[2])
    o1 = o0 + len(imgs[0])
    m["out_of_order_with_gaps_ok"] = (make_file(d2, index_image([(idx[1][0], o1, len(imgs[1])), (idx[2][0], o2, len(imgs[2])),
                                                                   (idx[0][0], o0, len(imgs[0]))])), "ok")
    m["empty_table_ok"] = (make_file(b"", index_image([])), "ok")
    m["empty_table_with_data_ok"] = (make_file(b"junk", index_image([])), "ok")
    return m


def with_one(body, c, z, key, pad=0):
    """A file of one hand-written block with body bytes ``body`` in a body of z bytes."""
    img = block_image([], c=c, z=z, body=body, fill=pad)
    return make_file(img, index_image([(key, 0, len(img))]))


# ---- the C ABI with canaried outputs -------------------------------------------------------------------

CANARY8, CANARY32, CANARY64 = 0xC7, 0xC7C7C7C7, 0xC7C7C7C7C7C7C7C7


class HostOutputs:
    """Canaried numpy outputs of a host scan call sized for n entries, nb blocks, ks / vs arena bytes."""

    def __init__(self, n, nb, ks, vs):
        self.key_off, self.val_off = np.full(n + 1, CANARY64, np.uint64), np.full(n + 1, CANARY64, np.uint64)
        self.key_len, self.val_len = np.full(n + 1, CANARY32, np.uint32), np.full(n + 1, CANARY32, np.uint32)
        self.keys, self.vals = np.full(ks + 16, CANARY8, np.uint8), np.full(vs + 16, CANARY8, np.uint8)
        self.block_off = np.full(nb + 1, CANARY64, np.uint64)
        self.block_size, self.block_first = np.full(nb + 1, CANARY32, np.uint32), np.full(nb + 1, CANARY32, np.uint32)
        self.caps = (n, nb, ks, vs)

    def arrays(self):
        return (self.key_off, self.key_len, self.val_off, self.val_len, self.keys, self.vals, self.block_off,
                self.block_size, self.block_first)

    def untouched(self):
        cans = (CANARY64, CANARY32, CANARY64, CANARY32, CANARY8, CANARY8, CANARY64, CANARY32, CANARY32)
        return all(bool((a == c).all()) for a, c in zip(self.arrays(), cans))


def call_scan(lib, fn_name, file_bytes, flags=0, out=None, caps=None, tail=()):
    """Call tkv_sst_scan / tkv_debug_sst_scan_parse on host bytes. Returns (rc, (n_entries, n_blocks,
    keys_size, vals_size, bad_block)). out = None: every array NULL and every cap 0 (the sizing call)."""
    buf = np.frombuffer(bytes(file_bytes), np.uint8).copy()  # exactly the file's size
    res = [ctypes.c_uint64(0x5EED) for _ in range(5)]
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    fp = p(buf) if buf.size else None
    if out is None:
        args = [None, None, None, None, 0, None, 0, None, 0, None, None, None, 0]
    else:
        n, nb, ks, vs = out.caps if caps is None else caps
        args = [p(out.key_off), p(out.key_len), p(out.val_off), p(out.val_len), n, p(out.keys), ks, p(out.vals), vs,
                p(out.block_off), p(out.block_size), p(out.block_first), nb]
    rc = getattr(lib, fn_name)(fp, buf.size, flags, *args, *[ctypes.byref(r) for r in res], *tail)
    return rc, tuple(r.value for r in res)


def columns_entries(file_bytes, out, n, flags=0):
    """[(key, value)] from the columns of a finished call."""
    src_k = bytes(file_bytes) if flags & KEY_VIEWS else out.keys.tobytes()
    src_v = bytes(file_bytes) if flags & VAL_VIEWS else out.vals.tobytes()
    return [(src_k[int(out.key_off[i]):int(out.key_off[i]) + int(out.key_len[i])],
             src_v[int(out.val_off[i]):int(out.val_off[i]) + int(out.val_len[i])]) for i in range(n)]
