"""SSTable data-block stamping and verification on the GPU CRC engine.

The reference leaves the checksum fields dead: get_data_block writes
``sstable_data_block_header::crc32_ = 0`` (/root/reference/src/storage/sstable_writer.cpp:138-144)
and read_data_block never checks it (sstable_reader.cpp:61-89). The format here is this library's
decision (include/tkv_crc32.h, "parity unpinned"): a data-block image, as get_data_block builds it
(sstable_writer.cpp:150-168), is

    varint(20) | header[20] | varint(n) | body[n] | padding up to 36 + n bytes

with header = u32 entry_count | u32 uncompressed_size | u32 compressed_size | u8 compression |
3 pad | u32 crc32_ (sstable_format.hpp:91-99), so crc32_ sits at image byte CRC_OFFSET = 17. The
stamp is crc32 over the whole image with those 4 bytes read as zero, stored little-endian.
"""
import ctypes
import struct

import numpy as np

from ._lib import CORRUPTED, OK, check, load_library

CRC_OFFSET = 17   # 1-byte varint(20) + 16 header bytes before crc32_
MIN_IMAGE = 22    # varint(20) + header + varint(0)


def _varint(v):
    """codec::encode_varint (core/serialization/codec.hpp:31-39): LEB128."""
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def encode_data_block_image(entries):
    """Unstamped image of a data block holding ``entries`` [(ikey, value), ...], laid out as
    sstable_writer::get_data_block does: the body is write_string(ikey) | write_string(value) per
    entry (sstable_writer.cpp:113) and the block size counts 4 + |ikey| + 4 + |value| per entry
    (:60,122); the reference leaves arena bytes in the slack past the written entries and in the
    image padding, which are zero here."""
    body = b"".join(_varint(len(k)) + k + _varint(len(v)) + v for k, v in entries)
    size = sum(8 + len(k) + len(v) for k, v in entries)
    body = body[:size].ljust(size, b"\0")
    header = struct.pack("<IIIB3xI", len(entries), size, size, 0, 0)
    image = _varint(len(header)) + header + _varint(size) + body
    return image.ljust(8 + len(header) + 8 + size, b"\0")


def _host_arrays(offsets, sizes):
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    sz = np.ascontiguousarray(sizes, dtype=np.uint64)
    if off.size != sz.size:
        raise ValueError("offsets and sizes differ in length")
    return off, sz


def stamp_blocks(file, offsets, sizes):
    """Stamp images in place in a writable uint8 numpy buffer (the SSTable file being written)."""
    if not isinstance(file, np.ndarray) or file.dtype != np.uint8 or not file.flags.writeable:
        raise ValueError("file must be a writable uint8 numpy array")
    off, sz = _host_arrays(offsets, sizes)
    check(load_library().tkv_sst_stamp_blocks(ctypes.c_void_p(file.ctypes.data), ctypes.c_void_p(off.ctypes.data),
                                              ctypes.c_void_p(sz.ctypes.data), off.size))


def verify_blocks(file, offsets, sizes):
    """Verify images of a host buffer. Returns (status, n_bad, first_bad); status "ok" or "corrupted"."""
    buf = np.ascontiguousarray(np.frombuffer(file, np.uint8) if not isinstance(file, np.ndarray) else file)
    off, sz = _host_arrays(offsets, sizes)
    n_bad, first = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = load_library().tkv_sst_verify_blocks(ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(off.ctypes.data),
                                              ctypes.c_void_p(sz.ctypes.data), off.size, ctypes.byref(n_bad),
                                              ctypes.byref(first))
    if rc not in (OK, CORRUPTED):
        check(rc)
    return ("ok" if rc == OK else "corrupted"), n_bad.value, first.value


def block_crcs_device(file, offsets, sizes, store=False, out=None, stream=None):
    """Device-resident images (torch uint8 CUDA tensor, int64 offsets, int32 sizes): the stamp value
    of every image (its CRC with the field read as zero); store=True also writes it into the field."""
    import torch
    from .crc32 import _check_data, _check_vec, _launch_stream, _out_vec
    n = offsets.numel()
    if sizes.numel() != n:
        raise ValueError("offsets and sizes differ in length")
    if file.dtype != torch.uint8:
        raise ValueError("file must be a uint8 tensor")
    _check_data(file)
    for name, t, dt in (("offsets", offsets, torch.int64), ("sizes", sizes, torch.int32)):
        _check_vec(name, t, dt, n, file.device)
    out = _out_vec(out, n, file.device, stream)
    check(load_library().tkv_sst_block_crcs_device(
        ctypes.c_void_p(file.data_ptr()), ctypes.c_void_p(offsets.data_ptr()), ctypes.c_void_p(sizes.data_ptr()),
        ctypes.c_void_p(out.data_ptr()), n, int(bool(store)), _launch_stream(stream, file.device)))
    return out


# ---- index image + footer (include/tkv_crc32.h "SSTable index image + footer stamping") ----------
FOOTER_SIZE = 20      # sizeof(sstable_footer) (sstable_format.hpp:129-135)
FOOTER_CRC_OFFSET = 16


def encode_index_image(entries):
    """Index image as sstable_writer::get_index lays it out: u64 entry count, then per entry
    write_string(smallest_key) | u64 data_block_offset | u64 data_block_size (write_string is
    varint length + bytes, buffer_writer.hpp:75-77). ``entries`` is [(smallest_key, offset, size)]."""
    out = bytearray(struct.pack("<Q", len(entries)))
    for key, off, size in entries:
        out += _varint(len(key)) + key + struct.pack("<QQ", off, size)
    return bytes(out)


def encode_footer(index_offset, index_size, bloom_offset=0, bloom_size=0):
    """Unstamped 20-byte footer in sstable_footer declaration order (crc32_ = 0)."""
    return struct.pack("<IIIII", index_offset, index_size, bloom_offset, bloom_size, 0)


def _index_ptr(index_image):
    buf = np.ascontiguousarray(np.frombuffer(index_image, np.uint8) if not isinstance(index_image, np.ndarray)
                               else index_image)
    return buf, buf.size


def stamp_footer(index_image, footer):
    """Stamped copy of ``footer`` (20 bytes): crc32_ = CRC-32 of index image || footer[0:16]."""
    if len(footer) != FOOTER_SIZE:
        raise ValueError("footer must be 20 bytes")
    idx, n = _index_ptr(index_image)
    f = (ctypes.c_uint8 * FOOTER_SIZE).from_buffer_copy(bytes(footer))
    check(load_library().tkv_sst_stamp_footer(ctypes.c_void_p(idx.ctypes.data if n else 0), n, f))
    return bytes(f)


def verify_footer(index_image, footer):
    """"ok" when the footer's crc32_ matches the index image and its own fields, else "corrupted"."""
    if len(footer) != FOOTER_SIZE:
        raise ValueError("footer must be 20 bytes")
    idx, n = _index_ptr(index_image)
    f = (ctypes.c_uint8 * FOOTER_SIZE).from_buffer_copy(bytes(footer))
    rc = load_library().tkv_sst_verify_footer(ctypes.c_void_p(idx.ctypes.data if n else 0), n, f)
    if rc not in (OK, CORRUPTED):
        check(rc)
    return "ok" if rc == OK else "corrupted"


# ---- flush: data blocks, index and footer in one call (include/tkv_crc32.h "SSTable flush") ---------
class BuiltTable:
    """What build_device / build return: ``file`` (the file image, ``size`` bytes), the data blocks'
    ``block_off`` / ``block_size`` / ``block_first`` (offset, image size and first entry of every block)
    and where the index lies."""

    __slots__ = ("file", "size", "block_off", "block_size", "block_first", "index_offset", "index_size")

    def __init__(self, file, size, block_off, block_size, block_first, index_offset, index_size):
        self.file, self.size = file, size
        self.block_off, self.block_size, self.block_first = block_off, block_size, block_first
        self.index_offset, self.index_size = index_offset, index_size

    @property
    def n_blocks(self):
        return len(self.block_off)


def build_device(keys, key_off, key_len, vals=None, val_off=None, val_len=None, target_block_size=4096, out=None,
                 stream=None):
    """The writer loop for entries held on the device (tkv_sst_build_device): ``keys`` / ``vals`` uint8
    CUDA arenas, ``key_off`` / ``val_off`` int64 and ``key_len`` / ``val_len`` int32 (u32 values) CUDA
    tensors with one entry per element, the dtypes wal.decode_device returns. Entries are written in the
    order given (the caller sorts and builds the internal keys). Makes the sizing call, then the build
    into ``out[:size]`` (a uint8 CUDA tensor of any alignment; allocated when not given). Returns a
    BuiltTable of CUDA tensors: file uint8, block_off int64, block_size / block_first int32 (u32 values).
    An ``out`` that is too small raises with the size needed. Synchronous on ``stream``."""
    import torch
    from ._lib import BUFFER_OVERFLOW
    from .crc32 import _check_data, _check_vec, _launch_stream
    if keys.dtype != torch.uint8:
        raise ValueError("keys must be a uint8 tensor")
    _check_data(keys)
    dev = keys.device
    n = key_len.numel()
    _check_vec("key_off", key_off, torch.int64, n, dev)
    _check_vec("key_len", key_len, torch.int32, n, dev)
    if val_len is not None:
        if vals is None or val_off is None:
            raise ValueError("val_len needs vals and val_off")
        _check_vec("vals", vals, torch.uint8, 0, dev)
        _check_vec("val_off", val_off, torch.int64, n, dev)
        _check_vec("val_len", val_len, torch.int32, n, dev)
    other = stream is not None and stream != torch.cuda.current_stream(dev)

    def alloc(count, dtype):
        t = torch.empty(count, dtype=dtype, device=dev)
        if other:
            t.record_stream(stream)
        return t

    def ptr(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())
    # An arena without a byte has no address (data_ptr() of an empty tensor is 0), and the call requires one
    # for keys, and for vals beside val_len: a batch whose values are all empty, decoded into a copied arena
    # and replayed, arrives here like that. A spare byte stands in (uninitialised, alive until this function
    # returns, which is after the stream's end): every sound span into an arena without a byte is empty, so the
    # byte is never read. The call takes no arena sizes, so a key_len or val_len above 0 beside an empty arena
    # is the caller's error here as it is beside any arena that is too short; it used to be refused as a null
    # pointer and would now read that byte.
    if keys.numel() == 0:
        keys = alloc(1, torch.uint8)
    if val_len is not None and vals.numel() == 0:
        vals = alloc(1, torch.uint8)
    lib = load_library()
    st = _launch_stream(stream, dev)
    sizes = [ctypes.c_uint64(0) for _ in range(4)]  # file_size, n_blocks, index_offset, index_size

    def call(file, cap, boff, bsize, bfirst, bcap):
        return lib.tkv_sst_build_device(ptr(keys), ptr(key_off), ptr(key_len), ptr(vals) if val_len is not None else None,
                                        ptr(val_off) if val_len is not None else None, ptr(val_len), n,
                                        int(target_block_size), file, cap, boff, bsize, bfirst, bcap,
                                        *[ctypes.byref(s) for s in sizes], st)
    rc = call(None, 0, None, None, None, 0)  # the sizing call
    if rc not in (OK, BUFFER_OVERFLOW):
        check(rc)
    size, nb = sizes[0].value, sizes[1].value
    if out is None:
        out = alloc(size, torch.uint8)
    _check_vec("out", out, torch.uint8, 0, dev)
    if out.numel() < size:
        raise ValueError(f"out holds {out.numel()} bytes, the file needs {size}")
    boff, bsize, bfirst = alloc(nb, torch.int64), alloc(nb, torch.int32), alloc(nb, torch.int32)
    check(call(ptr(out), out.numel(), ptr(boff), ptr(bsize), ptr(bfirst), nb))
    return BuiltTable(out[:size], size, boff, bsize, bfirst, sizes[2].value, sizes[3].value)


def build(entries, target_block_size=4096):
    """The same on the host (tkv_sst_build): ``entries`` is [(ikey, value), ...] or a tuple of numpy arrays
    (keys uint8, key_off uint64, key_len uint32, vals uint8, val_off uint64, val_len uint32). The cut and
    the layout run on host threads, the stamps on the GPU. Returns a BuiltTable of numpy arrays (file
    uint8, block_off uint64, block_size / block_first uint32)."""
    from ._lib import BUFFER_OVERFLOW
    if isinstance(entries, tuple):
        keys, koff, klen, vals, voff, vlen = entries
        keys, vals = (np.ascontiguousarray(a, dtype=np.uint8) for a in (keys, vals))
        koff, voff = (np.ascontiguousarray(a, dtype=np.uint64) for a in (koff, voff))
        klen, vlen = (np.ascontiguousarray(a, dtype=np.uint32) for a in (klen, vlen))
    else:
        from .wal import _arena
        keys, koff, klen = _arena([k for k, _ in entries])
        vals, voff, vlen = _arena([v for _, v in entries])
    n = klen.size
    lib = load_library()
    sizes = [ctypes.c_uint64(0) for _ in range(4)]

    def ptr(a):
        return None if a is None else ctypes.c_void_p(a.ctypes.data)

    def call(file, cap, boff, bsize, bfirst, bcap):
        return lib.tkv_sst_build(ptr(keys), ptr(koff), ptr(klen), ptr(vals), ptr(voff), ptr(vlen), n,
                                 int(target_block_size), ptr(file), cap, ptr(boff), ptr(bsize), ptr(bfirst), bcap,
                                 *[ctypes.byref(s) for s in sizes])
    rc = call(None, 0, None, None, None, 0)  # the sizing call
    if rc not in (OK, BUFFER_OVERFLOW):
        check(rc)
    size, nb = sizes[0].value, sizes[1].value
    file = np.empty(size, np.uint8)
    boff, bsize, bfirst = np.empty(nb, np.uint64), np.empty(nb, np.uint32), np.empty(nb, np.uint32)
    check(call(file, size, boff, bsize, bfirst, nb))
    return BuiltTable(file, size, boff, bsize, bfirst, sizes[2].value, sizes[3].value)


def _read_varint(buf, pos):
    v = shift = 0
    while True:
        if pos >= len(buf) or shift > 63:
            raise ValueError("truncated varint in the index image")
        b = buf[pos]
        pos += 1
        v |= (b & 0x7F) << shift
        shift += 7
        if b < 0x80:
            return v, pos


def read_index(file):
    """Open a built file again (pure Python, no GPU): parse the footer at the file's end, check its
    crc32_ over index image || footer[0:16] and the index's framing, and return
    [(smallest_key, offset, size)], the input of verify_blocks. Raises ValueError when the footer, its
    checksum or the index does not hold."""
    import zlib
    buf = bytes(file.tobytes() if isinstance(file, np.ndarray) else file)
    if len(buf) < FOOTER_SIZE + 8:
        raise ValueError("file shorter than an index and a footer")
    ioff, isz, _, _, crc = struct.unpack("<IIIII", buf[-FOOTER_SIZE:])
    if ioff + isz + FOOTER_SIZE != len(buf) or isz < 8:
        raise ValueError("footer does not describe this file")
    if zlib.crc32(buf[ioff:ioff + isz + FOOTER_CRC_OFFSET]) != crc:
        raise ValueError("corrupted SSTable index or footer")
    idx = buf[ioff:ioff + isz]
    (count,) = struct.unpack_from("<Q", idx, 0)
    pos, out = 8, []
    for _ in range(count):
        kl, pos = _read_varint(idx, pos)
        if pos + kl + 16 > len(idx):
            raise ValueError("index entry reaches past the index image")
        key = idx[pos:pos + kl]
        off, size = struct.unpack_from("<QQ", idx, pos + kl)
        if off + size > ioff:
            raise ValueError("index entry reaches past the data blocks")
        out.append((key, off, size))
        pos += kl + 16
    if pos != len(idx):
        raise ValueError("bytes left behind the last index entry")
    return out


# ---- scan: verify, index and entries of a file image (include/tkv_crc32.h "SSTable scan") ------------
SCAN_KEY_VIEWS = 1
SCAN_VAL_VIEWS = 2
BAD_FOOTER = 2**64 - 1
BAD_INDEX = 2**64 - 2


class SstCorrupted(ValueError):
    """A file the scan rejects. ``bad_block`` is "footer", "index" or the number of the first bad block."""

    def __init__(self, bad_block, msg):
        self.bad_block = {BAD_FOOTER: "footer", BAD_INDEX: "index"}.get(bad_block, bad_block)
        super().__init__(f"corrupted SSTable ({self.bad_block}): {msg}")


class ScannedTable:
    """What scan_device / scan return: the entries as ``keys`` / ``key_off`` / ``key_len`` and ``vals`` /
    ``val_off`` / ``val_len`` (the columns build_device takes; with a views flag the arena is the file
    image itself) and the data blocks' ``block_off`` / ``block_size`` / ``block_first``."""

    __slots__ = ("keys", "key_off", "key_len", "vals", "val_off", "val_len", "block_off", "block_size", "block_first",
                 "n_entries", "n_blocks")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    def entries(self):
        """[(key, value)] as bytes (tests and small tables)."""
        def host(t):
            return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
        keys, vals = host(self.keys).view(np.uint8).tobytes(), host(self.vals).view(np.uint8).tobytes()
        ko, vo = host(self.key_off).view(np.uint64), host(self.val_off).view(np.uint64)
        kl, vl = host(self.key_len).view(np.uint32), host(self.val_len).view(np.uint32)
        return [(keys[int(ko[i]):int(ko[i]) + int(kl[i])], vals[int(vo[i]):int(vo[i]) + int(vl[i])])
                for i in range(self.n_entries)]


def _scan(fn, file_ptr, size, flags, alloc, ptr, file_arena, tail):
    """The sizing call, then the scan into freshly allocated arrays. ``alloc(count, kind)`` makes an array
    (kind "u8" / "u64" / "u32"), ``ptr`` its address, ``tail`` the trailing arguments (the stream)."""
    from ._lib import BUFFER_OVERFLOW
    out = [ctypes.c_uint64(0) for _ in range(5)]  # n_entries, n_blocks, keys_size, vals_size, bad_block
    refs = [ctypes.byref(s) for s in out]

    def done(rc):
        if rc == CORRUPTED:
            raise SstCorrupted(out[4].value, load_library().tkv_last_error().decode(errors="replace"))
        return rc
    rc = done(fn(file_ptr, size, flags, None, None, None, None, 0, None, 0, None, 0, None, None, None, 0, *refs, *tail))
    if rc not in (OK, BUFFER_OVERFLOW):
        check(rc)
    n, nb, ks, vs = (s.value for s in out[:4])
    kviews, vviews = bool(flags & SCAN_KEY_VIEWS), bool(flags & SCAN_VAL_VIEWS)
    koff, klen, voff, vlen = alloc(n, "u64"), alloc(n, "u32"), alloc(n, "u64"), alloc(n, "u32")
    keys = file_arena if kviews else alloc(ks, "u8")
    vals = file_arena if vviews else alloc(vs, "u8")
    boff, bsize, bfirst = alloc(nb, "u64"), alloc(nb, "u32"), alloc(nb, "u32")
    check(done(fn(file_ptr, size, flags, ptr(koff), ptr(klen), ptr(voff), ptr(vlen), n,
                  None if kviews else ptr(keys), ks, None if vviews else ptr(vals), vs,
                  ptr(boff), ptr(bsize), ptr(bfirst), nb, *refs, *tail)))
    return ScannedTable(keys=keys, key_off=koff, key_len=klen, vals=vals, val_off=voff, val_len=vlen, block_off=boff,
                        block_size=bsize, block_first=bfirst, n_entries=n, n_blocks=nb)


def scan_device(file, key_views=False, val_views=False, stream=None):
    """Verify a file image held on the device (a uint8 CUDA tensor of any alignment) and take it apart
    (tkv_sst_scan_device): makes the sizing call, then the scan. Returns a ScannedTable of CUDA tensors in
    the dtypes build_device takes: keys / vals uint8, key_off / val_off / block_off int64, key_len /
    val_len / block_size / block_first int32 (u32 values). With ``key_views`` / ``val_views`` nothing is
    copied for that arena: ``keys`` / ``vals`` is ``file`` and the offsets point into it. A corrupted file
    raises SstCorrupted. Synchronous on ``stream``."""
    import torch
    from .crc32 import _launch_stream
    if not isinstance(file, torch.Tensor) or file.dtype != torch.uint8 or not file.is_cuda or file.dim() != 1 or \
            not file.is_contiguous():
        raise ValueError("file must be a contiguous 1-D uint8 CUDA tensor")
    dev = file.device
    other = stream is not None and stream != torch.cuda.current_stream(dev)
    kinds = {"u8": torch.uint8, "u64": torch.int64, "u32": torch.int32}

    def alloc(count, kind):
        # (an arena without a byte is returned as one spare byte: it still has an address, which
        # build_device requires)
        t = torch.empty(max(count, 1), dtype=kinds[kind], device=dev)
        if count or kind != "u8":
            t = t[:count]
        if other:
            t.record_stream(stream)
        return t
    flags = (SCAN_KEY_VIEWS if key_views else 0) | (SCAN_VAL_VIEWS if val_views else 0)
    return _scan(load_library().tkv_sst_scan_device, ctypes.c_void_p(file.data_ptr()) if file.numel() else None,
                 file.numel(), flags, alloc, lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None, file,
                 (_launch_stream(stream, dev),))


def scan(file, key_views=False, val_views=False):
    """The same on the host (tkv_sst_scan): ``file`` is bytes or a uint8 numpy array; the parse and the
    copies run on host threads, the checksums on the GPU. Returns a ScannedTable of numpy arrays (uint8,
    uint64 offsets, uint32 lengths)."""
    if isinstance(file, np.ndarray):
        if file.dtype != np.uint8 or file.ndim != 1:
            raise ValueError("file must be a 1-D uint8 numpy array")
        buf = np.ascontiguousarray(file)
    else:
        buf = np.frombuffer(bytes(file), np.uint8)
    kinds = {"u8": np.uint8, "u64": np.uint64, "u32": np.uint32}
    flags = (SCAN_KEY_VIEWS if key_views else 0) | (SCAN_VAL_VIEWS if val_views else 0)
    return _scan(load_library().tkv_sst_scan, ctypes.c_void_p(buf.ctypes.data) if buf.size else None, buf.size, flags,
                 lambda count, kind: np.empty(count, kinds[kind]),
                 lambda a: ctypes.c_void_p(a.ctypes.data) if a.size else None, buf, ())


# ---- merge: k-way merge of sorted runs, newest wins (include/tkv_crc32.h "SSTable merge") -------------
MERGE_DROP_TOMBSTONES = 1
MERGE_MAX_RUNS = 64
MERGE_NONE = 2**64 - 1


class MergeCorrupted(ValueError):
    """A run the merge rejects: entry ``index`` of run ``run`` has a key span that does not hold (shorter
    than the 17 metadata bytes, 2^28 bytes or more, past its arena) or a user key below the one in front of it."""

    def __init__(self, run, index):
        self.run, self.index = run, index
        super().__init__(f"entry {index} of run {run} has a bad key span or is out of order")


class MergedRun:
    """What merge_device / merge return: one entry per surviving user key, ascending. ``key_off`` /
    ``val_off`` count from the addresses ``key_base`` / ``val_base`` (the lowest key / value arena among the
    runs; ``keys`` / ``vals`` are those arenas), ``key_len`` / ``val_len`` are the entries' own, ``src`` =
    run << 32 | index names the surviving entry. ``arenas`` keeps every input arena alive; ``key_arenas`` /
    ``val_arenas`` are its two kinds (the bounds of the offsets for a later get)."""

    __slots__ = ("keys", "vals", "key_base", "val_base", "key_off", "key_len", "val_off", "val_len", "src", "n_entries",
                 "keys_bytes", "vals_bytes", "arenas", "key_arenas", "val_arenas")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    def entries(self):
        """[(ikey, value)] as bytes, read through the bases and offsets as the flush reads them (tests and
        small runs)."""
        def host(t):
            return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)

        def addr(t):
            return t.data_ptr() if hasattr(t, "data_ptr") else t.ctypes.data
        held = [(addr(t), host(t).view(np.uint8).tobytes()) for t in self.arenas]

        def read(at, ln):
            if ln == 0:
                return b""
            for base, raw in held:
                if base <= at and at + ln <= base + len(raw):
                    return raw[at - base:at - base + ln]
            raise ValueError("a span lies in no input arena")
        ko, vo = host(self.key_off).view(np.uint64), host(self.val_off).view(np.uint64)
        kl, vl = host(self.key_len).view(np.uint32), host(self.val_len).view(np.uint32)
        return [(read(self.key_base + int(ko[j]), int(kl[j])), read(self.val_base + int(vo[j]), int(vl[j])))
                for j in range(self.n_entries)]

    def flush(self, target_block_size=4096, out=None, stream=None):
        """The run as an SSTable file image: build_device straight through the two bases for a device run;
        a host run gathers its entries first (build takes one arena of each kind). A run without an entry
        (every survivor a dropped tombstone) raises: the flush refuses an empty table."""
        if self.n_entries == 0:
            raise ValueError("nothing survives the merge: an SSTable holds at least one entry")
        if isinstance(self.key_off, np.ndarray):
            return build(self.entries(), target_block_size=target_block_size)
        return build_device(self.keys, self.key_off, self.key_len, self.vals, self.val_off, self.val_len,
                            target_block_size=target_block_size, out=out, stream=stream)


def _run_columns(run):
    """(keys, key_off, key_len, vals, val_off, val_len) of a ScannedTable, a MemtableRun or such a tuple."""
    if isinstance(run, ScannedTable):
        return run.keys, run.key_off, run.key_len, run.vals, run.val_off, run.val_len
    if hasattr(run, "ikeys"):
        return run.ikeys, run.ikey_off, run.ikey_len, run.vals, run.val_off, run.val_len
    keys, key_off, key_len, vals, val_off, val_len = run
    return keys, key_off, key_len, vals, val_off, val_len


def _merge(fn, cols, addr, count, alloc, ptr, drop_tombstones, tail, spare):
    """The sizing call, then the merge into freshly allocated columns. ``addr(t)`` / ``count(t)`` give an
    array's address and element count, ``alloc(count, kind)`` makes one, ``ptr`` its address or None,
    ``spare()`` a one-byte arena for a merge without a value arena."""
    from ._lib import BUFFER_OVERFLOW
    K = len(cols)
    if K > MERGE_MAX_RUNS:
        raise ValueError(f"{K} runs: a merge takes at most {MERGE_MAX_RUNS}")
    n = [count(c[2]) for c in cols]

    def has(t):
        return t is not None and count(t) > 0
    key_arenas = [c[0] for c, k in zip(cols, n) if k and has(c[0])]
    val_arenas = [c[3] for c, k in zip(cols, n) if k and has(c[3])]
    keys = min(key_arenas, key=addr) if key_arenas else None
    vals = min(val_arenas, key=addr) if val_arenas else spare()
    key_base, val_base = addr(keys) if keys is not None else 0, addr(vals)

    def table(ctype, values):
        return (ctype * max(K, 1))(*values)
    vp = ctypes.c_void_p
    a_keys = table(vp, [addr(c[0]) if has(c[0]) else None for c in cols])
    a_size = table(ctypes.c_uint64, [count(c[0]) if c[0] is not None else 0 for c in cols])
    a_koff = table(vp, [addr(c[1]) if has(c[1]) else None for c in cols])
    a_klen = table(vp, [addr(c[2]) if has(c[2]) else None for c in cols])
    a_voff = table(vp, [addr(c[4]) if has(c[4]) and has(c[5]) else None for c in cols])
    a_vlen = table(vp, [addr(c[5]) if has(c[4]) and has(c[5]) else None for c in cols])
    a_n = table(ctypes.c_uint64, n)
    a_bias = table(ctypes.c_uint64, [addr(c[3]) - val_base if k and has(c[3]) else 0 for c, k in zip(cols, n)])
    res = [ctypes.c_uint64(0) for _ in range(4)]  # n_entries, keys_bytes, vals_bytes, first_bad
    flags = MERGE_DROP_TOMBSTONES if drop_tombstones else 0

    def call(out, cap):
        rc = fn(K, a_keys, a_size, a_koff, a_klen, a_voff, a_vlen, a_n, vp(key_base) if key_base else None, a_bias, flags,
                *[ptr(t) for t in out], cap, *[ctypes.byref(r) for r in res], *tail)
        if rc == CORRUPTED:
            raise MergeCorrupted(res[3].value >> 32, res[3].value & 0xFFFFFFFF)
        return rc
    rc = call([None] * 5, 0)  # the sizing call
    if rc not in (OK, BUFFER_OVERFLOW):
        check(rc)
    m = res[0].value
    out = [alloc(m, k) for k in ("u64", "u32", "u64", "u32", "u64")]  # key_off, key_len, val_off, val_len, src
    if m:
        check(call(out, m))
    return MergedRun(keys=keys, vals=vals, key_base=key_base, val_base=val_base, key_off=out[0], key_len=out[1],
                     val_off=out[2], val_len=out[3], src=out[4], n_entries=m, keys_bytes=res[1].value,
                     vals_bytes=res[2].value,
                     arenas=[t for c in cols for t in (c[0], c[3]) if has(t)], key_arenas=key_arenas, val_arenas=val_arenas)


def merge_device(runs, drop_tombstones=False, stream=None):
    """The k-way merge of sorted runs held on the device (tkv_sst_merge_device). ``runs`` is a list, OLDEST
    FIRST, of ScannedTables scanned with both view flags, of MemtableRuns, or of (keys, key_off, key_len,
    vals, val_off, val_len) tuples of CUDA tensors (uint8 arenas, int64 offsets, int32 lengths; vals,
    val_off and val_len may be None). Of all entries with one user key the one from the last run survives;
    ``drop_tombstones`` leaves surviving tombstones out (the last level only). Picks the lowest arena
    addresses as the bases, makes the sizing call, then the merge. Returns a MergedRun of CUDA tensors
    (key_off / val_off / src int64, key_len / val_len int32, u32 / u64 values). A bad run raises
    MergeCorrupted. Synchronous on ``stream``."""
    import torch
    from .crc32 import _check_data, _check_vec, _launch_stream
    cols = [_run_columns(r) for r in runs]
    dev = next((c[2].device for c in cols), torch.device("cuda", torch.cuda.current_device()))
    for keys, key_off, key_len, vals, val_off, val_len in cols:
        n = key_len.numel()
        if keys.dtype != torch.uint8:
            raise ValueError("keys must be a uint8 tensor")
        _check_data(keys)
        _check_vec("key_off", key_off, torch.int64, n, dev)
        _check_vec("key_len", key_len, torch.int32, n, dev)
        if val_len is not None:
            if val_off is None:
                raise ValueError("val_len needs val_off")
            _check_vec("val_off", val_off, torch.int64, n, dev)
            _check_vec("val_len", val_len, torch.int32, n, dev)
        if vals is not None:
            _check_vec("vals", vals, torch.uint8, 0, dev)
    other = stream is not None and stream != torch.cuda.current_stream(dev)
    kinds = {"u8": torch.uint8, "u64": torch.int64, "u32": torch.int32}

    def alloc(count, kind):
        t = torch.empty(count, dtype=kinds[kind], device=dev)
        if other:
            t.record_stream(stream)
        return t
    return _merge(load_library().tkv_sst_merge_device, cols, lambda t: t.data_ptr(), lambda t: t.numel(), alloc,
                  lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None, drop_tombstones,
                  (_launch_stream(stream, dev),), lambda: alloc(1, "u8"))


def merge(runs, drop_tombstones=False):
    """The same on the host (tkv_sst_merge: host threads, no GPU): runs of numpy arrays (uint8 arenas,
    uint64 offsets, uint32 lengths). Returns a MergedRun of numpy arrays."""
    cols = []
    for run in runs:
        keys, key_off, key_len, vals, val_off, val_len = _run_columns(run)

        def arr(a, dt):
            return None if a is None else np.ascontiguousarray(a, dtype=dt)
        cols.append((arr(keys, np.uint8), arr(key_off, np.uint64), arr(key_len, np.uint32), arr(vals, np.uint8),
                     arr(val_off, np.uint64), arr(val_len, np.uint32)))
    kinds = {"u8": np.uint8, "u64": np.uint64, "u32": np.uint32}
    return _merge(load_library().tkv_sst_merge, cols, lambda a: a.ctypes.data, lambda a: a.size,
                  lambda count, kind: np.empty(count, kinds[kind]),
                  lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else None, drop_tombstones, (),
                  lambda: np.zeros(1, np.uint8))


def compact_device(files, target_block_size=4096, drop_tombstones=False, stream=None):
    """Compaction on the device: scan_device of every file image (OLDEST FIRST, both arenas as views),
    merge_device, and the flush of the merged run. Returns the BuiltTable of the new file. Only a compaction
    into the last level may drop tombstones; one that leaves no entry raises ValueError."""
    runs = [scan_device(f, key_views=True, val_views=True, stream=stream) for f in files]
    return merge_device(runs, drop_tombstones=drop_tombstones, stream=stream).flush(target_block_size, stream=stream)


def compact(files, target_block_size=4096, drop_tombstones=False):
    """The same through the host calls (scan, merge, build)."""
    runs = [scan(f, key_views=True, val_views=True) for f in files]
    return merge(runs, drop_tombstones=drop_tombstones).flush(target_block_size)


# ---- get: batched point lookup over sorted runs, newest wins (include/tkv_crc32.h "SSTable get") ------
GET_ABSENT, GET_FOUND, GET_DELETED = 0, 1, 2


class GetCorrupted(ValueError):
    """A run the get rejects: entry ``index`` of run ``run`` was read by a search and its key span (or, as a
    hit, its value span) does not hold."""

    def __init__(self, run, index):
        self.run, self.index = run, index
        super().__init__(f"entry {index} of run {run} has a bad key or value span")


class GetResult:
    """What get_device / get return, one element per query: ``state`` (GET_ABSENT / GET_FOUND /
    GET_DELETED), ``src`` = run << 32 | index of the hit (MERGE_NONE when absent), ``seq`` the hit's
    sequence, ``val_off`` / ``val_len`` the value span of a found key (``val_off`` counts from the lowest
    value arena among the runs), and with values ``val_pos`` / ``vals``: the found values back to back in
    query order, value j at ``vals[val_pos[j]:val_pos[j] + val_len[j]]``. ``n_found`` and ``vals_bytes``
    are the totals."""

    __slots__ = ("state", "src", "seq", "val_off", "val_len", "val_pos", "vals", "n_found", "vals_bytes")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    def items(self):
        """(state, value-or-None) per query; the value as bytes for a found key when values were gathered."""
        def host(t, dt):
            return None if t is None else (t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)).view(dt)
        state, vl = host(self.state, np.uint8), host(self.val_len, np.uint32)
        pos, raw = host(self.val_pos, np.uint64), host(self.vals, np.uint8)
        raw = None if raw is None else raw.tobytes()
        for j in range(state.size):
            found = int(state[j]) == GET_FOUND and raw is not None
            yield int(state[j]), (raw[int(pos[j]):int(pos[j]) + int(vl[j])] if found else None)


def _get_columns(run, addr, count):
    """_run_columns, and also a MergedRun (its offsets count from its bases: the key arena is passed from
    the key base to the end of the highest input key arena, the value arena likewise over the value arenas,
    0 bytes when the merge had none) and a dict with the six column names. Returns (columns, keys_size,
    vals_size)."""
    if isinstance(run, MergedRun):
        keys_end = max([addr(t) + count(t) for t in run.key_arenas], default=run.key_base)
        vals_end = max([addr(t) + count(t) for t in run.val_arenas], default=run.val_base)
        return (run.keys, run.key_off, run.key_len, run.vals, run.val_off, run.val_len), max(keys_end - run.key_base, 0), \
            max(vals_end - run.val_base, 0)
    if isinstance(run, dict):
        run = tuple(run.get(k) for k in ("keys", "key_off", "key_len", "vals", "val_off", "val_len"))
    cols = _run_columns(run)
    return cols, (count(cols[0]) if cols[0] is not None else 0), (count(cols[3]) if cols[3] is not None else 0)


def _get(fn, runs, queries, values, addr, count, alloc, ptr, tail):
    """The sizing call, then the get into freshly allocated columns (``addr`` / ``count`` / ``alloc`` /
    ``ptr`` as in _merge). ``queries`` = (arena, off, len)."""
    from ._lib import BUFFER_OVERFLOW
    K = len(runs)
    if K > MERGE_MAX_RUNS:
        raise ValueError(f"{K} runs: a get takes at most {MERGE_MAX_RUNS}")
    got = [_get_columns(r, addr, count) for r in runs]
    cols = [g[0] for g in got]
    n = [count(c[2]) for c in cols]

    def has(t):
        return t is not None and count(t) > 0
    val_arenas = [c[3] for c, k in zip(cols, n) if k and has(c[3])]
    val_base = min(addr(t) for t in val_arenas) if val_arenas else 0

    def table(ctype, vals):
        return (ctype * max(K, 1))(*vals)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    a_keys = table(vp, [addr(c[0]) if has(c[0]) else None for c in cols])
    a_size = table(u64, [g[1] for g in got])
    a_koff = table(vp, [addr(c[1]) if has(c[1]) else None for c in cols])
    a_klen = table(vp, [addr(c[2]) if has(c[2]) else None for c in cols])
    a_voff = table(vp, [addr(c[4]) if has(c[4]) and has(c[5]) else None for c in cols])
    a_vlen = table(vp, [addr(c[5]) if has(c[4]) and has(c[5]) else None for c in cols])
    a_n = table(u64, n)
    a_vals = table(vp, [addr(c[3]) if has(c[3]) else None for c in cols]) if values else None
    a_vsize = table(u64, [g[2] if has(c[3]) else 0 for g, c in zip(got, cols)]) if values else None
    a_bias = table(u64, [addr(c[3]) - val_base if k and has(c[3]) else 0 for c, k in zip(cols, n)])
    qkeys, q_off, q_len = queries
    nq = count(q_len)
    res = [u64(0) for _ in range(3)]  # n_found, vals_bytes, first_bad

    def call(out, cap):
        rc = fn(K, a_keys, a_size, a_koff, a_klen, a_voff, a_vlen, a_n, a_vals, a_vsize, a_bias, ptr(qkeys), count(qkeys),
                ptr(q_off), ptr(q_len), nq, 0, *[ptr(t) for t in out], cap, *[ctypes.byref(r) for r in res], *tail)
        if rc == CORRUPTED:
            raise GetCorrupted(res[2].value >> 32, res[2].value & 0xFFFFFFFF)
        return rc
    rc = call([None] * 7, 0)  # the sizing call
    if rc not in (OK, BUFFER_OVERFLOW):
        check(rc)
    total = res[1].value
    kinds = ("u8", "u64", "u64", "u64", "u32", "u64", "u8")  # state, src, seq, val_off, val_len, val_pos, vals
    out = [alloc(total if k == 6 else nq, kind) if values or k < 5 else None for k, kind in enumerate(kinds)]
    if nq:
        check(call(out, total))
    return GetResult(state=out[0], src=out[1], seq=out[2], val_off=out[3], val_len=out[4], val_pos=out[5], vals=out[6],
                     n_found=res[0].value, vals_bytes=total)


def _query_arena(keys):
    """(arena, off, len) as numpy arrays of a list of bytes."""
    ln = np.array([len(k) for k in keys], np.uint32)
    off = np.zeros(len(keys), np.uint64)
    if len(keys) > 1:
        off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
    return np.frombuffer(b"".join(keys), np.uint8).copy(), off, ln


def get_device(runs, keys, values=True, stream=None):
    """engine::get for a batch on the device (tkv_sst_get_device). ``runs`` is a list, OLDEST FIRST (the
    memtable runs last), of what merge_device takes, of MergedRuns, or of dicts with the column names
    ``keys, key_off, key_len, vals, val_off, val_len``. ``keys`` is a list of ``bytes`` (copied to the device
    once) or an (arena, off, len) triple of CUDA tensors (uint8, int64, int32). For every key the newest run
    that holds it decides: found, deleted (a tombstone) or absent. With ``values`` the found values are
    gathered into one arena. Makes the sizing call, then the get. Returns a GetResult of CUDA tensors. A bad
    entry a search reads raises GetCorrupted. Synchronous on ``stream``."""
    import torch
    from .crc32 import _check_vec, _launch_stream
    dev = torch.device("cuda", torch.cuda.current_device())
    if isinstance(keys, (list, tuple)) and not (len(keys) == 3 and hasattr(keys[0], "data_ptr")):
        a, off, ln = _query_arena(list(keys))
        keys = (torch.from_numpy(a).to(dev), torch.from_numpy(off.view(np.int64)).to(dev), torch.from_numpy(ln.view(np.int32)).to(dev))
    qkeys, q_off, q_len = keys
    nq = q_len.numel()
    _check_vec("keys", qkeys, torch.uint8, 0, q_len.device)
    _check_vec("key offsets", q_off, torch.int64, nq, q_len.device)
    _check_vec("key lengths", q_len, torch.int32, nq, q_len.device)
    dev = q_len.device
    other = stream is not None and stream != torch.cuda.current_stream(dev)
    kinds = {"u8": torch.uint8, "u64": torch.int64, "u32": torch.int32}

    def alloc(count, kind):
        t = torch.empty(count, dtype=kinds[kind], device=dev)
        if other:
            t.record_stream(stream)
        return t
    return _get(load_library().tkv_sst_get_device, runs, (qkeys, q_off, q_len), values, lambda t: t.data_ptr(),
                lambda t: t.numel(), alloc, lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None,
                (_launch_stream(stream, dev),))


def get(runs, keys, values=True):
    """The same on the host (tkv_sst_get: host threads, no GPU): runs of numpy arrays, ``keys`` a list of
    ``bytes`` or an (arena, off, len) triple of arrays. Returns a GetResult of numpy arrays."""
    def arr(a, dt):
        return None if a is None else np.ascontiguousarray(a, dtype=dt)
    dts = (np.uint8, np.uint64, np.uint32, np.uint8, np.uint64, np.uint32)
    host = []
    for run in runs:
        if isinstance(run, MergedRun):
            host.append(run)
            continue
        if isinstance(run, dict):
            run = tuple(run.get(k) for k in ("keys", "key_off", "key_len", "vals", "val_off", "val_len"))
        host.append(tuple(arr(a, dt) for a, dt in zip(_run_columns(run), dts)))
    if isinstance(keys, (list, tuple)) and not (len(keys) == 3 and isinstance(keys[0], np.ndarray)):
        keys = _query_arena(list(keys))
    queries = tuple(arr(a, dt) for a, dt in zip(keys, dts[:3]))
    kinds = {"u8": np.uint8, "u64": np.uint64, "u32": np.uint32}
    return _get(load_library().tkv_sst_get, host, queries, values, lambda a: a.ctypes.data, lambda a: a.size,
                lambda count, kind: np.empty(count, kinds[kind]),
                lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else None, ())
