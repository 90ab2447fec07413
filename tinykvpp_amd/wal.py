"""WAL record stamping and batched verification on the GPU CRC engine.

Mirrors the CRC call sites of frankie::engine::wal_entry (/root/reference/src/engine/wal.cpp):
  * encode (wal.cpp:19-61): record = u32 record_len | u32 crc32 | u8 op | u64 seq | u8 tombstone |
    u32 key_len | u32 value_len | key | value (LE, packed, 26-byte header, wal.hpp:21-27);
    record_len = size - 8; crc32 = crc32{}.update([8, size)).finalize() stored LE at offset 4.
  * decode (wal.cpp:63-130): eof on empty input; corrupted when fewer than 26 bytes remain, when
    record_len + 8 exceeds the input, on a CRC mismatch, or when key/value overflow the record.

Here a whole slurped WAL (wal_reader::open, wal.cpp:204-240) is verified on the GPU: the image is
copied to the device once, the record_len chain is walked there (speculative parallel walk with exact
stitching) and every record's CRC is checked in ONE batch (tkv_wal_verify; tkv_wal_verify_device for
an image already in HBM). Many records are stamped in one batch (tkv_wal_stamp) — the recovery loop
of engine::create (engine.cpp:31-53) and group commit. A whole put batch held as keys, values and
sequence numbers is encoded in one call (tkv_wal_encode: encode_batch; tkv_wal_encode_device for arenas
already in HBM: encode_device), layout and CRCs included. The inverse takes the fields of a list of
records out into that columnar form (tkv_wal_decode_device: decode_device; tkv_wal_decode_host:
decode_batch), and recover_device / recover chain index and decode into what the recovery loop consumes.
"""
import collections
import ctypes
import struct

import numpy as np

from ._lib import CORRUPTED, OK, check, load_library

kMetadataSize = 26  # wal.hpp:21-27
PUT, DEL = 0, 1     # wal_operation (wal.hpp:14-17)


def encode_unstamped(op, seq, key, value, tombstone):
    """Record bytes laid out as wal.cpp:30-52 with the CRC field left zero (wal.cpp:28 memset)."""
    body = struct.pack("<BQBII", op, seq, int(bool(tombstone)), len(key), len(value)) + key + value
    return struct.pack("<II", len(body), 0) + body


def stamp(records):
    """Stamp a list of unstamped records (bytes) in one batch; returns the stamped bytes list."""
    if not records:
        return []
    sizes = np.array([len(r) for r in records], np.uint32)
    offs = np.zeros(len(records), np.uint64)
    offs[1:] = np.cumsum(sizes[:-1], dtype=np.uint64)
    buf = np.frombuffer(b"".join(records), np.uint8).copy()
    check(load_library().tkv_wal_stamp(ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(offs.ctypes.data),
                                       ctypes.c_void_p(sizes.ctypes.data), len(records)))
    raw = buf.tobytes()
    return [raw[int(o):int(o) + int(s)] for o, s in zip(offs, sizes)]


def encode(op, seq, key, value, tombstone):
    """wal_entry::encode: one stamped record (uses the batch path with n = 1)."""
    return stamp([encode_unstamped(op, seq, key, value, tombstone)])[0]


def _arena(chunks):
    """(arena uint8 array, offsets uint64, lengths uint32) of a list of bytes laid back to back."""
    lens = np.array([len(c) for c in chunks], np.uint32)
    offs = np.zeros(len(chunks), np.uint64)
    if len(chunks) > 1:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    arena = np.frombuffer(b"".join(chunks) + b"\0", np.uint8).copy()  # never empty: the pointer is required
    return arena, offs, lens


def encode_batch(keys, values, seqs=None, first_seq=0, ops=None, tombstones=None):
    """wal_entry::encode for a whole batch (tkv_wal_encode): ``keys`` and ``values`` are lists of bytes,
    ``seqs`` (default first_seq + i), ``ops`` (default PUT) and ``tombstones`` (default 0) per-record
    sequences. The records are laid out on the host and stamped in one GPU batch. Returns
    (image bytes, offsets): the records back to back and a uint64 numpy array of their start offsets."""
    n = len(keys)
    if len(values) != n:
        raise ValueError("keys and values differ in length")
    if n == 0:
        return b"", np.zeros(0, np.uint64)
    karena, koff, klen = _arena(keys)
    varena, voff, vlen = _arena(values)
    seq = None if seqs is None else np.ascontiguousarray(np.asarray(seqs, dtype=np.uint64))
    op = None if ops is None else np.ascontiguousarray(np.asarray(ops, dtype=np.uint8))
    tomb = None if tombstones is None else np.ascontiguousarray(np.asarray(tombstones).astype(bool).astype(np.uint8))
    for name, a in (("seqs", seq), ("ops", op), ("tombstones", tomb)):
        if a is not None and a.size != n:
            raise ValueError(f"{name} must have one entry per record")
    total = int(klen.sum(dtype=np.uint64) + vlen.sum(dtype=np.uint64)) + kMetadataSize * n
    img = np.empty(total, np.uint8)
    offs = np.empty(n, np.uint64)
    size = ctypes.c_uint64(0)

    def ptr(a):
        return None if a is None else ctypes.c_void_p(a.ctypes.data)
    check(load_library().tkv_wal_encode(ptr(karena), ptr(koff), ptr(klen), ptr(varena), ptr(voff), ptr(vlen),
                                        ptr(op), ptr(tomb), ptr(seq), int(first_seq), n, ptr(img), total,
                                        ptr(offs), None, ctypes.byref(size)))
    return img[:size.value].tobytes(), offs


def encode_device(keys, key_off, key_len, vals=None, val_off=None, val_len=None, op=None, tomb=None, seq=None,
                  first_seq=0, out=None, stream=None):
    """wal_entry::encode for a batch held on the device (tkv_wal_encode_device): ``keys`` / ``vals`` uint8
    CUDA arenas, ``key_off`` / ``val_off`` int64 and ``key_len`` / ``val_len`` int32 (u32 values) CUDA
    tensors with one entry per record, ``op`` / ``tomb`` uint8 and ``seq`` int64 per record (defaults:
    no values, PUT, 0, first_seq + i). Returns (image, rec_off, crc): image is ``out[:total]`` (a uint8 CUDA
    tensor of any alignment, e.g. the tail of an image the caller holds; allocated when not given),
    rec_off an int64 tensor of the records' start offsets, crc an int32 tensor of their stamped CRCs.
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
    for name, t, dt in (("op", op, torch.uint8), ("tomb", tomb, torch.uint8), ("seq", seq, torch.int64)):
        if t is not None:
            _check_vec(name, t, dt, n, dev)
    other = stream is not None and stream != torch.cuda.current_stream(dev)

    def alloc(count, dtype):
        t = torch.empty(count, dtype=dtype, device=dev)
        if other:
            t.record_stream(stream)
        return t

    def ptr(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())
    lib = load_library()
    st = _launch_stream(stream, dev)
    size = ctypes.c_uint64(0)

    def call(img, cap, rec_off, crc):
        return lib.tkv_wal_encode_device(ptr(keys), ptr(key_off), ptr(key_len), ptr(vals) if val_len is not None else None,
                                         ptr(val_off) if val_len is not None else None, ptr(val_len), ptr(op), ptr(tomb),
                                         ptr(seq), int(first_seq), n, img, cap, rec_off, crc, ctypes.byref(size), st)
    if out is None:
        rc = call(None, 0, None, None)  # the sizing call
        if rc not in (OK, BUFFER_OVERFLOW):
            check(rc)
        out = alloc(size.value, torch.uint8)
    _check_vec("out", out, torch.uint8, 0, dev)
    rec_off, crc = alloc(n, torch.int64), alloc(n, torch.int32)
    rc = call(ptr(out) if out.numel() else None, out.numel(), ptr(rec_off) if n else None, ptr(crc) if n else None)
    if rc == BUFFER_OVERFLOW:
        raise ValueError(f"out holds {out.numel()} bytes, the image needs {size.value}")
    check(rc)
    return out[:size.value], rec_off, crc


def verify(wal_bytes):
    """Verify a slurped WAL image. Returns (status, n_good_records, stop_offset).

    status is "ok" (every record verified, clean eof) or "corrupted" (first bad record at
    stop_offset, the position wal_entry::decode leaves the view parked on, wal_test.cpp:809-850).
    """
    if isinstance(wal_bytes, np.ndarray):
        buf = np.ascontiguousarray(wal_bytes).reshape(-1).view(np.uint8)
    else:
        buf = np.frombuffer(wal_bytes, np.uint8)  # bytes / bytearray / memoryview: no copy
    good, stop = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = load_library().tkv_wal_verify(ctypes.c_void_p(buf.ctypes.data) if buf.size else None, buf.size,
                                       ctypes.byref(good), ctypes.byref(stop))
    if rc not in (OK, CORRUPTED):
        check(rc)
    return ("ok" if rc == OK else "corrupted"), good.value, stop.value


def verify_device(image, size=None, stream=None):
    """Verify a WAL image held in a uint8 CUDA tensor (first ``size`` bytes; default all).
    Returns (status, n_good_records, stop_offset) as verify()."""
    import torch
    if image.dtype != torch.uint8 or not image.is_cuda or not image.is_contiguous():
        raise ValueError("image must be a contiguous uint8 CUDA tensor")
    n = image.numel() if size is None else int(size)
    if n > image.numel():
        raise ValueError("size exceeds the tensor")
    from .crc32 import _check_data, _launch_stream
    _check_data(image)  # the library's WAL scratch and tables are the current device's
    st = _launch_stream(stream, image.device)
    good, stop = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = load_library().tkv_wal_verify_device(ctypes.c_void_p(image.data_ptr()), n, ctypes.byref(good),
                                              ctypes.byref(stop), st)
    if rc not in (OK, CORRUPTED):
        check(rc)
    return ("ok" if rc == OK else "corrupted"), good.value, stop.value


def index(wal_bytes):
    """Verify a slurped WAL image and list its good records (tkv_wal_index): what engine::create's
    recovery loop needs (engine.cpp:31-53). Returns (status, offsets, stop_offset, max_sequence):
    status and stop_offset as verify(), offsets a uint64 numpy array of the n_good good records' start
    offsets in chain order, max_sequence the largest sequence_ among them (0 for none)."""
    if isinstance(wal_bytes, np.ndarray):
        buf = np.ascontiguousarray(wal_bytes).reshape(-1).view(np.uint8)
    else:
        buf = np.frombuffer(wal_bytes, np.uint8)
    cap = buf.size // kMetadataSize  # a good record is at least 26 bytes long
    offs = np.empty(cap, np.uint64)
    good, stop, seq = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = load_library().tkv_wal_index(ctypes.c_void_p(buf.ctypes.data) if buf.size else None, buf.size,
                                      ctypes.c_void_p(offs.ctypes.data) if cap else None, cap,
                                      ctypes.byref(good), ctypes.byref(stop), ctypes.byref(seq))
    if rc not in (OK, CORRUPTED):
        check(rc)
    return ("ok" if rc == OK else "corrupted"), offs[:good.value], stop.value, seq.value


def index_device(image, size=None, out=None, offsets32=False, stream=None):
    """Verify a WAL image held in a uint8 CUDA tensor (first ``size`` bytes; default all) and list its
    good records on the device (tkv_wal_index_device). Returns (status, offsets, stop_offset,
    max_sequence): offsets is ``out[:n_good]``, the good records' start offsets in chain order, an int64
    CUDA tensor, or an int32 one (u32 offsets, images up to 4 GiB: what check_records_device takes) with
    ``offsets32``. ``out`` (of that dtype) is allocated with size // 26 entries when not given; one with
    fewer entries than there are good records is an error (the C call reports the full count)."""
    import torch
    if image.dtype != torch.uint8 or not image.is_cuda or not image.is_contiguous():
        raise ValueError("image must be a contiguous uint8 CUDA tensor")
    n = image.numel() if size is None else int(size)
    if n > image.numel():
        raise ValueError("size exceeds the tensor")
    from .crc32 import _check_data, _check_vec, _launch_stream
    _check_data(image)
    dtype = torch.int32 if offsets32 else torch.int64
    if out is None:
        out = torch.empty(n // kMetadataSize, dtype=dtype, device=image.device)
        if stream is not None and stream != torch.cuda.current_stream(image.device):
            out.record_stream(stream)
    _check_vec("out", out, dtype, 0, image.device)
    cap = out.numel()
    st = _launch_stream(stream, image.device)
    ptr = ctypes.c_void_p(out.data_ptr()) if cap else None
    good, stop, seq = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = load_library().tkv_wal_index_device(ctypes.c_void_p(image.data_ptr()), n, None if offsets32 else ptr,
                                             ptr if offsets32 else None, cap, ctypes.byref(good),
                                             ctypes.byref(stop), ctypes.byref(seq), st)
    if rc not in (OK, CORRUPTED):
        check(rc)
    if good.value > cap:
        raise ValueError(f"out holds {cap} offsets, the image has {good.value} good records")
    return ("ok" if rc == OK else "corrupted"), out[:good.value], stop.value, seq.value


def check_records_device(image, rec_offsets, max_payload=64, crc_out=None, first_bad=None, stream=None):
    """wal_entry::decode's per-record checks (wal.cpp:63-127) for records whose starts are known:
    ``image`` a uint8 CUDA tensor, ``rec_offsets`` an int32/uint32 CUDA tensor of record start offsets
    (u32; images up to 4 GiB). Returns (first_bad, crc): first_bad is a 1-element int64 CUDA tensor
    holding the index of the first record that fails (len(rec_offsets) when none), crc an int32 CUDA
    tensor of each payload's computed CRC (``crc_out`` if given). Asynchronous on ``stream``, like a
    torch op issued there (tkv_wal_check_records_device)."""
    import torch
    from .crc32 import _check_data, _check_vec, _launch_stream
    if image.dtype != torch.uint8:
        raise ValueError("image must be a uint8 tensor (its size in bytes is its numel)")
    _check_data(image)
    n = rec_offsets.numel()
    if rec_offsets.dtype not in (torch.int32,):
        raise ValueError("rec_offsets must be an int32 tensor (u32 offsets)")
    _check_vec("rec_offsets", rec_offsets, torch.int32, n, image.device)
    # outputs allocated here are tied to a non-current stream for the caching allocator (as _out_vec)
    other = stream is not None and stream != torch.cuda.current_stream(image.device)
    if crc_out is None:
        crc_out = torch.empty(n, dtype=torch.int32, device=image.device)
        if other:
            crc_out.record_stream(stream)
    _check_vec("crc_out", crc_out, torch.int32, n, image.device)
    if first_bad is None:
        first_bad = torch.empty(1, dtype=torch.int64, device=image.device)
        if other:
            first_bad.record_stream(stream)
    _check_vec("first_bad", first_bad, torch.int64, 1, image.device)
    check(load_library().tkv_wal_check_records_device(
        ctypes.c_void_p(image.data_ptr()), image.numel(), ctypes.c_void_p(rec_offsets.data_ptr()), n,
        int(max_payload), ctypes.c_void_p(crc_out.data_ptr()), ctypes.c_void_p(first_bad.data_ptr()),
        _launch_stream(stream, image.device)))
    return first_bad, crc_out


WalBatch = collections.namedtuple("WalBatch", "op tomb seq key_off key_len val_off val_len keys vals")
WalBatch.__doc__ = """A decoded record list in the columnar form encode_device takes: per-record op, tomb, seq,
key_off, key_len, val_off, val_len and the key / value arenas (for a views arena: the image itself)."""
KEY_VIEWS, VAL_VIEWS = 1, 2  # TKV_WAL_DECODE_KEY_VIEWS / _VAL_VIEWS


def decode_device(image, rec_off, size=None, key_views=False, val_views=False, stream=None):
    """wal_entry::decode's fields (wal.cpp:98-127) for the records of a WAL image in a uint8 CUDA tensor
    (first ``size`` bytes; default all) that start at ``rec_off``, an int64 or int32 (u32 offsets) CUDA
    tensor such as index_device returns (tkv_wal_decode_device). Returns a WalBatch of CUDA tensors: op /
    tomb uint8, seq / key_off / val_off int64, key_len / val_len int32 (u32 values) and the key / value
    arenas, the keys (values) back to back in batch order, or the image itself with offsets into it with
    ``key_views`` (``val_views``). The batch is what encode_device takes. No checksum is computed: the
    offsets come from index_device or are checked by check_records_device. A record that fails
    wal_entry::decode's structural checks raises ValueError naming its index. Synchronous on ``stream``."""
    import torch
    from ._lib import BUFFER_OVERFLOW
    from .crc32 import _check_data, _check_vec, _launch_stream
    if image.dtype != torch.uint8:
        raise ValueError("image must be a uint8 tensor")
    _check_data(image)
    dev = image.device
    size = image.numel() if size is None else int(size)
    if size > image.numel():
        raise ValueError("size exceeds the tensor")
    if rec_off.dtype not in (torch.int64, torch.int32):
        raise ValueError("rec_off must be an int64 or int32 (u32 offsets) tensor")
    n = rec_off.numel()
    _check_vec("rec_off", rec_off, rec_off.dtype, n, dev)
    other = stream is not None and stream != torch.cuda.current_stream(dev)

    def alloc(count, dtype):
        t = torch.empty(count, dtype=dtype, device=dev)
        if other:
            t.record_stream(stream)
        return t

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    flags = (KEY_VIEWS if key_views else 0) | (VAL_VIEWS if val_views else 0)
    lib = load_library()
    st = _launch_stream(stream, dev)
    ks, vs, bad = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    off64, off32 = (ptr(rec_off), None) if rec_off.dtype == torch.int64 else (None, ptr(rec_off))

    def call(cols, keys, vals):
        return lib.tkv_wal_decode_device(ptr(image), size, off64, off32, n, flags, *[ptr(c) for c in cols], ptr(keys),
                                         0 if keys is None else keys.numel(), ptr(vals),
                                         0 if vals is None else vals.numel(), ctypes.byref(ks), ctypes.byref(vs),
                                         ctypes.byref(bad), st)
    rc = call([None] * 7, None, None)  # the sizing call
    if rc == CORRUPTED:
        raise ValueError(f"record {bad.value} of {n} fails wal_entry::decode's structural checks")
    if rc not in (OK, BUFFER_OVERFLOW):
        check(rc)
    cols = [alloc(n, dt) for dt in (torch.uint8, torch.uint8, torch.int64, torch.int64, torch.int32, torch.int64,
                                    torch.int32)]
    keys = image if key_views else alloc(ks.value, torch.uint8)
    vals = image if val_views else alloc(vs.value, torch.uint8)
    rc = call(cols, None if key_views else keys, None if val_views else vals)
    if rc == CORRUPTED:
        raise ValueError(f"record {bad.value} of {n} fails wal_entry::decode's structural checks")
    check(rc)
    return WalBatch(*cols, keys, vals)


MODES = ("strict", "tolerate_tail", "skip_corrupted")
_NO_LIMIT = (1 << 64) - 1


def _device_image(image, size):
    import torch
    if image.dtype != torch.uint8 or not image.is_cuda or not image.is_contiguous():
        raise ValueError("image must be a contiguous uint8 CUDA tensor")
    n = image.numel() if size is None else int(size)
    if n > image.numel():
        raise ValueError("size exceeds the tensor")
    return n


def resync_device(image, start, size=None, stream=None):
    """The smallest position >= ``start`` of a WAL image in a uint8 CUDA tensor (first ``size`` bytes;
    default all) at which a record passes every check of wal_entry::decode (length inside the image, key
    and value inside the record, CRC), or None when there is none (tkv_wal_resync_device). Every byte
    offset is a candidate; a CRC collision (2^-32 per plausible header) is accepted. Synchronous on
    ``stream``."""
    from ._lib import NOT_FOUND
    from .crc32 import _check_data, _launch_stream
    n = _device_image(image, size)
    _check_data(image)
    found = ctypes.c_uint64(0)
    rc = load_library().tkv_wal_resync_device(ctypes.c_void_p(image.data_ptr()) if n else None, n, int(start),
                                              ctypes.byref(found), _launch_stream(stream, image.device))
    if rc == NOT_FOUND:
        return None
    check(rc)
    return found.value


GAPS_CAP = 1 << 16  # gaps a salvage wrapper lists in its first (and nearly always only) call: a 1 MiB array


def _gaps_array(call, size):
    """Runs call(gaps array, gap_cap) -> (rc, n_gaps) with room for every gap the image can hold (a gap
    is at least one byte and, but for a tail gap, is followed by a record of at least 26 bytes), at most
    GAPS_CAP. Only an image with more gaps than GAPS_CAP is salvaged a second time, with room for all."""
    cap = max(1, min(size // (kMetadataSize + 1) + 1, GAPS_CAP))
    gaps = np.zeros((cap, 2), np.uint64)
    rc, k = call(gaps, cap)
    if rc in (OK, CORRUPTED) and k > cap:
        gaps = np.zeros((k, 2), np.uint64)
        rc, k = call(gaps, k)
    return rc, gaps[:k]


def salvage_device(image, size=None, out=None, max_gaps=None, stream=None):
    """Every valid record of a WAL image in a uint8 CUDA tensor, corrupted ranges skipped
    (tkv_wal_salvage_device): the sequential program ``p = 0; while p < size: valid(p) ? emit, p += record
    size : p += 1``. Returns (status, offsets, gaps, stop_offset, max_sequence): offsets is ``out[:n]``, an
    int64 CUDA tensor of the salvaged records' start offsets in increasing order (allocated with
    size // 26 entries when not given), gaps a (k, 2) uint64 numpy array of the skipped ranges
    [start, end) (end == size: a tail gap), status "ok" when there is no gap and the image was read to its
    end. ``max_gaps`` bounds the resynchronisations: the call stops at the next invalid position, which is
    stop_offset (else size); 0 is index_device. Valid records nested in a corrupted record's value are
    salvaged, by the definition; the caller decides what to do with the gaps."""
    import torch
    from .crc32 import _check_data, _check_vec, _launch_stream
    n = _device_image(image, size)
    _check_data(image)
    if out is None:
        out = torch.empty(n // kMetadataSize, dtype=torch.int64, device=image.device)
        if stream is not None and stream != torch.cuda.current_stream(image.device):
            out.record_stream(stream)
    _check_vec("out", out, torch.int64, 0, image.device)
    cap = out.numel()
    st = _launch_stream(stream, image.device)
    nrec, ngap, stop, skipped, seq = (ctypes.c_uint64(0) for _ in range(5))
    limit = _NO_LIMIT if max_gaps is None else int(max_gaps)

    def call(gaps, gap_cap):
        rc = load_library().tkv_wal_salvage_device(
            ctypes.c_void_p(image.data_ptr()) if n else None, n, ctypes.c_void_p(out.data_ptr()) if cap else None, cap,
            ctypes.c_void_p(gaps.ctypes.data), gap_cap, limit, ctypes.byref(nrec), ctypes.byref(ngap),
            ctypes.byref(stop), ctypes.byref(skipped), ctypes.byref(seq), st)
        return rc, ngap.value
    rc, gaps = _gaps_array(call, n)
    if rc not in (OK, CORRUPTED):
        check(rc)
    if nrec.value > cap:
        raise ValueError(f"out holds {cap} offsets, the image has {nrec.value} valid records")
    return ("ok" if rc == OK else "corrupted"), out[:nrec.value], gaps, stop.value, seq.value


def salvage(wal_bytes, max_gaps=None):
    """salvage_device for a slurped WAL image on the host (tkv_wal_salvage): copied to the device as
    index() copies it and salvaged there. Returns (status, offsets, gaps, stop_offset, max_sequence) with
    offsets a uint64 numpy array. An image the device cannot hold gets index()'s result (no
    resynchronisation, stop_offset at its stop)."""
    buf = _host_image(wal_bytes)
    cap = buf.size // kMetadataSize
    offs = np.empty(cap, np.uint64)
    nrec, ngap, stop, skipped, seq = (ctypes.c_uint64(0) for _ in range(5))
    limit = _NO_LIMIT if max_gaps is None else int(max_gaps)

    def call(gaps, gap_cap):
        rc = load_library().tkv_wal_salvage(
            ctypes.c_void_p(buf.ctypes.data) if buf.size else None, buf.size,
            ctypes.c_void_p(offs.ctypes.data) if cap else None, cap, ctypes.c_void_p(gaps.ctypes.data), gap_cap, limit,
            ctypes.byref(nrec), ctypes.byref(ngap), ctypes.byref(stop), ctypes.byref(skipped), ctypes.byref(seq))
        return rc, ngap.value
    rc, gaps = _gaps_array(call, buf.size)
    if rc not in (OK, CORRUPTED):
        check(rc)
    return ("ok" if rc == OK else "corrupted"), offs[:nrec.value], gaps, stop.value, seq.value


def recover_device(image, size=None, key_views=False, val_views=False, stream=None, mode="strict"):
    """What engine::create's recovery loop (engine.cpp:31-53) consumes, for a WAL image in HBM:
    index_device, then decode_device on the good records. Returns (status, WalBatch, stop_offset,
    max_sequence); status, stop_offset and max_sequence are index_device's, the batch holds exactly the
    good prefix.

    ``mode`` picks the recovery policy. "strict" (default) is the above, the reference's only one.
    "tolerate_tail": when the index reports corrupted and no valid record follows its stop offset
    (resync_device(stop + 1) finds none: a torn tail), the result is the good prefix with status "ok";
    otherwise the strict result. "skip_corrupted": every salvaged record is decoded (salvage_device),
    status "corrupted" when there was a gap, and the gaps are returned as a fifth element."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}")
    if mode == "skip_corrupted":
        status, offs, gaps, stop, max_seq = salvage_device(image, size=size, stream=stream)
        batch = decode_device(image, offs, size=size, key_views=key_views, val_views=val_views, stream=stream)
        return status, batch, stop, max_seq, gaps
    status, offs, stop, max_seq = index_device(image, size=size, stream=stream)
    if mode == "tolerate_tail" and status == "corrupted" and resync_device(image, stop + 1, size=size, stream=stream) is None:
        status = "ok"
    batch = decode_device(image, offs, size=size, key_views=key_views, val_views=val_views, stream=stream)
    return status, batch, stop, max_seq


def _host_image(wal_bytes):
    if isinstance(wal_bytes, np.ndarray):
        return np.ascontiguousarray(wal_bytes).reshape(-1).view(np.uint8)
    return np.frombuffer(wal_bytes, np.uint8)


def decode_batch(wal_bytes, rec_off, key_views=False, val_views=False):
    """decode_device for an image held on the host (tkv_wal_decode_host: host threads, no GPU, no
    checksum): ``rec_off`` a sequence of record start offsets such as index() returns. Returns a WalBatch
    of numpy arrays (op / tomb uint8, seq / key_off / val_off uint64, key_len / val_len uint32, the
    arenas uint8; a views arena is the image as a uint8 array)."""
    from ._lib import BUFFER_OVERFLOW
    buf = _host_image(wal_bytes)
    off = np.ascontiguousarray(np.asarray(rec_off, dtype=np.uint64))
    n = off.size
    flags = (KEY_VIEWS if key_views else 0) | (VAL_VIEWS if val_views else 0)
    ks, vs, bad = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)

    def ptr(a):
        return ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else None

    def call(cols, keys, vals):
        return load_library().tkv_wal_decode_host(ptr(buf), buf.size, ptr(off), n, flags, *[ptr(c) for c in cols],
                                                  ptr(keys), 0 if keys is None else keys.size, ptr(vals),
                                                  0 if vals is None else vals.size, ctypes.byref(ks), ctypes.byref(vs),
                                                  ctypes.byref(bad))
    rc = call([None] * 7, None, None)  # the sizing call
    if rc == CORRUPTED:
        raise ValueError(f"record {bad.value} of {n} fails wal_entry::decode's structural checks")
    if rc not in (OK, BUFFER_OVERFLOW):
        check(rc)
    cols = [np.empty(n, dt) for dt in (np.uint8, np.uint8, np.uint64, np.uint64, np.uint32, np.uint64, np.uint32)]
    keys = buf if key_views else np.empty(ks.value, np.uint8)
    vals = buf if val_views else np.empty(vs.value, np.uint8)
    check(call(cols, None if key_views else keys, None if val_views else vals))
    return WalBatch(*cols, keys, vals)


def recover(wal_bytes, key_views=False, val_views=False, mode="strict"):
    """recover_device for a slurped WAL image on the host: index() (verify and list on the GPU), then
    decode_batch (host threads) on the good records. Returns (status, WalBatch of numpy arrays,
    stop_offset, max_sequence). ``mode`` as recover_device: "tolerate_tail" asks salvage() with one
    resynchronisation whether a valid record follows the stop offset, "skip_corrupted" decodes every
    salvaged record and appends the gaps."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}")
    if mode == "skip_corrupted":
        status, offs, gaps, stop, max_seq = salvage(wal_bytes)
        return status, decode_batch(wal_bytes, offs, key_views=key_views, val_views=val_views), stop, max_seq, gaps
    status, offs, stop, max_seq = index(wal_bytes)
    if mode == "tolerate_tail" and status == "corrupted":
        # one resynchronisation: a torn tail is a single gap that ends at the image's end, no record behind it
        _, more, gaps, _, _ = salvage(wal_bytes, max_gaps=1)
        if more.size == offs.size and gaps.shape[0] == 1 and int(gaps[0, 1]) == _host_image(wal_bytes).size:
            status = "ok"
    return status, decode_batch(wal_bytes, offs, key_views=key_views, val_views=val_views), stop, max_seq


def decode_fields(rec):
    """Header fields of one record (no checking): (record_len, crc, op, seq, tomb, key, value)."""
    record_len, crc = struct.unpack_from("<II", rec, 0)
    op, seq, tomb, klen, vlen = struct.unpack_from("<BQBII", rec, 8)
    key = rec[kMetadataSize:kMetadataSize + klen]
    value = rec[kMetadataSize + klen:kMetadataSize + klen + vlen]
    return record_len, crc, op, seq, tomb, key, value
