"""Memtable replay: the content a memtable holds after a whole decoded WAL batch was inserted.

engine::create's replay loop (/root/reference/src/engine/engine.cpp:30-47) inserts every recovered record
into a memtable (memtable.cpp:58-72), a skiplist ordered by user key in which an insert of an equal key
replaces the node (skiplist.hpp:201-242). For a whole batch that is a stable sort of variable-length byte
strings with last-writer-wins, and it runs here as one call (include/tkv_crc32.h "Memtable replay"):
``build_device`` for the columns wal.decode_device / wal.recover_device return, on the GPU, and ``build``
for a record list on host threads. The result is a run of encoded internal keys (user_key | u64 seq |
u64 timestamp | u8 tombstone, sstable_format.cpp:9-25) in ascending order with the surviving records'
value spans: what sst.build_device takes.
"""
import collections
import ctypes

import numpy as np

from ._lib import BUFFER_OVERFLOW, CORRUPTED, OK, check, load_library

META = 17        # bytes encode_internal_key puts behind the user key
PUT, DEL = 0, 1  # wal_operation


class MemtableRun(collections.namedtuple("MemtableRun", "ikeys ikey_off ikey_len val_off val_len src vals")):
    """One entry per distinct user key, ascending: the internal keys back to back in ``ikeys`` with
    ``ikey_off`` / ``ikey_len``, the surviving record's value span ``val_off`` / ``val_len`` in ``vals``
    (the batch's value arena, untouched; length 0 for a delete) and its index ``src`` in the batch."""
    __slots__ = ()

    def flush(self, target_block_size=4096, out=None, stream=None):
        """The run as an SSTable file image (sst.build_device for a device run, sst.build for a host run)."""
        from . import sst
        if isinstance(self.ikeys, np.ndarray):
            return sst.build((self.ikeys, self.ikey_off, self.ikey_len, self.vals, self.val_off, self.val_len),
                             target_block_size=target_block_size)
        return sst.build_device(self.ikeys, self.ikey_off, self.ikey_len, self.vals, self.val_off, self.val_len,
                                target_block_size=target_block_size, out=out, stream=stream)

    def entries(self):
        """[(ikey, value)] as bytes (tests and small runs)."""
        def host(t):
            return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
        ik, vals = host(self.ikeys).view(np.uint8).tobytes(), host(self.vals).view(np.uint8).tobytes()
        ko, vo = host(self.ikey_off).view(np.uint64), host(self.val_off).view(np.uint64)
        kl, vl = host(self.ikey_len).view(np.uint32), host(self.val_len).view(np.uint32)
        return [(ik[int(ko[j]):int(ko[j]) + int(kl[j])], vals[int(vo[j]):int(vo[j]) + int(vl[j])])
                for j in range(len(kl))]


class BadOperation(ValueError):
    """A record whose op is neither put nor delete (the reference's FR_VERIFY abort). ``index`` names it."""

    def __init__(self, index, n):
        self.index = index
        super().__init__(f"record {index} of {n} has an operation that is neither put nor delete")


def _two_calls(call, n, alloc):
    """The sizing call, then the build into freshly allocated arrays. ``call(ikeys, cap, cols, entry_cap)``
    returns (rc, n_entries, ikeys_size, first_bad)."""
    rc, m, size, bad = call(None, 0, [None] * 5, 0)
    if rc == CORRUPTED:
        raise BadOperation(bad, n)
    if rc not in (OK, BUFFER_OVERFLOW):
        check(rc)
    ikeys = alloc(size, "u8")
    cols = [alloc(m, k) for k in ("u64", "u32", "u64", "u32", "u32")]  # ikey_off, ikey_len, val_off, val_len, src
    if m:
        check(call(ikeys, size, cols, m)[0])
    return ikeys, cols


def build_device(batch=None, timestamp_ms=0, stream=None, **columns):
    """The replay of a decoded batch on the device (tkv_memtable_build_device). ``batch`` is a wal.WalBatch
    of CUDA tensors (or pass its columns by keyword: keys, key_off, key_len and optionally val_off, val_len,
    op, tomb, seq, vals): keys a uint8 arena (under key_views the WAL image itself), key_off / val_off / seq
    int64, key_len / val_len int32 (u32 values), op / tomb uint8. Returns a MemtableRun of CUDA tensors:
    ikeys uint8, ikey_off / val_off int64, ikey_len / val_len / src int32 (u32 values), ``vals`` the batch's
    value arena. Makes the sizing call, then the build. A record with an unknown op raises BadOperation.
    Synchronous on ``stream``."""
    import torch
    from .crc32 import _check_data, _check_vec, _launch_stream
    if batch is not None:
        columns = dict(batch._asdict(), **columns)
    keys, key_off, key_len = columns["keys"], columns["key_off"], columns["key_len"]
    if keys.dtype != torch.uint8:
        raise ValueError("keys must be a uint8 tensor")
    _check_data(keys)
    dev = keys.device
    n = key_len.numel()
    _check_vec("key_off", key_off, torch.int64, n, dev)
    _check_vec("key_len", key_len, torch.int32, n, dev)
    opt = {}
    for name, dt in (("val_off", torch.int64), ("val_len", torch.int32), ("op", torch.uint8), ("tomb", torch.uint8),
                     ("seq", torch.int64)):
        t = columns.get(name)
        if t is not None:
            _check_vec(name, t, dt, n, dev)
        opt[name] = t
    if opt["val_len"] is not None and opt["val_off"] is None:
        raise ValueError("val_len needs val_off")
    vals = columns.get("vals")
    other = stream is not None and stream != torch.cuda.current_stream(dev)
    kinds = {"u8": torch.uint8, "u64": torch.int64, "u32": torch.int32}

    def alloc(count, kind):
        # (an arena without a byte has no address: data_ptr() of an empty tensor is 0. So MemtableRun.vals
        # may be such a tensor, when the batch has no value arena or an empty one. sst.build_device stands a
        # spare byte in for it and sst.merge_device leaves it out; any other caller that hands run.vals to
        # a C call beside a non-NULL val_len has to do the same, or the call answers "null pointer")
        t = torch.empty(count, dtype=kinds[kind], device=dev)
        if other:
            t.record_stream(stream)
        return t

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    lib = load_library()
    st = _launch_stream(stream, dev)
    outs = [ctypes.c_uint64(0) for _ in range(3)]

    def call(ikeys, cap, cols, entry_cap):
        rc = lib.tkv_memtable_build_device(ptr(keys), keys.numel(), ptr(key_off), ptr(key_len), ptr(opt["val_off"]),
                                           ptr(opt["val_len"]), ptr(opt["op"]), ptr(opt["tomb"]), ptr(opt["seq"]), n,
                                           int(timestamp_ms), ptr(ikeys), cap, *[ptr(c) for c in cols], entry_cap,
                                           *[ctypes.byref(o) for o in outs], st)
        return rc, outs[0].value, outs[1].value, outs[2].value
    ikeys, cols = _two_calls(call, n, alloc)
    if vals is None:
        vals = alloc(0, "u8")
    return MemtableRun(ikeys, cols[0], cols[1], cols[2], cols[3], cols[4], vals)


def build(records, timestamp_ms=0):
    """The same on the host (tkv_memtable_build: host threads, no GPU): ``records`` is a list of
    (op, seq, key, value, tomb) in log order. Returns a MemtableRun of numpy arrays (uint8 arenas, uint64
    offsets, uint32 lengths and src); ``vals`` holds the records' values back to back."""
    from .wal import _arena
    n = len(records)
    keys, koff, klen = _arena([r[2] for r in records])
    vals, voff, vlen = _arena([r[3] for r in records])
    op = np.array([r[0] for r in records], np.uint8)
    seq = np.array([r[1] for r in records], np.uint64)
    tomb = np.array([int(r[4]) & 0xFF for r in records], np.uint8)
    return build_host_columns(keys[:-1], koff, klen, voff, vlen, op, tomb, seq, timestamp_ms, vals, n)


def build_host_columns(keys, key_off, key_len, val_off=None, val_len=None, op=None, tomb=None, seq=None,
                       timestamp_ms=0, vals=None, n=None):
    """tkv_memtable_build over numpy columns (the dtypes wal.decode_batch returns); each of val_off, val_len,
    op, tomb and seq may be None."""
    keys = np.ascontiguousarray(keys, dtype=np.uint8)
    key_off = np.ascontiguousarray(key_off, dtype=np.uint64)
    key_len = np.ascontiguousarray(key_len, dtype=np.uint32)
    n = key_len.size if n is None else n
    cols = []
    for a, dt in ((val_off, np.uint64), (val_len, np.uint32), (op, np.uint8), (tomb, np.uint8), (seq, np.uint64)):
        cols.append(None if a is None else np.ascontiguousarray(a, dtype=dt))
    kinds = {"u8": np.uint8, "u64": np.uint64, "u32": np.uint32}
    outs = [ctypes.c_uint64(0) for _ in range(3)]

    def ptr(a):
        return ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else None

    def call(ikeys, cap, out_cols, entry_cap):
        rc = load_library().tkv_memtable_build(ptr(keys), keys.size, ptr(key_off), ptr(key_len), *[ptr(c) for c in cols], n,
                                               int(timestamp_ms), ptr(ikeys), cap, *[ptr(c) for c in out_cols], entry_cap,
                                               *[ctypes.byref(o) for o in outs])
        return rc, outs[0].value, outs[1].value, outs[2].value
    ikeys, oc = _two_calls(call, n, lambda count, kind: np.empty(count, kinds[kind]))
    if vals is None:
        vals = np.zeros(1, np.uint8)
    return MemtableRun(ikeys, oc[0], oc[1], oc[2], oc[3], oc[4], vals)
