"""Sequential oracle of the memtable replay (tkv_memtable_build[_device]) and the inputs its tests share.

``oracle`` replays the records into a dict in input order (a later insert of an equal key overwrites, a
delete stores an empty value, an unknown op raises with its index) and iterates ``sorted(dict)``: Python's
order of ``bytes`` is simd_comparator's (unsigned bytewise, a prefix first). It does not use
tinykvpp_amd.memtable.
"""
import collections
import ctypes
import struct

import numpy as np

META = 17
FUZZ_SEEDS = 64
PAD = 8              # canary elements on either side of an output column
ARENA_PAD = 64       # canary bytes on either side of the internal-key arena
CANARY8, CANARY32, CANARY64 = 0xC7, 0xC7C7C7C7, 0xC7C7C7C7C7C7C7C7
OUT_NAMES = ("ikeys", "ikey_off", "ikey_len", "val_off", "val_len", "src")

Columns = collections.namedtuple("Columns", "keys key_off key_len val_off val_len op tomb seq")
Expected = collections.namedtuple("Expected", "ikeys ikey_off ikey_len val_off val_len src")


class BadOp(ValueError):
    def __init__(self, index):
        self.index = index
        super().__init__(f"bad op at {index}")


def columns(records, rng=None, views=False):
    """Columns of records [(op, seq, key, value, tomb)]. The keys lie back to back, or with ``views`` as
    overlapping, unaligned views into one blob: equal keys share bytes, the rest lies in shuffled order
    behind a random lead. Values are spans of a notional arena (never read): back to back."""
    n = len(records)
    kl = np.array([len(r[2]) for r in records], np.uint32)
    ko = np.zeros(n, np.uint64)
    if views:
        blob, seen = bytearray(rng.integers(0, 256, int(rng.integers(0, 7)), dtype=np.uint8).tobytes()), {}
        for i in rng.permutation(n).tolist():
            k = records[i][2]
            at = blob.find(k) if len(k) and rng.integers(0, 2) else -1  # any earlier occurrence will do
            if at < 0:
                at = seen.get(k, -1)
            if at < 0:
                at = len(blob)
                blob += k
            seen[k] = at
            ko[i] = at
        keys = np.frombuffer(bytes(blob), np.uint8).copy()
    else:
        if n > 1:
            ko[1:] = np.cumsum(kl[:-1], dtype=np.uint64)
        keys = np.frombuffer(b"".join(r[2] for r in records), np.uint8).copy()
    vl = np.array([len(r[3]) for r in records], np.uint32)
    vo = np.zeros(n, np.uint64)
    if n > 1:
        vo[1:] = np.cumsum(vl[:-1], dtype=np.uint64)
    return Columns(keys, ko, kl, vo, vl, np.array([r[0] for r in records], np.uint8),
                   np.array([r[4] for r in records], np.uint8), np.array([r[1] for r in records], np.uint64))


def values_arena(records):
    return np.frombuffer(b"".join(r[3] for r in records) + b"\0", np.uint8).copy()


def oracle(c, ts=0):
    """Expected outputs of a Columns (numpy; optional columns may be None)."""
    raw = c.keys.tobytes()
    n = c.key_len.size
    d = {}
    for i in range(n):
        if c.op is not None and int(c.op[i]) > 1:
            raise BadOp(i)
        o, ln = int(c.key_off[i]), int(c.key_len[i])
        d[raw[o:o + ln]] = i
    order = sorted(d)
    src = np.array([d[k] for k in order], np.uint32)
    ik = []
    for k in order:
        i = d[k]
        seq = 0 if c.seq is None else int(c.seq[i])
        tomb = 0 if c.tomb is None else int(c.tomb[i] != 0)
        ik.append(k + struct.pack("<QQB", seq, ts, tomb))
    il = np.array([len(x) for x in ik], np.uint32)
    io = np.zeros(len(ik), np.uint64)
    if len(ik) > 1:
        io[1:] = np.cumsum(il[:-1], dtype=np.uint64)
    vo = np.zeros(len(ik), np.uint64) if c.val_off is None else c.val_off[src].astype(np.uint64)
    vl = np.zeros(len(ik), np.uint32) if c.val_len is None else c.val_len[src].astype(np.uint32)
    if c.op is not None:
        vl = np.where(c.op[src] == 1, 0, vl).astype(np.uint32)
    return Expected(b"".join(ik), io, il, vo, vl, src)


def entries(exp, vals):
    """[(ikey, value)] of an Expected over the value arena ``vals`` (bytes): sst_build_util.oracle_file's input."""
    return [(exp.ikeys[int(o):int(o) + int(ln)], vals[int(vo):int(vo) + int(vl)])
            for o, ln, vo, vl in zip(exp.ikey_off, exp.ikey_len, exp.val_off, exp.val_len)]


def shared_first_word(c):
    """Records longer than 8 bytes whose first 8 bytes equal another such record's: what enters round 2."""
    raw = c.keys.tobytes()
    heads = [raw[int(o):int(o) + 8] for o, ln in zip(c.key_off, c.key_len) if ln > 8]
    cnt = collections.Counter(heads)
    return sum(1 for h in heads if cnt[h] > 1)


# ---- cases ----------------------------------------------------------------------------------------------

def _recs(keys, rng=None):
    """Put records over a key list: seq = index + 1, value = 1-5 bytes naming the index."""
    return [(0, i + 1, k, (b"v%d" % i)[:5], 0) for i, k in enumerate(keys)]


def random_keys(rng, n, max_len=23):
    blob = rng.integers(0, 256, n * max_len + 1, dtype=np.uint8).tobytes()
    lens = rng.integers(0, max_len + 1, n)
    return [blob[i * max_len:i * max_len + int(ln)] for i, ln in enumerate(lens)]


def order_cases():
    """Named record lists on the comparator's edges."""
    rng = np.random.default_rng(7)
    base = bytes(range(0x30, 0x30 + 17))
    same16 = b"ABCDEFGHIJKLMNOP"
    cases = {
        "empty_key": [b"b", b"", b"a", b"\x00", b"", b"ab"],
        "prefix_zero": [b"a\x01", b"a\x00\x00", b"a", b"a\x00", b"", b"\x80", b"a"],
        "unsigned": [b"\xff", b"\x7f", b"\x80", b"\x00", b"\x7f\xff", b"\x80\x00", b"\xff\xff", b"\x7f\x80"],
        "one_byte_differs": [base[:p] + bytes([base[p] ^ x]) + base[p + 1:] for p in range(17) for x in (0x40, 0, 1)],
        "lengths_7_to_17": [same16[:ln] if ln <= 16 else same16 + b"Q" for ln in (17, 9, 7, 16, 8, 15, 17, 7, 8, 9, 15, 16)] +
                           [same16[:8] + b"\x00", same16[:8] + b"\x00\x00", same16 + b"\x00", same16[:15] + b"\x00\x00"],
    }
    ks = sorted(set(random_keys(rng, 300)))
    cases["sorted"] = ks
    cases["reverse"] = ks[::-1]
    return {name: _recs(keys) for name, keys in cases.items()}


def long_tail_case():
    """130 keys of 1000 bytes that differ only in the last byte, in shuffled order."""
    rng = np.random.default_rng(11)
    body = rng.integers(0, 256, 999, dtype=np.uint8).tobytes()
    last = rng.permutation(256)[:130]
    return _recs([body + bytes([int(b)]) for b in last])


def replacement_cases():
    rng = np.random.default_rng(13)
    cases = {"all_equal": [(0, 5000 - i, b"same-key", b"%d" % i, 0) for i in range(4097)]}
    for gap in (1, 64, 256, 4096):
        ks = list(dict.fromkeys(random_keys(rng, 2 * gap + 50, 12)))[:gap] if gap > 1 else [b"k0", b"k1", b"k2"]
        assert len(ks) == max(gap, 3)
        # every block of `gap` distinct keys twice: the second copy `gap` positions later
        recs = [(0, 10 + i, k, b"first", 0) for i, k in enumerate(ks)] + [(0, 5 + i, k, b"second!", 0) for i, k in enumerate(ks)]
        if gap == 1:
            recs = [r for k in ks for r in ((0, 9, k, b"first", 0), (0, 3, k, b"second!", 0))]
        cases[f"twice_gap_{gap}"] = recs
    cases["lower_seq_survives"] = [(0, 900, b"k", b"old", 0), (0, 7, b"k", b"new", 0), (0, 8, b"j", b"x", 0)]
    cases["del_after_put"] = [(0, 1, b"k", b"value", 0), (1, 2, b"k", b"carried-bytes", 1), (0, 3, b"a", b"z", 0)]
    cases["put_after_del"] = [(1, 1, b"k", b"", 1), (0, 2, b"k", b"back", 0), (1, 3, b"zz", b"gone", 0)]
    cases["tomb_bytes"] = [(0, 1, b"t0", b"a", 0), (0, 2, b"t1", b"b", 1), (1, 3, b"t2", b"c", 2), (0, 4, b"t255", b"d", 0xFF),
                           (1, 5, b"t1del0", b"e", 0)]
    return cases


def fuzz_case(seed):
    """(Columns, records, ts): n <= 5000 records, key lengths 0-40 over a small alphabet (duplicates and
    shared prefixes are common), ops 0/1, tomb any byte, random seq; every fifth case takes its keys as
    overlapping views into one blob."""
    rng = np.random.default_rng(0x3E3E + seed)
    n = int(rng.integers(1, 5001)) if seed % 4 else int(rng.integers(1, 80))
    alpha = np.array([0x00, 0x01, 0x61, 0x62, 0x7F, 0x80, 0xFF][:int(rng.integers(2, 8))], np.uint8)
    if seed % 3 == 0:
        lens = rng.integers(0, 41, n)
    else:  # mostly short: many duplicates
        lens = np.where(rng.random(n) < 0.8, rng.integers(0, 6, n), rng.integers(0, 41, n))
    stem = alpha[rng.integers(0, alpha.size, 40)].tobytes()
    recs = []
    for i in range(n):
        ln = int(lens[i])
        if rng.random() < 0.5:  # a shared stem with a random tail
            cut = int(rng.integers(0, ln + 1))
            k = stem[:cut] + alpha[rng.integers(0, alpha.size, ln - cut)].tobytes()
        else:
            k = alpha[rng.integers(0, alpha.size, ln)].tobytes()
        op = int(rng.integers(0, 2))
        recs.append((op, int(rng.integers(0, 1 << 62)), k, bytes(int(rng.integers(0, 9))), int(rng.choice([0, 0, 1, 1, 2, 0xFF]))))
    return columns(recs, rng, views=seed % 5 == 0), recs, int(rng.integers(0, 1 << 48))


# ---- calling the C ABI with canaried outputs ---------------------------------------------------------------

class Outputs:
    """Output arrays for one call: ``entry_cap`` entries per column and ``ikeys_cap`` arena bytes (at byte
    misalignment ``misalign``), canaries on both sides of each; names in ``nulls`` are passed as NULL."""
    DT = {"ikeys": np.uint8, "ikey_off": np.uint64, "ikey_len": np.uint32, "val_off": np.uint64, "val_len": np.uint32,
          "src": np.uint32}

    def __init__(self, entry_cap, ikeys_cap, misalign=0, nulls=()):
        self.entry_cap, self.ikeys_cap, self.misalign, self.nulls = entry_cap, ikeys_cap, misalign, set(nulls)
        self.lead = {"ikeys": ARENA_PAD + misalign}
        self.host = {}
        for name, dt in self.DT.items():
            lead = self.lead.setdefault(name, PAD)
            count = ikeys_cap if name == "ikeys" else entry_cap
            can = {np.uint8: CANARY8, np.uint32: CANARY32, np.uint64: CANARY64}[dt]
            self.host[name] = np.full(lead + count + (ARENA_PAD if name == "ikeys" else PAD), can, dt)
        self.dev = None

    def to(self, device):
        import torch
        self.dev = {k: torch.from_numpy(v if v.dtype == np.uint8 else v.view(v.dtype.str.replace("u", "i"))).to(device)
                    for k, v in self.host.items()}
        return self

    def ptr(self, name):
        if name in self.nulls:
            return None
        item = self.host[name].itemsize
        base = self.dev[name].data_ptr() if self.dev is not None else self.host[name].ctypes.data
        return ctypes.c_void_p(base + self.lead[name] * item)

    def fetch(self):
        if self.dev is not None:
            for k, v in self.dev.items():
                self.host[k] = v.cpu().numpy().view(self.DT[k])

    def get(self, name, count):
        lead = self.lead[name]
        return self.host[name][lead:lead + count]

    def untouched(self, name, written=0):
        """Whether everything but the first ``written`` elements of a column still is canary."""
        a = self.host[name]
        can = a.dtype.type({1: CANARY8, 4: CANARY32, 8: CANARY64}[a.itemsize])
        lead = self.lead[name]
        return bool((a[:lead] == can).all() and (a[lead + written:] == can).all())


def call(fn, c, ts, outs, ptr, n=None, keys_size=None, stream=None):
    """tkv_memtable_build[_device] over Columns ``c`` (``ptr(x)`` gives an input's address or None) into an
    Outputs. Returns (rc, n_entries, ikeys_size, first_bad); the scalar outputs start as 0xDEADBEEF."""
    res = [ctypes.c_uint64(0xDEADBEEF) for _ in range(3)]
    n = len(c.key_len) if n is None else n
    ks = len(c.keys) if keys_size is None else keys_size
    tail = () if stream is None else (stream,)
    rc = fn(ptr(c.keys), ks, ptr(c.key_off), ptr(c.key_len), ptr(c.val_off), ptr(c.val_len), ptr(c.op), ptr(c.tomb),
            ptr(c.seq), n, ts, outs.ptr("ikeys"), outs.ikeys_cap, outs.ptr("ikey_off"), outs.ptr("ikey_len"),
            outs.ptr("val_off"), outs.ptr("val_len"), outs.ptr("src"), outs.entry_cap, *[ctypes.byref(r) for r in res], *tail)
    outs.fetch()
    return (rc,) + tuple(r.value for r in res)


def np_ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else None


def assert_matches(outs, exp, rc, m, size, bad, n):
    """A successful call's outputs against the oracle, byte for byte, canaries included."""
    assert (rc, m, size, bad) == (0, exp.src.size, len(exp.ikeys), n)
    for name, want in (("ikey_off", exp.ikey_off), ("ikey_len", exp.ikey_len), ("val_off", exp.val_off),
                       ("val_len", exp.val_len), ("src", exp.src)):
        if name in outs.nulls:
            assert outs.untouched(name), name
            continue
        got = outs.get(name, m)
        assert np.array_equal(got, want), (name, np.flatnonzero(got != want)[:5])
        assert outs.untouched(name, m), f"{name}: a canary was overwritten"
    if "ikeys" in outs.nulls:
        assert outs.untouched("ikeys")
    else:
        got = outs.get("ikeys", size).tobytes()
        if got != exp.ikeys:
            at = next(i for i in range(size) if got[i] != exp.ikeys[i])
            raise AssertionError(f"internal keys differ from byte {at} of {size}")
        assert outs.untouched("ikeys", size), "ikeys: a canary was overwritten"


def assert_untouched(outs):
    for name in OUT_NAMES:
        assert outs.untouched(name), f"{name} was written"
