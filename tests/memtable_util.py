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


# ---- the same oracle in numpy, for lists the dict is too slow for ---------------------------------------

def key_words(c, words=None):
    """The keys of a Columns as big-endian u64 words, zero-padded: an array [words, n]."""
    kl, ko = c.key_len.astype(np.int64), c.key_off.astype(np.int64)
    longest = int(kl.max()) if kl.size else 0
    words = max(1, -(-longest // 8)) if words is None else words
    assert longest <= 8 * words
    raw = c.keys if c.keys.size else np.zeros(1, np.uint8)
    w = np.zeros((words, kl.size), np.uint64)
    for b in range(longest):  # one gather per byte column: no n x 8 index matrix
        byte = np.where(kl > b, np.take(raw, ko + b, mode="clip"), 0).astype(np.uint64)
        w[b // 8] |= byte << np.uint64(8 * (7 - b % 8))
    return w


def np_oracle(c, ts=0, words=None):
    """``oracle`` without a Python loop over the records, for keys of at most 8 * words bytes (default: as
    many words as the longest key needs). Zero-padded words and then the length are the comparator's order:
    two keys with equal padded words differ only in trailing zero bytes, and the shorter is the prefix. The
    index as the last sort key keeps equal keys in log order, so the last of a run is the survivor."""
    n = c.key_len.size
    if c.op is not None:
        bad = np.flatnonzero(c.op > 1)
        if bad.size:
            raise BadOp(int(bad[0]))
    w = key_words(c, words)
    order = np.lexsort((np.arange(n), c.key_len) + tuple(w[::-1]))
    ws, ls = w[:, order], c.key_len[order]
    same_next = np.zeros(n, bool)
    same_next[:-1] = (ls[1:] == ls[:-1]) & (ws[:, 1:] == ws[:, :-1]).all(axis=0)
    keep = ~same_next
    src = order[keep].astype(np.uint32)
    m, width = src.size, 8 * w.shape[0]
    kl = ls[keep].astype(np.int64)
    # one row per entry: the padded key bytes and the 17 metadata bytes; the mask drops the padding, and a
    # boolean index reads row by row: the arena
    row = np.empty((m, width + META), np.uint8)
    row[:, :width] = ws[:, keep].T.astype(">u8", order="C").view(np.uint8).reshape(m, width)
    seq = np.zeros(m, "<u8") if c.seq is None else c.seq[src].astype("<u8")
    row[:, width:width + 8] = seq.view(np.uint8).reshape(m, 8)
    row[:, width + 8:width + 16] = np.full(m, ts, "<u8").view(np.uint8).reshape(m, 8)
    row[:, width + 16] = 0 if c.tomb is None else c.tomb[src] != 0
    mask = np.ones((m, width + META), bool)
    mask[:, :width] = np.arange(width)[None, :] < kl[:, None]
    il = (kl + META).astype(np.uint32)
    io = np.zeros(m, np.uint64)
    if m > 1:
        io[1:] = np.cumsum(il[:-1], dtype=np.uint64)
    vo = np.zeros(m, np.uint64) if c.val_off is None else c.val_off[src].astype(np.uint64)
    vl = np.zeros(m, np.uint32) if c.val_len is None else c.val_len[src].astype(np.uint32)
    if c.op is not None:
        vl = np.where(c.op[src] == 1, 0, vl).astype(np.uint32)
    return Expected(row[mask].tobytes(), io, il, vo, vl, src)


def np_shared_first_word(c):
    """``shared_first_word`` in numpy."""
    long = c.key_len > 8
    _, inv, cnt = np.unique(key_words(c._replace(key_len=np.minimum(c.key_len, 8)), 1)[0][long], return_inverse=True,
                            return_counts=True)
    return int(np.count_nonzero(cnt[inv] > 1))


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


# ---- lists for the rounds past the first, built in numpy (tests/test_gpu_memtable_rounds.py) -------------

def pack(rng, rows, kl):
    """Columns over the keys rows[i, :kl[i]] (a u8 matrix): behind a lead byte, 0-3 junk bytes between
    neighbours, so that key_off (and key_off + 8 r) takes every byte misalignment; random op, tomb, seq
    and value spans (a notional arena, never read)."""
    n, width = rows.shape
    kl = np.asarray(kl, np.uint32)
    step = kl.astype(np.uint64) + rng.integers(0, 4, n).astype(np.uint64)
    ko = np.ones(n, np.uint64)
    ko[1:] += np.cumsum(step[:-1], dtype=np.uint64)
    keys = rng.integers(0, 256, int(ko[-1] + step[-1]) + 1, dtype=np.uint8)
    col = np.arange(width)[None, :]
    for a in range(0, n, 1 << 20):  # by chunks: the index matrix stays small
        b = min(n, a + (1 << 20))
        mask = col < kl[a:b, None]
        keys[(ko[a:b, None].astype(np.int64) + col)[mask]] = rows[a:b][mask]
    vl = rng.integers(0, 9, n).astype(np.uint32)
    vo = np.zeros(n, np.uint64)
    vo[1:] = np.cumsum(vl[:-1], dtype=np.uint64)
    return Columns(keys, ko, kl, vo, vl, rng.integers(0, 2, n, dtype=np.uint8),
                   rng.choice(np.array([0, 0, 1, 1, 2, 0xFF], np.uint8), n), rng.integers(0, 1 << 62, n, dtype=np.uint64))


def word_rows(w):
    """Key bytes of u64 words [n, k]: big-endian, 8 k bytes a row."""
    w = np.ascontiguousarray(w, np.uint64)
    return w.astype(">u8").view(np.uint8).reshape(w.shape[0], 8 * w.shape[1])


def distinct_words(rng, count, top):
    """``count`` distinct random u64 in random order, bit 63 = ``top``."""
    w = np.unique(rng.integers(0, 1 << 63, 2 * count + 16, dtype=np.uint64))
    assert w.size >= count
    return rng.permutation(w)[:count] | np.uint64(top << 63)


def one_pass_case(rng, p, n, longest=8):
    """A list in which only radix pass p tells entries apart. p = 0: keys of 0..longest zero bytes (equal
    words, the digit alone differs; with longest > 8 most keys are longer than 8 bytes, and their second
    round again has only pass 0). p = 1..8: 8-byte keys over one random base in which key byte 8 - p takes
    all 256 values, each many times, in shuffled order."""
    if p == 0:
        kl = rng.integers(0, 9, n)
        if longest > 8:
            kl = np.where(rng.random(n) < 0.6, rng.integers(9, longest + 1, n), kl)
        kl[:longest + 1] = rng.permutation(longest + 1)  # every length occurs
        return pack(rng, np.zeros((n, longest), np.uint8), kl)
    rows = np.tile(rng.integers(0, 256, 8, dtype=np.uint8), (n, 1))
    rows[:, 8 - p] = rng.permutation(n) % 256
    return pack(rng, rows, np.full(n, 8))


FEW_KEYS = (b"", b"k", b"k\0", b"headhead9", b"headheadsecond8!!", b"headheadsecond8!tail")


def few_keys_case(rng, n):
    """(Columns, which): n records over FEW_KEYS in random order; which[i] is record i's key."""
    rows = np.zeros((len(FEW_KEYS), 20), np.uint8)
    for i, k in enumerate(FEW_KEYS):
        rows[i, :len(k)] = np.frombuffer(k, np.uint8)
    which = rng.integers(0, len(FEW_KEYS), n)
    which[:len(FEW_KEYS)] = rng.permutation(len(FEW_KEYS))
    return pack(rng, rows[which], np.array([len(k) for k in FEW_KEYS])[which]), which


def segments_case(rng, heads, each):
    """``heads`` distinct 8-byte heads with ``each`` tails of 1-3 bytes over a small alphabet (some equal),
    which all enter round 2 as ``heads`` segments, shuffled among keys that round 1 resolves: lengths 0-8
    (some equal) and keys of 9-11 bytes with a first word of their own."""
    n2 = heads * each
    fill = max(64, n2 // 16)
    rows = np.zeros((n2 + 2 * fill, 11), np.uint8)
    kl = np.zeros(n2 + 2 * fill, np.int64)
    rows[:n2, :8] = word_rows(np.repeat(distinct_words(rng, heads, 0), each)[:, None])
    rows[:n2, 8:] = np.array([0, 1, 0x80, 0xFF], np.uint8)[rng.integers(0, 4, (n2, 3))]
    kl[:n2] = rng.integers(9, 12, n2)
    rows[n2:n2 + fill, :8] = np.array([0, 0x61, 0xFF], np.uint8)[rng.integers(0, 3, (fill, 8))]
    kl[n2:n2 + fill] = rng.integers(0, 9, fill)
    rows[n2 + fill:, :8] = word_rows(distinct_words(rng, fill, 1)[:, None])
    rows[n2 + fill:, 8:] = rng.integers(0, 256, (fill, 3), dtype=np.uint8)
    kl[n2 + fill:] = rng.integers(9, 12, fill)
    at = rng.permutation(kl.size)
    return pack(rng, rows[at], kl[at])


def tree_case(rng, heads, tile):
    """(Columns, far): 32-byte keys as a tree (``heads`` first words, two second words under each, two third
    under each of those, two fourth under each of those: all of them enter rounds 2, 3 and 4), beside keys
    that end exactly at 8, 16 and 24 bytes of one of them, 33-byte keys in pairs over one of them (a fifth
    round of one byte), all shuffled, and 300 exact copies of keys of 32 and 33 bytes from the first half of
    the log at random places of the second. far = how many of the copies lie in another stretch of ``tile``
    records than their original."""
    n = 8 * heads
    w = np.empty((n, 4), np.uint64)
    w[:, 0] = np.repeat(distinct_words(rng, heads, 0), 8)
    for lv in (1, 2, 3):  # siblings differ in the word's lowest bit at least
        below = 8 >> lv
        w[:, lv] = (np.repeat(rng.integers(0, 1 << 63, n // below, dtype=np.uint64), below) & ~np.uint64(1)) | \
                   np.uint64(1) * ((np.arange(n, dtype=np.uint64) // np.uint64(below)) & np.uint64(1))
    tree = np.zeros((n, 33), np.uint8)
    tree[:, :32] = word_rows(w)
    parts, lens = [tree], [np.full(n, 32)]
    for end in (8, 16, 24):
        parts.append(tree[rng.integers(0, n, 50)])
        lens.append(np.full(50, end))
    over = np.repeat(tree[rng.permutation(n)[:60]], 2, axis=0)
    over[:, 32] = rng.integers(0, 256, 120)
    over[1::2, 32] = over[::2, 32] ^ np.where(rng.random(60) < 0.25, 0, 0x40).astype(np.uint8)  # a quarter: equal pairs
    parts.append(over)
    lens.append(np.full(120, 33))
    at = rng.permutation(n + 270)
    rows, kl = np.concatenate(parts)[at], np.concatenate(lens)[at]
    # the copies: originals from the first half of the log, 100 of them of 33 bytes, copies into the second
    half = kl.size // 2
    long, full = np.flatnonzero(kl[:half] == 33), np.flatnonzero(kl[:half] >= 32)
    orig = np.concatenate([long[rng.integers(0, long.size, 100)], full[rng.integers(0, full.size, 200)]])
    to = np.sort(rng.integers(half, kl.size + 1, 300))
    far = int(np.count_nonzero((to + np.arange(300)) // tile != orig // tile))
    return pack(rng, np.insert(rows, to, rows[orig], axis=0), np.insert(kl, to, kl[orig])), far


def two_tails_case(rng, n):
    """n records (even): n / 2 distinct 8-byte heads with two 1-byte tails each (one pair in eight equal),
    shuffled: every record enters round 2, in n / 2 segments."""
    rows = np.empty((n, 9), np.uint8)
    rows[:, :8] = word_rows(np.repeat(distinct_words(rng, n // 2, 0), 2)[:, None])
    rows[:, 8] = rng.integers(0, 256, n)
    rows[1::2, 8] = np.where(rng.random(n // 2) < 0.125, rows[::2, 8], rows[1::2, 8])
    return pack(rng, rows[rng.permutation(n)], np.full(n, 9))


def four_byte_case(rng, n, values):
    """n 4-byte keys drawn from ``values`` random values: one round of four word passes."""
    pool = rng.integers(0, 1 << 32, values, dtype=np.uint32)
    return pack(rng, pool[rng.integers(0, values, n)].astype(">u4").view(np.uint8).reshape(n, 4), np.full(n, 4))


def np_rounds(c, tile, block):
    """What tkv_memtable_build_device's refinement does with a Columns, restated from DESIGN.md §4.11:
    (sizes, one, many, passes, levels) = the list size of every round and tkv_debug_memtable_passes' four
    words: the passes (bit p) that lists of at most ``tile`` entries run, those that longer lists run, how
    many run in all, and the levels of the deepest histogram scan (``block`` entries per workgroup of a scan
    level, 256 buckets per workgroup of a pass). Round r's entry is {word r of the key, segment << 4 |
    min(key_len - 8 r, 9)}; pass 0 sorts by the 4 digit bits, 1-8 by the word's bytes from the lowest, 9-12
    by the segment's, and runs when its bits differ somewhere in the list. Entries with digit 9 that share
    segment and word with another such entry go on, their segments numbered in sorted order."""
    w, kl = key_words(c), c.key_len.astype(np.int64)
    live, seg = np.arange(kl.size), np.zeros(kl.size, np.uint64)
    sizes, masks, r = [], [0, 0], 0
    while live.size:
        sizes.append(int(live.size))
        word = w[r][live]
        digit = np.minimum(kl[live] - 8 * r, 9).astype(np.uint64)
        kx = (seg << np.uint64(4)) | digit
        dw = int(np.bitwise_or.reduce(word) ^ np.bitwise_and.reduce(word))
        dx = int(np.bitwise_or.reduce(kx) ^ np.bitwise_and.reduce(kx))
        ran = sum(1 << p for p in range(13)
                  if (dx & 15 if p == 0 else (dw >> 8 * (p - 1)) & 255 if p <= 8 else (dx >> 4 + 8 * (p - 9)) & 255))
        masks[live.size > tile] |= ran
        sizes[-1] = (sizes[-1], ran)
        more = np.flatnonzero(digit == 9)
        o = more[np.lexsort((word[more], seg[more]))]
        first = np.ones(o.size, bool)
        first[1:] = (seg[o][1:] != seg[o][:-1]) | (word[o][1:] != word[o][:-1])
        group = np.cumsum(first) - 1
        shared = np.bincount(group, minlength=1)[group] > 1 if o.size else np.zeros(0, bool)
        seg = (np.cumsum(first & shared) - 1)[shared].astype(np.uint64)
        live = live[o][shared]
        r += 1
    deepest = max([scan_levels(256 * -(-s // tile), block) for s, ran in sizes if ran and s > tile], default=0)
    return [s for s, _ in sizes], masks[0], masks[1], sum(bin(m).count("1") for _, m in sizes), deepest


def scan_levels(entries, block):
    """Levels of the shared u64 scan over ``entries`` values: block sums of block sums down to a single one."""
    levels = 1
    while (entries := -(-entries // block)) > 1:
        levels += 1
    return levels


SEGMENT_SHAPES = ("2xT+1", "256x17", "257x17", "65536x2", "65537x2", "257x2")


def segment_shape(shape, tile):
    """(heads, tails per head) of a SEGMENT_SHAPES name."""
    heads, each = shape.split("x")
    return int(heads), tile + 1 if each == "T+1" else int(each)


def rounds_cases(tile, block, small=False):
    """{name: (make, ts)} of the lists above at the sort's geometry: ``tile`` entries per workgroup of a radix
    pass and ``block`` entries per workgroup of a scan level. make() builds the Columns (few_keys and tree
    return a pair). ``small``: the same generators at a few thousand records, for the dict oracle."""
    seed = lambda name: np.random.default_rng([0x526F, sum(name.encode()), len(name)])  # noqa: E731
    cases = {}

    def add(name, fn, *args):
        cases[name] = (lambda: fn(seed(name), *args), 1 + len(cases))

    for p in range(9):
        add(f"one_pass_{p}", one_pass_case, p, 2 * tile + 1)
    add("one_pass_0_len12", one_pass_case, 0, 2 * tile + 1, 12)
    add("few_keys", few_keys_case, 12 * tile + 5)
    for shape in SEGMENT_SHAPES:
        heads, each = segment_shape(shape, tile)
        add(f"segments_{shape}", segments_case, min(heads, 1500 + heads % 2) if small else heads, each)
    add("tree", tree_case, 40 if small else tile // 4 + 76, tile)
    add("two_tails", two_tails_case, block * block + 2)
    add("four_byte", four_byte_case, tile * tile + 1, max(4, tile * tile // 4))
    return cases


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
