"""Sequential oracle of the SSTable merge (tkv_sst_merge[_device]) and the inputs its tests share.

A run is a list of (ikey, value) in the order given; ``columns`` turns runs into the arrays of the C ABI
(``Run``), ``Placed`` puts them into host or device memory and builds the call's pointer tables. ``oracle``
replays the runs in order into a dict keyed by the user key (ikey without its last 17 bytes), so a later run
and a later index overwrite; ``sorted`` over ``bytes`` is the comparator's order (unsigned bytewise, a prefix
first). It does not use tinykvpp_amd.sst's merge.
"""
import collections
import ctypes
import struct

import numpy as np

META = 17
NONE = 2**64 - 1
DROP = 1
MAX_RUNS = 64
FUZZ_SEEDS = 32
PAD = 8
CANARY32, CANARY64 = 0xC7C7C7C7, 0xC7C7C7C7C7C7C7C7
OUT_NAMES = ("key_off", "key_len", "val_off", "val_len", "src")
OK, IO_ERROR, INVALID, CORRUPTED, OVERFLOW = 0, 2, 3, 4, 7

Run = collections.namedtuple("Run", "keys key_off key_len vals val_off val_len")


def ikey(user, seq=0, ts=0, tomb=0):
    return user + struct.pack("<QQB", seq, ts, tomb)


def _arena(items):
    ln = np.array([len(x) for x in items], np.uint32)
    off = np.zeros(len(items), np.uint64)
    if len(items) > 1:
        off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
    return np.frombuffer(b"".join(items), np.uint8).copy(), off, ln


def columns(runs, shared=False, null_vals=()):
    """A Run per run of [(ikey, value)]: an arena pair of its own, or with ``shared`` every run's keys in one
    key arena and values in one value arena (the same array object in every Run). Runs named in ``null_vals``
    get no value columns."""
    out = []
    if shared:
        keys, ko, kl = _arena([k for run in runs for k, _ in run])
        vals, vo, vl = _arena([v for run in runs for _, v in run])
        at = 0
        for run in runs:
            s = slice(at, at + len(run))
            out.append(Run(keys, ko[s].copy(), kl[s].copy(), vals, vo[s].copy(), vl[s].copy()))
            at += len(run)
    else:
        for run in runs:
            keys, ko, kl = _arena([k for k, _ in run])
            vals, vo, vl = _arena([v for _, v in run])
            out.append(Run(keys, ko, kl, vals, vo, vl))
    return [r._replace(vals=None, val_off=None, val_len=None) if i in null_vals else r for i, r in enumerate(out)]


def file_columns(lib, runs, target=256):
    """Runs as views into built file images: every run flushed by the Python writer oracle and taken apart
    again by the host parse with both view flags (tkv_debug_sst_scan_parse, no GPU)."""
    import sst_build_util as bu
    import sst_scan_util as su
    out = []
    for run in runs:
        image = bu.oracle_file(run, target)[0]
        rc, (n, nb, ks, vs, _) = su.call_scan(lib, "tkv_debug_sst_scan_parse", image, 3)
        assert rc in (OK, OVERFLOW) and n == len(run)
        o = su.HostOutputs(n, nb, ks, vs)
        rc, _ = su.call_scan(lib, "tkv_debug_sst_scan_parse", image, 3, o)
        assert rc == OK
        buf = np.frombuffer(image, np.uint8).copy()
        out.append(Run(buf, o.key_off[:n].copy(), o.key_len[:n].copy(), buf, o.val_off[:n].copy(), o.val_len[:n].copy()))
    return out


def run_entries(run):
    """[(ikey, value)] of a Run with sound spans."""
    raw = run.keys.tobytes()
    vraw = b"" if run.vals is None else run.vals.tobytes()
    out = []
    for i in range(run.key_len.size):
        o, ln = int(run.key_off[i]), int(run.key_len[i])
        v = b""
        if run.val_len is not None:
            v = vraw[int(run.val_off[i]):int(run.val_off[i]) + int(run.val_len[i])]
        out.append((raw[o:o + ln], v))
    return out


def oracle(cols, drop=False):
    """[(r, i)] of the survivors in output order."""
    d = {}
    ents = [run_entries(c) for c in cols]
    for r, run in enumerate(ents):
        for i, (k, _) in enumerate(run):
            d[k[:-META]] = (r, i)
    out = [d[u] for u in sorted(d)]
    if drop:
        out = [(r, i) for r, i in out if ents[r][i][0][-1] == 0]
    return out


def first_bad(cols, keys_size=None):
    """The smallest r << 32 | i the contract calls bad, or NONE."""
    for r, c in enumerate(cols):
        size = c.keys.size if keys_size is None else keys_size[r]
        raw = c.keys.tobytes()
        prev = None
        for i in range(c.key_len.size):
            o, ln = int(c.key_off[i]), int(c.key_len[i])
            ok = META <= ln < 2**28 and o + ln <= size
            user = raw[o:o + ln - META] if ok else None
            if not ok or (prev is not None and user < prev):
                return r << 32 | i
            prev = user
    return NONE


class Placed:
    """The Runs in host memory (``device`` None) or on a torch device: every distinct arena (by object) once,
    at byte misalignment ``misalign`` of an allocation; with ``below`` > 0 all arenas lie in ONE allocation,
    ``below`` bytes behind its start, and the key / value base is that start."""

    def __init__(self, cols, device=None, misalign=0, below=0):
        self.cols, self.device, self.keep, self._at = cols, device, [], {}
        arenas = []
        for c in cols:
            for a in (c.keys, c.vals):
                if a is not None and id(a) not in [id(x) for x in arenas]:
                    arenas.append(a)
        if below:
            total = below + sum(a.size + 32 for a in arenas) + misalign
            slab, base = self._alloc(total)
            self.slab_base = base
            at = below + misalign
            for a in arenas:
                self._fill(slab, at, a)
                self._at[id(a)] = base + at
                at += a.size + 16 - (a.size % 16) + misalign % 3
        else:
            self.slab_base = None
            for a in arenas:
                buf, base = self._alloc(a.size + misalign + 1)
                self._fill(buf, misalign, a)
                self._at[id(a)] = base + misalign
        self.k = len(cols)
        self.n = [c.key_len.size for c in cols]
        self.key_addr = [self._at[id(c.keys)] for c in cols]
        self.val_addr = [0 if c.vals is None else self._at[id(c.vals)] for c in cols]
        self.col_addr = [[self._col(x) for x in (c.key_off, c.key_len, c.val_off, c.val_len)] for c in cols]
        live_k = [a for a, n in zip(self.key_addr, self.n) if n]
        live_v = [a for a, n in zip(self.val_addr, self.n) if n and a]
        self.key_base = self.slab_base if below else (min(live_k) if live_k else 0)
        self.val_base = self.slab_base if below else (min(live_v) if live_v else 0)

    def _alloc(self, size):
        if self.device is None:
            buf = np.zeros(size, np.uint8)
            self.keep.append(buf)
            return buf, buf.ctypes.data
        import torch
        buf = torch.zeros(size, dtype=torch.uint8, device=self.device)
        self.keep.append(buf)
        return buf, buf.data_ptr()

    def _fill(self, buf, at, a):
        if self.device is None:
            buf[at:at + a.size] = a
        else:
            import torch
            buf[at:at + a.size].copy_(torch.from_numpy(a))

    def _col(self, a):
        if a is None or a.size == 0:
            return 0
        if self.device is None:
            a = np.ascontiguousarray(a)
            self.keep.append(a)
            return a.ctypes.data
        import torch
        t = torch.from_numpy(a.view(a.dtype.str.replace("u", "i"))).to(self.device)
        self.keep.append(t)
        return t.data_ptr()

    def bias(self):
        return [a - self.val_base if a and n else 0 for a, n in zip(self.val_addr, self.n)]

    def tables(self, keys_size=None, n=None, bias=True):
        """The per-run host arrays of the call: d_keys, keys_size, key_off, key_len, val_off, val_len, n,
        val_bias (None when ``bias`` is False)."""
        k = max(self.k, 1)
        vp, u64 = ctypes.c_void_p, ctypes.c_uint64
        size = [c.keys.size for c in self.cols] if keys_size is None else keys_size
        t = [(vp * k)(*[a or None for a in self.key_addr]), (u64 * k)(*size)]
        for j in range(4):
            t.append((vp * k)(*[row[j] or None for row in self.col_addr]))
        t.append((u64 * k)(*(self.n if n is None else n)))
        t.append((u64 * k)(*self.bias()) if bias else None)
        return t


def expected(placed, src, bias=True):
    """What the call must write for the survivors ``src`` [(r, i)]."""
    cols = placed.cols
    ko = np.array([placed.key_addr[r] - placed.key_base + int(cols[r].key_off[i]) for r, i in src], np.uint64)
    kl = np.array([cols[r].key_len[i] for r, i in src], np.uint32)
    b = placed.bias() if bias else [0] * placed.k
    vo = np.array([b[r] + (0 if cols[r].val_off is None else int(cols[r].val_off[i])) for r, i in src], np.uint64)
    vl = np.array([0 if cols[r].val_len is None else cols[r].val_len[i] for r, i in src], np.uint32)
    s = np.array([r << 32 | i for r, i in src], np.uint64)
    return {"key_off": ko, "key_len": kl, "val_off": vo, "val_len": vl, "src": s}


class Outputs:
    """Output columns for one call: ``entry_cap`` entries each with canaries on both sides; names in
    ``nulls`` are passed as NULL."""
    DT = {"key_off": np.uint64, "key_len": np.uint32, "val_off": np.uint64, "val_len": np.uint32, "src": np.uint64}

    def __init__(self, entry_cap, nulls=(), device=None):
        self.entry_cap, self.nulls, self.dev = entry_cap, set(nulls), None
        self.host = {k: np.full(entry_cap + 2 * PAD, CANARY64 if dt == np.uint64 else CANARY32, dt) for k, dt in self.DT.items()}
        if device is not None:
            import torch
            self.dev = {k: torch.from_numpy(v.view(v.dtype.str.replace("u", "i"))).to(device) for k, v in self.host.items()}

    def ptr(self, name):
        if name in self.nulls:
            return None
        a = self.host[name]
        base = self.dev[name].data_ptr() if self.dev is not None else a.ctypes.data
        return ctypes.c_void_p(base + PAD * a.itemsize)

    def fetch(self):
        if self.dev is not None:
            for k, v in self.dev.items():
                self.host[k] = v.cpu().numpy().view(self.DT[k])

    def get(self, name, count):
        return self.host[name][PAD:PAD + count]

    def untouched(self, name, written=0):
        a = self.host[name]
        can = a.dtype.type(CANARY64 if a.itemsize == 8 else CANARY32)
        return bool((a[:PAD] == can).all() and (a[PAD + written:] == can).all())


def call(fn, placed, flags, outs, key_base=None, bias=True, k=None, tail=(), tables=None):
    """tkv_sst_merge[_device] over a Placed into an Outputs. Returns (rc, n_entries, keys_bytes, vals_bytes,
    first_bad); the scalar outputs start as 0xDEADBEEF. ``tail`` = the trailing arguments (the stream)."""
    res = [ctypes.c_uint64(0xDEADBEEF) for _ in range(4)]
    t = placed.tables(bias=bias) if tables is None else tables
    kb = placed.key_base if key_base is None else key_base
    rc = fn(placed.k if k is None else k, *t[:7], ctypes.c_void_p(kb) if kb else None, t[7], flags,
            *[outs.ptr(name) for name in OUT_NAMES], outs.entry_cap, *[ctypes.byref(r) for r in res], *tail)
    outs.fetch()
    return (rc,) + tuple(r.value for r in res)


def assert_untouched(outs):
    for name in OUT_NAMES:
        assert outs.untouched(name), f"{name} was written"


def check_merge(fn, cols, flags=0, device=None, misalign=0, below=0, nulls=(), bias=True, tail=(), also=None):
    """Sizing call and merge of ``cols`` through ``fn`` against the oracle, canaries included; ``also`` is a
    second entry point (the host call) whose columns must agree bit for bit. Returns the survivors."""
    src = oracle(cols, bool(flags & DROP))
    placed = Placed(cols, device, misalign, below)
    want = expected(placed, src, bias)
    kb = int(want["key_len"].astype(np.uint64).sum())
    vb = int(want["val_len"].astype(np.uint64).sum())
    total = sum(placed.n)
    sizing = Outputs(0, nulls=OUT_NAMES, device=device)
    assert call(fn, placed, flags, sizing, bias=bias, tail=tail) == (OK, len(src), kb, vb, NONE)
    outs = Outputs(len(src), nulls=nulls, device=device)
    assert call(fn, placed, flags, outs, bias=bias, tail=tail) == (OK, len(src), kb, vb, NONE)
    for name in OUT_NAMES:
        if name in outs.nulls:
            assert outs.untouched(name), name
            continue
        got = outs.get(name, len(src))
        assert np.array_equal(got, want[name]), (name, np.flatnonzero(got != want[name])[:5], total)
        assert outs.untouched(name, len(src)), f"{name}: a canary was overwritten"
    if also is not None:
        hp = Placed(cols)
        ho = Outputs(len(src))
        assert call(also, hp, flags, ho, bias=bias) == (OK, len(src), kb, vb, NONE)
        for name in ("key_len", "val_len", "src"):
            if name not in outs.nulls:
                assert np.array_equal(ho.get(name, len(src)), outs.get(name, len(src))), name
    return src


# ---- cases ----------------------------------------------------------------------------------------------

def distinct_keys(rng, n, lo=1, hi=12, alpha=256):
    """n distinct user keys, sorted."""
    seen = set()
    while len(seen) < n:
        ln = int(rng.integers(lo, hi + 1))
        seen.add(rng.integers(0, alpha, ln, dtype=np.uint8).tobytes() if alpha < 256 else rng.bytes(ln))
    return sorted(seen)


def make_run(keys, r, tomb=0, seq=None, ts=None):
    """A run over sorted user keys: seq counts down in newer runs by default (so that "highest seq" would
    pick the wrong entry), the value names the entry."""
    return [(ikey(k, (10**6 - 1000 * r + i) if seq is None else seq, r if ts is None else ts,
                  tomb[i] if isinstance(tomb, (list, tuple, np.ndarray)) else tomb), b"r%d.%d" % (r, i))
            for i, k in enumerate(keys)]


def overlapping(rng, sizes, **kw):
    """Runs of the given sizes over one pool of keys, so that about half the keys of a run occur elsewhere."""
    pool = distinct_keys(rng, max(sizes) + sum(sizes) // 3 + 1, **kw)
    return [make_run(sorted(pool[j] for j in rng.choice(len(pool), n, replace=False)), r) for r, n in enumerate(sizes)]


def count_cases(T):
    """K = 2 around the tile T: the sizes and the shapes of the issue."""
    rng = np.random.default_rng(21)
    cases = {}
    for n0 in (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1):
        for n1 in (1, 64, T + 1):
            cases[f"counts_{n0}_{n1}"] = overlapping(rng, [n0, n1])
            cases[f"counts_{n1}_{n0}"] = overlapping(rng, [n1, n0])
    cases["counts_3T+5_1"] = overlapping(rng, [3 * T + 5, 1])
    ks = distinct_keys(rng, 2 * T + 10)
    half = len(ks) // 2
    cases["below"] = [make_run(ks[:half], 0), make_run(ks[half:], 1)]
    cases["above"] = [make_run(ks[half:], 0), make_run(ks[:half], 1)]
    cases["interleaved"] = [make_run(ks[::2], 0), make_run(ks[1::2], 1)]
    cases["identical"] = [make_run(ks[:T + 3], 0), make_run(ks[:T + 3], 1)]
    return cases


def tie_cases(T):
    """Groups of equal keys across the output's tile boundary and the split of either input."""
    rng = np.random.default_rng(22)
    ks = distinct_keys(rng, 2 * T, lo=9, hi=14)  # longer than a word: some ties need the full compare
    cases = {}
    for a, b in ((3, 3), (5, 4), (1, 7)):
        # T - a keys in front, then key X a times in run 0 and b times in run 1: X's group lies around output T
        front, x, back = ks[:T - a], ks[T], ks[T + 1:T + 40]
        cases[f"straddle_{a}_{b}"] = [make_run(front[::2] + [x] * a + back[::2], 0),
                                      make_run(front[1::2] + [x] * b + back[1::2], 1)]
    cases["all_equal"] = [make_run([b"the-one-key!"] * (T + 1), 0), make_run([b"the-one-key!"] * (T + 1), 1)]
    cases["all_equal_short"] = [make_run([b"k"] * (T + 1), 0), make_run([b"k"] * (T + 1), 1)]
    return cases


def comparator_cases():
    import memtable_util as mu
    cases = {}
    for name, recs in mu.order_cases().items():
        ks = sorted(set(r[2] for r in recs))
        cases[f"order_{name}_parity"] = [make_run(ks[::2], 0), make_run(ks[1::2], 1), make_run(ks[::3], 2)]
        cases[f"order_{name}_halves"] = [make_run(ks[len(ks) // 2:], 0), make_run(ks[:len(ks) // 2], 1)]
    head = b"HEADhead"
    for at in (8, 9, 15, 16, 17):
        body = bytearray(head + bytes(range(0x40, 0x40 + 12)))
        ks = []
        for v in (0x00, 0x41, 0x80, 0xFF):
            body[at] = v
            ks.append(bytes(body))
        ks = sorted(set(ks))
        cases[f"differs_at_{at}"] = [make_run(ks[1::2], 0), make_run(ks[::2], 1), make_run(ks[:1] + ks[-1:], 2)]
    rng = np.random.default_rng(23)
    long = rng.bytes(999)
    ks = sorted(long + bytes([b]) for b in rng.permutation(256)[:40].tolist())
    cases["differs_at_999"] = [make_run(ks[::2], 0), make_run(ks[1::2], 1), make_run(ks[5:25], 2)]
    cases["a_vs_a0"] = [make_run([b"a", b"b"], 0), make_run([b"a\x00"], 1), make_run([b"", b"a\x00\x00"], 2)]
    cases["empty_user_key"] = [make_run([b"", b"x"], 0), make_run([b""], 1), make_run([b"", b"", b"y"], 2)]
    # metadata that would sort the other way: the older run has the high seq and 0xFF timestamps
    cases["metadata_no_part"] = [
        [(ikey(b"k1", 2**64 - 1, 2**64 - 1, 0), b"old"), (ikey(b"k2", 2**63, 2**64 - 1, 0xFF), b"old2")],
        [(ikey(b"k1", 0, 0, 0), b"new"), (ikey(b"k2", 1, 0, 0), b"new2")]]
    return cases


def k_cases(T):
    rng = np.random.default_rng(24)
    cases = {"k1_identity": overlapping(rng, [T + 7])}
    ks = distinct_keys(rng, 300)
    cases["k1_dedupe"] = [make_run(sorted(ks + ks[::3] + ks[::7]), 0)]
    for k in (3, 5, 8, 9):
        cases[f"k{k}"] = overlapping(rng, [int(x) for x in rng.integers(1, T, k)])
    cases["k5_some_empty"] = overlapping(rng, [0, T // 2, 0, 77, 0])
    cases["k8_empty_ends"] = overlapping(rng, [0, 0, 40, T + 1, 0, 9, 300, 0])
    cases["k64"] = overlapping(rng, [int(x) for x in np.where(rng.random(64) < 0.3, 0, rng.integers(1, 120, 64))])
    cases["k64_one_live"] = overlapping(rng, [0] * 40 + [55] + [0] * 23)
    return cases


def duplicate_cases():
    rng = np.random.default_rng(25)
    ks = distinct_keys(rng, 200, alpha=3, hi=10)
    dup = sorted(ks + ks[::2] + ks[::5] + ks[:20] * 3)
    return {"in_run_dups": [make_run(dup, 0), make_run(sorted(ks[::3] * 2), 1)],
            "old_dups_shadowed": [make_run(sorted(ks[:50] * 4), 0), make_run(ks[:50:2], 1)]}


def tombstone_cases():
    rng = np.random.default_rng(26)
    ks = distinct_keys(rng, 120)
    t = rng.choice(np.array([0, 0, 1, 2, 0xFF]), 120).tolist()
    return {
        "tomb_over_puts": [make_run(ks, 0), make_run(ks[::2], 1, tomb=1)],
        "put_over_tomb": [make_run(ks, 0, tomb=1), make_run(ks[::3], 1)],
        "tomb_byte_2": [make_run(ks[:10], 0), make_run(ks[:10:2], 1, tomb=2)],
        "tomb_mixed": [make_run(ks, 0, tomb=t), make_run(ks[10:90], 1, tomb=t[10:90][::-1]), make_run(ks[::4], 2, tomb=t[::4])],
        "all_tombstones": [make_run(ks, 0), make_run(ks, 1, tomb=0xFF)],
    }


def named_cases(T):
    cases = {}
    for part in (count_cases(T), tie_cases(T), comparator_cases(), k_cases(T), duplicate_cases(), tombstone_cases()):
        cases.update(part)
    return cases


def fuzz_case(seed, n_max=3000):
    """(runs, drop): K in 1..8, n[r] in 0..n_max, key lengths 0..40 over a small alphabet, random tombstones."""
    rng = np.random.default_rng(0x4D47 + seed)
    k = int(rng.integers(1, 9))
    alpha = np.array([0x00, 0x01, 0x61, 0x62, 0x7F, 0x80, 0xFF][:int(rng.integers(2, 8))], np.uint8)
    stem = alpha[rng.integers(0, alpha.size, 40)].tobytes()
    runs = []
    for r in range(k):
        n = int(rng.integers(0, n_max + 1)) if rng.random() < 0.85 else 0
        lens = np.where(rng.random(n) < 0.6, rng.integers(0, 8, n), rng.integers(0, 41, n))
        ks = []
        for ln in lens.tolist():
            cut = int(rng.integers(0, ln + 1)) if rng.random() < 0.5 else 0
            ks.append(stem[:cut] + alpha[rng.integers(0, alpha.size, ln - cut)].tobytes())
        ks.sort()
        runs.append(make_run(ks, r, tomb=rng.choice(np.array([0, 0, 0, 1, 2, 0xFF]), n).tolist(),
                             seq=int(rng.integers(0, 1 << 62))))
    return runs, bool(rng.integers(0, 2))


def corrupt(cols, r, i, kind):
    """A copy of the Runs with entry i of run r made bad; returns (cols, keys_size)."""
    cols = [c._replace(key_off=c.key_off.copy(), key_len=c.key_len.copy()) for c in cols]
    size = [c.keys.size for c in cols]
    c = cols[r]
    if kind == "short":
        c.key_len[i] = 16
    elif kind == "huge":
        c.key_len[i] = 2**28
    elif kind == "past_end":
        c.key_off[i] = size[r] - int(c.key_len[i]) + 1
    elif kind == "off_wraps":
        c.key_off[i] = 2**64 - 8
    elif kind == "order":
        j = i - 1 if i > 0 else 1  # swap with a neighbour that has another user key
        a, b = (j, i) if j < i else (i, j)
        assert run_entries(c)[a][0][:-META] != run_entries(c)[b][0][:-META]
        c.key_off[[a, b]] = c.key_off[[b, a]]
        c.key_len[[a, b]] = c.key_len[[b, a]]
    else:
        raise KeyError(kind)
    return cols, size


CORRUPT_KINDS = ("short", "huge", "past_end", "off_wraps", "order")
