"""Sequential oracle of the SSTable get (tkv_sst_get[_device]) and what its tests share.

``oracle`` replays the concatenated runs in order into a dict keyed by the user key (ikey without its last 17
bytes), so a later run and a later index overwrite, and answers every query from that dict: state, hit, seq
and value. ``search_model`` is the contract's probe sequence restated entry by entry; it says which entries a
call reads, which is what decides TKV_CORRUPTED and *first_bad. Runs, placement and case builders are
sst_merge_util's (``ikey``, ``columns``, ``Placed``, ``make_run``, ``comparator_cases``); ``Queries`` places a
query batch, ``Outputs`` the output columns and the value arena between canaries, ``check_get`` holds a call
against the oracle. It does not use tinykvpp_amd.sst's get.
"""
import ctypes

import numpy as np

import sst_merge_util as gu
from sst_merge_util import CANARY32, CANARY64, META, NONE, OK, PAD

ABSENT, FOUND, DELETED = 0, 1, 2
FUZZ_SEEDS = 32
COLS = ("state", "src", "seq", "val_off", "val_len", "val_pos")
DT = {"state": np.uint8, "src": np.uint64, "seq": np.uint64, "val_off": np.uint64, "val_len": np.uint32, "val_pos": np.uint64}
CANARY = {1: 0xC7, 4: CANARY32, 8: CANARY64}
VPAD = 48  # canary bytes on either side of the value arena


def oracle(cols, queries):
    """Per query (state, r, i, seq, value): r, i None when absent; value b"" unless found."""
    d = {}
    ents = [gu.run_entries(c) for c in cols]
    for r, run in enumerate(ents):
        for i, (k, _) in enumerate(run):
            d[k[:-META]] = (r, i)
    out = []
    for q in queries:
        if q not in d:
            out.append((ABSENT, None, None, 0, b""))
            continue
        r, i = d[q]
        k, v = ents[r][i]
        seq = int.from_bytes(k[-META:-META + 8], "little")
        out.append((DELETED, r, i, seq, b"") if k[-1] else (FOUND, r, i, seq, v))
    return out


def search_model(cols, queries, keys_size=None, vals_size=None):
    """The contract's search: per run, newest first, pos = 0; for step = 2^(b - 1) .. 1 (b = n.bit_length()):
    entry pos + step - 1 is probed when pos + step <= n. Returns (first_bad, hits, steps): the smallest
    r << 32 | i that was read and failed (NONE), [(r, i) or None] per query, and the most steps a query
    made. ``vals_size`` (a list) switches the value span check of found hits on."""
    bad, hits, most = NONE, [], 0
    raws = [c.keys.tobytes() for c in cols]
    for q in queries:
        hit, steps, stop = None, 0, False
        for r in reversed(range(len(cols))):
            c = cols[r]
            n = c.key_len.size
            if n == 0:
                continue
            size = c.keys.size if keys_size is None else keys_size[r]
            steps += n.bit_length()
            pos, eq, step = 0, False, 1 << (n.bit_length() - 1)
            while step and not stop:
                cand = pos + step
                step >>= 1
                if cand > n:
                    continue
                o, ln = int(c.key_off[cand - 1]), int(c.key_len[cand - 1])
                if not (META <= ln < 2**28 and o + ln <= size):
                    bad, stop = min(bad, r << 32 | (cand - 1)), True
                    break
                user = raws[r][o:o + ln - META]
                if user <= q:
                    pos, eq = cand, user == q
            if stop:
                break
            if eq:
                i = pos - 1
                o, ln = int(c.key_off[i]), int(c.key_len[i])
                if raws[r][o + ln - 1] == 0 and vals_size is not None:
                    vo = 0 if c.val_off is None else int(c.val_off[i])
                    vl = 0 if c.val_len is None else int(c.val_len[i])
                    if vo + vl > vals_size[r]:
                        bad, stop = min(bad, r << 32 | i), True
                        break
                hit = (r, i)
                break
        hits.append(None if stop else hit)
        most = max(most, steps)
    return bad, hits, most


def steps_of(sizes):
    """The steps a query makes that searches runs of these sizes: the sum of ceil(log2(n + 1))."""
    return sum(int(n).bit_length() for n in sizes)


class Queries:
    """A batch of user keys as (arena, off, len) in host memory or on a torch device, the arena ``misalign``
    bytes into an allocation of exactly misalign + its size (+ 1 so that an empty arena has an address)."""

    def __init__(self, keys, device=None, misalign=0, arena=None, off=None):
        self.keys, self.keep = list(keys), []
        ln = np.array([len(k) for k in self.keys], np.uint32)
        if arena is None:
            arena, off, _ = gu._arena(self.keys) if self.keys else (np.zeros(0, np.uint8), np.zeros(0, np.uint64), None)
        self.size, self.nq = arena.size, len(self.keys)
        if device is None:
            buf = np.zeros(arena.size + misalign + 1, np.uint8)
            buf[misalign:misalign + arena.size] = arena
            off, ln = np.ascontiguousarray(off, np.uint64), np.ascontiguousarray(ln)
            self.keep += [buf, off, ln]
            self.addr, self.off_addr, self.len_addr = buf.ctypes.data + misalign, off.ctypes.data, ln.ctypes.data
        else:
            import torch
            buf = torch.zeros(arena.size + misalign + 1, dtype=torch.uint8, device=device)
            buf[misalign:misalign + arena.size].copy_(torch.from_numpy(arena))
            o = torch.from_numpy(np.ascontiguousarray(off, np.uint64).view(np.int64)).to(device)
            n = torch.from_numpy(ln.view(np.int32)).to(device)
            self.keep += [buf, o, n]
            self.addr, self.off_addr, self.len_addr = buf.data_ptr() + misalign, o.data_ptr(), n.data_ptr()

    def args(self, size=None, nq=None):
        vp = ctypes.c_void_p
        return [vp(self.addr), self.size if size is None else size, vp(self.off_addr) if self.nq else None,
                vp(self.len_addr) if self.nq else None, self.nq if nq is None else nq]


def expected(placed, answers, bias=True):
    """What the call must write for ``answers`` (the oracle's): the six columns, the value arena, n_found."""
    b = placed.bias() if bias else [0] * placed.k
    cols = placed.cols
    state = np.array([a[0] for a in answers], np.uint8)
    src = np.array([NONE if a[1] is None else a[1] << 32 | a[2] for a in answers], np.uint64)
    seq = np.array([a[3] for a in answers], np.uint64)
    vo = np.array([b[a[1]] + (0 if cols[a[1]].val_off is None else int(cols[a[1]].val_off[a[2]])) if a[0] == FOUND else 0
                   for a in answers], np.uint64)
    vl = np.array([len(a[4]) for a in answers], np.uint32)
    pos = np.zeros(len(answers), np.uint64)
    if len(answers) > 1:
        pos[1:] = np.cumsum(vl[:-1], dtype=np.uint64)
    return ({"state": state, "src": src, "seq": seq, "val_off": vo, "val_len": vl, "val_pos": pos},
            b"".join(a[4] for a in answers), int((state == FOUND).sum()))


class Outputs:
    """The six per-query columns of ``nq`` entries and a value arena of ``vals_cap`` bytes at byte phase
    ``phase`` of a 16-byte granule, each with canaries on both sides; names in ``nulls`` ("vals" too) are
    passed as NULL."""

    def __init__(self, nq, vals_cap=0, nulls=(), device=None, phase=0):
        self.nq, self.vals_cap, self.nulls, self.dev, self.phase = nq, vals_cap, set(nulls), None, phase
        self.host = {k: np.full(nq + 2 * PAD, CANARY[np.dtype(dt).itemsize], dt) for k, dt in DT.items()}
        self.host["vals"] = np.full(VPAD + 16 + vals_cap + VPAD, 0xC7, np.uint8)
        if device is not None:
            import torch
            self.dev = {k: torch.from_numpy(v.view(v.dtype.str.replace("u", "i")) if v.itemsize > 1 else v).to(device)
                        for k, v in self.host.items()}
        base = self._base("vals")
        self.vat = VPAD + (phase - (base + VPAD)) % 16  # index of the arena's first byte

    def _base(self, name):
        return self.dev[name].data_ptr() if self.dev is not None else self.host[name].ctypes.data

    def ptr(self, name):
        if name in self.nulls:
            return None
        if name == "vals":
            return ctypes.c_void_p(self._base("vals") + self.vat)
        return ctypes.c_void_p(self._base(name) + PAD * self.host[name].itemsize)

    def fetch(self):
        if self.dev is not None:
            for k, v in self.dev.items():
                self.host[k] = v.cpu().numpy().view(np.uint8 if k == "vals" else DT[k])

    def get(self, name, count):
        if name == "vals":
            return self.host["vals"][self.vat:self.vat + count].tobytes()
        return self.host[name][PAD:PAD + count]

    def untouched(self, name, written=0):
        a = self.host[name]
        at = self.vat if name == "vals" else PAD
        can = a.dtype.type(CANARY[a.itemsize])
        return bool((a[:at] == can).all() and (a[at + written:] == can).all())


def call(fn, placed, q, outs, gather=True, bias=True, tail=(), tables=None, vals_size=None, k=None, flags=0, qargs=None):
    """tkv_sst_get[_device]. Returns (rc, n_found, vals_bytes, first_bad); the scalars start as 0xDEADBEEF."""
    res = [ctypes.c_uint64(0xDEADBEEF) for _ in range(3)]
    t = placed.tables(bias=bias) if tables is None else tables
    kk = max(placed.k, 1)
    vals = (ctypes.c_void_p * kk)(*[a or None for a in placed.val_addr]) if gather else None
    if vals_size is None:
        vals_size = [0 if c.vals is None else c.vals.size for c in placed.cols]
    vsize = (ctypes.c_uint64 * kk)(*vals_size) if gather else None
    qa = q.args() if qargs is None else qargs
    rc = fn(placed.k if k is None else k, *t[:7], vals, vsize, t[7], *qa, flags, *[outs.ptr(name) for name in COLS],
            outs.ptr("vals"), outs.vals_cap, *[ctypes.byref(r) for r in res], *tail)
    outs.fetch()
    return (rc,) + tuple(r.value for r in res)


def assert_untouched(outs):
    for name in COLS + ("vals",):
        assert outs.untouched(name), f"{name} was written"


def check_get(fn, cols, queries, device=None, misalign=0, qmisalign=0, phase=0, gather=True, nulls=(), bias=True, tail=(),
              also=None, placed=None):
    """Sizing call and get of ``queries`` over ``cols`` through ``fn`` against the oracle, canaries
    included; ``also`` is a second entry point (the host call) that must pass the same check. Returns the
    oracle's answers."""
    answers = oracle(cols, queries)
    placed = gu.Placed(cols, device, misalign) if placed is None else placed
    q = Queries(queries, device, qmisalign)
    want, vals, found = expected(placed, answers, bias)
    nq = len(queries)
    asked = set(nulls)
    nulls = asked if gather else asked | {"vals", "val_pos"}  # (both need the value arenas)
    sizing = Outputs(0, 0, nulls=COLS + ("vals",), device=device)
    assert call(fn, placed, q, sizing, gather, bias, tail) == (OK, found, len(vals), NONE)
    outs = Outputs(nq, len(vals), nulls=nulls, device=device, phase=phase)
    assert call(fn, placed, q, outs, gather, bias, tail) == (OK, found, len(vals), NONE)
    for name in COLS:
        if name in outs.nulls:
            assert outs.untouched(name), name
            continue
        got = outs.get(name, nq)
        assert np.array_equal(got, want[name]), (name, np.flatnonzero(got != want[name])[:5], nq)
        assert outs.untouched(name, nq), f"{name}: a canary was overwritten"
    if "vals" in outs.nulls:
        assert outs.untouched("vals")
    else:
        got = outs.get("vals", len(vals))
        assert got == vals, next(i for i in range(len(vals)) if got[i] != vals[i])
        assert outs.untouched("vals", len(vals)), "vals: a canary was overwritten"
    if also is not None:
        check_get(also, cols, queries, gather=gather, nulls=asked, bias=bias)
    return answers


# ---- cases ----------------------------------------------------------------------------------------------

def users_of(runs):
    return sorted({k[:-META] for run in runs for k, _ in run})


def between(a, b):
    """A key strictly between neighbours a < b in the comparator's order, or None when there is none
    (b == a + b"\\0")."""
    c = a + b"\x00"
    return c if c < b else None


def edge_queries(runs):
    """Every present key, a key below the first, one above the last, one between each pair of neighbours."""
    ks = users_of(runs)
    out = list(ks)
    if ks:
        if ks[0] != b"":
            out.append(ks[0][:-1] if len(ks[0]) > 1 else b"")
            if out[-1] in ks:
                out.pop()
        out.append(ks[-1] + b"\xff")
        for a, b in zip(ks, ks[1:]):
            c = between(a, b)
            if c is not None:
                out.append(c)
    return out


def valued_run(keys, r, sizes=None, tomb=0):
    """make_run with values of the given sizes (a pattern that names run, index and byte)."""
    run = gu.make_run(keys, r, tomb=tomb)
    if sizes is None:
        return run
    return [(k, bytes((r * 31 + i * 7 + b) & 0xFF for b in range(sizes[i % len(sizes)]))) for i, (k, _) in enumerate(run)]


def named_cases():
    """name -> (runs, queries): hand-sized shapes of the lookup rule (the golden file holds these)."""
    cases = {}
    ks = [b"apple", b"banana", b"cherry", b"damson", b"elder"]
    cases["one_run"] = ([gu.make_run(ks, 0)], ks + [b"", b"a", b"apple\x00", b"zebra", b"banan"])
    cases["newest_wins"] = ([gu.make_run(ks, 0), gu.make_run(ks[1:4], 1), gu.make_run(ks[2:3], 2)], ks)
    cases["tomb_over_put"] = ([gu.make_run(ks, 0), gu.make_run(ks[::2], 1, tomb=1)], ks + [b"fig"])
    cases["put_over_tomb"] = ([gu.make_run(ks, 0, tomb=1), gu.make_run(ks[1::2], 1)], ks)
    cases["tomb_byte_ff"] = ([gu.make_run(ks[:2], 0), gu.make_run(ks[:1], 1, tomb=0xFF)], ks[:2])
    cases["dups_in_run"] = ([gu.make_run([b"a", b"b", b"b", b"b", b"c", b"c"], 0)], [b"a", b"b", b"c", b"bb"])
    cases["dup_tomb_last"] = ([[(gu.ikey(b"k", 5, 0, 0), b"v1"), (gu.ikey(b"k", 6, 0, 1), b"v2")]], [b"k"])
    cases["dup_put_last"] = ([[(gu.ikey(b"k", 5, 0, 1), b"v1"), (gu.ikey(b"k", 6, 0, 0), b"v2")]], [b"k"])
    cases["empty_runs_between"] = ([[], gu.make_run(ks, 1), [], gu.make_run(ks[:1], 3), []], ks)
    cases["empty_user_key"] = ([gu.make_run([b"", b"x"], 0), gu.make_run([b""], 1, tomb=1)], [b"", b"x", b"\x00"])
    cases["prefixes"] = ([gu.make_run([b"a", b"a\x00", b"a\x00\x00", b"a\x01", b"\x80"], 0)],
                         [b"", b"a", b"a\x00", b"a\x00\x00", b"a\x00\x00\x00", b"a\x01", b"\x7f", b"\x80", b"\x80\x00"])
    cases["seq_no_part"] = ([[(gu.ikey(b"k1", 2**64 - 1, 2**64 - 1, 0), b"old")], [(gu.ikey(b"k1", 0, 0, 0), b"new")]], [b"k1"])
    cases["same_key_many_times"] = ([gu.make_run(ks, 0)], [b"cherry"] * 5 + [b"nope"] * 2 + [b"apple"])
    cases["no_runs"] = ([], [b"a", b""])
    return cases


def comparator_cases():
    """sst_merge_util.comparator_cases with queries: every present key, every proper prefix of some and an
    extension of each."""
    cases = {}
    for name, runs in gu.comparator_cases().items():
        ks = users_of(runs)
        qs = list(ks) + [k + b"\x00" for k in ks[:40]] + [k[:-1] for k in ks[:40] if k] + [k[:8] for k in ks[:8]] + \
            [k[:7] for k in ks[:8]] + [k[:9] for k in ks[:8]]
        cases[name] = (runs, qs + edge_queries(runs)[len(ks):][:60])
    head = b"HEADhead"
    ks = sorted(head[:7] + bytes([x]) * (ln - 7) for ln in (7, 8, 9, 16, 17) for x in (0x00, 0x41))
    ks = sorted(set(ks))
    cases["word_ties_7_8_9_16_17"] = ([gu.make_run(ks[::2], 0), gu.make_run(ks[1::2], 1)], ks + [k + b"\x00" for k in ks] + [head[:6], head])
    return cases


def duplicate_cases():
    """Groups of 2, 64, 65 and 300 equal user keys inside one run, slid across every pivot position: the
    run is lead fill keys + [x] * g + 9 tail keys for every lead in 0..129, so that the pivots of every step
    (2^k - 1 and the sums the search reaches from there) land on the first, an interior and the last element
    of the group and on both neighbours; the highest index must be the hit."""
    cases = {}
    fill = [b"f%04d" % i for i in range(130)]
    tail = [b"z%04d" % i for i in range(9)]
    for g in (2, 64, 65, 300):
        for lead in range(130):
            run = gu.make_run(fill[:lead] + [b"k-dup"] * g + tail, 0)
            cases[f"dup_{g}_lead_{lead}"] = ([run], [b"k-dup", b"k-du", b"k-dup\x00"] + fill[:lead][-2:] + tail[:2])
    return cases


def fuzz_case(seed, n_max=600):
    """(runs, queries) over sst_merge_util.fuzz_case: every user key of the union and as many absent keys."""
    runs, _ = gu.fuzz_case(seed, n_max)
    rng = np.random.default_rng(0x6E7 + seed)
    ks = users_of(runs)
    have = set(ks)
    absent = []
    for k in ks:
        c = k + bytes([int(rng.integers(0, 256))]) if rng.random() < 0.5 else k[:int(rng.integers(0, len(k) + 1))]
        if c not in have:
            absent.append(c)
    qs = ks + absent
    order = rng.permutation(len(qs))
    return runs, [qs[j] for j in order]
