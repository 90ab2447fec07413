"""Random WAL images with one mutation each, and everything the device pipeline (index -> record check ->
decode -> encode) and the host entries must make of them. Numpy and the test oracle only: no GPU, no
product library. The expected values come from the sequential decode written here (`decode`: the
record_len chain in Python integers, CRCs from oracle.batch, the key/value bounds; wal.cpp:63-121) and
from the numpy restatements next to it (`records_expected`, wal_decode_util.expected).

case(seed, oracle) draws, in this order: a length profile, a record count, the image's shift inside its
buffer, the records, and one mutation (seed % 8) of a victim record ((seed // 8) % 8 == 0: record 0,
== 1: the last record, else random). The profiles sit on the kernels' own constants, named below and
compared with the tkv_debug_*_geometry calls in test_wal_fuzz_cpu.py.
"""
import os
import sys
import types

import numpy as np

import wal_decode_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

META = 26            # kWalMeta: the header; record_len counts the bytes behind its first 8
LANE_PIECE = 112     # kPiece: image bytes per lane of a sweep / index region
SHORT_SPAN = 64      # kShortSpan: keys / values up to this long are copied by their record's lane
LANE_FOLD = 240      # kLaneFold: record_len up to this is folded by one lane (the encoder's fused limit)
DECODE_TILE = 4096   # image bytes per wave tile of decode and encode
REGION = 7168        # kRegion: image bytes per region of the sweep and of the index
MED_MAX = 65536      # kMedMax: record_len up to this is folded inside the sweep
SCAN_BLOCK = 1024    # entries per workgroup of the encode / decode offset scans
HOST_THREADS_MIN = 1 << 14  # parallel_for: host threads from this many records
MAX_IMAGE = 8 << 20
SEEDS = range(64)    # the seeds test_gpu_wal_fuzz.py runs and test_wal_fuzz_cpu.py checks the checker on

PROFILES = ("tiny", "lane_wave", "fold_edge", "mixed", "decoys", "empties")
COUNTS = (0, 1, 2, 7, 300, 5000, 40_000)
KINDS = ("none", "payload_bit", "crc_bit", "record_len", "val_len_restamped", "merge", "torn_tail", "appended")
LEN_DELTAS = (-9, -1, 1, 5, 4096, 1 << 20)


def _wal_images():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import wal_images
    return wal_images, wal_images.load()


# ---- the sequential decode and the per-record checks ------------------------------------------------------

def chain(img, size):
    """The structural record_len chain from byte 0 (wal.cpp:63-87), Python integers: (starts uint64, the
    position it ends at, whether it broke on a header that does not fit)."""
    b = img[:size].tobytes()
    starts, p, broke = [], 0, False
    while p < size:
        if size - p < META:
            broke = True
            break
        rlen = int.from_bytes(b[p:p + 4], "little")
        if rlen + 8 > size - p:
            broke = True
            break
        starts.append(p)
        p += 8 + rlen
    return np.array(starts, np.uint64), p, broke


def decode(oracle, img, size):
    """wal_entry::decode record after record (engine.cpp:31-53): (status, n_good, stop_offset), the
    good records' starts (uint64) and their largest sequence_ (0 for none)."""
    img = np.ascontiguousarray(img[:size])
    r, p, broke = chain(img, size)
    status, n_good, stop = ("corrupted" if broke else "ok"), r.size, p
    if r.size:
        at = r.astype(np.int64)
        field = lambda o, w, t: img[at[:, None] + o + np.arange(w)].copy().view(t).reshape(-1)  # noqa: E731
        rl, stored = field(0, 4, "<u4"), field(4, 4, "<u4")
        kl, vl = field(18, 4, "<u4").astype(np.uint64), field(22, 4, "<u4").astype(np.uint64)
        got = oracle.batch(img, r + 8, rl)
        bad = np.flatnonzero((got != stored) | (26 + kl + vl > 8 + rl.astype(np.uint64)))
        if bad.size:
            status, n_good, stop = "corrupted", int(bad[0]), int(r[bad[0]])
        seq = field(9, 8, "<u8")[:n_good]
    mseq = int(seq.max()) if r.size and n_good else 0
    return (status, n_good, stop), r[:n_good], mseq


def records_expected(oracle, img, size, offs):
    """Per record of a start list: (computed CRC or 0 when its length check fails, ok), ok meaning all of
    wal_entry::decode's checks pass (wal.cpp:68, :83, :89-96, :118-121)."""
    offs = np.asarray(offs, np.int64)
    n = offs.size
    crc = np.zeros(n, np.uint32)
    ok = np.zeros(n, bool)
    left = np.where(offs < size, size - offs, 0)
    hdr = left >= 26
    idx = np.flatnonzero(hdr)
    rlen = np.zeros(n, np.int64)
    if idx.size:
        o = offs[idx]
        b = img[(o[:, None] + np.arange(26)).astype(np.int64)]
        rl = b[:, 0:4].copy().view("<u4").reshape(-1).astype(np.int64)
        rlen[idx] = rl
    len_ok = hdr & (rlen + 8 <= left)
    li = np.flatnonzero(len_ok)
    if li.size:
        o = offs[li]
        crc[li] = oracle.batch(img, (o + 8).astype(np.uint64), rlen[li].astype(np.uint32))
        b = img[(o[:, None] + np.arange(26)).astype(np.int64)]
        stored = b[:, 4:8].copy().view("<u4").reshape(-1)
        klen = b[:, 18:22].copy().view("<u4").reshape(-1).astype(np.int64)
        vlen = b[:, 22:26].copy().view("<u4").reshape(-1).astype(np.int64)
        ok[li] = (crc[li] == stored) & (18 + klen + vlen <= rlen[li])
    return crc, ok


# ---- images -------------------------------------------------------------------------------------------------

def _u32(img, p):
    return int.from_bytes(img[p:p + 4].tobytes(), "little")


def _put_u32(img, p, v):
    img[p:p + 4] = np.frombuffer(int(v).to_bytes(4, "little"), np.uint8)


def restamp(oracle, img, offs):
    """The CRC field of the records at offs written again from the oracle (wal.cpp:54-58)."""
    offs = np.asarray(offs, np.uint64)
    rl = np.array([_u32(img, int(o)) for o in offs], np.uint32)
    crc = oracle.batch(img, offs + 8, rl)
    img[offs.astype(np.int64)[:, None] + 4 + np.arange(4)] = crc.astype("<u4").view(np.uint8).reshape(-1, 4)


def lengths(rng, profile, n):
    """(key_len, val_len) of n records of a profile."""
    tiny = lambda m: (rng.integers(0, 24, m), rng.integers(0, 41, m))  # noqa: E731
    if profile == "tiny":        # several records per 112-byte lane piece; every span lane-copied
        return tiny(n)
    if profile == "lane_wave":   # both sides of kShortSpan, in every pairing
        edge = np.array([0, 1, SHORT_SPAN - 1, SHORT_SPAN, SHORT_SPAN + 1, 80])
        return rng.choice(edge, n), rng.choice(edge, n)
    if profile == "fold_edge":   # record_len 226..256 around kLaneFold
        rl = rng.integers(LANE_FOLD - 14, LANE_FOLD + 17, n)
        kl = np.minimum(rng.integers(0, 24, n), rl - 18)
        return kl, rl - 18 - kl
    if profile == "mixed":       # long values across the decode tile, the sweep region and kMedMax
        kl, vl = tiny(n)
        big = np.flatnonzero(rng.random(n) < 0.1)
        vl[big] = np.exp(rng.uniform(np.log(300), np.log(70_000), big.size)).astype(np.int64)
        if n >= 50:  # among the first records, which an image cut at MAX_IMAGE keeps
            vl[int(rng.integers(0, min(n, 300) - 1))] = int(rng.integers(MED_MAX - 36, MED_MAX + 65))
        return kl, vl
    if profile == "decoys":      # values that are runs of whole well-formed 40-byte records
        return rng.integers(0, 40, n), np.minimum(rng.zipf(1.6, n) * 48, 4000)
    assert profile == "empties"  # runs of 26-byte records between tiny ones
    kl, vl = tiny(n)
    p = 0
    while p < n:
        run = int(rng.integers(1, 401))
        kl[p:p + run], vl[p:p + run] = 0, 0
        p += run + int(rng.integers(1, 60))
    return kl, vl


def build(rng, oracle, profile, n):
    """A clean image of up to n records of a profile (fewer when it would reach MAX_IMAGE): random
    sequence numbers below 2^62, op and tombstone 0/1. Returns (image, offsets u64, sizes u64)."""
    wi, ora = _wal_images()
    kl, vl = lengths(rng, profile, n)
    total = np.cumsum(META + kl.astype(np.int64) + vl.astype(np.int64))
    keep = int(np.searchsorted(total, MAX_IMAGE - 4096))
    kl, vl, n = kl[:keep], vl[:keep], min(n, keep)
    img, offs, size = wi.build(ora, kl, vl, rng, fake_values=profile == "decoys")
    if n:
        at = offs.astype(np.int64)
        img[at + 8] = rng.integers(0, 2, n, dtype=np.uint8)
        img[at[:, None] + 9 + np.arange(8)] = rng.integers(0, 1 << 62, n).astype("<u8").view(np.uint8).reshape(-1, 8)
        img[at + 17] = rng.integers(0, 2, n, dtype=np.uint8)
        restamp(oracle, img, offs)
    return img, offs, size


def mutate(rng, oracle, seed, img, offs, sizes):
    """One mutation, seed % 8: (image, logical size, the kind's name or "none" when it cannot apply, notes)."""
    kind = KINDS[seed % 8]
    n = offs.size
    notes = {}
    if n == 0 and kind != "appended":
        return img, img.size, "none", notes
    pick = (seed // 8) % 8
    v = 0 if pick == 0 else n - 1 if pick == 1 else int(rng.integers(0, n)) if n else 0
    notes["victim"] = v
    if n:
        o, sz = int(offs[v]), int(sizes[v])
    if kind == "payload_bit":
        img[o + 8 + int(rng.integers(0, sz - 8))] ^= 1 << int(rng.integers(0, 8))
    elif kind == "crc_bit":
        img[o + 4 + int(rng.integers(0, 4))] ^= 1 << int(rng.integers(0, 8))
    elif kind == "record_len":  # not restamped: the chain leaves the records here
        _put_u32(img, o, (sz - 8 + int(rng.choice(LEN_DELTAS))) & 0xFFFFFFFF)
    elif kind == "val_len_restamped":  # a valid CRC, the bounds fail (wal.cpp:118-121)
        _put_u32(img, o + 22, sz + int(rng.integers(0, 1000)))
        restamp(oracle, img, offs[v:v + 1])
    elif kind == "merge":  # the victim swallows the next 1-5 records: a valid image, one record with slack
        if n < 2:
            return img, img.size, "none", notes
        v = notes["victim"] = min(v, n - 2)
        o = int(offs[v])
        last = min(n - 1, v + int(rng.integers(1, 6)))
        _put_u32(img, o, int(offs[last] + sizes[last]) - o - 8)
        restamp(oracle, img, offs[v:v + 1])
        notes["swallowed"] = last - v
    elif kind == "torn_tail":  # cut inside the victim: inside its header, or inside its payload
        header = (seed // 16) % 2 == 0
        if not header and sz == META:
            bigger = np.flatnonzero(sizes > META)
            if bigger.size:
                v = notes["victim"] = int(bigger[np.argmin(np.abs(bigger - v))])
                o, sz = int(offs[v]), int(sizes[v])
            else:
                header = True
        cut = int(rng.integers(1, META)) if header else int(rng.integers(META, sz))
        notes["torn"] = "header" if header else "payload"
        return img[:o + cut], o + cut, kind, notes
    elif kind == "appended":
        img = np.concatenate([img, rng.integers(0, 256, int(rng.integers(1, 61)), dtype=np.uint8)])
    return img, img.size, kind, notes


def case(seed, oracle, profile=None, count=None, kind=None):
    """The case of a seed: image (numpy view of `size` bytes at `shift` inside `buf`), and what is
    expected of it. profile / count / kind override the seed's draw (kind as a number 0-7 replaces
    seed % 8 and keeps seed // 8's victim rule)."""
    rng = np.random.default_rng(424_000 + seed)
    drawn_profile, drawn_count = PROFILES[int(rng.integers(0, len(PROFILES)))], int(rng.choice(COUNTS))
    profile = drawn_profile if profile is None else profile
    count = drawn_count if count is None else count
    shift = int(rng.integers(0, 16))
    img, offs, sizes = build(rng, oracle, profile, count)
    mseed = seed if kind is None else seed // 8 * 8 + kind
    img, size, kind_name, notes = mutate(rng, oracle, mseed, img, offs, sizes)
    buf = np.zeros(shift + size, np.uint8)
    buf[shift:] = img[:size]
    img = buf[shift:]
    c = types.SimpleNamespace(seed=seed, profile=profile, count=offs.size, kind=kind_name, notes=notes, buf=buf,
                              shift=shift, img=img, size=size)
    c.verdict, c.starts, c.max_seq = decode(oracle, img, size)
    c.status, c.n_good, c.stop = c.verdict
    c.chain, c.chain_end, c.chain_broke = chain(img, size)
    c.chain_goes_on = c.chain.size > c.n_good  # the structural chain has records at and past `stop`
    c.crc, c.ok = records_expected(oracle, img, size, c.chain)
    assert c.ok[:c.n_good].all() and (c.n_good == c.chain.size or not c.ok[c.n_good])
    c.want = wal_decode_util.expected(img, c.starts)
    at = c.starts.astype(np.int64)
    rl = img[at[:, None] + np.arange(4)].copy().view("<u4").reshape(-1).astype(np.int64) if c.n_good else np.zeros(0, np.int64)
    c.record_len = rl
    c.slack = rl - 18 - c.want["key_len"].astype(np.int64) - c.want["val_len"].astype(np.int64)
    c.ref_shape = bool((c.slack == 0).all() and (c.want["tomb"] <= 1).all())  # what the reference encoder writes
    return c


def coverage(cases):
    """How many of the cases hold each situation the fuzz exists for."""
    cnt = dict.fromkeys(("no_good_nonempty", "empty_image", "stop_at_last_record", "torn_in_header", "torn_in_payload",
                         "structural_behind_valid_crc", "slack_in_good_prefix", "record_len_near_med_max",
                         "three_regions", "host_threads", "chain_goes_on", "no_closed_loop"), 0)
    for c in cases:
        cnt["no_good_nonempty"] += c.n_good == 0 and c.size > 0
        cnt["empty_image"] += c.size == 0
        cnt["stop_at_last_record"] += c.status == "corrupted" and c.count > 1 and c.n_good == c.count - 1
        cnt["torn_in_header"] += c.kind == "torn_tail" and c.notes["torn"] == "header" and c.size - c.stop < META
        cnt["torn_in_payload"] += c.kind == "torn_tail" and c.notes["torn"] == "payload" and c.size - c.stop >= META
        if c.chain_goes_on:
            j = c.n_good
            stored = int.from_bytes(c.img[int(c.chain[j]) + 4:int(c.chain[j]) + 8].tobytes(), "little")
            cnt["structural_behind_valid_crc"] += int(c.crc[j]) == stored and not c.ok[j]
        cnt["slack_in_good_prefix"] += bool((c.slack > 0).any())
        cnt["record_len_near_med_max"] += bool(((c.record_len >= 65_500) & (c.record_len <= 65_700)).any())
        cnt["three_regions"] += c.size >= 3 * REGION
        cnt["host_threads"] += c.n_good >= HOST_THREADS_MIN
        cnt["chain_goes_on"] += c.chain_goes_on
        cnt["no_closed_loop"] += not c.ref_shape
    return {k: int(v) for k, v in cnt.items()}
