"""Random record batches for the device LSM pipeline (WAL encode -> recover -> memtable replay -> flush ->
scan -> merge -> compaction) and everything the pipeline must make of them. Numpy and the sequential
helpers of the per-path suites only: no GPU, no product library.

case(seed) draws, in this order: the batch count, the key pool, the per-batch record counts, whether the
sequence numbers and the timestamps run against the log order, the block size, the files' byte misalignment,
the stream, and the records, oldest batch first. expect(case) is what every stage must give: the memtable
oracle's entries per batch (memtable_util.oracle / entries), the writer oracle's files (sst_build_util.
oracle_file), the merge oracle's survivors (sst_merge_util.oracle), and the compaction model: a dict over the
per-batch entries keyed by the user key, a newer batch overwriting, iterated in ``sorted`` order, surviving
tombstones removed under the drop flag. With the CRC oracle it also holds the WAL images (wal_encode_util.
expected) and their decode (wal_decode_util.expected).
"""
import types

import numpy as np

import memtable_util as mu
import sst_build_util as bu
import sst_merge_util as gu
import sst_scan_util as su
import wal_decode_util as wd
import wal_encode_util as we

SEEDS = range(32)    # the seeds test_gpu_lsm_fuzz.py runs and test_lsm_fuzz_cpu.py checks the generator on
META = 17            # bytes behind the user key of an internal key
SCAN_BLOCK = 1024    # kScanBlock: entries per workgroup of the format paths' scans
COUNTS = (1, 7, 300, 1100, 2100, 3000)   # records of a batch: both sides of SCAN_BLOCK and of the merge tile (2048)
POOLS = (40, 600, 2500, 6000)            # distinct keys of a seed
VAL_LENS = (0, 1, 5, 40, 127, 128, 300)  # both sides of the two-byte varint; BIG_VALUE at about 1 %
BIG_VALUE = 5000                         # more than most targets: a block of one entry
TARGETS = (1, 64, 100, 512, 4096, 65536)
NESTED_TARGET = 512  # block size of the intermediate file of a nested compaction
ALPHABET = (0x00, 0x61, 0x62, 0x7F, 0x80, 0xFF)
GUARD = 64           # canary bytes on both sides of a placed file image
CANARY = 0xA5

# Seeds the GPU tests name; test_lsm_fuzz_cpu.py checks that they are what the comments say.
LARGEST, SMALLEST = 25, 16      # most / least work (see work())
DAMAGED = 9                     # three or more files, a middle file of many blocks
THREAD_SEEDS = (8, 12, 14, 27)  # one per thread: three or more batches, under 6000 records, three targets


def make_pool(rng, size):
    """``size`` distinct keys of 0..40 bytes over ALPHABET, sorted: half of them behind a random-length prefix
    of one 40-byte stem (first-word ties, the full compare), the empty key, and some k / k\\0 pairs."""
    alpha = np.array(ALPHABET, np.uint8)
    stem = alpha[rng.integers(0, alpha.size, 40)].tobytes()
    seen = {b""}
    while len(seen) < size:
        ln = int(rng.integers(0, 41))
        cut = int(rng.integers(0, ln + 1)) if rng.random() < 0.5 else 0
        k = stem[:cut] + alpha[rng.integers(0, alpha.size, ln - cut)].tobytes()
        seen.add(k)
        if ln < 40 and len(seen) < size and rng.random() < 0.1:
            seen.add(k + b"\0")
    return sorted(seen), stem


def fresh_key(rng, pool):
    alpha = np.array(ALPHABET, np.uint8)
    have = set(pool)
    while True:
        k = alpha[rng.integers(0, alpha.size, int(rng.integers(1, 41)))].tobytes()
        if k not in have:
            return k


def case(seed):
    """The case of a seed: ``batches`` [[(op, seq, key, value, tomb)]] oldest first, ``ts`` one timestamp_ms
    per batch, and the pipeline's choices ``target``, ``flags`` (the WAL decode's view flags), ``misalign``
    (of every flushed file image), ``other_stream``. The last record of the last batch is a put of a key no
    other record has, so a non-tombstone always survives; every batch holds a record."""
    rng = np.random.default_rng(0x15A0000 + seed)
    k = int(rng.integers(2, 9))
    pool_size = int(rng.choice(POOLS))
    pool, _ = make_pool(rng, pool_size)
    counts = [int(x) for x in rng.choice(COUNTS, k)]
    seq_descends = bool(rng.integers(0, 2))
    ts_descends = rng.random() < 1 / 3
    target = int(rng.choice(TARGETS))
    misalign = int(rng.integers(0, 16))
    other_stream = bool(rng.integers(0, 2))
    blob = rng.integers(0, 256, 70_000, dtype=np.uint8).tobytes()
    base_ts = 1_700_000_000_000 + 7 * seed
    batches, ts, seq = [], [], 1
    for b, n in enumerate(counts):
        if seq_descends:  # newer batches start lower; 4000 > max(COUNTS) keeps every seq of a seed distinct
            seq = 1 + 4000 * (k - 1 - b)
        ts.append(base_ts + 1000 * ((k - b) if ts_descends else b))
        which = rng.integers(0, len(pool), n)
        op = rng.random(n) < 0.2
        vl = np.where(rng.random(n) < 0.01, BIG_VALUE, rng.choice(VAL_LENS, n))
        vl = np.where(op, np.where(rng.random(n) < 0.1, vl, 0), vl)  # one delete in ten carries bytes: they are dropped
        at = rng.integers(0, len(blob) - BIG_VALUE, n)
        recs = [(int(op[i]), seq + i, pool[which[i]], blob[at[i]:at[i] + vl[i]], int(op[i])) for i in range(n)]
        seq += n
        batches.append(recs)
    last = batches[-1][-1]
    batches[-1][-1] = (0, last[1], fresh_key(rng, pool), blob[:5], 0)
    return types.SimpleNamespace(seed=seed, k=k, pool_size=pool_size, counts=counts, seq_descends=seq_descends,
                                 ts_descends=bool(ts_descends), target=target, flags=seed % 4, misalign=misalign,
                                 other_stream=other_stream, batches=batches, ts=ts)


def work(c):
    """The size of a case: its records (what the WAL paths and the replay handle) plus its run entries (what
    flush, scan and merge handle)."""
    return sum(c.counts) + sum(len(set(r[2] for r in recs)) for recs in c.batches)


def wal_batch(recs):
    """A record batch as the arenas and columns of wal_encode_util (what tkv_wal_encode[_device] takes)."""
    c = mu.columns(recs)
    keys = np.frombuffer(b"".join(r[2] for r in recs) + b"\0", np.uint8).copy()  # never empty: an address is required
    return dict(n=len(recs), keys=keys, key_off=c.key_off, key_len=c.key_len, vals=mu.values_arena(recs),
                val_off=c.val_off, val_len=c.val_len, op=c.op, tomb=c.tomb, seq=c.seq, first_seq=0)


def model(entries, drop=False):
    """The compaction of per-batch entries [[(ikey, value)]], oldest first: a dict by user key, the newest batch
    wins, in ``sorted`` order; ``drop`` removes the surviving tombstones."""
    d = {}
    for run in entries:
        for k, v in run:
            d[k[:-META]] = (k, v)
    out = [d[u] for u in sorted(d)]
    return [(k, v) for k, v in out if k[-1] == 0] if drop else out


def expect(c, oracle=None):
    """Everything the pipeline must give for a case. Per batch: ``mem`` (the memtable oracle's Expected),
    ``entries``, ``files`` (oracle_file's tuples at the case's target), ``scans`` (oracle_scan's entries of
    those files). For the merge: ``src`` [(run, index)], ``model``, ``live`` (the model without tombstones),
    the files ``flat`` and ``dropped``, and ``half`` (the first k // 2 batches compacted at NESTED_TARGET, None
    when k // 2 < 2). With ``oracle`` (the CRC oracle) also ``wal`` [(image, offsets, crcs)] and ``decoded``
    (wal_decode_util.expected under the case's flags)."""
    e = types.SimpleNamespace(mem=[], entries=[], files=[], scans=[], wal=[], decoded=[])
    for recs, ts in zip(c.batches, c.ts):
        exp = mu.oracle(mu.columns(recs), ts)
        ents = mu.entries(exp, mu.values_arena(recs).tobytes())
        e.mem.append(exp)
        e.entries.append(ents)
        e.files.append(bu.oracle_file(ents, c.target))
        status, _, scanned, _ = su.oracle_scan(e.files[-1][0])
        assert status == "ok" and scanned == ents
        e.scans.append(scanned)
        if oracle is not None:
            img, offs, crc = we.expected(wal_batch(recs), oracle)
            e.wal.append((img, offs, crc))
            e.decoded.append(wd.expected(img, offs, c.flags))
    e.src = gu.oracle(gu.columns(e.entries))
    e.model, e.live = model(e.entries), model(e.entries, drop=True)
    e.flat = bu.oracle_file(e.model, c.target)[0]
    e.dropped = bu.oracle_file(e.live, c.target)[0]
    e.half = bu.oracle_file(model(e.entries[:c.k // 2]), NESTED_TARGET)[0] if c.k // 2 >= 2 else None
    return e


def coverage(cases, tile):
    """How many of the cases hold each situation the fuzz exists for (``tile``: the merge's workgroup tile)."""
    names = ("five_runs", "entries_over_tile", "batch_over_tile", "pool_40_batch_1000", "nested", "big_value_survives",
             "seq_descends", "ts_descends", "other_stream", "cross_batch_duplicates", "tombstone_survives")
    cnt = dict.fromkeys(names, 0)
    for c in cases:
        ents = [mu.entries(mu.oracle(mu.columns(r), t), mu.values_arena(r).tobytes()) for r, t in zip(c.batches, c.ts)]
        m = model(ents)
        total = sum(len(x) for x in ents)
        cnt["five_runs"] += c.k >= 5
        cnt["entries_over_tile"] += total > tile
        cnt["batch_over_tile"] += max(c.counts) > tile
        cnt["pool_40_batch_1000"] += c.pool_size == 40 and max(c.counts) >= 1000
        cnt["nested"] += c.k // 2 >= 2
        cnt["big_value_survives"] += any(len(v) == BIG_VALUE for _, v in m)
        cnt["seq_descends"] += c.seq_descends
        cnt["ts_descends"] += c.ts_descends
        cnt["other_stream"] += c.other_stream
        cnt["cross_batch_duplicates"] += len(m) < total
        cnt["tombstone_survives"] += any(k[-1] for k, _ in m)
    return {k: int(v) for k, v in cnt.items()}
