"""Images for the device WAL sweep (wal_sweep / wal_idx_emit in tkv_wal_device.hip) placed on its own
constants, and what the sequential decode makes of them. Numpy and the test oracle only: no GPU, no
product library. Every expected value comes from wal_fuzz_util.decode (the record_len chain, the C
oracle's CRCs and the key/value bounds of wal.cpp:63-121), never from the library's walk.

start_phase_image   short records with a start at every phase of a lane piece and at every distance from
                    a region end at which the header is cut, full and empty pieces, a region of 26-byte
                    records
chunk_image         long payloads against region ends, records longer than MED_MAX inside chunks
tail_sizes          truncations of an image inside a record whose header a region end cuts
off_chain_headers   positions off the chain that the sweep's header search would take for a record start
mutations           single corruptions of placed records, each with the decode's verdict

test_wal_sweep_grid_cpu.py counts every promise of the builders from the built images.
"""
import numpy as np

from wal_fuzz_util import LANE_FOLD, LANE_PIECE as PIECE, MED_MAX, META, REGION, decode, restamp

SEED_START, SEED_CHUNK = 4101, 4102  # the seeds both test files build the two clean images from
SHORT_MAX = 90          # record_len of the short records: 18 .. SHORT_MAX (26 .. 98 bytes)
NO_START_LEN = 216      # the one longer record of start_phase_image (see there)
CUT_D = tuple(range(1, 27))                       # start_phase_image: starts at REGION - d
CHUNK_D = (1, 2, 3, 4, 5, 6, 7, 8, 26, 27)        # chunk_image: starts at REGION - d
CHUNK_LENS = (240, 241, 352, REGION - 8, REGION, REGION + 1, 20000, MED_MAX, MED_MAX + 1, 100000)
MUTATIONS = ("cut_d1", "cut_d8", "cut_d26", "medium_first", "medium_last", "medium_region_end", "giant",
             "record_len_17")


def record(rng, plen, klen=4):
    """One unstamped record with record_len = plen >= 18: random body and sequence number (below 2^62),
    op = tombstone = 0, record_len = 18 + key_len + value_len."""
    klen = min(klen, plen - 18)
    vlen = plen - 18 - klen
    body = bytearray(rng.integers(0, 256, 8 + plen, dtype=np.uint8).tobytes())
    body[0:4] = plen.to_bytes(4, "little")
    body[4:8] = b"\0\0\0\0"
    body[8] = 0
    body[16] &= 0x3F
    body[17] = 0
    body[18:22] = klen.to_bytes(4, "little")
    body[22:26] = vlen.to_bytes(4, "little")
    return bytes(body)


class _Layout:
    """Records appended one after the other; pad_to(t) fills with short records up to exactly t."""

    def __init__(self, rng):
        self.rng, self.recs, self.pos = rng, [], 0

    def add(self, plen):
        """Appends a record of record_len plen; returns its (index, start)."""
        at = (len(self.recs), self.pos)
        self.recs.append(record(self.rng, plen))
        self.pos += 8 + plen
        return at

    def short(self):
        return self.add(int(self.rng.integers(18, 83)))

    def pad_to(self, t):
        """Short records (record_len 18 .. SHORT_MAX) ending exactly at t >= pos + 26 (or t == pos)."""
        assert t == self.pos or t - self.pos >= META, (t, self.pos)
        top = 8 + SHORT_MAX
        while t - self.pos > top + META:  # what is left stays at least META
            self.short()
        left = t - self.pos
        if left > top:  # 99 .. 124: two records
            self.add(left - 60 - 8)
            left = 60
        if left:
            self.add(left - 8)
        assert self.pos == t

    def next_at(self, d, parity=None):
        """The nearest position REGION - d of a region (of the given parity) that pad_to can reach."""
        k = (self.pos + d) // REGION
        while True:
            t = k * REGION - d
            if (t == self.pos or t - self.pos >= META) and (parity is None or (k - 1) % 2 == parity):
                return t
            k += 1

    def finish(self, oracle):
        img = np.frombuffer(b"".join(self.recs), np.uint8).copy()
        sizes = np.array([len(r) for r in self.recs], np.uint64)
        offs = np.zeros(sizes.size, np.uint64)
        offs[1:] = np.cumsum(sizes[:-1])
        restamp(oracle, img, offs)
        return img, offs, sizes


def start_phase_image(rng, oracle):
    """(img, offs, sizes, marks). Short records (record_len 18 .. SHORT_MAX, random bodies, op = tomb = 0)
    holding, counted from the image by test_wal_sweep_grid_cpu.py:
      * a record start at every piece phase offs % PIECE in 0 .. 111;
      * a start at every REGION - d, d = 1 .. 26 (the header cut by the region end at every byte), and a
        second one at a region's last byte;
      * a start at region byte 0 behind a record that ends exactly on the region end;
      * a piece with five starts (26-byte records from a piece phase <= 7): 5 of kStore's 6 slots;
      * a piece with no start. No record of at most 98 bytes covers a 112-byte piece, so this one record
        has record_len NO_START_LEN (still folded by one lane, <= LANE_FOLD); it is the only exception;
      * a region whose records are all 26 bytes long: 276 starts (kList = 291).
    At most 64 regions; ends with a short record. marks: record indices by name."""
    lay, marks = _Layout(rng), {}
    for _ in range(3):
        lay.short()
    for d in CUT_D + (1,):  # each in a region of its own
        lay.pad_to(lay.next_at(d))
        marks.setdefault(("cut", d), lay.add(int(rng.integers(40, SHORT_MAX + 1)))[0])
    lay.pad_to(lay.next_at(0))
    marks["ends_at_region_end"] = len(lay.recs) - 1
    marks["region_byte_0"] = lay.short()[0]
    for ph in range(PIECE):  # every piece phase, deliberately
        t = lay.pos + META + (ph - lay.pos - META) % PIECE
        lay.pad_to(t)
        lay.short()
    # five starts in one piece: 26-byte records from phase 5
    t = lay.pos + META + (5 - lay.pos - META) % PIECE
    lay.pad_to(t)
    marks["five_starts"] = len(lay.recs)
    for _ in range(5):
        lay.add(18)
    # a piece without a start: a record from phase 50 of one piece to phase 50 of the next but one
    t = lay.pos + META + (50 - lay.pos - META) % PIECE
    lay.pad_to(t)
    marks["no_start"] = lay.add(NO_START_LEN)[0]
    assert NO_START_LEN <= LANE_FOLD and 8 + NO_START_LEN == 2 * PIECE
    # a region of 26-byte records, from its byte 0
    lay.pad_to(lay.next_at(0))
    marks["all_26"] = len(lay.recs)
    for _ in range(REGION // META + 1):
        lay.add(18)
    for _ in range(40):
        lay.short()
    lay.add(42)
    img, offs, sizes = lay.finish(oracle)
    assert img.size <= 64 * REGION
    return img, offs, sizes, marks


def chunk_placements():
    """(record_len, d) of chunk_image's placed records, in image order: the lengths up to REGION + 1 at
    every d; the longer ones up to MED_MAX at a few d each (every pair would pass 2 MiB). The four records
    over MED_MAX follow them (GIANTS)."""
    small = [(L, d) for L in CHUNK_LENS[:6] for d in CHUNK_D]
    big = [(20000, 1), (20000, 8), (20000, 26), (MED_MAX, 3), (MED_MAX, 8), (MED_MAX, 27)]
    return small + big


# (record_len, d, region parity). The region's parity alone does not fix the slot of the sweep's
# two-region ring in which a wave meets the record: every pass-over of an odd number of regions swaps the
# slots of all later regions (giant_restart_parities). In this order a wave that walks the whole image
# restarts its ring from slots 0, 1, 1, 0.
GIANTS = ((MED_MAX + 1, 2, 0), (100000, 8, 0), (100000, 5, 1), (MED_MAX + 1, 26, 1))


def chunk_image(rng, oracle):
    """(img, offs, sizes, placed). Long payloads against region ends, as region_end_records of
    test_gpu_wal_device.py: record_len in CHUNK_LENS, each start d in CHUNK_D bytes before a region end
    (so a payload begins exactly on a region end at d = 8, and record_len = REGION there ends on the next
    one); four records of record_len > MED_MAX, two starting in an even-numbered region and two in an
    odd-numbered one, each followed by at least three whole regions of short records; short records in
    between and at the end. At most 2 MiB. placed: (record index, start, record_len, d) of each."""
    lay, placed = _Layout(rng), []
    for _ in range(5):
        lay.short()
    for L, d in chunk_placements():
        lay.pad_to(lay.next_at(d))
        i, s = lay.add(L)
        placed.append((i, s, L, d))
    for L, d, parity in GIANTS:
        lay.pad_to(lay.next_at(d, parity))
        i, s = lay.add(L)
        placed.append((i, s, L, d))
        lay.pad_to(lay.next_at(0))
        lay.pad_to(lay.pos + 3 * REGION + 30)
    for _ in range(20):
        lay.short()
    lay.add(50)
    img, offs, sizes = lay.finish(oracle)
    assert img.size <= 2 << 20
    return img, offs, sizes, placed


def tail_sizes(offs, sizes):
    """For the first record that starts 10 bytes before a region end (s, 8 + rl bytes): the image sizes
    s, s + 1, s + 25, s + 26, s + 27, s + 8 + rl - 1, s + 8 + rl."""
    at = np.flatnonzero(offs % np.uint64(REGION) == np.uint64(REGION - 10))
    assert at.size, "no record starts 10 bytes before a region end"
    s, n = int(offs[at[0]]), int(sizes[at[0]])
    return [s, s + 1, s + 25, s + 26, s + 27, s + n - 1, s + n]


def off_chain_headers(img, offs):
    """The positions q of the image that are not record starts and that the sweep's search
    (search_piece) would take for one: bytes q + 8 and q + 17 at most 1, u32[q] == 18 + u32[q + 18] +
    u32[q + 22], u32[q] + 8 <= size - q, size - q >= 26. int64, increasing."""
    size = int(img.size)
    n = size - META + 1
    if n <= 0:
        return np.zeros(0, np.int64)
    b = img.astype(np.uint64)
    u = b[0:size - 3] | b[1:size - 2] << np.uint64(8) | b[2:size - 1] << np.uint64(16) | b[3:size] << np.uint64(24)
    q = np.arange(n, dtype=np.uint64)
    rl = u[0:n]
    ok = (img[8:8 + n] <= 1) & (img[17:17 + n] <= 1) & (rl == np.uint64(18) + u[18:18 + n] + u[22:22 + n]) & \
        (rl + np.uint64(8) <= np.uint64(size) - q)
    ok[np.asarray(offs, np.int64)[np.asarray(offs, np.int64) < n]] = False
    return np.flatnonzero(ok).astype(np.int64)


def _flip(pos):
    return lambda img: img.__setitem__(pos, img[pos] ^ 0x10)


def mutations(oracle, img, offs, sizes):
    """Single corruptions of records of a clean image: {name: (record index, expected, apply)}.
    apply(copy of the image) makes the change; expected is ((verdict, n_good, stop), starts, max_sequence)
    of wal_fuzz_util.decode on the changed image. The names of MUTATIONS whose record the image holds:
      cut_d1, cut_d8, cut_d26   a payload byte (the last) of a record starting REGION - d, flipped
      medium_first / _last / _region_end
                                one record with LANE_FOLD < record_len <= MED_MAX that crosses a region
                                end: its first payload byte, its last, the first byte of the next region
      giant                     a byte in the middle of a record with record_len > MED_MAX
      record_len_17             record_len = 17 with the CRC stamped again: the bounds fail, not the CRC
    """
    o, z = offs.astype(np.int64), sizes.astype(np.int64)
    rl = z - 8
    out = {}

    def put(name, i, apply):
        m = img.copy()
        apply(m)
        out[name] = (int(i), decode(oracle, m, m.size), apply)

    for d in (1, 8, 26):
        at = np.flatnonzero(o % REGION == REGION - d)
        if at.size:
            i = at[at.size // 2]
            put(f"cut_d{d}", i, _flip(int(o[i] + z[i]) - 1))
    cross = np.flatnonzero((rl > LANE_FOLD) & (rl <= MED_MAX) & ((o + 8) // REGION != (o + z - 1) // REGION))
    if cross.size:
        i = cross[cross.size // 2]
        a = int(o[i]) + 8
        put("medium_first", i, _flip(a))
        put("medium_last", i, _flip(int(o[i] + z[i]) - 1))
        put("medium_region_end", i, _flip((a // REGION + 1) * REGION))
    giant = np.flatnonzero(rl > MED_MAX)
    if giant.size:
        i = giant[giant.size // 2]
        put("giant", i, _flip(int(o[i] + z[i] // 2)))
    short = np.flatnonzero((z <= 98) & (z >= 40) & (o % REGION > 2000) & (o % REGION < 5000))
    i = short[short.size // 2]

    def len17(m, s=int(o[i])):
        m[s:s + 4] = np.frombuffer((17).to_bytes(4, "little"), np.uint8)
        restamp(oracle, m, np.array([s], np.uint64))
    put("record_len_17", i, len17)
    return out


def giant_restart_parities(offs, sizes, nreg):
    """The ring slots (k of sweep_wave's kAhead = 2 loop) at which one wave that walks the whole image
    from region 0 restarts its pipeline after passing a record of record_len > MED_MAX over, with the
    landing region inside the image: region rr runs in slot (rr + c) % 2, and a restart at nx moves c by
    the regions passed over."""
    c, seen = 0, []
    for s, n in zip(offs.astype(np.int64).tolist(), sizes.astype(np.int64).tolist()):
        if n - 8 > MED_MAX:
            rr, nx = s // REGION, (s + n) // REGION
            if nx > rr + 1 and nx < nreg:
                seen.append((rr + c) % 2)
                c = (c + nx - rr - 1) % 2
    return seen
