"""The WAL sweep grid images (wal_sweep_util) without a GPU: every placement the builders promise is
counted from the built image, so a builder that loses coverage fails here; the sequential decode calls
both images clean; neither holds a plausible header off the chain (which is what lets
test_gpu_wal_sweep_grid.py demand a sweep without fix-up rounds); every mutation's expected verdict names
the mutated record."""
import ctypes

import numpy as np
import pytest

import wal_sweep_util as sw
from wal_fuzz_util import LANE_FOLD, LANE_PIECE, MED_MAX, META, REGION, decode
from wal_sweep_util import PIECE, SEED_CHUNK, SEED_START


@pytest.fixture(scope="module")
def start_phase(oracle):
    return sw.start_phase_image(np.random.default_rng(SEED_START), oracle)


@pytest.fixture(scope="module")
def chunk(oracle):
    return sw.chunk_image(np.random.default_rng(SEED_CHUNK), oracle)


def test_constants_are_the_kernels(lib):
    """REGION and PIECE against what the library reports (no sweep has run on this thread: W = nreg = 0
    or whatever an earlier test of this process left)."""
    g = (ctypes.c_uint64 * 4)()
    lib.tkv_debug_wal_sweep_geometry(g)
    assert (g[0], g[1]) == (REGION, PIECE) and PIECE == LANE_PIECE and REGION == 64 * PIECE
    prev = lib.tkv_debug_set_wal_sweep_waves(3)
    assert lib.tkv_debug_set_wal_sweep_waves(0) == 3  # returns the previous setting; 0 restores the default
    assert lib.tkv_debug_set_wal_sweep_waves(prev) == 0


def test_start_phase_image_holds_every_case(start_phase):
    img, offs, sizes, marks = start_phase
    o, z = offs.astype(np.int64), sizes.astype(np.int64)
    assert img.size <= 64 * REGION and int(o[-1] + z[-1]) == img.size
    exception = marks["no_start"]
    rl = z - 8
    assert rl[exception] == sw.NO_START_LEN <= LANE_FOLD
    rest = np.delete(rl, exception)
    assert rest.min() >= 18 and rest.max() <= sw.SHORT_MAX
    assert (img[o + 8] == 0).all() and (img[o + 17] == 0).all()  # op = tomb = 0
    # every piece phase
    assert set((o % PIECE).tolist()) == set(range(PIECE))
    # the header cut by a region end at every byte; two starts at a region's last byte
    in_region = o % REGION
    for d in range(1, 27):
        assert (in_region == REGION - d).any(), d
    assert np.count_nonzero(in_region == REGION - 1) >= 2
    # a start at region byte 0 behind a record that ends exactly on the region end
    ends = o + z
    assert np.intersect1d(ends[ends % REGION == 0], o).size >= 1
    # pieces: one with five starts from a phase <= 7, all 26 bytes; one inside the image with none
    piece = o // PIECE
    per_piece = np.bincount(piece, minlength=(img.size + PIECE - 1) // PIECE)
    five = [p for p in np.flatnonzero(per_piece == 5)
            if (z[piece == p] == META).all() and int(o[piece == p][0]) % PIECE <= 7]
    assert five, "no piece with five 26-byte starts"
    assert per_piece.max() == 5  # kStore = 6 slots are never exceeded
    whole = per_piece[:img.size // PIECE]
    assert (whole == 0).any(), "no piece without a start inside the image"
    assert np.count_nonzero(whole == 0) == 1  # (the one behind the NO_START_LEN record)
    # a region whose records are all 26 bytes: 276 starts
    region = o // REGION
    full = [r for r in np.unique(region) if (z[region == r] == META).all()]
    assert full and max(np.count_nonzero(region == r) for r in full) == REGION // META + 1 == 276
    # tail_sizes finds its record, whose header the region end cuts
    t = sw.tail_sizes(offs, sizes)
    assert t[0] % REGION == REGION - 10 and t[-1] - t[0] >= META and len(set(t)) == 7 and t[-1] < img.size


def test_chunk_image_holds_every_case(chunk):
    img, offs, sizes, placed = chunk
    o, z = offs.astype(np.int64), sizes.astype(np.int64)
    assert img.size <= 2 << 20 and int(o[-1] + z[-1]) == img.size
    assert z[-1] <= 98  # ends with a short record
    nreg = (img.size + REGION - 1) // REGION
    for i, s, L, d in placed:
        assert int(o[i]) == s and int(z[i]) == 8 + L and s % REGION == REGION - d
    rl = z - 8
    long_ = np.flatnonzero(rl > sw.SHORT_MAX)
    assert sorted(long_.tolist()) == sorted(p[0] for p in placed)  # everything else is short
    assert {p[2] for p in placed} == set(sw.CHUNK_LENS)
    assert {p[3] for p in placed} == set(sw.CHUNK_D)
    for L in sw.CHUNK_LENS[:6]:  # the lengths up to REGION + 1 at every d
        assert {p[3] for p in placed if p[2] == L} == set(sw.CHUNK_D), L
    pay, end = o[long_] + 8, o[long_] + z[long_]
    assert (pay % REGION == 0).any(), "no payload begins exactly on a region end"
    assert (end % REGION == 0).any(), "no payload ends exactly on a region end"
    # records over MED_MAX: two from an even region, two from an odd one, each followed by at least
    # three whole regions of short records, each passed over inside the image
    giants = np.flatnonzero(rl > MED_MAX)
    assert giants.size == 4
    assert sorted(((o[giants] // REGION) % 2).tolist()) == [0, 0, 1, 1]
    region = o // REGION
    for g in giants:
        first = -(-int(o[g] + z[g]) // REGION)  # the first region that starts at or behind its end
        assert first + 3 <= nreg
        for r in range(first, first + 3):
            assert (region == r).any() and (z[region == r] <= 98).all(), (g, r)
        assert int(o[g] + z[g]) // REGION > int(o[g]) // REGION + 1
    # a single wave over the whole image restarts its ring after a pass-over in both slots
    assert set(sw.giant_restart_parities(offs, sizes, nreg)) == {0, 1}
    # a medium record that covers whole regions (walked one by one, folded as carries)
    med = (rl > LANE_FOLD) & (rl <= MED_MAX)
    assert ((o[med] + z[med]) // REGION - o[med] // REGION >= 3).any()


@pytest.mark.parametrize("which", ["start_phase", "chunk"])
def test_clean_images_decode_and_hold_no_off_chain_header(oracle, start_phase, chunk, which):
    img, offs, sizes, _ = start_phase if which == "start_phase" else chunk
    verdict, starts, _ = decode(oracle, img, img.size)
    assert verdict == ("ok", offs.size, img.size)
    assert np.array_equal(starts, offs)
    # the condition under which every speculative start of the sweep is a record start
    assert sw.off_chain_headers(img, offs).size == 0
    # (the rule itself: every record start passes it, and a planted header off the chain shows)
    assert sw.off_chain_headers(img, offs[1:]).tolist() == [0]
    assert sw.off_chain_headers(img, np.delete(offs, offs.size // 2)).tolist() == [int(offs[offs.size // 2])]


@pytest.mark.parametrize("which", ["start_phase", "chunk"])
def test_mutations_name_their_record(oracle, start_phase, chunk, which):
    img, offs, sizes, _ = start_phase if which == "start_phase" else chunk
    muts = sw.mutations(oracle, img, offs, sizes)
    want = set(sw.MUTATIONS) if which == "chunk" else {"cut_d1", "cut_d8", "cut_d26", "record_len_17"}
    assert set(muts) == want
    for name, (i, (verdict, starts, _), apply) in muts.items():
        assert verdict == ("corrupted", i, int(offs[i])), name
        assert np.array_equal(starts, offs[:i]), name
        m = img.copy()
        apply(m)
        assert np.count_nonzero(m != img) in ((1,) if name != "record_len_17" else range(1, 9)), name
    o, z = offs.astype(np.int64), sizes.astype(np.int64)
    for d in (1, 8, 26):
        assert int(o[muts[f"cut_d{d}"][0]]) % REGION == REGION - d
    if which == "chunk":
        i = muts["medium_first"][0]
        assert muts["medium_last"][0] == muts["medium_region_end"][0] == i
        assert LANE_FOLD < z[i] - 8 <= MED_MAX and (o[i] + 8) // REGION != (o[i] + z[i] - 1) // REGION
        assert z[muts["giant"][0]] - 8 > MED_MAX
    i = muts["record_len_17"][0]
    m = img.copy()
    muts["record_len_17"][2](m)
    assert int.from_bytes(m[o[i]:o[i] + 4].tobytes(), "little") == 17
    assert oracle.crc(m[o[i] + 8:o[i] + 25].tobytes()) == int.from_bytes(m[o[i] + 4:o[i] + 8].tobytes(), "little")


def test_tails_decode(oracle, start_phase):
    """The truncations of tail_sizes: clean at the record's start and end, corrupted at the record in
    between (a torn header, then a record_len that overruns the image)."""
    img, offs, sizes, _ = start_phase
    t = sw.tail_sizes(offs, sizes)
    i = int(np.flatnonzero(offs == t[0])[0])
    got = [decode(oracle, img, n)[0] for n in t]
    assert got[0] == ("ok", i, t[0]) and got[-1] == ("ok", i + 1, t[-1])
    for n, g in zip(t[1:-1], got[1:-1]):
        assert g == ("corrupted", i, t[0]), n
