"""WAL salvage without a GPU: the sequential oracle of wal_salvage_util (the sub-image decode and the
numpy resync the GPU tests compare with) against the byte-by-byte salvage program on the small fuzz
cases and on hand-built images; the argument checks of tkv_wal_resync_device, tkv_wal_salvage_device and
tkv_wal_salvage, all decided before any device work; the search geometry."""
import ctypes

import numpy as np
import pytest

import tinykvpp_amd as tk
import wal_fuzz_util as fz
import wal_salvage_util as su
from tinykvpp_amd._lib import INVALID_ARGUMENT, NOT_FOUND, OK

U64 = ctypes.c_uint64
DUMMY = ctypes.c_void_p(16)  # never dereferenced: the argument checks come first
SMALL = 20_000


def same_as_brute(oracle, img, size):
    status, starts, gaps, stop, _, skipped = su.salvage(oracle, img, size)
    bstarts, bgaps = su.brute_salvage(oracle, img, size)
    assert starts.tolist() == bstarts and [tuple(g) for g in gaps.tolist()] == bgaps
    assert stop == size and skipped == sum(b - a for a, b in bgaps)
    assert status == ("corrupted" if bgaps else "ok")
    return starts, gaps


def test_util_equals_the_byte_by_byte_program_on_small_fuzz_cases(oracle):
    small = 0
    for seed in fz.SEEDS:
        c = fz.case(seed, oracle)
        if c.size > SMALL:
            continue
        small += 1
        starts, gaps = same_as_brute(oracle, c.img, c.size)
        assert np.array_equal(starts[:c.n_good], c.starts)
        if c.status == "ok":
            assert gaps.size == 0
        else:
            assert int(gaps[0, 0]) == c.stop
    assert small >= 8


def test_util_on_hand_built_images(oracle):
    rng = np.random.default_rng(7)
    r = [su.record(oracle, b"k%d" % i, bytes(rng.integers(0, 256, 5 + 3 * i, dtype=np.uint8)), seq=i + 1) for i in range(6)]
    arr = lambda parts: np.frombuffer(b"".join(parts), np.uint8).copy()  # noqa: E731
    # clean; noise in front, between and behind; a torn tail; a flipped payload bit in the middle
    img = arr(r)
    assert same_as_brute(oracle, img, img.size)[1].size == 0
    img = arr([su.noise(rng, 37), r[0], r[1], su.noise(rng, 1), r[2], su.noise(rng, 300), r[3], su.noise(rng, 25)])
    starts, gaps = same_as_brute(oracle, img, img.size)
    assert starts.size == 4 and gaps.shape[0] == 4 and int(gaps[-1, 1]) == img.size
    img = arr(r)[:-3]
    starts, gaps = same_as_brute(oracle, img, img.size)
    assert starts.size == 5 and gaps.tolist() == [[img.size - len(r[5]) + 3, img.size]]
    img = arr(r)
    img[len(r[0]) + len(r[1]) + 30] ^= 4
    starts, gaps = same_as_brute(oracle, img, img.size)
    assert starts.size == 5 and gaps.tolist() == [[len(r[0]) + len(r[1]), len(r[0]) + len(r[1]) + len(r[2])]]
    # nested: an outer record whose value is three valid records, its CRC flipped
    outer = bytearray(su.record(oracle, b"outer", r[0] + r[1] + r[2], seq=9))
    outer[5] ^= 1
    img = arr([r[3], bytes(outer), r[4]])
    starts, gaps = same_as_brute(oracle, img, img.size)
    inner0 = len(r[3]) + 26 + 5
    assert starts.tolist() == [0, inner0, inner0 + len(r[0]), inner0 + len(r[0]) + len(r[1]), len(r[3]) + len(outer)]
    assert gaps.tolist() == [[len(r[3]), inner0]]
    # max_gaps: the oracle's prefix
    img = arr([r[0], su.noise(rng, 9), r[1], su.noise(rng, 9), r[2]])
    status, starts, gaps, stop, mseq, skipped = su.salvage(oracle, img, img.size, max_gaps=1)
    assert (status, starts.size, gaps.shape[0], stop, mseq, skipped) == ("corrupted", 2, 1, len(r[0]) + 9 + len(r[1]), 2, 9)
    assert su.salvage(oracle, img, img.size, max_gaps=0)[:2][1].tolist() == [0]
    assert su.resync(oracle, img, img.size, 1) == len(r[0]) + 9 and su.resync(oracle, img, img.size, img.size - 30) is None


def test_field_edges_in_the_util(oracle):
    """Decoys whose fields wrap in 32-bit arithmetic are not candidates."""
    rng = np.random.default_rng(8)
    good = su.record(oracle, b"key", b"value", seq=3)
    decoys = [su.header(0xFFFFFFFF), su.header(0xFFFFFFF8), su.header(200, kl=0xFFFFFFFF, vl=20), su.header(17)]
    img = np.frombuffer(b"".join(d + su.noise(rng, 40) for d in decoys) + good, np.uint8).copy()
    assert su.structural(img, img.size, 0, img.size).tolist() == [img.size - len(good)]
    assert su.resync(oracle, img, img.size, 0) == img.size - len(good)


def outs():
    return [U64(7) for _ in range(5)]


def test_resync_argument_errors(lib):
    f = lib.tkv_wal_resync_device
    found = U64(7)
    assert f(None, 100, 0, ctypes.byref(found), None) == INVALID_ARGUMENT   # no image
    assert f(DUMMY, 100, 0, None, None) == INVALID_ARGUMENT                 # no result
    assert f(DUMMY, 100, 101, ctypes.byref(found), None) == INVALID_ARGUMENT  # from behind the end
    assert found.value == 7
    # an image too short for a record anywhere: decided without a device
    assert f(DUMMY, 25, 0, ctypes.byref(found), None) == NOT_FOUND and found.value == 25
    assert f(None, 0, 0, ctypes.byref(found), None) == NOT_FOUND and found.value == 0


@pytest.mark.parametrize("host", (False, True))
def test_salvage_argument_errors(lib, host):
    tail = () if host else (None,)
    f = lib.tkv_wal_salvage if host else lib.tkv_wal_salvage_device
    o = outs()
    R = [ctypes.byref(x) for x in o]
    for k in range(5):  # each result pointer missing
        assert f(DUMMY, 100, DUMMY, 4, DUMMY, 4, 9, *[None if i == k else R[i] for i in range(5)], *tail) == INVALID_ARGUMENT
    assert f(None, 100, DUMMY, 4, DUMMY, 4, 9, *R, *tail) == INVALID_ARGUMENT   # no image
    assert f(DUMMY, 100, None, 4, DUMMY, 4, 9, *R, *tail) == INVALID_ARGUMENT   # cap > 0, no offsets array
    assert f(DUMMY, 100, DUMMY, 4, None, 4, 9, *R, *tail) == INVALID_ARGUMENT   # gap_cap > 0, no gaps array
    assert [x.value for x in o] == [7] * 5  # results untouched by a rejected call
    assert f(None, 0, None, 0, None, 0, 9, *R, *tail) == OK
    assert [x.value for x in o] == [0] * 5


def test_geometry(lib):
    g = (U64 * 4)()
    lib.tkv_debug_wal_salvage_geometry(g)
    window, first, largest, handoff = list(g)
    assert window >= 64 and first >= window and largest >= first
    assert window == fz.DECODE_TILE
    assert handoff == 0 or handoff <= window
    last = (U64 * 6)()
    lib.tkv_debug_wal_salvage_last(last)  # callable before any salvage


def test_python_argument_checks():
    with pytest.raises(ValueError):
        tk.wal.recover(b"", mode="lenient")
    assert tk.wal.MODES == ("strict", "tolerate_tail", "skip_corrupted")
    assert tk.resync_device is tk.wal.resync_device and tk.salvage is tk.wal.salvage
