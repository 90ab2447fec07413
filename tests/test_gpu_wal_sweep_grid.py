"""The device WAL sweep (wal_sweep, wal_idx_emit and verify_locked in tkv_wal_device.hip) over the images
of wal_sweep_util, at every alignment of the image's base and at every chunking.

The sweep's header search, its carry fold and its last load all depend on o = base & 15; and its chunks
hold one region per wave for every image below about 22 MB, where every region's entry is speculative.
tkv_debug_set_wal_sweep_waves caps the waves, so that a 2 MiB image runs chunks of many regions with
exact entries (the path of the large images): the carry of a whole region, the register ring in steady
state, the pass-over of a record longer than kMedMax and the pipeline restart behind it.
tkv_debug_wal_sweep_geometry tells which chunking ran.

Every run sends one image, at byte `shift` of its allocation, through tkv_wal_verify_device and
tkv_wal_index_device (both offset widths, sentinel-padded) and compares verdict, n_good, stop offset,
every start and max_sequence with wal_fuzz_util.decode; nothing may be written at or past
min(n_good, cap). The clean images hold no plausible header off the chain
(test_wal_sweep_grid_cpu.py), so every speculative start is a record start and every boundary holds:
a sweep that needs a fix-up round there missed or misplaced a header.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import tinykvpp_amd as tk
import wal_salvage_util as su
import wal_sweep_util as sw
from test_gpu_wal_index import SENT32, SENT64, index_raw, to_device, wal_last
from wal_fuzz_util import REGION, decode
from wal_sweep_util import SEED_CHUNK, SEED_START

pytestmark = pytest.mark.gpu

SWEEP_WAVES_PER_CU = 12  # kSweepWaves: cap_waves = CUs x 12
WHICH = ("start_phase", "chunk")


class Case:
    """An image (or its first `size` bytes) with the decode's results, made once."""

    def __init__(self, oracle, img, size=None):
        self.size = img.size if size is None else size
        self.img = img
        self.want, self.starts, self.mseq = decode(oracle, img, self.size)
        self.nreg = (self.size + REGION - 1) // REGION


@pytest.fixture(scope="module")
def images(gpu, oracle):
    """{name: (Case, offs, sizes)} of the two clean images."""
    out = {}
    for name, build, seed in (("start_phase", sw.start_phase_image, SEED_START), ("chunk", sw.chunk_image, SEED_CHUNK)):
        img, offs, sizes, _ = build(np.random.default_rng(seed), oracle)
        c = Case(oracle, img)
        assert c.want == ("ok", offs.size, img.size)
        out[name] = (c, offs, sizes)
    return out


@pytest.fixture(scope="module")
def mutated(oracle, images):
    """{(which, mutation name): (Case, record index)}."""
    out = {}
    for which, (c, offs, sizes) in images.items():
        for name, (i, _, apply) in sw.mutations(oracle, c.img, offs, sizes).items():
            m = c.img.copy()
            apply(m)
            out[which, name] = (Case(oracle, m), i)
    return out


@pytest.fixture(scope="module")
def tails(oracle, images):
    c, offs, sizes = images["start_phase"]
    return [Case(oracle, c.img, n) for n in sw.tail_sizes(offs, sizes)]


def geometry():
    g = (ctypes.c_uint64 * 4)()
    tk.load_library().tkv_debug_wal_sweep_geometry(g)
    return {"region": g[0], "piece": g[1], "waves": g[2], "nreg": g[3]}


def cap_waves():
    return torch.cuda.get_device_properties(0).multi_processor_count * SWEEP_WAVES_PER_CU


@contextlib.contextmanager
def sweep_waves(waves):
    """tkv_debug_set_wal_sweep_waves(waves) for a block, the previous value put back behind it; None
    leaves the default."""
    if waves is None:
        yield
        return
    lib = tk.load_library()
    prev = lib.tkv_debug_set_wal_sweep_waves(waves)
    try:
        yield
    finally:
        lib.tkv_debug_set_wal_sweep_waves(prev)


def run(c, shift, waves=None):
    """One image through the verify and the index against the decode. Returns what tkv_debug_wal_last
    says of the verify and of the index, and the raw outputs."""
    view = to_device(c.img, c.size, shift)
    assert c.size == 0 or view.data_ptr() % 16 == shift
    cap = c.size // 26
    with sweep_waves(waves):
        verdict = tk.wal.verify_device(view, c.size)
        last_v, geo_v = wal_last(), geometry()
        got, o64, o32, seq = index_raw(view, c.size, cap)
        last_i, geo_i = wal_last(), geometry()
    note = (shift, waves, verdict, got, c.want)
    assert verdict == c.want, note
    assert got == c.want, note
    k = min(c.want[1], cap)
    assert np.array_equal(o64[:k].view(np.uint64), c.starts[:k]), note
    assert np.array_equal(o32[:k].view(np.uint32), c.starts[:k].astype(np.uint32)), note
    assert (o64[k:] == SENT64).all() and (o32[k:] == SENT32).all(), "an entry at or past min(n_good, cap) was written"
    assert seq == c.mseq, note
    assert last_v["host_walk"] == 0 and last_i["host_walk"] == 0, (note, last_v, last_i)
    want_w = min(c.nreg, cap_waves()) if waves is None else min(c.nreg, cap_waves(), waves)
    for g in (geo_v, geo_i):
        assert (g["region"], g["waves"], g["nreg"]) == (REGION, want_w, c.nreg), (note, g)
    return (last_v, last_i), (got, o64, o32, seq)


def one_pass(lasts, note):
    for last in lasts:
        assert last["passes"] == 1 and last["fast"] == 1, (note, last)


# ---- 1. every alignment -------------------------------------------------------------------------------------

@pytest.mark.parametrize("shift", range(16))
@pytest.mark.parametrize("which", WHICH)
def test_every_alignment(images, which, shift):
    """Both clean images at every base & 15, one region per wave. No fix-up round at any shift: with no
    plausible header off the chain, a speculative start that is not a record start, or a region that
    finds none where one lies, is a fault of the search (its 16 masks of the positions in front of the
    piece, sh = (piece start + o + 8) & 15), and a boundary that fails is one of the walk."""
    c = images[which][0]
    assert c.nreg <= cap_waves()  # one region per wave
    lasts, _ = run(c, shift)
    one_pass(lasts, (which, shift))


# ---- 2. every chunking --------------------------------------------------------------------------------------

@pytest.mark.parametrize("waves", [1, 2, 3, 5])
@pytest.mark.parametrize("which", WHICH)
def test_every_chunking(images, which, waves):
    """Chunks of nreg / waves regions: exact entries, whole-region carries, the ring in steady state, the
    pass-over and the restart. One chunk entered at 0 has no speculative boundary at all."""
    c = images[which][0]
    assert c.nreg >= 4 * waves
    for shift in (0, 1, 5, 15):
        lasts, _ = run(c, shift, waves)
        assert geometry()["waves"] == waves
        if waves == 1:
            one_pass(lasts, (which, shift))


# ---- 3. mutations -------------------------------------------------------------------------------------------

MUTATED = [("chunk", m) for m in sw.MUTATIONS] + [("start_phase", m) for m in ("cut_d1", "cut_d8", "cut_d26", "record_len_17")]


@pytest.mark.parametrize("which,name", MUTATED)
def test_mutations(images, mutated, which, name):
    """One corrupted record at a time, at one region per wave and in chunks of many regions."""
    c, i = mutated[which, name]
    offs = images[which][1]
    assert c.want == ("corrupted", i, int(offs[i]))
    for waves in (1, 3, None):
        for shift in (0, 7):
            run(c, shift, waves)


# ---- 4. tails -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shift", range(16))
def test_tails_every_alignment(tails, shift):
    """The image cut inside a record that starts 10 bytes before a region end: the descriptor's end
    follows (o + size) & 15, and the last region holds the record's first 10 bytes at the most."""
    for c in tails:
        run(c, shift)


@pytest.mark.parametrize("shift", [0, 9])
def test_tails_one_wave(tails, shift):
    for c in tails:
        run(c, shift, 1)


# ---- 5. salvage through the capped sweep ----------------------------------------------------------------------

@pytest.mark.parametrize("waves", [1, None])
def test_salvage_through_the_sweep(oracle, images, waves):
    """One flipped bit: the salvage indexes the image, then the sub-image behind the gap, which begins
    at an arbitrary byte of the buffer."""
    c, offs, sizes = images["start_phase"]
    img = c.img.copy()
    bad = offs.size // 3
    img[int(offs[bad]) + 11] ^= 0x20
    status, starts, gaps, stop, mseq, _ = su.salvage(oracle, img, img.size)
    assert status == "corrupted" and starts.size == offs.size - 1 and gaps.tolist() == [[int(offs[bad]), int(offs[bad + 1])]]
    for shift in (0, 5):
        view = to_device(img, img.size, shift)
        with sweep_waves(waves):
            got = tk.wal.salvage_device(view)
        assert (got[0], got[3], got[4]) == (status, stop, mseq), (waves, shift)
        assert np.array_equal(got[1].cpu().numpy().view(np.uint64), starts), (waves, shift)
        assert np.array_equal(got[2], gaps), (waves, shift)
        sub = img.size - int(gaps[-1, 1])  # the last sweep ran over the sub-image behind the gap
        g = geometry()
        assert g["nreg"] == (sub + REGION - 1) // REGION
        assert g["waves"] == min(g["nreg"], cap_waves() if waves is None else waves)


# ---- 6. the hook is inert when unset ------------------------------------------------------------------------

def test_hook_is_inert_when_unset(images):
    c = images["chunk"][0]
    lib = tk.load_library()
    assert lib.tkv_debug_set_wal_sweep_waves(0) == 0  # unset on entry, as every test above leaves it
    _, before = run(c, 3)
    assert geometry()["waves"] == min(c.nreg, cap_waves())
    run(c, 3, 2)
    assert geometry()["waves"] == 2
    assert lib.tkv_debug_set_wal_sweep_waves(0) == 0  # restored by the block above
    _, after = run(c, 3)
    assert geometry()["waves"] == min(c.nreg, cap_waves())
    assert before[0] == after[0] and before[3] == after[3]
    assert np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
