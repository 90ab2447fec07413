"""tkv_wal_decode_device on the GPU: the golden records and a small batch at every arena alignment in all
four flag combinations with u64 and u32 offsets, spans around the lane / wave limit, corruption and
overflow (nothing written), the closed loop encode -> index -> decode -> encode, and recovery. Expected
values are the numpy restatement of wal.cpp:98-125 (wal_decode_util.expected) on images from the numpy
encode (wal_encode_util.expected); every byte and record is compared, every arena lies between 0xA5
sentinels."""
import numpy as np
import pytest

import tinykvpp_amd as tk
from conftest import golden
from test_gpu_wal_encode import small_batch
from tinykvpp_amd._lib import BUFFER_OVERFLOW, CORRUPTED
from wal_decode_util import (COLS, FLAGS, KEY_VIEWS, VAL_VIEWS, DevOut, check_device, corrupt, decode_device, dev_offsets,
                             expected, first_bad, geometry, last)
from wal_encode_util import geometry as enc_geometry
from wal_encode_util import loop_pattern, make_batch
from wal_encode_util import expected as encoded

pytestmark = pytest.mark.gpu


def upload(gpu, img):
    import torch
    return torch.from_numpy(img).to(gpu)


@pytest.fixture(scope="module")
def golden_case(gpu):
    raw = [bytes.fromhex(r["hex"]) for r in golden("wal.json")["records"]]
    img = np.frombuffer(b"".join(raw), np.uint8).copy()
    offs = np.cumsum([0] + [len(r) for r in raw[:-1]]).astype(np.uint64)
    return img, offs, upload(gpu, img)


@pytest.fixture(scope="module")
def small_case(gpu, oracle):
    b = small_batch(np.random.default_rng(1301), 1000)
    img, offs, _ = encoded(b, oracle)
    return img, offs, upload(gpu, img)


@pytest.mark.parametrize("flags", FLAGS)
def test_golden_and_small_every_alignment(gpu, lib, golden_case, small_case, flags):
    for img, offs, image in (golden_case, small_case):
        want = expected(img, offs, flags)
        for align in range(16):
            for u32 in (False, True):  # both offset widths against the same expected values
                check_device(lib, gpu, image, img, offs, flags, kalign=align, valign=(align + 5) % 16, u32=u32, want=want)


def test_side_stream(gpu, lib, small_case):
    import torch
    img, offs, image = small_case
    s = torch.cuda.Stream(gpu)
    for flags in FLAGS:
        check_device(lib, gpu, image, img, offs, flags, kalign=3, valign=9, stream=s.cuda_stream)
    b = tk.wal.decode_device(image, dev_offsets(gpu, offs), stream=s)
    s.synchronize()
    want = expected(img, offs)
    assert np.array_equal(b.keys.cpu().numpy(), want["keys"]) and np.array_equal(b.vals.cpu().numpy(), want["vals"])


def test_lane_wave_boundary(gpu, lib, oracle):
    """Key and value lengths around the longest span a lane copies, each as key and as value, in every
    pairing, at shifting residues."""
    lim = geometry(lib)[2]
    assert lim == 64
    edge = (0, 1, lim - 1, lim, lim + 1)
    klen = [k for k in edge for _ in edge] * 7
    vlen = [v for _ in edge for v in edge] * 7
    rng = np.random.default_rng(1302)
    p = rng.permutation(len(klen))
    b = make_batch(rng, np.array(klen)[p], np.array(vlen)[p])
    img, offs, _ = encoded(b, oracle)
    image = upload(gpu, img)
    for flags, ka, va in ((0, 0, 0), (0, 7, 13), (KEY_VIEWS, 0, 1), (VAL_VIEWS, 15, 0)):
        check_device(lib, gpu, image, img, offs, flags, kalign=ka, valign=va)


def test_permuted_duplicate_and_slack(gpu, lib, small_case):
    img, offs, _ = small_case
    rng = np.random.default_rng(1303)
    at, nxt = int(offs[500]), int(offs[501])
    slack = np.concatenate([img[:nxt], np.full(5, 0xEE, np.uint8), img[nxt:]])
    rl = int.from_bytes(slack[at:at + 4].tobytes(), "little") + 5
    slack[at:at + 4] = np.frombuffer(rl.to_bytes(4, "little"), np.uint8)
    o2 = offs.copy()
    o2[501:] += np.uint64(5)
    p = rng.permutation(o2.size)
    p[17] = p[3]
    image = upload(gpu, slack)
    for flags in FLAGS:
        check_device(lib, gpu, image, slack, o2[p], flags, kalign=11, valign=6)


def test_delete_only_wal(gpu, lib, oracle):
    rng = np.random.default_rng(1304)
    b = make_batch(rng, rng.integers(1, 24, 300), np.zeros(300, np.int64))
    img, offs, _ = encoded(b, oracle)
    want = expected(img, offs)
    out = DevOut(gpu, 300, want["keys_size"], None, 4)
    assert decode_device(lib, upload(gpu, img), dev_offsets(gpu, offs), 0, out) == (0, want["keys_size"], 0, 300)
    assert np.array_equal(out.arena("keys", want["keys_size"]).cpu().numpy(), want["keys"])
    st = last(lib)
    assert out.guards_ok(want["keys_size"], 0) and st[0] > 0 and st[1] == 0


def test_image_placement(gpu, lib, oracle):
    """The image at the first byte of its allocation and ending at its last byte (a tensor made exactly
    that size, of a size that is no multiple of 16): the granule rule of the loads."""
    import torch
    rng = np.random.default_rng(1305)
    klen, vlen = np.r_[rng.integers(0, 24, 400), 70, 3], np.r_[rng.integers(0, 200, 400), 9, 131]
    vlen[-1] += int((26 * klen.size + klen.sum() + vlen.sum()) % 16 == 0)
    b = make_batch(rng, klen, vlen)
    img, offs, _ = encoded(b, oracle)
    assert img.size % 16 != 0
    image = torch.empty(img.size, dtype=torch.uint8, device=gpu)
    image.copy_(torch.from_numpy(img))
    assert image.storage_offset() == 0 and image.untyped_storage().nbytes() == img.size
    for flags in FLAGS:
        check_device(lib, gpu, image, img, offs, flags, kalign=2, valign=14)


@pytest.mark.parametrize("kind", ("short", "record_len", "key_len"))
def test_corruption_writes_nothing(gpu, lib, small_case, kind):
    img, offs, _ = small_case
    n = offs.size
    for i in (0, n // 2, n - 1):
        bimg, size, boffs = corrupt(kind, img, offs, i)
        assert first_bad(bimg, boffs, size) == i
        image = upload(gpu, bimg)
        for flags, u32 in ((0, False), (KEY_VIEWS | VAL_VIEWS, True)):
            out = DevOut(gpu, n, 1 << 17, 1 << 17, 5, 5)
            assert decode_device(lib, image, dev_offsets(gpu, boffs, u32), flags, out, size=size) == (CORRUPTED, 0, 0, i)
            assert out.untouched() and last(lib) == [0, 0, 0, 0]


def test_two_bad_records_and_the_prefix(gpu, lib, small_case):
    img, offs, _ = small_case
    bimg, size, boffs = corrupt("record_len", img, offs, 700)
    bimg, size, boffs = corrupt("short", bimg, boffs, 123)
    image = upload(gpu, bimg)
    out = DevOut(gpu, offs.size, 1 << 17, 1 << 17)
    assert decode_device(lib, image, dev_offsets(gpu, boffs), 0, out, size=size) == (CORRUPTED, 0, 0, 123)
    assert out.untouched() and last(lib) == [0, 0, 0, 0]
    check_device(lib, gpu, image, bimg, boffs[:123], 0, kalign=1, valign=1)
    with pytest.raises(ValueError, match="record 123"):
        tk.wal.decode_device(image, dev_offsets(gpu, boffs))


def test_overflow_and_sizing(gpu, lib, small_case):
    img, offs, image = small_case
    want = expected(img, offs)
    K, V, n = want["keys_size"], want["vals_size"], offs.size
    doffs = dev_offsets(gpu, offs)
    for short_k, short_v in ((1, 0), (0, 1)):
        out = DevOut(gpu, n, K, V, 3, 8)
        out.kcap -= short_k
        out.vcap -= short_v
        assert decode_device(lib, image, doffs, 0, out) == (BUFFER_OVERFLOW, K, V, n)
        assert out.untouched() and last(lib) == [0, 0, 0, 0]
    out = DevOut(gpu, n, None, None)
    assert decode_device(lib, image, doffs, 0, out) == (BUFFER_OVERFLOW, K, V, n) and out.untouched()  # the sizing call


def loop_batch(lib, seed, size):
    rng = np.random.default_rng(seed)
    b = loop_pattern(rng, size, enc_geometry(lib)[0])
    b["tomb"] = rng.integers(0, 2, b["n"]).astype(np.uint8)  # the shape the reference encoder writes
    return b


@pytest.mark.parametrize("views", (False, True))
def test_closed_loop(gpu, lib, oracle, views):
    """encode -> index -> decode -> encode: the second image equals the first byte for byte (CRC fields
    included) and the decoded columns equal the inputs; with copied arenas, and with both arenas as views
    re-encoded with keys = vals = image."""
    import torch
    b = loop_batch(lib, 1306, 1 << 20)
    t = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else  # noqa: E731
                                   a.view(np.int32) if a.dtype == np.uint32 else a).to(gpu)
    first, rec_off, _ = tk.wal.encode_device(t(b["keys"]), t(b["key_off"]), t(b["key_len"]), t(b["vals"]), t(b["val_off"]),
                                             t(b["val_len"]), t(b["op"]), t(b["tomb"]), t(b["seq"]))
    assert np.array_equal(first.cpu().numpy(), encoded(b, oracle)[0])
    status, offs, stop, max_seq = tk.wal.index_device(first)
    assert (status, stop, max_seq) == ("ok", first.numel(), int(b["seq"].max())) and torch.equal(offs, rec_off)
    d = tk.wal.decode_device(first, offs, key_views=views, val_views=views)
    for k in ("op", "tomb", "seq", "key_len", "val_len"):
        assert np.array_equal(getattr(d, k).cpu().numpy().view(b[k].dtype), b[k]), k
    if views:
        assert d.keys is first and d.vals is first
    second, rec_off2, _ = tk.wal.encode_device(d.keys, d.key_off, d.key_len, d.vals, d.val_off, d.val_len, d.op, d.tomb, d.seq)
    assert torch.equal(second, first) and torch.equal(rec_off2, rec_off)


def test_recover(gpu, lib, oracle):
    """recover_device on a clean image and on one with a corrupted record in the middle: status,
    stop_offset and max_sequence are index_device's, the batch is exactly the good prefix, and recover on
    the host gives the same arrays."""
    b = loop_batch(lib, 1307, 1 << 18)
    img, offs, _ = encoded(b, oracle)
    bad = img.copy()
    mid = b["n"] // 2
    bad[int(offs[mid]) + 9] ^= 0x40  # a sequence byte: the checksum fails, the structure holds
    for data, good in ((img, b["n"]), (bad, mid)):
        image = upload(gpu, data)
        ist, ioffs, istop, iseq = tk.wal.index_device(image)
        status, batch, stop, max_seq = tk.wal.recover_device(image)
        assert (status, stop, max_seq) == (ist, istop, iseq) and ioffs.numel() == good
        assert status == ("ok" if good == b["n"] else "corrupted")
        want = expected(data, offs[:good])
        hstatus, hbatch, hstop, hseq = tk.wal.recover(data)
        assert (hstatus, hstop, hseq) == (status, stop, max_seq)
        for k in COLS + ("keys", "vals"):
            got = getattr(batch, k).cpu().numpy()
            assert np.array_equal(got.view(want[k].dtype), want[k]), k
            assert np.array_equal(getattr(hbatch, k), want[k]), k
        status, vb, _, _ = tk.wal.recover_device(image, key_views=True, val_views=True)
        assert vb.keys is image and vb.vals is image
        assert np.array_equal(vb.key_off.cpu().numpy().view(np.uint64), offs[:good] + np.uint64(26))
