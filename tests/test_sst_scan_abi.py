"""The SSTable scan's contract without a GPU: the sequential oracle (tests/sst_scan_util.py) against the
writer's oracle, and the host parse tkv_debug_sst_scan_parse (tkv_sst_scan with every checksum comparison
skipped) against it on built files, the golden files and every structural mutation; argument errors,
sizing and each overflow kind, which both scan entry points decide without a GPU."""
import base64
import ctypes
import json
import os

import numpy as np
import pytest

import sst_build_util as bu
import sst_scan_util as su
from tinykvpp_amd._lib import BUFFER_OVERFLOW, CORRUPTED, INVALID_ARGUMENT, OK, load_library

HERE = os.path.dirname(os.path.abspath(__file__))
PARSE = "tkv_debug_sst_scan_parse"


@pytest.fixture(scope="module")
def lib():
    return load_library()


def built_cases():
    cases = {f"edge_{k}": v for k, v in bu.edge_cases().items()}
    cases.update({f"fuzz_{s}": bu.fuzz_case(s) for s in range(bu.FUZZ_SEEDS)})
    return cases


CASES = built_cases()


@pytest.fixture(scope="module")
def built():
    return {name: (ents, bu.oracle_file(ents, t)) for name, (ents, t) in CASES.items()}


def test_oracle_scan_inverts_the_writer_oracle(built):
    for name, (ents, (file, blocks, _, _)) in built.items():
        status, bad, got, gblocks = su.oracle_scan(file)
        assert (status, bad) == ("ok", len(blocks)), name
        assert got == ents, name
        assert gblocks == blocks, name


def scan_full(lib, fn, file, flags=0, tail=()):
    """Sizing call, then the full call with exactly sized, canaried outputs."""
    rc, (n, nb, ks, vs, bad) = su.call_scan(lib, fn, file, flags, tail=tail)
    if rc == CORRUPTED:
        return rc, (n, nb, ks, vs, bad), None
    assert rc in (OK, BUFFER_OVERFLOW)
    out = su.HostOutputs(n, nb, ks, vs)
    rc, sizes = su.call_scan(lib, fn, file, flags, out, tail=tail)
    assert sizes == (n, nb, ks, vs, nb)
    return rc, sizes, out


def check_ok(file, out, sizes, ents, blocks, flags=0):
    n, nb, ks, vs, bad = sizes
    assert n == len(ents) and nb == len(blocks) and bad == nb
    assert ks == sum(len(k) for k, _ in ents) and vs == sum(len(v) for _, v in ents)
    assert su.columns_entries(file, out, n, flags) == ents
    assert [(int(out.block_off[j]), int(out.block_size[j]), int(out.block_first[j])) for j in range(nb)] == blocks
    # nothing behind the sizes reported
    assert out.key_off[n] == su.CANARY64 and out.val_len[n] == su.CANARY32 and out.block_first[nb] == su.CANARY32
    if not flags & su.KEY_VIEWS:
        assert (out.keys[ks:] == su.CANARY8).all()
        assert [int(x) for x in out.key_off[:n]] == list(np.cumsum([0] + [len(k) for k, _ in ents])[:-1])
    else:
        assert (out.keys == su.CANARY8).all()
    if not flags & su.VAL_VIEWS:
        assert (out.vals[vs:] == su.CANARY8).all()
    else:
        assert (out.vals == su.CANARY8).all()


def test_parse_matches_the_oracle_on_built_files(lib, built):
    for name, (ents, (file, blocks, _, _)) in built.items():
        rc, sizes, out = scan_full(lib, PARSE, file)
        assert rc == OK, name
        check_ok(file, out, sizes, ents, blocks)


def test_parse_ignores_the_stamps(lib, built):
    ents, (file, blocks, _, _) = built["edge_uniform"]
    rc, sizes, out = scan_full(lib, PARSE, bu.unstamped(file, blocks))
    assert rc == OK
    check_ok(file, out, sizes, ents, blocks)


@pytest.mark.parametrize("flags", [su.KEY_VIEWS, su.VAL_VIEWS, su.KEY_VIEWS | su.VAL_VIEWS])
def test_parse_views(lib, built, flags):
    for name in ("edge_T_1", "edge_one_larger_than_T", "fuzz_3", "fuzz_4"):
        ents, (file, blocks, _, _) = built[name]
        rc, sizes, out = scan_full(lib, PARSE, file, flags)
        assert rc == OK, name
        check_ok(file, out, sizes, ents, blocks, flags)


MUT = su.mutations()


@pytest.mark.parametrize("name", sorted(MUT))
def test_oracle_verdict_of_every_mutation(name):
    file, expect = MUT[name]
    status, bad, ents, blocks = su.oracle_scan(file)
    if expect == "ok":
        assert status == "ok" and bad == len(blocks)
    else:
        assert (status, bad) == ("corrupted", expect)
        # and it is the structure, not a stamp, that fails (but for the two checksum mutations)
        if name not in ("footer_crc", "block_crc", "two_bad_blocks"):
            assert su.oracle_scan(file, check_crc=False)[:2] == ("corrupted", expect)


@pytest.mark.parametrize("name", sorted(MUT))
def test_parse_verdict_of_every_mutation(lib, name):
    file, _ = MUT[name]
    status, bad, ents, blocks = su.oracle_scan(file, check_crc=False)
    if status == "ok":
        rc, sizes, out = scan_full(lib, PARSE, file)
        assert rc == OK
        check_ok(file, out, sizes, ents, blocks)
        return
    out = su.HostOutputs(64, 8, 4096, 4096)
    rc, sizes = su.call_scan(lib, PARSE, file, 0, out)
    assert rc == CORRUPTED and sizes == (0, 0, 0, 0, bad)
    assert out.untouched()


def test_golden_files(lib):
    with open(os.path.join(HERE, "golden", "sst_build.json")) as f:
        gold = json.load(f)
    cases = gold["cases"] if isinstance(gold, dict) and "cases" in gold else gold
    seen = 0
    for case in (cases.values() if isinstance(cases, dict) else cases):
        file = golden_file(case)
        if file is None:
            continue
        seen += 1
        status, bad, ents, blocks = su.oracle_scan(file)
        assert status == "ok"
        rc, sizes, out = scan_full(lib, PARSE, file)
        assert rc == OK
        check_ok(file, out, sizes, ents, blocks)
    assert seen == 4


def golden_file(case):
    for key in ("file_hex", "file", "file_b64"):
        if isinstance(case, dict) and key in case:
            v = case[key]
            return bytes.fromhex(v) if key != "file_b64" else base64.b64decode(v)
    return None


# ---- decided without a GPU, by the debug call and by both scan entry points ---------------------------

ENTRY_POINTS = [(PARSE, ()), ("tkv_sst_scan", ()), ("tkv_sst_scan_device", (None,))]


@pytest.mark.parametrize("fn,tail", ENTRY_POINTS)
def test_argument_errors(lib, fn, tail):
    file = MUT["base"][0]
    buf = np.frombuffer(file, np.uint8).copy()
    res = [ctypes.c_uint64(0x5EED) for _ in range(5)]
    refs = [ctypes.byref(r) for r in res]
    nulls = [None, None, None, None, 0, None, 0, None, 0, None, None, None, 0]
    f = getattr(lib, fn)
    fp = ctypes.c_void_p(buf.ctypes.data)
    assert f(None, buf.size, 0, *nulls, *refs, *tail) == INVALID_ARGUMENT
    assert f(fp, buf.size, 4, *nulls, *refs, *tail) == INVALID_ARGUMENT
    assert f(fp, buf.size, 0x80000001, *nulls, *refs, *tail) == INVALID_ARGUMENT
    assert f(fp, 2**32, 0, *nulls, *refs, *tail) == INVALID_ARGUMENT
    for k in range(5):
        r = list(refs)
        r[k] = None
        assert f(fp, buf.size, 0, *nulls, *r, *tail) == INVALID_ARGUMENT
    assert all(r.value == 0x5EED for r in res)


@pytest.mark.parametrize("fn,tail", ENTRY_POINTS)
@pytest.mark.parametrize("size", [0, 1, 27])
def test_short_file_is_a_bad_footer(lib, fn, tail, size):
    out = su.HostOutputs(4, 4, 16, 16)
    rc, sizes = su.call_scan(lib, fn, b"\x14" * size, 0, out, tail=tail)
    assert rc == CORRUPTED and sizes == (0, 0, 0, 0, su.BAD_FOOTER)
    assert out.untouched()


@pytest.mark.parametrize("fn,tail", [(PARSE, ()), ("tkv_sst_scan", ())])
def test_footer_fields_fail_without_a_gpu(lib, fn, tail):
    for name in ("footer_sum_plus_1", "footer_sum_minus_1", "index_size_7"):
        out = su.HostOutputs(4, 4, 16, 16)
        rc, sizes = su.call_scan(lib, fn, MUT[name][0], 0, out, tail=tail)
        assert rc == CORRUPTED and sizes == (0, 0, 0, 0, su.BAD_FOOTER)
        assert out.untouched()


def test_sizing_and_each_overflow_kind(lib, built):
    ents, (file, blocks, _, _) = built["edge_uniform"]
    rc, (n, nb, ks, vs, bad) = su.call_scan(lib, PARSE, file)
    assert rc == BUFFER_OVERFLOW and (n, nb, bad) == (len(ents), len(blocks), len(blocks))
    assert ks == 16 * n and vs == 17 * n
    for caps in ((n - 1, nb, ks, vs), (n, nb - 1, ks, vs), (n, nb, ks - 1, vs), (n, nb, ks, vs - 1)):
        out = su.HostOutputs(n, nb, ks, vs)
        rc, sizes = su.call_scan(lib, PARSE, file, 0, out, caps=caps)
        assert rc == BUFFER_OVERFLOW and sizes == (n, nb, ks, vs, nb), caps
        assert out.untouched(), caps
    # a views arena has no cap
    out = su.HostOutputs(n, nb, ks, vs)
    rc, sizes = su.call_scan(lib, PARSE, file, su.KEY_VIEWS | su.VAL_VIEWS, out, caps=(n, nb, 0, 0))
    assert rc == OK
    check_ok(file, out, sizes, ents, blocks, su.KEY_VIEWS | su.VAL_VIEWS)
    # the empty table and a table without a key or value byte need no arena
    rc, sizes = su.call_scan(lib, PARSE, MUT["empty_table_ok"][0])
    assert rc == OK and sizes == (0, 0, 0, 0, 0)
    rc, sizes = su.call_scan(lib, PARSE, MUT["empty_key_value_80_00_ok"][0])
    assert rc == OK and sizes == (1, 1, 0, 0, 1)


def test_nullable_arrays(lib, built):
    ents, (file, blocks, _, _) = built["fuzz_3"]
    rc, (n, nb, ks, vs, _) = su.call_scan(lib, PARSE, file)
    buf = np.frombuffer(file, np.uint8).copy()
    res = [ctypes.c_uint64(0) for _ in range(5)]
    klen, bfirst = np.zeros(n, np.uint32), np.zeros(nb, np.uint32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    rc = lib.tkv_debug_sst_scan_parse(p(buf), buf.size, su.KEY_VIEWS | su.VAL_VIEWS, None, p(klen), None, None, n, None, 0,
                                      None, 0, None, None, p(bfirst), nb, *[ctypes.byref(r) for r in res])
    assert rc == OK
    assert list(klen) == [len(k) for k, _ in ents] and list(bfirst) == [b[2] for b in blocks]


def test_python_wrappers_check_their_arguments():
    from tinykvpp_amd import sst
    with pytest.raises(ValueError):
        sst.scan(np.zeros(40, np.uint32))
    with pytest.raises(ValueError):
        sst.scan(np.zeros((4, 10), np.uint8))
    with pytest.raises(ValueError):
        sst.scan_device(np.zeros(40, np.uint8))
    with pytest.raises(sst.SstCorrupted) as e:
        sst.scan(b"\0" * 27)
    assert e.value.bad_block == "footer"
    with pytest.raises(sst.SstCorrupted) as e:
        sst.scan(MUT["footer_sum_plus_1"][0])
    assert e.value.bad_block == "footer"


def test_every_single_bit_flip_of_a_small_file(lib):
    """One flipped bit in every byte of a file of about 600 bytes with three blocks (the bit chosen by a
    fixed seed, the same as on the device): the oracle never answers ok, and the parse, which compares no
    checksum, gives the oracle's verdict without the checksums."""
    file = MUT["base"][0]
    assert 600 <= len(file) <= 800
    bits = np.random.default_rng(0xB17).integers(0, 8, len(file))
    out = su.HostOutputs(16, 8, 1024, 1024)
    structural = 0
    for pos in range(len(file)):
        mutated = bytearray(file)
        mutated[pos] ^= 1 << int(bits[pos])
        assert su.oracle_scan(bytes(mutated))[0] == "corrupted", pos
        status, bad, ents, blocks = su.oracle_scan(bytes(mutated), check_crc=False)
        if status == "corrupted":
            structural += 1
            rc, sizes = su.call_scan(lib, PARSE, bytes(mutated), 0, out)
            assert rc == CORRUPTED and sizes == (0, 0, 0, 0, bad), pos
            assert out.untouched()
        else:
            rc, sizes, got = scan_full(lib, PARSE, bytes(mutated))
            assert rc == OK, pos
            check_ok(bytes(mutated), got, sizes, ents, blocks)
    assert structural > 100
