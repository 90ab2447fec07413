"""The WAL fuzz cases (wal_fuzz_util.case) without a GPU: the helper's sequential decode against the
independent C decode of the test oracle (oracle_wal_decode) for every seed the GPU test runs, the
counts that prove the seed range holds every situation the fuzz exists for, and tkv_wal_decode_host over
every case's good records in all four flag combinations."""
import numpy as np
import pytest

import wal_fuzz_util as fz
from wal_decode_util import FLAGS, check_host, geometry
from wal_encode_util import geometry as enc_geometry


@pytest.fixture(scope="module")
def cases(oracle):
    """case(seed) for every seed, made once for this module."""
    made = {}

    def get(seed):
        if seed not in made:
            made[seed] = fz.case(seed, oracle)
        return made[seed]
    return get


def test_profile_constants_are_the_kernels(lib):
    """The lengths the profiles sit on, against what the library reports."""
    tile, per_wg, lane_max, _ = geometry(lib)
    etile, eper_wg, fold_max, _ = enc_geometry(lib)
    assert (tile, etile) == (fz.DECODE_TILE, fz.DECODE_TILE)
    assert (per_wg, eper_wg) == (fz.SCAN_BLOCK, fz.SCAN_BLOCK)
    assert lane_max == fz.SHORT_SPAN and fold_max == fz.LANE_FOLD
    assert fz.REGION == 64 * fz.LANE_PIECE


@pytest.mark.parametrize("seed", fz.SEEDS)
def test_helper_decode_equals_the_c_oracle(oracle, cases, seed):
    """Checks the checker: (status, n_good, stop) of the helper's decode equals oracle_wal_decode's."""
    wi, ora = fz._wal_images()
    c = cases(seed)
    assert c.verdict == wi.decode(ora, np.ascontiguousarray(c.img), c.size), (c.profile, c.count, c.kind, c.notes)
    assert c.starts.size == c.n_good and (c.n_good == 0 or int(c.starts[-1]) < c.stop)
    if c.kind == "none":
        assert c.verdict == ("ok", c.count, c.size)
    elif c.kind == "merge":
        assert c.verdict == ("ok", c.count - c.notes["swallowed"], c.size)
    elif c.kind != "appended":
        assert c.status == "corrupted" and c.n_good == c.notes["victim"]


def test_coverage(oracle, cases):
    """The seed range holds every situation at least once, and at most a quarter of the seeds cannot run
    the closed loop (their good prefix is not what the reference encoder writes)."""
    cov = fz.coverage([cases(s) for s in fz.SEEDS])
    print("coverage over", len(fz.SEEDS), "seeds:", cov)
    for k in ("no_good_nonempty", "empty_image", "stop_at_last_record", "torn_in_header", "torn_in_payload",
              "structural_behind_valid_crc", "slack_in_good_prefix", "record_len_near_med_max", "three_regions",
              "host_threads", "chain_goes_on"):
        assert cov[k] >= 1, (k, cov)
    assert 4 * cov["no_closed_loop"] <= len(fz.SEEDS), cov
    kinds = {cases(s).kind for s in fz.SEEDS}
    assert kinds == set(fz.KINDS), kinds
    assert {cases(s).profile for s in fz.SEEDS} == set(fz.PROFILES)
    assert {cases(s).shift for s in fz.SEEDS} >= {0, 15}


@pytest.mark.parametrize("seed", fz.SEEDS)
def test_host_decode_of_every_case(lib, cases, seed):
    """tkv_wal_decode_host over the good starts in all four flag combinations, sentinels included."""
    c = cases(seed)
    for flags in FLAGS:
        check_host(lib, c.img, c.starts, flags, kalign=(seed + 3 * flags) % 16, valign=(5 * seed + flags) % 16)
