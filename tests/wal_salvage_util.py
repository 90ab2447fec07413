"""The sequential WAL salvage and resync every tkv_wal_salvage / tkv_wal_resync_device test is compared
with. Numpy and the test oracle only: no GPU, no product library.

valid(p) for an image [0, size) (64-bit arithmetic): size - p >= 26; rl + 8 <= size - p; 18 + kl + vl <=
rl; CRC-32 of [p + 8, p + 8 + rl) == the u32 at p + 4 - the checks of wal_fuzz_util.records_expected.
resync(from) is the smallest valid p >= from; the salvage is
    p = 0; while p < size: valid(p) ? (emit p, p += 8 + rl) : (p is skipped, p += 1)
and a gap a maximal run of skipped bytes. `salvage` runs it as the loop it equals: wal_fuzz_util.decode
on the sub-image [p, size), a gap opened at its stop s, closed at resync(s + 1). `resync` is a numpy
filter of checks 1-3 over growing ranges, then records_expected on the survivors in order.
`brute_salvage` is the program itself, byte by byte, for small images.
"""
import numpy as np

import wal_fuzz_util as fz

META = 26


def u32_at_every_offset(img, lo, hi):
    """The u32 LE at each of the offsets [lo, hi) (hi + 3 <= img.size), as uint64."""
    b = img[lo:hi + 3].astype(np.uint64)
    n = hi - lo
    return b[0:n] | (b[1:n + 1] << np.uint64(8)) | (b[2:n + 2] << np.uint64(16)) | (b[3:n + 3] << np.uint64(24))


def structural(img, size, lo, hi):
    """The positions of [lo, hi) that pass checks 1-3 (int64, increasing)."""
    hi = min(hi, size - META + 1)
    if hi <= lo:
        return np.zeros(0, np.int64)
    u = u32_at_every_offset(img, lo, hi + 22)
    n = hi - lo
    p = np.arange(lo, hi, dtype=np.uint64)
    rl, kl, vl = u[0:n], u[18:18 + n], u[22:22 + n]
    ok = (rl + np.uint64(8) <= np.uint64(size) - p) & (np.uint64(18) + kl + vl <= rl)
    return p[ok].astype(np.int64)


def resync(oracle, img, size, start, first_span=1 << 16, batch=64):
    """The smallest valid p >= start, or None."""
    img = img[:size]
    pos, span = start, first_span
    while pos < size - META + 1:
        hi = min(pos + span, size - META + 1)
        cand = structural(img, size, pos, hi)
        for i in range(0, cand.size, batch):
            _, ok = fz.records_expected(oracle, img, size, cand[i:i + batch])
            hit = np.flatnonzero(ok)
            if hit.size:
                return int(cand[i + hit[0]])
        pos, span = hi, span * 4
    return None


def salvage(oracle, img, size, max_gaps=None):
    """(status, starts uint64, gaps (k, 2) uint64, stop_offset, max_sequence, bytes_skipped)."""
    img = img[:size]
    p, recs, gaps, stop, mseq = 0, [], [], size, 0
    while p < size:
        (status, _, rel), starts, ms = fz.decode(oracle, img[p:], size - p)
        recs.append(starts + np.uint64(p))
        mseq = max(mseq, ms)
        if status == "ok":
            break
        s = p + rel
        if max_gaps is not None and len(gaps) == max_gaps:
            stop = s
            break
        q = resync(oracle, img, size, s + 1)
        q = size if q is None else q
        gaps.append((s, q))
        p = q
    starts = np.concatenate(recs) if recs else np.zeros(0, np.uint64)
    g = np.array(gaps, np.uint64).reshape(-1, 2)
    status = "ok" if not gaps and stop == size else "corrupted"
    return status, starts.astype(np.uint64), g, stop, mseq, int((g[:, 1] - g[:, 0]).sum())


def valid(oracle, b, size, p):
    """valid(p) on the image bytes b, Python integers."""
    if size - p < META:
        return False
    rl = int.from_bytes(b[p:p + 4], "little")
    if rl + 8 > size - p:
        return False
    kl, vl = int.from_bytes(b[p + 18:p + 22], "little"), int.from_bytes(b[p + 22:p + 26], "little")
    if 18 + kl + vl > rl:
        return False
    return oracle.crc(b[p + 8:p + 8 + rl]) == int.from_bytes(b[p + 4:p + 8], "little")


def brute_salvage(oracle, img, size):
    """The salvage program byte by byte: (starts list, gaps list of (a, b))."""
    b = img[:size].tobytes()
    p, starts, gaps = 0, [], []
    while p < size:
        if valid(oracle, b, size, p):
            starts.append(p)
            p += 8 + int.from_bytes(b[p:p + 4], "little")
        else:
            if gaps and gaps[-1][1] == p:
                gaps[-1][1] = p + 1
            else:
                gaps.append([p, p + 1])
            p += 1
    return starts, [tuple(g) for g in gaps]


# ---- hand-built records ------------------------------------------------------------------------------------

def record(oracle, key=b"", value=b"", seq=0, op=0, tomb=0, slack=0, stamp=True):
    """One record as wal_entry::encode lays it out (slack: bytes of record_len behind the value)."""
    body = bytes([op]) + int(seq).to_bytes(8, "little") + bytes([tomb]) + len(key).to_bytes(4, "little") + \
        len(value).to_bytes(4, "little") + key + value + b"\0" * slack
    crc = oracle.crc(body) if stamp else 0
    return len(body).to_bytes(4, "little") + crc.to_bytes(4, "little") + body


def header(rl, crc=0, kl=0, vl=0):
    """26 header bytes with the given fields (a decoy when its CRC is wrong)."""
    return (rl & 0xFFFFFFFF).to_bytes(4, "little") + (crc & 0xFFFFFFFF).to_bytes(4, "little") + b"\0" * 10 + \
        (kl & 0xFFFFFFFF).to_bytes(4, "little") + (vl & 0xFFFFFFFF).to_bytes(4, "little")


def noise(rng, n):
    """n random bytes none of which starts a structurally plausible record: every byte is at least 0x80,
    so each u32 is above 2^31 and no record_len + 8 fits an image below 2 GiB."""
    return rng.integers(0x80, 0x100, n, dtype=np.uint8).tobytes()
