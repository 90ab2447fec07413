#!/usr/bin/env python3
"""Generate tests/golden/memtable.json (TEST INFRASTRUCTURE): a few dozen WAL records in log order and
the memtable run tkv_memtable_build must make of them.

    python tests/golden/make_memtable.py

The case is accepted only when two independent constructions agree byte for byte: the dict replay of
tests/memtable_util.py (sorted(dict), Python's bytes order) and a list kept sorted record after record
with a comparator written out byte by byte (unsigned bytes, then the shorter key first), an equal key
replacing its node as skiplist::insert does. Only data is written: the records and the expected run, as
hex and numbers.
"""
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import memtable_util as mu  # noqa: E402

TS = 1_700_000_000_123


def compare(a, b):
    for x, y in zip(a, b):
        if x != y:
            return -1 if x < y else 1
    return (len(a) > len(b)) - (len(a) < len(b))


def by_insertion(recs, ts):
    nodes = []  # (key, record index), ascending
    for i, r in enumerate(recs):
        at = 0
        while at < len(nodes) and compare(nodes[at][0], r[2]) < 0:
            at += 1
        if at < len(nodes) and compare(nodes[at][0], r[2]) == 0:
            nodes[at] = (r[2], i)
        else:
            nodes.insert(at, (r[2], i))
    ikeys = b"".join(k + struct.pack("<QQB", recs[i][1], ts, 1 if recs[i][4] else 0) for k, i in nodes)
    return ikeys, [i for _, i in nodes], [0 if recs[i][0] == 1 else len(recs[i][3]) for _, i in nodes]


def main():
    keys = [b"", b"a", b"a\x00", b"a\x00\x00", b"a\x01", b"\x80", b"\x7f", b"\xff", b"12345678", b"123456789", b"1234567",
            b"12345678\x00", b"123456780", b"ABCDEFGHIJKLMNOP", b"ABCDEFGHIJKLMNOPQ", b"ABCDEFGHIJKLMNO", b"ABCDEFGHIJKLMNOQ",
            b"a", b"", b"12345678", b"\xff", b"ABCDEFGHIJKLMNOP", b"zz", b"a\x00", b"zz", b"zz"]
    recs = []
    for i, k in enumerate(keys):
        op = 1 if i % 5 == 3 else 0
        recs.append((op, (9001 - 37 * i) if i % 2 else i, k, b"value-%02d" % i if i % 7 else b"", (0, 1, 2, 0xFF)[i % 4] if op else i % 3 == 0))
    recs = [(op, seq, k, v, int(t)) for op, seq, k, v, t in recs]
    exp = mu.oracle(mu.columns(recs), TS)
    ikeys, src, vlen = by_insertion(recs, TS)
    if ikeys != exp.ikeys or src != exp.src.tolist() or vlen != exp.val_len.tolist():
        sys.exit("the dict replay and the insertion list disagree")
    doc = {"comment": "tests/golden/make_memtable.py: a WAL batch and the run tkv_memtable_build makes of it; hex",
           "timestamp_ms": TS,
           "records": [{"op": op, "seq": seq, "key": k.hex(), "value": v.hex(), "tomb": t} for op, seq, k, v, t in recs],
           "ikeys": exp.ikeys.hex(), "ikey_off": exp.ikey_off.tolist(), "src": src, "val_len": vlen}
    with open(os.path.join(HERE, "memtable.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {len(recs)} records, {len(src)} entries")


if __name__ == "__main__":
    main()
