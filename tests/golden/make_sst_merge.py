#!/usr/bin/env python3
"""Generate tests/golden/sst_merge.json (TEST INFRASTRUCTURE): a handful of small merges that can be checked
by hand, and what tkv_sst_merge must make of them.

    python tests/golden/make_sst_merge.py

Every case is written by the dict replay of tests/sst_merge_util.py and accepted only when a list kept
sorted entry after entry, with a comparator written out byte by byte and an equal user key replacing its
node, gives the same survivors. Only data is written: the runs (internal keys and values as hex, oldest run
first), the flag, and the expected src pairs [run, index]; one case has a run out of order and names the
first bad entry instead.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sst_merge_util as gu  # noqa: E402


def compare(a, b):
    for x, y in zip(a, b):
        if x != y:
            return -1 if x < y else 1
    return (len(a) > len(b)) - (len(a) < len(b))


def by_insertion(runs, drop):
    nodes = []  # (user key, (r, i)), ascending
    for r, run in enumerate(runs):
        for i, (k, _) in enumerate(run):
            user, at = k[:-gu.META], 0
            while at < len(nodes) and compare(nodes[at][0], user) < 0:
                at += 1
            if at < len(nodes) and compare(nodes[at][0], user) == 0:
                nodes[at] = (user, (r, i))
            else:
                nodes.insert(at, (user, (r, i)))
    return [list(s) for _, s in nodes if not (drop and runs[s[0]][s[1]][0][-1] != 0)]


def main():
    ik = gu.ikey
    cases = [
        ("two_runs_newest_wins", False,
         [[(ik(b"apple", 9, 50), b"old-apple"), (ik(b"cherry", 8, 50), b"old-cherry")],
          [(ik(b"apple", 1, 60), b"new-apple"), (ik(b"banana", 2, 60), b"banana")]]),
        ("lower_seq_in_newer_run_still_wins", False,
         [[(ik(b"k", 2**64 - 1, 2**64 - 1), b"older")], [(ik(b"k", 0, 0), b"newer")]]),
        ("prefix_order", False,
         [[(ik(b"a\x00"), b"2"), (ik(b"a\x01"), b"4"), (ik(b"\x80"), b"5")],
          [(ik(b""), b"0"), (ik(b"a"), b"1"), (ik(b"a\x00\x00"), b"3")]]),
        ("in_run_duplicates_highest_index", False,
         [[(ik(b"d", 1), b"d0"), (ik(b"d", 2), b"d1"), (ik(b"d", 3), b"d2"), (ik(b"e", 4), b"e0")],
          [(ik(b"c", 5), b"c0"), (ik(b"e", 6), b"e1"), (ik(b"e", 7), b"e2")]]),
        ("tombstones_kept", False,
         [[(ik(b"gone", 1), b"value"), (ik(b"kept", 2, 0, 1), b""), (ik(b"stay", 3), b"s")],
          [(ik(b"gone", 4, 0, 1), b""), (ik(b"kept", 5), b"back")], []]),
        ("tombstones_dropped", True,
         [[(ik(b"gone", 1), b"value"), (ik(b"kept", 2, 0, 1), b""), (ik(b"stay", 3), b"s"), (ik(b"two", 3, 0, 2), b"")],
          [(ik(b"gone", 4, 0, 1), b""), (ik(b"kept", 5), b"back")], []]),
        ("long_keys_three_runs", False,
         [[(ik(b"12345678"), b"a"), (ik(b"123456789"), b"b"), (ik(b"ABCDEFGHIJKLMNOPQ"), b"c")],
          [],
          [(ik(b"1234567"), b"d"), (ik(b"12345678\x00"), b"e"), (ik(b"ABCDEFGHIJKLMNOP"), b"f")],
          [(ik(b"123456789"), b"g"), (ik(b"ABCDEFGHIJKLMNOPQ"), b"h"), (ik(b"ABCDEFGHIJKLMNOQ"), b"i")]]),
    ]
    doc = {"comment": "tests/golden/make_sst_merge.py: runs (oldest first) and the survivors tkv_sst_merge leaves; hex",
           "cases": []}
    for name, drop, runs in cases:
        src = [list(s) for s in gu.oracle(gu.columns(runs), drop)]
        if src != by_insertion(runs, drop):
            sys.exit(f"{name}: the dict replay and the insertion list disagree")
        doc["cases"].append({"name": name, "drop_tombstones": drop,
                             "runs": [[{"ikey": k.hex(), "value": v.hex()} for k, v in run] for run in runs], "src": src})
    bad = [[(ik(b"a"), b""), (ik(b"b"), b"")], [(ik(b"m"), b""), (ik(b"z"), b""), (ik(b"y"), b""), (ik(b"zz"), b"")]]
    assert gu.first_bad(gu.columns(bad)) == (1 << 32 | 2)
    doc["bad_order"] = {"runs": [[{"ikey": k.hex(), "value": v.hex()} for k, v in run] for run in bad], "first_bad": [1, 2]}
    with open(os.path.join(HERE, "sst_merge.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {len(cases)} cases and one bad-order case")


if __name__ == "__main__":
    main()
