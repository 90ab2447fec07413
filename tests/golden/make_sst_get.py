#!/usr/bin/env python3
"""Generate tests/golden/sst_get.json (TEST INFRASTRUCTURE): a handful of small lookups that can be checked by
hand, and what tkv_sst_get must answer.

    python tests/golden/make_sst_get.py

Every case is written by the dict replay of tests/sst_get_util.py and accepted only when a scan written out
entry by entry (runs newest first, in a run the last entry whose user key compares equal byte by byte) gives
the same answers. Only data is written: the runs (internal keys and values as hex, oldest run first), the
queries (hex), and per query state, src as [run, index] or null, seq and the value; and the gathered value
arena.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sst_get_util as tu  # noqa: E402
import sst_merge_util as gu  # noqa: E402


def equal(a, b):
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if x != y:
            return False
    return True


def by_scan(runs, queries):
    out = []
    for q in queries:
        ans = (tu.ABSENT, None, None, 0, b"")
        for r in reversed(range(len(runs))):
            at = [i for i, (k, _) in enumerate(runs[r]) if equal(k[:-gu.META], q)]
            if at:
                k, v = runs[r][at[-1]]
                seq = sum(k[len(k) - gu.META + b] << (8 * b) for b in range(8))
                ans = (tu.DELETED, r, at[-1], seq, b"") if k[-1] else (tu.FOUND, r, at[-1], seq, v)
                break
        out.append(ans)
    return out


def main():
    doc = {"comment": "tests/golden/make_sst_get.py: runs (oldest first), queries and what tkv_sst_get answers; hex",
           "cases": []}
    cases = tu.named_cases()
    for name in sorted(cases):
        runs, queries = cases[name]
        answers = tu.oracle(gu.columns(runs), queries)
        if answers != by_scan(runs, queries):
            sys.exit(f"{name}: the dict replay and the scan disagree")
        doc["cases"].append({
            "name": name,
            "runs": [[{"ikey": k.hex(), "value": v.hex()} for k, v in run] for run in runs],
            "queries": [q.hex() for q in queries],
            "answers": [{"state": s, "src": None if r is None else [r, i], "seq": seq, "value": v.hex()}
                        for s, r, i, seq, v in answers],
            "vals": b"".join(a[4] for a in answers).hex()})
    with open(os.path.join(HERE, "sst_get.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {len(cases)} cases")


if __name__ == "__main__":
    main()
