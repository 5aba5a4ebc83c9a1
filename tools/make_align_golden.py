#!/usr/bin/env python3
"""Writes the two alignment fixtures from the reference's own global_align_aff (oracle/_ref/libalign_ref.so, built by `make -C oracle`
where the reference sources are present).

tests/golden/align_ref.tsv: for every (S, T) pair of tests/test_oracle_golden.py align_cases(), one line S, T, aligned S, aligned T,
separated by tabs.

tests/golden/align_edge_ref.tsv: for every case of tests/align_cases.py, one line
    id <tab> len(S) <tab> len(T) <tab> first 12 hex digits of sha1(S + "\t" + T) <tab> alignment
where the alignment is a run-length string over M (both characters), D (a character of S against '-'), I ('-' against a character of
T), or the word `undefined` where the reference's traceback leaves its matrix (undefined behaviour in the reference: it may crash,
so the library is NOT called on such a pair; the oracle's bounds-checked walk decides which they are).  The strings themselves are
not stored: tests/align_cases.py draws them again and the hash catches a generator that drifted.  At most 2 % of the table may be
undefined, and none outside the family of unrelated strings: a family that breaks this has to change, not the cap.

Usage:  python tools/make_align_golden.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle  # noqa: E402
import align_cases as ac  # noqa: E402
import test_oracle_golden as t  # noqa: E402

UNDEFINED_CAP = 0.02


def edge_lines():
    lines, undefined = [], []
    for cid, s, tt in ac.cases():
        if oracle.align(s, tt) is None:
            undefined.append(cid)
            ops = ac.UNDEFINED
        else:
            a, b = oracle.ref_align(s, tt)
            ops = ac.encode_ops(a, b)
            assert ac.decode_ops(ops, s, tt) == (a, b), cid
        lines.append(f"{cid}\t{len(s)}\t{len(tt)}\t{ac.pair_hash(s, tt)}\t{ops}\n")
    outside = [c for c in undefined if ac.family(c) != "unrel"]
    if outside:
        sys.exit(f"undefined pairs outside the unrelated family: {outside}")
    if len(undefined) > UNDEFINED_CAP * len(lines):
        sys.exit(f"{len(undefined)} of {len(lines)} pairs are undefined in the reference: above {UNDEFINED_CAP:.0%}")
    return lines, undefined


def main():
    if not oracle.ref_align_available():
        sys.exit("oracle/_ref/libalign_ref.so is not built (make -C oracle with the reference sources present)")
    with open(t.ALIGN_GOLDEN, "w") as fh:
        for s, tt in t.align_cases():
            a, b = oracle.ref_align(s, tt)
            fh.write(f"{s}\t{tt}\t{a}\t{b}\n")
    print(t.ALIGN_GOLDEN)
    lines, undefined = edge_lines()
    with open(ac.FIXTURE, "w") as fh:
        fh.writelines(lines)
    print(ac.FIXTURE, f"{len(lines)} pairs, {len(undefined)} undefined ({100.0 * len(undefined) / len(lines):.1f} %)")


if __name__ == "__main__":
    main()
