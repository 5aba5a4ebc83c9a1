#!/usr/bin/env python3
"""Writes tests/golden/align_ref.tsv: for every (S, T) pair of tests/test_oracle_golden.py align_cases(), the two aligned rows
that the reference's own global_align_aff returns (oracle/_ref/libalign_ref.so, built by `make -C oracle` where the reference
sources are present).  One line per pair: S, T, aligned S, aligned T, separated by tabs.

Usage:  python tools/make_align_golden.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle  # noqa: E402
import test_oracle_golden as t  # noqa: E402


def main():
    if not oracle.ref_align_available():
        sys.exit("oracle/_ref/libalign_ref.so is not built (make -C oracle with the reference sources present)")
    with open(t.ALIGN_GOLDEN, "w") as fh:
        for s, tt in t.align_cases():
            a, b = oracle.ref_align(s, tt)
            fh.write(f"{s}\t{tt}\t{a}\t{b}\n")
    print(t.ALIGN_GOLDEN)


if __name__ == "__main__":
    main()
