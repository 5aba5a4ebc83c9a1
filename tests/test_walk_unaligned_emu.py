"""The transcript walk's three routes without a GPU (kernels.h count_ref_path): a path that spells the reference takes none of the
alignment plumbing, a path the Hamming test lets through (1..5 mismatches) gets its columns straight from the mismatch positions, an
aligned path goes through walk_prepare as before.  Every case of tests/walk_cases.py runs through the emulated kernels twice -- the
routes above, and LANCET_OLD_WALK=1: the aligned strings, walk_prepare and the one-lane walk on every path -- and both must equal the
oracle: records, window statistics and every event of the -v trace, in order.

snv5_ends: the source and the sink are reference k-mers, so column k (right behind the source k-mer) and column L - 1 - k are the first and
the last a path can differ at; column 0 itself cannot, and the look-back for prev_bp (with the reference's assert when it runs off the
string) is the code both routes share."""
import os
import sys

import pytest

import golden_util as gu
import walk_cases as wc
from oracle import oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402

_KEY = lambda s: (s["status"], s["final_k"], s["n_builds"], s["n_variants"], s["n_kmers"], s["max_nodes"])


@pytest.mark.parametrize("case", wc.CASES)
def test_walk_routes_equal_the_one_lane_walk_and_the_oracle(case, monkeypatch):
    batch, p = wc.make(case)
    ov, ost, otr = oracle.run(batch, p, verbose=True)
    assert wc.paths_of(otr) == wc.PATHS[case] and len(ov) == wc.N_RECORDS[case]      # the case still reaches the route it is here for
    monkeypatch.delenv("LANCET_OLD_WALK", raising=False)
    new = emu.run(batch, p, evt_cap=1 << 16)
    monkeypatch.setenv("LANCET_OLD_WALK", "1")
    old = emu.run(batch, p, evt_cap=1 << 16)
    for v, st, tr in (new, old):
        assert v == ov
        assert [_KEY(s) for s in st] == [_KEY(s) for s in ost]
        assert tr == otr or gu.digest_trace(tr) == gu.digest_trace(otr)
    assert new[0] == old[0] and new[1] == old[1] and new[2] == old[2]                 # the two forms: event for event
    if case.endswith("_lr"):
        assert any(r["hp"] for r in ov) or any(any(len(x) for x in r["bx"]) for r in ov)


def test_the_cases_cover_the_three_routes():
    classes = set()
    for paths in wc.PATHS.values():
        for m, s, i, d in paths:
            classes.add("perfect" if s + i + d == 0 else ("unaligned" if i + d == 0 and s <= 5 else "aligned"))
    assert classes == {"perfect", "unaligned", "aligned"}
    assert wc.PATHS["het_ref_first"][0] == wc.PATHS["het_alt_first"][1] == (200, 0, 0, 0)
