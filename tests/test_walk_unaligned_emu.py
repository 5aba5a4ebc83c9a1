"""The transcript walk's three routes without a GPU (kernels.h count_ref_path): a path that spells the reference takes none of the
alignment plumbing, a path the Hamming test lets through (1..5 mismatches) gets its columns straight from the mismatch positions, an
aligned path goes through walk_prepare as before.  Every case of tests/walk_cases.py runs through the emulated kernels twice -- the
routes above, and LANCET_OLD_WALK=1: the aligned strings, walk_prepare and the one-lane walk on every path -- and both must equal the
oracle: records, window statistics and every event of the -v trace, in order.

snv5_ends: the source and the sink are reference k-mers, so column k (right behind the source k-mer) and column L - 1 - k are the first and
the last a path can differ at; column 0 itself cannot, and the look-back for prev_bp (with the reference's assert when it runs off the
string) is the code both routes share.

The cases from many_ts on are there for the rules the two walk drivers share (kernels.h walk_column, walk_extend, walk_record): see
tests/walk_cases.py.  Every case also runs through the emulator build of the re-run tier's source."""
import functools
import os
import sys

import pytest

import golden_util as gu
import walk_cases as wc
from oracle import oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402

_KEY = lambda s: (s["status"], s["final_k"], s["n_builds"], s["n_variants"], s["n_kmers"], s["max_nodes"])


@functools.lru_cache(maxsize=None)
def _case(case):
    """(batch, params, the oracle's records, statistics and trace) of a case: made once, shared by the tests below and left unchanged."""
    batch, p = wc.make(case)
    return (batch, p) + tuple(oracle.run(batch, p, verbose=True))


def _routes_equal_the_one_lane_walk_and_the_oracle(case, monkeypatch):
    batch, p, ov, ost, otr = _case(case)
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


@pytest.mark.parametrize("case", wc.CASES)
def test_walk_routes_equal_the_one_lane_walk_and_the_oracle(case, monkeypatch):
    monkeypatch.setattr(emu, "FAT", [False])
    _routes_equal_the_one_lane_walk_and_the_oracle(case, monkeypatch)


@pytest.mark.parametrize("case", wc.CASES)
def test_walk_routes_on_the_rerun_tier(case, monkeypatch):
    """The same through the re-run tier's source (window_fat.hip compiles the same walk on 512 lanes; its staging area holds more transcripts)."""
    monkeypatch.setattr(emu, "FAT", [True])
    _routes_equal_the_one_lane_walk_and_the_oracle(case, monkeypatch)


def test_the_transcript_cases_straddle_the_lds_capacity(monkeypatch):
    """many_ts has one transcript more on its aligned path than the window kernel's LDS staging area holds (the wave driver stops and the
    one-lane driver redoes the path), ts_exact exactly as many: the last that still fits."""
    monkeypatch.setattr(emu, "FAT", [False])
    cap = emu.ts_lds_cap()
    assert wc.PATHS["many_ts"][0][1] == wc.N_RECORDS["many_ts"] == len(_case("many_ts")[2]) and wc.N_RECORDS["many_ts"] > cap
    assert wc.PATHS["ts_exact"][0][1] == wc.N_RECORDS["ts_exact"] == len(_case("ts_exact")[2]) == cap


def test_the_cases_cover_the_three_routes():
    classes = set()
    for paths in wc.PATHS.values():
        for m, s, i, d in paths:
            classes.add("perfect" if s + i + d == 0 else ("unaligned" if i + d == 0 and s <= 5 else "aligned"))
    assert classes == {"perfect", "unaligned", "aligned"}
    assert wc.PATHS["het_ref_first"][0] == wc.PATHS["het_alt_first"][1] == (200, 0, 0, 0)
