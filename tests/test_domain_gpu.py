"""The edges of the accepted domain (tests/domain_cases.py) on the device, through engine.Engine: what the emulator cannot show -- a
race between lanes, an LDS area sized for k <= 101, a miscompile at a shape no other test reaches.  Records, per-window statistics
and -- where asked for -- the digest of the -v trace equal the oracle's, bit for bit."""
import os
import time

import pytest

import domain_cases as dc
import golden_util as gu
from lancet_amd import abi, engine

pytestmark = pytest.mark.gpu

# (tools/fat_check.sh runs the suite with a 64-entry tier-1 node table: what tier 1 itself served is not counted then)
TIER1 = "LANCET_NODE_CAP1" not in os.environ


def _high_k(pair):
    p = abi.default_params(min_k=pair[0], max_k=pair[1])
    eng = engine.Engine(p, device=0, trace_words=1 << 17)
    out = []
    for which in ("plain", "str"):
        ov, ost, otr = dc.high_k_oracle(which, *pair)
        v, st = eng.process(dc.high_k_batch(which))
        dc.assert_equal_to_oracle((v, st), (ov, ost), what=(which, pair))
        assert gu.digest_trace(eng.trace_text()) == gu.digest_trace(otr), (which, pair)
        out.append((eng.prebuilt_count(), eng.rerun_count(), [h for h in eng.pre_headers() if h["built"]]))
    eng.close()
    return out


@pytest.mark.parametrize("pair", dc.HIGH_K, ids=lambda p: f"k{p[0]}-{p[1]}")
def test_k_above_101_with_the_default_hand_off(pair):
    """k = 97..127 through the general build (the narrow hand-off areas hold one-word keys): four-word keys whose top word holds up to
    62 bits, on 150-base reads and on 250-base reads over STR-rich sequence (final k 121 and 127)."""
    for built, _, hd in _high_k(pair):
        if pair[0] > 101:
            assert all(h["K"] > 101 for h in hd), hd


@pytest.mark.parametrize("pair", dc.HIGH_K, ids=lambda p: f"k{p[0]}-{p[1]}")
def test_k_above_101_built_in_lds(pair, monkeypatch):
    """LANCET_PRE_WIDE=1: the 1024-lane configuration of the LDS build kernel (BL_KMAX 127, keys of four words) builds all 12 windows of
    an odd-k draw, none of k = 126."""
    monkeypatch.setenv("LANCET_PRE_WIDE", "1")
    for built, _, hd in _high_k(pair):
        if TIER1:
            assert built == (0 if pair[0] % 2 == 0 else 12), (pair, built)
        if pair[0] > 101:
            assert all(h["K"] > 101 for h in hd), hd
            assert not TIER1 or pair[0] % 2 == 0 or len(hd) == 12


def test_k_above_101_through_the_rerun_tier(monkeypatch):
    """A tier 1 of 64 nodes: the several-wave kernel of the re-run tier assembles the windows at k = 103..127."""
    monkeypatch.setenv("LANCET_NODE_CAP1", "64")
    for _, reruns, _ in _high_k(dc.HIGH_K_RERUN):
        assert reruns > 0


@pytest.mark.parametrize("si", range(len(dc.TINY_SETS)), ids=lambda i: "k{}-{}{}".format(dc.TINY_SETS[i][0], dc.TINY_SETS[i][1], "-loose" if dc.TINY_SETS[i][2] else ""))
def test_k_below_10_and_references_shorter_than_reads_and_k(si):
    """The batches of one parameter set through one engine: references of 1..150 bases, reads as long as the reference or shorter,
    min_k 3..9."""
    if si == 0:
        dc.tiny_preconditions()
    eng = engine.Engine(dc.tiny_params(si), device=0)
    for i in range(si, dc.TINY_BATCHES, len(dc.TINY_SETS)):
        got = eng.process(dc.tiny_batch(i))
        dc.assert_equal_to_oracle(got, dc.tiny_oracle(i), what=("tiny batch", i))
    eng.close()


@pytest.mark.parametrize("k", dc.LONG_K)
def test_reads_at_the_length_limit(k):
    """Reads of 1023, 1024 and 1023 + k bases equal the oracle; with 1024 + k bases that window alone fails (status < 0) and the
    ordinary windows beside it equal the oracle."""
    p = abi.default_params(min_k=k, max_k=k)
    W = dc.LONG_ORDINARY
    eng = engine.Engine(p, device=0)
    for L in dc.long_read_lengths(k):
        want = dc.long_read_oracle(L, k)
        got = eng.process(dc.long_read_batch(L))
        if k == 25 and TIER1:                # (the ordinary windows come out of the LDS build, the long-read one never)
            assert [h["built"] for h in eng.pre_headers()] == [True] * W + [False], (L, eng.pre_headers())
        if L <= 1023 + k:
            dc.assert_equal_to_oracle(got, want, what=(k, L))
        else:
            assert got[1][W]["status"] < 0, (k, L, got[1][W])
            dc.assert_equal_to_oracle(got, want, windows=range(W), what=(k, L))
    eng.close()


def test_the_lds_build_turns_reads_of_1024_bases_away(monkeypatch):
    """Wide hand-off areas, k = 25: the window of 1023-base reads is built in LDS like the ordinary ones beside it, the one of 1024-base
    reads by the general build."""
    monkeypatch.setenv("LANCET_PRE_WIDE", "1")
    p = abi.default_params(min_k=25, max_k=25)
    eng = engine.Engine(p, device=0)
    for L, built in ((1023, dc.LONG_ORDINARY + 1), (1024, dc.LONG_ORDINARY)):
        want = dc.long_read_oracle(L, 25)
        assert all(s["n_builds"] == 1 for s in want[1])
        got = eng.process(dc.long_read_batch(L))
        dc.assert_equal_to_oracle(got, want, what=L)
        if TIER1:
            assert eng.prebuilt_count() == built, (L, eng.prebuilt_count())
            assert [h["built"] for h in eng.pre_headers()] == [True] * dc.LONG_ORDINARY + [L == 1023]
    eng.close()


@pytest.mark.parametrize("kind,n", [("insert170", 100), ("insert170", 250), ("insert170", 500), ("short30", 32768), ("short30", 49152)])
def test_deep_windows_of_overlapping_pairs(kind, n):
    """Short-insert libraries at depth: 8 windows of 150-base reads from 170-base fragments at 100x, 250x and 500x
    per sample, one 120-base window of 32 768 and of 49 152 30-base reads paired two by two.  At 500x and with 49 152 reads the
    mate-overlap prefilter flags more occurrences than the k-mer table of the re-run tier has slots; its list holds them all."""
    batch, ov, ost = dc.deep_oracle(kind, n)
    eng = engine.Engine(abi.default_params(), device=0)
    t0 = time.perf_counter()
    v, st = eng.process(batch)
    print(f"deep pairs {kind} {n}: {time.perf_counter() - t0:.2f} s on the device, {eng.rerun_count()} windows re-run")
    assert all(s["status"] >= 0 for s in st), [s["status"] for s in st]
    dc.assert_equal_to_oracle((v, st), (ov, ost), what=(kind, n))
    if (kind, n) == ("insert170", 500):
        assert eng.rerun_count() > 0
    eng.close()
