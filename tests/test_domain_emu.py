"""The edges of the accepted domain (tests/domain_cases.py) on both host builds of the kernels: the one-wave source and the re-run
tier's (LANCET_FAT), each laid out as the engine lays its re-run tier out.  Records, per-window statistics and -- where asked for --
the digest of the -v trace equal the oracle's, bit for bit.  The same cases run on the device in test_domain_gpu.py."""
import os
import sys

import pytest

import domain_cases as dc
import golden_util as gu
from lancet_amd import abi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402


@pytest.fixture
def both_builds():
    """Yields the setter of emu.FAT; the thin build is selected again afterwards."""
    def use(fat):
        emu.FAT[0] = fat
    yield use
    emu.FAT[0] = False


@pytest.mark.parametrize("wide", [False, True], ids=["default", "wide"])
@pytest.mark.parametrize("pair", dc.HIGH_K, ids=lambda p: f"k{p[0]}-{p[1]}")
def test_k_above_101(pair, wide, both_builds, monkeypatch):
    """k = 97..127: the fourth key word holds up to 62 bits (left-align, fingerprint, reverse-complement and LC_TAKE shifts next to a
    full word).  Default hand-off areas: the general build takes every k above 101; wide ones (LANCET_PRE_WIDE=1): the 1024-lane
    configuration of the LDS build kernel builds all 12 windows of an odd-k draw and none of the even k = 126."""
    if wide:
        monkeypatch.setenv("LANCET_PRE_WIDE", "1")
    p = abi.default_params(min_k=pair[0], max_k=pair[1])
    for which in ("plain", "str"):
        ov, ost, otr = dc.high_k_oracle(which, *pair)
        for fat in (False, True):
            both_builds(fat)
            v, st, tr = emu.run(dc.high_k_batch(which), p, evt_cap=1 << 17)
            dc.assert_equal_to_oracle((v, st), (ov, ost), what=(which, pair, wide, fat))
            assert gu.digest_trace(tr) == gu.digest_trace(otr), (which, pair, wide, fat)
            if wide:
                assert emu.LAST_PREBUILT[0] == (0 if pair[0] % 2 == 0 else 12), (which, pair, emu.LAST_PREBUILT)
            elif pair[0] >= 97:
                assert emu.LAST_PREBUILT[0] == 0, (which, pair, emu.LAST_PREBUILT)


@pytest.mark.parametrize("fat", [False, True], ids=["wave", "fat"])
def test_k_below_10_and_references_shorter_than_reads_and_k(fat, both_builds):
    """60 batches of 8 hand-made windows: references of 1..150 bases, reads as long as the reference, one base shorter or half of it,
    min_k 3..9 (a window reference shorter than min_k among them), one planted substitution / insertion / deletion each."""
    dc.tiny_preconditions()
    both_builds(fat)
    for i in range(dc.TINY_BATCHES):
        v, st, _ = emu.run(dc.tiny_batch(i), dc.tiny_params(i % len(dc.TINY_SETS)))
        dc.assert_equal_to_oracle((v, st), dc.tiny_oracle(i), what=("tiny batch", i))


@pytest.mark.parametrize("k", dc.LONG_K)
def test_reads_at_the_length_limit(k, both_builds):
    """Reads of 1023, 1024 and 1023 + k bases equal the oracle (k-mer positions 0..1023: ten bits); with 1024 + k bases that window
    alone is reported as an overflow and the ordinary windows beside it equal the oracle."""
    p = abi.default_params(min_k=k, max_k=k)
    W = dc.LONG_ORDINARY
    for L in dc.long_read_lengths(k):
        want = dc.long_read_oracle(L, k)
        for fat in (False, True):
            both_builds(fat)
            v, st, _ = emu.run(dc.long_read_batch(L), p)
            if k == 25:                      # (the ordinary windows come out of the LDS build, the long-read one never: BLW_QV, then BLW_SIZE from 1024 bases on)
                assert emu.LAST_PREBUILT[0] == W, (L, fat, emu.LAST_PREBUILT)
            if L <= 1023 + k:
                dc.assert_equal_to_oracle((v, st), want, what=(k, L, fat))
            else:
                assert st[W]["status"] < 0, (k, L, fat, st[W])
                dc.assert_equal_to_oracle((v, st), want, windows=range(W), what=(k, L, fat))


def test_the_lds_build_turns_reads_of_1024_bases_away(both_builds, monkeypatch):
    """Wide hand-off areas, k = 25: the window of 1023-base reads is built in LDS like the ordinary ones beside it, the one of 1024-base
    reads (a k-mer position would need an eleventh bit there) by the general build."""
    monkeypatch.setenv("LANCET_PRE_WIDE", "1")
    p = abi.default_params(min_k=25, max_k=25)
    for L, built in ((1023, dc.LONG_ORDINARY + 1), (1024, dc.LONG_ORDINARY)):
        want = dc.long_read_oracle(L, 25)
        assert all(s["n_builds"] == 1 for s in want[1])
        for fat in (False, True):
            both_builds(fat)
            v, st, _ = emu.run(dc.long_read_batch(L), p)
            dc.assert_equal_to_oracle((v, st), want, what=(L, fat))
            assert emu.LAST_PREBUILT[0] == built, (L, fat, emu.LAST_PREBUILT)


@pytest.mark.parametrize("kind,n", [("insert170", 100), ("insert170", 250), ("insert170", 500), ("short30", 32768), ("short30", 49152)])
def test_deep_windows_of_overlapping_pairs(kind, n, both_builds):
    """Short-insert libraries at depth: every pair's mates overlap, so the mate-overlap prefilter flags a k-mer occurrence per shared
    k-mer start.  The list of flagged occurrences holds one entry per occurrence of the window in the re-run tier's work space (it had
    as many entries as the k-mer table has slots, 131 072: the 500x windows and the 49 152-read window were reported as overflows)."""
    batch, ov, ost = dc.deep_oracle(kind, n)
    p = abi.default_params()
    for fat in (False, True):
        both_builds(fat)
        v, st, _ = emu.run(batch, p)
        assert all(s["status"] >= 0 for s in st), (fat, [s["status"] for s in st])
        dc.assert_equal_to_oracle((v, st), (ov, ost), what=(kind, n, fat))
