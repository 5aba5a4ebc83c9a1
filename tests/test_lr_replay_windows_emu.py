"""Hand-made --linked-reads windows aimed at the two routes of the barcode / haplotype replay (tests/lr_replay_cases.py), on the host
builds of the kernels: records (hp[12], the barcode sets), per-window statistics and the digest of the -v trace equal the oracle's, on
both sources (the window kernel's and the re-run tier's, 64-bit csr words), with the LDS build (the replay under load_prebuilt_lr) and
without it (under build_gather), and once with the wide hand-off areas.

Every family is taken whole by the LDS build kernel (emu.LAST_PREBUILT) -- the deep ones, 460..500 reads of 100 bases, by its 1024-lane
configuration (emu.LAST_BIGLIST), which holds their ~45 000 occurrences; none is turned away, so both call sites of the replay see every
family.  The same cases run on the device in test_lr_replay_gpu.py."""
import os
import sys

import pytest

import lr_replay_cases as lc
import nref_cases as nc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402

EVT = 1 << 18
DEEP = [f for f in lc.FAMILIES if f.startswith("lane_")]


@pytest.fixture
def build_of():
    """Yields the setter of emu.FAT; the thin build is selected again afterwards."""
    def use(fat):
        emu.FAT[0] = fat
    yield use
    emu.FAT[0] = False


@pytest.mark.parametrize("name", lc.FAMILIES)
def test_family_is_a_test_of_its_route(name):
    lc.preconditions(name)


@pytest.mark.parametrize("prebuild", [True, False], ids=["lds-build", "general-build"])
@pytest.mark.parametrize("fat", [False, True], ids=["window-kernel", "rerun-source"])
@pytest.mark.parametrize("name", lc.FAMILIES)
def test_family_equals_the_oracle(name, fat, prebuild, build_of, monkeypatch):
    if not prebuild:
        monkeypatch.setenv("LANCET_NO_PREBUILD", "1")
    batch, _, want = lc.family(name)
    build_of(fat)
    got = emu.run(batch, lc.params(), evt_cap=EVT)
    built, big = emu.LAST_PREBUILT[0], emu.LAST_BIGLIST[0]
    nc.assert_equal_to_oracle(got, want, what=(name, fat, prebuild))
    assert built == (batch.n_windows if prebuild else 0), (name, built)
    if prebuild:
        assert big == (batch.n_windows if name in DEEP else 0), (name, big)


@pytest.mark.parametrize("name", ["coop_over_127", "lane_ref_distinct", "lane_alt"])
def test_family_with_wide_hand_off_areas(name, monkeypatch):
    monkeypatch.setenv("LANCET_PRE_WIDE", "1")
    batch, _, want = lc.family(name)
    got = emu.run(batch, lc.params(), evt_cap=EVT)
    nc.assert_equal_to_oracle(got, want, what=(name, "wide"))
    assert emu.LAST_PREBUILT[0] == batch.n_windows
