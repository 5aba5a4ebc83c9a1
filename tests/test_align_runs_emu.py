"""The traceback by runs (kernels.h align_traceback_runs) in the emulated kernels, on the table of tests/align_run_cases.py against
oracle.align: both emulator builds, and both forms of the walk -- the run driver the device also compiles (the emulator's default) and
the one-cell walk of one lane (LANCET_OLD_TRACEBACK, the comparison form)."""
import os
import sys

import pytest

import align_cases as ac
import align_run_cases as rc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402


def _emu_build(fat):
    was = emu.FAT[0]
    emu.FAT[0] = fat
    try:
        return emu.lib()
    finally:
        emu.FAT[0] = was


@pytest.fixture(params=[False, True], ids=["runs", "cells"])
def old_traceback(request, monkeypatch):
    if request.param:
        monkeypatch.setenv("LANCET_OLD_TRACEBACK", "1")
    else:
        monkeypatch.delenv("LANCET_OLD_TRACEBACK", raising=False)
    return request.param


def test_the_table_holds_what_its_families_are_about():
    """Every run length and gap length of every kind, both orders of two adjacent gaps, every residue of n + m modulo 4."""
    ids = {c[0] for c in rc.cases()}
    for r in rc.RUNS:
        assert {f"diag1/{k}_run{r}" for k in "DI"} <= ids
        assert {f"diag2/{a}{b}_run{r if r > 1 else rc.diag2_shortest(a, b)}" for a in "DI" for b in "DI"} <= ids
    for g in rc.GAPS:
        assert {f"gaprun/{k}{g}" for k in "DI"} <= ids
    assert not rc.TURN_MISSING, rc.TURN_MISSING
    for order in ("DI", "ID"):
        for cid, s, t in rc.cases():
            if cid.startswith(f"turn/{order}_"):
                o = rc.ops(*rc.expected()[cid])
                assert any((o[x][0], o[x + 1][0]) == tuple(order) for x in range(len(o) - 1)), cid
    seams = [(len(s), len(t)) for cid, s, t in rc.cases() if rc.family(cid) == "seam"]
    assert {(n + m) % 4 for n, m in seams} == {0, 1, 2, 3} and len(seams) == 24
    assert all(len(s) <= rc.MAX_BASES and len(t) <= rc.MAX_BASES for _, s, t in rc.cases())


@pytest.mark.parametrize("fat", [False, True], ids=["thin", "fat"])
def test_emulated_traceback_by_runs_equals_oracle(fat, old_traceback):
    """Full matrix (mode 1) and band with fall-back (mode 0) must answer the oracle's rows for every pair; the band alone (mode 2)
    refuses or answers them, and certifies at least 90 % of the pairs with one indel and nothing else."""
    L = _emu_build(fat)
    want = rc.expected()
    certified = single = 0
    for cid, s, t in rc.cases():
        assert ac.emu_align(L, s, t, 1) == want[cid], cid
        assert ac.emu_align(L, s, t, 0) == want[cid], cid
        band = ac.emu_align(L, s, t, 2)
        assert band is None or band == want[cid], cid
        if rc.family(cid) in rc.SINGLE_INDEL:
            single += 1
            certified += band is not None
    print(f"emulator ({'fat' if fat else 'thin'}, {'cells' if old_traceback else 'runs'}): band certified {certified} of {single} single-indel pairs")
    assert 10 * certified >= 9 * single, (certified, single)
