"""The device traceback by runs (kernels.h align_traceback_runs under align_traceback_wg: wave ballot, one coalesced store of a run's
notes) behind both fills, on the table of tests/align_run_cases.py against oracle.align, through the one-wave hook and the 512-lane
build of the same source.  A case is one one-wave launch on strings of at most 300 bases."""
import os
import sys

import pytest

import align_cases as ac
import align_run_cases as rc
import golden_util as gu
from lancet_amd import abi, engine
from oracle import oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def align_engine():
    meta, batch, kept, (min_k, max_k) = gu.case_batch("cfg1_k25")
    eng = engine.Engine(abi.default_params(min_k=min_k, max_k=max_k), device=0)
    yield eng
    eng.close()


def _emu_thin():
    was = emu.FAT[0]
    emu.FAT[0] = False
    try:
        return emu.lib()
    finally:
        emu.FAT[0] = was


@pytest.mark.parametrize("fat", [False, True], ids=["wave", "fat"])
def test_device_traceback_by_runs_equals_oracle(align_engine, fat):
    """Modes 0 (band, full matrix as fall-back) and 1 (full matrix) answer every pair with the oracle's rows; the band alone (mode 2)
    decides as the emulator's band does for the same pair, answers the oracle's rows where it certifies, and certifies at least 90 % of
    the pairs with one indel and nothing else."""
    eng = align_engine
    L = _emu_thin()
    want = rc.expected()
    certified = single = 0
    differ = []
    for cid, s, t in rc.cases():
        assert eng.debug_align(s, t, mode=0, fat=fat) == want[cid], cid
        assert eng.debug_align(s, t, mode=1, fat=fat) == want[cid], cid
        band = eng.debug_align(s, t, mode=2, fat=fat)
        assert band is None or band == want[cid], cid
        emu_band = ac.emu_align(L, s, t, 2)
        if (band is None) != (emu_band is None):
            differ.append(cid)
        if rc.family(cid) in rc.SINGLE_INDEL:
            single += 1
            certified += band is not None
    print(f"device ({'fat' if fat else 'wave'}): band certified {certified} of {single} single-indel pairs")
    assert not differ, differ
    assert 10 * certified >= 9 * single, (certified, single)


def test_small_batch_is_assembled_after_the_alignment_hook(align_engine):
    eng = align_engine
    meta, batch, kept, (min_k, max_k) = gu.case_batch("cfg1_k25")
    variants, stats = eng.process(batch)
    ov, ostats, _ = oracle.run(batch, eng.params)
    assert variants == ov and len(variants) == 1
    assert [s["status"] for s in stats] == [s["status"] for s in ostats] and stats[0]["n_kmers"] == ostats[0]["n_kmers"]
