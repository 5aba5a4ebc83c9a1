"""The cleaning passes inside whole windows on the device: the hand-made windows of clean_window_cases.py (see there and
test_clean_passes_windows_emu.py), one batch per parameter set, under the default route, without the LDS build and in the re-run tier (the
512-lane source).  What the emulator cannot show: the device library's double division, sqrt and floor and its float sums at the (1, 1) term,
and the lanes of pass_candidates_wg / clean_dead_flags_wg side by side.  Every batch runs twice on its engine with equal read-backs; the
oracle's trace is held to each window's precondition before a device value is looked at."""
import pytest

import clean_window_cases as cw
import nref_cases as nc
from lancet_amd import abi, engine

pytestmark = pytest.mark.gpu

EVT = 1 << 16


@pytest.mark.parametrize("env", [{}, {"LANCET_NO_PREBUILD": "1"}, {"LANCET_NODE_CAP1": "64"}], ids=["lds-build", "general-build", "rerun-tier"])
@pytest.mark.parametrize("gi", range(cw.N_GROUPS))
def test_windows_equal_the_oracle(gi, env, monkeypatch):
    cw.assert_preconditions(gi)                                 # the oracle's trace first
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    params, cs, batch = cw.groups()[gi]
    eng = engine.Engine(abi.default_params(**params), device=0, trace_words=EVT)
    try:
        first = None
        for _ in range(2):
            v, st = eng.process(batch)
            got = (v, st, eng.trace_text())
            nc.assert_equal_to_oracle(got, cw.oracle_of(gi), what=(env, [c.name for c in cs]))
            assert first is None or got == first
            first = got
        if "LANCET_NODE_CAP1" in env:
            assert eng.rerun_count() > 0                        # (220 k-mers and more: no window fits 64 nodes)
    finally:
        eng.close()


@pytest.mark.parametrize("env", [{}, {"LANCET_NO_PREBUILD": "1"}, {"LANCET_NODE_CAP1": "64"}], ids=["lds-build", "general-build", "rerun-tier"])
def test_noisy_batch_equals_the_oracle(env, monkeypatch):
    cw.assert_noisy_preconditions()                             # more than 64 and more than 512 live nodes when the passes run
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    batch, want = cw.noisy_batch()
    eng = engine.Engine(abi.default_params(), device=0, trace_words=1 << 18)
    try:
        first = None
        for _ in range(2):
            v, st = eng.process(batch)
            got = (v, st, eng.trace_text())
            nc.assert_equal_to_oracle(got, want, what=env)
            assert first is None or got == first
            first = got
        if "LANCET_NODE_CAP1" in env:
            assert eng.rerun_count() > 0
    finally:
        eng.close()
