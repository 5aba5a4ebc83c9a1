"""The cleaning passes inside whole windows, on the host emulation of the kernels: the hand-made windows of clean_window_cases.py -- a tip at
max_tip_len - 1 | max_tip_len, the Y in both table orders, three tip rounds that remove, the ratio term of removeLowCov on an exact product and
one base below it, a unitig that is (1, 1) only through compressNode's average (and the same reads where the float sum is a step off) -- each
first held to what the oracle's -v trace must show for it, then both host builds of the kernels (the one-wave source and the re-run tier's)
against the oracle in records, every statistic and the trace digest, through the LDS build and with LANCET_NO_PREBUILD=1 (the general build).
The device's side is test_clean_passes_gpu.py; the rules at every threshold are test_clean_passes_emu.py's."""
import os
import sys

import pytest

import clean_window_cases as cw
import nref_cases as nc
from lancet_amd import abi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402

EVT = 1 << 16


@pytest.fixture(params=["wave", "fat"])
def source(request):
    emu.FAT[0] = request.param == "fat"
    yield request.param
    emu.FAT[0] = False


def test_the_oracle_trace_shows_what_the_windows_are_for():
    facts = []
    assert len(cw.groups()) == cw.N_GROUPS
    for gi, (_, cs, _) in enumerate(cw.groups()):
        facts += list(zip(cs, cw.assert_preconditions(gi)))
    cw.assert_group_wide(facts)


@pytest.mark.parametrize("env", [{}, {"LANCET_NO_PREBUILD": "1"}], ids=["lds-build", "general-build"])
@pytest.mark.parametrize("gi", range(cw.N_GROUPS))
def test_windows_equal_the_oracle(gi, env, source, monkeypatch):
    cw.assert_preconditions(gi)                                 # the oracle's trace first
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    params, cs, batch = cw.groups()[gi]
    got = emu.run(batch, abi.default_params(**params), evt_cap=EVT)
    nc.assert_equal_to_oracle(got, cw.oracle_of(gi), what=(source, env, [c.name for c in cs]))
    if not env:
        assert emu.LAST_PREBUILT[0] == (len(cs) if params["min_k"] % 2 else 0)      # (every window's graph came from the LDS build kernel; an even k is the general build's)
    else:
        assert emu.LAST_PREBUILT[0] == 0


def test_noisy_batch_equals_the_oracle(source):
    cw.assert_noisy_preconditions()                             # more than 64 and more than 512 live nodes when the passes run
    batch, want = cw.noisy_batch()
    nc.assert_equal_to_oracle(emu.run(batch, abi.default_params(), evt_cap=1 << 18), want, what=source)
