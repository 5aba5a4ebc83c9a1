"""Hand-made --linked-reads windows aimed at the two routes of the barcode / haplotype replay (tests/lr_replay_cases.py) on the device,
through engine.Engine: what the emulator (tests/test_lr_replay_emu.py, tests/test_lr_replay_windows_emu.py: lanes one after the other)
cannot show in lr_replay_batches -- the run-order flag set by the lanes' dev_atomic_or, the winners of win[] settled by dev_atomic_max,
raw[] used again as win[] across a barrier, a barrier missing between its passes, a miscompile of either route.

Records (hp[12], the barcode sets), per-window statistics and the digest of the -v trace equal the oracle's under three settings: the
default (the replay under load_prebuilt_lr), without the LDS build (under build_gather), and with a 64-entry tier-1 node table (the
re-run tier: 64-bit csr words).  Every family runs twice on its engine and must give the same output both times.  At most 6 windows of
at most 500 reads per family.

The second run of a deep family (2 or 3 windows, all built by the 1024-lane configuration of the LDS build kernel) is also the regression
test of that kernel's grid: it was sized max(8, windows the last batch listed) while its scratch has min(windows, CUs) slots, one per
workgroup index, so the second batch of fewer than 8 such windows on one engine wrote past the scratch buffer (an illegal memory access)."""
import os

import pytest

import golden_util as gu
import lr_replay_cases as lc
import nref_cases as nc
from lancet_amd import engine

pytestmark = pytest.mark.gpu

# (tools/fat_check.sh runs the suite with a 64-entry tier-1 node table: what tier 1 itself served is not counted then)
TIER1 = "LANCET_NODE_CAP1" not in os.environ
EVT = 1 << 18
SETTINGS = {"lds-build": {}, "general-build": {"LANCET_NO_PREBUILD": "1"}, "rerun-tier": {"LANCET_NODE_CAP1": "64"}}


@pytest.fixture(scope="module", params=list(SETTINGS))
def eng(request):
    """One engine per setting (the engine reads its settings when it is made), shared by the families."""
    env = SETTINGS[request.param]
    before = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        e = engine.Engine(lc.params(), device=0, trace_words=EVT)
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    yield request.param, e
    e.close()


@pytest.mark.parametrize("name", lc.FAMILIES)
def test_family_equals_the_oracle_twice(name, eng):
    setting, e = eng
    lc.preconditions(name)
    batch, _, want = lc.family(name)
    runs = []
    for i in range(2):
        v, st = e.process(batch)
        tr = e.trace_text()
        nc.assert_equal_to_oracle((v, st, tr), want, what=(name, setting, i))
        if setting == "rerun-tier":
            assert e.rerun_count() == batch.n_windows, (name, i, e.rerun_count())
        elif TIER1:                                                # (the LDS build takes every window of every family, as on the emulator)
            assert e.prebuilt_count() == (0 if setting == "general-build" else batch.n_windows), (name, setting, i, e.prebuilt_count())
        runs.append((v, [nc.KEY(s) for s in st], gu.digest_trace(tr)))
    assert runs[0] == runs[1], (name, setting)
