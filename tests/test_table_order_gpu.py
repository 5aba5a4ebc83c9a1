"""The engineered windows of tests/table_order_cases.py on the device, through engine.Engine and lancet_debug_pre_order: what the emulator
cannot show of kernel A's tail -- bl_min16 / bl_add16 on halves of LDS words, the LDS atomics of the stages, the lock-free union-find and
the stamped bucket minima under real interleaving.  Per configuration (the LDS build, LANCET_PRE_WIDE=1) two runs of one engine: each
equal to the oracle's dump of a real std::unordered_map graph by graph (hash sequence, comp per position, numcomp, refcomp, bucket
count, the table after compress(1) where the build kernel did it), and the two read-backs equal to each other; records, statistics and
the -v trace against the oracle.  One run each through the general build alone (LANCET_NO_PREBUILD=1) and with a tier 1 of 64 nodes
(LANCET_NODE_CAP1=64: the re-run tier), for records, statistics and trace."""
import numpy as np
import pytest

import table_order_cases as tc
from lancet_amd import abi, engine

pytestmark = pytest.mark.gpu

EVT = 1 << 16
FAMILIES = ["boundaries", "switches_large", "tiny", "all_survive", "components", "later_graphs"]


def _same(a, b):
    if len(a) != len(b):
        return False
    for ga, gb in zip(a, b):
        if ga.keys() != gb.keys():
            return False
        for k in ga:
            if not (np.array_equal(ga[k], gb[k]) if isinstance(ga[k], np.ndarray) else ga[k] == gb[k]):
                return False
    return True


def _run_family(family, wide, read_back, runs):
    n_order = n_done = 0
    for gi, (params, cases, batch) in enumerate(tc.groups(family)):
        tc.assert_oracle_side(family, gi)
        eng = engine.Engine(abi.default_params(**params), device=0, trace_words=EVT)
        seen = []
        for rep in range(runs):
            what = (family, gi, "wide" if wide else "default", "run", rep)
            v, st = eng.process(batch)
            tc.assert_results_equal_oracle(family, gi, (v, st, eng.trace_text()), what)
            if read_back:
                seen.append([eng.pre_order(w) for w in range(batch.n_windows)])
                a, b = tc.assert_orders_equal_oracle(family, gi, seen[-1], wide, what)
                n_order += a; n_done += b
        if read_back and runs > 1:
            differ = [cases[w].name for w in range(batch.n_windows) if not _same(seen[0][w], seen[1][w])]
            assert not differ, ("two runs of one engine left different hand-off areas", family, gi, differ)
        eng.close()
    return n_order, n_done


@pytest.mark.parametrize("wide", [False, True], ids=["lds", "wide"])
@pytest.mark.parametrize("family", FAMILIES)
def test_table_order_of_the_build_kernel(family, wide, monkeypatch):
    monkeypatch.delenv("LANCET_NODE_CAP1", raising=False)
    if wide:
        monkeypatch.setenv("LANCET_PRE_WIDE", "1")
    n_order, n_done = _run_family(family, wide, read_back=True, runs=2)
    assert n_order > 0, "no graph came with its table order: the comparison compared nothing"
    if family in ("all_survive", "components"):
        assert n_done > 0, "no graph came with its first compress done"


@pytest.mark.parametrize("env", [{"LANCET_NO_PREBUILD": "1"}, {"LANCET_NODE_CAP1": "64"}], ids=["general-build", "rerun-tier"])
@pytest.mark.parametrize("family", FAMILIES)
def test_table_order_through_the_other_routes(family, env, monkeypatch):
    """first_lowcov, clean_dead_wg, mark_connected_components_wg and order_insert of kernels.h order every graph (the window kernel, and the
    several-wave kernel of the re-run tier): their order is not read back, records, statistics and the trace of these windows -- the
    per-component lines of the many-component cases among them -- are its witnesses."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _run_family(family, False, read_back=False, runs=1)
