"""Kernel A's tail and the whole route on the engineered windows of tests/table_order_cases.py, on both host builds of the kernels: the
table order, the components and the hashtable state that the LDS build kernel leaves in the hand-off areas (read back through the twin of
lancet_debug_pre_order) against the oracle's dump of a real std::unordered_map, graph by graph; beside that records, statistics and the
-v trace of the same batch against the oracle -- on the LDS build, with wide hand-off areas (LANCET_PRE_WIDE=1), through the general build
alone (LANCET_NO_PREBUILD=1: first_lowcov, clean_dead_wg, mark_connected_components_wg of kernels.h order every graph; their order is
not read back, the trace of the many-component cases is its witness and test_table_order_emu.py holds the order itself) and on the
re-run tier's source.  The same cases run on the device in test_table_order_gpu.py."""
import os
import sys

import pytest

import table_order_cases as tc
from lancet_amd import abi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402

EVT = 1 << 16


@pytest.fixture
def build_of():
    def use(fat):
        emu.FAT[0] = fat
    yield use
    emu.FAT[0] = False


def _run(family, gi, what, wide, read_back=True):
    params, cases, batch = tc.groups(family)[gi]
    got = emu.run(batch, abi.default_params(**params), evt_cap=EVT, pre_order=read_back)
    tc.assert_results_equal_oracle(family, gi, got, what)
    if not read_back:
        return 0, 0
    return tc.assert_orders_equal_oracle(family, gi, list(emu.LAST_PRE_ORDER), wide, what)


ROUTES = ["lds", "wide", "general", "fat"]


def _route(route, monkeypatch, build_of):
    if route == "wide":
        monkeypatch.setenv("LANCET_PRE_WIDE", "1")
    if route == "general":
        monkeypatch.setenv("LANCET_NO_PREBUILD", "1")
    build_of(route == "fat")


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("family", ["boundaries", "switches_large", "tiny", "all_survive", "components"])
def test_engineered_windows(family, route, monkeypatch, build_of):
    n_order = n_done = 0
    for gi in range(len(tc.groups(family))):
        tc.assert_oracle_side(family, gi)
        _route(route, monkeypatch, build_of)
        a, b = _run(family, gi, (family, gi, route), wide=route == "wide", read_back=route != "general")
        n_order += a; n_done += b
    if route != "general":
        assert n_order > 0, "no graph came with its table order: the comparison compared nothing"
    if route != "general" and family in ("all_survive", "components"):
        assert n_done > 0, "no graph came with its first compress done"


def test_which_form_orders_which_table(monkeypatch, build_of):
    """512-lane form: 4096 nodes come with their order, 4097 .. 5632 are built without it (the window kernel orders a prebuilt graph).
    1024-lane form: 4097 nodes come with their order whatever the hand-off (wide_tab); 5633 .. 14336 with wide hand-off areas only, 14337
    never."""
    for wide in (False, True):
        if wide:
            monkeypatch.setenv("LANCET_PRE_WIDE", "1")
        seen = {}
        for family in ("boundaries", "switches_large"):
            params, cases, batch = tc.groups(family)[0]
            emu.run(batch, abi.default_params(**params), pre_order=True)
            seen.update({c.name: emu.LAST_PRE_ORDER[w][0] for w, c in enumerate(cases)})
        flags = lambda name: (seen[name]["built"], bool(seen[name]["have_order"]), bool(seen[name]["big"]))
        assert flags("N4096") == (True, True, False), (wide, seen["N4096"])
        for name in ("N4097", "N%d" % tc.NARROW_CAP):
            assert flags(name) == (True, False, False), (wide, name, seen[name])
        assert flags("large_N4096") == (True, True, True) and flags("large_N4097") == (True, True, True), (wide, seen["large_N4097"])
        for name in ("N%d" % (tc.NARROW_CAP + 1), "N10273"):
            assert flags(name) == ((True, True, True) if wide else (False, False, False)), (wide, name, seen[name])
        top = [flags("N%d" % n) for n in (tc.WIDE_CAP - 1, tc.WIDE_CAP)]          # (87 % of the slots taken: either may be turned away for its probes)
        assert all(f in ((True, True, True), (False, False, False)) for f in top) and (wide or not any(f[0] for f in top)), (wide, top)
        assert not seen["N%d" % (tc.WIDE_CAP + 1)]["built"]


@pytest.mark.parametrize("route", ["lds", "service", "general", "fat"])
def test_the_same_table_as_a_later_graph(route, monkeypatch, build_of):
    """(f) the boundary at the second k: as a graph built ahead (the heavy windows of the 1024-lane configuration), as one the build
    service builds (the others; with LANCET_AHEAD_DEPTH=0 all of them), through the general build; and a window whose k climbs through
    twelve graphs"""
    if route == "service":
        monkeypatch.setenv("LANCET_AHEAD_DEPTH", "0")
    if route == "general":
        monkeypatch.setenv("LANCET_NO_PREBUILD", "1")
    build_of(route == "fat")
    for gi in range(len(tc.groups("later_graphs"))):
        tc.assert_oracle_side("later_graphs", gi)
        _run("later_graphs", gi, ("later_graphs", gi, route), wide=False, read_back=route != "general")
        if route == "general":
            continue
        cases = tc.groups("later_graphs")[gi][1]
        if any(c.name.startswith("ahead_") for c in cases):
            assert emu.LAST_SVC[1] > 0, emu.LAST_SVC
            assert (emu.LAST_AHEAD[0] == 0) if route == "service" else (emu.LAST_AHEAD[0] > 0 and emu.LAST_AHEAD[1] > 0), emu.LAST_AHEAD
        for w, c in enumerate(cases):
            ks = [g["K"] for g in emu.LAST_PRE_ORDER[w] if g["built"] and g["have_order"]]
            # (many_k: twelve graphs at k = 19 .. 41; the narrow hand-off areas hold one-word keys, k <= 31 -- the rest is the general build's)
            assert ks == ([c.second, c.k] if c.name != "many_k" else list(range(19, 33, 2))), (c.name, ks)


@pytest.mark.parametrize("fat", [False, True], ids=["wave", "fat"])
def test_tiny_windows_in_a_work_space_of_64_nodes(fat, monkeypatch, build_of):
    """The tiny windows in a tier 1 laid out for 64 nodes (128 table slots), as LANCET_NODE_CAP1=64 lays the engine's out: they fit, so
    they are assembled there -- the even k by the general build, whose first table size was 1024 slots whatever the work space held (it
    cleared and filled slots past the end of the array; on the device an illegal memory access)."""
    monkeypatch.setenv("LANCET_EMU_TIER1", "64")
    build_of(fat)
    for gi in range(len(tc.groups("tiny"))):
        tc.assert_oracle_side("tiny", gi)
        _run("tiny", gi, ("tiny", gi, "64 nodes", fat), wide=False)
