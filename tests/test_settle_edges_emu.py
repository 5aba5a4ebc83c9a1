"""The settle rule at its capacity, group and word edges on the host emulation of the kernels (tests/settle_emu, LANCET_EMU_SETTLE=1): the
windows of settle_edge_cases.py against the oracle with the rule on, with LANCET_SETTLE_CHAIN_ONLY=1 and with settling off, under the
hand-off the batch gets by itself and under LANCET_PRE_WIDE=1, on both host builds.  The settled set is exactly what the cases state, and
the hand-off headers say the same.  The device's side of the same checks is test_settle_edges_gpu.py."""
import os
import sys

import pytest

import settle_edge_cases as sec
from lancet_amd import abi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "settle_emu"))
import emu  # noqa: E402
import settle_emu  # noqa: E402


@pytest.fixture(params=["wave", "fat"])
def source(request):
    """both host builds of the kernels: the one-wave source and the re-run tier's (LANCET_FAT)"""
    emu.FAT[0] = request.param == "fat"
    yield request.param
    emu.FAT[0] = False


def test_the_sizes_come_from_the_headers():
    """cap as build_lds_impl.h forms it: the edge slots begin where st_own[cap] ends; and the cases on both sides of every size fit the forms"""
    for large in (False, True):
        L = sec.limits(large)
        assert L["cap"] + L["st_fixed"] == L["ncap"] // 4                     # ST + ST_FIXED + cap == E - (S.big + BL_NCAP / 32)
        assert L["st_fixed"] == 4 + 3 * (L["maxw"] // 32) + L["scap"] // 32
        assert 0 < L["gmax"] < min(L["cap"], L["scap"]) <= 2 * L["gmax"]      # one group or two, never more
    assert sec.limits(False)["cap"] < sec.limits(False)["scap"] <= sec.limits(True)["cap"]      # the 512-lane form is held by its words, the 1024-lane form by PB_SCAP


def _routes(batch, p, monkeypatch, wide):
    """{route: (records, stats, settled windows)} and, of the route with the rule, the hand-off headers and why a window was not built"""
    out = {}
    if wide:
        monkeypatch.setenv("LANCET_PRE_WIDE", "1")
    try:
        for tag in ("rule", "chain_only", "off"):
            if tag == "chain_only":
                monkeypatch.setenv("LANCET_SETTLE_CHAIN_ONLY", "1")
            try:
                v, st, _, _, settled = settle_emu.run(batch, p, settle=tag != "off", pre_order=tag == "rule")
            finally:
                monkeypatch.delenv("LANCET_SETTLE_CHAIN_ONLY", raising=False)
            out[tag] = (v, st, settled)
            if tag == "rule":
                heads, why = [g[0] if g else None for g in emu.LAST_PRE_ORDER], list(settle_emu.LAST_WHY)
    finally:
        monkeypatch.delenv("LANCET_PRE_WIDE", raising=False)
    return out, heads, why


@pytest.mark.parametrize("wide", [False, True], ids=["default", "pre_wide"])
@pytest.mark.parametrize("family,gi", sec.all_groups())
def test_edge_windows_settled_or_not_and_equal_to_the_oracle(family, gi, wide, source, monkeypatch):
    params, cs, batch = sec.groups(family)[gi]
    sec.assert_oracle_side(family, gi)
    routes, heads, why = _routes(batch, abi.default_params(**params), monkeypatch, wide)
    sec.assert_results(family, gi, routes, wide, what="emu %s %s" % (source, "pre_wide" if wide else "default"))
    settled = routes["rule"][2]
    assert [w for w, g in enumerate(heads) if g and g["settled"]] == settled
    for w, c in enumerate(cs):
        g, want_why = heads[w], c.why_wide if wide else c.why
        assert g is not None, c.name
        if g["settled"]:
            assert g["built"] and not g["have_order"] and not g["done"], (c.name, g)
        if want_why is not None:
            assert why[w] == want_why and g["built"] == (want_why == 0), (c.name, "why", why[w], g)
        if g["built"]:
            assert bool(g["big"]) == (c.big or c.params["min_k"] > 31), (c.name, "1024-lane form", g["big"])
            if c.nsurv is not None:
                assert g["nsurv"] == c.nsurv, (c.name, g["nsurv"])
            if c.N is not None:
                assert g["N"] == c.N, (c.name, g["N"])
