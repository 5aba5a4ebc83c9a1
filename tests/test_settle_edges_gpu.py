"""The settle rule at its capacity, group and word edges on the device: the windows of settle_edge_cases.py, one batch per family and
parameter set, against the oracle with the rule on, with LANCET_SETTLE_CHAIN_ONLY=1 and with LANCET_NO_SETTLE=1, under the hand-off the
batch gets by itself and under LANCET_PRE_WIDE=1.  Every batch runs twice on one engine and reads back the same both times: the barriers
around the fill of the test's words, the atomic passes over the bitmaps and the loop over the groups of survivors are real only here (the
host emulation runs the lanes one after the other)."""
import pytest

import settle_edge_cases as sec
from lancet_amd import abi, engine

pytestmark = pytest.mark.gpu

DKEYS = sec.KEYS + ("sum_nodes",)
ENV = {"rule": None, "chain_only": "LANCET_SETTLE_CHAIN_ONLY", "off": "LANCET_NO_SETTLE"}


def _read_back(eng, batch, tag):
    """(records, stats, windows the hand-off headers mark settled, the headers); the build kernel's count equals the marks"""
    v, st = eng.process(batch)
    marks, heads = [], []
    for w in range(batch.n_windows):
        g = eng.pre_order(w)
        heads.append(g[0] if g else None)
        if g and g[0]["settled"]:
            assert g[0]["built"] and not g[0]["have_order"] and not g[0]["done"], (w, g[0])
            marks.append(w)
    assert eng.settled_count() == len(marks), (tag, eng.settled_count(), len(marks))
    return v, st, marks, heads


def _run(batch, p, monkeypatch, tag, wide):
    """one engine on one route, the batch twice: the second read-back equal to the first"""
    for name in ([ENV[tag]] if ENV[tag] else []) + (["LANCET_PRE_WIDE"] if wide else []):
        monkeypatch.setenv(name, "1")
    try:
        eng = engine.Engine(p, device=0)
    finally:
        for name in ("LANCET_SETTLE_CHAIN_ONLY", "LANCET_NO_SETTLE", "LANCET_PRE_WIDE"):
            monkeypatch.delenv(name, raising=False)
    first = _read_back(eng, batch, tag)
    again = _read_back(eng, batch, tag)
    eng.close()
    key = lambda r: (r[0], [[s[k] for k in DKEYS] for s in r[1]], r[2], [(g["built"], g["N"], g["nsurv"], g["big"], g["settled"]) if g else None for g in r[3]])
    assert key(again) == key(first), (tag, "a second run on the same engine reads back differently")
    return first


@pytest.mark.parametrize("wide", [False, True], ids=["default", "pre_wide"])
@pytest.mark.parametrize("family,gi", sec.all_groups())
def test_edge_windows_settled_or_not_and_equal_to_the_oracle(family, gi, wide, monkeypatch):
    params, cs, batch = sec.groups(family)[gi]
    sec.assert_oracle_side(family, gi)
    p = abi.default_params(**params)
    got = {tag: _run(batch, p, monkeypatch, tag, wide) for tag in ENV}
    sec.assert_results(family, gi, {tag: r[:3] for tag, r in got.items()}, wide, what="device " + ("pre_wide" if wide else "default"), keys=DKEYS)
    for w, (c, g) in enumerate(zip(cs, got["rule"][3])):
        assert g is not None, c.name
        want_why = c.why_wide if wide else c.why
        if want_why is not None:
            assert g["built"] == (want_why == 0), (c.name, g)
        if g["built"]:
            assert bool(g["big"]) == (c.big or c.params["min_k"] > 31), (c.name, "1024-lane form", g["big"])
            if c.nsurv is not None:
                assert g["nsurv"] == c.nsurv, (c.name, g["nsurv"])
            if c.N is not None:
                assert g["N"] == c.N, (c.name, g["N"])
