"""The wider settle rule on the device: the hand-made windows of settle_component_cases.py and the first 128 windows of the scan batch
against the oracle with the rule on, with LANCET_SETTLE_CHAIN_ONLY=1 and with LANCET_NO_SETTLE=1; two engines taking turns against one
engine; three draws of the suite's random sweep against LANCET_NO_SETTLE=1."""
import pytest

import settle_cases as sc
import settle_component_cases as scc
from lancet_amd import abi, engine, workload

pytestmark = pytest.mark.gpu

DKEYS = sc.KEYS + ("sum_nodes",)
ENV = {"rule": None, "chain_only": "LANCET_SETTLE_CHAIN_ONLY", "off": "LANCET_NO_SETTLE"}


def _run(batch, p, monkeypatch, tag="rule"):
    """(records, stats, windows the hand-off headers mark settled) of one engine on one route; the build kernel's count equals the marks"""
    if ENV[tag]:
        monkeypatch.setenv(ENV[tag], "1")
    try:
        eng = engine.Engine(p, device=0)
    finally:
        if ENV[tag]:
            monkeypatch.delenv(ENV[tag], raising=False)
    v, st = eng.process(batch)
    marks = []
    for w in range(batch.n_windows):
        g = eng.pre_order(w)
        if g and g[0]["settled"]:
            assert g[0]["built"] and not g[0]["have_order"] and not g[0]["done"], (w, g[0])
            marks.append(w)
    assert eng.settled_count() == len(marks), (tag, eng.settled_count(), len(marks))
    eng.close()
    return v, st, marks


def _routes(batch, p, monkeypatch):
    return {tag: _run(batch, p, monkeypatch, tag) for tag in ENV}


def test_hand_made_windows_settled_or_not_and_equal_to_the_oracle(monkeypatch):
    scc.assert_oracle_side()
    scc.assert_results(_routes(scc.batch(), abi.default_params(**scc.PARAMS), monkeypatch), what="device", keys=DKEYS)


def test_hand_made_windows_with_kmer_recovery(monkeypatch):
    b = workload.sub_batch(scc.batch(), 0, scc.R_CASES)
    scc.assert_results(_routes(b, abi.default_params(kmer_recovery=1, **scc.PARAMS), monkeypatch), what="device -R", keys=DKEYS, n=scc.R_CASES)


def test_scan_batch_with_the_rule_chain_only_and_off(monkeypatch):
    b = sc.scan_batch(128)
    ov, ost, otr = sc.scan_oracle(128)
    routes = _routes(b, abi.default_params(), monkeypatch)
    for tag, (v, st, _) in routes.items():
        bad = [w for w in range(b.n_windows) if any(st[w][k] != ost[w][k] for k in DKEYS)]
        assert not bad, (tag, bad[:5], [(st[w], ost[w]) for w in bad[:2]])
        assert v == ov, tag
    settled, old = routes["rule"][2], routes["chain_only"][2]
    assert routes["off"][2] == []
    have_rec = {r["window"] for r in ov}
    for w in settled:
        assert ost[w]["n_builds"] == 1 and ost[w]["n_variants"] == 0 and ost[w]["status"] == 0 and w not in have_rec, (w, ost[w])
    cls = scc.source_chain_class(otr, ov, b)
    plain = sc.plain_chains(otr, ov, b)
    print("settled %d (chain only %d), class of the oracle's trace %d, of it not settled %s" % (len(settled), len(old), len(cls), sorted(set(cls) - set(settled))))
    assert len(cls) >= 25 and len(settled) >= 0.8 * len(cls), (len(settled), len(cls))
    assert set(old) <= set(settled) and set(old) <= set(plain) and len(old) < len(settled), (len(old), len(settled))


def test_two_engines_taking_turns_leave_one_engine_s_records():
    """two batches of 256 windows through a pair of engines submitted in turn (the second batch's build kernel starts under the end of the
    first's window kernel, where the settled windows are taken) against one engine batch by batch"""
    p = abi.default_params()
    batches = [workload.make_scan_batch(256, 30, 30, seed=sd) for sd in (61, 62)]
    key = lambda s: tuple(s[k] for k in DKEYS)
    one = engine.Engine(p)
    want = []
    for b in batches:
        v, st = one.process(b)
        assert one.settled_count() > 0
        want.append((v, [key(s) for s in st]))
    one.close()
    pair = [engine.Engine(p), engine.Engine(p)]
    got = [None, None]
    pair[0].upload(batches[0]); pair[0].submit()
    pair[1].upload(batches[1]); pair[1].submit(after=pair[0])
    for i in (0, 1):
        pair[i].wait()
        v, st = pair[i].results()
        got[i] = (v, [key(s) for s in st])
    for e_ in pair:
        e_.close()
    assert got == want, [a == b for a, b in zip(got, want)]


@pytest.mark.parametrize("seed", [1, 4, 9])
def test_draws_of_the_random_sweep_with_the_rule_and_with_settling_off(seed, monkeypatch):
    """options and workloads as test_engine_gpu_sweep.py draws them, 128 windows each"""
    from test_engine_gpu_sweep import draw
    over, wl = draw(seed)
    p = abi.default_params(**over)
    batch = workload.make_scan_batch(128, seed=900 + seed, **wl)
    v1, s1, _ = _run(batch, p, monkeypatch)
    v0, s0, none = _run(batch, p, monkeypatch, "off")
    assert none == []
    assert v1 == v0, (over, wl)
    assert [[s[k] for k in DKEYS] for s in s1] == [[s[k] for k in DKEYS] for s in s0], (over, wl)
