"""Settled windows on the device: the hand-made windows of settle_cases.py and the first 128 windows of its scan batch against the oracle
with settling on and with LANCET_NO_SETTLE=1, the switches that keep settling off, and settling under the engine's scheduling (two engines
taking turns, a run repeated, one draw of the suite's random sweep)."""
import pytest

import golden_util as gu
import hap_cases as hc
import settle_cases as sc
from lancet_amd import abi, engine, workload
from oracle import oracle

pytestmark = pytest.mark.gpu

DKEYS = sc.KEYS + ("sum_nodes",)


def _run(batch, p, monkeypatch, settle=True, **kw):
    """(records, stats, windows the hand-off headers mark settled, the build kernel's count) of one engine"""
    if not settle:
        monkeypatch.setenv("LANCET_NO_SETTLE", "1")
    try:
        eng = engine.Engine(p, device=0, **kw)
    finally:
        monkeypatch.delenv("LANCET_NO_SETTLE", raising=False)
    v, st = eng.process(batch)
    marks = []
    for w in range(batch.n_windows):
        g = eng.pre_order(w)
        if g and g[0]["settled"]:
            assert g[0]["built"] and not g[0]["have_order"] and not g[0]["done"], (w, g[0])
            marks.append(w)
    n = eng.settled_count()
    return eng, v, st, marks, n


@pytest.mark.parametrize("gi", range(len(sc.groups())))
def test_hand_made_windows_settled_or_not_and_equal_to_the_oracle(gi, monkeypatch):
    params, cs, batch = sc.groups()[gi]
    sc.assert_oracle_side(gi)
    p = abi.default_params(**params)
    e1, v1, s1, settled, n1 = _run(batch, p, monkeypatch)
    e0, v0, s0, none, n0 = _run(batch, p, monkeypatch, settle=False)
    e1.close(); e0.close()
    assert (none, n0) == ([], 0) and n1 == len(settled)
    sc.assert_case_results(gi, (v1, s1), (v0, s0), set(settled), device=True, what="device")


def test_scan_batch_settled_windows_are_the_plain_reference_chains(monkeypatch):
    b = sc.scan_batch(128)
    p = abi.default_params()
    ov, ost, otr = sc.scan_oracle(128)
    e1, v1, s1, settled, n1 = _run(b, p, monkeypatch)
    e0, v0, s0, none, n0 = _run(b, p, monkeypatch, settle=False)
    e1.close(); e0.close()
    assert (none, n0) == ([], 0) and n1 == len(settled)
    for tag, v, st in (("on", v1, s1), ("off", v0, s0)):
        bad = [w for w in range(b.n_windows) if any(st[w][k] != ost[w][k] for k in DKEYS)]
        assert not bad, (tag, bad[:5], [(st[w], ost[w]) for w in bad[:2]])
        assert v == ov, tag
    have_rec = {r["window"] for r in ov}
    for w in settled:
        assert ost[w]["n_builds"] == 1 and ost[w]["n_variants"] == 0 and ost[w]["status"] == 0 and w not in have_rec, (w, ost[w])
    plain = sc.plain_chains(otr, ov, b)
    print("settled %d, plain chains of the oracle's trace %d, plain chains not settled %s" % (len(settled), len(plain), sorted(set(plain) - set(settled))))
    assert len(plain) >= 20 and len(settled) >= 0.8 * len(plain), (len(settled), len(plain))


def test_trace_haplotypes_and_linked_reads_keep_settling_off(monkeypatch):
    params, cs, batch = sc.groups()[0]
    p = abi.default_params(**params)
    eng, v, st, settled, n = _run(batch, p, monkeypatch, trace_words=1 << 15)
    assert (settled, n) == ([], 0) and v == sc.oracle_of(0)[0]
    assert gu.digest_trace(eng.trace_text()) == gu.digest_trace(sc.oracle_of(0)[2])
    eng.close()
    eng, v, st, settled, n = _run(batch, p, monkeypatch, haplotype_words=hc.ample_words(batch, p))
    haps, _ = eng.haplotypes()
    eng.close()
    assert (settled, n) == ([], 0) and v == sc.oracle_of(0)[0]
    for w, c in enumerate(cs):
        if c.settled:
            mine = [h for h in haps if h["window"] == w]
            assert len(mine) >= 1 and all(h["flags"] & abi.HAP_IS_REF for h in mine), (c.name, mine)
    lparams, _, lbatch = sc.linked_group()
    lp = abi.default_params(**lparams)
    ov, ost, _ = oracle.run(lbatch, lp)
    eng, v, st, settled, n = _run(lbatch, lp, monkeypatch)
    eng.close()
    assert (settled, n) == ([], 0) and v == ov
    assert [[s[k] for k in sc.KEYS] for s in st] == [[s[k] for k in sc.KEYS] for s in ost]


def test_two_engines_taking_turns_and_a_repeated_run_leave_the_same_records():
    """Two batches of 256 windows through a pair of engines submitted in turn (the gate on: the second batch's build kernel starts under the
    end of the first's window kernel, where the settled windows are taken): what one engine gives batch by batch, twice over."""
    p = abi.default_params()
    batches = [workload.make_scan_batch(256, 30, 30, seed=sd) for sd in (51, 52)]
    key = lambda s: tuple(s[k] for k in DKEYS)
    one = engine.Engine(p)
    want = []
    for b in batches:
        v, st = one.process(b)
        assert one.settled_count() > 0
        want.append((v, [key(s) for s in st]))
    v, st = one.process(batches[1])                                    # the same batch again on the same engine
    assert (v, [key(s) for s in st]) == want[1]
    one.close()
    pair = [engine.Engine(p), engine.Engine(p)]
    for rep in range(2):
        got = [None, None]
        pair[0].upload(batches[0]); pair[0].submit()
        pair[1].upload(batches[1]); pair[1].submit(after=pair[0])
        for i in (0, 1):
            pair[i].wait()
            v, st = pair[i].results()
            got[i] = (v, [key(s) for s in st])
        assert got == want, (rep, [a == b for a, b in zip(got, want)])
    for e_ in pair:
        e_.close()


@pytest.mark.parametrize("seed", [0, 3, 7])
def test_draws_of_the_random_sweep_with_settling_on_and_off(seed, monkeypatch):
    """options and workloads as test_engine_gpu_sweep.py draws them (odd first k: the build kernel takes the windows), 128 windows each"""
    from test_engine_gpu_sweep import draw
    over, wl = draw(seed)
    p = abi.default_params(**over)
    batch = workload.make_scan_batch(128, seed=700 + seed, **wl)
    e1, v1, s1, settled, n1 = _run(batch, p, monkeypatch)
    e0, v0, s0, none, n0 = _run(batch, p, monkeypatch, settle=False)
    e1.close(); e0.close()
    assert (none, n0) == ([], 0) and n1 == len(settled)
    assert v1 == v0, (over, wl)
    assert [[s[k] for k in DKEYS] for s in s1] == [[s[k] for k in DKEYS] for s in s0], (over, wl)
