"""Settled windows on the host emulation of the kernels (tests/settle_emu): the hand-made windows of settle_cases.py and a scan batch, each
against the oracle with settling on and with settling off, and the switches that keep settling off (trace, haplotype capture, linked
reads).  The device's side of the same checks is test_settle_gpu.py."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

import golden_util as gu
import hap_cases as hc
import settle_cases as sc
from lancet_amd import abi, workload
from oracle import oracle

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


@pytest.mark.parametrize("gi", range(len(sc.groups())))
def test_hand_made_windows_settled_or_not_and_equal_to_the_oracle(gi, source):
    params, cs, batch = sc.groups()[gi]
    sc.assert_oracle_side(gi)
    p = abi.default_params(**params)
    v1, s1, _, _, settled = settle_emu.run(batch, p, settle=True, pre_order=True)
    marks = [g[0]["settled"] if g else 0 for g in emu.LAST_PRE_ORDER]      # (the read-back of the hand-off areas says the same as the headers)
    v0, s0, _, _, none = settle_emu.run(batch, p, settle=False)
    assert none == []
    sc.assert_case_results(gi, (v1, s1), (v0, s0), set(settled), what="emu " + source)
    assert [w for w, m in enumerate(marks) if m] == settled
    for w in settled:
        g = emu.LAST_PRE_ORDER[w][0] if emu.LAST_PRE_ORDER and emu.LAST_PRE_ORDER[w] else None
        assert g is None or (g["built"] and not g["have_order"] and not g["done"]), (cs[w].name, g)


def _oracle_scan():
    """the oracle on the scan batch, in slices side by side: (records, stats, -v trace)"""
    b = sc.scan_batch()
    cuts = [(a, min(b.n_windows, a + 25)) for a in range(0, b.n_windows, 25)]

    def one(ab):
        v, st, tr = oracle.run(workload.sub_batch(b, ab[0], ab[1]), abi.default_params(), verbose=True)
        for r in v:
            r["window"] += ab[0]
        return v, st, tr

    oracle.lib()
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        res = list(ex.map(one, cuts))
    return [r for v, _, _ in res for r in v], [s for _, st, _ in res for s in st], "".join(tr for _, _, tr in res)


def test_scan_batch_settled_windows_are_the_plain_reference_chains():
    b = sc.scan_batch()
    p = abi.default_params()
    ov, ost, otr = _oracle_scan()
    v1, s1, _, _, settled = settle_emu.run(b, p, settle=True)
    v0, s0, _, _, none = settle_emu.run(b, p, settle=False)
    assert none == []
    for tag, v, st in (("on", v1, s1), ("off", v0, s0)):
        bad = [w for w in range(b.n_windows) if any(st[w][k] != ost[w][k] for k in sc.KEYS)]
        assert not bad, (tag, bad[:5], [(st[w], ost[w]) for w in bad[:2]])
        assert v == ov, tag
    have_rec = {r["window"] for r in ov}
    for w in settled:
        assert ost[w]["n_builds"] == 1 and ost[w]["n_variants"] == 0 and ost[w]["status"] == 0 and w not in have_rec, (w, ost[w])
    plain = sc.plain_chains(otr, ov, b)
    assert len(plain) == sc.P_EXPECTED, len(plain)
    print("settled %d, plain chains of the oracle's trace %d, plain chains not settled %s" % (len(settled), len(plain), sorted(set(plain) - set(settled))))
    assert len(settled) >= 0.8 * len(plain), (len(settled), len(plain))


def test_tracing_keeps_settling_off():
    for gi, (params, cs, batch) in enumerate(sc.groups()):
        p = abi.default_params(**params)
        v, st, text, _, settled = settle_emu.run(batch, p, settle=True, evt_cap=1 << 15)
        assert settled == []
        assert gu.digest_trace(text) == gu.digest_trace(sc.oracle_of(gi)[2])
        assert v == sc.oracle_of(gi)[0]


def test_haplotype_capture_keeps_settling_off_and_reference_only_windows_deliver_their_haplotype():
    params, cs, batch = sc.groups()[0]
    p = abi.default_params(**params)
    v, st, _, haps, settled = settle_emu.run(batch, p, settle=True, hap_words=hc.ample_words(batch, p))
    assert settled == []
    assert v == sc.oracle_of(0)[0]
    for w, c in enumerate(cs):
        if c.settled:                                                  # settled without the capture: here its one path, identical to the reference
            mine = [h for h in haps if h["window"] == w]
            assert len(mine) >= 1 and all(h["flags"] & abi.HAP_IS_REF for h in mine), (c.name, mine)


def test_linked_reads_keep_settling_off():
    params, cs, batch = sc.linked_group()
    p = abi.default_params(**params)
    ov, ost, _ = oracle.run(batch, p)
    v, st, _, _, settled = settle_emu.run(batch, p, settle=True)
    assert settled == []
    assert v == ov and [[s[k] for k in sc.KEYS] for s in st] == [[s[k] for k in sc.KEYS] for s in ost]
