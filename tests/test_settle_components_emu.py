"""The wider settle rule on the host emulation of the kernels (tests/settle_emu, LANCET_EMU_SETTLE=1): the hand-made windows of
settle_component_cases.py and the scan batch of settle_cases.py, each against the oracle with the rule on, with LANCET_SETTLE_CHAIN_ONLY=1
(the rule before it) and with settling off.  The device's side of the same checks is test_settle_components_gpu.py."""
import os
import sys

import pytest

import settle_cases as sc
import settle_component_cases as scc
from lancet_amd import abi
from test_settle_emu import _oracle_scan

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "settle_emu"))
import emu  # noqa: E402
import settle_emu  # noqa: E402

# the windows the rule before this one settles in the scan batch (the parent's set, read off its build): LANCET_SETTLE_CHAIN_ONLY=1 has to give it back
CHAIN_ONLY_SCAN = 97
NOT_CHAIN_ONLY = (329, 368)          # plain chains of the oracle's trace that it does not settle


@pytest.fixture(params=["wave", "fat"])
def source(request):
    """both host builds of the kernels: the one-wave source and the re-run tier's (LANCET_FAT)"""
    emu.FAT[0] = request.param == "fat"
    yield request.param
    emu.FAT[0] = False


def _routes(batch, p, monkeypatch):
    """{route: (records, stats, settled windows)} with the rule, with the chain-only rule and with settling off"""
    out = {}
    for tag in ("rule", "chain_only", "off"):
        if tag == "chain_only":
            monkeypatch.setenv("LANCET_SETTLE_CHAIN_ONLY", "1")
        try:
            v, st, _, _, settled = settle_emu.run(batch, p, settle=tag != "off")
        finally:
            monkeypatch.delenv("LANCET_SETTLE_CHAIN_ONLY", raising=False)
        out[tag] = (v, st, settled)
    return out


def test_hand_made_windows_settled_or_not_and_equal_to_the_oracle(source, monkeypatch):
    scc.assert_oracle_side()
    scc.assert_results(_routes(scc.batch(), abi.default_params(**scc.PARAMS), monkeypatch), what="emu " + source)


def test_hand_made_windows_with_kmer_recovery(source, monkeypatch):
    from lancet_amd import workload
    b = workload.sub_batch(scc.batch(), 0, scc.R_CASES)
    scc.assert_results(_routes(b, abi.default_params(kmer_recovery=1, **scc.PARAMS), monkeypatch), what="emu -R " + source, n=scc.R_CASES)


def test_scan_batch_settles_the_chains_beside_source_less_components(monkeypatch):
    b = sc.scan_batch()
    ov, ost, otr = _oracle_scan()
    routes = _routes(b, abi.default_params(), monkeypatch)
    for tag, (v, st, _) in routes.items():
        bad = [w for w in range(b.n_windows) if any(st[w][k] != ost[w][k] for k in sc.KEYS)]
        assert not bad, (tag, bad[:5], [(st[w], ost[w]) for w in bad[:2]])
        assert v == ov, tag
    settled, old = routes["rule"][2], routes["chain_only"][2]
    assert routes["off"][2] == []
    have_rec = {r["window"] for r in ov}
    for w in settled:
        assert ost[w]["n_builds"] == 1 and ost[w]["n_variants"] == 0 and ost[w]["status"] == 0 and w not in have_rec, (w, ost[w])
    cls = scc.source_chain_class(otr, ov, b)
    print("settled %d (chain only %d), class of the oracle's trace %d, of it not settled %s, settled outside it %s"
          % (len(settled), len(old), len(cls), sorted(set(cls) - set(settled)), sorted(set(settled) - set(cls))))
    assert len(cls) == scc.C_EXPECTED, len(cls)
    assert len(settled) >= 0.8 * len(cls), (len(settled), len(cls))
    assert len(old) == CHAIN_ONLY_SCAN and not set(old) & set(NOT_CHAIN_ONLY) and set(old) <= set(settled), (len(old), sorted(set(old) - set(settled)))
    plain = sc.plain_chains(otr, ov, b)
    assert set(old) == set(plain) - set(NOT_CHAIN_ONLY), sorted(set(old) ^ set(plain))
