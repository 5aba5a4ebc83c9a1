"""Windows whose reference contains N through the LDS build kernel (tests/nref_cases.py) on the device, through engine.Engine: what the
emulator cannot show -- a race between the lanes that settle the N nodes, a barrier missing around the table fix-up, a miscompile.
Records, per-window statistics and the digest of the -v trace equal the oracle's, and every window's first graph comes from the LDS
build (Engine.prebuilt_count()); until the build kernel took N that count was 0 for these batches."""
import os

import pytest

import golden_util as gu
import nref_cases as nc
from lancet_amd import abi, engine

pytestmark = pytest.mark.gpu

# (tools/fat_check.sh runs the suite with a 64-entry tier-1 node table: what tier 1 itself served is not counted then)
TIER1 = "LANCET_NODE_CAP1" not in os.environ
EVT = 1 << 18


def _check(eng, batch, want, what, n_built=None):
    v, st = eng.process(batch)
    nc.assert_equal_to_oracle((v, st, eng.trace_text()), want, what=what)
    if TIER1:
        assert eng.prebuilt_count() == (batch.n_windows if n_built is None else n_built), (what, eng.prebuilt_count(), batch.n_windows)


def test_hand_made_windows():
    """One N, runs of k - 1, k, k + 1 and 2k, N at the window's edges, the k-mer that is its own reverse complement at odd k, the inverted
    repeat across N, reads that carry A -- or the other three bases -- where the reference shows N; the batch, then every window alone."""
    from lancet_amd import workload
    from oracle import oracle
    nc.hand_preconditions()
    batch, _ = nc.hand_made()
    p = abi.default_params()
    eng = engine.Engine(p, device=0, trace_words=EVT)
    _check(eng, batch, nc.oracle_of("hand"), "hand")
    for w, name in enumerate(nc.HAND):
        one = workload.sub_batch(batch, w, w + 1)
        _check(eng, one, oracle.run(one, p, verbose=True), name)
    eng.close()


@pytest.mark.parametrize("wide", [False, True], ids=["default", "wide"])
def test_the_1024_lane_configuration(wide, monkeypatch):
    """A window of more than 512 reads, and STR-rich 100x / 40x windows that climb past k = 31 (keys of more than one word), with the
    narrow and with the wide hand-off areas."""
    if wide:
        monkeypatch.setenv("LANCET_PRE_WIDE", "1")
    eng = engine.Engine(abi.default_params(), device=0, trace_words=EVT)
    _check(eng, nc.many_reads()[0], nc.oracle_of("many_reads"), ("many_reads", wide))
    want = nc.oracle_of("deep_str")
    assert max(s["final_k"] for s in want[1]) > 63
    _check(eng, nc.deep_str()[0], want, ("deep_str", wide))
    eng.close()


@pytest.mark.parametrize("env", [{}, {"LANCET_NO_SVC": "1"}, {"LANCET_AHEAD_DEPTH": "0", "LANCET_SVC_DEPTH": "0"}, {"LANCET_NO_PREBUILD": "1"}],
                         ids=["service", "no-service", "nothing-ahead", "no-lds-build"])
def test_graphs_built_ahead_and_by_the_service_next_to_n(env, monkeypatch):
    """Duplications next to N: k climbs through several graphs per window; the same records whoever builds the later graphs."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    batch, _ = nc.climbing()
    want = nc.oracle_of("climbing")
    assert max(s["n_builds"] for s in want[1]) >= 5
    eng = engine.Engine(abi.default_params(), device=0, trace_words=EVT)
    _check(eng, batch, want, env, n_built=0 if "LANCET_NO_PREBUILD" in env else None)
    if not env and TIER1:
        assert sum(eng.ahead_counts()) > 0 or sum(eng.svc_counts()) > 0
    eng.close()


def test_linked_reads_with_n():
    """--linked-reads: haplotype counts and barcode sets in the records; an N node has no run to replay."""
    batch, _ = nc.linked()
    want = nc.oracle_of("linked", True)
    assert any(any(len(x) for x in r["bx"]) for r in want[0]) and any(any(r["hp"]) for r in want[0])
    eng = engine.Engine(abi.default_params(lr_mode=1), device=0, trace_words=EVT)
    _check(eng, batch, want, "linked")
    eng.close()


def test_recovery_finds_no_acceptor_in_an_n_node():
    """-R on the hand-made window whose donor k-mers, mutated, are the 2-bit image of the reference's N k-mers: same records, statistics
    and route with and without the flag (and without it, the oracle's)."""
    batch, _ = nc.recovery_window()
    want = nc.oracle_of("recovery")
    runs = []
    for flag in (0, 1):
        eng = engine.Engine(abi.default_params(kmer_recovery=flag), device=0, trace_words=EVT)
        v, st = eng.process(batch)
        tr = eng.trace_text()
        runs.append((v, [nc.KEY(s) for s in st], gu.digest_trace(tr), eng.prebuilt_count()))
        if flag == 0:
            nc.assert_equal_to_oracle((v, st, tr), want, what="recovery")
        eng.close()
    assert runs[0] == runs[1]
    if TIER1:
        assert runs[0][3] == 1


def test_mixed_batch_twice_through_one_engine():
    """N windows between ordinary ones, twice through one engine (the hand-off areas are used again)."""
    batch, _ = nc.mixed()
    eng = engine.Engine(abi.default_params(), device=0, trace_words=EVT)
    for i in range(2):
        _check(eng, batch, nc.oracle_of("mixed"), ("mixed", i))
    eng.close()


def test_the_reference_made_goldens_take_the_new_route():
    """tests/golden/nref.* and tests/golden/recovery/rec_nref.*: every window's first graph is built in LDS now; their parity with the
    reference's own output is test_engine_gpu.py's and test_recovery_gpu.py's."""
    import recovery_util as ru
    meta, batch, kept, (min_k, max_k) = gu.case_batch("nref")
    eng = engine.Engine(gu.params(meta), device=0)
    eng.process(batch)
    if TIER1:
        assert eng.prebuilt_count() == batch.n_windows
    eng.close()
    m, rbatch, _ = ru.case_batch("rec_nref")
    for flag in (False, True):
        eng = engine.Engine(ru.params(m, flag), device=0)
        eng.process(rbatch)
        if TIER1:
            assert eng.prebuilt_count() == rbatch.n_windows, flag
        eng.close()
