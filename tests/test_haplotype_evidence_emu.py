"""The variant evidence (lancet_engine_set_haplotype_evidence) without a GPU: the emulated window kernels with the capture and the emulated
evidence kernel behind them (tests/hap_evid_emu: lancet_amd/csrc/hap_evidence.h, the source the engine compiles for the device), on the
one-wave form and on the LANCET_FAT form of the window kernels.  Hand-made windows whose counts are known from how their reads were cut;
every edge of the kernel and the five more_verbose fixtures against the plain model of tests/hap_evid_cases.py; hand-written entry buffers
for the shapes no assembly produces; lc_evid_join against abi.evidence_variant and the reference's own records.
test_haplotype_evidence_gpu.py holds the engine to the same."""
import os
import sys

import numpy as np
import pytest

import hap_evid_cases as ec
import hap_place_cases as pc
import hap_sup_cases as sc
import more_verbose_util as mv
from lancet_amd import abi

_TESTS = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_TESTS, "hap_evid_emu"))
import hap_evid_emu  # noqa: E402
from hap_evid_emu import emu  # noqa: E402

BUILDS = pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
K = 15


@pytest.fixture
def build(request):
    emu.FAT[0] = request.param == "fat"
    yield request.param
    emu.FAT[0] = False


def _run(batch, p, words=None, mm=5, evid=64, **kw):
    return hap_evid_emu.run(batch, p, hap_words=sc.ample_words(batch, p) + 32 * 64 if words is None else words, mm=mm, evid=evid, **kw)


def _rand(seed, n):
    return sc._rand(np.random.default_rng(seed), n)


def _hand(entries, reads, mm=5, **kw):
    """The hand-written window through the kernel, held to the model; returns the events per entry."""
    got, marked = hap_evid_emu.hand(entries, reads, mm, **kw)
    want = ec.model_hand(entries, reads, mm)
    assert not marked and [ec.strip(g) for g in got] == want, ([ec.strip(g) for g in got], want)
    assert all(e["variant"] == -1 for g in got for e in g)
    return got


# ---------------------------------------------------------------- counts known without the model

@BUILDS
@pytest.mark.parametrize("variant", ["snv", "del3"])
def test_planted_counts(variant, build):
    """Item 1: the two paths, one group; the alt path's one event has alt = [5, 4, 0, 0], ref = [2, 3, 4, 6], other = 0."""
    batch, p, alt, ref, _ = sc.basic_batch(variant)
    v, st, text, haps, trunc, marked = _run(batch, p, sup=True)
    sc.check_basic(variant, batch, st, haps, trunc)
    ec.check_basic(variant, batch, st, haps, trunc, marked)
    ec.check_model(batch, p, haps, 5)
    ec.check_invariants(haps, True)
    ec.check_join(batch, haps, v, marked, abi.evidence_variant)


# ---------------------------------------------------------------- the fixtures: join, model, invariants, nothing else changes

@BUILDS
@pytest.mark.parametrize("case", mv.CASES)
def test_fixtures_join_model_and_invariants(case, build):
    m, batch, kept = mv.case_batch(case)
    p = mv.params(m)
    words = sc.ample_words(batch, p) + 32 * 64
    tw = mv.trace_words(batch, p)
    on = hap_evid_emu.run(batch, p, evt_cap=tw, hap_words=words, aln=True, sup=True, evid=256)
    off = hap_evid_emu.run(batch, p, evt_cap=tw, hap_words=words, aln=True, sup=True, evid=0)
    v, st, text, haps, trunc, marked = on
    assert haps and not any(trunc) and not any(marked) and any(h["events"] for h in haps)
    assert on[:3] == off[:3] and on[4] == off[4] and [{k: x for k, x in h.items() if k != "events"} for h in haps] == off[3]
    ec.check_join(batch, haps, v, marked, abi.evidence_variant)
    ec.check_model(batch, p, haps, 5)
    ec.check_invariants(haps, True)
    # without the alignments the switch does nothing
    none = hap_evid_emu.run(batch, p, hap_words=words, aln=False, evid=256)
    assert all(h["events"] == [] for h in none[3]) and not any(none[5])


@BUILDS
def test_rerun_tier(build, monkeypatch):
    m, batch, kept = mv.case_batch("mv_dups")
    p = mv.params(m)
    want = _run(batch, p, evid=256)
    monkeypatch.setenv("LANCET_EMU_TIER1", "64")
    got = _run(batch, p, evid=256)
    assert got[3] == want[3] and got[5] == want[5]


# ---------------------------------------------------------------- edges on assembled windows

@BUILDS
@pytest.mark.parametrize("k", [11, 15, 35])
def test_edges_against_the_model(k, build):
    """sc.edge_batch: read lengths 15 .. 65, k and k - 1, trimmed reads, the N read, 63 .. 129 offsets, two components, no entry, no reads."""
    batch, p, names = sc.edge_batch(k)
    v, st, text, haps, trunc, marked = _run(batch, p, sup=True)
    assert not any(trunc) and not any(marked)
    want, _ = ec.check_model(batch, p, haps, 5)
    ec.check_invariants(haps, True)
    ec.check_join(batch, haps, v, marked, abi.evidence_variant)
    snv = [h for h in haps if h["window"] == names.index("snv")]
    assert sum(len(h["events"]) for h in snv) >= 1 and any(sum(e["alt"]) and sum(e["ref"]) for h in snv for e in h["events"])


@BUILDS
def test_mismatch_limit(build):
    batch, p, names = sc.edge_batch(15)
    total = []
    for mm in (0, 4, 5, 6, 255):
        v, st, text, haps, trunc, marked = _run(batch, p, mm=mm)
        ec.check_model(batch, p, haps, mm)
        total.append(sum(sum(e["alt"]) + sum(e["ref"]) + sum(e["other"]) for h in haps for e in h["events"]))
    assert total == sorted(total) and total[0] > 0


@BUILDS
def test_one_string_at_two_k(build):
    """sc.dups_batch: the same two strings at two k -- two groups, each judged on its own: the event of the changed string has the same
    counts at either k, 5 + 5 tumour reads for it and 5 + 5 normal reads against it."""
    batch, p = sc.dups_batch()
    v, st, text, haps, trunc, marked = _run(batch, p)
    ec.check_model(batch, p, haps, 5)
    ks = {}
    for h in haps:
        ks.setdefault(h["seq"], []).append(h)
    twice = [hs for hs in ks.values() if len({h["kmer"] for h in hs}) >= 2 and hs[0]["events"]]
    assert len(twice) == 1
    for h in twice[0]:
        (e,) = h["events"]
        assert (e["alt"], e["ref"], e["other"]) == ([5, 5, 0, 0], [0, 0, 5, 5], [0] * 4), (h["kmer"], e)


@BUILDS
def test_events_per_window_one_short(build):
    """A window with one event more than it may keep is marked and keeps the first ones, whole and equal to an ample run's."""
    m, batch, kept = mv.case_batch("mv_nref")
    p = mv.params(m)
    full = _run(batch, p, evid=256)
    per = {}
    for h in full[3]:
        per[h["window"]] = per.get(h["window"], 0) + len(h["events"])
    w, n = max(per.items(), key=lambda x: x[1])
    assert n >= 2
    cut = _run(batch, p, evid=n - 1)
    assert cut[:3] == full[:3] and cut[5] == [1 if per.get(x, 0) > n - 1 else 0 for x in range(batch.n_windows)] and cut[5][w] == 1
    ec.check_model(batch, p, cut[3], 5, cap=n - 1)
    mine_full = [e for h in full[3] if h["window"] == w for e in h["events"]]
    mine_cut = [e for h in cut[3] if h["window"] == w for e in h["events"]]
    assert mine_cut == mine_full[:n - 1]
    exact = _run(batch, p, evid=n)
    assert exact[5][w] == 0 and exact[3] == full[3]


# ---------------------------------------------------------------- hand-written entry buffers

def _ref_alt(seed, at=60, n=120):
    ref = _rand(seed, n)
    return ref, ec.entry(ref, []), ec.entry(ref, [(at, "X", ec._OTHER[ref[at]])])


def test_flank_exactly_and_one_short():
    """A read that covers one base on either side of the site exactly, one that is a base short on the left, one a base short on the right."""
    ref, r, a = _ref_alt(1)
    alt = a[0]
    reads = [(alt[59:99], 0), (alt[60:100], 0), (alt[22:62], 1), (alt[21:61], 1), (ref[59:99], 2), (ref[60:100], 2), (ref[22:62], 3), (ref[21:61], 3)]
    got = _hand([r, a], reads)
    (e,) = got[1]
    assert got[0] == [] and (e["alt"], e["ref"], e["other"]) == ([1, 1, 0, 0], [0, 0, 1, 1], [0] * 4)


@pytest.mark.parametrize("at,flank", [(0, False), (1, True), (118, True), (119, False)])
def test_site_at_the_ends_of_a_path(at, flank):
    """A site at path base 1 and at M - 2 has both flanks, one at base 0 and at M - 1 has none: no informative read."""
    ref, r, a = _ref_alt(2, at)
    alt = a[0]
    reads = [(alt[:40], 0), (alt[-40:], 1), (ref[:40], 2), (ref[-40:], 3), (_rand(3, 10) + alt[:30], 0), (alt[-30:] + _rand(4, 10), 1)]
    got = _hand([r, a], reads)
    (e,) = got[1]
    assert (sum(e["alt"]) > 0 and sum(e["ref"]) > 0) == flank and (flank or e["alt"] + e["ref"] + e["other"] == [0] * 12)


def test_indel_beside_a_substitution_is_one_event():
    """A pure insertion (rs = 0) and a pure deletion (ps = 0), each beside an X: one event each, not two."""
    ref = _rand(5, 120)
    r = ec.entry(ref, [])
    ins = ec.entry(ref, [(50, "I", "ACG"), (50, "X", ec._OTHER[ref[50]])])
    dele = ec.entry(ref, [(50, "X", ec._OTHER[ref[50]]), (51, "D", 4)])
    assert [c for c in ins[3]] == [(50, "="), (3, "I"), (1, "X"), (69, "=")] and dele[3] == [(50, "="), (1, "X"), (4, "D"), (65, "=")]
    reads = ec.tile(ins[0], 20, 60) + ec.tile(dele[0], 20, 60, cls0=1) + ec.tile(ref, 20, 60, cls0=2)
    got = _hand([r, ins, dele], reads)
    (ei,), (ed,) = got[1], got[2]
    assert (ei["rb"], ei["rs"], ei["pb"], ei["ps"]) == (50, 1, 50, 4) and (ed["rb"], ed["rs"], ed["pb"], ed["ps"]) == (50, 5, 50, 1)
    assert sum(ei["alt"]) and sum(ei["ref"]) and sum(ei["other"]) and sum(ed["alt"]) and sum(ed["ref"]) and sum(ed["other"])
    # pure ones alone: an insertion at either edge of another entry's event touches it
    pure_i, pure_d = ec.entry(ref, [(50, "I", "ACG")]), ec.entry(ref, [(50, "D", 4)])
    at_edge = ec.entry(ref, [(54, "I", "TT")])
    got = _hand([r, pure_i, pure_d, at_edge], ec.tile(pure_i[0], 20, 60) + ec.tile(pure_d[0], 20, 60, cls0=1) + ec.tile(at_edge[0], 20, 60, cls0=2) + ec.tile(ref, 20, 60, cls0=3))
    assert (got[1][0]["rs"], got[1][0]["ps"]) == (0, 3) and (got[2][0]["rs"], got[2][0]["ps"]) == (4, 0)


def test_two_events_one_column_apart():
    """Two events with one '=' column between them are two events and do not touch: an entry that has only the first carries REF at the second."""
    ref = _rand(6, 120)
    both = ec.entry(ref, [(50, "X", ec._OTHER[ref[50]]), (52, "X", ec._OTHER[ref[52]])])
    first = ec.entry(ref, [(50, "X", ec._OTHER[ref[50]])])
    assert both[3] == [(50, "="), (1, "X"), (1, "="), (1, "X"), (67, "=")]
    reads = ec.tile(both[0], 20, 47) + ec.tile(first[0], 20, 47, cls0=2)
    got = _hand([ec.entry(ref, []), both, first], reads)
    e0, e1 = got[1]
    assert (e0["rb"], e1["rb"]) == (50, 52) and sum(e0["alt"]) == len(reads) and sum(e0["ref"]) == 0
    assert sum(e1["alt"]) == len(reads) // 2 and sum(e1["ref"]) == len(reads) // 2 and sum(e1["other"]) == 0


def test_alt_ref_and_other_carriers_at_one_site():
    """Three entries, one ALT, one REF, one OTHER (another base at the same place), reads cut from each."""
    ref = _rand(7, 120)
    b1 = ec._OTHER[ref[60]]
    b2 = ec._OTHER[b1]
    a1, a2, r = ec.entry(ref, [(60, "X", b1)]), ec.entry(ref, [(60, "X", b2)]), ec.entry(ref, [])
    n1, n2, nr = ec.tile(a1[0], 30, 50), ec.tile(a2[0], 30, 50, cls0=1), ec.tile(ref, 30, 50, cls0=2)
    got = _hand([a1, r, a2], n1 + n2 + nr)
    (e1,), (e2,) = got[0], got[2]
    assert (sum(e1["alt"]), sum(e1["ref"]), sum(e1["other"])) == (len(n1), len(nr), len(n2))
    assert (sum(e2["alt"]), sum(e2["ref"]), sum(e2["other"])) == (len(n2), len(nr), len(n1))


def test_two_alt_carriers_that_differ_elsewhere():
    """A read over the shared site only fits both carriers and counts alt on both; it counts nothing for the site it does not reach."""
    ref = _rand(8, 160)
    b40, b120 = ec._OTHER[ref[40]], ec._OTHER[ref[120]]
    a1, a2 = ec.entry(ref, [(40, "X", b40)]), ec.entry(ref, [(40, "X", b40), (120, "X", b120)])
    got = _hand([ec.entry(ref, []), a1, a2], [(a1[0][20:60], 0)])
    assert got[1][0]["alt"] == [1, 0, 0, 0] and got[2][0]["alt"] == [1, 0, 0, 0] and got[2][1]["alt"] + got[2][1]["ref"] + got[2][1]["other"] == [0] * 12


def test_best_holds_an_alt_and_a_ref_carrier():
    """A read with a third base at the site lies on both entries with one mismatch and is informative on both: it counts other."""
    ref, r, a = _ref_alt(9)
    third = ec._OTHER[a[0][60]] if ec._OTHER[a[0][60]] != ref[60] else ec._OTHER[ec._OTHER[a[0][60]]]
    read = ref[40:60] + third + ref[61:80]
    got = _hand([r, a], [(read, 1)])
    assert got[1][0]["other"] == [0, 1, 0, 0] and got[1][0]["alt"] + got[1][0]["ref"] == [0] * 8
    assert _hand([r, a], [(read, 1)], mm=0)[1][0]["other"] == [0] * 4


def test_offset_tie_on_a_lower_lane_of_a_later_trip():
    """pc.tie_batch's path and read: four mismatches at offset 35 (first trip, lane 60) and at offset 105 (third trip, lane 2).  With an
    event at path base 50 the read is informative only at the smaller offset."""
    _, _, ref, read = pc.tie_batch()
    e = (ref, pc.TIE_K, 0, [(50, "="), (1, "X"), (149, "=")])
    got = _hand([e], [(read, 0)])
    assert got[0][0]["alt"] == [1, 0, 0, 0]
    e = (ref, pc.TIE_K, 0, [(120, "="), (1, "X"), (79, "=")])          # ... and not at the larger one
    assert _hand([e], [(read, 0)])[0][0]["alt"] == [0] * 4


def test_offset_tie_on_an_exactly_periodic_path():
    """A path of three equal units of 64 bases: a read of 40 bases lies at offsets 0, 64 and 128 without a mismatch, all three on one lane.
    o* is the first: the read is informative for an event at path base 20 and for none at base 84 or 148."""
    unit = _rand(30, 64)
    read = unit[:40]
    for at, n in ((20, 1), (84, 0), (148, 0)):
        e = (unit * 3, K, 0, [(at, "="), (1, "X"), (191 - at, "=")])
        assert _hand([e], [(read, 2)])[0][0]["alt"] == [0, 0, n, 0]


@pytest.mark.parametrize("k", [11, 15, 35])
def test_read_lengths_on_hand_written_entries(k):
    ref, r, a = _ref_alt(10 + k, 100, 200)
    r, a = (r[0], k, 0, r[3]), (a[0], k, 0, a[3])
    reads = []
    for j, t in enumerate(sc.READ_LENS + [k, k - 1]):
        for hap, cls in ((a[0], j & 1), (ref, 2 + (j & 1))):
            s = 100 - t // 2 + (j % 3) - 1
            reads.append((hap[s:s + t], cls))
    got = _hand([r, a], reads)
    n = sum(1 for t in sc.READ_LENS + [k] if t >= max(k, 16))                     # (the shortest reads may fit elsewhere as well)
    assert sum(got[1][0]["alt"]) >= n - 1 and sum(got[1][0]["ref"]) >= n - 1 and n >= 4


def test_a_group_beyond_the_lists_is_unevaluated():
    """A group one entry beyond the entry list, and one whose events are one beyond the event list: every event UNEVALUATED, every count 0,
    the groups beside them untouched; at the capacities themselves the groups are evaluated."""
    c = hap_evid_emu.consts()
    assert (c["ents"], c["events"]) == (ec.ENTS, ec.EVENTS)
    ref = _rand(20, 200)

    def group(n_ent, n_evt_each, comp):
        return [ec.entry(ref, [(20 + 2 * j + (i % 2), "X", ec._OTHER[ref[20 + 2 * j + (i % 2)]]) for j in range(n_evt_each)], K, comp) for i in range(n_ent)]
    reads = ec.tile(ref, 0, 160, t=50, step=7) + ec.tile(group(1, 1, 0)[0][0], 0, 100, t=50, step=7, cls0=1)
    for n_ent, n_evt_each in ((ec.ENTS + 1, 1), (5, 13), (ec.ENTS, 2), (4, 16)):
        over = n_ent > ec.ENTS or n_ent * n_evt_each > ec.EVENTS
        before, after = group(2, 1, 0), group(3, 2, 2)
        got = _hand(before + group(n_ent, n_evt_each, 1) + after, reads)
        mid = got[2:2 + n_ent]
        assert all(len(g) == n_evt_each for g in mid)
        assert all((e["flags"] == ec.UNEVALUATED and e["alt"] + e["ref"] + e["other"] == [0] * 12) == over for g in mid for e in g)
        assert all(e["flags"] == 0 for g in got[:2] + got[2 + n_ent:] for e in g) and sum(sum(e["alt"]) for g in got[:2] + got[2 + n_ent:] for e in g) > 0
        alone = _hand(before, reads) + _hand(after, reads)
        assert got[:2] + got[2 + n_ent:] == alone


def test_hand_records_one_short_and_truncated_windows():
    ref = _rand(21, 120)
    ents = [ec.entry(ref, [(30 + 10 * i, "X", ec._OTHER[ref[30 + 10 * i]])]) for i in range(4)]
    reads = ec.tile(ref, 0, 80)
    full, m0 = hap_evid_emu.hand(ents, reads, 5, cap=4)
    cut, m1 = hap_evid_emu.hand(ents, reads, 5, cap=3)
    assert (m0, m1) == (0, 1) and cut[:3] == full[:3] and cut[3] == []
    none, m2 = hap_evid_emu.hand(ents, reads, 5, cap=256, len_word=0)
    assert none == [] and m2 == 0
    # a truncated window: the candidates are its whole entries
    words = lambda e: 8 + (len(e[0]) + 15) // 16 + len(e[3])
    two, _ = hap_evid_emu.hand(ents, reads, 5, len_word=(words(ents[0]) + words(ents[1])) | 0x80000000)
    assert [ec.strip(g) for g in two] == ec.model_hand(ents[:2], reads, 5)


def test_no_reads_no_entries_and_a_path_beyond_the_pool():
    ref = _rand(22, 120)
    a = ec.entry(ref, [(60, "X", ec._OTHER[ref[60]])])
    got = _hand([a], [])
    assert got[0][0]["alt"] == [0] * 4
    assert hap_evid_emu.hand([], [(ref[:40], 0)], 5) == ([], 0)
    pool = hap_evid_emu.consts()["pool"]
    long_ref = _rand(23, 16 * (pool // 2))                           # two of them do not fit the pool: the second is read in place
    ents = [ec.entry(long_ref, []), ec.entry(long_ref, [(len(long_ref) - 30, "X", ec._OTHER[long_ref[-30]])])]
    reads = ec.tile(ents[1][0], len(long_ref) - 60, len(long_ref) - 40, step=5) + ec.tile(long_ref, len(long_ref) - 60, len(long_ref) - 40, step=5, cls0=2)
    got = _hand(ents, reads)
    assert sum(got[1][0]["alt"]) == 5 and sum(got[1][0]["ref"]) == 5


# ---------------------------------------------------------------- plumbing

def test_argument_rules_and_the_struct():
    assert hap_evid_emu.lib().lancet_hapevid_emu_struct_size() == __import__("ctypes").sizeof(abi.LancetVariantEvidence) == 76
    for evid, mm in ((1 << 24, 5), (64, -1), (64, 256), (0, 256)):
        assert hap_evid_emu.set_switches(4096, evid, mm) == -1                              # LANCET_E_ARG
    assert hap_evid_emu.set_switches(4096, (1 << 24) - 1, 255) == 0 and hap_evid_emu.set_switches(4096, 0, 0) == 0
    assert hap_evid_emu.set_switches(4096, 64, 5, max_indel_len=1 << 17) == -1 and hap_evid_emu.set_switches(4096, 0, 5, max_indel_len=1 << 17) == 0
    hap_evid_emu.set_switches(0, 0, 0)


def test_join_rule():
    """lc_evid_join: the record's pos + 1 - window start - ref_off is the event's rb, and the record is one of the haplotype's."""
    assert hap_evid_emu.join(3, 2, 7, 120, 1001, 4, 1001 + 7 + 120 - 1)
    assert not hap_evid_emu.join(3, 2, 7, 120, 1001, 5, 1001 + 7 + 120 - 1)               # another haplotype's record
    assert not hap_evid_emu.join(3, 2, 7, 120, 1001, 2, 1001 + 7 + 120 - 1)
    assert not hap_evid_emu.join(3, 2, 7, 120, 1001, 4, 1001 + 7 + 120) and not hap_evid_emu.join(3, 2, 7, 120, 1001, 4, 1001 + 7 + 120 - 2)
    h = dict(window=0, first_variant=3, n_variants=2, ref_off=7)
    vs = [dict(window=0, seq=2, pos=1127), dict(window=0, seq=4, pos=1127), dict(window=1, seq=4, pos=1127)]
    assert abi.evidence_variant(h, 120, 1001, vs) == 1 and abi.evidence_variant(h, 121, 1001, vs) == -1


def test_product_library_exports_the_calls():
    from lancet_amd import build as _build, engine
    _build.build()
    L = engine.lib()
    assert L.lancet_engine_set_haplotype_evidence(None, 64, 5) == -1
    assert L.lancet_engine_results_haplotype_evidence(None, None, None, None, None) == -1
    assert L.lancet_engine_haplotype_evidence_ms(None) == 0.0 and L.lancet_engine_haplotype_evidence_readback_ms(None) == 0.0


def test_python_cli_does_not_get_the_option():
    from lancet_amd import cli
    ap = cli.build_parser()
    with pytest.raises(SystemExit):
        ap.parse_args(["--tumor", "t.bam", "--normal", "n.bam", "--ref", "r.fa", "--reg", "chr22:1-10", "--variant-evidence", "ev.tsv"])
