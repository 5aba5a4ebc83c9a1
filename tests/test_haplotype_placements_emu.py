"""The reads' placements (lancet_engine_set_haplotype_placements) without a GPU: the emulated window kernels with the capture and the
emulated placement kernel behind them (tests/hap_place_emu: lancet_amd/csrc/hap_place.h, the source the engine compiles for the device), on
the one-wave form and on the LANCET_FAT form of the window kernels.  Hand-made windows whose records are known from how their reads were
cut; every edge of the kernel and the five more_verbose fixtures against the plain model of tests/hap_place_cases.py; hand-written entry
buffers for the shapes no assembly produces; lc_read_cigar against abi.read_cigar and hand-written expectations.
test_haplotype_placements_gpu.py holds the engine to the same."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import hap_place_cases as pc
import hap_sup_cases as sc
import more_verbose_util as mv
from lancet_amd import abi, cli

_TESTS = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_TESTS, "hap_place_emu"))
sys.path.insert(0, os.path.join(_TESTS, "hap_sup_emu"))
import hap_place_emu  # noqa: E402
from hap_place_emu import emu  # noqa: E402

_ROOT = os.path.dirname(_TESTS)
BUILDS = pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)


@pytest.fixture
def build(request):
    emu.FAT[0] = request.param == "fat"
    yield request.param
    emu.FAT[0] = False


def _run(batch, p, words=None, mm=5, **kw):
    v, st, text, haps, trunc, pl = hap_place_emu.run(batch, p, hap_words=sc.ample_words(batch, p) if words is None else words, mm=mm, **kw)
    return v, st, haps, trunc, pl


def _rand(seed, n):
    return sc._rand(np.random.default_rng(seed), n)


# ---------------------------------------------------------------- held to the model, and to how the reads were cut

@BUILDS
@pytest.mark.parametrize("variant", ["snv", "del3"])
def test_planted_records(variant, build):
    """One SNV / one 3-base deletion: every tiled read at the position it was cut at, without a mismatch; over the site one haplotype, away
    from it two and the lower index; the reads that keep k, k - 1 and no bases on the window."""
    batch, p, alt, ref, _ = sc.basic_batch(variant)
    v, st, haps, trunc, pl = _run(batch, p)
    pc.check_basic(variant, batch, st, haps, pl)
    pc.check_model(batch, p, haps, pl, 5)


@BUILDS
@pytest.mark.parametrize("k", [11, 15, 35])
def test_edges_against_the_model(k, build):
    """sc.edge_batch: reads of k and k - 1 bases, trimmed reads, the N read, 63 .. 129 offsets, reads longer than the path, two components, no
    entry, no reads; the leftmost placement is offset k - t, the rightmost M - k."""
    batch, p, names = sc.edge_batch(k)
    v, st, haps, trunc, pl = _run(batch, p)
    assert not any(trunc)
    pc.check_model(batch, p, haps, pl, 5)
    assert pc.check_snv_ends(k, batch, p, names, haps, pl) or k == 11
    recs, rb, _ = pl
    for n in ("junk", "empty"):
        w = names.index(n)
        assert all(tuple(int(x) for x in r) == pc.NONE for r in recs[int(rb[w]):int(rb[w + 1])])
    w = names.index("short")                                        # reads longer than the path: no offset above 0
    mine = recs[int(rb[w]):int(rb[w + 1])]
    assert (mine["haplotype"] >= 0).any() and (mine["offset"][mine["haplotype"] >= 0] <= 0).all()


@BUILDS
def test_mismatch_limit(build):
    """The reads with exactly 5 and exactly 6 substitutions at limits 4 / 5 / 6; 0 and 255."""
    batch, p, names = sc.edge_batch(15)
    w = names.index("snv")
    reads = [r for r, _ in sc.trimmed_reads(batch, p, w)]
    placed = {}
    for mm in (0, 4, 5, 6, 255):
        v, st, haps, trunc, pl = _run(batch, p, mm=mm)
        pc.check_model(batch, p, haps, pl, mm)
        recs = pc.as_tuples(pl[0])[int(pl[1][w]):int(pl[1][w + 1])]
        placed[mm] = {i: r for i, r in enumerate(recs) if r[0] >= 0}
    ref = next(h["seq"] for h in haps if h["window"] == w and h["flags"] & abi.HAP_IS_REF)
    five, six = (next(i for i, r in enumerate(reads) if r == sc._sub(ref[20:100], [7 + 11 * j for j in range(n)])) for n in (5, 6))
    assert five not in placed[4] and six not in placed[4] and five in placed[5] and six not in placed[5] and five in placed[6] and six in placed[6]
    assert placed[5][five][1:3] == (20, 5) and placed[6][six][1:3] == (20, 6)
    assert set(placed[0]) <= set(placed[4]) <= set(placed[5]) <= set(placed[6]) <= set(placed[255])


@BUILDS
def test_one_string_at_two_k(build):
    """sc.dups_batch: the same string at two k counts twice in n_haplotypes, and the lower index wins."""
    batch, p = sc.dups_batch()
    v, st, haps, trunc, pl = _run(batch, p)
    pc.check_model(batch, p, haps, pl, 5)
    seqs = [h["seq"] for h in haps]
    twice = {s for s in seqs if len({h["kmer"] for h in haps if h["seq"] == s}) >= 2}
    assert len(twice) == 2
    recs = pc.as_tuples(pl[0])
    on_twice = [r for r in recs if r[0] >= 0 and seqs[r[0]] in twice]
    assert on_twice and all(r[4] >= 2 and r[0] == seqs.index(seqs[r[0]]) for r in on_twice)


@BUILDS
@pytest.mark.parametrize("case", mv.CASES)
def test_fixtures_against_the_model(case, build):
    """The five more_verbose cases, support on at the same limit: the model, the invariants that tie placements to support counts, and
    support counts, entries, records, stats and trace words identical with the placement switch on and off."""
    m, batch, kept = mv.case_batch(case)
    p = mv.params(m)
    words = sc.ample_words(batch, p) + 32 * 64
    ec = mv.trace_words(batch, p)
    on = hap_place_emu.run(batch, p, evt_cap=ec, hap_words=words, aln=True, sup=True, place=True)
    raw_on = hap_place_emu.LAST_RAW[0]
    off = hap_place_emu.run(batch, p, evt_cap=ec, hap_words=words, aln=True, sup=True, place=False)
    raw_off = hap_place_emu.LAST_RAW[0]
    assert on[:5] == off[:5] and len(off[5][0]) == 0 and on[3]
    assert (raw_on[0] == raw_off[0]).all() and (raw_on[1] == raw_off[1]).all()          # no entry word changes
    pc.check_model(batch, p, on[3], on[5], 5)
    pc.check_support_invariants(batch, on[3], on[5])
    # the switch alone, another support limit: the same records
    alone = hap_place_emu.run(batch, p, hap_words=words, place=True)
    other = hap_place_emu.run(batch, p, hap_words=words, sup=True, sup_mm=0, place=True)
    assert pc.as_tuples(alone[5][0]) == pc.as_tuples(on[5][0]) == pc.as_tuples(other[5][0])
    if case == "mv_dups":
        assert max(int(x) for x in on[5][0]["n_haplotypes"]) >= 2


@BUILDS
def test_rerun_tier_places_on_the_second_tiers_entries(build, monkeypatch):
    m, batch, kept = mv.case_batch("mv_dups")
    p = mv.params(m)
    want = _run(batch, p)
    monkeypatch.setenv("LANCET_EMU_TIER1", "64")
    got = _run(batch, p)
    assert got[:4] == want[:4] and pc.as_tuples(got[4][0]) == pc.as_tuples(want[4][0])
    pc.check_model(batch, p, got[2], got[4], 5)


@BUILDS
def test_a_buffer_that_truncates(build):
    """A window's second entry loses its last word: the candidates are the whole entries, nothing else changes."""
    m, batch, kept = mv.case_batch("mv_nref")
    p = mv.params(m)
    fv, fst, fh, ft, fpl = _run(batch, p)
    per = {w: [h for h in fh if h["window"] == w] for w in range(batch.n_windows)}
    w = next(w for w, hs in per.items() if len(hs) >= 2 and any(int(r["haplotype"]) >= 1 for r in fpl[0][int(fpl[1][w]):int(fpl[1][w + 1])]))
    cap = sc.hc.words_of(per[w][0]) + sc.hc.words_of(per[w][1]) - 1
    cv, cst, ch, ct, cpl = _run(batch, p, words=cap)
    assert ct[w] == 1 and [h["index"] for h in ch if h["window"] == w] == [0]
    pc.check_model(batch, p, ch, cpl, 5)
    mine = cpl[0][int(cpl[1][w]):int(cpl[1][w + 1])]
    assert (mine["haplotype"] <= 0).all() and (mine["n_haplotypes"] <= 1).all()


# ---------------------------------------------------------------- offset ties against lane order

@BUILDS
def test_offset_tie_on_a_lower_lane_of_a_later_trip(build):
    batch, p, ref, read = pc.tie_batch()
    v, st, haps, trunc, pl = _run(batch, p)
    pc.check_tie(batch, st, haps, pl)
    pc.check_model(batch, p, haps, pl, 5)


def _hand(entries, reads, mm=5, **kw):
    recs, tl = hap_place_emu.hand(entries, reads, mm, **kw)
    assert [int(x) for x in tl] == [len(s) for s, _ in reads]
    got = pc.as_tuples(recs)
    assert got == pc.model_hand(entries, reads, mm), (got, pc.model_hand(entries, reads, mm))
    return got


def test_offset_tie_on_an_exactly_periodic_path():
    """The same shape on a path no assembly reports: a unit of 70 bases two and a half times, a read of 40 from it: offsets 35 and 105."""
    unit = _rand(5, 70)
    path = (unit * 3)[:180]
    got = _hand([(path, 15)], [(unit[35:] + unit[:5], 0), (unit[:40], 3)])
    assert got[0] == (0, 35, 0, 2, 1, 0) and got[1] == (0, 0, 0, 3, 1, 3)


# ---------------------------------------------------------------- edges of the new code (hand-written buffers)

def test_one_more_entry_than_the_list_holds():
    """LC_PL_ENTS entries and one more, each with its own k: the read that lies only on the last one, one that ties between the last listed and
    the first unlisted, and k taken from the right entry (the unlisted entry's k admits a placement the neighbours' k does not)."""
    c = hap_place_emu.consts()
    n = c["ents"] + 1
    paths = [_rand(100 + i, 90) for i in range(n)]
    paths[n - 1] = paths[n - 2][:60] + _rand(999, 30)               # the last two share their first 60 bases
    ks = [20] * n
    ks[n - 1] = ks[5] = 12                                          # ... and the unlisted one and one of the listed ones have a smaller k
    entries = list(zip(paths, ks))
    hang = _rand(7, 30) + paths[n - 1][:14]                         # 14 bases on the last path's start: a placement at k = 12 only
    reads = [(paths[n - 1][50:90], 0), (paths[n - 1][10:50], 1), (paths[3][5:55], 2), (hang, 3), (paths[n - 2][70:], 0), (_rand(8, 30) + paths[5][:14], 1)]
    got = _hand(entries, reads)
    assert got[0][:3] == (n - 1, 50, 0) and got[1] == (n - 2, 10, 0, 1, 2, 1) and got[2][0] == 3 and got[3][:3] == (n - 1, -30, 0) and got[4][0] == n - 2
    assert got[5][:3] == (5, -30, 0)
    got = _hand(entries + [(paths[0], 20)], reads + [(paths[0][:50], 0)])      # two beyond the list; the first entry again: the lower index
    assert got[-1] == (0, 0, 0, 1, 2, 0)


@pytest.mark.parametrize("extra", [0, 1, 16])
def test_path_words_at_the_staging_boundary(extra):
    """A path of exactly LC_PL_STAGE words, one of a base more (a word past it: read in place) and one of a whole word more; reads on its last
    bases, hanging over its end and over its start."""
    c = hap_place_emu.consts()
    m = 16 * c["stage"] + extra
    path = _rand(31, m)
    reads = [(path[-50:], 0), (path[-20:] + _rand(8, 30), 1), (_rand(9, 30) + path[:20], 2), (path[m - 70:m - 20], 3), (sc._sub(path[-50:], [49, 0, 17]), 0)]
    got = _hand([(path, 15)], reads)
    assert got[0][:3] == (0, m - 50, 0) and got[1][:3] == (0, m - 20, 0) and got[2][:3] == (0, -30, 0) and got[4][:3] == (0, m - 50, 3)
    # the words beside the path read as A's: a read of A's hanging over A's on either end counts its overlap only -- 15 .. 20 bases of it on
    # the path, six offsets on either end
    path = "A" * 20 + _rand(32, m - 40) + "A" * 20
    got = _hand([(path, 15)], [("A" * 40, 0)], mm=255)
    assert got[0] == (0, -25, 0, 12, 1, 0)


@pytest.mark.parametrize("n_reads", [1, 4, 5])
def test_read_counts_around_the_waves(n_reads):
    assert hap_place_emu.consts()["waves"] == 4
    path = _rand(41, 150)
    reads = [(path[10 * i:10 * i + 60], i % 4) for i in range(n_reads)]
    got = _hand([(path, 15), (sc._sub(path, [75]), 15)], reads)
    assert [g[1] for g in got] == [10 * i for i in range(n_reads)] and [g[5] for g in got] == [i % 4 for i in range(n_reads)]
    assert [g[4] for g in got] == [2 if 10 * i > 75 or 10 * i + 60 <= 75 else 1 for i in range(n_reads)]


def test_truncated_length_word_and_no_entries():
    """HP_TRUNC in the length word: the whole entries in front of it count, the cut one does not; a buffer without entries; no reads."""
    a, b = _rand(51, 100), _rand(52, 100)
    words = 8 + 7
    reads = [(a[10:60], 0), (b[10:60], 1)]
    recs, _ = hap_place_emu.hand([(a, 15), (b, 15)], reads, cap=2 * words, len_word=words | 0x80000000)
    assert pc.as_tuples(recs) == [(0, 10, 0, 1, 1, 0), pc.NONE]
    recs, _ = hap_place_emu.hand([(a, 15), (b, 15)], reads, cap=2 * words - 1, len_word=2 * words)      # (a length word beyond the buffer: capped)
    assert pc.as_tuples(recs) == [(0, 10, 0, 1, 1, 0), pc.NONE]
    recs, _ = hap_place_emu.hand([], reads, cap=4)
    assert pc.as_tuples(recs) == [pc.NONE, pc.NONE]
    assert len(hap_place_emu.hand([(a, 15)], [])[0]) == 0


def test_both_counts_saturate():
    c = hap_place_emu.consts()
    assert c["count_max"] == pc.COUNT_MAX == abi.PLACEMENT_COUNT_MAX
    got = _hand([("A" * 300, 15)], [("A" * 20, 0)])                 # 291 offsets without a mismatch
    assert got[0] == (0, -5, 0, pc.COUNT_MAX, 1, 0)
    path = _rand(61, 60)
    got = _hand([(path, 15)] * (pc.COUNT_MAX + 3), [(path[5:45], 2)])
    assert got[0] == (0, 5, 0, 1, pc.COUNT_MAX, 2)
    got = _hand([(path, 15)] * pc.COUNT_MAX, [(path[5:45], 2)])     # exactly the largest count that is not a saturation
    assert got[0][4] == pc.COUNT_MAX


# ---------------------------------------------------------------- lc_read_cigar

CIGAR_CASES = [
    # o, t, M, ref_off, haplotype's CIGAR, expected (start, ops, has_m)
    ("inside =", 10, 50, 200, 7, [(200, "=")], (17, [(50, "M")], True)),
    ("across X", 90, 30, 200, 0, [(100, "="), (1, "X"), (99, "=")], (90, [(30, "M")], True)),
    ("starts inside I", 102, 30, 205, 0, [(100, "="), (5, "I"), (100, "=")], (100, [(3, "I"), (27, "M")], True)),
    ("ends inside I", 80, 23, 205, 0, [(100, "="), (5, "I"), (100, "=")], (80, [(20, "M"), (3, "I")], True)),
    ("spans D", 80, 40, 200, 3, [(100, "="), (6, "D"), (100, "=")], (83, [(20, "M"), (6, "D"), (20, "M")], True)),
    ("D at the start of the interval", 100, 40, 200, 0, [(100, "="), (6, "D"), (100, "=")], (106, [(40, "M")], True)),
    ("D at the end of the interval", 60, 40, 200, 0, [(100, "="), (6, "D"), (100, "=")], (60, [(40, "M")], True)),
    ("leading D of the path", 0, 40, 100, 10, [(4, "D"), (100, "=")], (14, [(40, "M")], True)),
    ("overhang left", -12, 40, 200, 0, [(200, "=")], (0, [(12, "S"), (28, "M")], True)),
    ("overhang right", 180, 40, 200, 5, [(200, "=")], (185, [(20, "M"), (20, "S")], True)),
    ("overhang both", -5, 70, 60, 2, [(30, "="), (2, "X"), (28, "=")], (2, [(5, "S"), (60, "M"), (5, "S")], True)),
    ("wholly inside I", 103, 10, 220, 0, [(100, "="), (20, "I"), (100, "=")], (100, [(10, "I")], False)),
    ("I then D then =", 98, 20, 210, 0, [(100, "="), (10, "I"), (3, "D"), (100, "=")], (98, [(2, "M"), (10, "I"), (3, "D"), (8, "M")], True)),
    ("no CIGAR words", 10, 50, 200, 7, [], (17, [(50, "M")], True)),
]


@pytest.mark.parametrize("case", CIGAR_CASES, ids=[c[0] for c in CIGAR_CASES])
def test_read_cigar(case):
    _, o, t, m, ref_off, cig, want = case
    assert hap_place_emu.read_cigar(o, t, m, ref_off, cig) == want
    assert abi.read_cigar(o, t, m, ref_off, cig) == want


def test_read_cigar_two_statements_agree_at_random():
    rng = np.random.default_rng(3)
    for _ in range(300):
        runs, m = [], 0
        for i in range(int(rng.integers(1, 7))):
            op = "=XID"[int(rng.integers(0, 4))]
            if runs and runs[-1][1] == op:
                continue
            n = int(rng.integers(1, 30))
            runs.append((n, op))
            m += n if op != "D" else 0
        if m < 20:
            continue
        t = int(rng.integers(10, 60))
        o = int(rng.integers(10 - t, m - 9))
        assert hap_place_emu.read_cigar(o, t, m, 11, runs) == abi.read_cigar(o, t, m, 11, runs), (o, t, m, runs)


@BUILDS
def test_read_cigar_on_the_planted_windows(build):
    """Through the SNV and the deletion windows: every placed read's CIGAR has the read's length, a read on the reference path is all M at
    its offset, a read over the deletion carries that D at the deletion's reference position."""
    for variant in ("snv", "del3"):
        batch, p, alt, ref, _ = sc.basic_batch(variant)
        v, st, text, haps, trunc, pl = hap_place_emu.run(batch, p, hap_words=sc.ample_words(batch, p) + 32 * 64, aln=True)
        recs, rb, tl = pl
        n_del = 0
        for r, t in zip(recs, tl):
            if int(r["haplotype"]) < 0:
                continue
            h = haps[int(r["haplotype"])]
            got = hap_place_emu.read_cigar(int(r["offset"]), int(t), h["len"], h["ref_off"], h["cigar"])
            assert got == abi.read_cigar(int(r["offset"]), int(t), h["len"], h["ref_off"], h["cigar"])
            start, ops, has_m = got
            assert has_m and sum(n for n, op in ops if op in "MIS") == int(t) and 0 <= start < len(ref)
            if h["seq"] == ref or variant == "snv":
                assert ops == [(n, op) for n, op in ((max(0, -int(r["offset"])), "S"), (min(int(t), h["len"] - int(r["offset"])) - max(0, -int(r["offset"])), "M"),
                                                     (max(0, int(r["offset"]) + int(t) - h["len"]), "S")) if n]
                assert start == max(0, int(r["offset"]))
            elif int(r["offset"]) < sc.SITE < int(r["offset"]) + int(t):
                d = [i for i, (n, op) in enumerate(ops) if op == "D"]
                assert len(d) == 1 and ops[d[0]][0] == 3
                at = start + sum(n for n, op in ops[:d[0]] if op == "M")
                # (a deletion inside a repeat may be placed anywhere in it: the reference without those three bases is the allele)
                assert ref[:at] + ref[at + 3:] == alt
                n_del += 1
        assert variant == "snv" or n_del >= 9


# ---------------------------------------------------------------- arguments, layout, exports

def test_setter_arguments():
    c = hap_place_emu.consts()
    for place, mm in ((2, 5), (-1, 5), (1, -1), (1, 256), (0, 256)):
        assert hap_place_emu.set_switches(256, place, mm) == -1                           # LANCET_E_ARG
    assert hap_place_emu.set_switches(256, 1, 0) == 0 and hap_place_emu.set_switches(256, 1, 255) == 0
    # a buffer that could hold more entries than the index field: refused with the switch, taken without
    limit = c["idx_max"] * c["min_words"]
    assert hap_place_emu.set_switches(limit + c["min_words"] - 1, 1, 5) == 0 and hap_place_emu.set_switches(limit + c["min_words"], 1, 5) == -1
    assert hap_place_emu.set_switches(limit + c["min_words"], 0, 5) == 0
    # paths that could reach 2^17 bases
    assert hap_place_emu.set_switches(256, 1, 5, max_indel_len=(1 << 17) - 1024 - 256 - 1) == 0
    assert hap_place_emu.set_switches(256, 1, 5, max_indel_len=(1 << 17) - 1024 - 256) == -1
    assert hap_place_emu.set_switches(0, 0, 0) == 0


def test_struct_and_layout():
    assert ctypes.sizeof(abi.LancetReadPlacement) == hap_place_emu.lib().lancet_happlace_emu_struct_size() == 16 == abi.PLACEMENT_DTYPE.itemsize
    src = open(os.path.join(_ROOT, "include", "lancet_engine.h")).read()
    layout = open(os.path.join(_ROOT, "lancet_amd", "csrc", "layout.h")).read()
    assert int(re.search(r"#define LANCET_PLACEMENT_COUNT_MAX (\d+)u", src).group(1)) == abi.PLACEMENT_COUNT_MAX
    bits = {n: int(re.search(rf"#define {n} (\d+)", layout).group(1)) for n in ("PL_IDX_BITS", "PL_OFF_BITS", "PL_CNT_BITS")}
    assert bits["PL_IDX_BITS"] + 8 == 32 and bits["PL_OFF_BITS"] + 2 * bits["PL_CNT_BITS"] == 32            # a record is two words: 8 bytes per read
    assert (1 << bits["PL_CNT_BITS"]) - 1 == abi.PLACEMENT_COUNT_MAX and re.search(r"#define PL_WORDS 2u", layout)
    # one statement of the mask arithmetic: the placement kernel has none of its own
    place = open(os.path.join(_ROOT, "lancet_amd", "csrc", "hap_place.h")).read()
    assert "0x55555555" not in place and "sup_mm_at<true>" in place and "atomic" not in place.split("#pragma once")[1]


def test_product_library_exports_the_calls():
    from lancet_amd import build as _build, engine
    _build.build()
    L = engine.lib()
    assert L.lancet_engine_set_haplotype_placements(None, 1, 5) == -1
    assert L.lancet_engine_results_haplotype_placements(None, None, None, None, None) == -1
    assert L.lancet_engine_haplotype_placement_ms(None) == 0.0


def test_python_cli_does_not_get_the_option():
    ap = cli.build_parser()
    with pytest.raises(SystemExit):
        ap.parse_args(["--tumor", "t.bam", "--normal", "n.bam", "--ref", "r.fa", "--reg", "chr22:1-10", "--haplotype-reads", "h.sam"])
