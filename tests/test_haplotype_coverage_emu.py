"""The haplotypes' per-base coverages (lancet_engine_set_haplotype_coverage) without a GPU: the emulated kernels with the capture, the CIGAR
words and the coverage words (tests/hap_cov_emu: tests/emu's driver, buffers and switches handed to the kernels through the emulation's sink),
on the one-wave form and on the LANCET_FAT form, against the tables the REFERENCE printed itself under -V (tests/golden/hap_cov/, see
tests/hap_cov_cases.py) and, on hand-made windows, against a plain model of its Ref_t::computeCoverage.
test_haplotype_coverage_gpu.py holds the engine to the same."""
import ctypes
import os
import re
import sys

import pytest

import hap_align_cases as hac
import hap_cases as hc
import hap_cov_cases as hcc
import more_verbose_util as mv
import walk_cases as wc
from lancet_amd import abi, cli

_TESTS = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_TESTS, "hap_cov_emu"))
sys.path.insert(0, os.path.join(_TESTS, "hap_align_emu"))
import hap_cov_emu  # noqa: E402
from hap_cov_emu import emu  # noqa: E402

_ROOT = os.path.dirname(_TESTS)
EDGE_WORDS = 2400               # ample for the edge batch: its largest entry is 8 + 33 + 3 + 2 * (513 + 512) words


@pytest.fixture
def build(request):
    emu.FAT[0] = request.param == "fat"
    yield request.param
    emu.FAT[0] = False


def _run(batch, p, words, aln=True, cov=True, evt_cap=0):
    v, st, text, haps, trunc = hap_cov_emu.run(batch, p, evt_cap=evt_cap, hap_words=words, aln=aln, cov=cov)
    return v, st, haps, trunc


def test_the_fixtures_hold_what_they_must():
    """The generator's conditions, counted on the committed files: enough paths of each route (the thresholds of
    test_haplotype_alignments_emu.py), a stretch that starts past its window's first base, insertion and deletion columns, rows whose strands
    differ; one table per r: / p: pair of the -V trace, spelling both."""
    pairs, rows = [], {}
    for case in mv.CASES:
        r, p = hc.golden_lines(case)
        tabs = hcc.golden_tables(case)
        assert len(tabs) == len(r) == len(p)
        for a, b, t in zip(r, p, tabs):
            assert "".join(x[1] for x in t if x[1] != "-") == a and "".join(x[2] for x in t if x[2] != "-") == b
            assert all(len(x) == 12 for x in t)
        pairs += list(zip(r, p))
        rows[case] = [x for t in tabs for x in t]
        assert os.path.getsize(os.path.join(hcc.DIR, f"{case}.tables.txt.gz")) < (1 << 20)
    al, short, same = hac.route_counts(pairs)
    assert al >= 20 and short >= 20 and same >= 50, (al, short, same)
    hcc.check_set(rows)
    trims = [int(x) for case in mv.CASES for x in re.findall(r"^ref trim5: (\d+)", mv.golden_trace(case), re.M)]
    assert any(t > 0 for t in trims)


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
@pytest.mark.parametrize("route", ["default", "no_prebuild"])
@pytest.mark.parametrize("case", mv.CASES)
def test_coverages_are_the_references_tables(case, route, build, monkeypatch):
    """Every haplotype's path and reference arrays are the numbers of the reference's table for that path, the columns laid out from the
    haplotype's CIGAR; records, stats and the haplotypes' other fields are those of a run without the switch, records and stats those of
    a run without the capture."""
    m, batch, kept = mv.case_batch(case)
    p = mv.params(m)
    if route == "no_prebuild":
        monkeypatch.setenv("LANCET_NO_PREBUILD", "1")
    words = hcc.ample_words(batch, p)
    v, st, haps, trunc = _run(batch, p, words)
    assert (emu.LAST_PREBUILT[0] > 0) == (route == "default") and not any(trunc)
    hcc.check_tables(case, batch, haps)
    assert hap_cov_emu.LAST_NCOV[0] == sum(4 * (h["len"] + h["ref_len"]) for h in haps)
    hac.check_expected(batch, haps, pairs=list(zip(*hc.golden_lines(case))))
    v1, st1, haps1, trunc1 = _run(batch, p, words, cov=False)
    assert hap_cov_emu.LAST_NCOV[0] == 0
    assert (v1, st1, haps1, trunc1) == (v, st, hcc.strip_cov(haps), trunc)
    hc.check_goldens(case, batch, st1, hac.strip_cigar(haps1), trunc1)
    v0, st0, _ = emu.run(batch, p)
    assert v == v0 and [hc.KEY(s) for s in st] == [hc.KEY(s) for s in st0]


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
def test_edges_of_the_pass(build, monkeypatch):
    """Paths and stretches of 62 .. 66, 126 .. 130 and 511 .. 513 bases: every lane trip's last, first and only base, on both routes."""
    batch, p, names, reads = hcc.edge_batch()
    for route in ("default", "general"):
        if route == "general":
            monkeypatch.setenv("LANCET_NO_PREBUILD", "1")
        v, st, haps, trunc = _run(batch, p, EDGE_WORDS)
        hcc.check_edges(batch, names, reads, v, st, haps, trunc)
        assert {h["len"] for h in haps} >= {63, 64, 65, 127, 128, 129, 511, 512, 513}
        assert {h["ref_len"] for h in haps} >= {63, 64, 65, 127, 128, 129, 512, 513}
        hac.check_expected(batch, haps)


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
def test_coverage_that_does_not_fit(build):
    """The smallest buffer that holds every entry of the edge batch; one word less cuts exactly the largest: its window's length word stops
    in front of it, the window's other results and its neighbours stay whole."""
    batch, p, names, reads = hcc.edge_batch()
    v, st, haps, trunc = _run(batch, p, EDGE_WORDS)
    need = max(hcc.words_of(h) for h in haps)
    big = [h["window"] for h in haps if hcc.words_of(h) == need]
    assert len(big) == 1 and 0 < big[0] < batch.n_windows - 1
    v2, st2, haps2, trunc2 = _run(batch, p, need)
    assert (v2, st2, hcc.norm(haps2), trunc2) == (v, st, hcc.norm(haps), trunc)
    lens, bufs = hap_cov_emu.LAST_RAW[0]
    assert [int(x) for x in lens] == [hcc.words_of(h) for h in haps]
    v3, st3, haps3, trunc3 = _run(batch, p, need - 1)
    assert v3 == v and [hc.KEY(s) for s in st3] == [hc.KEY(s) for s in st]
    assert trunc3 == [1 if w == big[0] else 0 for w in range(batch.n_windows)]
    assert hcc.norm(haps3) == hcc.norm([h for h in haps if h["window"] != big[0]])
    lens, bufs = hap_cov_emu.LAST_RAW[0]
    assert int(lens[big[0]]) == 0x80000000                                               # nothing closed in front of the entry that was cut
    assert all(int(lens[h["window"]]) == hcc.words_of(h) for h in haps3)
    # a window with several paths: the entries in front of the one that does not fit stay whole
    m, batch, kept = mv.case_batch("mv_dups")
    p = mv.params(m)
    fv, fst, fh, ft = _run(batch, p, hcc.ample_words(batch, p))
    w = next(w for w in range(1, batch.n_windows) if sum(1 for h in fh if h["window"] == w) >= 2)
    mine = [h for h in fh if h["window"] == w]
    cap = hcc.words_of(mine[0]) + hcc.words_of(mine[1]) - 1
    assert cap >= hcc.words_of(mine[0]) + hac.words_of(mine[1])                          # header, path and CIGAR words of the second fit: its coverages do not
    cv, cst, ch, ct = _run(batch, p, cap)
    assert cv == fv and [hc.KEY(s) for s in cst] == [hc.KEY(s) for s in fst]
    assert ct[w] == 1 and hcc.norm([h for h in ch if h["window"] == w]) == hcc.norm(mine[:1])
    lens, bufs = hap_cov_emu.LAST_RAW[0]
    assert int(lens[w]) == (hcc.words_of(mine[0]) | 0x80000000)
    for o in range(batch.n_windows):
        want, fits, n = [h for h in fh if h["window"] == o], 0, 0
        for h in want:
            if fits + hcc.words_of(h) > cap:
                break
            fits += hcc.words_of(h)
            n += 1
        assert hcc.norm([h for h in ch if h["window"] == o]) == hcc.norm(want[:n]) and ct[o] == (1 if n < len(want) else 0), o


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
@pytest.mark.parametrize("case", ["many_ts", "ts_exact", "del70", "del40_lr", "perfect"])
def test_once_per_path_under_both_walk_drivers(case, build, monkeypatch):
    """tests/walk_cases.py's windows (many_ts: a path the wave driver gives up at WALK_FULL and the one-lane driver redoes): one entry with
    one set of coverages per path, the same under the one-lane walk driver (LANCET_OLD_WALK)."""
    batch, p = wc.make(case)
    got = {}
    for old in (False, True):
        if old:
            monkeypatch.setenv("LANCET_OLD_WALK", "1")
        v, st, haps, trunc = _run(batch, p, hcc.ample_words(batch, p))
        hc.check_shape(batch, st, hcc.strip_cov(hac.strip_cigar(haps)), trunc)
        hcc.check_shape(haps)
        lens, bufs = hap_cov_emu.LAST_RAW[0]
        assert int(lens[0]) == sum(hcc.words_of(h) for h in haps)
        got[old] = (v, hcc.norm(haps), trunc)
        if case == "many_ts":
            hcc.check_many_ts(haps)
    assert got[False] == got[True] and not any(got[False][2])
    assert [hac.totals(h["cigar"]) for h in got[False][1]] == list(wc.PATHS[case])


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
def test_rerun_tier_and_climbing_windows_report_every_entry_once(build, monkeypatch):
    """mv_dups climbs through several k per window (on the device: windows the build service suspends between them).  A tier 1 of 64 nodes
    per window: windows overflow there after some of their paths were written, the second tier starts them over in the same buffers.  Either
    way every path's table is there once, in the reference's order."""
    m, batch, kept = mv.case_batch("mv_dups")
    p = mv.params(m)
    words = hcc.ample_words(batch, p)
    want = _run(batch, p, words)
    assert len({h["kmer"] for h in want[2]}) >= 3 and max(s["n_builds"] for s in want[1]) >= 3
    monkeypatch.setenv("LANCET_EMU_TIER1", "64")
    _, st1, _ = emu.run(batch, p)
    assert sum(1 for s in st1 if s["status"] < 0) >= 2                                      # tier 1 alone does overflow
    got = _run(batch, p, words)
    assert got[0] == want[0] and [hc.KEY(s) for s in got[1]] == [hc.KEY(s) for s in want[1]]
    assert hcc.norm(got[2]) == hcc.norm(want[2]) and got[3] == want[3]
    hcc.check_tables("mv_dups", batch, got[2])


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
def test_switch_off_leaves_the_entries_as_they_were(build):
    """Without the switch the raw buffers are those of a run of tests/hap_align_emu, word for word -- a driver that does not know the switch,
    compiled from the same kernels (what an entry was before the switch existed is held by test_haplotypes_emu.py's and
    test_haplotype_alignments_emu.py's own raw-buffer tests, which are unchanged); with it and without the alignments an entry has the bit, no
    CIGAR word and the coverage words."""
    import hap_align_emu
    batch, p, names, reads = hcc.edge_batch()
    for aln in (False, True):
        v, st, haps, trunc = _run(batch, p, EDGE_WORDS, aln=aln, cov=False)
        lens, bufs = hap_cov_emu.LAST_RAW[0]
        v0, st0, _, haps0, trunc0 = hap_align_emu.run(batch, p, hap_words=EDGE_WORDS, aln=aln)
        lens0, bufs0 = hap_align_emu.LAST_RAW[0]
        assert (v, st, haps, trunc) == (v0, st0, haps0, trunc0) and all("cov" not in h and not h["flags"] & abi.HAP_HAS_COVERAGE for h in haps)
        assert (lens == lens0).all() and (bufs == bufs0).all()                             # (the unwritten words included: both drivers fill alike)
        assert hap_cov_emu.LAST_NCOV[0] == 0
    full = _run(batch, p, EDGE_WORDS)
    von, ston, hapson, truncon = _run(batch, p, EDGE_WORDS, aln=False)
    lens, bufs = hap_cov_emu.LAST_RAW[0]
    assert len(hapson) == len(names)
    for h in hapson:
        e = bufs[h["window"]]
        assert "cigar" not in h and int(e[abi.HAP_W_NCIGAR]) == 0 and int(e[6]) & abi.HAP_HAS_COVERAGE
        assert int(lens[h["window"]]) == hcc.words_of(h) == hc.words_of(h) + 2 * (h["len"] + h["ref_len"])
        first = int(e[abi.HAP_HEADER_WORDS + (h["len"] + 15) // 16])                       # the first coverage word follows the path words
        assert first == int(h["cov"]["path"][0][0]) | (int(h["cov"]["path"][0][1]) << 16)
    assert (von, ston, hcc.norm(hapson), truncon) == (full[0], full[1], hcc.norm(hac.strip_cigar(full[2])), full[3])
    # the switch without the capture: nothing
    v0, st0, haps0, trunc0 = _run(batch, p, 0, aln=True, cov=True)
    assert v0 == full[0] and haps0 == [] and hap_cov_emu.LAST_NCOV[0] == 0
    assert hap_cov_emu.set_switches(256, 0, 2) == -1 and hap_cov_emu.set_switches(256, 1, -1) == -1         # LANCET_E_ARG
    assert hap_cov_emu.set_switches(0, 0, 0) == 0


def test_struct_header_and_layout():
    """lancet_haplotype keeps its 40 bytes, the header its 8 words; header, layout.h and binding agree on the flag's value."""
    assert ctypes.sizeof(abi.LancetHaplotype) == hap_cov_emu.lib().lancet_hapcov_emu_struct_size() == 40
    src = open(os.path.join(_ROOT, "include", "lancet_engine.h")).read()
    layout = open(os.path.join(_ROOT, "lancet_amd", "csrc", "layout.h")).read()
    assert int(re.search(r"#define LANCET_HAP_HAS_COVERAGE (\d+)u", src).group(1)) == abi.HAP_HAS_COVERAGE == 4
    assert hap_cov_emu.lib().lancet_hapcov_emu_flag() == 4                                  # (what the kernels were compiled with)
    assert re.search(r"uint32_t flags;\s*/\*[^*]*LANCET_HAP_HAS_COVERAGE", src)            # (the comment of `flags` names the bit)
    assert int(re.search(r"#define LANCET_HAP_HEADER_WORDS (\d+)", src).group(1)) == abi.HAP_HEADER_WORDS == 8
    assert re.search(r"#define HP_HDR 8u", layout) and "LANCET_HAP_HAS_COVERAGE" in layout and re.search(r"uint32_t hap_cov;", layout)
    assert abi.HAP_HAS_COVERAGE & (abi.HAP_UNALIGNED | abi.HAP_IS_REF) == 0


def test_product_library_exports_the_calls():
    """The symbols are in liblancet_engine.so; without an engine both refuse a null handle (the state rules need a device:
    test_haplotype_coverage_gpu.py)."""
    from lancet_amd import build as _build, engine
    _build.build()
    L = engine.lib()
    assert L.lancet_engine_set_haplotype_coverage(None, 1) == -1
    assert L.lancet_engine_results_haplotype_coverage(None, None, None, None) == -1


def test_python_cli_does_not_get_the_option():
    ap = cli.build_parser()
    with pytest.raises(SystemExit):
        ap.parse_args(["--tumor", "t.bam", "--normal", "n.bam", "--ref", "r.fa", "--reg", "chr22:1-10", "--haplotype-coverage", "h.txt"])
