"""The haplotypes' alignments (lancet_engine_set_haplotype_alignments) without a GPU: the emulated kernels with the capture and the CIGAR words
(tests/hap_align_emu: tests/emu's driver, buffers and switch handed to the kernels through the emulation's sink), on the one-wave form and on
the LANCET_FAT form, against the alignment the REFERENCE makes of the strings it printed itself (tests/hap_align_cases.py) and against the
totals of its `>p_` lines.  test_haplotype_alignments_gpu.py holds the engine to the same."""
import ctypes
import os
import re
import sys

import pytest

import golden_util as gu
import hap_align_cases as hac
import hap_cases as hc
import more_verbose_util as mv
import walk_cases as wc
from lancet_amd import abi, cli

_TESTS = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_TESTS, "hap_align_emu"))
import hap_align_emu  # noqa: E402
from hap_align_emu import emu  # noqa: E402

_ROOT = os.path.dirname(_TESTS)
V_CASES = ["dups20", "knobs", "evenk", "lr30", "w1000"]


@pytest.fixture
def build(request):
    emu.FAT[0] = request.param == "fat"
    yield request.param
    emu.FAT[0] = False


def _run(batch, p, words, aln=True, evt_cap=0):
    v, st, text, haps, trunc = hap_align_emu.run(batch, p, evt_cap=evt_cap, hap_words=words, aln=aln)
    return v, st, haps, trunc


def test_the_expected_cigars_come_from_the_reference():
    """Where the reference's sources are at hand the expectation is its own align.cc, not the checker's copy of it; and the -V goldens hold
    enough paths of each of the three routes."""
    refsrc = re.search(r"^REFSRC\s*\?=\s*(\S+)", open(os.path.join(_ROOT, "oracle", "Makefile")).read(), re.M).group(1)
    if os.path.exists(os.path.dirname(refsrc)):                      # (where the build compiles oracle/_ref from)
        assert hac.oracle.ref_align_available()
    pairs = [x for case in mv.CASES for x in zip(*hc.golden_lines(case))]
    al, short, same = hac.route_counts(pairs)
    assert al >= 20 and short >= 20 and same >= 50, (al, short, same)


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
@pytest.mark.parametrize("route", ["default", "no_prebuild"])
@pytest.mark.parametrize("case", mv.CASES)
def test_cigars_are_the_references_alignment_of_its_own_lines(case, route, build, monkeypatch):
    """Every haplotype's CIGAR is the reference's alignment of the r: / p: pair it printed, in order; records, stats and the haplotypes' other
    fields are those of a capture run without alignments, records and stats those of a run without the capture."""
    m, batch, kept = mv.case_batch(case)
    p = mv.params(m)
    if route == "no_prebuild":
        monkeypatch.setenv("LANCET_NO_PREBUILD", "1")
    v, st, haps, trunc = _run(batch, p, hac.ample_words(batch, p))
    assert (emu.LAST_PREBUILT[0] > 0) == (route == "default") and not any(trunc)
    hac.check_expected(batch, haps, pairs=list(zip(*hc.golden_lines(case))))
    hac.check_cigars(batch, haps, v)
    assert hap_align_emu.LAST_NCIGAR[0] == sum(len(h["cigar"]) for h in haps)
    v1, st1, haps1, trunc1 = _run(batch, p, hac.ample_words(batch, p), aln=False)
    assert hap_align_emu.LAST_NCIGAR[0] == 0
    assert (v1, st1, haps1, trunc1) == (v, st, hac.strip_cigar(haps), trunc)
    hc.check_goldens(case, batch, st1, haps1, trunc1)
    v0, st0, _ = emu.run(batch, p)
    assert v == v0 and [hc.KEY(s) for s in st] == [hc.KEY(s) for s in st0]


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
@pytest.mark.parametrize("case", V_CASES)
def test_totals_are_the_references_path_lines(case, build):
    """match / snp / ins / del of every `>p_` line the reference printed under -v, in order per window."""
    meta, batch, kept, _ = gu.case_batch(case)
    p = gu.params(meta)
    v, st, haps, trunc = _run(batch, p, hac.ample_words(batch, p))
    assert not any(trunc)
    want = hac.golden_totals(gu.golden_trace(case))
    got = [[hac.totals(h["cigar"]) for h in haps if h["window"] == w] for w in range(batch.n_windows)]
    assert [g for g in got if g] == [t for _, t in want]
    assert sum(len(t) for _, t in want) >= 29
    hac.check_cigars(batch, haps, v)


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
@pytest.mark.parametrize("case", wc.CASES)
def test_one_cigar_per_path_under_both_walk_drivers(case, build, monkeypatch):
    """tests/walk_cases.py's hand-made windows (many_ts: a path the wave driver gives up at WALK_FULL and the one-lane driver redoes): the
    totals are wc.PATHS', the CIGARs the reference's, and the one-lane walk driver (LANCET_OLD_WALK) gives the same."""
    batch, p = wc.make(case)
    got = {}
    for old in (False, True):
        if old:
            monkeypatch.setenv("LANCET_OLD_WALK", "1")
        v, st, haps, trunc = _run(batch, p, hac.ample_words(batch, p))
        hc.check_shape(batch, st, haps, trunc)
        hac.check_cigars(batch, haps, v)
        hac.check_expected(batch, haps)
        got[old] = (v, haps, trunc)
    assert got[False] == got[True] and not any(got[False][2])
    assert [hac.totals(h["cigar"]) for h in got[False][1]] == list(wc.PATHS[case])


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
def test_run_encoder_edges(build, monkeypatch):
    """Alignments of 63 .. 129 columns, runs that cross or start at column 64, mismatches on both sides of it, and the short-cut's own runs."""
    batch, p, names = hac.edge_batch()
    for route in ("default", "general"):
        if route == "general":
            monkeypatch.setenv("LANCET_NO_PREBUILD", "1")
        v, st, haps, trunc = _run(batch, p, 256)
        hac.check_edges(batch, names, v, st, haps, trunc)
    # the smallest buffer that holds every window's one entry with its CIGAR; one word less cuts exactly the largest
    need = max(hac.words_of(h) for h in haps)
    v2, st2, haps2, trunc2 = _run(batch, p, need)
    assert (v2, haps2, trunc2) == (v, haps, trunc)
    v3, st3, haps3, trunc3 = _run(batch, p, need - 1)
    assert v3 == v and trunc3 == [1 if hac.words_of(h) == need else 0 for h in haps]
    assert haps3 == [h for h in haps if hac.words_of(h) < need]


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
def test_a_cigar_that_does_not_fit(build):
    m, batch, kept = mv.case_batch("mv_dups")
    p = mv.params(m)
    full = _run(batch, p, hac.ample_words(batch, p))
    w, cap = hac.truncation_plan(full[2])
    cut = _run(batch, p, cap)
    hac.check_truncated(batch, w, cap, full, cut)
    assert all(s["status"] >= 0 for s in cut[1])
    # the entry that was cut: header and path words were written, its CIGAR was not counted -- the length word stops in front of it
    lens, bufs = hap_align_emu.LAST_RAW[0]
    first = [h for h in full[2] if h["window"] == w][0]
    assert int(lens[w]) == (hac.words_of(first) | 0x80000000)


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
def test_rerun_tier_reports_every_cigar_once(build, monkeypatch):
    """A tier 1 of 64 nodes per window: windows overflow there after some of their paths were written, the second tier starts them over in
    the same buffers (tests/hap_align_emu/emu_hap_align.cc runs the two tiers over one set of buffers)."""
    m, batch, kept = mv.case_batch("mv_dups")
    p = mv.params(m)
    words = hac.ample_words(batch, p)
    want = _run(batch, p, words)
    monkeypatch.setenv("LANCET_EMU_TIER1", "64")
    _, st1, _ = emu.run(batch, p)
    assert sum(1 for s in st1 if s["status"] < 0) >= 2                                      # tier 1 alone does overflow
    got = _run(batch, p, words)
    assert got[0] == want[0] and [hc.KEY(s) for s in got[1]] == [hc.KEY(s) for s in want[1]] and got[2:] == want[2:]
    hac.check_expected(batch, got[2], pairs=list(zip(*hc.golden_lines("mv_dups"))))


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
def test_switch_off_leaves_the_entries_as_they_were(build):
    """Without the switch no CIGAR word comes back and word 7 of every entry in the windows' buffers is 0."""
    batch, p, names = hac.edge_batch()
    v, st, haps, trunc = _run(batch, p, 256, aln=False)
    assert hap_align_emu.LAST_NCIGAR[0] == 0 and all("cigar" not in h for h in haps) and len(haps) == len(names)
    lens, bufs = hap_align_emu.LAST_RAW[0]
    for h in haps:
        assert int(lens[h["window"]]) == hc.words_of(h) and int(bufs[h["window"]][abi.HAP_W_NCIGAR]) == 0
    von, ston, hapson, truncon = _run(batch, p, 256)
    lens, bufs = hap_align_emu.LAST_RAW[0]
    for h in hapson:
        assert int(lens[h["window"]]) == hac.words_of(h) and int(bufs[h["window"]][abi.HAP_W_NCIGAR]) == len(h["cigar"])
    assert (von, ston, hac.strip_cigar(hapson), truncon) == (v, st, haps, trunc)
    # the switch without the capture: nothing
    v0, st0, haps0, trunc0 = _run(batch, p, 0, aln=True)
    assert v0 == v and haps0 == [] and hap_align_emu.LAST_NCIGAR[0] == 0
    assert hap_align_emu.set_switches(256, 2) == -1 and hap_align_emu.set_switches(256, -1) == -1          # LANCET_E_ARG
    assert hap_align_emu.set_switches(0, 0) == 0


def test_struct_header_and_layout():
    """lancet_haplotype keeps its 40 bytes; header, layout and binding agree on the word that counts the CIGAR words and on the op codes."""
    assert ctypes.sizeof(abi.LancetHaplotype) == hap_align_emu.lib().lancet_hapaln_emu_struct_size() == 40
    src = open(os.path.join(_ROOT, "include", "lancet_engine.h")).read()
    layout = open(os.path.join(_ROOT, "lancet_amd", "csrc", "layout.h")).read()
    assert int(re.search(r"#define LANCET_HAP_W_NCIGAR (\d+)", src).group(1)) == abi.HAP_W_NCIGAR == 7
    assert "header word LANCET_HAP_W_NCIGAR" in src                                          # (the entry comment names it)
    enum = re.search(r"enum \{ HP_W_KC = 0,(.*?)\};", layout, re.S).group(1)
    names = re.findall(r"\b(HP_W_\w+)", re.sub(r"/\*.*?\*/", "", enum, flags=re.S))
    assert (["HP_W_KC"] + names).index("HP_W_NCIG") == abi.HAP_W_NCIGAR
    assert re.search(r"HP_W_NCIG \};\s*/\* = 7", layout)
    for c_name, l_name, code in (("I", "I", 1), ("D", "D", 2), ("EQ", "EQ", 7), ("X", "X", 8)):
        assert int(re.search(rf"#define LANCET_HAP_OP_{c_name} (\d+)u", src).group(1)) == code
        assert int(re.search(rf"HP_OP_{l_name} = (\d+)", layout).group(1)) == code
    assert abi.HAP_OPS == {1: "I", 2: "D", 7: "=", 8: "X"}


def test_product_library_exports_the_calls():
    """The symbols are in liblancet_engine.so; without an engine both refuse a null handle (the state rules need a device:
    test_haplotype_alignments_gpu.py)."""
    from lancet_amd import build as _build, engine
    _build.build()
    L = engine.lib()
    assert L.lancet_engine_set_haplotype_alignments(None, 1) == -1
    assert L.lancet_engine_results_haplotype_alignments(None, None, None, None) == -1


def test_python_cli_does_not_get_the_option():
    ap = cli.build_parser()
    with pytest.raises(SystemExit):
        ap.parse_args(["--tumor", "t.bam", "--normal", "n.bam", "--ref", "r.fa", "--reg", "chr22:1-10", "--haplotype-sam", "h.sam"])
