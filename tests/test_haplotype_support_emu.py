"""The haplotypes' read support (lancet_engine_set_haplotype_support) without a GPU: the emulated window kernels with the capture and the
emulated support kernel behind them (tests/hap_sup_emu: lancet_amd/csrc/hap_support.h, the source the engine compiles for the device), on
the one-wave form and on the LANCET_FAT form of the window kernels.  Hand-made windows whose counts are known from how their reads were cut;
every edge of the kernel and the five more_verbose fixtures against the plain model of tests/hap_sup_cases.py.
test_haplotype_support_gpu.py holds the engine to the same."""
import ctypes
import os
import re
import sys

import pytest

import hap_cases as hc
import hap_sup_cases as sc
import more_verbose_util as mv
from lancet_amd import abi, cli

_TESTS = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_TESTS, "hap_sup_emu"))
sys.path.insert(0, os.path.join(_TESTS, "hap_cov_emu"))
import hap_sup_emu  # noqa: E402
from hap_sup_emu import emu  # noqa: E402

_ROOT = os.path.dirname(_TESTS)


@pytest.fixture
def build(request):
    emu.FAT[0] = request.param == "fat"
    yield request.param
    emu.FAT[0] = False


def _run(batch, p, words=None, sup=True, mm=5, aln=False, cov=False, evt_cap=0):
    v, st, text, haps, trunc = hap_sup_emu.run(batch, p, evt_cap=evt_cap, hap_words=sc.ample_words(batch, p) if words is None else words,
                                               aln=aln, cov=cov, sup=sup, mm=mm)
    return v, st, haps, trunc


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
@pytest.mark.parametrize("variant", ["snv", "del3"])
def test_planted_counts(variant, build):
    """One SNV / one 3-base deletion, a stated number of reads per sample and strand on either allele, reads that keep k, k - 1 and no
    bases on the window: the two paths, one group, and the numbers the reads were cut to give."""
    batch, p, alt, ref, expected = sc.basic_batch(variant)
    v, st, haps, trunc = _run(batch, p)
    sc.check_basic(variant, batch, st, haps, trunc)
    sc.check_model(batch, p, haps, 5)                              # (and the model says what the construction says)
    assert len(v) == 1


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
@pytest.mark.parametrize("k", [11, 15, 35])
def test_edges_against_the_model(k, build):
    """Read lengths on both sides of a word and of a lane trip, t == k and t == k - 1, reads longer than the path, 63 .. 129 offsets, the
    leftmost and the rightmost placement, two components, one entry, no entry, no reads; k = 11, 15 and 35."""
    batch, p, names = sc.edge_batch(k)
    v, st, haps, trunc = _run(batch, p)
    byname, want = sc.check_edges(k, batch, names, st, haps, trunc, 5)
    if k == 11:
        assert any(h["kmer"] == 11 for h in haps)
    # the reads that keep exactly k bases on an end of the paths lie there without a mismatch, and nowhere else: the model's distance at the
    # leftmost / rightmost offset, and one offset further in there is none that good
    a, b = byname["snv"]
    kk = a["kmer"]
    reads = [r for r, _ in sc.trimmed_reads(batch, p, names.index("snv"))]
    left = [r for r in reads if len(r) == 80 and r[80 - k:] == a["seq"][:k] and r[:k] != a["seq"][:k]]
    right = [r for r in reads if len(r) == 80 and r[:k] == a["seq"][-k:] and r[-k:] != a["seq"][-k:]]
    assert len(left) == 1 and len(right) == 1
    if kk == k:
        assert sc.distance(left[0], a["seq"], k) == 0 and sc.distance(right[0], a["seq"], k) == 0
        assert sc.distance(left[0][:-1], a["seq"], k) > 5 and sc.distance(right[0][1:], a["seq"], k) > 5      # (one base less on the path: no placement that good)


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
def test_mismatch_limit(build):
    """d == max_mm counts, d == max_mm + 1 does not; 0 and 255."""
    batch, p, names = sc.edge_batch(15)
    got = {}
    for mm in (0, 4, 5, 6, 255):
        v, st, haps, trunc = _run(batch, p, mm=mm)
        sc.check_model(batch, p, haps, mm)
        got[mm] = haps
    sc.check_snv_reads(names, got)
    assert [sc.strip_support(h) for h in got.values()] == [sc.strip_support(got[0])] * 5


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
@pytest.mark.parametrize("case", mv.CASES)
def test_fixtures_against_the_model(case, build):
    """Every entry of the five more_verbose cases (--linked-reads, -R and N in the reference among them); with the switch on, records,
    statistics, trace and the words / cigar / cov results are those of a run without it."""
    m, batch, kept = mv.case_batch(case)
    p = mv.params(m)
    words = sc.ample_words(batch, p) + 32 * 64 + 32 * 2 * (2 * 700 + int(p.max_indel_len) + 256)
    ec = mv.trace_words(batch, p)
    v, st, text, haps, trunc = hap_sup_emu.run(batch, p, evt_cap=ec, hap_words=words, aln=True, cov=True, sup=True)
    assert not any(trunc) and haps
    sc.check_model(batch, p, haps, 5)
    v0, st0, text0, haps0, trunc0 = hap_sup_emu.run(batch, p, evt_cap=ec, hap_words=words, aln=True, cov=True, sup=False)
    assert hap_sup_emu.LAST_NULL[0]
    import hap_cov_cases as hcc
    assert (v, st, text, trunc) == (v0, st0, text0, trunc0) and hcc.norm(sc.strip_support(haps)) == hcc.norm(haps0)
    assert all(not h["flags"] & abi.HAP_HAS_SUPPORT for h in haps0)
    if case == "mv_dups":                                           # a window that reports entries at several k
        assert any(len({h["kmer"] for h in haps if h["window"] == w}) >= 3 for w in range(batch.n_windows))
    # the switch alone: the same counts
    v1, st1, haps1, trunc1 = _run(batch, p)
    assert [h["support"] for h in haps1] == [h["support"] for h in haps]
    hc.check_goldens(case, batch, st1, sc.strip_support(haps1), trunc1)


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
def test_one_string_at_two_k(build):
    """A window that climbs after its first component was reported: the same path strings at two k, each judged in the group of its own k."""
    batch, p = sc.dups_batch()
    v, st, haps, trunc = _run(batch, p)
    assert st[0]["status"] == 0 and not any(trunc)
    sc.check_dups(batch, p, haps)


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
def test_rerun_tier_reports_the_second_tiers_entries_once(build, monkeypatch):
    """A tier 1 of 64 nodes per window: windows overflow there after some of their paths were written, the second tier starts them over in
    the same buffers; the support kernel runs behind both and counts every entry once."""
    m, batch, kept = mv.case_batch("mv_dups")
    p = mv.params(m)
    want = _run(batch, p)
    monkeypatch.setenv("LANCET_EMU_TIER1", "64")
    _, st1, _ = emu.run(batch, p)
    assert sum(1 for s in st1 if s["status"] < 0) >= 2                                      # tier 1 alone does overflow
    got = _run(batch, p)
    assert got == want
    sc.check_model(batch, p, got[2], 5)


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
def test_a_buffer_that_truncates(build):
    """A window's second entry loses its last word: the first stays whole and its counts are those among the whole entries (it is alone
    now), the window is marked, the kernel writes nothing behind the mark, no window overflows."""
    m, batch, kept = mv.case_batch("mv_nref")
    p = mv.params(m)
    fv, fst, fh, ft = _run(batch, p)
    per = {w: [h for h in fh if h["window"] == w] for w in range(1, batch.n_windows)}
    w = next(w for w, hs in per.items() if len(hs) >= 2 and (hs[0]["kmer"], hs[0]["component"]) == (hs[1]["kmer"], hs[1]["component"])
             and hs[0]["support"]["alone"] != hs[0]["support"]["fit"])      # (its first two entries are rivals that share reads)
    mine = per[w]
    cap = sc.words_of(mine[0]) + sc.words_of(mine[1]) - 1
    raws = {}
    for mm in (5, 255):
        cv, cst, ch, ct = _run(batch, p, words=cap, mm=mm)
        assert cv == fv and [hc.KEY(s) for s in cst] == [hc.KEY(s) for s in fst] and all(s["status"] >= 0 for s in cst)
        assert ct[w] == 1 and [h["index"] for h in ch if h["window"] == w] == [0]
        sc.check_model(batch, p, ch, mm)
        raws[mm] = hap_sup_emu.LAST_RAW[0]
        if mm == 5:
            (first,) = [h for h in ch if h["window"] == w]
            assert first["support"]["alone"] == first["support"]["fit"] and first["support"]["alone"] != mine[0]["support"]["alone"]
            for o in range(batch.n_windows):
                want, fits, n = [h for h in fh if h["window"] == o], 0, 0
                for h in want:
                    if fits + sc.words_of(h) > cap:
                        break
                    fits += sc.words_of(h)
                    n += 1
                assert sc.strip_support([h for h in ch if h["window"] == o]) == sc.strip_support(want[:n]) and ct[o] == (1 if n < len(want) else 0), o
    (l5, b5), (l255, b255) = raws[5], raws[255]
    assert (l5 == l255).all() and int(l5[w]) == (sc.words_of(mine[0]) | 0x80000000)
    for o in range(batch.n_windows):                                # the two runs differ in the support words of whole entries only
        used = int(l5[o]) & 0x7FFFFFFF
        assert (b5[o][used:] == b255[o][used:]).all(), o


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
def test_switch_off_leaves_the_entries_as_they_were(build):
    """Without the switch the raw buffers are those of a run of tests/hap_cov_emu, word for word -- a driver that does not know the switch,
    compiled from the same kernels (what an entry was before is held by the earlier raw-buffer tests, which are unchanged); the bit is never
    set and the results call returns NULL.  With it, an entry is the same words and eight more behind them."""
    import hap_cov_emu
    batch, p, names = sc.edge_batch(15)
    words = sc.ample_words(batch, p) + 32 * 64 + 32 * 2 * (2 * 300 + int(p.max_indel_len) + 256)
    for aln, cov in ((False, False), (True, False), (True, True)):
        v, st, haps, trunc = _run(batch, p, words=words, sup=False, aln=aln, cov=cov)
        lens, bufs = hap_sup_emu.LAST_RAW[0]
        assert hap_sup_emu.LAST_NULL[0] and all("support" not in h and not h["flags"] & abi.HAP_HAS_SUPPORT for h in haps)
        v0, st0, _, haps0, trunc0 = hap_cov_emu.run(batch, p, hap_words=words, aln=aln, cov=cov)
        lens0, bufs0 = hap_cov_emu.LAST_RAW[0]
        assert (v, st, trunc) == (v0, st0, trunc0) and len(haps) == len(haps0)
        assert (lens == lens0).all() and (bufs == bufs0).all()
        von, ston, hapson, truncon = _run(batch, p, words=words, aln=aln, cov=cov)
        lens1, bufs1 = hap_sup_emu.LAST_RAW[0]
        assert (von, ston, truncon) == (v, st, trunc)
        at = {}
        for h in hapson:
            o = at.get(h["window"], 0)
            n = sc.words_of(h)
            e, e0 = bufs1[h["window"]][o:o + n], bufs[h["window"]][o - 8 * h["index"]:o - 8 * h["index"] + n - 8]
            assert int(e[6]) == int(e0[6]) | abi.HAP_HAS_SUPPORT and (e[:6] == e0[:6]).all() and (e[7:n - 8] == e0[7:]).all()
            assert [int(x) for x in e[n - 8:]] == h["support"]["fit"] + h["support"]["alone"]
            at[h["window"]] = o + n
        assert all(int(lens1[w]) == at.get(w, 0) for w in range(batch.n_windows))
    # the switch without the capture: nothing
    v0, st0, haps0, trunc0 = _run(batch, p, words=0)
    assert haps0 == [] and hap_sup_emu.LAST_NULL[0]


def test_setter_arguments():
    for bad in ((256, 0, 0, 2, 5), (256, 0, 0, -1, 5), (256, 0, 0, 1, -1), (256, 0, 0, 1, 256), (256, 0, 0, 0, 256)):
        assert hap_sup_emu.set_switches(*bad) == -1                                       # LANCET_E_ARG
    assert hap_sup_emu.set_switches(256, 0, 0, 1, 0) == 0 and hap_sup_emu.set_switches(256, 0, 0, 1, 255) == 0
    assert hap_sup_emu.set_switches(0, 0, 0, 0, 0) == 0


def test_struct_header_and_layout():
    """lancet_haplotype keeps its 40 bytes, the header its 8 words; header, layout.h and binding agree on the flag's value."""
    assert ctypes.sizeof(abi.LancetHaplotype) == hap_sup_emu.lib().lancet_hapsup_emu_struct_size() == 40
    src = open(os.path.join(_ROOT, "include", "lancet_engine.h")).read()
    layout = open(os.path.join(_ROOT, "lancet_amd", "csrc", "layout.h")).read()
    assert int(re.search(r"#define LANCET_HAP_HAS_SUPPORT (\d+)u", src).group(1)) == abi.HAP_HAS_SUPPORT == 8
    assert hap_sup_emu.lib().lancet_hapsup_emu_flag() == 8                                  # (what the kernels were compiled with)
    assert re.search(r"uint32_t flags;\s*/\*[^*]*LANCET_HAP_HAS_SUPPORT", src)
    assert int(re.search(r"#define LANCET_HAP_HEADER_WORDS (\d+)", src).group(1)) == abi.HAP_HEADER_WORDS == 8
    assert int(re.search(r"#define LANCET_HAP_W_NCIGAR (\d+)", src).group(1)) == abi.HAP_W_NCIGAR == 7
    assert re.search(r"#define HP_HDR 8u", layout) and re.search(r"#define HP_SUP_WORDS 8u", layout) and re.search(r"uint32_t hap_sup;", layout)
    assert abi.HAP_HAS_SUPPORT & (abi.HAP_UNALIGNED | abi.HAP_IS_REF | abi.HAP_HAS_COVERAGE) == 0


def test_product_library_exports_the_calls():
    """The symbols are in liblancet_engine.so; without an engine they refuse a null handle (the state rules need a device:
    test_haplotype_support_gpu.py)."""
    from lancet_amd import build as _build, engine
    _build.build()
    L = engine.lib()
    assert L.lancet_engine_set_haplotype_support(None, 1, 5) == -1
    assert L.lancet_engine_results_haplotype_support(None, None) == -1
    assert L.lancet_engine_haplotype_support_ms(None) == 0.0


def test_python_cli_does_not_get_the_option():
    ap = cli.build_parser()
    with pytest.raises(SystemExit):
        ap.parse_args(["--tumor", "t.bam", "--normal", "n.bam", "--ref", "r.fa", "--reg", "chr22:1-10", "--haplotype-support", "h.txt"])
