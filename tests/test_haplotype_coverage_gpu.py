"""The haplotypes' per-base coverages on the GPU: engine.Engine(haplotype_words=..., haplotype_coverage=True) with everything a throughput
run has, the re-run tier's 512-lane kernel, and `lancet_gpu --haplotype-coverage`, against the tables the REFERENCE printed itself under -V
(tests/golden/hap_cov/, tests/hap_cov_cases.py) and a plain model of its Ref_t::computeCoverage.  test_haplotype_coverage_emu.py holds the
emulated kernels to the same."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import hap_align_cases as hac
import hap_cases as hc
import hap_cov_cases as hcc
import more_verbose_util as mv
import walk_cases as wc
from lancet_amd import abi, engine

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lancet_amd", "bin", "lancet_gpu")
CLI_CASE = "mv_low"
DATE = "Sun Sep 27 05:27:00 2026"
EDGE_WORDS = 2400               # ample for the edge batch: its largest entry is 8 + 33 + 3 + 2 * (513 + 512) words


def _process(eng, batch):
    v, st = eng.process(batch)
    haps, trunc = eng.haplotypes()
    return v, st, haps, trunc


def _n_cov(eng):
    op, vp, nv = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint16)(), C.c_uint32()
    assert eng.L.lancet_engine_results_haplotype_coverage(eng.h, C.byref(op), C.byref(vp), C.byref(nv)) == 0
    return nv.value, op


def _cov_engine(batch, p, words=None, aln=True):
    return engine.Engine(p, device=0, haplotype_words=words or hcc.ample_words(batch, p), haplotype_alignments=aln, haplotype_coverage=True)


@pytest.mark.parametrize("tier", ["one_tier", "rerun"])
@pytest.mark.parametrize("case", mv.CASES)
def test_engine_coverages_are_the_references_tables(case, tier, monkeypatch):
    """The default route (graphs from the LDS build kernel, windows the build service suspends while they climb through k) and the re-run
    tier: every path's table once, in the reference's order; records and stats are those of a run without the capture."""
    m, batch, kept = mv.case_batch(case)
    p = mv.params(m)
    eng = engine.Engine(p, device=0)
    v0, st0 = eng.process(batch)
    eng.close()
    if tier == "rerun":                              # tier 1's node table too small on purpose: the 512-lane kernel starts windows over
        monkeypatch.setenv("LANCET_NODE_CAP1", "64")
    eng = _cov_engine(batch, p)
    v, st, haps, trunc = _process(eng, batch)
    assert eng.prebuilt_count() > 0 and (eng.rerun_count() > 0) == (tier == "rerun")
    assert v == v0 and [hc.KEY(s) for s in st] == [hc.KEY(s) for s in st0] and not any(trunc)
    hcc.check_tables(case, batch, haps)
    hac.check_expected(batch, haps, pairs=list(zip(*hc.golden_lines(case))))
    assert _n_cov(eng)[0] == sum(4 * (h["len"] + h["ref_len"]) for h in haps)
    eng.close()


@pytest.mark.parametrize("case", mv.CASES)
def test_engine_second_run_and_switch_off(case):
    """The same engine again without the switch: the same haplotypes, no coverage word, no flag bit; every offset 0."""
    m, batch, kept = mv.case_batch(case)
    p = mv.params(m)
    eng = _cov_engine(batch, p)
    v, st, haps, trunc = _process(eng, batch)
    hcc.check_tables(case, batch, haps)
    eng.set_haplotype_coverage(False)
    v1, st1, haps1, trunc1 = _process(eng, batch)
    assert (v1, st1, haps1, trunc1) == (v, st, hcc.strip_cov(haps), trunc)
    n, off = _n_cov(eng)
    assert n == 0 and all(off[i] == 0 for i in range(len(haps1) + 1))
    hc.check_goldens(case, batch, st1, hac.strip_cigar(haps1), trunc1)
    eng.close()


def test_engine_run_again_is_the_same_run():
    """Deterministic, and the buffers start over per upload."""
    m, batch, kept = mv.case_batch("mv_dups")
    p = mv.params(m)
    eng = _cov_engine(batch, p)
    v, st, haps, trunc = _process(eng, batch)
    v2, st2, haps2, trunc2 = _process(eng, batch)
    assert (v2, st2, hcc.norm(haps2), trunc2) == (v, st, hcc.norm(haps), trunc)
    hcc.check_tables("mv_dups", batch, haps2)
    eng.close()


@pytest.mark.parametrize("case", mv.CASES)
def test_engine_no_prebuild_route(case, monkeypatch):
    """LANCET_NO_PREBUILD: every graph from the window kernel's general build."""
    monkeypatch.setenv("LANCET_NO_PREBUILD", "1")
    m, batch, kept = mv.case_batch(case)
    p = mv.params(m)
    eng = _cov_engine(batch, p)
    v, st, haps, trunc = _process(eng, batch)
    assert eng.prebuilt_count() == 0 and not any(trunc)
    hcc.check_tables(case, batch, haps)
    eng.close()


@pytest.mark.parametrize("tier", ["one_tier", "rerun"])
def test_engine_edges_of_the_pass(tier, monkeypatch):
    batch, p, names, reads = hcc.edge_batch()
    if tier == "rerun":
        monkeypatch.setenv("LANCET_NODE_CAP1", "64")
    eng = _cov_engine(batch, p, EDGE_WORDS)
    v, st, haps, trunc = _process(eng, batch)
    assert (eng.rerun_count() > 0) == (tier == "rerun")
    hcc.check_edges(batch, names, reads, v, st, haps, trunc)
    hac.check_expected(batch, haps)
    assert {h["len"] for h in haps} >= {63, 64, 65, 127, 128, 129, 511, 512, 513}
    # without the alignments: the bit, no CIGAR, the same coverages
    eng.set_haplotype_alignments(False)
    v4, st4, haps4, trunc4 = _process(eng, batch)
    assert all("cigar" not in h and h["flags"] & abi.HAP_HAS_COVERAGE for h in haps4)
    assert (v4, st4, hcc.norm(haps4), trunc4) == (v, st, hcc.norm(hac.strip_cigar(haps)), trunc)
    eng.close()


@pytest.mark.parametrize("less", [0, 1], ids=["exact_fit", "one_word_less"])
@pytest.mark.parametrize("tier", ["one_tier", "rerun"])
def test_engine_smallest_buffer_and_one_word_less(tier, less, monkeypatch):
    """The smallest buffer that holds every entry of the edge batch gives the ample run's result; one word less cuts exactly the largest."""
    batch, p, names, reads = hcc.edge_batch()
    if tier == "rerun":
        monkeypatch.setenv("LANCET_NODE_CAP1", "64")
    eng = _cov_engine(batch, p, EDGE_WORDS)
    v, st, haps, trunc = _process(eng, batch)
    need = max(hcc.words_of(h) for h in haps)
    big = [h["window"] for h in haps if hcc.words_of(h) == need]
    assert len(big) == 1 and 0 < big[0] < batch.n_windows - 1 and not any(trunc)
    eng.set_haplotypes(need - less)
    v3, st3, haps3, trunc3 = _process(eng, batch)
    assert (eng.rerun_count() > 0) == (tier == "rerun")
    assert v3 == v and [hc.KEY(s) for s in st3] == [hc.KEY(s) for s in st]
    assert trunc3 == [1 if less and w == big[0] else 0 for w in range(batch.n_windows)]
    assert hcc.norm(haps3) == hcc.norm([h for h in haps if not less or h["window"] != big[0]])
    eng.close()


@pytest.mark.parametrize("tier", ["one_tier", "rerun"])
def test_engine_entries_in_front_of_a_cut_stay_whole(tier, monkeypatch):
    m, batch, kept = mv.case_batch("mv_dups")
    p = mv.params(m)
    if tier == "rerun":
        monkeypatch.setenv("LANCET_NODE_CAP1", "64")
    eng = _cov_engine(batch, p)
    fv, fst, fh, ft = _process(eng, batch)
    assert (eng.rerun_count() > 0) == (tier == "rerun")
    hcc.check_tables("mv_dups", batch, fh)
    w = next(w for w in range(1, batch.n_windows) if sum(1 for h in fh if h["window"] == w) >= 2)
    mine = [h for h in fh if h["window"] == w]
    cap = hcc.words_of(mine[0]) + hcc.words_of(mine[1]) - 1
    eng.set_haplotypes(cap)
    cv, cst, ch, ct = _process(eng, batch)
    assert cv == fv and [hc.KEY(s) for s in cst] == [hc.KEY(s) for s in fst] and all(s["status"] >= 0 for s in cst)
    assert ct[w] == 1 and hcc.norm([h for h in ch if h["window"] == w]) == hcc.norm(mine[:1])
    for o in range(batch.n_windows):
        want, fits, n = [h for h in fh if h["window"] == o], 0, 0
        for h in want:
            if fits + hcc.words_of(h) > cap:
                break
            fits += hcc.words_of(h)
            n += 1
        assert hcc.norm([h for h in ch if h["window"] == o]) == hcc.norm(want[:n]) and ct[o] == (1 if n < len(want) else 0), o
    eng.close()


def test_engine_walk_full_redo_has_its_coverages_once():
    """walk_cases.py's many_ts (a path the wave driver gives up at WALK_FULL and the one-lane driver redoes): one set of coverages per path, the
    values those of a run without the alignments, and what the case's reads say -- 8 + 8 tumour reads, all on the changed string, 8 + 8
    normal reads, all on the reference."""
    batch, p = wc.make("many_ts")
    eng = _cov_engine(batch, p)
    v, st, haps, trunc = _process(eng, batch)
    hcc.check_shape(haps)
    assert not any(trunc) and [hac.totals(h["cigar"]) for h in haps] == list(wc.PATHS["many_ts"])
    assert _n_cov(eng)[0] == sum(4 * (h["len"] + h["ref_len"]) for h in haps)
    eng.set_haplotype_alignments(False)
    v1, st1, haps1, trunc1 = _process(eng, batch)
    assert (v1, st1, hcc.norm(haps1), trunc1) == (v, st, hcc.norm(hac.strip_cigar(haps)), trunc)
    eng.close()
    hcc.check_many_ts(haps)


def test_engine_switch_without_the_capture_and_its_arguments():
    batch, p, names, reads = hcc.edge_batch()
    eng = engine.Engine(p, device=0, haplotype_coverage=True)                            # the switch without the capture: nothing
    v, st, haps, trunc = _process(eng, batch)
    assert haps == [] and trunc == [0] * batch.n_windows and _n_cov(eng)[0] == 0
    for bad in (2, -1, 7):
        assert eng.L.lancet_engine_set_haplotype_coverage(eng.h, bad) == -1             # LANCET_E_ARG
    eng.close()


def test_engine_state_rules_of_the_switch():
    batch, p, names, reads = hcc.edge_batch()
    eng = engine.Engine(p, device=0, haplotype_words=EDGE_WORDS, haplotype_coverage=True)
    L = eng.L
    eng.upload(batch)
    assert L.lancet_engine_set_haplotype_coverage(eng.h, 0) == -6                       # LANCET_E_STATE: between an upload and its run
    with pytest.raises(engine.EngineError):
        eng.set_haplotype_coverage(False)
    eng.run()
    (v, st), (haps, trunc) = eng.results(), eng.haplotypes()
    assert all("cov" in h and "cigar" not in h for h in haps) and len(haps) == len(names)                 # the refused calls changed nothing
    hcc.check_edges(batch, names, reads, v, st, haps, trunc)
    eng.set_haplotype_coverage(False)                                                   # takes effect at the next upload
    v1, st1, haps1, trunc1 = _process(eng, batch)
    assert (v1, st1, haps1, trunc1) == (v, st, hcc.strip_cov(haps), trunc)
    eng.close()


# ---------------------------------------------------------------- lancet_gpu --haplotype-coverage

def _run_bin(tmp_path, extra):
    for src, dst in ((f"{CLI_CASE}.tumor.bam", "tumor.bam"), (f"{CLI_CASE}.normal.bam", "normal.bam"), (f"{CLI_CASE}.fa", "ref.fa")):
        shutil.copy(os.path.join(mv.DIR, src), os.path.join(tmp_path, dst))
    argv = ["--tumor", "tumor.bam", "--normal", "normal.bam", "--ref", "ref.fa", "--reg", mv.meta(CLI_CASE)["region"], "--num-threads", "1"] + extra
    return subprocess.run([BIN] + argv + ["--date-line", DATE], cwd=tmp_path, capture_output=True, text=True, timeout=300), argv


@pytest.mark.parametrize("extra", [[], ["--devices", "0,0", "--batch-windows", "5"]], ids=["plain", "two_engines"])
def test_lancet_gpu_haplotype_coverage(extra, tmp_path):
    assert mv.meta(CLI_CASE)["cli"]
    tmp = str(tmp_path)
    r0, _ = _run_bin(tmp, extra)
    r, argv = _run_bin(tmp, extra + ["--haplotypes", "hap.fa", "--haplotype-sam", "hap.sam", "--haplotype-coverage", "hap.cov"])
    assert r0.returncode == 0 and r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == r0.stdout                                                        # the VCF, ##cmdline included: byte for byte
    fa = open(os.path.join(tmp, "hap.fa")).read().splitlines()
    heads = fa[0::2]
    text = open(os.path.join(tmp, "hap.cov")).read()
    # below each header line, the reference's table for that path, byte for byte: without the header lines the file is the fixture
    lines = text.splitlines(keepends=True)
    mine = [l for l in lines if l.startswith(">")]
    assert [l.rstrip("\n") for l in mine] == [h.split("|variants=")[0] for h in heads]
    assert "".join(l for l in lines if not l.startswith(">")) == hcc.golden_text(CLI_CASE)
    assert all(lines[i + 1] == hcc.HEADER + "\n" for i, l in enumerate(lines) if l.startswith(">"))
    assert "did not all fit" not in r.stderr and f"{len(mine)} haplotypes written to hap.cov" in r.stderr
    # the SAM's four tags: SEQ's length, the table's numbers
    tabs = hcc.golden_tables(CLI_CASE)
    recs = [l.split("\t") for l in open(os.path.join(tmp, "hap.sam")).read().splitlines() if not l.startswith("@")]
    assert len(recs) == len(tabs)
    for f, tab in zip(recs, tabs):
        assert [t[:6] for t in f[-4:]] == ["nf:B:S", "nr:B:S", "tf:B:S", "tr:B:S"]
        rows = [x for x in tab if x[3] != "v"]
        for q, t in enumerate(f[-4:]):
            vals = t.split(",")[1:]
            assert len(vals) == len(f[9]) == len(rows) and vals == [x[4 + q] for x in rows]
    # alone: the same file; and the SAM without the option is what it was
    r2, _ = _run_bin(tmp, extra + ["--haplotype-coverage", "alone.cov"])
    assert r2.returncode == 0 and r2.stdout == r0.stdout and open(os.path.join(tmp, "alone.cov")).read() == text
    r3, _ = _run_bin(tmp, extra + ["--haplotype-sam", "plain.sam"])
    assert r3.returncode == 0
    plain = [l.split("\t") for l in open(os.path.join(tmp, "plain.sam")).read().splitlines() if not l.startswith("@")]
    assert all(f[-5].startswith("fl:i:") and g[-1].startswith("fl:i:") for f, g in zip(recs, plain))
    assert [g[:-1] for g in plain] == [f[:-5] for f in recs]                             # all but the flags, which say what the entry carried
    assert [int(g[-1][5:]) | abi.HAP_HAS_COVERAGE for g in plain] == [int(f[-5][5:]) for f in recs]


def test_lancet_gpu_haplotype_coverage_refused_with_ranks(tmp_path):
    r, _ = _run_bin(str(tmp_path), ["--ranks", "2", "--haplotype-coverage", "hap.cov"])
    assert r.returncode != 0 and r.stdout == "" and "--haplotype-coverage" in r.stderr and "--ranks" in r.stderr
    assert not os.path.exists(os.path.join(str(tmp_path), "hap.cov"))                   # before any work
