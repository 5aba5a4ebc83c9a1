"""The haplotypes' read support on the GPU: engine.Engine(haplotype_words=..., haplotype_support=True) -- the support kernel
(lancet_amd/csrc/hap_support.h) behind the window kernels and the re-run tier's 512-lane kernel -- and `lancet_gpu --haplotype-support`.
Hand-made windows whose counts are known from how their reads were cut; every edge of the kernel and the five more_verbose fixtures against
the plain model of tests/hap_sup_cases.py.  test_haplotype_support_emu.py holds the emulated kernels to the same."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import golden_util as gu
import hap_cases as hc
import hap_cov_cases as hcc
import hap_sup_cases as sc
import more_verbose_util as mv
from lancet_amd import abi, engine, host

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lancet_amd", "bin", "lancet_gpu")
CLI_CASE = "mv_low"
DATE = "Sun Sep 27 05:27:00 2026"
COLUMNS = "#haplotype\tfit_tf\tfit_tr\tfit_nf\tfit_nr\talone_tf\talone_tr\talone_nf\talone_nr"


def _process(eng, batch):
    v, st = eng.process(batch)
    haps, trunc = eng.haplotypes()
    return v, st, haps, trunc


def _engine(batch, p, words=None, mm=5, **kw):
    return engine.Engine(p, device=0, haplotype_words=words or sc.ample_words(batch, p), haplotype_support=True, haplotype_support_mismatches=mm, **kw)


def _null(eng) -> bool:
    sp = C.POINTER(C.c_uint32)()
    assert eng.L.lancet_engine_results_haplotype_support(eng.h, C.byref(sp)) == 0
    return not sp


@pytest.mark.parametrize("tier", ["one_tier", "rerun"])
@pytest.mark.parametrize("variant", ["snv", "del3"])
def test_engine_planted_counts(variant, tier, monkeypatch):
    """The two paths, one group, and the numbers the reads were cut to give -- from the window kernel and from the re-run tier's."""
    batch, p, alt, ref, expected = sc.basic_batch(variant)
    if tier == "rerun":
        monkeypatch.setenv("LANCET_NODE_CAP1", "64")
    eng = _engine(batch, p)
    v, st, haps, trunc = _process(eng, batch)
    assert (eng.rerun_count() > 0) == (tier == "rerun") and eng.haplotype_support_ms() > 0
    sc.check_basic(variant, batch, st, haps, trunc)
    eng.close()


@pytest.mark.parametrize("k", [11, 15, 35])
def test_engine_edges_against_the_model(k):
    batch, p, names = sc.edge_batch(k)
    eng = _engine(batch, p)
    v, st, haps, trunc = _process(eng, batch)
    sc.check_edges(k, batch, names, st, haps, trunc, 5)
    eng.close()


def test_engine_mismatch_limit_and_second_runs():
    """d == max_mm counts, d == max_mm + 1 does not; 0 and 255; the same engine, one upload after the other, and a run repeated."""
    batch, p, names = sc.edge_batch(15)
    eng = _engine(batch, p)
    got = {}
    for mm in (0, 4, 5, 6, 255):
        eng.set_haplotype_support(True, mm)
        v, st, haps, trunc = _process(eng, batch)
        sc.check_model(batch, p, haps, mm)
        got[mm] = haps
    sc.check_snv_reads(names, got)
    eng.run()                                                       # again without an upload: the window kernels clear the words they reserve
    assert eng.haplotypes()[0] == got[255]
    eng.close()


@pytest.mark.parametrize("tier", ["one_tier", "rerun"])
@pytest.mark.parametrize("case", mv.CASES)
def test_engine_fixtures_against_the_model(case, tier, monkeypatch):
    """Every entry of the five more_verbose cases; records, statistics, trace and the words / cigar / cov results are those of a run without
    the switch; re-run windows report the second tier's entries with their counts, once."""
    m, batch, kept = mv.case_batch(case)
    p = mv.params(m)
    words = hcc.ample_words(batch, p) + 32 * 8
    ec = mv.trace_words(batch, p)
    kw = dict(device=0, trace_words=ec, trace_level=2, haplotype_words=words, haplotype_alignments=True, haplotype_coverage=True)
    if tier == "rerun":
        monkeypatch.setenv("LANCET_NODE_CAP1", "64")
    eng = engine.Engine(p, **kw)
    v0, st0, haps0, trunc0 = _process(eng, batch)
    text0 = eng.trace_text()
    assert _null(eng) and eng.haplotype_support_ms() == 0 and all(not h["flags"] & abi.HAP_HAS_SUPPORT for h in haps0)
    eng.close()
    eng = engine.Engine(p, haplotype_support=True, **kw)
    v, st, haps, trunc = _process(eng, batch)
    assert not any(trunc) and (eng.rerun_count() > 0) == (tier == "rerun") and eng.haplotype_support_ms() > 0
    assert (v, st, trunc) == (v0, st0, trunc0) and eng.trace_text() == text0
    assert hcc.norm(sc.strip_support(haps)) == hcc.norm(haps0)
    sc.check_model(batch, p, haps, 5)
    eng.close()


def test_engine_one_string_at_two_k():
    batch, p = sc.dups_batch()
    eng = _engine(batch, p)
    v, st, haps, trunc = _process(eng, batch)
    assert st[0]["status"] == 0 and not any(trunc)
    sc.check_dups(batch, p, haps)
    eng.close()


@pytest.mark.parametrize("tier", ["one_tier", "rerun"])
def test_engine_a_buffer_that_truncates(tier, monkeypatch):
    """The first entry of a window whose second is cut is counted among the whole entries -- alone; marked, no overflow, every whole entry
    against the model."""
    m, batch, kept = mv.case_batch("mv_nref")
    p = mv.params(m)
    if tier == "rerun":
        monkeypatch.setenv("LANCET_NODE_CAP1", "64")
    eng = _engine(batch, p)
    fv, fst, fh, ft = _process(eng, batch)
    per = {w: [h for h in fh if h["window"] == w] for w in range(1, batch.n_windows)}
    w = next(w for w, hs in per.items() if len(hs) >= 2 and (hs[0]["kmer"], hs[0]["component"]) == (hs[1]["kmer"], hs[1]["component"])
             and hs[0]["support"]["alone"] != hs[0]["support"]["fit"])
    cap = sc.words_of(per[w][0]) + sc.words_of(per[w][1]) - 1
    eng.set_haplotypes(cap)
    cv, cst, ch, ct = _process(eng, batch)
    assert cv == fv and [hc.KEY(s) for s in cst] == [hc.KEY(s) for s in fst] and all(s["status"] >= 0 for s in cst)
    (first,) = [h for h in ch if h["window"] == w]
    assert ct[w] == 1 and first["support"]["alone"] == first["support"]["fit"]
    sc.check_model(batch, p, ch, 5)
    for o in range(batch.n_windows):
        want, fits, n = [h for h in fh if h["window"] == o], 0, 0
        for h in want:
            if fits + sc.words_of(h) > cap:
                break
            fits += sc.words_of(h)
            n += 1
        assert sc.strip_support([h for h in ch if h["window"] == o]) == sc.strip_support(want[:n]) and ct[o] == (1 if n < len(want) else 0), o
    eng.close()


def test_engine_reads_stored_once():
    """lancet_engine_upload_packed with read_index (a read of several windows is stored once): the counts of the plain upload, and the model's."""
    G = gu.GOLDEN
    paths = [os.path.join(G, f"ar_small.{x}") for x in ("tumor.bam", "normal.bam", "fa")]
    p = abi.default_params()
    o = host.default_opts(active_region=0, min_qual_call=p.min_qual_call)
    H = host.NativeHost(*paths)
    hdrs = H.tile("chr22:900-3100", o)
    b, idx = H.batch(0, len(hdrs), o)
    b2, idx2, pk = H.batch(0, len(hdrs), o, pack_params=p)
    H.close()
    assert "read_index" in pk and pk["n_distinct"] < b.n_reads
    eng = _engine(b, p)
    v, st, haps, trunc = _process(eng, b)
    assert haps and not any(trunc)
    sc.check_model(b, p, haps, 5)
    eng.upload_packed(b2, pk)
    eng.run()
    assert eng.results() == (v, st) and eng.haplotypes() == (haps, trunc)
    eng.close()


def test_engine_switch_off_without_capture_and_arguments():
    batch, p, names = sc.edge_batch(15)
    eng = engine.Engine(p, device=0, haplotype_support=True)                             # the switch without the capture: nothing
    v, st, haps, trunc = _process(eng, batch)
    assert haps == [] and trunc == [0] * batch.n_windows and _null(eng) and eng.haplotype_support_ms() == 0
    for on, mm in ((2, 5), (-1, 5), (1, -1), (1, 256), (0, 256)):
        assert eng.L.lancet_engine_set_haplotype_support(eng.h, on, mm) == -1           # LANCET_E_ARG
    eng.close()
    # off: the dense words are those of an engine that was never told of the switch; the bit is never set; NULL
    a = engine.Engine(p, device=0, haplotype_words=sc.ample_words(batch, p))
    b = _engine(batch, p)
    b.set_haplotype_support(False, 5)
    ra, rb = _process(a, batch), _process(b, batch)
    assert ra == rb and _null(a) and _null(b) and all(not h["flags"] & abi.HAP_HAS_SUPPORT and "support" not in h for h in rb[2])
    a.close()
    b.close()


def test_engine_state_rules_of_the_switch():
    batch, p, names = sc.edge_batch(15)
    eng = _engine(batch, p)
    L = eng.L
    eng.upload(batch)
    assert L.lancet_engine_set_haplotype_support(eng.h, 0, 5) == -6                     # LANCET_E_STATE: between an upload and its run
    with pytest.raises(engine.EngineError):
        eng.set_haplotype_support(False)
    eng.run()
    (v, st), (haps, trunc) = eng.results(), eng.haplotypes()
    sc.check_model(batch, p, haps, 5)                                                   # the refused calls changed nothing
    eng.set_haplotype_support(False)                                                    # takes effect at the next upload
    v1, st1, haps1, trunc1 = _process(eng, batch)
    assert (v1, st1, haps1, trunc1) == (v, st, sc.strip_support(haps), trunc) and _null(eng)
    eng.close()


# ---------------------------------------------------------------- lancet_gpu --haplotype-support

def _run_bin(tmp_path, extra):
    for src, dst in ((f"{CLI_CASE}.tumor.bam", "tumor.bam"), (f"{CLI_CASE}.normal.bam", "normal.bam"), (f"{CLI_CASE}.fa", "ref.fa")):
        shutil.copy(os.path.join(mv.DIR, src), os.path.join(tmp_path, dst))
    argv = ["--tumor", "tumor.bam", "--normal", "normal.bam", "--ref", "ref.fa", "--reg", mv.meta(CLI_CASE)["region"], "--num-threads", "1"] + extra
    return subprocess.run([BIN] + argv + ["--date-line", DATE], cwd=tmp_path, capture_output=True, text=True, timeout=300), argv


def test_lancet_gpu_haplotype_support(tmp_path):
    assert mv.meta(CLI_CASE)["cli"]
    tmp = str(tmp_path)
    r0, _ = _run_bin(tmp, [])
    r, argv = _run_bin(tmp, ["--haplotypes", "hap.fa", "--haplotype-sam", "hap.sam", "--haplotype-support", "hap.sup", "--haplotype-support-mismatches", "5"])
    assert r0.returncode == 0 and r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == r0.stdout                                                        # the VCF, ##cmdline included: byte for byte
    assert "haplotype-support" not in r.stdout
    heads = open(os.path.join(tmp, "hap.fa")).read().splitlines()[0::2]
    text = open(os.path.join(tmp, "hap.sup")).read()
    lines = text.splitlines()
    assert lines[0] == COLUMNS and len(lines) == len(heads) + 1                         # one line per haplotype, and the column names
    assert [l.split("\t")[0] for l in lines[1:]] == [h[1:].split("|variants=")[0] for h in heads]
    rows = [[int(x) for x in l.split("\t")[1:]] for l in lines[1:]]
    assert all(len(x) == 8 and all(a <= f for a, f in zip(x[4:], x[:4])) for x in rows) and any(sum(x[:4]) > 0 for x in rows)
    assert "did not all fit" not in r.stderr and f"{len(rows)} haplotypes written to hap.sup" in r.stderr
    # the numbers are the engine's for the same windows (and so the model's: test_engine_fixtures_against_the_model)
    m, batch, kept = mv.case_batch(CLI_CASE)
    p = mv.params(m)
    eng = _engine(batch, p)
    v, st, haps, trunc = _process(eng, batch)
    eng.close()
    assert rows == [h["support"]["fit"] + h["support"]["alone"] for h in haps]
    # the SAM's two tags, exactly when both files are asked for
    recs = [l.split("\t") for l in open(os.path.join(tmp, "hap.sam")).read().splitlines() if not l.startswith("@")]
    assert len(recs) == len(rows)
    for f, x in zip(recs, rows):
        assert f[-2] == "sf:B:I," + ",".join(map(str, x[:4])) and f[-1] == "sa:B:I," + ",".join(map(str, x[4:]))
    r3, _ = _run_bin(tmp, ["--haplotype-sam", "plain.sam"])
    plain = open(os.path.join(tmp, "plain.sam")).read()
    assert r3.returncode == 0 and "sf:B:I" not in plain and "sa:B:I" not in plain
    # alone, another limit, and the device read selection: the same file where the limit is the same
    r2, _ = _run_bin(tmp, ["--haplotype-support", "alone.sup"])
    assert r2.returncode == 0 and r2.stdout == r0.stdout and open(os.path.join(tmp, "alone.sup")).read() == text
    r4, _ = _run_bin(tmp, ["--device-select", "--haplotype-support", "select.sup"])
    assert r4.returncode == 0 and r4.stdout == r0.stdout and open(os.path.join(tmp, "select.sup")).read() == text
    r5, _ = _run_bin(tmp, ["--haplotype-support", "zero.sup", "--haplotype-support-mismatches", "0"])
    zero = [[int(x) for x in l.split("\t")[1:]] for l in open(os.path.join(tmp, "zero.sup")).read().splitlines()[1:]]
    assert r5.returncode == 0 and r5.stdout == r0.stdout and len(zero) == len(rows) and zero != rows
    assert all(a <= b for x, y in zip(zero, rows) for a, b in zip(x[:4], y[:4]))


def test_lancet_gpu_haplotype_support_refusals(tmp_path):
    r, _ = _run_bin(str(tmp_path), ["--ranks", "2", "--haplotype-support", "hap.sup"])
    assert r.returncode != 0 and r.stdout == "" and "--haplotype-support" in r.stderr and "--ranks" in r.stderr
    assert not os.path.exists(os.path.join(str(tmp_path), "hap.sup"))                   # before any work
    r, _ = _run_bin(str(tmp_path), ["--haplotype-support", "hap.sup", "--haplotype-support-mismatches", "256"])
    assert r.returncode != 0 and "--haplotype-support-mismatches" in r.stderr
