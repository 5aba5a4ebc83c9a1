"""The haplotypes' alignments on the GPU: engine.Engine(haplotype_words=..., haplotype_alignments=True) with everything a throughput run has,
the re-run tier's 512-lane kernel, and `lancet_gpu --haplotype-sam`, against the alignment the REFERENCE makes of the strings it printed
itself under -V (tests/hap_align_cases.py).  test_haplotype_alignments_emu.py holds the emulated kernels to the same."""
import os
import re
import shutil
import subprocess

import pytest

import hap_align_cases as hac
import hap_cases as hc
import more_verbose_util as mv
from lancet_amd import engine

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lancet_amd", "bin", "lancet_gpu")
CLI_CASE = "mv_low"
DATE = "Sun Sep 27 05:27:00 2026"


def _process(eng, batch):
    v, st = eng.process(batch)
    haps, trunc = eng.haplotypes()
    return v, st, haps, trunc


def _n_cigar(eng):
    import ctypes as C
    op, cp, nc = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.c_uint32()
    assert eng.L.lancet_engine_results_haplotype_alignments(eng.h, C.byref(op), C.byref(cp), C.byref(nc)) == 0
    return nc.value, op


@pytest.mark.parametrize("tier", ["one_tier", "rerun"])
@pytest.mark.parametrize("case", mv.CASES)
def test_engine_cigars_are_the_references_alignment_of_its_own_lines(case, tier, monkeypatch):
    m, batch, kept = mv.case_batch(case)
    p = mv.params(m)
    eng = engine.Engine(p, device=0)
    v0, st0 = eng.process(batch)
    eng.close()
    if tier == "rerun":                              # tier 1's node table too small on purpose: the 512-lane kernel starts windows over
        monkeypatch.setenv("LANCET_NODE_CAP1", "64")
    eng = engine.Engine(p, device=0, haplotype_words=hac.ample_words(batch, p), haplotype_alignments=True)
    v, st, haps, trunc = _process(eng, batch)
    assert eng.prebuilt_count() > 0 and (eng.rerun_count() > 0) == (tier == "rerun")
    assert v == v0 and [hc.KEY(s) for s in st] == [hc.KEY(s) for s in st0] and not any(trunc)
    hac.check_expected(batch, haps, pairs=list(zip(*hc.golden_lines(case))))
    hac.check_cigars(batch, haps, v)
    assert _n_cigar(eng)[0] == sum(len(h["cigar"]) for h in haps)
    assert _process(eng, batch) == (v, st, haps, trunc)                                 # deterministic, and the buffers start over per upload
    eng.set_haplotype_alignments(False)                                                 # the capture alone: the same haplotypes, no CIGAR word
    v1, st1, haps1, trunc1 = _process(eng, batch)
    assert (v1, st1, haps1, trunc1) == (v, st, hac.strip_cigar(haps), trunc)
    n, off = _n_cigar(eng)
    assert n == 0 and all(off[i] == 0 for i in range(len(haps1) + 1))
    hc.check_goldens(case, batch, st1, haps1, trunc1)
    eng.close()


@pytest.mark.parametrize("tier", ["one_tier", "rerun"])
def test_engine_run_encoder_edges(tier, monkeypatch):
    batch, p, names = hac.edge_batch()
    if tier == "rerun":
        monkeypatch.setenv("LANCET_NODE_CAP1", "64")
    eng = engine.Engine(p, device=0, haplotype_words=256, haplotype_alignments=True)
    v, st, haps, trunc = _process(eng, batch)
    assert (eng.rerun_count() > 0) == (tier == "rerun")
    hac.check_edges(batch, names, v, st, haps, trunc)
    need = max(hac.words_of(h) for h in haps)
    eng.set_haplotypes(need)
    assert _process(eng, batch) == (v, st, haps, trunc)
    eng.set_haplotypes(need - 1)
    v3, st3, haps3, trunc3 = _process(eng, batch)
    assert v3 == v and trunc3 == [1 if hac.words_of(h) == need else 0 for h in haps] and haps3 == [h for h in haps if hac.words_of(h) < need]
    eng.close()


@pytest.mark.parametrize("tier", ["one_tier", "rerun"])
def test_engine_cigar_that_does_not_fit(tier, monkeypatch):
    m, batch, kept = mv.case_batch("mv_dups")
    p = mv.params(m)
    if tier == "rerun":
        monkeypatch.setenv("LANCET_NODE_CAP1", "64")
    eng = engine.Engine(p, device=0, haplotype_words=hac.ample_words(batch, p), haplotype_alignments=True)
    full = _process(eng, batch)
    assert (eng.rerun_count() > 0) == (tier == "rerun")
    hac.check_expected(batch, full[2], pairs=list(zip(*hc.golden_lines("mv_dups"))))    # (the re-run tier: every CIGAR once)
    w, cap = hac.truncation_plan(full[2])
    eng.set_haplotypes(cap)
    cut = _process(eng, batch)
    hac.check_truncated(batch, w, cap, full, cut)
    assert all(s["status"] >= 0 for s in cut[1])
    eng.close()


def test_engine_state_rules_of_the_switch():
    batch, p, names = hac.edge_batch()
    eng = engine.Engine(p, device=0, haplotype_alignments=True)                          # the switch without the capture: nothing
    v, st, haps, trunc = _process(eng, batch)
    assert haps == [] and trunc == [0] * batch.n_windows and _n_cigar(eng)[0] == 0
    L = eng.L
    for bad in (2, -1, 7):
        assert L.lancet_engine_set_haplotype_alignments(eng.h, bad) == -1               # LANCET_E_ARG
    eng.set_haplotypes(256)
    eng.upload(batch)
    assert L.lancet_engine_set_haplotype_alignments(eng.h, 0) == -6                     # LANCET_E_STATE: between an upload and its run
    with pytest.raises(engine.EngineError):
        eng.set_haplotype_alignments(False)
    eng.run()
    got = (eng.results(), eng.haplotypes())
    assert got[0] == (v, st) and all("cigar" in h for h in got[1][0]) and len(got[1][0]) == len(names)      # the refused calls changed nothing
    eng.set_haplotype_alignments(False)                                                 # takes effect at the next upload
    v1, st1, haps1, trunc1 = _process(eng, batch)
    assert (v1, st1, haps1, trunc1) == (v, st, hac.strip_cigar(got[1][0]), got[1][1])
    eng.close()


# ---------------------------------------------------------------- lancet_gpu --haplotype-sam

def _run_bin(tmp_path, extra):
    for src, dst in ((f"{CLI_CASE}.tumor.bam", "tumor.bam"), (f"{CLI_CASE}.normal.bam", "normal.bam"), (f"{CLI_CASE}.fa", "ref.fa")):
        shutil.copy(os.path.join(mv.DIR, src), os.path.join(tmp_path, dst))
    argv = ["--tumor", "tumor.bam", "--normal", "normal.bam", "--ref", "ref.fa", "--reg", mv.meta(CLI_CASE)["region"], "--num-threads", "1"] + extra
    return subprocess.run([BIN] + argv + ["--date-line", DATE], cwd=tmp_path, capture_output=True, text=True, timeout=300), argv


def _fasta(path):
    seqs, name = {}, None
    for l in open(path).read().splitlines():
        if l.startswith(">"):
            name = l[1:].split()[0]
            seqs[name] = []
        else:
            seqs[name].append(l.strip())
    return {k: "".join(x) for k, x in seqs.items()}


_CIG = re.compile(r"(\d+)([=XID])")


def _check_sam(path, fasta, fa_heads, fa_seqs):
    lines = open(path).read().splitlines()
    head, recs = [l for l in lines if l.startswith("@")], [l for l in lines if not l.startswith("@")]
    assert lines[:len(head)] == head and head[0] == "@HD\tVN:1.6\tSO:unsorted"
    assert head[1:-1] == [f"@SQ\tSN:{n}\tLN:{len(s)}" for n, s in fasta.items()]
    assert head[-1].startswith("@PG\tID:lancet_gpu")
    assert len(recs) == len(fa_seqs)                                                     # one record per haplotype of the FASTA, in its order
    for l, fh, fs in zip(recs, fa_heads, fa_seqs):
        f = l.split("\t")
        qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
        tags = dict((t[:2], t[5:]) for t in f[11:])
        assert [t[:4] for t in f[11:]] == ["kk:i", "cp:i", "pi:i", "wn:Z", "vf:i", "vn:i", "fl:i"]
        assert (flag, mapq, rnext, pnext, tlen, qual) == ("0", "255", "*", "0", "0", "*") and seq == fs
        assert fh.startswith(">" + qname + "|ref=") and qname.endswith("|path=" + tags["pi"])
        assert fh == f">{tags['wn']}|k={tags['kk']}|comp={tags['cp']}|path={tags['pi']}|ref={fh.split('|ref=')[1].split('|')[0]}|variants={tags['vf']}+{tags['vn']}"
        assert rname == tags["wn"].split(":")[0]
        ops = [(int(n), op) for n, op in _CIG.findall(cigar)]
        assert "".join(f"{n}{op}" for n, op in ops) == cigar and ops
        assert ops[0][1] != "D" and ops[-1][1] != "D" and all(a[1] != b[1] for a, b in zip(ops, ops[1:]))
        # the CIGAR walked over the contig at POS gives SEQ back, '=' and 'X' truthful
        ref, i, j = fasta[rname], int(pos) - 1, 0
        for n, op in ops:
            if op == "=":
                assert ref[i:i + n].upper() == seq[j:j + n], (qname, i, j)
            elif op == "X":
                assert len(ref[i:i + n]) == n and all(a != b for a, b in zip(ref[i:i + n].upper(), seq[j:j + n])), (qname, i, j)
            i += n if op in "=XD" else 0
            j += n if op in "=XI" else 0
        assert j == len(seq)
        # ... and it is the stretch of the FASTA header it covers: ref=off+len of the window, less a D run dropped at either end
        start = int(tags["wn"].split(":")[1].split("-")[0])
        off, ln = (int(x) for x in fh.split("|ref=")[1].split("|")[0].split("+"))
        assert start + off <= int(pos) and i <= start + off - 1 + ln
        if int(tags["fl"]) & 2:
            assert ops == [(len(seq), "=")] and int(pos) == start + off
    return recs


@pytest.mark.parametrize("extra", [[], ["--devices", "0,0", "--batch-windows", "5"]], ids=["plain", "two_engines"])
def test_lancet_gpu_haplotype_sam(extra, tmp_path):
    assert mv.meta(CLI_CASE)["cli"]
    tmp = str(tmp_path)
    r0, _ = _run_bin(tmp, extra)
    r, argv = _run_bin(tmp, extra + ["--haplotypes", "hap.fa", "--haplotype-sam", "hap.sam"])
    assert r0.returncode == 0 and r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == r0.stdout                                                        # the VCF, ##cmdline included: byte for byte
    lines = open(os.path.join(tmp, "hap.fa")).read().splitlines()
    heads, seqs = lines[0::2], lines[1::2]
    assert seqs == hc.golden_lines(CLI_CASE)[1]
    recs = _check_sam(os.path.join(tmp, "hap.sam"), _fasta(os.path.join(tmp, "ref.fa")), heads, seqs)
    assert "did not all fit" not in r.stderr
    assert f"{len(seqs)} haplotypes written to hap.fa" in r.stderr and f"{len(recs)} haplotypes written to hap.sam" in r.stderr
    # alone: the same file
    r2, _ = _run_bin(tmp, extra + ["--haplotype-sam", "alone.sam"])
    assert r2.returncode == 0 and r2.stdout == r0.stdout and f"{len(recs)} haplotypes written to alone.sam" in r2.stderr
    assert open(os.path.join(tmp, "alone.sam")).read() == open(os.path.join(tmp, "hap.sam")).read()
    assert "haplotypes written to hap.fa" not in r2.stderr


def test_lancet_gpu_haplotype_sam_refused_with_ranks(tmp_path):
    r, _ = _run_bin(str(tmp_path), ["--ranks", "2", "--haplotype-sam", "hap.sam"])
    assert r.returncode != 0 and r.stdout == "" and "--haplotype-sam" in r.stderr and "--ranks" in r.stderr
    assert not os.path.exists(os.path.join(str(tmp_path), "hap.sam"))                   # before any work
