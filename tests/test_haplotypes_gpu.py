"""Haplotype capture on the GPU: engine.Engine(haplotype_words=...) with everything a throughput run has (LDS build kernel, graphs built
ahead, build service), the re-run tier's 512-lane kernel, and `lancet_gpu --haplotypes`, against the `p:` / `r:` lines the REFERENCE ITSELF
printed under -V (tests/golden/more_verbose/) and the run's own records (tests/hap_cases.py).  test_haplotypes_emu.py holds the emulated
kernels to the same."""
import os
import re
import shutil
import subprocess

import pytest

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


def _plain(case):
    m, batch, kept = mv.case_batch(case)
    p = mv.params(m)
    eng = engine.Engine(p, device=0)
    v, st = eng.process(batch)
    haps, trunc = eng.haplotypes()
    assert haps == [] and trunc == [0] * batch.n_windows                                # off by default
    eng.close()
    return batch, p, v, st


@pytest.mark.parametrize("case", mv.CASES)
def test_engine_haplotypes_are_the_references_path_lines(case):
    batch, p, v0, st0 = _plain(case)
    eng = engine.Engine(p, device=0, haplotype_words=hc.ample_words(batch, p))
    v, st, haps, trunc = _process(eng, batch)
    assert eng.prebuilt_count() > 0                                                     # the throughput route: LDS build kernel and all
    assert v == v0 and [hc.KEY(s) for s in st] == [hc.KEY(s) for s in st0]              # records and stats of the run without the capture
    hc.check_goldens(case, batch, st, haps, trunc)
    hc.check_link(batch, v, st, haps)
    assert _process(eng, batch) == (v, st, haps, trunc)                                 # deterministic, and the buffers start over per upload
    eng.close()


@pytest.mark.parametrize("case", mv.CASES)
def test_engine_haplotypes_through_the_rerun_tier(case, monkeypatch):
    """Tier 1's node table is too small on purpose: windows overflow there after some of their paths were written, the 512-lane kernel of the
    re-run tier starts them over in the same buffers.  Every haplotype once."""
    batch, p, v0, st0 = _plain(case)
    monkeypatch.setenv("LANCET_NODE_CAP1", "64")
    eng = engine.Engine(p, device=0, haplotype_words=hc.ample_words(batch, p))
    v, st, haps, trunc = _process(eng, batch)
    assert eng.rerun_count() > 0
    assert v == v0 and [hc.KEY(s) for s in st] == [hc.KEY(s) for s in st0]
    hc.check_goldens(case, batch, st, haps, trunc)
    hc.check_link(batch, v, st, haps)
    eng.close()


def test_engine_word_edges():
    batch, p = hc.edge_batch()
    eng = engine.Engine(p, device=0, haplotype_words=64)
    v, st, haps, trunc = _process(eng, batch)
    hc.check_edges(batch, v, st, haps, trunc)
    need = max(hc.words_of(h) for h in haps)
    eng.set_haplotypes(need)
    hc.check_edges(batch, *_process(eng, batch))
    eng.close()


def test_engine_truncation_and_state_rules():
    m, batch, kept = mv.case_batch("mv_dups")
    p = mv.params(m)
    eng = engine.Engine(p, device=0, trace_words=1 << 17, haplotype_words=hc.ample_words(batch, p))
    full = _process(eng, batch)
    text = eng.trace_text()
    w, cap = hc.truncation_plan(full[2])
    eng.set_haplotypes(cap)
    cut = _process(eng, batch)
    hc.check_truncated(batch, w, cap, full, cut)
    assert eng.trace_text() == text and all(s["status"] >= 0 for s in cut[1])
    # the rules of the call: too small for one header and one word, and not between an upload and its run
    L = eng.L
    for bad in (1, hc.HDR - 1, hc.HDR):
        assert L.lancet_engine_set_haplotypes(eng.h, bad) == -1                         # LANCET_E_ARG
    eng.upload(batch)
    assert L.lancet_engine_set_haplotypes(eng.h, 4096) == -6                            # LANCET_E_STATE
    with pytest.raises(engine.EngineError):
        eng.set_haplotypes(4096)
    eng.run()
    assert (eng.results(), eng.haplotypes()) == ((cut[0], cut[1]), (cut[2], cut[3]))     # ... and the refused calls changed nothing
    eng.set_haplotypes(0)                                                               # off again: nothing comes back
    v, st, haps, trunc = _process(eng, batch)
    assert (v, st) == (full[0], full[1]) and haps == [] and trunc == [0] * batch.n_windows
    eng.close()


def _run_bin(tmp_path, extra):
    for src, dst in ((f"{CLI_CASE}.tumor.bam", "tumor.bam"), (f"{CLI_CASE}.normal.bam", "normal.bam"), (f"{CLI_CASE}.fa", "ref.fa")):
        shutil.copy(os.path.join(mv.DIR, src), os.path.join(tmp_path, dst))
    argv = ["--tumor", "tumor.bam", "--normal", "normal.bam", "--ref", "ref.fa", "--reg", mv.meta(CLI_CASE)["region"], "--num-threads", "1"] + extra
    return subprocess.run([BIN] + argv + ["--date-line", DATE], cwd=tmp_path, capture_output=True, text=True, timeout=300), argv


def _no_date(text):
    rs = lambda l: l.rstrip() if l.startswith("##cmdline") else l                       # (the reference ends that line with a blank)
    return "".join(rs(l) + "\n" for l in text.splitlines() if not l.startswith("##fileDate"))


_HEAD = re.compile(r">(\S+?):(\d+)-(\d+)\|k=(\d+)\|comp=(\d+)\|path=(\d+)\|ref=(\d+)\+(\d+)\|variants=(\d+)\+(\d+)$")


@pytest.mark.parametrize("extra", [[], ["-V"], ["--devices", "0,0", "--batch-windows", "5"], ["--device-select"]], ids=["plain", "V", "two_engines", "device_select"])
def test_lancet_gpu_haplotypes(extra, tmp_path):
    assert mv.meta(CLI_CASE)["cli"]
    r, argv = _run_bin(str(tmp_path), extra + ["--haplotypes", "hap.fa"])
    assert r.returncode == 0, r.stderr[-2000:]
    got, want = _no_date(r.stdout), _no_date(mv.golden_vcf(CLI_CASE, full=True))
    typed = [a for a in argv[:-2] if a != "--device-select"]                             # --haplotypes FILE is left out of ##cmdline
    assert [l for l in got.splitlines() if l.startswith("##cmdline")] == ["##cmdline=lancet " + " ".join(typed)]
    if extra == ["-V"]:
        assert got == want                                                              # byte for byte the VCF of the run without the option
    body = lambda t: "".join(l + "\n" for l in t.splitlines() if not l.startswith("##cmdline"))
    assert body(got) == body(want)
    lines = open(os.path.join(str(tmp_path), "hap.fa")).read().splitlines()
    heads, seqs = lines[0::2], lines[1::2]
    r_lines, p_lines = hc.golden_lines(CLI_CASE)
    assert seqs == p_lines                                                              # one record per path, in window processing order
    at = {}
    for h, s, rl in zip(heads, seqs, r_lines):
        mt = _HEAD.match(h)
        assert mt, h
        win = mt.group(1, 2, 3)
        assert int(mt.group(6)) == at.get(win, 0) and int(mt.group(8)) == len(rl)
        at[win] = int(mt.group(6)) + 1
    assert "did not all fit" not in r.stderr and f"{len(seqs)} haplotypes written to hap.fa" in r.stderr
    if "-V" in extra:
        assert mv.digest(r.stderr) == mv.golden_trace(CLI_CASE)                         # the trace digest: unchanged


def test_lancet_gpu_haplotypes_refused_with_ranks(tmp_path):
    r, _ = _run_bin(str(tmp_path), ["--ranks", "2", "--haplotypes", "hap.fa"])
    assert r.returncode != 0 and r.stdout == "" and "--haplotypes" in r.stderr and "--ranks" in r.stderr
    assert not os.path.exists(os.path.join(str(tmp_path), "hap.fa"))                    # before any work
