"""-V / --more-verbose on the GPU: the engine at trace level 2 through the binding, in tier 1 and in the re-run tier, and `lancet_gpu -V`,
against what the REFERENCE ITSELF printed under -V (tests/golden/more_verbose/, tools/make_more_verbose_goldens.py).
tests/test_more_verbose_emu.py pins the emulated kernels to the same fixtures."""
import os
import shutil
import subprocess

import pytest

import golden_util as gu
import more_verbose_util as mv
from lancet_amd import engine

pytestmark = pytest.mark.gpu

_KEY = lambda s: (s["status"], s["final_k"], s["n_builds"], s["n_variants"], s["n_kmers"], s["max_nodes"])
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lancet_amd", "bin", "lancet_gpu")
CLI_CASE = next(c for c in mv.CASES if mv.meta(c)["cli"])
DATE = "Sun Sep 27 05:27:00 2026"


def _names(batch):
    seen = {}
    for w in range(batch.n_windows):
        seen.setdefault(int(batch.chr_id[w]), batch.chrom[w])
    return [seen.get(i, "") for i in range(max(seen) + 1 if seen else 0)]


def _vcf(eng, batch, lr):
    db = engine.VariantDB()
    vp, n, blob, _ = eng.raw_results()
    if lr:
        lp, bp, _ = eng.raw_results_lr()
        db.add_raw_lr(vp, lp, n, blob + b"\0", bp, batch.bx_names, _names(batch))
    else:
        db.add_raw(vp, n, blob + b"\0", _names(batch))
    return db.vcf()


def _run_case(case, rerun):
    m, batch, kept = mv.case_batch(case)
    p = mv.params(m)
    plain = engine.Engine(p, device=0)                                              # level 0: no trace
    want = plain.process(batch)
    prebuilt = plain.prebuilt_count()
    plain.close()
    eng = engine.Engine(p, device=0, trace_words=mv.trace_words(batch, p), trace_level=2)
    got = eng.process(batch)
    assert all(s["status"] >= 0 for s in got[1]), [s for s in got[1] if s["status"] < 0][:3]
    assert mv.digest(eng.trace_text()) == mv.golden_trace(case)                     # line for line, in the reference's order
    assert "[trace truncated" not in eng.trace_text()
    assert got[0] == want[0] and [_KEY(s) for s in got[1]] == [_KEY(s) for s in want[1]]      # records and stats of the run without a trace
    assert _vcf(eng, batch, gu.case_lr(m)) == mv.golden_vcf(case)                   # ... which are the reference's
    assert eng.prebuilt_count() == 0                                                # every graph through the general build
    if rerun:
        assert eng.rerun_count() > 0
    assert eng.process(batch) == got                                                # deterministic
    eng.close()
    return prebuilt


@pytest.mark.parametrize("case", mv.CASES)
def test_engine_level2_trace_is_the_references(case):
    _run_case(case, False)


@pytest.mark.parametrize("case", mv.CASES)
def test_engine_level2_trace_through_the_rerun_tier(case, monkeypatch):
    """Tier 1's node table is too small on purpose: the 512-lane build of the same source assembles the windows and writes the events."""
    monkeypatch.setenv("LANCET_NODE_CAP1", "64")
    _run_case(case, True)


def test_level1_is_untouched_and_the_level_can_be_taken_back():
    m, batch, kept = mv.case_batch(CLI_CASE)
    p = mv.params(m)
    one = engine.Engine(p, device=0, trace_words=1 << 17)
    one.process(batch)
    t1 = one.trace_text()
    assert gu.digest_trace(t1) == mv.golden_trace(CLI_CASE, "v")                    # the reference's plain -v run of the same inputs
    assert one.prebuilt_count() > 0
    # level 2 and back on one engine: the LDS build kernel is off only while the level is set
    L = one.L
    assert L.lancet_engine_set_trace_level(one.h, mv.trace_words(batch, p), 2) == 0
    one.process(batch)
    assert one.prebuilt_count() == 0 and mv.digest(one.trace_text()) == mv.golden_trace(CLI_CASE)
    assert "".join(l + "\n" for l in one.trace_text().splitlines() if not l.startswith(mv.V_PREFIXES)) == t1
    assert L.lancet_engine_set_trace(one.h, 1 << 17) == 0
    one.process(batch)
    assert one.prebuilt_count() > 0 and one.trace_text() == t1
    assert L.lancet_engine_set_trace_level(one.h, 8, 2) == -1 and L.lancet_engine_set_trace_level(one.h, 64, 3) == -1      # LANCET_E_ARG
    one.close()


def test_engine_marks_a_window_whose_events_do_not_fit():
    m, batch, kept = mv.case_batch("mv_dups")
    p = mv.params(m)
    full = engine.Engine(p, device=0, trace_words=mv.trace_words(batch, p), trace_level=2)
    want = full.process(batch)
    text = full.trace_text()
    full.close()
    eng = engine.Engine(p, device=0, trace_words=1024, trace_level=2)
    assert eng.process(batch) == want
    cut = eng.trace_text()
    eng.close()
    marks = [l for l in cut.splitlines() if l.startswith("[trace truncated: window ")]
    assert 0 < len(marks) <= batch.n_windows and all(l.endswith(" needs more than 1024 trace words]") for l in marks)
    # what is there is the beginning of every window's text
    first = lambda t: {l.split(":")[0]: l for l in t.splitlines() if l.startswith("== Processing")}
    assert first(cut) == first(text)


def _run_bin(tmp_path, extra):
    for src, dst in ((f"{CLI_CASE}.tumor.bam", "tumor.bam"), (f"{CLI_CASE}.normal.bam", "normal.bam"), (f"{CLI_CASE}.fa", "ref.fa")):
        shutil.copy(os.path.join(mv.DIR, src), os.path.join(tmp_path, dst))
    argv = ["--tumor", "tumor.bam", "--normal", "normal.bam", "--ref", "ref.fa", "--reg", mv.meta(CLI_CASE)["region"], "--num-threads", "1"] + extra
    return subprocess.run([BIN] + argv + ["--date-line", DATE], cwd=tmp_path, capture_output=True, text=True, timeout=300), argv


def _no_date(text):
    rs = lambda l: l.rstrip() if l.startswith("##cmdline") else l                   # (the reference ends that line with a blank)
    return "".join(rs(l) + "\n" for l in text.splitlines() if not l.startswith("##fileDate"))


@pytest.mark.parametrize("extra", [["-V"], ["--more-verbose"], ["--devices", "0,0", "-V"], ["--device-select", "-V"], ["--batch-windows", "5", "-V"],
                                   ["--ranks", "1", "-V"]],
                         ids=["V", "long", "two_engines", "device_select", "small_batches", "one_rank"])
def test_lancet_gpu_more_verbose(extra, tmp_path):
    r, argv = _run_bin(str(tmp_path), extra)
    assert r.returncode == 0, r.stderr[-2000:]
    assert mv.digest(r.stderr) == mv.golden_trace(CLI_CASE)                         # stderr: the reference's -V lines, in its order
    assert "[trace truncated" not in r.stderr and "-V trace did not fit" not in r.stderr
    got, want = _no_date(r.stdout), _no_date(mv.golden_vcf(CLI_CASE, full=True))
    if extra == ["-V"]:
        assert got == want                                                          # ##cmdline and all: the flag stays as typed
    body = lambda t: "".join(l + "\n" for l in t.splitlines() if not l.startswith("##cmdline"))
    assert body(got) == body(want)
    cmd = [l for l in got.splitlines() if l.startswith("##cmdline")]
    assert cmd == ["##cmdline=lancet " + " ".join(a for a in argv if a != "--device-select")]


def test_lancet_gpu_verbose_is_what_it_was(tmp_path):
    r, argv = _run_bin(str(tmp_path), ["-v"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert gu.digest_trace(r.stderr) == mv.golden_trace(CLI_CASE, "v")              # the reference's -v run, stored beside the -V one
    assert not any(l.startswith(mv.V_PREFIXES) for l in r.stderr.splitlines())
    body = lambda t: "".join(l + "\n" for l in t.splitlines() if not l.startswith("##cmdline"))
    assert body(_no_date(r.stdout)) == body(_no_date(mv.golden_vcf(CLI_CASE, full=True)))
