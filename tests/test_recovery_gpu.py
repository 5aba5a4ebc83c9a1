"""-R / --kmer-recovery on the GPU: the engine through the C-ABI and the command-line program against what the REFERENCE ITSELF wrote
with and without the option (tests/golden/recovery/, tools/make_recovery_goldens.py).  Records and per-window statistics are also
compared with the emulated kernels', which tests/test_recovery_emu.py pins to the same fixtures."""
import io
import os
import shutil
import subprocess
import sys

import pytest

import golden_util as gu
import recovery_util as ru
from lancet_amd import cli, engine

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402

pytestmark = pytest.mark.gpu

_KEY = lambda s: (s["status"], s["final_k"], s["n_builds"], s["n_variants"], s["n_kmers"], s["max_nodes"])
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lancet_amd", "bin", "lancet_gpu")
CLI_CASE = "rec_low"
DATE = "Sun Sep 27 05:27:00 2026"


def _names(batch):
    names, seen = [], {}
    for w in range(batch.n_windows):
        seen.setdefault(int(batch.chr_id[w]), batch.chrom[w])
    for i in range(max(seen) + 1 if seen else 0):
        names.append(seen.get(i, ""))
    return names


def _check(case, recovery, eng, batch, variants, stats, trace=True):
    ev, est, _ = emu.run(batch, ru.params(ru.meta(case), recovery))
    assert all(s["status"] >= 0 for s in stats), [s for s in stats if s["status"] < 0][:3]
    assert variants == ev
    assert [_KEY(s) for s in stats] == [_KEY(s) for s in est]
    if trace:
        assert gu.digest_trace(eng.trace_text()) == ru.golden_trace(case, recovery)
    db = engine.VariantDB()
    vp, n, blob, _ = eng.raw_results()
    db.add_raw(vp, n, blob + b"\0", _names(batch))
    assert db.vcf() == ru.golden_vcf(case, recovery)                               # byte-identical to the reference's


@pytest.mark.parametrize("recovery", [True, False], ids=["R", "noR"])
@pytest.mark.parametrize("case", ru.CASES)
def test_engine_reproduces_the_reference_with_and_without_recovery(case, recovery):
    m, batch, kept = ru.case_batch(case)
    eng = engine.Engine(ru.params(m, recovery), device=0, trace_words=1 << 17)
    first = eng.process(batch)
    _check(case, recovery, eng, batch, *first)
    assert eng.process(batch) == first                                              # deterministic
    eng.close()


@pytest.mark.parametrize("case", ru.CASES)
def test_recovery_through_the_rerun_tier(case, monkeypatch):
    """Tier 1's small tables overflow on purpose (as tests/test_engine_gpu.py forces it): the 512-lane build of the same source assembles the windows."""
    monkeypatch.setenv("LANCET_NODE_CAP1", "256")
    m, batch, kept = ru.case_batch(case)
    eng = engine.Engine(ru.params(m, True), device=0, trace_words=1 << 17)
    variants, stats = eng.process(batch)
    assert eng.rerun_count() > 0
    _check(case, True, eng, batch, variants, stats)
    eng.close()


@pytest.mark.parametrize("case", ru.CASES)
def test_recovery_does_not_depend_on_who_builds_a_graph(case, monkeypatch):
    """Build service on (default), with more workgroups, off, nothing built ahead, no LDS build at all: the same records."""
    m, batch, kept = ru.case_batch(case)
    for env in ({}, {"LANCET_SVC_WGS": "64"}, {"LANCET_NO_SVC": "1"}, {"LANCET_AHEAD_DEPTH": "0", "LANCET_SVC_DEPTH": "0"}, {"LANCET_NO_PREBUILD": "1"}):
        for k_, v_ in env.items():
            monkeypatch.setenv(k_, v_)
        eng = engine.Engine(ru.params(m, True), device=0, trace_words=1 << 17)
        variants, stats = eng.process(batch)
        _check(case, True, eng, batch, variants, stats)
        eng.close()
        for k_ in env:
            monkeypatch.delenv(k_)


def test_route_counters_are_equal_with_the_flag_on_and_off():
    for case in ru.CASES:
        m, batch, kept = ru.case_batch(case)
        routes = []
        for recovery in (False, True):
            eng = engine.Engine(ru.params(m, recovery), device=0)
            _, stats = eng.process(batch)
            routes.append((eng.prebuilt_count(), eng.rerun_count(), [(s["status"], s["n_builds"], s["n_kmers"], s["max_nodes"]) for s in stats]))
            eng.close()
        assert routes[0] == routes[1], case
    # a case whose windows all start in LDS without -R still does with it
    m, batch, kept = ru.case_batch("rec_low")
    eng = engine.Engine(ru.params(m, True), device=0)
    eng.process(batch)
    assert eng.prebuilt_count() > 0
    eng.close()


def test_two_engines_taking_turns_with_recovery():
    cases = [c for c in ru.CASES]
    batches = [ru.case_batch(c)[1] for c in cases]
    p = ru.params(ru.meta("rec_low"), True)                                      # (the cases of default k range only)
    use = [i for i, c in enumerate(cases) if "--min-k" not in ru.meta(c)["flags"]]
    one = engine.Engine(p)
    want = [one.process(batches[i]) for i in use]
    one.close()
    pair = [engine.Engine(p), engine.Engine(p)]
    for rep in range(2):
        got = [None] * len(use)
        pair[0].upload(batches[use[0]]); pair[0].submit()
        for i in range(1, len(use) + 1):
            cur, prev = pair[i & 1], pair[(i - 1) & 1]
            if i < len(use):
                cur.upload(batches[use[i]]); cur.submit(after=prev)
            prev.wait()
            got[i - 1] = prev.results()
        assert got == want, rep
    for e_ in pair:
        e_.close()
    for i, w in zip(use, want):                                                    # and they are the reference's
        db = engine.VariantDB(); db.add_records(w[0], _names(batches[i]))
        assert db.vcf() == ru.golden_vcf(cases[i], True)


def _run_bin(tmp_path, extra):
    for src, dst in ((f"{CLI_CASE}.tumor.bam", "tumor.bam"), (f"{CLI_CASE}.normal.bam", "normal.bam"), (f"{CLI_CASE}.fa", "ref.fa")):
        shutil.copy(os.path.join(ru.DIR, src), os.path.join(tmp_path, dst))
    region = ru.meta(CLI_CASE)["region"]
    argv = ["--tumor", "tumor.bam", "--normal", "normal.bam", "--ref", "ref.fa", "--reg", region, "--num-threads", "1"] + extra
    argv += ["-v"]                                                                 # (the reference's runs were made with -v: it is part of ##cmdline)
    return subprocess.run([BIN] + argv + ["--date-line", DATE], cwd=tmp_path, capture_output=True, text=True, timeout=300), argv


def _no_date(text):
    return "".join(l + "\n" for l in text.splitlines() if not l.startswith("##fileDate"))


@pytest.mark.parametrize("opt", ["--kmer-recovery", "-R", None])
def test_lancet_gpu_bam_to_vcf_is_byte_identical_to_the_reference(opt, tmp_path):
    r, argv = _run_bin(str(tmp_path), [opt] if opt else [])
    assert r.returncode == 0, r.stderr[-2000:]
    want = ru.golden_vcf(CLI_CASE, opt is not None, full=True)
    got = _no_date(r.stdout)
    # ##cmdline carries the option exactly as typed; the reference was run with the long spelling
    cmd = [l for l in got.splitlines() if l.startswith("##cmdline")]
    assert [c.rstrip() for c in cmd] == ["##cmdline=lancet " + " ".join(argv)]
    if opt == "-R":
        got = got.replace(cmd[0] + "\n", cmd[0].replace(" -R ", " --kmer-recovery ") + "\n")
    rs = lambda text: "".join((l.rstrip() if l.startswith("##cmdline") else l) + "\n" for l in text.splitlines())   # (the reference ends the line with a blank)
    assert rs(got) == rs(want)


def test_python_cli_takes_the_option(tmp_path):
    for src, dst in ((f"{CLI_CASE}.tumor.bam", "tumor.bam"), (f"{CLI_CASE}.normal.bam", "normal.bam"), (f"{CLI_CASE}.fa", "ref.fa")):
        shutil.copy(os.path.join(ru.DIR, src), os.path.join(tmp_path, dst))
    t = str(tmp_path)
    for rec in (True, False):
        out = io.StringIO()
        argv = ["--tumor", t + "/tumor.bam", "--normal", t + "/normal.bam", "--ref", t + "/ref.fa", "--reg", ru.meta(CLI_CASE)["region"], "--num-threads", "1"]
        assert cli.run(argv + (["--kmer-recovery"] if rec else []), out=out, date_line=DATE + "\n") == 0
        body = "".join(l + "\n" for l in out.getvalue().splitlines() if not l.startswith(("##fileDate", "##cmdline", "##reference")))
        assert body == ru.golden_vcf(CLI_CASE, rec)


def test_lancet_gpu_refuses_linked_reads_with_recovery(tmp_path):
    r, _ = _run_bin(str(tmp_path), ["--linked-reads", "-R"])
    assert r.returncode != 0 and "--linked-reads" in r.stderr and r.stdout == ""
