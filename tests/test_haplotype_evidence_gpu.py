"""The variant evidence on the GPU: engine.Engine(haplotype_words=..., haplotype_alignments=True, haplotype_evidence=E) -- the evidence kernel
(lancet_amd/csrc/hap_evidence.h) behind the window kernels, the re-run tier's kernel and the support and placement kernels -- and
`lancet_gpu --variant-evidence`.  Hand-made windows whose counts are known from how their reads were cut; every edge an assembly yields and
the five more_verbose fixtures against the plain model of tests/hap_evid_cases.py.  test_haplotype_evidence_emu.py holds the emulated
kernel to the same, and to the hand-written shapes no assembly produces."""
import hashlib
import os
import re
import shutil
import subprocess

import pytest

import golden_util as gu
import hap_evid_cases as ec
import hap_sup_cases as sc
import more_verbose_util as mv
from lancet_amd import abi, engine, host

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lancet_amd", "bin", "lancet_gpu")
CLI_CASE = "mv_low"
DATE = "Sun Sep 27 05:27:00 2026"


def _engine(batch, p, words=None, mm=5, evid=256, **kw):
    return engine.Engine(p, device=0, haplotype_words=words or sc.ample_words(batch, p) + 32 * 64, haplotype_alignments=True, haplotype_evidence=evid,
                         haplotype_evidence_mismatches=mm, **kw)


def _process(eng, batch):
    v, st = eng.process(batch)
    haps, trunc = eng.haplotypes()
    return v, st, haps, trunc, eng.evidence_marked()


@pytest.mark.parametrize("tier", ["one_tier", "rerun"])
@pytest.mark.parametrize("variant", ["snv", "del3"])
def test_engine_planted_counts(variant, tier, monkeypatch):
    """Item 1: the two paths, one group; the alt path's one event has alt = [5, 4, 0, 0], ref = [2, 3, 4, 6], other = 0 -- from the window
    kernel's entries and from the re-run tier's."""
    batch, p, alt, ref, _ = sc.basic_batch(variant)
    if tier == "rerun":
        monkeypatch.setenv("LANCET_NODE_CAP1", "64")
    eng = _engine(batch, p, haplotype_support=True)
    v, st, haps, trunc, marked = _process(eng, batch)
    assert (eng.rerun_count() > 0) == (tier == "rerun") and eng.haplotype_evidence_ms() > 0
    sc.check_basic(variant, batch, st, haps, trunc)
    ec.check_basic(variant, batch, st, haps, trunc, marked)
    ec.check_model(batch, p, haps, 5)
    ec.check_invariants(haps, True)
    ec.check_join(batch, haps, v, marked, abi.evidence_variant)
    eng.close()


@pytest.mark.parametrize("tier", ["one_tier", "rerun"])
@pytest.mark.parametrize("case", mv.CASES)
def test_engine_fixtures_join_model_and_invariants(case, tier, monkeypatch):
    """The five more_verbose cases with support and placements on: the join against the reference's own records, the model, the invariants;
    records, stats, trace, entries, support counts and placements are identical with the switch on and off."""
    m, batch, kept = mv.case_batch(case)
    p = mv.params(m)
    words = sc.ample_words(batch, p) + 32 * 64
    tw = mv.trace_words(batch, p)
    kw = dict(device=0, trace_words=tw, trace_level=2, haplotype_words=words, haplotype_alignments=True, haplotype_support=True, haplotype_placements=True)
    if tier == "rerun":
        monkeypatch.setenv("LANCET_NODE_CAP1", "64")
    eng = engine.Engine(p, **kw)
    v0, st0 = eng.process(batch)
    haps0, trunc0 = eng.haplotypes()
    pl0, text0 = eng.placements(), eng.trace_text()
    assert eng.haplotype_evidence_ms() == 0 and not any(eng.evidence_marked())
    eng.close()
    eng = engine.Engine(p, haplotype_evidence=256, **kw)
    v, st, haps, trunc, marked = _process(eng, batch)
    pl = eng.placements()
    assert not any(trunc) and not any(marked) and (eng.rerun_count() > 0) == (tier == "rerun") and eng.haplotype_evidence_ms() > 0
    assert (v, st, trunc) == (v0, st0, trunc0) and eng.trace_text() == text0 and [{k: x for k, x in h.items() if k != "events"} for h in haps] == haps0
    assert all((a == b).all() for a, b in zip(pl, pl0))
    assert any(h["events"] for h in haps)
    ec.check_join(batch, haps, v, marked, abi.evidence_variant)
    ec.check_model(batch, p, haps, 5)
    ec.check_invariants(haps, True)
    eng.close()


@pytest.mark.parametrize("k", [11, 15, 35])
def test_engine_edges_against_the_model(k):
    batch, p, names = sc.edge_batch(k)
    eng = _engine(batch, p, haplotype_support=True)
    v, st, haps, trunc, marked = _process(eng, batch)
    assert not any(trunc) and not any(marked)
    ec.check_model(batch, p, haps, 5)
    ec.check_invariants(haps, True)
    ec.check_join(batch, haps, v, marked, abi.evidence_variant)
    eng.close()


def test_engine_mismatch_limit_and_second_runs():
    """Limits 0, 4, 5, 6, 255 on one engine, one upload after the other; a run repeated (the records are zeroed per run); a stricter limit
    afterwards leaves nothing of the last run."""
    batch, p, names = sc.edge_batch(15)
    eng = _engine(batch, p)
    total = []
    for mm in (0, 4, 5, 6, 255):
        eng.set_haplotype_evidence(256, mm)
        v, st, haps, trunc, marked = _process(eng, batch)
        ec.check_model(batch, p, haps, mm)
        total.append(sum(sum(e["alt"]) + sum(e["ref"]) + sum(e["other"]) for h in haps for e in h["events"]))
    assert total == sorted(total) and total[0] > 0
    eng.run()
    assert eng.haplotypes()[0] == haps
    eng.set_haplotype_evidence(256, 0)
    v, st, haps0, trunc, marked = _process(eng, batch)
    ec.check_model(batch, p, haps0, 0)
    eng.close()


def test_engine_one_string_at_two_k():
    batch, p = sc.dups_batch()
    eng = _engine(batch, p)
    v, st, haps, trunc, marked = _process(eng, batch)
    ec.check_model(batch, p, haps, 5)
    ks = {}
    for h in haps:
        ks.setdefault(h["seq"], []).append(h)
    twice = [hs for hs in ks.values() if len({h["kmer"] for h in hs}) >= 2 and hs[0]["events"]]
    assert len(twice) == 1
    for h in twice[0]:
        (e,) = h["events"]
        assert (e["alt"], e["ref"], e["other"]) == ([5, 5, 0, 0], [0, 0, 5, 5], [0] * 4), (h["kmer"], e)
    eng.close()


def test_engine_events_per_window_one_short():
    m, batch, kept = mv.case_batch("mv_nref")
    p = mv.params(m)
    eng = _engine(batch, p)
    fv, fst, fh, ft, fm = _process(eng, batch)
    per = {}
    for h in fh:
        per[h["window"]] = per.get(h["window"], 0) + len(h["events"])
    w, n = max(per.items(), key=lambda x: x[1])
    assert n >= 2 and not any(fm)
    eng.set_haplotype_evidence(n - 1, 5)
    cv, cst, ch, ct, cm = _process(eng, batch)
    assert (cv, cst, ct) == (fv, fst, ft) and cm == [1 if per.get(x, 0) > n - 1 else 0 for x in range(batch.n_windows)] and cm[w] == 1
    ec.check_model(batch, p, ch, 5, cap=n - 1)
    assert [e for h in ch if h["window"] == w for e in h["events"]] == [e for h in fh if h["window"] == w for e in h["events"]][:n - 1]
    eng.close()


def test_engine_every_upload_route():
    """lancet_engine_upload, _upload_packed with read_index and _upload_windows (the batch made on the device): the same events, the model's."""
    G = gu.GOLDEN
    paths = [os.path.join(G, f"ar_small.{x}") for x in ("tumor.bam", "normal.bam", "fa")]
    p = abi.default_params()
    o = host.default_opts(active_region=0, min_qual_call=p.min_qual_call)
    H = host.NativeHost(*paths)
    n = len(H.tile("chr22:900-3100", o))
    b, idx = H.batch(0, n, o)
    b2, idx2, pk = H.batch(0, n, o, pack_params=p)
    eng = _engine(b, p)
    v, st, haps, trunc, marked = _process(eng, b)
    assert haps and not any(trunc) and not any(marked) and any(h["events"] for h in haps)
    ec.check_model(b, p, haps, 5)
    ec.check_join(b, haps, v, marked, abi.evidence_variant)
    eng.upload_packed(b2, pk)
    eng.run()
    assert eng.results() == (v, st) and eng.haplotypes() == (haps, trunc)
    reads = engine.DeviceReads(H.alignment_table(o, p))
    kept = eng.upload_windows(reads, H.windows(0, n, o), o, host=H)
    assert kept == idx, eng.last_error()
    eng.run()
    assert eng.results() == (v, st) and eng.haplotypes() == (haps, trunc)
    reads.close(); H.close(); eng.close()


def test_engine_state_rules_arguments_and_switch_off():
    batch, p, names = sc.edge_batch(15)
    words = sc.ample_words(batch, p) + 32 * 64
    eng = engine.Engine(p, device=0, haplotype_evidence=64)                              # the switch without the capture: nothing
    v, st = eng.process(batch)
    assert eng.haplotypes() == ([], [0] * batch.n_windows) and eng.haplotype_evidence_ms() == 0
    L = eng.L
    for n, mm in ((1 << 24, 5), (64, -1), (64, 256), (0, 256)):
        assert L.lancet_engine_set_haplotype_evidence(eng.h, n, mm) == -1                # LANCET_E_ARG
    eng.close()
    eng = engine.Engine(p, device=0, haplotype_words=words, haplotype_evidence=64)       # ... and without the alignments: no events, no kernel
    eng.process(batch)
    haps, trunc = eng.haplotypes()
    assert haps and all(h["events"] == [] for h in haps) and eng.haplotype_evidence_ms() == 0
    eng.close()
    eng = _engine(batch, p)
    eng.upload(batch)
    assert L.lancet_engine_set_haplotype_evidence(eng.h, 0, 5) == -6                     # LANCET_E_STATE: between an upload and its run
    with pytest.raises(engine.EngineError):
        eng.set_haplotype_evidence(0)
    eng.submit()
    assert L.lancet_engine_set_haplotype_evidence(eng.h, 0, 5) == -6                     # ... and in flight
    eng.wait()
    (v, st), (haps, trunc) = eng.results(), eng.haplotypes()
    ec.check_model(batch, p, haps, 5)                                                   # the refused calls changed nothing
    eng.set_haplotype_evidence(0)                                                       # takes effect at the next upload
    v1, st1 = eng.process(batch)
    h1, t1 = eng.haplotypes()
    assert (v1, st1, t1) == (v, st, trunc) and h1 == [{k: x for k, x in h.items() if k != "events"} for h in haps]
    ep, n, op, mp = (abi.C.POINTER(abi.LancetVariantEvidence)(), abi.C.c_uint32(7), abi.C.POINTER(abi.C.c_uint32)(), abi.C.POINTER(abi.C.c_uint8)())
    assert L.lancet_engine_results_haplotype_evidence(eng.h, abi.C.byref(ep), abi.C.byref(n), abi.C.byref(op), abi.C.byref(mp)) == 0
    assert not ep and n.value == 0 and eng.haplotype_evidence_ms() == 0
    eng.close()


# ---------------------------------------------------------------- lancet_gpu --variant-evidence

def _run_bin(tmp_path, extra):
    for src, dst in ((f"{CLI_CASE}.tumor.bam", "tumor.bam"), (f"{CLI_CASE}.normal.bam", "normal.bam"), (f"{CLI_CASE}.fa", "ref.fa")):
        shutil.copy(os.path.join(mv.DIR, src), os.path.join(tmp_path, dst))
    argv = ["--tumor", "tumor.bam", "--normal", "normal.bam", "--ref", "ref.fa", "--reg", mv.meta(CLI_CASE)["region"], "--num-threads", "1"] + extra
    return subprocess.run([BIN] + argv + ["--date-line", DATE], cwd=tmp_path, capture_output=True, text=True, timeout=300)


def test_lancet_gpu_variant_evidence(tmp_path):
    assert mv.meta(CLI_CASE)["cli"]
    tmp = str(tmp_path)
    r0 = _run_bin(tmp, [])
    r = _run_bin(tmp, ["--variant-evidence", "ev.tsv"])
    assert r0.returncode == 0 and r.returncode == 0, r.stderr[-2000:]
    assert hashlib.md5(r.stdout.encode()).hexdigest() == hashlib.md5(r0.stdout.encode()).hexdigest() and "variant-evidence" not in r.stdout
    lines = open(os.path.join(tmp, "ev.tsv")).read().splitlines()
    assert lines[0] == "#window\tchrom\tpos\tcode\tref\talt\tk\tcomponent\tpath\talt_Tf\talt_Tr\talt_Nf\talt_Nr\tref_Tf\tref_Tr\tref_Nf\tref_Nr\tother_Tf\tother_Tr\tother_Nf\tother_Nr"
    rows = [l.split("\t") for l in lines[1:]]
    assert rows and f"{len(rows)} events written to ev.tsv" in r.stderr and "unevaluated" not in r.stderr.replace("0 unevaluated", "")
    # the rows are the binding's for the same windows (and so the model's: test_engine_fixtures_join_model_and_invariants)
    m, batch, kept = mv.case_batch(CLI_CASE)
    p = mv.params(m)
    eng = _engine(batch, p)
    v, st, haps, trunc, marked = _process(eng, batch)
    eng.close()
    want = []
    for h in haps:
        for e in h["events"]:
            if e["variant"] >= 0:
                x = v[e["variant"]]
                want.append([x["pos"], x["code"], x["ref"], x["alt"], h["kmer"], h["component"], h["index"]] + e["alt"] + e["ref"] + e["other"])
    assert len(rows) == len(want)
    for f, x in zip(rows, want):
        c, span = f[0].split(":")
        assert f[1] == c and [int(f[2]), f[3], f[4], f[5]] + [int(y) for y in f[6:]] == x, (f, x)
    # with --haplotype-sam every record gains a tag with its events' counts; the file is otherwise what it is alone
    r2 = _run_bin(tmp, ["--haplotype-sam", "hap.sam", "--variant-evidence", "ev2.tsv"])
    r2b = _run_bin(tmp, ["--haplotype-sam", "alone.sam"])
    assert r2.returncode == 0 and r2b.returncode == 0 and r2.stdout == r0.stdout and open(os.path.join(tmp, "ev2.tsv")).read().splitlines() == lines
    with_tag = open(os.path.join(tmp, "hap.sam")).read().splitlines()
    alone = open(os.path.join(tmp, "alone.sam")).read().splitlines()
    assert [re.sub(r"\tev:Z:\S*", "", l) for l in with_tag] == alone and any("\tev:Z:" in l for l in with_tag)
    n_events = sum(len(h["events"]) for h in haps)
    assert sum(len(re.search(r"\tev:Z:(\S*)", l).group(1).split(";")) for l in with_tag if re.search(r"\tev:Z:\S", l)) == n_events
    # with --device-select the device route works unchanged: the kernel reads the resident batch whatever made it
    r4 = _run_bin(tmp, ["--device-select", "--variant-evidence", "ev4.tsv"])
    assert r4.returncode == 0 and r4.stdout == r0.stdout and open(os.path.join(tmp, "ev4.tsv")).read().splitlines() == lines
    r4b = _run_bin(tmp, ["--device-select"])
    line = lambda r: re.search(r"device select: (\d+) batches taken, .*", r.stderr).group(0)
    assert r4b.returncode == 0 and line(r4) == line(r4b) and "evidence" not in line(r4), (line(r4), line(r4b))      # the batches go the route they go without the option
    # another limit
    r5 = _run_bin(tmp, ["--variant-evidence", "zero.tsv", "--variant-evidence-mismatches", "0"])
    zero = [l.split("\t") for l in open(os.path.join(tmp, "zero.tsv")).read().splitlines()[1:]]
    assert r5.returncode == 0 and r5.stdout == r0.stdout and len(zero) == len(rows)
    assert sum(int(y) for f in zero for y in f[9:]) <= sum(int(y) for f in rows for y in f[9:])


def test_lancet_gpu_variant_evidence_refusals(tmp_path):
    r = _run_bin(str(tmp_path), ["--ranks", "2", "--variant-evidence", "ev.tsv"])
    assert r.returncode != 0 and r.stdout == "" and "--variant-evidence" in r.stderr and "--ranks" in r.stderr
    assert not os.path.exists(os.path.join(str(tmp_path), "ev.tsv"))                    # before any work
    r = _run_bin(str(tmp_path), ["--variant-evidence", "ev.tsv", "--variant-evidence-mismatches", "256"])
    assert r.returncode != 0 and "--variant-evidence-mismatches" in r.stderr
