"""The reads' placements on the GPU: engine.Engine(haplotype_words=..., haplotype_placements=True) -- the placement kernel
(lancet_amd/csrc/hap_place.h) behind the window kernels, the re-run tier's kernel and the support kernel -- and `lancet_gpu --haplotype-reads`.
Hand-made windows whose records are known from how their reads were cut; every edge of the kernel and the five more_verbose fixtures against
the plain model of tests/hap_place_cases.py.  test_haplotype_placements_emu.py holds the emulated kernel to the same, and to the
hand-written shapes no assembly produces."""
import os
import re
import shutil
import subprocess

import pytest

import golden_util as gu
import hap_cases as hc
import hap_place_cases as pc
import hap_sup_cases as sc
import more_verbose_util as mv
from lancet_amd import abi, engine, host

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lancet_amd", "bin", "lancet_gpu")
CLI_CASE = "mv_low"
DATE = "Sun Sep 27 05:27:00 2026"


def _engine(batch, p, words=None, mm=5, **kw):
    return engine.Engine(p, device=0, haplotype_words=words or sc.ample_words(batch, p), haplotype_placements=True, haplotype_placement_mismatches=mm, **kw)


def _process(eng, batch):
    v, st = eng.process(batch)
    haps, trunc = eng.haplotypes()
    return v, st, haps, trunc, eng.placements()


@pytest.mark.parametrize("tier", ["one_tier", "rerun"])
@pytest.mark.parametrize("variant", ["snv", "del3"])
def test_engine_planted_records(variant, tier, monkeypatch):
    """Every tiled read at the position it was cut at; one haplotype over the site, two and the lower index away from it; the reads that keep
    k, k - 1 and no bases on the window -- from the window kernel's entries and from the re-run tier's."""
    batch, p, alt, ref, _ = sc.basic_batch(variant)
    if tier == "rerun":
        monkeypatch.setenv("LANCET_NODE_CAP1", "64")
    eng = _engine(batch, p)
    v, st, haps, trunc, pl = _process(eng, batch)
    assert (eng.rerun_count() > 0) == (tier == "rerun") and eng.haplotype_placement_ms() > 0
    pc.check_basic(variant, batch, st, haps, pl)
    pc.check_model(batch, p, haps, pl, 5)
    eng.close()


@pytest.mark.parametrize("k", [11, 15, 35])
def test_engine_edges_against_the_model(k):
    batch, p, names = sc.edge_batch(k)
    eng = _engine(batch, p)
    v, st, haps, trunc, pl = _process(eng, batch)
    assert not any(trunc)
    pc.check_model(batch, p, haps, pl, 5)
    assert pc.check_snv_ends(k, batch, p, names, haps, pl) or k == 11
    eng.close()


def test_engine_mismatch_limit_and_second_runs():
    """d == max_mm is placed, d == max_mm + 1 is not; 0 and 255; the same engine, one upload after the other, and a run repeated (the records
    are zeroed per run)."""
    batch, p, names = sc.edge_batch(15)
    eng = _engine(batch, p)
    n_placed = []
    for mm in (0, 4, 5, 6, 255):
        eng.set_haplotype_placements(True, mm)
        v, st, haps, trunc, pl = _process(eng, batch)
        pc.check_model(batch, p, haps, pl, mm)
        n_placed.append(int((pl[0]["haplotype"] >= 0).sum()))
    assert n_placed == sorted(n_placed) and n_placed[1] < n_placed[2] < n_placed[3]        # (the reads with exactly 5 and exactly 6 substitutions)
    eng.run()
    again = eng.placements()
    assert pc.as_tuples(again[0]) == pc.as_tuples(pl[0])
    eng.set_haplotype_placements(True, 0)                               # a stricter limit on the same resident engine: nothing of the last run is left
    v, st, haps, trunc, pl0 = _process(eng, batch)
    pc.check_model(batch, p, haps, pl0, 0)
    eng.close()


@pytest.mark.parametrize("tier", ["one_tier", "rerun"])
@pytest.mark.parametrize("case", mv.CASES)
def test_engine_fixtures_against_the_model(case, tier, monkeypatch):
    """The five more_verbose cases with support on at the same limit: the model, the invariants that tie placements to the support counts;
    support counts, entries, records, stats and trace are identical with the placement switch on and off."""
    m, batch, kept = mv.case_batch(case)
    p = mv.params(m)
    words = sc.ample_words(batch, p) + 32 * 64
    ec = mv.trace_words(batch, p)
    kw = dict(device=0, trace_words=ec, trace_level=2, haplotype_words=words, haplotype_alignments=True, haplotype_support=True)
    if tier == "rerun":
        monkeypatch.setenv("LANCET_NODE_CAP1", "64")
    eng = engine.Engine(p, **kw)
    v0, st0, haps0, trunc0, pl0 = _process(eng, batch)
    text0 = eng.trace_text()
    assert len(pl0[0]) == 0 and eng.haplotype_placement_ms() == 0
    eng.close()
    eng = engine.Engine(p, haplotype_placements=True, **kw)
    v, st, haps, trunc, pl = _process(eng, batch)
    assert not any(trunc) and (eng.rerun_count() > 0) == (tier == "rerun") and eng.haplotype_placement_ms() > 0
    assert (v, st, haps, trunc) == (v0, st0, haps0, trunc0) and eng.trace_text() == text0
    pc.check_model(batch, p, haps, pl, 5)
    pc.check_support_invariants(batch, haps, pl)
    eng.close()


def test_engine_one_string_at_two_k():
    batch, p = sc.dups_batch()
    eng = _engine(batch, p)
    v, st, haps, trunc, pl = _process(eng, batch)
    pc.check_model(batch, p, haps, pl, 5)
    assert max(int(x) for x in pl[0]["n_haplotypes"]) >= 2
    eng.close()


def test_engine_offset_tie_on_a_lower_lane_of_a_later_trip():
    batch, p, ref, read = pc.tie_batch()
    eng = _engine(batch, p)
    v, st, haps, trunc, pl = _process(eng, batch)
    pc.check_tie(batch, st, haps, pl)
    pc.check_model(batch, p, haps, pl, 5)
    eng.close()


def test_engine_a_buffer_that_truncates():
    m, batch, kept = mv.case_batch("mv_nref")
    p = mv.params(m)
    eng = _engine(batch, p)
    fv, fst, fh, ft, fpl = _process(eng, batch)
    per = {w: [h for h in fh if h["window"] == w] for w in range(batch.n_windows)}
    w = next(w for w, hs in per.items() if len(hs) >= 2 and any(int(r["haplotype"]) >= 1 for r in fpl[0][int(fpl[1][w]):int(fpl[1][w + 1])]))
    eng.set_haplotypes(hc.words_of(per[w][0]) + hc.words_of(per[w][1]) - 1)
    cv, cst, ch, ct, cpl = _process(eng, batch)
    assert ct[w] == 1 and [h["index"] for h in ch if h["window"] == w] == [0]
    pc.check_model(batch, p, ch, cpl, 5)
    eng.close()


def test_engine_every_upload_route():
    """lancet_engine_upload, _upload_packed with read_index (a read of several windows is stored once) and _upload_windows (the batch made on
    the device): the same records, and the model's."""
    G = gu.GOLDEN
    paths = [os.path.join(G, f"ar_small.{x}") for x in ("tumor.bam", "normal.bam", "fa")]
    p = abi.default_params()
    o = host.default_opts(active_region=0, min_qual_call=p.min_qual_call)
    H = host.NativeHost(*paths)
    n = len(H.tile("chr22:900-3100", o))
    b, idx = H.batch(0, n, o)
    b2, idx2, pk = H.batch(0, n, o, pack_params=p)
    assert "read_index" in pk and pk["n_distinct"] < b.n_reads
    eng = _engine(b, p)
    v, st, haps, trunc, pl = _process(eng, b)
    assert haps and not any(trunc) and (pl[0]["haplotype"] >= 0).any()
    pc.check_model(b, p, haps, pl, 5)
    eng.upload_packed(b2, pk)
    eng.run()
    pl2 = eng.placements()
    assert eng.results() == (v, st) and pc.as_tuples(pl2[0]) == pc.as_tuples(pl[0]) and list(pl2[1]) == list(pl[1]) and list(pl2[2]) == list(pl[2])
    reads = engine.DeviceReads(H.alignment_table(o, p))
    kept = eng.upload_windows(reads, H.windows(0, n, o), o, host=H)
    assert kept == idx, eng.last_error()
    eng.run()
    pl3 = eng.placements()
    assert eng.results() == (v, st) and pc.as_tuples(pl3[0]) == pc.as_tuples(pl[0]) and list(pl3[1]) == list(pl[1]) and list(pl3[2]) == list(pl[2])
    reads.close(); H.close(); eng.close()


def test_engine_state_rules_arguments_and_independence():
    batch, p, names = sc.edge_batch(15)
    eng = engine.Engine(p, device=0, haplotype_placements=True)                         # the switch without the capture: nothing
    v, st = eng.process(batch)
    assert len(eng.placements()[0]) == 0 and eng.haplotype_placement_ms() == 0
    L = eng.L
    for on, mm in ((2, 5), (-1, 5), (1, -1), (1, 256), (0, 256)):
        assert L.lancet_engine_set_haplotype_placements(eng.h, on, mm) == -1             # LANCET_E_ARG
    # more entries than the index field holds: refused where either of the two is set, nothing allocated
    limit = 9 * ((1 << 24) - 1)
    assert L.lancet_engine_set_haplotypes(eng.h, limit + 9) == -1 and L.lancet_engine_set_haplotypes(eng.h, limit + 8) == 0
    assert L.lancet_engine_set_haplotype_placements(eng.h, 0, 5) == 0 and L.lancet_engine_set_haplotypes(eng.h, limit + 9) == 0
    assert L.lancet_engine_set_haplotype_placements(eng.h, 1, 5) == -1
    eng.close()
    eng = _engine(batch, p)
    eng.upload(batch)
    assert L.lancet_engine_set_haplotype_placements(eng.h, 0, 5) == -6                   # LANCET_E_STATE: between an upload and its run
    with pytest.raises(engine.EngineError):
        eng.set_haplotype_placements(False)
    eng.submit()
    assert L.lancet_engine_set_haplotype_placements(eng.h, 0, 5) == -6                   # ... and in flight
    eng.wait()
    (v, st), (haps, trunc), pl = eng.results(), eng.haplotypes(), eng.placements()
    want = pc.check_model(batch, p, haps, pl, 5)                                        # the refused calls changed nothing
    # the two limits are independent, and neither switch changes the other's output
    both = engine.Engine(p, device=0, haplotype_words=sc.ample_words(batch, p), haplotype_support=True, haplotype_support_mismatches=0,
                         haplotype_placements=True, haplotype_placement_mismatches=5)
    bv, bst = both.process(batch)
    bh, bt = both.haplotypes()
    assert pc.as_tuples(both.placements()[0]) == want and (bv, bst, bt) == (v, st, trunc)
    sup = engine.Engine(p, device=0, haplotype_words=sc.ample_words(batch, p), haplotype_support=True, haplotype_support_mismatches=0)
    sup.process(batch)
    assert sup.haplotypes() == (bh, bt) and sc.strip_support(bh) == haps
    eng.set_haplotype_placements(False)                                                 # takes effect at the next upload
    v1, st1 = eng.process(batch)
    assert (v1, st1) == (v, st) and eng.haplotypes() == (haps, trunc) and len(eng.placements()[0]) == 0
    for e in (eng, both, sup):
        e.close()


# ---------------------------------------------------------------- lancet_gpu --haplotype-reads

def _run_bin(tmp_path, extra):
    for src, dst in ((f"{CLI_CASE}.tumor.bam", "tumor.bam"), (f"{CLI_CASE}.normal.bam", "normal.bam"), (f"{CLI_CASE}.fa", "ref.fa")):
        shutil.copy(os.path.join(mv.DIR, src), os.path.join(tmp_path, dst))
    argv = ["--tumor", "tumor.bam", "--normal", "normal.bam", "--ref", "ref.fa", "--reg", mv.meta(CLI_CASE)["region"], "--num-threads", "1"] + extra
    return subprocess.run([BIN] + argv + ["--date-line", DATE], cwd=tmp_path, capture_output=True, text=True, timeout=300)


def _sam(path):
    lines = open(path).read().splitlines()
    return [l for l in lines if l.startswith("@")], [l.split("\t") for l in lines if not l.startswith("@")]


def test_lancet_gpu_haplotype_reads(tmp_path):
    assert mv.meta(CLI_CASE)["cli"]
    tmp = str(tmp_path)
    r0 = _run_bin(tmp, [])
    r = _run_bin(tmp, ["--haplotype-reads", "reads.sam"])
    assert r0.returncode == 0 and r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == r0.stdout and "haplotype-read" not in r.stdout                   # the VCF, ##cmdline included: byte for byte
    text = open(os.path.join(tmp, "reads.sam")).read()
    head, recs = _sam(os.path.join(tmp, "reads.sam"))
    assert recs and f"{len(recs)} reads written to reads.sam" in r.stderr and "did not all fit" not in r.stderr
    # the records are the engine's for the same windows (and so the model's: test_engine_fixtures_against_the_model)
    m, batch, kept = mv.case_batch(CLI_CASE)
    p = mv.params(m)
    eng = engine.Engine(p, device=0, haplotype_words=sc.ample_words(batch, p) + 32 * 64, haplotype_alignments=True, haplotype_placements=True)
    v, st, haps, trunc, (pl, rb, tl) = _process(eng, batch)
    eng.close()
    first = {}
    for i, h in enumerate(haps):
        first.setdefault(h["window"], i)
    want = []
    for w in range(batch.n_windows):
        reads = sc.trimmed_reads(batch, p, w)
        for r in range(int(rb[w]), int(rb[w + 1])):
            x = pl[r]
            if int(x["haplotype"]) >= 0:
                h = haps[first[w] + int(x["haplotype"])]
                start, ops, has_m = abi.read_cigar(int(x["offset"]), int(tl[r]), h["len"], h["ref_off"], h["cigar"])
                want.append((r - int(rb[w]), 16 if int(x["cls"]) & 1 else 0, start, "".join(f"{n}{op}" for n, op in ops), reads[r - int(rb[w])][0],
                             [f"hi:i:{int(x['haplotype'])}", f"kk:i:{h['kmer']}", f"cp:i:{h['component']}", f"ho:i:{int(x['offset'])}", f"hm:i:{int(x['mismatches'])}",
                              f"on:i:{int(x['n_offsets'])}", f"hn:i:{int(x['n_haplotypes'])}", f"sm:A:{'N' if int(x['cls']) & 2 else 'T'}"]))
    assert len(recs) == len(want)
    for f, (rn, flag, start, cigar, seq, tags) in zip(recs, want):
        win = f[11][5:]
        c, span = win.split(":")
        lo, hi = (int(x) for x in span.split("-"))
        assert f[0] == f"{win}|r={rn}" and int(f[1]) == flag and f[2] == c and f[4] == "255" and f[5] == cigar and f[9] == seq and f[10] == "*"
        assert f[11].startswith("wn:Z:") and f[12:] == tags
        assert lo <= int(f[3]) <= hi and int(f[3]) == lo + start                         # POS lies inside the window
        assert sum(int(n) for n, op in re.findall(r"(\d+)([MIDS])", f[5]) if op in "MIS") == len(f[9])      # SEQ length = the CIGAR's query length
    # with --haplotype-sam: the same header, the same records; hi is the pi of that file
    r2 = _run_bin(tmp, ["--haplotype-sam", "hap.sam", "--haplotype-reads", "reads2.sam"])
    assert r2.returncode == 0 and r2.stdout == r0.stdout and open(os.path.join(tmp, "reads2.sam")).read() == text
    head2, hrecs = _sam(os.path.join(tmp, "hap.sam"))
    assert head2 == head and {(f[11], f[12]) for f in recs} <= {(next(t for t in g if t.startswith("wn:Z:")), "hi:i:" + next(t for t in g if t.startswith("pi:i:"))[5:]) for g in hrecs}
    # with --haplotype-support at the same limit: both files as they are alone
    r3 = _run_bin(tmp, ["--haplotype-support", "hap.sup", "--haplotype-reads", "reads3.sam"])
    r3b = _run_bin(tmp, ["--haplotype-support", "alone.sup"])
    assert r3.returncode == 0 and r3b.returncode == 0 and r3.stdout == r0.stdout and open(os.path.join(tmp, "reads3.sam")).read() == text
    assert open(os.path.join(tmp, "hap.sup")).read() == open(os.path.join(tmp, "alone.sup")).read()
    # with --device-select: the batches go the host route, counted under a reason of their own
    r4 = _run_bin(tmp, ["--device-select", "--haplotype-reads", "reads4.sam"])
    assert r4.returncode == 0 and r4.stdout == r0.stdout and open(os.path.join(tmp, "reads4.sam")).read() == text
    assert re.search(r"device select: 0 batches taken, \d+ not taken \(haplotype reads \d+\)", r4.stderr), r4.stderr[-1000:]
    # another limit
    r5 = _run_bin(tmp, ["--haplotype-reads", "zero.sam", "--haplotype-read-mismatches", "0"])
    _, zero = _sam(os.path.join(tmp, "zero.sam"))
    assert r5.returncode == 0 and r5.stdout == r0.stdout and 0 < len(zero) < len(recs) and all("hm:i:0" in f for f in zero)


def test_lancet_gpu_haplotype_reads_refusals(tmp_path):
    r = _run_bin(str(tmp_path), ["--ranks", "2", "--haplotype-reads", "reads.sam"])
    assert r.returncode != 0 and r.stdout == "" and "--haplotype-reads" in r.stderr and "--ranks" in r.stderr
    assert not os.path.exists(os.path.join(str(tmp_path), "reads.sam"))                 # before any work
    r = _run_bin(str(tmp_path), ["--haplotype-reads", "reads.sam", "--haplotype-read-mismatches", "256"])
    assert r.returncode != 0 and "--haplotype-read-mismatches" in r.stderr
