"""Device read selection on the GPU: the batch lancet_engine_upload_windows makes on the device (read back through the debug hook)
against the host batch array by array, the engine's records / stats / trace against the host route's and the goldens, two engines on
one resident table, and `lancet_gpu --device-select` against the golden VCFs and traces."""
import json
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu
import select_cases as sc
from lancet_amd import abi, build, engine, host
from test_host_native import FLT_CASES, _body

pytestmark = pytest.mark.gpu
G = sc.G
DATE = "Sun Sep 27 05:27:00 2026"


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build()


def _open(case, region, o, bed=None):
    H = host.NativeHost(*sc.fixture_paths(case))
    n = len(H.tile_regions([region] if region else [], o, bed=bed))
    return H, n


def _device_words(dbg):
    return lambda bo, go, ln: (sc._gather(dbg["bases"], bo, (ln + 15) // 16), sc._gather(dbg["good"], go, (ln + 31) // 32))


CASES = {"ar_small": ("chr22:900-3000", {}, None), "ar_small_ar_off": ("chr22:900-3000", {"active_region": 0}, None),
         "flt_small": (FLT_CASES["flt_small"][0], FLT_CASES["flt_small"][1], None),
         "flt_small_cov": (FLT_CASES["flt_small"][0], {"max_avg_cov": 24, "active_region": 0}, None),
         "bed2": (json.load(open(os.path.join(G, "bed2.case.txt")))["region"], {}, os.path.join(G, "bed2.bed"))}


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_made_batch_equals_the_host_batch_array_by_array(name):
    region, kw, bed = CASES[name]
    case = name.split("_ar_off")[0].split("_cov")[0]
    o = host.default_opts(**kw)
    P = abi.default_params()
    H, n = _open(case, region, o, bed)
    reads = engine.DeviceReads(H.alignment_table(o, P))
    assert reads.nbytes > 0
    eng = engine.Engine(P)
    skipped = kept_any = False
    for lo, hi in ((0, n), (0, n // 2), (n // 2, n)):           # the whole scan, then in two batches
        sl = H.windows(lo, hi, o)
        kept = eng.upload_windows(reads, sl, o, host=H)
        assert kept is not None, eng.last_error()
        dbg = eng.debug_batch() if kept else None
        summ = eng.select_summaries()
        skipped |= any((s[0] & 3) == 2 for s in summ); kept_any |= bool(kept)
        want = sc.host_expectation(H, lo, hi, o, P)
        assert kept == want["kept"]
        if kept:
            sc.assert_same(dict(dbg, kept=kept), want, _device_words(dbg))
            sc.assert_summaries(summ, sl, want)
    assert kept_any and skipped == (name == "flt_small_cov")      # (--max-avg-cov 24 skips some windows of flt_small and keeps others)
    reads.close(); H.close()


@pytest.mark.parametrize("case,region,kw", [("ar_small", "chr22:900-3000", {}), ("flt_small", FLT_CASES["flt_small"][0], FLT_CASES["flt_small"][1])])
def test_records_stats_and_trace_equal_the_host_route_and_the_golden(case, region, kw):
    o = host.default_opts(**kw)
    P = abi.default_params()
    H, n = _open(case, region, o)
    reads = engine.DeviceReads(H.alignment_table(o, P))
    dev = engine.Engine(P, trace_words=1 << 17)
    kept = dev.upload_windows(reads, H.windows(0, n, o), o, host=H)
    assert kept
    H.windows_done(0, n)
    dev.run()
    got_v, got_s = dev.results()
    got_t = dev.trace_text()
    H2, _ = _open(case, region, o)
    b, idx, pk = H2.batch(0, n, o, pack_params=P)
    ref = engine.Engine(P, trace_words=1 << 17)
    ref.upload_packed(b, pk)
    ref.run()
    want_v, want_s = ref.results()
    assert kept == idx and got_v == want_v and got_s == want_s and len(got_v) > 0
    assert gu.digest_trace(got_t) == gu.digest_trace(ref.trace_text()) == gu.digest_trace(gu.golden_trace(case))
    db = engine.VariantDB()
    db.add_records(got_v, ["chr22"])
    assert db.vcf(sample_normal="NORMAL", sample_tumor="TUMOR") == gu.golden_vcf(case)
    reads.close(); H.close(); H2.close()


def test_two_engines_share_one_table_and_take_turns():
    o = host.default_opts()
    P = abi.default_params()
    H, n = _open("ar_small", "chr22:900-3000", o)
    reads = engine.DeviceReads(H.alignment_table(o, P))
    ranges = [(lo, min(n, lo + 5)) for lo in range(0, n, 5)]
    one = engine.Engine(P)
    want = []
    for lo, hi in ranges:
        kept = one.upload_windows(reads, H.windows(lo, hi, o), o)
        assert kept is not None
        H.windows_done(lo, hi)
        if kept:
            one.run()
            want.append((kept, one.results()))
        else:
            want.append((kept, ([], [])))
    assert sum(len(k) for k, _ in want) > 5
    pair = [engine.Engine(P), engine.Engine(P)]
    for rep in range(2):                                        # twice: the same again
        got, pend, prev = {}, [], None                          # pend: (engine, range number, kept) of the batches in flight
        for i, (lo, hi) in enumerate(ranges):
            cur = pair[i & 1]
            for e, j, k in [x for x in pend if x[0] is cur]:    # its batch before this one: collect it, the engine is reused
                e.wait(); got[j] = (k, e.results()); pend.remove((e, j, k))
            kept = cur.upload_windows(reads, H.windows(lo, hi, o), o)      # (while the other engine's kernels run)
            assert kept is not None
            H.windows_done(lo, hi)
            if kept:
                cur.submit(after=prev)
                pend.append((cur, i, kept)); prev = cur
            else:
                got[i] = (kept, ([], []))
        for e, j, k in pend:
            e.wait(); got[j] = (k, e.results())
        assert [got[i] for i in range(len(ranges))] == want
    reads.close(); H.close()


def test_a_batch_of_one_window_and_an_empty_range():
    o = host.default_opts(active_region=0)
    P = abi.default_params()
    H, n = _open("ar_small", "chr22:900-3000", o)
    reads = engine.DeviceReads(H.alignment_table(o, P))
    eng = engine.Engine(P)
    assert eng.upload_windows(reads, H.windows(3, 3, o), o) == []
    H.windows_done(3, 3)
    kept = eng.upload_windows(reads, H.windows(3, 4, o), o, host=H)
    assert kept == [3]
    dbg = eng.debug_batch()
    want = sc.host_expectation(H, 3, 4, o, P)
    sc.assert_same(dict(dbg, kept=kept), want, _device_words(dbg))
    eng.run()
    v, s = eng.results()
    ref = engine.Engine(P)
    H2, _ = _open("ar_small", "chr22:900-3000", o)
    b, idx, pk = H2.batch(3, 4, o, pack_params=P)
    ref.upload_packed(b, pk); ref.run()
    assert (v, s) == ref.results() and len(s) == 1
    # an engine made for other thresholds than the table's refuses it
    other = engine.Engine(abi.default_params(min_qual_trim=33 + 20))
    with pytest.raises(engine.EngineError, match="thresholds"):
        other.upload_windows(reads, H2.windows(0, 2, o), o)
    reads.close(); H.close(); H2.close()


def _cli(case, region, extra, env=None, bed=None):
    p = sc.fixture_paths(case)
    cmd = [build.BIN, "--tumor", p[0], "--normal", p[1], "--ref", p[2], "--date-line", DATE] + (["--reg", region] if region else []) + (["--bed", bed] if bed else []) + extra
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def _select_line(err):
    lines = [l for l in err.splitlines() if l.startswith("[lancet_gpu] device select:") and "batches taken" in l]
    assert len(lines) == 1, err[-1500:]
    return lines[0]


CLI = [("ar_small", "chr22:900-3000", [], None, "ar_small"), ("ar_small", "chr22:900-3000", ["--batch-windows", "4", "--devices", "0,0"], None, "ar_small"),
       ("flt_small", FLT_CASES["flt_small"][0], FLT_CASES["flt_small"][2] + ["--batch-windows", "9"], None, "flt_small"),
       ("lrflt_small", FLT_CASES["lrflt_small"][0], FLT_CASES["lrflt_small"][2], None, "lrflt_small"),
       ("bed2", json.load(open(os.path.join(G, "bed2.case.txt")))["region"], ["--batch-windows", "9"], os.path.join(G, "bed2.bed"), "bed2"),
       ("leak_small", "chr22:1000-3000", ["--active-region-off", "--batch-windows", "4"], None, "leak_small")]


@pytest.mark.parametrize("case,region,extra,bed,golden", CLI)
def test_lancet_gpu_device_select_vcf_and_trace_equal_the_goldens(case, region, extra, bed, golden):
    r = _cli(case, region, extra + ["--device-select", "-v"], bed=bed)
    assert _body(r.stdout) == gu.golden_vcf(golden) and "--device-select" not in r.stdout and "##cmdline=lancet --tumor" in r.stdout
    assert gu.digest_trace(r.stderr) == gu.digest_trace(gu.golden_trace(golden))
    line = _select_line(r.stderr)
    if case == "ar_small":
        assert " 0 not taken" in line and " 0 batches taken" not in line
    if case == "leak_small":                                    # batches of four: [4, 8) holds the run without mapped reads, [8, 12) inherits its reads
        assert "2 not taken (leak 2)" in line and " 0 batches taken" not in line
    if case == "lrflt_small":
        assert " 0 batches taken" in line and "linked reads" in line
    # the host route's output, byte for byte (the option is taken out of ##cmdline as --date-line is)
    assert _cli(case, region, extra + ["-v"], bed=bed).stdout == r.stdout


def test_lancet_gpu_environment_switch_and_rg_file():
    a = _cli("ar_small", "chr22:900-3000", ["--device-select"])
    b = _cli("ar_small", "chr22:900-3000", [], env={"LANCET_DEVICE_SELECT": "1"})
    assert a.stdout == b.stdout and _body(a.stdout) == gu.golden_vcf("ar_small")
    assert _select_line(a.stderr) == _select_line(b.stderr) and " 0 not taken" in _select_line(b.stderr)
    rg = os.path.join(G, "rg_small.rg.txt")
    r = _cli("rg_small", "chr22:900-3100", ["--rg-file", rg, "--device-select", "-v"])
    assert _body(r.stdout) == gu.golden_vcf("rg_small") and gu.digest_trace(r.stderr) == gu.digest_trace(gu.golden_trace("rg_small"))
    assert " 0 batches taken" in _select_line(r.stderr) and "rg-file" in _select_line(r.stderr)


@pytest.mark.parametrize("case,region,extra,bed,golden", [
    ("bed2", json.load(open(os.path.join(G, "bed2.case.txt")))["region"], ["--ranks", "2", "--devices", "0,0", "--batch-windows", "9"], os.path.join(G, "bed2.bed"), "bed2"),
    ("leak_small", "chr22:1000-3000", ["--active-region-off", "--ranks", "2", "--devices", "0,0", "--batch-windows", "2"], None, "leak_small")])
def test_lancet_gpu_device_select_with_ranks(case, region, extra, bed, golden):
    """Every rank exports what lancet_host_load_range loaded for it (bed2 has indexes: each rank loads its own range) and makes its own
    table resident; the records reach rank 0 as ever (two processes on the one GPU: the test transport)."""
    r = _cli(case, region, extra + ["--device-select"], env={"LANCET_COMM_TEST_FILES": "1"}, bed=bed)
    assert _body(r.stdout) == gu.golden_vcf(golden) and "--device-select" not in r.stdout
    lines = [l for l in r.stderr.splitlines() if l.startswith("[lancet_gpu] device select:") and "batches taken" in l]
    assert len(lines) == 2 and {l.split("[rank ")[1][0] for l in lines} == {"0", "1"}
    assert not any(" 0 batches taken" in l for l in lines)
    if case == "leak_small":
        assert sum(int(l.split(" not taken")[0].split()[-1]) for l in lines) >= 2 and any("leak" in l for l in lines)
