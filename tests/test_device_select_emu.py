"""Device read selection without a GPU: the selection rules and the planning between its two passes (lancet_amd/csrc/select_rules.h,
select_host.h -- the product's source, lanes run one after the other by tests/select_emu) over lancet_host_alignment_table /
lancet_host_windows, against lancet_host_batch_packed on the same windows.  Exact equality; CPU only."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import bam_writer
import read_variety
import select_cases as sc
from lancet_amd import abi, build, engine, host, synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "select_emu"))
import select_emu  # noqa: E402

G = sc.G
from test_host_native import FLT_CASES, _OPT_FLAGS, _OPT_MAP  # noqa: E402  (the fixtures' option sets, as the host tests map them)


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build()


def _check_range(H, lo, hi, o, P, lds=(512, 32768)):
    """Both routes over [lo, hi): returns (emulated result, host expectation).  Taken: everything equal.  The host object ends behind hi."""
    tab = H.alignment_table(o, P)
    sl = H.windows(lo, hi, o)
    got = select_emu.run(tab, sl, o, *lds)
    want = sc.host_expectation(H, lo, hi, o, P)
    if got["rc"] == 0:
        sc.assert_same(got, want, sc.table_words(tab))
        sc.assert_summaries(got["summaries"], sl, want)
        assert got["need_large"] == sc.need_large(want, *lds)
    return got, want


def _scan(paths, region, o, P, step=None, bed=None, lds=(512, 32768)):
    H = host.NativeHost(*paths)
    n = len(H.tile_regions([region] if region else [], o, bed=bed))
    step = step or n
    out = [_check_range(H, lo, min(n, lo + step), o, P, lds) for lo in range(0, n, step)]
    H.close()
    return n, out


@pytest.mark.parametrize("kw", [{}, {"active_region": 0}, {"padding": 0, "window_size": 400, "max_k": 31}])
def test_ar_small_selection_equals_the_host_batch(kw):
    o = host.default_opts(**kw)
    P = abi.default_params()
    n, out = _scan(sc.fixture_paths("ar_small"), "chr22:900-3000" if "padding" not in kw else "chr22:1200-1900", o, P)
    assert out[0][0]["rc"] == 0 and 0 < len(out[0][1]["kept"]) <= n and out[0][1]["rinfo"].size > 100
    # the same windows in batches of five, and with small limits of the LDS build configuration (the size test counts some windows)
    n, parts = _scan(sc.fixture_paths("ar_small"), "chr22:900-3000" if "padding" not in kw else "chr22:1200-1900", o, P, step=5, lds=(60, 8192))
    assert all(g["rc"] == 0 for g, _ in parts) and sum((w["kept"] for _, w in parts), []) == out[0][1]["kept"]
    assert sum(g["need_large"] for g, _ in parts) > 0


@pytest.mark.parametrize("case", sorted(FLT_CASES))
def test_read_filter_fixtures_selection_equals_the_host_batch(case):
    region, opts, _, linked = FLT_CASES[case]
    P = abi.default_params()
    if linked:                                          # --linked-reads goes through the host route, and says so
        o = host.default_opts(**opts)
        n, out = _scan(sc.fixture_paths(case), region, o, P)
        assert out[0][0]["rc"] == abi.LANCET_NOT_TAKEN and "linked" in out[0][0]["reason"]
        opts = dict(opts, linked=0)
    o = host.default_opts(**opts)
    n, out = _scan(sc.fixture_paths(case), region, o, P)
    assert out[0][0]["rc"] == 0 and len(out[0][1]["kept"]) > 15


def test_every_option_set_of_flt_small_selection_equals_the_host_batch():
    """tests/golden/flt_small.options.txt: fifteen option sets of the reference (tiling, coverage cut-off -- some sets skip windows --,
    MAPQ, active-region thresholds, XA / primary-alignment filters); the windows and read counts are the reference's own."""
    spec = json.load(open(os.path.join(G, "flt_small.options.txt")))
    P = abi.default_params()
    skipped_any = False
    for optstr, ref_windows in spec["option_sets"].items():
        toks, kw, i = optstr.split(), {}, 0
        while i < len(toks):
            if toks[i] in _OPT_FLAGS:
                kw[_OPT_FLAGS[toks[i]][0]] = _OPT_FLAGS[toks[i]][1]; i += 1
            else:
                field, conv = _OPT_MAP[toks[i]]
                if field:
                    kw[field] = conv(toks[i + 1])
                i += 2
        o = host.default_opts(**kw)
        n, out = _scan(sc.fixture_paths("flt_small"), spec["region"], o, P)
        got, want = out[0]
        assert got["rc"] == 0, (optstr, got["reason"])
        assert [int(x) for x in np.diff(got["read_begin"].astype(np.int64))] == [int(w.split()[1]) for w in ref_windows], optstr
        skipped_any |= bool(((got["summaries"][:, 0] & 3) == 2).any())
    assert skipped_any                                  # (a --max-avg-cov set skipped windows)


def test_bed2_two_contigs_selection_equals_the_host_batch():
    case = json.load(open(os.path.join(G, "bed2.case.txt")))
    o = host.default_opts()
    P = abi.default_params()
    for step in (None, 9):
        n, out = _scan(sc.fixture_paths("bed2"), case["region"], o, P, step=step, bed=os.path.join(G, "bed2.bed"))
        assert all(g["rc"] == 0 for g, _ in out)
        chr_ids = np.concatenate([w["chr_id"] for _, w in out])
        assert sum(len(w["kept"]) for _, w in out) == 32 and set(chr_ids.tolist()) == {0, 1}      # (reads of the other contig never enter: equal to the host batch)


def test_rec_low_selection_equals_the_host_batch():
    o = host.default_opts()
    n, out = _scan(sc.fixture_paths("rec_low"), "chr22:900-2700", o, abi.default_params())
    assert out[0][0]["rc"] == 0 and len(out[0][1]["kept"]) > 3
    # packed for other thresholds: the table's words and trimmed lengths follow
    n, out2 = _scan(sc.fixture_paths("rec_low"), "chr22:900-2700", o, abi.default_params(min_qual_trim=33 + 25, min_qual_call=33 + 30))
    assert out2[0][0]["rc"] == 0 and not np.array_equal(out2[0][1]["rinfo"], out[0][1]["rinfo"])


@pytest.mark.parametrize("seed", [0, 2])
def test_randomized_bams_with_filtered_reads_selection_equals_the_host_batch(tmp_path, seed):
    """The randomized BAMs of test_host_native.py: XT / XA / XS tags, duplicates, secondary alignments, low MAPQ, soft clips, unmapped flags."""
    rng = np.random.default_rng(400 + seed)
    data = synth.make_tumor_normal(ref_len=6000, cov_t=25, cov_n=20, ref_seed=30 + seed, tumor_seed=130 + seed, normal_seed=230 + seed,
                                   somatic_every=500, germline_every=400, str_fraction=0.05 if seed == 2 else 0.0)
    tumor = read_variety.decorate(synth.pairs_to_sorted_reads(data["tumor"]), rng, False)
    normal = read_variety.decorate(synth.pairs_to_sorted_reads(data["normal"]), rng, False)
    refs = [("chrA", 1000), (data["rname"], len(data["ref"]))]
    tb, nb, fa = str(tmp_path / "t.bam"), str(tmp_path / "n.bam"), str(tmp_path / "r.fa")
    bam_writer.write_bam(tb, refs, tumor, sample="TT")
    bam_writer.write_bam(nb, refs, normal, sample="NN")
    synth.write_fasta(fa, "chrA", "ACGT" * 250)
    with open(fa, "a") as fh:
        fh.write(f">{data['rname']}\n{data['ref']}\n")
    P = abi.default_params()
    taken = 0
    for kw in ({}, {"active_region": 0, "primary_alignment_only": 1, "xa_filter": 1, "min_map_qual": 10}, {"max_avg_cov": 20, "active_region": 0}):
        o = host.default_opts(**kw)
        n, out = _scan([tb, nb, fa], f"{data['rname']}:700-5200", o, P, step=6)
        for got, want in out:
            # a batch whose windows hold reads but no mapped read is the one case the route leaves to the host: it must say so
            assert got["rc"] == 0 or "leak" in got["reason"], got["reason"]
            taken += got["rc"] == 0
    assert taken > 10


@pytest.mark.parametrize("name", sorted(sc.synthetic_cases()))
def test_synthetic_single_window_cases(tmp_path, name):
    tumor, normal, kw, expect = sc.synthetic_cases()[name]
    o = host.default_opts(padding=0, **kw)
    P = abi.default_params()
    H = sc.open_case(sc.write_case(str(tmp_path), tumor, normal), o)
    got, want = _check_range(H, 0, 1, o, P)
    H.close()
    assert got["rc"] == 0
    status = int(got["summaries"][0][0]) & 3
    assert {"kept": 1, "filtered": 0, "skipped": 2}[expect] == status and len(want["kept"]) == (1 if expect == "kept" else 0)
    if name == "names_r1_r10_r2":                       # tumor r10 r2 r1 | normal r2 r1, ranked under strcmp: r1 < r10 < r2
        assert got["name_rank"].tolist() == [1, 2, 0, 2, 0]
    if name == "three_reads_of_one_name":
        assert got["name_rank"].tolist() == [1, 0, 1, 2, 1, 1]
    if name == "names_equal_in_8_bytes":                # readname < readnameXYZ < readname_ < readname_a < readname_ab < readname_b
        assert got["name_rank"].tolist() == [5, 0, 3, 1, 2, 3, 4]
    if name == "no_candidate":
        assert got["read_begin"].tolist() == [0, 0]
    if name == "reads_in_one_sample_only":
        assert tuple(int(x) for x in got["summaries"][0][1:3]) == (0, 2)


def test_more_reads_or_evidence_than_the_kernel_stages_is_not_taken(tmp_path):
    cap, hcap = select_emu.caps()
    many = [sc.read(f"q{i:05d}", 520 + (i % 250)) for i in range(cap + 1)]
    o = host.default_opts(padding=0, active_region=0)
    H = sc.open_case(sc.write_case(str(tmp_path / "a"), many, []), o)
    got, _ = _check_range(H, 0, 1, o, abi.default_params())
    H.close()
    assert got["rc"] == abi.LANCET_NOT_TAKEN and "oversize" in got["reason"]
    # exactly the staged number is taken (and sorted: the names are unique, the ranks a permutation)
    H = sc.open_case(sc.write_case(str(tmp_path / "b"), many[:cap], []), o)
    got, _ = _check_range(H, 0, 1, o, abi.default_params())
    H.close()
    assert got["rc"] == 0 and sorted(got["name_rank"].tolist()) == list(range(cap))
    # more distinct evidence positions than counters, none reaching the threshold: the window's state is unknown -> not taken.
    # (hard clips move isActiveRegion's position without using read bases: read i counts its insertion at 600 + i + 10)
    for n_reads, taken in ((hcap // 2, True), (hcap + 200, False)):
        noisy = [sc.read(f"e{i:04d}", 601, cigar=f"{i + 1}H10M1I10M", md="20") for i in range(n_reads)]
        o = host.default_opts(padding=0, min_evidence=100000)
        H = sc.open_case(sc.write_case(str(tmp_path / f"c{n_reads}"), noisy, []), o)
        tab = H.alignment_table(o, abi.default_params())
        ne = int(tab.evt_off[n_reads])
        distinct = len({(int(k), int(p)) for k, p in zip(np.ctypeslib.as_array(tab.evt_kind, shape=(ne,)), np.ctypeslib.as_array(tab.evt_pos, shape=(ne,)))})
        assert (distinct > hcap) == (not taken) and distinct >= n_reads
        got, want = _check_range(H, 0, 1, o, abi.default_params())
        H.close()
        if taken:
            assert got["rc"] == 0 and want["kept"] == [] and (int(got["summaries"][0][0]) & 3) == 0
        else:
            assert got["rc"] == abi.LANCET_NOT_TAKEN and "oversize" in got["reason"]
    # ... a position that reached the threshold before the table filled up makes the window active whatever is dropped later
    noisy = [sc.read(f"s{i}", 601, cigar="10M1I10M", md="20") for i in range(3)] + [sc.read(f"e{i:04d}", 601, cigar=f"{i + 1}H10M1I10M", md="20") for i in range(hcap + 200)]
    o = host.default_opts(padding=0, min_evidence=3, max_avg_cov=1000000)
    H = sc.open_case(sc.write_case(str(tmp_path / "d"), noisy, []), o)
    got, want = _check_range(H, 0, 1, o, abi.default_params(), lds=(4096, 1 << 20))
    H.close()
    assert got["rc"] == abi.LANCET_NOT_TAKEN and "oversize: a window selects" in got["reason"] and want["kept"] == [0]      # (kept by the host; too many READS for pass 2)


def test_leak_small_ranges_with_the_read_leak_go_to_the_host_route():
    """`leak_small`: windows 6, 7, 8 (counted from 1) hold reads but no mapped read, window 9 inherits them.  The ranges before the run are
    taken; the range that holds the run is NOT TAKEN; the scan stitched from both routes equals the host route's batches -- also when it
    starts inside the leaking run."""
    paths = sc.fixture_paths("leak_small")
    o = host.default_opts(active_region=0)
    P = abi.default_params()
    H0 = host.NativeHost(*paths)
    n = len(H0.tile("chr22:1000-3000", o))
    H0.close()
    for first in (0, 6):
        H = host.NativeHost(*paths)                     # the stitched scan
        Hh = host.NativeHost(*paths)                    # the host route alone
        assert len(H.tile("chr22:1000-3000", o)) == n == len(Hh.tile("chr22:1000-3000", o))
        taken = []
        for lo in range(first, n, 4):
            hi = min(n, lo + 4)
            want = sc.host_expectation(Hh, lo, hi, o, P)
            tab = H.alignment_table(o, P)
            sl = H.windows(lo, hi, o)
            got = select_emu.run(tab, sl, o)
            taken.append(got["rc"] == 0)
            if got["rc"] == 0:
                sc.assert_same(got, want, sc.table_words(tab))
                H.windows_done(lo, hi)
            else:
                assert "leak" in got["reason"]
                mine = sc.host_expectation(H, lo, hi, o, P)              # this batch through the host route of the SAME host object
                for f in ("kept", ):
                    assert mine[f] == want[f]
                for f in ("read_begin", "rinfo", "name_rank", "base_words", "good_words"):
                    assert np.array_equal(mine[f], want[f]), f
        if first == 0:
            assert taken == [True, False, False] + [True] * (len(taken) - 3)      # windows [4, 8) hold the run, [8, 12) inherit its reads
        else:
            assert taken[0] is False                    # the scan starts inside the run: its first range has reads entering
        H.close(); Hh.close()
    # done is legal only for the range the slice was made for
    H = host.NativeHost(*paths)
    H.tile("chr22:1000-3000", o)
    H.windows(0, 4, o)
    with pytest.raises(engine.EngineError):
        H.windows_done(0, 3)
    H.windows_done(0, 4)
    H.close()


def test_rg_file_and_batch_by_batch_loading_are_not_taken(tmp_path, monkeypatch):
    paths = [os.path.join(G, f"rg_small.{x}") for x in ("tumor.bam", "normal.bam", "fa")]
    o = host.default_opts()
    P = abi.default_params()
    H = host.NativeHost(*paths)
    H.set_rg_file(os.path.join(G, "rg_small.rg.txt"))
    n = len(H.tile("chr22:900-3100", o))
    got, _ = _check_range(H, 0, n, o, P)
    assert got["rc"] == abi.LANCET_NOT_TAKEN and "rg-file" in got["reason"]
    H.close()
    H = host.NativeHost(*paths)                         # without the file the same input is taken
    H.tile("chr22:900-3100", o)
    assert _check_range(H, 0, n, o, P)[0]["rc"] == 0
    H.close()
    # lazy loading: taken inside lancet_host_load_range's range, not taken without it; a table of another load is refused
    from lancet_amd import bamio
    lp = []
    for nm, sample in (("tumor", "TUMOR"), ("normal", "NORMAL")):
        hdr, reads = bamio.read_bam(os.path.join(G, f"ar_small.{nm}.bam"))
        out = str(tmp_path / (nm + ".bam"))
        bam_writer.write_bam(out, hdr["refs"], reads, sample=sample, index=True)
        lp.append(out)
    lp.append(os.path.join(G, "ar_small.fa"))
    monkeypatch.setenv("LANCET_HOST_LAZY", "1")
    H = host.NativeHost(*lp)
    n = len(H.tile("chr22:900-3000", o))
    sl = H.windows(0, 5, o)
    assert sl.host_reason == 2
    got = select_emu.run(H.alignment_table(o, P), sl, o)
    assert got["rc"] == abi.LANCET_NOT_TAKEN and "not loaded" in got["reason"]
    H.load_range(0, n, o)
    old = H.alignment_table(o, P)
    old_id = int(old.load_id)
    assert _check_range(H, 0, 6, o, P)[0]["rc"] == 0 and _check_range(H, 6, n, o, P)[0]["rc"] == 0
    H.load_range(3, n, o)                               # a reload: the table made before it is of another load
    tab = H.alignment_table(o, P)
    assert int(tab.load_id) != old_id
    stale = abi.LancetAlignmentTable.from_buffer_copy(tab)
    stale.load_id = old_id
    got = select_emu.run(stale, H.windows(3, n, o), o)
    assert got["rc"] == abi.LANCET_NOT_TAKEN and "another load" in got["reason"]
    H.close()


def test_a_rank_s_own_load_of_two_contigs(monkeypatch):
    """--ranks: every rank loads the range it owns (lancet_host_load_range, batch-by-batch loading) and exports that.  A load can hold
    nothing of a contig the tiling knows: its span in the table is empty, inside the sample."""
    case = json.load(open(os.path.join(G, "bed2.case.txt")))
    monkeypatch.setenv("LANCET_HOST_LAZY", "1")
    o = host.default_opts()
    P = abi.default_params()
    H = host.NativeHost(*sc.fixture_paths("bed2"))
    n = len(H.tile_regions([case["region"]], o, bed=os.path.join(G, "bed2.bed")))
    kept = 0
    for lo, hi in ((0, n // 3), (n // 3, n)):
        H.load_range(lo, hi, o)
        for b0 in range(lo, hi, 9):
            got, want = _check_range(H, b0, min(hi, b0 + 9), o, P)
            assert got["rc"] == 0, got["reason"]
            kept += len(want["kept"])
    assert kept == 32
    H.close()


def test_new_symbols_struct_sizes_and_no_device():
    import torch
    L = engine.lib()
    for sym in ("lancet_host_alignment_table", "lancet_host_windows", "lancet_host_windows_done", "lancet_device_reads_create", "lancet_device_reads_destroy",
                "lancet_device_reads_bytes", "lancet_engine_upload_windows", "lancet_engine_debug_select", "lancet_engine_debug_batch"):
        assert hasattr(L, sym), sym
    assert C.sizeof(abi.LancetAlignmentTable) == 168 and C.sizeof(abi.LancetWindowSlice) == 72 and C.sizeof(abi.LancetSelectSummary) == 24
    paths = sc.fixture_paths("flt_small")
    o = host.default_opts(**FLT_CASES["flt_small"][1])
    H = host.NativeHost(*paths)
    H.tile(FLT_CASES["flt_small"][0], o)
    tab = H.alignment_table(o, abi.default_params())
    assert tab.struct_size == C.sizeof(abi.LancetAlignmentTable) and H.windows(0, 3, o).struct_size == C.sizeof(abi.LancetWindowSlice)
    t = sc.table_arrays(tab)
    assert t["n"] > 500 and 0 < int((t["flags"] & 1).sum()) < t["n"] and int(t["evt_off"][-1]) > 0
    assert not (t["rinfo"][(t["flags"] & 1) == 0]).any()                  # only selectable alignments are trimmed and packed
    bad = abi.LancetAlignmentTable.from_buffer_copy(tab)
    bad.struct_size = 8
    h = C.c_void_p()
    assert L.lancet_device_reads_create(0, C.byref(bad), C.byref(h)) == -1 and not h.value
    if not torch.cuda.is_available():                   # there is no CPU path: loud, not a fallback
        assert L.lancet_device_reads_create(0, C.byref(tab), C.byref(h)) == -2 and not h.value
        with pytest.raises(engine.EngineError, match="no HIP device"):
            engine.DeviceReads(tab, 0)
    H.close()
