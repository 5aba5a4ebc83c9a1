"""Haplotype capture (lancet_engine_set_haplotypes) without a GPU: the emulated kernels with the capture (tests/hap_emu: tests/emu's driver,
the buffers handed to the kernels through the emulation's sink), on the one-wave form and on the LANCET_FAT form, against the `p:` / `r:`
lines the REFERENCE ITSELF printed under -V (tests/golden/more_verbose/) and against the run's own records (tests/hap_cases.py).
test_haplotypes_gpu.py holds the engine to the same."""
import ctypes
import os
import re
import sys

import pytest

import hap_cases as hc
import more_verbose_util as mv
import walk_cases as wc
from lancet_amd import abi, cli

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hap_emu"))
import hap_emu  # noqa: E402
from hap_emu import emu  # noqa: E402

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def build(request):
    emu.FAT[0] = request.param == "fat"
    yield request.param
    emu.FAT[0] = False


def _run(batch, p, words, evt_cap=0):
    v, st, text, haps, trunc = hap_emu.run(batch, p, evt_cap=evt_cap, hap_words=words)
    return v, st, haps, trunc, text


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
@pytest.mark.parametrize("case", mv.CASES)
def test_haplotypes_are_the_references_path_lines(case, build):
    """Default route (LDS build kernel, graphs built ahead, build service): strings and stretches are the golden's, the ranges tile the
    window's records and replay onto the stretch, and records and stats are those of a run without the capture."""
    m, batch, kept = mv.case_batch(case)
    p = mv.params(m)
    v, st, haps, trunc, _ = _run(batch, p, hc.ample_words(batch, p))
    assert emu.LAST_PREBUILT[0] > 0
    hc.check_goldens(case, batch, st, haps, trunc)
    hc.check_link(batch, v, st, haps)
    v0, st0, _ = emu.run(batch, p)
    assert v == v0 and [hc.KEY(s) for s in st] == [hc.KEY(s) for s in st0]
    # ... of which the capture-off run of the library with the capture is one: nothing comes back
    v1, st1, haps1, trunc1, _ = _run(batch, p, 0)
    assert v1 == v0 and haps1 == [] and trunc1 == [0] * batch.n_windows


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
@pytest.mark.parametrize("prebuild", ["default", "no_prebuild"])
@pytest.mark.parametrize("case", ["mv_dups", "mv_nref"])
def test_capture_does_not_depend_on_the_build_route(case, prebuild, build, monkeypatch):
    """The strings of a capture run equal the EV_ALN strings of a level-2 run of the same batch (level 2 takes the general build), with the
    LDS build kernel and without it; and capture and level 2 together give both, unchanged."""
    m, batch, kept = mv.case_batch(case)
    p = mv.params(m)
    cap = mv.trace_words(batch, p)
    monkeypatch.setenv("LANCET_NO_PREBUILD", "1")
    monkeypatch.setenv("LANCET_TRACE_LEVEL", "2")
    v2, st2, haps2, trunc2, _ = _run(batch, p, hc.ample_words(batch, p), evt_cap=cap)     # both at once
    events = [e.copy() for e in emu.LAST_EVENTS]
    _, _, _ = emu.run(batch, p, evt_cap=cap)                                               # level 2 alone
    assert all((a == b).all() for a, b in zip(events, emu.LAST_EVENTS)) and len(events) == len(emu.LAST_EVENTS)      # not a trace word changed
    monkeypatch.delenv("LANCET_TRACE_LEVEL")
    if prebuild == "default":
        monkeypatch.delenv("LANCET_NO_PREBUILD")
    texts = mv.window_texts(batch, events, cap, p)
    want = [[l[4:] for l in t.splitlines() if l.startswith("p:  ")] for t in texts]
    want_r = [[l[4:] for l in t.splitlines() if l.startswith("r:  ")] for t in texts]
    v, st, haps, trunc, _ = _run(batch, p, hc.ample_words(batch, p))
    assert (emu.LAST_PREBUILT[0] > 0) == (prebuild == "default")
    for got in (haps, haps2):
        assert [[h["seq"] for h in got if h["window"] == w] for w in range(batch.n_windows)] == want
        assert [[hc.stretch(batch, h) for h in got if h["window"] == w] for w in range(batch.n_windows)] == want_r
    assert haps == haps2 and v == v2 and [hc.KEY(s) for s in st] == [hc.KEY(s) for s in st2] and not any(trunc) and not any(trunc2)


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
def test_word_edges(build, monkeypatch):
    """Path strings of 63, 64, 65, 79, 80 and 81 bases into buffers that start as 0xCD: whole words, the part of a word, nothing above it."""
    batch, p = hc.edge_batch()
    for route in ("default", "general"):
        if route == "general":
            monkeypatch.setenv("LANCET_NO_PREBUILD", "1")
        v, st, haps, trunc, _ = _run(batch, p, 64)
        hc.check_edges(batch, v, st, haps, trunc)
    # the smallest buffers that hold each window's one entry, and one word less
    need = max(hc.words_of(h) for h in haps)
    v, st, haps, trunc, _ = _run(batch, p, need)
    hc.check_edges(batch, v, st, haps, trunc)
    v, st, haps1, trunc1, _ = _run(batch, p, need - 1)
    assert [h["window"] for h in haps1] == [w for w, L in enumerate(hc.EDGE_LENS) if hc.HDR + (L + 15) // 16 <= need - 1]
    assert trunc1 == [0 if hc.HDR + (L + 15) // 16 <= need - 1 else 1 for L in hc.EDGE_LENS] and v == []


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
def test_a_window_whose_haplotypes_do_not_fit(build):
    m, batch, kept = mv.case_batch("mv_dups")
    p = mv.params(m)
    v, st, haps, trunc, text = _run(batch, p, hc.ample_words(batch, p), evt_cap=1 << 17)
    w, cap = hc.truncation_plan(haps)
    cv, cst, ch, ct, ctext = _run(batch, p, cap, evt_cap=1 << 17)
    hc.check_truncated(batch, w, cap, (v, st, haps, trunc), (cv, cst, ch, ct))
    assert ctext == text                                                                    # the level-1 trace: not a line
    assert all(s["status"] >= 0 for s in cst)                                               # never an overflow
    # too small for a single header: refused when it is set
    for bad in (1, hc.HDR - 1, hc.HDR):
        assert hap_emu.set_words(bad) == -1                                                 # LANCET_E_ARG
    assert hap_emu.set_words(hc.HDR + 1) == 0 and hap_emu.set_words(0) == 0


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
@pytest.mark.parametrize("case", ["mv_dups", "mv_rec"])
def test_rerun_tier_reports_every_haplotype_once(case, build, monkeypatch):
    """A tier 1 of 64 nodes per window: windows overflow there after some of their paths were written, the second tier starts them over in the
    same buffers (tests/hap_emu/emu_hap.cc runs the two tiers over one set of buffers)."""
    m, batch, kept = mv.case_batch(case)
    p = mv.params(m)
    words = hc.ample_words(batch, p)
    want = _run(batch, p, words)[:4]
    monkeypatch.setenv("LANCET_EMU_TIER1", "64")
    _, st1, _ = emu.run(batch, p)
    assert sum(1 for s in st1 if s["status"] < 0) >= 2                                      # tier 1 alone does overflow
    got = _run(batch, p, words)[:4]
    assert got[0] == want[0] and [hc.KEY(s) for s in got[1]] == [hc.KEY(s) for s in want[1]] and got[2:] == want[2:]
    hc.check_goldens(case, batch, got[1], got[2], got[3])


def test_struct_and_defaults():
    """The ctypes struct is the C one; the header, the binding and the emulator agree on the header words."""
    assert ctypes.sizeof(abi.LancetHaplotype) == hap_emu.lib().lancet_hap_emu_struct_size() == 40
    src = open(os.path.join(_ROOT, "include", "lancet_engine.h")).read()
    assert int(re.search(r"#define LANCET_HAP_HEADER_WORDS (\d+)", src).group(1)) == abi.HAP_HEADER_WORDS
    layout = open(os.path.join(_ROOT, "lancet_amd", "csrc", "layout.h")).read()
    assert int(re.search(r"#define HP_HDR (\d+)u", layout).group(1)) == abi.HAP_HEADER_WORDS
    fields = re.search(r"typedef struct lancet_haplotype \{(.*?)\} lancet_haplotype;", src, re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [f[0] for f in abi.LancetHaplotype._fields_]


def test_product_library_exports_the_calls_and_keeps_its_state_rules():
    """The symbols are in liblancet_engine.so; without an engine both refuse a null handle (the state rules need a device:
    test_haplotypes_gpu.py)."""
    from lancet_amd import build as _build, engine
    _build.build()
    L = engine.lib()
    assert L.lancet_engine_set_haplotypes(None, 64) == -1 and L.lancet_engine_results_haplotypes(None, None, None, None, None, None) == -1
    assert L.lancet_engine_haplotype_readback_ms(None) == 0.0


def test_python_cli_does_not_get_the_option():
    ap = cli.build_parser()
    with pytest.raises(SystemExit):
        ap.parse_args(["--tumor", "t.bam", "--normal", "n.bam", "--ref", "r.fa", "--reg", "chr22:1-10", "--haplotypes", "h.fa"])


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
@pytest.mark.parametrize("case", wc.CASES)
def test_one_haplotype_per_path_under_both_walk_drivers(case, build, monkeypatch):
    """The hand-made windows of tests/walk_cases.py (paths that spell the reference, paths with 1..5 mismatches that skip the alignment, aligned
    paths; many_ts: a path the wave driver gives up at WALK_FULL and the one-lane driver redoes): one haplotype per path, its record range
    closed once, the same under the one-lane walk driver (LANCET_OLD_WALK)."""
    batch, p = wc.make(case)
    got = {}
    for old in (False, True):
        if old:
            monkeypatch.setenv("LANCET_OLD_WALK", "1")
        v, st, haps, trunc, _ = _run(batch, p, hc.ample_words(batch, p))
        hc.check_shape(batch, st, haps, trunc)
        hc.check_link(batch, v, st, haps)
        got[old] = (v, haps, trunc)
    assert got[False] == got[True] and not any(got[False][2])
    assert len(got[False][1]) == len(wc.PATHS[case])
    for h, (m_, s_, i_, d_) in zip(got[False][1], wc.PATHS[case]):                          # lengths as the `>p_` line counts them
        assert h["ref_len"] == m_ + s_ + d_ and h["len"] == m_ + s_ + i_
        assert bool(h["flags"] & abi.HAP_IS_REF) == (s_ + i_ + d_ == 0)
