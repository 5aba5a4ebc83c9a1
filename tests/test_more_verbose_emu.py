"""-V / --more-verbose without a GPU: the emulated kernels (tests/emu) at trace level 2 against what the REFERENCE ITSELF printed under -V
(tests/golden/more_verbose/, tools/make_more_verbose_goldens.py), on the one-wave form and on the LANCET_FAT form (the re-run tier's source).

The level reaches the emulated kernels through the shared caps helper (host_common.h lc_caps_for_sizes reads LANCET_TRACE_LEVEL), the build
route through LANCET_NO_PREBUILD, which the engine's level 2 implies (engine.hip lancet_engine_set_trace_level): both are set here.

The -V lines (reference src/Graph.cc): `cycle detected in read` :328-332, `refid:` :539, `Looking at` :2030-2034, `checking for other ... edges`
and `  removing node ...` :2168-2213, `alignment` / `r:` / `p:` :800-802."""
import os
import sys

import pytest

import golden_util as gu
import more_verbose_util as mv
import walk_cases as wc
from lancet_amd import abi, cli, trace
from oracle import oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402

_KEY = lambda s: (s["status"], s["final_k"], s["n_builds"], s["n_variants"], s["n_kmers"], s["max_nodes"])


@pytest.fixture
def build(request):
    emu.FAT[0] = request.param == "fat"
    yield request.param
    emu.FAT[0] = False


def _level2(monkeypatch, batch, p, cap):
    """(variants, stats, text per window, raw event words per window) of a level-2 run."""
    monkeypatch.setenv("LANCET_NO_PREBUILD", "1")
    monkeypatch.setenv("LANCET_TRACE_LEVEL", "2")
    v, st, _ = emu.run(batch, p, evt_cap=cap)
    events = [e.copy() for e in emu.LAST_EVENTS]
    monkeypatch.delenv("LANCET_NO_PREBUILD")
    monkeypatch.delenv("LANCET_TRACE_LEVEL")
    return v, st, mv.window_texts(batch, events, cap, p), events


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
@pytest.mark.parametrize("case", mv.CASES)
def test_level2_text_is_the_references(case, build, monkeypatch):
    m, batch, kept = mv.case_batch(case)
    p = mv.params(m)
    cap = mv.trace_words(batch, p)
    v, st, texts, events = _level2(monkeypatch, batch, p, cap)
    text = "".join(texts)
    assert all(len(e) < cap for e in events)                                     # no window truncated at the size lancet_gpu would give it
    assert mv.digest(text) == mv.golden_trace(case)                              # line for line, in the reference's order
    # records and stats: the oracle's where it applies (it knows nothing of -R), the VCF the reference wrote in every case
    assert all(s["status"] >= 0 for s in st)
    if not m["recovery"]:
        ov, ost, _ = oracle.run(batch, p)
        assert v == ov and [_KEY(s) for s in st] == [_KEY(s) for s in ost]
    assert mv.records_vcf(batch, v, lr=gu.case_lr(m), bx_names=getattr(batch, "bx_names", None)) == mv.golden_vcf(case)
    # level 1 of the same batch: the -v digest the reference wrote; the same text with the LDS build kernel and without; and what level 2
    # adds to it is lines of its own, nothing else
    v1, st1, t1 = emu.run(batch, p, evt_cap=1 << 17)
    assert gu.digest_trace(t1) == mv.digest_v(mv.golden_trace(case))
    monkeypatch.setenv("LANCET_NO_PREBUILD", "1")
    v1g, st1g, t1g = emu.run(batch, p, evt_cap=1 << 17)
    assert t1g == t1 and v1g == v1 == v and [_KEY(s) for s in st1] == [_KEY(s) for s in st1g] == [_KEY(s) for s in st]
    assert "".join(l + "\n" for l in text.splitlines() if not l.startswith(mv.V_PREFIXES)) == t1
    # a level-1 stream holds none of the new events
    assert all(int(e[i]) < trace.EV_REFID for e in emu.LAST_EVENTS for i in _event_starts(e))


def _event_starts(words):
    """Indices of the event records of a LEVEL-1 stream (the byte blocks after EV_TS skipped as trace.format_window skips them)."""
    i, out = 0, []
    while i + 8 <= len(words):
        out.append(i)
        code, b = int(words[i]), int(words[i + 2])
        i += 8
        if code == trace.EV_TS:
            i += 2 * (((b + 3) // 4 + 7) // 8 * 8) + 8
    return out


def test_fixture_set_covers_what_the_lines_depend_on():
    """The generator's check_set, on the committed files: without these the digests above could not tell a missing line."""
    tot = {}
    metas = {c: mv.meta(c) for c in mv.CASES}
    for c, m in metas.items():
        for k, n in m["lines"].items():
            tot[k] = tot.get(k, 0) + n
        assert 8 <= m["n_windows"] <= 20
    assert tot["before_source"] >= 1 and tot["after_sink"] >= 1 and tot["aligned"] >= 1 and tot["ref_spelling"] >= 1 and tot["mismatch_1_5"] >= 1
    assert any(m["synth"].get("read_len") == 100 and m["synth"].get("dup_prob") and m["lines"]["rebuilds"] >= 3 and m["lines"]["cycle"] >= 20 for m in metas.values())
    assert any(m["synth"].get("n_runs") for m in metas.values())
    assert any("--linked-reads" in m["flags"] for m in metas.values()) and any(m["recovery"] for m in metas.values())
    assert sum(1 for m in metas.values() if m["cli"]) == 1
    for f in os.listdir(mv.DIR):
        assert os.path.getsize(os.path.join(mv.DIR, f)) < (1 << 20), f


@pytest.mark.parametrize("case", mv.CASES)
def test_every_path_string_is_its_transcripts_replayed_onto_the_reference(case, monkeypatch):
    """Needs no reference: the p: line of a path is its r: line with the transcripts of its `>p_` line applied."""
    m, batch, kept = mv.case_batch(case)
    p = mv.params(m)
    _, _, texts, _ = _level2(monkeypatch, batch, p, mv.trace_words(batch, p))
    pairs = mv.replay_paths("".join(texts))
    assert len(pairs) == sum(1 for l in mv.golden_trace(case).splitlines() if l.startswith("p:  "))      # every path has its three lines
    assert pairs and all(pl is not None and pl == made for pl, made in pairs)


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
@pytest.mark.parametrize("case", wc.CASES)
def test_both_walk_drivers_write_a_path_once(case, build, monkeypatch):
    """The hand-made windows of tests/walk_cases.py (paths that spell the reference, paths with 1..5 mismatches that skip the alignment, aligned
    paths; many_ts: a path the wave driver gives up at WALK_FULL and the one-lane driver redoes): every `>p_` line has exactly one
    `alignment` / `r:` / `p:` group in front of it, the p: line is the transcripts replayed onto the r: line, and the one-lane walk driver
    (LANCET_OLD_WALK) gives the same text as the wave driver."""
    batch, p = wc.make(case)
    cap = mv.trace_words(batch, p)
    texts = {}
    for old in (False, True):
        if old:
            monkeypatch.setenv("LANCET_OLD_WALK", "1")
        texts[old] = "".join(_level2(monkeypatch, batch, p, cap)[2])
    monkeypatch.delenv("LANCET_OLD_WALK")
    assert texts[False] == texts[True]
    lines = texts[False].splitlines()
    heads = [i for i, l in enumerate(lines) if l.startswith(">p_")]
    assert len(heads) == len(wc.PATHS[case]) == sum(1 for l in lines if l == "alignment") == sum(1 for l in lines if l.startswith("p:  "))
    for i in heads:
        assert lines[i - 3] == "alignment" and lines[i - 2].startswith("r:  ") and lines[i - 1].startswith("p:  ")
    pairs = mv.replay_paths(texts[False])
    assert len(pairs) == len(heads) and all(pl == made for pl, made in pairs)
    # lengths as the `>p_` line counts them: match + snp + del columns of r, match + snp + ins of p
    for i, (m_, s_, i_, d_) in zip(heads, wc.PATHS[case]):
        assert len(lines[i - 2]) - 4 == m_ + s_ + d_ and len(lines[i - 1]) - 4 == m_ + s_ + i_
    _, _, t1 = emu.run(batch, p, evt_cap=1 << 16)
    assert "".join(l + "\n" for l in lines if not l.startswith(mv.V_PREFIXES)) == t1


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
def test_a_window_whose_events_do_not_fit_says_so(build, monkeypatch):
    """words_per_window between the needs of a batch's windows: the windows that need more end with the truncation line after whole events,
    the others are complete.  (The fixture with the cycle lines: its windows need between a few hundred and a few thousand words.)"""
    m, batch, kept = mv.case_batch("mv_dups")
    p = mv.params(m)
    full_cap = mv.trace_words(batch, p)
    _, st_full, full, ev_full = _level2(monkeypatch, batch, p, full_cap)
    need = sorted(len(e) for e in ev_full)
    cap = (need[len(need) // 2] + 8 + 7) // 8 * 8                                # the median window just fits (eight words are the mark's)
    assert need[0] + 8 <= cap < need[-1] + 8
    v, st, texts, events = _level2(monkeypatch, batch, p, cap)
    assert [_KEY(s) for s in st] == [_KEY(s) for s in st_full]                   # the trace never changes what is computed
    cut = whole = 0
    for w in range(batch.n_windows):
        if len(ev_full[w]) + 8 <= cap:
            assert texts[w] == full[w] and len(events[w]) == len(ev_full[w])
            whole += 1
        else:
            assert len(events[w]) == cap and int(events[w][cap - 8]) == trace.EV_TRUNC and int(events[w][cap - 7]) <= cap - 8
            lines, want = texts[w].splitlines(), full[w].splitlines()
            assert lines[-1] == f"[trace truncated: window {w + 1} needs more than {cap} trace words]"
            assert lines[:-2] == want[:len(lines) - 2] and len(lines) - 2 < len(want)     # (the line before the mark may be cut: a transcript's strings follow its event)
            assert list(events[w][:int(events[w][cap - 7])]) == list(ev_full[w][:int(events[w][cap - 7])])
            cut += 1
    assert cut >= 1 and whole >= 1
    # the smallest buffer level 2 takes: every window with events is cut, nothing is written past the buffer
    _, st16, t16, e16 = _level2(monkeypatch, batch, p, 16)
    assert [_KEY(s) for s in st16] == [_KEY(s) for s in st_full]
    assert all(len(e) == 16 and int(e[8]) == trace.EV_TRUNC and int(e[9]) == 8 for e in e16)
    assert all(t.splitlines()[-1].startswith("[trace truncated: ") for t in t16)
    # level 1 keeps dropping what does not fit, silently: no mark, and a length below the capacity
    _, _, t1 = emu.run(batch, p, evt_cap=cap)
    assert "[trace truncated" not in t1 and all(len(e) <= cap for e in emu.LAST_EVENTS)


@pytest.mark.parametrize("case", ["mv_dups", "mv_nref"])
def test_native_formatter_matches_the_python_one_at_level_2(case, monkeypatch):
    """lancet_trace_format2 (host C++, what `lancet_gpu -V` prints) against lancet_amd/trace.py format_window2 on the level-2 event streams of
    the emulated kernels, whole and truncated: every window, byte for byte.  lancet_trace_format is the same function without a reference."""
    import ctypes
    import numpy as np
    from lancet_amd import build as _build, engine
    _build.build()
    L = engine.lib()
    L.lancet_trace_format2.restype = ctypes.c_void_p
    L.lancet_trace_format2.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int32, ctypes.c_char_p, ctypes.c_char_p,
                                       ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_char_p, ctypes.c_uint32]
    L.lancet_free.argtypes = [ctypes.c_void_p]
    m, batch, kept = mv.case_batch(case)
    p = mv.params(m)
    for cap in (mv.trace_words(batch, p), 1024):
        _, _, texts, events = _level2(monkeypatch, batch, p, cap)
        if cap == 1024:
            assert any("[trace truncated" in t for t in texts)
        for w, words in enumerate(events):
            words = np.ascontiguousarray(words, dtype=np.uint32)
            raw = bytes(batch.ref_bases[int(batch.ref_off[w]):int(batch.ref_off[w + 1])])
            ptr = L.lancet_trace_format2(words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(words), cap, w + 1, batch.hdr[w].encode(),
                                         batch.chrom[w].encode(), int(batch.ref_start[w]), int(batch.ref_start[w]) + len(raw), int(p.dfs_limit), raw, len(raw))
            assert ptr
            got = ctypes.string_at(ptr).decode()
            L.lancet_free(ptr)
            assert got == texts[w], (case, cap, w)


def test_python_cli_still_refuses_the_option():
    """lancet_amd.cli is the Python twin of lancet_gpu's parser for the options both offer; -V is lancet_gpu's alone (tests/test_recovery_emu.py
    pins the same)."""
    base = ["--tumor", "t.bam", "--normal", "n.bam", "--ref", "r.fa", "--reg", "chr22:1-10"]
    ap = cli.build_parser()
    for opt in ("--more-verbose", "-V"):
        with pytest.raises(SystemExit):
            ap.parse_args(base + [opt])
    assert "more-verbose" in (cli.__doc__ or "")


def test_params_block_keeps_its_size():
    import ctypes
    assert ctypes.sizeof(abi.LancetParams) == 72
