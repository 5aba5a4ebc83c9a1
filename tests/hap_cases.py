"""Shared by test_haplotypes_emu.py / test_haplotypes_gpu.py: what a run with the haplotype capture (lancet_engine_set_haplotypes) has to
return, held against what the REFERENCE ITSELF printed under -V (the `r:` / `p:` lines of tests/golden/more_verbose/*.V.trace.txt.gz) and
against the run's own records.  A run is (records, stats, haplotypes, truncated): records and stats as every parity test has them,
haplotypes as abi.haplotypes_to_py makes them."""
from __future__ import annotations

import functools

import numpy as np

import more_verbose_util as mv
from lancet_amd import abi, frontend
from lancet_amd.frontend import FWD, NML, REV, TMR

KEY = lambda s: (s["status"], s["final_k"], s["n_builds"], s["n_variants"], s["n_kmers"], s["max_nodes"])
HDR = abi.HAP_HEADER_WORDS


def words_of(h) -> int:
    """Words of its window's buffer a haplotype takes."""
    return HDR + (h["len"] + 15) // 16


def ample_words(batch, p) -> int:
    """lancet_gpu's size for the batch (lancet_main.cc hap_words_for): 32 paths of (longest window reference + --max-indel-len + 256) bases."""
    longest = max(int(batch.ref_off[w + 1] - batch.ref_off[w]) for w in range(batch.n_windows))
    return 32 * (HDR + (longest + int(p.max_indel_len) + 256 + 15) // 16)


def stretch(batch, h) -> str:
    """The piece of the window reference the haplotype was compared with (Ref_t::seq)."""
    w = h["window"]
    raw = bytes(batch.ref_bases[int(batch.ref_off[w]):int(batch.ref_off[w + 1])]).decode()
    assert h["ref_off"] + h["ref_len"] <= len(raw)
    return raw[h["ref_off"]:h["ref_off"] + h["ref_len"]]


@functools.lru_cache(maxsize=None)
def golden_lines(case: str):
    """(r: lines, p: lines) of the case's golden, in the reference's order."""
    lines = mv.golden_trace(case).splitlines()
    r, p = [l[4:] for l in lines if l.startswith("r:  ")], [l[4:] for l in lines if l.startswith("p:  ")]
    assert len(r) == len(p) >= 26
    return r, p


def check_shape(batch, st, haps, trunc):
    """What holds for every result: the order, the indices, the packing, nothing for a window without a result."""
    assert [(h["window"], h["index"]) for h in haps] == sorted((h["window"], h["index"]) for h in haps)
    per = {}
    for h in haps:
        assert h["index"] == per.get(h["window"], 0)
        per[h["window"]] = h["index"] + 1
        assert st[h["window"]]["status"] >= 0
        assert h["len"] >= 1 and len(h["seq"]) == h["len"] and h["n_words"] == (h["len"] + 15) // 16 and h["pad_bits"] == 0
        assert h["flags"] & ~(abi.HAP_UNALIGNED | abi.HAP_IS_REF) == 0
        assert h["kmer"] >= 3 and h["component"] >= 1
    assert len(trunc) == batch.n_windows and all(t in (0, 1) for t in trunc)
    assert all(trunc[w] == 0 for w in range(batch.n_windows) if st[w]["status"] < 0)


def check_goldens(case, batch, st, haps, trunc):
    """The strings are the reference's p: lines, (ref_off, ref_len) cut its r: lines out of the window reference -- all of them, in order."""
    check_shape(batch, st, haps, trunc)
    r, p = golden_lines(case)
    assert not any(trunc)
    assert [h["seq"] for h in haps] == p
    assert [stretch(batch, h) for h in haps] == r
    for h in haps:                                                  # the flags say what the strings say
        same = h["seq"] == stretch(batch, h)
        assert bool(h["flags"] & abi.HAP_IS_REF) == same
        if h["flags"] & abi.HAP_UNALIGNED:
            assert h["len"] == h["ref_len"]
        if same:
            assert h["flags"] & abi.HAP_UNALIGNED and h["n_variants"] == 0


def replay(batch, h, recs):
    """more_verbose_util.replay_paths' rule on records: a record sits at offset pos + 1 - (window start + ref_off) of the stretch (its pos is
    0-based, the transcript's 1-based) and puts its alt without the '-' in place of its ref without the '-'."""
    r = stretch(batch, h)
    made, at = [], 0
    for x in recs:
        o = x["pos"] + 1 - int(batch.ref_start[h["window"]]) - h["ref_off"]
        ref, qry = x["ref"].replace("-", ""), x["alt"].replace("-", "")
        assert o >= at and r[o:o + len(ref)] == ref, (h["window"], h["index"], x)
        made += [r[at:o], qry]
        at = o + len(ref)
    return "".join(made) + r[at:]


def check_link(batch, v, st, haps, windows=None):
    """Per window the [first_variant, first_variant + n_variants) ranges tile [0, stats.n_variants) in order, and a haplotype is its reference
    stretch with exactly its own records applied.  `windows`: only these (a truncated window's ranges stop short)."""
    byw = {}
    for x in v:
        byw.setdefault(x["window"], []).append(x)
    for w in (range(batch.n_windows) if windows is None else windows):
        recs = byw.get(w, [])
        assert [x["seq"] for x in recs] == list(range(len(recs)))
        at = 0
        for h in (h for h in haps if h["window"] == w):
            assert h["first_variant"] == at and h["n_variants"] >= 0, (w, h["index"])
            mine = recs[at:at + h["n_variants"]]
            assert len(mine) == h["n_variants"] and all(x["kmer"] == h["kmer"] for x in mine)
            assert replay(batch, h, mine) == h["seq"], (w, h["index"])
            at += h["n_variants"]
        if st[w]["status"] >= 0:
            assert at == st[w]["n_variants"] == len(recs), (w, at, st[w])


# ---------------------------------------------------------------- hand-made windows at the edges of a word

EDGE_LENS = [63, 64, 65, 79, 80, 81]


@functools.lru_cache(maxsize=None)
def edge_batch():
    """One window per length of EDGE_LENS whose reads all spell its reference: one path, the reference itself, no records.  (The windows of
    tests/domain_cases.py's tiny family, without a variant.)"""
    rng = np.random.default_rng(16)
    wins, reads = [], []
    for w, L in enumerate(EDGE_LENS):
        ref = "".join("ACGT"[i] for i in rng.integers(0, 4, size=L))
        rs = [(f"{'T' if i < 8 else 'N'}{i // 2:04d}", ref, "I" * L, TMR if i < 8 else NML, FWD if i & 1 else REV, 1 + (i & 1), True) for i in range(12)]
        start = 1000 + 200 * w
        wins.append(frontend.Window(f"chr22:{start}-{start + L}", "chr22", start, start + L, ref))
        reads.append(rs)
    return frontend.build_batch(wins, reads), abi.default_params(min_k=9, max_k=31)


def check_edges(batch, v, st, haps, trunc):
    check_shape(batch, st, haps, trunc)
    assert v == [] and all(s["status"] == 0 and s["n_variants"] == 0 for s in st) and not any(trunc)
    assert [h["window"] for h in haps] == list(range(len(EDGE_LENS)))                    # one path each
    for h, L in zip(haps, EDGE_LENS):
        assert (h["ref_off"], h["ref_len"], h["len"]) == (0, L, L)                       # the whole window: lengths on both sides of a word
        assert h["seq"] == stretch(batch, h)
        assert h["flags"] == abi.HAP_UNALIGNED | abi.HAP_IS_REF and (h["first_variant"], h["n_variants"]) == (0, 0)
        assert h["n_words"] == (L + 15) // 16 and h["pad_bits"] == 0                      # (buffers start as 0xCD on the host, as whatever was there on the device)


# ---------------------------------------------------------------- a window that does not fit

def truncation_plan(haps):
    """(window, words_per_window): a window of the ample run with at least three paths and a size that holds its first two and not its third."""
    for w in sorted({h["window"] for h in haps}):
        mine = [h for h in haps if h["window"] == w]
        if len(mine) >= 3:
            two = words_of(mine[0]) + words_of(mine[1])
            return w, two + words_of(mine[2]) - 1
    raise AssertionError("no window with three paths")


def check_truncated(batch, w, cap, full, cut):
    """full / cut: (records, stats, haplotypes, truncated) of the ample run and of the run with `cap` words per window."""
    (fv, fst, fh, ft), (cv, cst, ch, ct) = full, cut
    assert cv == fv and [KEY(s) for s in cst] == [KEY(s) for s in fst]                    # nothing else changes
    check_shape(batch, cst, ch, ct)
    assert ct[w] == 1 and [h for h in ch if h["window"] == w] == [h for h in fh if h["window"] == w][:2]       # the two that fit, whole
    for o in range(batch.n_windows):
        mine, want = [h for h in ch if h["window"] == o], [h for h in fh if h["window"] == o]
        fits, n = 0, 0
        for h in want:                                                                    # the ones in front of the first that does not fit
            if fits + words_of(h) > cap:
                break
            fits += words_of(h)
            n += 1
        assert mine == want[:n] and ct[o] == (1 if n < len(want) else 0), o
    neighbours = [o for o in (w - 1, w + 1) if 0 <= o < batch.n_windows]
    assert any(ct[o] == 0 and [h for h in fh if h["window"] == o] for o in neighbours)     # a whole neighbour with haplotypes of its own
    check_link(batch, cv, cst, ch, windows=[o for o in range(batch.n_windows) if not ct[o]])
