"""Shared by test_haplotype_placements_emu.py / test_haplotype_placements_gpu.py: what a run with the reads' placements
(lancet_engine_set_haplotype_placements) has to return.  There is no reference value for the quantity: include/lancet_engine.h defines it, and
model() below restates that definition as plain loops over strings -- it shares nothing with the kernel (no packed words, no masks, no
lanes, no entry buffers).  The hand-made windows carry numbers that are known from how their reads were cut, not from the model.
Placements are abi.placements_to_py's (records, read_begin, tlen); haplotypes abi.haplotypes_to_py's dicts."""
from __future__ import annotations

import functools

import numpy as np

import hap_sup_cases as sc
from hap_sup_cases import _Reads, _ends, _rand, _sub
from lancet_amd import abi, frontend
from lancet_amd.frontend import FWD, NML, REV, TMR

COUNT_MAX = 127                       # LANCET_PLACEMENT_COUNT_MAX
NONE = (-1, 0, 0, 0, 0, 0)            # a read that is not placed: haplotype, offset, mismatches, n_offsets, n_haplotypes, cls


# ---------------------------------------------------------------- the definition, restated

@functools.lru_cache(maxsize=1 << 20)
def place_one(read: str, path: str, k: int):
    """(d, smallest offset with mm = d, how many offsets have it) over the placements of the read on the path -- every offset whose overlap
    is at least k -- or None without one.  (A placement is given up once it has more mismatches than the best so far: neither the minimum
    nor the count of the offsets that reach it changes.)"""
    t, m = len(read), len(path)
    best = first = None
    n = 0
    for o in range(-t, m + 1):
        lo, hi = max(0, -o), min(t, m - o)
        if hi - lo < k:
            continue
        mm, over = 0, False
        for i in range(lo, hi):
            if read[i] != path[o + i]:
                mm += 1
                if best is not None and mm > best:
                    over = True
                    break
        if over:
            continue
        if best is None or mm < best:
            best, first, n = mm, o, 1
        else:
            n += 1
    return None if best is None else (best, first, n)


def place_read(read: str, cls: int, entries, max_mm: int):
    """One record.  entries: [(index_in_window, path string, k)] in index order."""
    got = [(place_one(read, s, k), i) for i, s, k in entries] if read else []
    got = [(x, i) for x, i in got if x is not None]
    if not got:
        return NONE
    d = min(x[0] for x, _ in got)
    if d > max_mm:
        return NONE
    (_, off, n_off), idx = next((x, i) for x, i in got if x[0] == d)
    return (idx, off, d, min(n_off, COUNT_MAX), min(sum(1 for x, _ in got if x[0] == d), COUNT_MAX), cls)


def model(batch, p, haps, max_mm: int):
    """[record] per read of the batch, in its order."""
    out = []
    for w in range(batch.n_windows):
        entries = [(h["index"], h["seq"], h["kmer"]) for h in haps if h["window"] == w]
        assert [e[0] for e in entries] == list(range(len(entries)))
        out += [place_read(read, cls, entries, max_mm) for read, cls in sc.trimmed_reads(batch, p, w)]
    return out


def as_tuples(recs):
    return [tuple(int(x) for x in r) for r in recs]


def check_model(batch, p, haps, pl, max_mm: int):
    recs, rb, tl = pl
    assert len(recs) == batch.n_reads and [int(x) for x in rb] == [int(x) for x in batch.read_begin[:batch.n_windows + 1]]
    want = model(batch, p, haps, max_mm)
    got = as_tuples(recs)
    for i, (g, x) in enumerate(zip(got, want)):
        assert g == x, (i, g, x)
    k = 0
    for w in range(batch.n_windows):
        for read, _ in sc.trimmed_reads(batch, p, w):
            assert int(tl[k]) == len(read), (k, int(tl[k]), len(read))
            k += 1
    return want


def check_support_invariants(batch, haps, pl):
    """With the support switch on at the same limit: per haplotype and class the reads placed on it are no more than `fit`; in a window with
    one group the placed reads with n_haplotypes == 1 are the sum of `alone`."""
    recs, rb, _ = pl
    for w in range(batch.n_windows):
        mine = [h for h in haps if h["window"] == w]
        placed = [[0] * 4 for _ in mine]
        single = 0
        for r in recs[int(rb[w]):int(rb[w + 1])]:
            if int(r["haplotype"]) >= 0:
                placed[int(r["haplotype"])][int(r["cls"])] += 1
                single += int(r["n_haplotypes"]) == 1
        for h, n in zip(mine, placed):
            assert all(a <= f for a, f in zip(n, h["support"]["fit"])), (w, h["index"], n, h["support"])
        if len({(h["kmer"], h["component"]) for h in mine}) == 1:
            assert single == sum(sum(h["support"]["alone"]) for h in mine), (w, single)


# ---------------------------------------------------------------- known from how the reads were cut

def check_basic(variant, batch, st, haps, pl):
    """sc.basic_batch: every read's record from where it was cut (the strings are random: a read of 80 bases lies at one place of its allele).
      - a read cut over the site lies on its own allele at the position it was cut at, without a mismatch, there alone;
      - a read on an end of the window lies on both paths: two haplotypes, the lower index, at the end it was cut from;
      - the read that keeps exactly k bases on the window lies at M - k of the lower index; the two that keep fewer are not placed."""
    _, _, alt, ref, _ = sc.basic_batch(variant)
    recs = as_tuples(pl[0])
    by_seq = {h["seq"]: h["index"] for h in haps}
    assert sorted(by_seq) == sorted([alt, ref]) and all(s["status"] == 0 for s in st)
    first = next(h["seq"] for h in haps if h["index"] == 0)
    reads = [bytes(batch.seq[int(batch.seq_off[r]):int(batch.seq_off[r + 1])]).decode() for r in range(batch.n_reads)]
    tumour = [r for r in range(batch.n_reads) if int(batch.label[r]) == TMR]
    normal = [r for r in range(batch.n_reads) if int(batch.label[r]) == NML]
    (na_f, na_r), (nt_f, nt_r), (nn_f, nn_r) = sc.OVER[(TMR, True)], sc.OVER[(TMR, False)], sc.OVER[(NML, False)]
    n_alt, n_tref, n_nref, n_end = na_f + na_r, nt_f + nt_r, nn_f + nn_r, 2 * sc.PER_END
    groups = [(tumour[:n_alt], alt), (tumour[n_alt:n_alt + n_tref], ref), (normal[:n_nref], ref)]
    for rs, allele in groups:
        for r in rs:
            at = allele.find(reads[r])
            assert at >= 0 and allele.find(reads[r], at + 1) < 0
            assert recs[r][:5] == (by_seq[allele], at, 0, 1, 1), (r, recs[r])
    ends = tumour[n_alt + n_tref:n_alt + n_tref + n_end] + normal[n_nref:n_nref + n_end]
    assert len(ends) == 2 * n_end
    for r in ends:
        at = 0 if reads[r] == ref[:80] else len(first) - 80
        assert reads[r] in (ref[:80], ref[-80:]) and recs[r][:5] == (0, at, 0, 1, 2), (r, recs[r])
    keep_k, keep_less, keep_none = tumour[-3:]
    assert recs[keep_k][:5] == (0, len(first) - sc.K_BASIC, 0, 1, 2) and recs[keep_less] == NONE and recs[keep_none] == NONE
    for r in range(batch.n_reads):                                 # the class is the read's, placed or not ... 0 where it is not
        want = (2 if int(batch.label[r]) == NML else 0) + (1 if int(batch.strand[r]) == REV else 0)
        assert recs[r][5] == (want if recs[r][0] >= 0 else 0)


def check_snv_ends(k, batch, p, names, haps, pl):
    """sc.edge_batch's `snv` window: the read that keeps exactly k bases on the left end of the paths lies at offset k - t, the one that keeps k
    on the right end at M - k; both on the lower index of two (the ends of both paths are the same).  Only where the window stayed at k."""
    w = names.index("snv")
    mine = [h for h in haps if h["window"] == w]
    if any(h["kmer"] != k for h in mine):
        return False
    recs = as_tuples(pl[0])[int(pl[1][w]):int(pl[1][w + 1])]
    reads = [r for r, _ in sc.trimmed_reads(batch, p, w)]
    a = mine[0]["seq"]
    left = [i for i, r in enumerate(reads) if len(r) == 80 and r[80 - k:] == a[:k] and r[:k] != a[:k]]
    right = [i for i, r in enumerate(reads) if len(r) == 80 and r[:k] == a[-k:] and r[-k:] != a[-k:]]
    assert len(left) == 1 and len(right) == 1
    assert recs[left[0]][:5] == (0, k - 80, 0, 1, 2), recs[left[0]]
    assert recs[right[0]][:5] == (0, len(a) - k, 0, 1, 2), recs[right[0]]
    return True


# ---------------------------------------------------------------- offset ties against lane order

TIE_K, TIE_T, TIE_A, TIE_B = 15, 40, 35, 105
TIE_DIFF = [2 + 5 * i for i in range(8)]             # positions of a segment at which its twin differs: three in every 15-mer


@functools.lru_cache(maxsize=None)
def tie_batch():
    """(batch, params, reference, read): one reference-only window of 200 bases whose bases TIE_A .. TIE_A + 40 and TIE_B .. TIE_B + 40 are twins
    that differ at TIE_DIFF -- at least three positions of every 15-mer, so neither the graph nor the reference's repeat tests see a repeat --
    and a read of 40 bases that takes every other one of those positions from either twin: four mismatches at offset 35, four at offset 105,
    far more anywhere else.  With k = 15 the offsets run from -25: offset 35 is the 61st (first trip of 64, lane 60), offset 105 the 131st
    (third trip, lane 2) -- the larger offset on the lower lane."""
    rng = np.random.default_rng(77)
    ref = list(_rand(rng, 200))
    seg = ref[TIE_A:TIE_A + TIE_T]
    twin = list(_sub("".join(seg), TIE_DIFF))
    ref[TIE_B:TIE_B + TIE_T] = twin
    ref = "".join(ref)
    read = "".join(twin[i] if i in TIE_DIFF[::2] else seg[i] for i in range(TIE_T))
    rd = _Reads()
    for sample in (TMR, NML):
        _ends(rd, ref, 80, sample, 4)
        for i, s in enumerate(range(0, 200 - 80 + 1, 4)):
            rd.add(ref[s:s + 80], sample, FWD if i & 1 else REV)
    rd.add(read, TMR, FWD)
    win = frontend.Window("chr22:5000-5200", "chr22", 5000, 5200, ref)
    return frontend.build_batch([win], [rd.ordered()]), abi.default_params(min_k=TIE_K, max_k=TIE_K), ref, read


def check_tie(batch, st, haps, pl):
    """First that the window reports the path it was made for -- the reference, whole, at k = 15 -- then the read's record."""
    _, _, ref, read = tie_batch()
    assert st[0]["status"] == 0 and [h["seq"] for h in haps if h["index"] == 0] == [ref] and haps[0]["kmer"] == TIE_K
    reads = [bytes(batch.seq[int(batch.seq_off[r]):int(batch.seq_off[r + 1])]).decode() for r in range(batch.n_reads)]
    (r,) = [i for i, s in enumerate(reads) if s == read]
    rec = as_tuples(pl[0])[r]
    assert rec[:4] == (0, TIE_A, 4, 2), rec


# ---------------------------------------------------------------- hand-written windows (the emulator's call)

def model_hand(entries, reads, max_mm: int):
    ent = [(i, e[0], e[1]) for i, e in enumerate(entries)]
    return [place_read(s, cls, ent, max_mm) for s, cls in reads]
