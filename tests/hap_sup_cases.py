"""Shared by test_haplotype_support_emu.py / test_haplotype_support_gpu.py: what a run with the haplotypes' read support
(lancet_engine_set_haplotype_support) has to return.  There is no reference value for the quantity: include/lancet_engine.h defines it, and
model() below restates that definition as plain loops over strings -- it shares nothing with the kernel (no packed words, no masks, no
lanes).  The hand-made windows carry numbers that are known from how their reads were cut, not from the model.
A haplotype is one of abi.haplotypes_to_py's dicts with "support" = {"fit": [Tf, Tr, Nf, Nr], "alone": [Tf, Tr, Nf, Nr]}."""
from __future__ import annotations

import functools

import numpy as np

import hap_cases as hc
from lancet_amd import abi, frontend
from lancet_amd.frontend import FWD, NML, REV, TMR

CLASSES = ("Tf", "Tr", "Nf", "Nr")


# ---------------------------------------------------------------- the definition, restated

def trimmed_reads(batch, p, w: int):
    """[(string, class)] of window w's reads as the kernels see them: Graph_t::trim (reference src/Graph.cc:355-384) cuts in front of the
    first and behind the last base that is one of ACGT with a quality of at least min_qual_trim; a read with anything else than ACGT in
    between, or nothing left, has no bases.  class: 0..3 = Tf Tr Nf Nr."""
    out = []
    for r in range(int(batch.read_begin[w]), int(batch.read_begin[w + 1])):
        s = bytes(batch.seq[int(batch.seq_off[r]):int(batch.seq_off[r + 1])]).decode().upper()
        q = batch.qual[int(batch.seq_off[r]):int(batch.seq_off[r + 1])]
        good = [i for i in range(len(s)) if s[i] in "ACGT" and int(q[i]) >= int(p.min_qual_trim)]
        t = s[good[0]:good[-1] + 1] if good else ""
        if any(c not in "ACGT" for c in t):
            t = ""
        out.append((t, (2 if int(batch.label[r]) == NML else 0) + (1 if int(batch.strand[r]) == REV else 0)))
    return out


@functools.lru_cache(maxsize=1 << 20)
def distance(read: str, path: str, k: int):
    """d(r, h): the fewest mismatches over all placements whose overlap is at least k; None without a placement.  (A placement is given
    up once it cannot beat the best one so far: the minimum is the same.)"""
    t, m = len(read), len(path)
    best = None
    for o in range(-t, m + 1):
        lo, hi = max(0, -o), min(t, m - o)
        if hi - lo < k:
            continue
        mm = 0
        for i in range(lo, hi):
            if read[i] != path[o + i]:
                mm += 1
                if best is not None and mm >= best:
                    break
        if best is None or mm < best:
            best = mm
    return best


def model(batch, p, haps, max_mm: int):
    """[{"fit": [4], "alone": [4]}] per haplotype, in order."""
    out = [{"fit": [0] * 4, "alone": [0] * 4} for _ in haps]
    byw = {}
    for i, h in enumerate(haps):
        byw.setdefault(h["window"], {}).setdefault((h["kmer"], h["component"]), []).append(i)
    for w, groups in byw.items():
        for read, cls in trimmed_reads(batch, p, w):
            for (k, _), members in groups.items():
                if len(read) < k:
                    continue
                ds = [distance(read, haps[i]["seq"], k) for i in members]
                have = [d for d in ds if d is not None]
                if not have or min(have) > max_mm:
                    continue
                fits = [i for i, d in zip(members, ds) if d == min(have)]
                for i in fits:
                    out[i]["fit"][cls] += 1
                    if len(fits) == 1:
                        out[i]["alone"][cls] += 1
    return out


def check_model(batch, p, haps, max_mm: int):
    want = model(batch, p, haps, max_mm)
    for h, x in zip(haps, want):
        assert h["support"] == x, (h["window"], h["index"], h["kmer"], h["component"], h["support"], x)
    check_invariants(batch, haps)
    return want


def check_invariants(batch, haps):
    """alone <= fit per class; the reads that are alone on the entries of one group are different reads: no more than the window has of the class."""
    assert all(h["flags"] & abi.HAP_HAS_SUPPORT for h in haps)
    n_cls = {}
    for h in haps:
        s = h["support"]
        assert all(0 <= a <= f for a, f in zip(s["alone"], s["fit"])), (h["window"], h["index"], s)
        w = h["window"]
        if w not in n_cls:
            n = [0] * 4
            for r in range(int(batch.read_begin[w]), int(batch.read_begin[w + 1])):
                n[(2 if int(batch.label[r]) == NML else 0) + (1 if int(batch.strand[r]) == REV else 0)] += 1
            n_cls[w] = n
        assert all(f <= n for f, n in zip(s["fit"], n_cls[w]))
    groups = {}
    for h in haps:
        g = groups.setdefault((h["window"], h["kmer"], h["component"]), [0] * 4)
        for c in range(4):
            g[c] += h["support"]["alone"][c]
    for (w, _, _), g in groups.items():
        assert all(a <= n for a, n in zip(g, n_cls[w])), (w, g, n_cls[w])


def words_of(h) -> int:
    """Words of its window's buffer a haplotype takes with everything it carries."""
    return hc.words_of(h) + len(h.get("cigar", ())) + (2 * (h["len"] + h["ref_len"]) if "cov" in h else 0) + (8 if "support" in h else 0)


def ample_words(batch, p) -> int:
    """lancet_gpu's size for the batch with --haplotype-support alone: hap_words_for plus 8 words for each of the 32 paths."""
    return hc.ample_words(batch, p) + 32 * 8


def strip_support(haps) -> list:
    """The dicts as a run without the switch returns them -- the flag bit included."""
    return [{k: (x & ~abi.HAP_HAS_SUPPORT if k == "flags" else x) for k, x in h.items() if k != "support"} for h in haps]


# ---------------------------------------------------------------- hand-made windows

_OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}


def _rand(rng, n: int) -> str:
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


class _Reads:
    """The reads of one window while it is being put together."""

    def __init__(self):
        self.recs, self.n = [], 0

    def add(self, seq: str, sample, strand, qual=None):
        self.recs.append((f"{'T' if sample == TMR else 'N'}{self.n:04d}", seq, qual or "I" * len(seq), sample, strand, 1, True))
        self.n += 1

    def ordered(self):
        return [r for r in self.recs if r[3] == TMR] + [r for r in self.recs if r[3] == NML]      # (tumour first: the reference's readid order)


def _tile(rd: _Reads, hap: str, read_len: int, sample, n_fwd: int, n_rev: int, site: int):
    """n_fwd + n_rev reads of read_len bases cut from hap, every one of them over base `site` with at least 20 bases on either side of it."""
    n = n_fwd + n_rev
    lo, hi = max(0, site - read_len + 21), min(len(hap) - read_len, site - 20)
    assert lo <= hi
    for i in range(n):
        s = lo + (hi - lo) * i // max(1, n - 1)
        rd.add(hap[s:s + read_len], sample, FWD if i < n_fwd else REV)


def _ends(rd: _Reads, hap: str, read_len: int, sample, per_end: int):
    """per_end reads on each end of hap, half of them on either strand: the first and the last k-mer become anchors."""
    for i in range(per_end):
        rd.add(hap[:read_len], sample, FWD if i & 1 else REV)
        rd.add(hap[-read_len:], sample, FWD if i & 1 else REV)


# The basic window and its twin with a deletion.  L bases of reference; the variant in the middle; reads of 80 bases.
L_BASIC, K_BASIC, SITE = 240, 15, 120
# reads over the site: (sample, carries the variant) -> (forward, reverse)
OVER = {(TMR, True): (5, 4), (TMR, False): (2, 3), (NML, False): (4, 6)}
PER_END = 4                      # reads per end, sample and allele, none of them over the site: they fit both paths


@functools.lru_cache(maxsize=None)
def basic_batch(variant: str):
    """(batch, params, alt string, ref string, expected): one window with a planted SNV ("snv") or 3-base deletion ("del3").
    expected = {"alt": (fit, alone), "ref": (fit, alone)}, worked out from how the reads were cut:
      - a read over the site has at least 20 of its own bases on either side of it.  Cut from one allele it lies on that path without a
        mismatch and on the other with at least one (a substitution) or with more than max_mm = 5 (the ungapped placements of a read with
        the deletion mismatch on one side of it, 20 random bases or more): it fits its own path alone;
      - a read on an end of the window, 80 bases, does not reach the site: it lies on both paths without a mismatch, fits both, alone on none;
      - three more tumour forward reads hang over the right end of the window: one keeps exactly k bases on it (a placement, no
        mismatch: it fits both), one k - 1 (no placement at its own position) and one none at all; the last two are random elsewhere and fit nothing."""
    rng = np.random.default_rng(5 if variant == "snv" else 6)
    genome = _rand(rng, L_BASIC + 100)
    ref = genome[:L_BASIC]
    alt = ref[:SITE] + _OTHER[ref[SITE]] + ref[SITE + 1:] if variant == "snv" else ref[:SITE] + ref[SITE + 3:]
    rd = _Reads()
    for (sample, on_alt), (nf, nr) in OVER.items():
        _tile(rd, alt if on_alt else ref, 80, sample, nf, nr, SITE)
    for sample in (TMR, NML):
        _ends(rd, ref, 80, sample, PER_END)                      # (the ends of both alleles are the same 80 bases)
    for keep in (K_BASIC, K_BASIC - 1, 0):
        rd.add(genome[L_BASIC - keep:L_BASIC - keep + 80], TMR, FWD)
    win = frontend.Window(f"chr22:1001-{1001 + L_BASIC}", "chr22", 1001, 1001 + L_BASIC, ref)
    ends = [PER_END, PER_END, PER_END, PER_END]                  # 2 ends * PER_END / 2 per strand, both samples
    both = [ends[0] + 1, ends[1], ends[2], ends[3]]              # ... and the read that keeps k bases on the window
    fa, fr = OVER[(TMR, True)]
    alt_alone = [fa, fr, 0, 0]
    tf, tr = OVER[(TMR, False)]
    nf, nr = OVER[(NML, False)]
    ref_alone = [tf, tr, nf, nr]
    expected = {"alt": ([a + b for a, b in zip(alt_alone, both)], alt_alone), "ref": ([a + b for a, b in zip(ref_alone, both)], ref_alone)}
    return frontend.build_batch([win], [rd.ordered()]), abi.default_params(min_k=K_BASIC, max_k=K_BASIC), alt, ref, expected


def check_basic(variant, batch, st, haps, trunc):
    """First that the window assembled into exactly the two paths, in one group -- else the counts prove nothing -- then the counts."""
    _, _, alt, ref, expected = basic_batch(variant)
    assert all(s["status"] == 0 for s in st) and not any(trunc)
    assert sorted(h["seq"] for h in haps) == sorted([alt, ref]) and len({(h["kmer"], h["component"]) for h in haps}) == 1
    assert all(h["kmer"] == K_BASIC and (h["ref_off"], h["ref_len"]) == (0, L_BASIC) for h in haps)
    for h in haps:
        fit, alone = expected["alt" if h["seq"] == alt else "ref"]
        assert h["support"] == {"fit": fit, "alone": alone}, (variant, h["seq"] == alt, h["support"], fit, alone)


# ---- the edges of the kernel: one batch per k, every window against the model
READ_LENS = [15, 16, 17, 31, 32, 33, 63, 64, 65]
TRIPS = [63, 64, 65, 128, 129]                                   # t + M - 2k + 1 for the reads of trip_t(k) bases


def trip_t(k: int) -> int:
    return k + 25


def _sub(s: str, at) -> str:
    x = list(s)
    for i in at:
        x[i] = _OTHER[x[i]]
    return "".join(x)


@functools.lru_cache(maxsize=None)
def edge_batch(k: int):
    """(batch, params, names).  Windows, by name:
      snv         a SNV window of 200 bases, reads of 80; beside them reads of READ_LENS bases, of k and of k - 1 bases cut over the
                  site from either allele, reads cut down to 17 / 33 bases by their qualities, reads with exactly 5 and exactly 6
                  substitutions, a read that keeps exactly k bases on the left end of the paths and one that keeps k on the right end
                  (the leftmost / rightmost placement, the only one without a mismatch), and one with an N (no bases at all)
      trip<N>     one path of N + 2k - 1 - trip_t(k) bases, reads of trip_t(k) bases: N offsets, the lane trips' edges
      short       a path of 60 bases under reads of 90: every read is longer than the path
      two_comp    reads on the left and on the right third only, a SNV in each: two components, two groups
      junk        reads that have nothing to do with the reference: no entry
      empty       no reads
    """
    rng = np.random.default_rng(100 + k)
    wins, reads, names = [], [], []

    def window(name, ref, rd):
        start = 1000 + 1000 * len(wins)
        wins.append(frontend.Window(f"chr22:{start}-{start + len(ref)}", "chr22", start, start + len(ref), ref))
        reads.append(rd.ordered())
        names.append(name)

    # snv
    W, site, rl = 200, 100, 80
    ref = _rand(rng, W)
    alt = _sub(ref, [site])
    rd = _Reads()
    _tile(rd, alt, rl, TMR, 4, 4, site)
    _tile(rd, ref, rl, TMR, 2, 1, site)
    _tile(rd, ref, rl, NML, 4, 4, site)
    for sample in (TMR, NML):
        _ends(rd, ref, rl, sample, 4)
    for j, t in enumerate(READ_LENS + [k, k - 1]):
        for hap, sample in ((alt, TMR), (ref, NML)):
            s = site - t // 2 + (j % 3) - 1
            rd.add(hap[s:s + t], sample, FWD if j & 1 else REV)
    for t, cut in ((17, 3), (33, 5)):                               # raw t + 2 * cut bases, `cut` on either side below the trimming quality
        s = site - t // 2 - cut
        rd.add(alt[s:s + t + 2 * cut], TMR, FWD, "#" * cut + "I" * t + "#" * cut)
    for n in (5, 6):
        rd.add(_sub(ref[20:20 + rl], [7 + 11 * i for i in range(n)]), TMR, REV)
    rd.add(_rand(rng, rl - k) + ref[:k], TMR, FWD)
    rd.add(ref[W - k:] + _rand(rng, rl - k), NML, REV)
    rd.add(ref[30:60] + "N" + ref[61:110], TMR, FWD)
    window("snv", ref, rd)
    # trips
    T = trip_t(k)
    for n in TRIPS:
        m = n + 2 * k - 1 - T
        ref = _rand(rng, m)
        rd = _Reads()
        for sample in (TMR, NML):
            _ends(rd, ref, T, sample, 4)
            for i, s in enumerate(range(0, m - T + 1, 4)):
                rd.add(ref[s:s + T], sample, FWD if i & 1 else REV)
        rd.add(_sub(ref[:T], [T - 1]), TMR, FWD)                    # (a mismatch in the last base: the far end of the mask)
        rd.add(_sub(ref[-T:], [0]), TMR, REV)
        window(f"trip{n}", ref, rd)
    # short
    g = _rand(rng, 120)
    ref = g[30:90]
    rd = _Reads()
    for sample in (TMR, NML):
        for i in range(8):
            rd.add(g[4 * i:4 * i + 90], sample, FWD if i & 1 else REV)
    window("short", ref, rd)
    # two_comp
    ref = _rand(rng, 300)
    a1, a2 = _sub(ref, [50]), _sub(ref, [250])
    rd = _Reads()
    for lo, hap in ((0, a1), (200, a2)):
        for i in range(10):
            s = lo + 20 * i // 9
            rd.add(hap[s:s + 80], TMR, FWD if i & 1 else REV)
            rd.add(ref[s:s + 80], NML, FWD if i & 1 else REV)
    window("two_comp", ref, rd)
    # junk, empty
    ref = _rand(rng, 120)
    rd = _Reads()
    for i in range(6):
        rd.add(_rand(rng, 80), TMR if i & 1 else NML, FWD)
    window("junk", ref, rd)
    window("empty", _rand(rng, 120), _Reads())
    # (k = 11: a window of 200 random bases usually repeats an 11-mer within two mismatches, so those windows may climb; the others stay at k)
    return frontend.build_batch(wins, reads), abi.default_params(min_k=k, max_k=k if k != 11 else 31), names


@functools.lru_cache(maxsize=None)
def dups_batch():
    """(batch, params): one window of 300 bases with reads on its left and its right third only -- two components.  The tumour carries a SNV
    on the left and a tandem duplication of 18 bases on the right: the right component has a cycle up to k = 19, so the window climbs, and
    the left component, which comes first at k = 19, is reported at 19 and again at 21 with the same two path strings."""
    rng = np.random.default_rng(302)
    u = 18
    ref = _rand(rng, 300)
    a1 = _sub(ref, [50])
    a2 = ref[:250] + ref[250 - u:250] + ref[250:]
    rd = _Reads()
    for i in range(10):
        s = 20 * i // 9
        rd.add(a1[s:s + 80], TMR, FWD if i & 1 else REV)
        rd.add(ref[s:s + 80], NML, FWD if i & 1 else REV)
        s = 200 + 20 * i // 9
        rd.add(a2[s:s + 80 + u], TMR, FWD if i & 1 else REV)
        rd.add(ref[s:s + 80], NML, FWD if i & 1 else REV)
    win = frontend.Window("chr22:1000-1300", "chr22", 1000, 1300, ref)
    return frontend.build_batch([win], [rd.ordered()]), abi.default_params(min_k=15, max_k=31)


def check_dups(batch, p, haps):
    """The same two strings at two k; each entry counted among the entries of its own k: 5 + 5 tumour reads alone on the changed string, 5 + 5
    normal reads alone on the reference's, at either k (the reads of the other third have no placement within 5 mismatches)."""
    ks = {}
    for h in haps:
        ks.setdefault(h["seq"], []).append(h["kmer"])
    twice = [s for s, x in ks.items() if len(set(x)) >= 2]
    assert len(twice) == 2
    for h in haps:
        if h["seq"] in twice:
            tumour = h["n_variants"] > 0
            assert h["support"] == {"fit": [5, 5, 0, 0] if tumour else [0, 0, 5, 5], "alone": [5, 5, 0, 0] if tumour else [0, 0, 5, 5]}, h["support"]
    check_model(batch, p, haps, 5)


def check_edges(k, batch, names, st, haps, trunc, max_mm: int):
    """The windows are what they were made to be, and every count is the model's."""
    byname = {n: [h for h in haps if h["window"] == w] for w, n in enumerate(names)}
    assert not any(trunc) and all(h["kmer"] == k for n in names if n.startswith("trip") or n == "short" for h in byname[n])
    assert len(byname["snv"]) == 2 and len({h["component"] for h in byname["snv"]}) == 1
    for n in TRIPS:
        (h,) = byname[f"trip{n}"]
        assert trip_t(k) + h["len"] - 2 * k + 1 == n and h["flags"] & abi.HAP_IS_REF
    (h,) = byname["short"]
    assert h["len"] < 90
    assert len({h["component"] for h in byname["two_comp"]}) == 2 and len(byname["two_comp"]) >= 3
    assert byname["junk"] == [] and byname["empty"] == []
    want = check_model(batch, batch_params(k), haps, max_mm)
    for n in TRIPS + ["short"]:                                     # one entry: nobody to share with
        (h,) = byname[n if isinstance(n, str) else f"trip{n}"]
        assert h["support"]["alone"] == h["support"]["fit"] and sum(h["support"]["fit"]) >= 16
    return byname, want


def batch_params(k: int):
    return edge_batch(k)[1]


def check_snv_reads(names, haps_by_mm):
    """What two special reads of the `snv` window do, from how they were cut.  haps_by_mm: {max_mm: haplotypes} for 0, 4, 5, 6, 255.
    The read with exactly 5 substitutions (tumour, reverse, cut from the reference where the paths do not differ) fits both paths from
    max_mm = 5 on, the one with exactly 6 from 6 on: one more Tr in both entries' `fit` each time, nothing in `alone`.  Below 5 nothing in
    the window has between 1 and 4 mismatches on its best path, so 0 and 4 count the same reads."""
    w = names.index("snv")

    def col(mm, what, c):
        return [h["support"][what][c] for h in haps_by_mm[mm] if h["window"] == w]
    assert [a + 1 for a in col(4, "fit", 1)] == col(5, "fit", 1) and [a + 1 for a in col(5, "fit", 1)] == col(6, "fit", 1)
    assert col(4, "alone", 1) == col(5, "alone", 1) == col(6, "alone", 1)
    for c in (0, 2, 3):
        assert col(4, "fit", c) == col(5, "fit", c) == col(6, "fit", c)
    assert all(a >= b for a, b in zip(col(255, "fit", 1), col(6, "fit", 1)))
