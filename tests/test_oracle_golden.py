"""Pins the oracle (oracle/lancet_oracle.cc + oracle/vcf_oracle.py) against outputs of the reference itself.

tests/golden/<case>.vcf and <case>.trace.txt were written by the unmodified reference binary
(tools/make_golden.py).  The oracle has to reproduce, byte for byte,
  * the VCF header + body (whole-program parity, --num-threads 1, --active-region-off), and
  * the digest of the reference's `-v` trace: every k attempt and its rejection reason, node/edge/span counts
    after each graph stage, source/sink anchors, every path and every transcript with its coverages.
CPU only."""
import os

import numpy as np
import pytest

import align_cases as ac
import golden_util as gu
from lancet_amd import abi
from oracle import oracle, vcf_oracle


@pytest.mark.parametrize("case", gu.CASES)
def test_oracle_reproduces_reference_vcf_and_trace(case):
    meta, batch, kept, (min_k, max_k) = gu.case_batch(case)
    lr = gu.case_lr(meta)                     # --linked-reads case
    variants, stats, trace = oracle.run(batch, gu.params(meta), verbose=True)
    db = vcf_oracle.VariantDB(lr=lr)
    for rec in variants:                      # replay addVar in window-processing order
        db.add(vcf_oracle.Variant(batch.chrom[rec["window"]], rec, lr=lr, bx_names=batch.bx_names))
    assert db.vcf() == gu.golden_vcf(case)
    assert gu.digest_trace(trace) == gu.golden_trace(case)
    assert sum(s["n_variants"] for s in stats) == len(variants)


def test_golden_cases_cover_the_k_loop_branches():
    """The fixtures must exercise: ref-repeat rejections, cycle-driven k bumps, k up to the 40s, multi-path
    windows, complex/ins/del/snv transcripts."""
    all_trace = "".join(gu.golden_trace(c) for c in gu.CASES)
    assert all_trace.count("Cycle found in the graph") > 100
    assert all_trace.count("Repeat in reference sequence") > 100
    assert all_trace.count("Near-perfect repeat in reference") > 100
    body = "".join(l for c in gu.CASES for l in gu.golden_vcf(c).splitlines(True) if not l.startswith("#"))
    for t in ("TYPE=snv", "TYPE=ins", "TYPE=del", "TYPE=complex", "SOMATIC", "SHARED", ";MS="):
        assert t in body or t == ";MS=", t
    ks = {int(l.split("KMERSIZE=")[1].split(";")[0]) for l in body.splitlines()}
    assert max(ks) >= 45 and min(ks) <= 13


def _rand_seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


ALIGN_GOLDEN = os.path.join(gu.GOLDEN, "align_ref.tsv")


def align_cases():
    """The (S, T) pairs the alignment restatement is checked on: random sequences with a few edits, then degenerate shapes."""
    rng = np.random.default_rng(5)
    pairs = []
    for it in range(60):
        n = int(rng.integers(30, 260))     # tiny S hits undefined behaviour in the reference traceback
        s = _rand_seq(rng, n)
        t = list(s)
        for _ in range(int(rng.integers(0, 6))):          # a few edits: sub / ins / del (some long)
            p = int(rng.integers(0, max(1, len(t))))
            r = rng.random()
            if r < 0.34 and t:
                t[p] = "ACGT"[int(rng.integers(0, 4))]
            elif r < 0.67:
                t[p:p] = list(_rand_seq(rng, int(rng.integers(1, 40))))
            elif t:
                del t[p:p + int(rng.integers(1, 40))]
        pairs.append((s, "".join(t) or "A"))
    return pairs + [("A", "A"), ("A", "C"), ("ACGT", "A"), ("A", "ACGT"), ("AAAAAAAA", "AAAA"), ("ACACACAC", "ACAC")]


def load_align_golden():
    """tests/golden/align_ref.tsv: S, T and the two aligned rows the reference's own global_align_aff returned for them
    (tools/make_align_golden.py)."""
    out = {}
    with open(ALIGN_GOLDEN) as fh:
        for line in fh:
            s, t, a, b = line.rstrip("\n").split("\t")
            out[(s, t)] = (a, b)
    return out


def test_alignment_restatement_equals_reference_align_cc():
    """oracle global_align_aff vs the reference's own align.cc (real reference code): its answers recorded in
    tests/golden/align_ref.tsv, and the library itself where oracle/_ref holds a build of it."""
    golden = load_align_golden()
    live = oracle.ref_align_available()
    for s, t in align_cases():
        assert (s, t) in golden, (s, t)
        assert oracle.align(s, t) == golden[(s, t)], (s, t)
        if live:
            assert oracle.ref_align(s, t) == golden[(s, t)], (s, t)


@pytest.mark.parametrize("fam", ac.FAMILIES)
def test_alignment_restatement_equals_reference_on_tie_rich_and_boundary_pairs(fam):
    """The oracle's global_align_aff on the table of tests/align_cases.py (length seams, STR expansions, long gaps, paths along the edge of
    the band, tiny and unrelated strings) against what the reference's own align.cc answered (tests/golden/align_edge_ref.tsv), and against
    the library itself where oracle/_ref holds a build of it.  Where the reference's traceback leaves its matrix (undefined behaviour
    there, `undefined` in the fixture) the oracle returns None -- it used to crash the process -- and the library is not called."""
    golden = ac.golden()
    live = oracle.ref_align_available()
    n = 0
    for cid, s, t in ac.by_family(fam):
        want = golden[cid]
        got = oracle.align(s, t)
        if want == ac.UNDEFINED:
            assert got is None, cid
            continue
        assert got == want, cid
        if live:
            assert oracle.ref_align(s, t) == want, cid
        n += 1
    assert n >= {"len": 62, "str": 108, "gap": 573, "edge": 24, "tiny": 12, "unrel": 10, "lowc": 10}[fam]


def test_alignment_fixture_keeps_its_undefined_share_and_size():
    """At most 2 % of the table may be undefined in the reference, and nothing outside the unrelated strings; the fixture stays small."""
    golden = ac.golden()
    und = [cid for cid, v in golden.items() if v == ac.UNDEFINED]
    assert all(ac.family(c) == "unrel" for c in und), und
    assert 0 < len(und) <= 0.02 * len(golden), (len(und), len(golden))
    assert os.path.getsize(ac.FIXTURE) < 128 * 1024
    assert len(golden) >= 773


def test_oracle_alignment_of_an_undefined_pair_returns_none():
    """446 x 151 unrelated bases of this kind made the oracle's traceback index S[-1] (forcex still set at i = 0)."""
    und = [(s, t) for cid, s, t in ac.by_family("unrel") if ac.golden()[cid] == ac.UNDEFINED]
    assert und
    for s, t in und:
        assert oracle.align(s, t) is None
    assert oracle.align("C", "ACGT") is None          # the smallest one: T's first base against a gap, then S's only base against a gap
    assert oracle.align("ACGT", "C") is None          # ... and its mirror image (forcey still set at j = 0)


def test_std_hash_known_answers():
    """libstdc++ std::hash<std::string> values that node-table order depends on."""
    kat = {"ACGT": 2120050921807290424, "source1": 5824865595435910722, "ACGTACGTACGTA": 613407185026648748,
           "ACGTACGTACGTACGT": 8653344979867301840, "AAAAACCCCCGGGGGTTTTTACGTA": 11793684898630242514}
    for s, h in kat.items():
        assert oracle.std_hash(s) == h
