"""Shared by test_haplotype_coverage_emu.py / test_haplotype_coverage_gpu.py: what a run with the haplotypes' coverages
(lancet_engine_set_haplotype_coverage) has to return.  The expected numbers come from the REFERENCE, never from the code under test: the
tables its Graph_t::printVerticalAlignment printed under -V for the five cases of tests/golden/more_verbose/
(tests/golden/hap_cov/<case>.tables.txt.gz, tools/make_haplotype_coverage_goldens.py), and for hand-made windows a plain model of its
Ref_t::computeCoverage (src/Ref.cc:186-250) and the reads' own strand and sample counts.
A haplotype is one of abi.haplotypes_to_py's dicts with "cov" = {"path": len x 4 uint16 (an+ an- at+ at-), "ref": ref_len x 4 (rn+ rn- rt+ rt-)}."""
from __future__ import annotations

import functools
import gzip
import os

import numpy as np

import golden_util as gu
import hap_align_cases as hac
import hap_cases as hc
from lancet_amd import abi, frontend
from lancet_amd.frontend import FWD, NML, REV, TMR

DIR = os.path.join(gu.GOLDEN, "hap_cov")
HEADER = "Pos\tr\tp\td\tan+\tan-\tat+\tat-\trn+\trn-\trt+\trt-"
_D = {"=": " ", "X": "x", "I": "^", "D": "v"}           # printVerticalAlignment's mark of a column class (reference src/Graph.cc:761-764)


def golden_text(case: str) -> str:
    return gzip.open(os.path.join(DIR, f"{case}.tables.txt.gz"), "rt").read()


@functools.lru_cache(maxsize=None)
def golden_tables(case: str):
    """The reference's tables of the case, one per processPath call in order: each a list of rows, each row its 12 cells."""
    tabs = []
    for l in golden_text(case).splitlines():
        if l == HEADER:
            tabs.append([])
        else:
            tabs[-1].append(l.split("\t"))
    return tabs


def table_text(r: str, p: str, h) -> str:
    """The table printVerticalAlignment prints for stretch r, path string p, from the haplotype's CIGAR and coverages: `Pos` is the path
    index and stays on a deletion column, the four cells of the side that has a gap are empty."""
    out, k, j = [HEADER], 0, 0
    pc, rc = h["cov"]["path"], h["cov"]["ref"]
    for n, op in h["cigar"]:
        for _ in range(n):
            a = "\t".join(str(int(x)) for x in pc[k]) if op != "D" else "\t\t\t"
            b = "\t".join(str(int(x)) for x in rc[j]) if op != "I" else "\t\t\t"
            out.append(f"{k}\t{r[j] if op != 'I' else '-'}\t{p[k] if op != 'D' else '-'}\t{_D[op]}\t{a}\t{b}")
            k += op != "D"
            j += op != "I"
    return "".join(l + "\n" for l in out)


def check_shape(haps):
    for h in haps:
        c = h["cov"]
        assert c["path"].shape == (h["len"], 4) and c["ref"].shape == (h["ref_len"], 4), (h["window"], h["index"])
        assert c["path"].dtype == np.uint16 and c["ref"].dtype == np.uint16
        assert h["flags"] & abi.HAP_HAS_COVERAGE


def check_tables(case: str, batch, haps):
    """Every haplotype's arrays are the numbers of the reference's table for that path, the columns laid out from its CIGAR, in order."""
    tabs = golden_tables(case)
    assert len(tabs) == len(haps)
    check_shape(haps)
    rows = []
    for h, tab in zip(haps, tabs):
        got = table_text(hc.stretch(batch, h), h["seq"], h).splitlines()[1:]
        want = ["\t".join(x) for x in tab]
        assert len(got) == len(want), (h["window"], h["index"], len(got), len(want))
        for i, (a, b) in enumerate(zip(got, want)):
            assert a == b, (h["window"], h["index"], i, a, b)
        rows += tab
    return rows


def check_set(rows_by_case):
    """What the fixtures must hold (the generator's own check_set), counted on the committed files."""
    rows = [x for r in rows_by_case.values() for x in r]
    assert any(x[3] == "^" for x in rows) and any(x[3] == "v" for x in rows)
    assert any(x[3] != "v" and (x[4] != x[5] or x[6] != x[7]) for x in rows)            # swapped strands cannot pass
    assert any(x[3] != "^" and (x[8] != x[9] or x[10] != x[11]) for x in rows)
    assert any(x[3] != "v" and (x[4], x[5]) != (x[6], x[7]) for x in rows)              # ... nor swapped samples


def words_of(h) -> int:
    """Words of its window's buffer a haplotype takes with its CIGAR (where it has one) and its coverages."""
    return hc.words_of(h) + len(h.get("cigar", ())) + 2 * (h["len"] + h["ref_len"])


def ample_words(batch, p) -> int:
    """lancet_gpu's size for the batch with --haplotype-coverage: --haplotype-sam's plus 2 * 2 words per base of 32 paths and stretches."""
    longest = max(int(batch.ref_off[w + 1] - batch.ref_off[w]) for w in range(batch.n_windows))
    return hac.ample_words(batch, p) + 32 * 2 * (2 * longest + int(p.max_indel_len) + 256)


def norm(haps) -> list:
    """The dicts with their arrays as lists: comparable with ==."""
    return [{k: ((x["path"].tolist(), x["ref"].tolist()) if k == "cov" else x) for k, x in h.items()} for h in haps]


def strip_cov(haps) -> list:
    """The dicts as a run without the coverages returns them -- the flag bit included."""
    return [{k: (x & ~abi.HAP_HAS_COVERAGE if k == "flags" else x) for k, x in h.items() if k != "cov"} for h in haps]


# ---------------------------------------------------------------- hand-made single-path windows at the edges of a lane trip

# name -> (reference length, deleted base, inserted base).  Every read spans the window and spells the changed string: one path.  A deletion
# makes the path one base shorter than the stretch, an insertion one longer: together path and stretch cover 62..66, 126..130 and 511..513.
EDGES = {
    "r63_p62": (63, 20, None), "r64_p63": (64, 20, None), "r65_p64": (65, 20, None), "r66_p65": (66, 20, None), "r64_p65": (64, None, 20),
    "r127_p126": (127, 70, None), "r128_p127": (128, 70, None), "r129_p128": (129, 70, None), "r130_p129": (130, 70, None), "r128_p129": (128, None, 70),
    "r512_p511": (512, 300, None), "r512_p513": (512, None, 300), "r513_p512": (513, 300, None),      # (the largest entry: not the last window)
}
N_FWD = {TMR: 4, NML: 2}           # reads per strand and sample: every path base reads an+ an- at+ at- = 2 2 4 4


@functools.lru_cache(maxsize=None)
def edge_batch():
    """(batch, params, names, reads): one window per EDGES entry, in its order; reads[w] = [(sequence, sample, strand)]."""
    rng = np.random.default_rng(41)
    wins, reads, names, plain = [], [], [], []
    for w, (name, (L, dele, ins)) in enumerate(EDGES.items()):
        ref = "".join("ACGT"[i] for i in rng.integers(0, 4, size=L))
        alt = hac._mut(ref, (), dele, ins)
        rs, pl = [], []
        for sample, tag in ((TMR, "T"), (NML, "N")):
            for i in range(2 * N_FWD[sample]):
                strand = FWD if i & 1 else REV
                # (a name of its own each: the second of two overlapping mates adds no coverage, reference src/Graph.cc:269-303)
                rs.append((f"{tag}{i:04d}", alt, "I" * len(alt), sample, strand, 1 + (i & 1), True))
                pl.append((alt, sample, strand))
        start = 1000 + 700 * w
        wins.append(frontend.Window(f"chr22:{start}-{start + L}", "chr22", start, start + L, ref))
        reads.append(rs)
        names.append(name)
        plain.append(pl)
    return frontend.build_batch(wins, reads), abi.default_params(min_k=11, max_k=31), names, plain


_RC = str.maketrans("ACGT", "TGCA")


def _canon(s: str) -> str:
    rc = s.translate(_RC)[::-1]
    return s if s <= rc else rc


def model_ref_cov(ref: str, reads, k: int) -> np.ndarray:
    """Ref_t::computeCoverage (reference src/Ref.cc:186-250) over a window reference that is its own stretch: the table holds, per canonical
    k-mer of the reference (those with i + k < length: indexMers, src/Ref.cc:40-64), the reads of each sample and strand that contain it; the
    first k-mer's counts go to bases 0..k-1, k-mer i's to base i + k - 1, and the last base is never written.  Columns rn+ rn- rt+ rt-."""
    table = {}
    for seq, sample, strand in reads:
        col = (0 if sample == NML else 2) + (0 if strand == FWD else 1)
        for m in {_canon(seq[i:i + k]) for i in range(len(seq) - k + 1)}:
            table.setdefault(m, [0, 0, 0, 0])[col] += 1
    cov = np.zeros((len(ref), 4), np.uint16)
    for i in range(len(ref) - k):
        v = table.get(_canon(ref[i:i + k]), [0, 0, 0, 0])
        if i == 0:
            cov[:k] = v
        else:
            cov[i + k - 1] = v
    return cov


def check_edges(batch, names, reads, v, st, haps, trunc):
    """One path per window; every path base reads 2 2 4 4; the stretch's coverage is the model's: 0 where the k-mer that ends at the base
    covers the change, 0 at the last base, the read counts elsewhere."""
    hc.check_shape(batch, st, strip_cov(haps), trunc)
    assert all(s["status"] == 0 for s in st) and not any(trunc)
    assert [h["window"] for h in haps] == list(range(len(names)))
    check_shape(haps)
    full = np.array([N_FWD[NML], N_FWD[NML], N_FWD[TMR], N_FWD[TMR]], np.uint16)
    for name, h, rs in zip(names, haps, reads):
        L, dele, ins = EDGES[name]
        assert (h["ref_off"], h["ref_len"]) == (0, L) and h["len"] == L + (1 if dele is None else -1), name
        assert (h["cov"]["path"] == full[None, :]).all(), name
        k = h["kmer"]
        ref = hc.stretch(batch, h)
        want = model_ref_cov(ref, rs, k)
        assert (h["cov"]["ref"] == want).all(), (name, np.argwhere(h["cov"]["ref"] != want)[:4].tolist())
        # the model itself says what the issue says of it
        at = dele if dele is not None else ins
        assert (want[L - 1] == 0).all(), name
        changed = [j for j in range(L - 1) if (want[j] == 0).all()]
        assert changed and all((want[j] == full).all() for j in range(L - 1) if j not in changed), name
        assert min(changed) >= (0 if at < k else at) and max(changed) <= at + k - 1, (name, changed)
        if "cigar" in h:
            assert sorted(op for _, op in h["cigar"]) == sorted(["=", "=", "D" if ins is None else "I"]), name


def check_many_ts(haps):
    """walk_cases.py's many_ts: 8 forward + 8 reverse tumour reads, all cut from the changed string (12 substitutions), as many normal reads, all
    cut from the reference; two paths, the changed string first.  So no count exceeds 8, the tumour supports every base of the changed path and
    the normal every base of the reference path, and the other sample is missing wherever the path's k-mer holds a substitution."""
    alt, ref = haps
    for h in haps:
        assert int(h["cov"]["path"].max()) <= 8 and int(h["cov"]["ref"].max()) <= 8
    a, r = alt["cov"]["path"].astype(int), ref["cov"]["path"].astype(int)
    assert ((a[:, 2] + a[:, 3]) > 0).all() and ((a[:, 0] + a[:, 1]) == 0).any()
    assert ((r[:, 0] + r[:, 1]) > 0).all() and ((r[:, 2] + r[:, 3]) == 0).any()
    assert (a[:, 2] != a[:, 3]).any() or (r[:, 0] != r[:, 1]).any()                      # (the strands are told apart somewhere)
