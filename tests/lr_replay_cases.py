"""Hand-made --linked-reads windows aimed at the two routes of the barcode / haplotype replay (kernels.h lr_node_replay: one lane, runs
of fewer than 3 or more than 192 occurrences; lr_replay_batches: the whole wave, 3..192), shared by test_lr_replay_windows_emu.py (both
host builds of the kernels) and test_lr_replay_gpu.py (the device).  The replay alone, its pair rule and its grown bits occurrence by
occurrence are held by test_lr_replay_emu.py; here the whole window runs and the checker is the oracle, which keeps the barcodes as
std::string sets like the reference does (reference src/Graph.cc:239-317, src/Node.cc:30-118).

One window: 130..180 reference bases, one substitution carried by a share of the tumour reads; every read has a name of its own (no
overlapping mates) and full-quality ends (trimming does not move it).  2..6 windows make a family:

  few               40 tumour + 30 normal reads of 50 bases, 4 barcodes shared by both samples and both strands, HP random
  null              the same, no read has a barcode
  mixed             40 % without barcode, 6 barcodes
  coop_over_127     165 tumour reads, all forward, all with barcodes of their own, + 20 normal reads; 100 bases, starting within the first
                    20 bases of the window, 12 % on the alternate haplotype: the reference k-mers over the variant have more than 127 and
                    at most 192 occurrences -- the wave's 8-bit counts above 127
  lane_ref_*        400 tumour + 60..100 normal reads of 100 bases, mixed strands, 30 % alternate: the reference k-mers over the variant
                    have 193 occurrences or more -- the one-lane route; with few, distinct (strands 97 : 3 in the tumour: a count above
                    255) and mixed barcodes
  lane_alt          the same at 70 %: the alternate allele's k-mers take the one-lane route; low-quality bases ('+') inside the reads,
                    so that hpX_minqv differs from the plain count

No family holds the pair rule (both LR events of loadSequence's offset 0 precede its coverage events, which shows only where a read's
k-mers at positions 0 and 1 are one node).  Two successive k-mers are one node when all their bases are equal or when the k + 1 bases are
their own reverse complement; a homopolymer in the reference only drives k up, and a palindrome s + rc(s) of k + 1 = 12 bases -- in the
reference beside the variant, or completed by the alternate base, a third of the reads starting on it, half of those without barcode --
makes a node with an edge to itself: k = 11 is skipped (the reference repeats there) or its graph is built, replayed and rejected for
its cycle; 30 draws of either shape all ended at k = 13..19, where the reads' starts are no palindromes.  A node that is on no reported path and is no reference k-mer shows its counts nowhere.  The pair rule
therefore stays with test_lr_replay_emu.py, which drives the replay directly.

Every family states, as asserts on the ORACLE's output and on a plain count of canonical k-mer occurrences at the window's final k, what
makes it a test of the thing it is named after (preconditions())."""
from __future__ import annotations

import functools

import numpy as np

from lancet_amd import abi, frontend
from lancet_amd.frontend import FWD, NML, REV, TMR
from oracle import oracle

COOP_MIN, COOP_MAX = 3, 192             # kernels.h LR_COOP_MIN, LR_COOP_MAX
FAMILIES = ["few", "null", "mixed", "coop_over_127", "lane_ref_few", "lane_ref_distinct", "lane_ref_mixed", "lane_alt"]
N_WINDOWS = {"few": 6, "null": 3, "mixed": 6, "coop_over_127": 3, "lane_ref_few": 2, "lane_ref_distinct": 2, "lane_ref_mixed": 2, "lane_alt": 3}
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def rc(s: str) -> str:
    return "".join(_COMP[c] for c in reversed(s))


def _rand(rng, n: int) -> str:
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def _barcode(rng, mode: str, i: int, sample: str) -> str:
    if mode == "null":
        return "null"
    if mode == "few":
        return "BXFEW%d-1" % int(rng.integers(0, 4))
    if mode == "mixed":
        return "null" if rng.random() < 0.4 else "BXMIX%d-1" % int(rng.integers(0, 6))
    assert mode == "distinct"
    return "BX%s%04d-1" % (sample, i)


def _quality(rng, rl: int, lowq: bool) -> str:
    if not lowq:
        return "I" * rl
    return "I" * 12 + "".join("+" if rng.random() < 0.25 else "I" for _ in range(rl - 24)) + "I" * 12


def _window(rng, w: int, n_t: int, n_n: int, rl: int, alt: float, mode: str, start_max=None, forward_t=0.5, lowq=False):
    L = int(rng.integers(130, 181))
    ref = _rand(rng, L)
    at = L // 2 if start_max is None else 60
    hap = ref[:at] + "ACGT"[("ACGT".index(ref[at]) + 1 + int(rng.integers(0, 3))) % 4] + ref[at + 1:]
    reads = []
    for i in range(n_t + n_n):
        tumour = i < n_t
        j = i if tumour else i - n_t
        src = hap if (tumour and rng.random() < alt) else ref
        a = int(rng.integers(0, (L - rl if start_max is None else start_max) + 1))
        if j < 2 and start_max is None:
            a = 0 if j == 0 else L - rl                            # (both window edges are covered)
        strand = FWD if rng.random() < (forward_t if tumour else 0.5) else REV
        sample = "T" if tumour else "N"
        reads.append((f"{sample}{j:05d}", src[a:a + rl], _quality(rng, rl, lowq), TMR if tumour else NML, strand, 1, True,
                      _barcode(rng, mode, j, sample), int(rng.integers(0, 3))))
    start = 1000 + 1000 * w
    return frontend.Window(f"chr22:{start}-{start + L}", "chr22", start, start + L, ref), reads, (at, hap)


def _draw(rng, w: int, family: str):
    if family in ("few", "null", "mixed"):
        return _window(rng, w, 40, 30, 50, 0.5, family)
    if family == "coop_over_127":
        return _window(rng, w, 165, 20, 100, 0.12, "distinct", start_max=20, forward_t=1.0)
    if family.startswith("lane_ref_"):
        # (distinct: 97 % of the tumour's reads forward, so that one class of the reference allele holds more than 255 barcodes)
        return _window(rng, w, 400, int(rng.integers(60, 101)), 100, 0.3, family[9:], forward_t=0.97 if family == "lane_ref_distinct" else 0.5)
    if family == "lane_alt":
        return _window(rng, w, 400, int(rng.integers(60, 101)), 100, 0.7, ("few", "distinct", "mixed")[w % 3], lowq=True)
    raise AssertionError(family)


def params():
    return abi.default_params(lr_mode=1)


@functools.lru_cache(maxsize=None)
def family(name: str):
    """(batch, (variant offset, alternate haplotype) per window, the oracle's (records, statistics, trace)): N_WINDOWS[name] windows, each
    drawn until the oracle assembles it (status 0) to at least one record."""
    rng = np.random.default_rng(7000 + FAMILIES.index(name))
    made = []
    for w in range(N_WINDOWS[name]):
        for _ in range(60):
            m = _draw(rng, w, name)
            ov, ost, _ = oracle.run(frontend.build_batch([m[0]], [m[1]], linked=True), params())
            if ost[0]["status"] == 0 and len(ov) >= 1:
                break
        else:
            raise AssertionError("no draw of %s assembles to a record" % name)
        made.append(m)
    batch = frontend.build_batch([m[0] for m in made], [m[1] for m in made], linked=True)
    assert batch.n_windows <= 8 and max(int(batch.read_begin[w + 1] - batch.read_begin[w]) for w in range(batch.n_windows)) <= 500
    return batch, [m[2] for m in made], oracle.run(batch, params(), verbose=True)


def _canon(s: str) -> str:
    r = rc(s)
    return s if s < r else r


def occurrences(batch, w: int, k: int):
    """canonical k-mer -> list of (read of the window, position), the reference pseudo-read as the window's last read"""
    seq = batch.seq.tobytes().decode()
    r0, r1 = int(batch.read_begin[w]), int(batch.read_begin[w + 1])
    strs = [seq[int(batch.seq_off[r]):int(batch.seq_off[r + 1])] for r in range(r0, r1)]
    strs.append(batch.ref_bases[int(batch.ref_off[w]):int(batch.ref_off[w + 1])].tobytes().decode())
    occ = {}
    for r, s in enumerate(strs):
        for p in range(len(s) - k + 1):
            occ.setdefault(_canon(s[p:p + k]), []).append((r, p))
    return occ


def allele_runs(batch, w: int, at: int, hap: str, k: int):
    """(occurrence counts of the reference k-mers over the variant, of the alternate allele's k-mers over it)"""
    occ = occurrences(batch, w, k)
    ref = batch.ref_bases[int(batch.ref_off[w]):int(batch.ref_off[w + 1])].tobytes().decode()
    span = range(max(0, at - k + 1), min(at, len(ref) - k) + 1)
    return [len(occ[_canon(ref[i:i + k])]) for i in span], [len(occ.get(_canon(hap[i:i + k]), ())) for i in span]


def preconditions(name: str):
    batch, ats, (ov, ost, _) = family(name)
    assert all(s["status"] == 0 for s in ost), name
    assert len(ov) >= 1, name
    recs = lambda w: [r for r in ov if r["window"] == w]
    if name == "few":                                              # some barcode occurs in both samples on one node
        hit = 0
        for w in range(batch.n_windows):
            r0 = int(batch.read_begin[w])
            for c, oc in occurrences(batch, w, ost[w]["final_k"]).items():
                by = {TMR: set(), NML: set()}
                for r, _ in oc:
                    if r0 + r < int(batch.read_begin[w + 1]) and int(batch.bx_rank[r0 + r]) != frontend.NO_BX:
                        by[int(batch.label[r0 + r])].add(int(batch.bx_rank[r0 + r]))
                hit += 1 if by[TMR] & by[NML] else 0
        assert hit > 100
    if name == "null":
        assert all(not any(r["bx"]) for r in ov) and any(any(r["hp"]) for r in ov)
    if name == "mixed":
        assert any(any(r["bx"]) for r in ov)
    if name == "coop_over_127":
        for w in range(batch.n_windows):
            over, _ = allele_runs(batch, w, *ats[w], ost[w]["final_k"])
            assert COOP_MIN <= min(over) and max(over) <= COOP_MAX, (w, over)
        assert any(r["cov"][2] > 127 for r in ov), [r["cov"] for r in ov]          # (RCT fwd)
    if name.startswith("lane_ref_"):
        for w in range(batch.n_windows):
            over, _ = allele_runs(batch, w, *ats[w], ost[w]["final_k"])
            assert min(over) > COOP_MAX, (w, over)
        if name == "lane_ref_distinct":
            assert any(max(r["cov"]) > 255 for r in ov), [r["cov"] for r in ov]
    if name == "lane_alt":
        for w in range(batch.n_windows):
            _, alts = allele_runs(batch, w, *ats[w], ost[w]["final_k"])
            assert min(alts) > COOP_MAX, (w, alts)
        assert any(r["cov"][6] + r["cov"][7] > COOP_MAX for r in ov if r["window"] == 1), [r["cov"] for r in ov]      # (ACT, the window of distinct barcodes)
