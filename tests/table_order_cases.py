"""Windows engineered so that the node table of a graph lands ON the edges of the table-order code (kernels.h ht_insert / first_lowcov /
order_insert, build_lds_impl.h from BL_TAIL_PRIO_SET to `H->have_order = 1` and its wide form): an exact number of distinct k-mers N next
to every bucket count of libstdc++'s growth chain, next to the switches between the forms of the stage loop and next to the hand-off
capacities; every k-mer a survivor with N next to a bucket count, so that the insertion of the two special nodes rehashes or just does
not; 31 to 40 components; and the same table as a window's first graph, as a graph built ahead and as one the build service builds.
Shared by test_table_order_windows_emu.py (both host builds of the kernels) and test_table_order_gpu.py (the device).

How a window reaches an exact N (all at odd k, min_k == max_k unless stated):
  1. a random reference without a repeated canonical k-mer, and perfect reads over it, deep enough that every reference k-mer survives;
  2. junk reads of random sequence, seen once each: nodes that do not survive the first removeLowCov;
  3. a last junk read of k - 1 + d bases that adds exactly d k-mers.
N is counted here as a plain set of canonical strings, and a draw that misses is drawn again.  The checker is the oracle: its table dump
(oracle.run(order_dump=True)) is a real std::unordered_map's iteration, and every case states on THAT what makes it its edge before a
device value is looked at (assert_oracle_side)."""
from __future__ import annotations

import functools

import numpy as np

from lancet_amd import abi, frontend
from lancet_amd.frontend import FWD, NML, REV, TMR
from oracle import oracle

CHAIN = [13, 29, 59, 127, 257, 541, 1109, 2357, 5087, 10273, 20753]
K = 21
NARROW_CAP, WIDE_CAP, ORDER_CAP = 5632, 14336, 4096          # layout.h PB_NCAP / PB_NCAP_WIDE ; build_lds_impl.h: the 512-lane form orders up to 4096 nodes
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def rc(s):
    return "".join(_COMP[c] for c in reversed(s))


def canon(s):
    r = rc(s)
    return s if s < r else r


def kmers(seq, k):
    """the canonical k-mers loadSequence makes nodes of: none for a sequence of k bases or fewer (reference src/Graph.cc:140)"""
    return {canon(seq[i:i + k]) for i in range(len(seq) - k + 1)} if len(seq) > k else set()


def _rand(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def buckets_for(n):
    return next(b for b in CHAIN if b >= n)


class Case:
    def __init__(self, name, k, ref, reads, N=None, nsurv=None, allcomp=None, refcomp=None, big=None, built=None, ends_rehash=None, params=None, second=None):
        self.name, self.k, self.ref, self.reads = name, k, ref, reads
        self.N, self.nsurv, self.allcomp, self.refcomp = N, nsurv, allcomp, refcomp       # asserted on the oracle's dump where not None
        self.big = big                       # the 1024-lane configuration has to build it (more than 512 reads)
        self.built = built                   # None: not stated; else (narrow hand-off, wide hand-off)
        self.ends_rehash = ends_rehash       # the bucket count changes over markRefEnds(1)
        self.params = params or dict(min_k=k, max_k=k)
        self.second = second                 # (k of the first graph that is rejected for a cycle): the case is about the graph at self.k


# ---------------------------------------------------------------- reads

def perfect_reads(seq, k, rl=100, step=10, edge_copies=4):
    """reads over seq such that every k-mer of it is seen at least four times at full quality"""
    if len(seq) <= rl:
        return [seq] * (2 * edge_copies + 2)
    starts = list(range(0, len(seq) - rl + 1, step)) + [len(seq) - rl]
    return [seq[a:a + rl] for a in starts] + [seq[:rl]] * edge_copies + [seq[-rl:]] * edge_copies


def junk_lengths(count, k, rl=150):
    """lengths of junk reads that hold `count` k-mers between them (a read of L > k bases holds L - k + 1, one of k bases none)"""
    per = rl - k + 1
    full, rem = divmod(count, per)
    out = [rl] * full
    if rem == 1:
        assert full > 0, "one junk k-mer alone cannot be had"
        out[-1] -= 1
        rem = 2
    if rem:
        out.append(k - 1 + rem)
    return out


def pack_reads(seqs):
    out = []
    for i, s in enumerate(seqs):
        out.append((f"r{i:05d}", s, "I" * len(s), TMR if i % 2 == 0 else NML, FWD if (i // 2) % 2 == 0 else REV, 1, True))
    return out


def exact_window(rng, name, target, k=K, n_ref=None, big=False, **kw):
    """a window with exactly `target` distinct k-mers of which the n_ref of the reference survive"""
    if n_ref is None:
        n_ref = target if target <= 20 else max(12, min(target // 2, 600))
        if target - n_ref == 1:
            n_ref -= 1
    for _ in range(60):
        ref = _rand(rng, n_ref + k - 1)
        have = kmers(ref, k)
        if len(have) != n_ref:
            continue
        seqs = perfect_reads(ref, k)
        junk = [_rand(rng, L) for L in junk_lengths(target - n_ref, k)]
        for j in junk:
            have |= kmers(j, k)
        if len(have) != target:
            continue
        if big:                                                       # more than 512 reads: the 512-lane configuration turns the window away
            at = rng.integers(0, max(1, len(ref) - (k + 4)), size=520 - len(seqs) - len(junk) if len(seqs) + len(junk) < 520 else 8)
            seqs += [ref[int(a):int(a) + k + 4] for a in at]
        # the junk goes first and the reference pseudo-read last: node ids run through the junk, the survivors are spread over the table
        return Case(name, k, ref, pack_reads(junk + seqs), N=target, nsurv=n_ref, big=big, **kw)
    raise AssertionError(f"{name}: no draw has exactly {target} distinct k-mers")


# ---------------------------------------------------------------- the families

def boundary_targets():
    t = set()
    for b in CHAIN[:-1]:
        t |= {b - 2, b - 1, b, b + 1, b + 2}
    for m in (1024, 2048, 4096, NARROW_CAP, WIDE_CAP):
        t |= {m - 1, m, m + 1}
    return sorted(t)


@functools.lru_cache(maxsize=None)
def family_boundaries():
    """(a) and the 512-lane half of (b): N on and around every bucket count, the stage-loop switches, 4096 | 4097 and both capacities"""
    rng = np.random.default_rng(13)
    # (a table beyond the narrow capacity is the 1024-lane configuration's, and a window goes there for ITS size: more than 512 reads)
    # (at 14335 and 14336 nodes the 1024-lane configuration's table of 16384 slots is 87 % full: whether an insertion then needs more than the
    #  256 probes it may take -- BLW_TABLE, the general build's -- is the hash's business, so `built` is not stated there; 14337 never is)
    full = lambda t: None if WIDE_CAP - 1 <= t <= WIDE_CAP else t <= WIDE_CAP
    return [exact_window(rng, f"N{t}", t, built=(t <= NARROW_CAP, full(t)), big=t > NARROW_CAP) for t in boundary_targets()]


@functools.lru_cache(maxsize=None)
def family_switches_large():
    """(b) on the 1024-lane form: more than 512 reads, N = 2047..2049 and 4095..4097 (4097: its wide table form, whatever the hand-off)"""
    rng = np.random.default_rng(1024)
    return [exact_window(rng, f"large_N{t}", t, built=(True, True), big=True) for t in (1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097)]


@functools.lru_cache(maxsize=None)
def family_tiny():
    """(c) N = 1..14 at k = 3..9 on references of k + 1 .. k + 13 bases (max_mismatch 0: at k = 3 two mismatches make every string a near-repeat)"""
    rng = np.random.default_rng(3)
    out = []
    for k in range(3, 10):
        params = dict(min_k=k, max_k=k, max_mismatch=0)
        half = _rand(rng, (k + 1) // 2)
        one = half + rc(half) if k % 2 else "A" * (k + 1)            # its two k-mers are one canonical k-mer
        assert len(kmers(one, k)) == 1
        out.append(Case(f"tiny_k{k}_N1", k, one, pack_reads([one] * 12), N=1, nsurv=1, params=params))
        for n in range(2, 15):
            if (n + k) % 3 != 0 and n not in (2, 13, 14):              # (every N at two or three k, the ends of the range at every k)
                continue
            for _ in range(4000):
                ref = _rand(rng, n + k - 1)
                if len(kmers(ref, k)) == n:
                    break
            else:
                raise AssertionError(f"tiny k={k} N={n}: no draw")
            out.append(Case(f"tiny_k{k}_N{n}", k, ref, pack_reads([ref] * 12), N=n, nsurv=n, params=params))
    return out


@functools.lru_cache(maxsize=None)
def family_all_survive():
    """(d) every k-mer a survivor and N = nsurv in {B - 2, B - 1, B}: markRefEnds' two insertions do not rehash, rehash at the second, at the first"""
    rng = np.random.default_rng(29)
    out = []
    for b in (29, 59, 127, 257, 541):
        for n in (b - 2, b - 1, b):
            out.append(exact_window(rng, f"all_B{b}_N{n}", n, n_ref=n, built=(True, True), allcomp=1, ends_rehash=n >= b - 1))
    for n in (1107, 1108, 1109):                                      # a reference of 1024 bases and a deeply covered insertion haplotype
        for _ in range(60):
            ref = _rand(rng, 1024)
            ins = _rand(rng, n - (1024 - K + 1) - (K - 1))
            hap = ref[:500] + ins + ref[500:]
            if len(kmers(ref, K)) == 1024 - K + 1 and len(kmers(ref, K) | kmers(hap, K)) == n:
                break
        else:
            raise AssertionError(f"B=1109 N={n}: no draw")
        lo, hi = 500 - 110, 500 + len(ins) + 110
        seqs = perfect_reads(ref, K) + perfect_reads(hap[lo:hi], K, step=4)
        out.append(Case(f"all_B1109_N{n}", K, ref, pack_reads(seqs), N=n, nsurv=n, built=(True, True), allcomp=1, ends_rehash=n >= 1108))
    return out


def _contigs(rng, count, length=24):
    return [_rand(rng, length) for _ in range(count)]


@functools.lru_cache(maxsize=None)
def family_components():
    """(e) 31, 32, 33 and 40 components: stretches of the reference (all on the reference), junk contigs (none), and a mix in which the
    one reference component is numbered above 32"""
    rng = np.random.default_rng(40)
    out = []
    for c in (31, 32, 33, 40):
        for _ in range(60):
            ref = _rand(rng, 1024)
            if len(kmers(ref, K)) == 1024 - K + 1:
                break
        period = 1024 // c
        seqs = [ref[i * period:i * period + 24] for i in range(c) for _ in range(6)]
        out.append(Case(f"ref_stretches_{c}", K, ref, pack_reads(seqs), N=1024 - K + 1, nsurv=4 * c, allcomp=c, refcomp=c, built=(True, True)))
        ref = _rand(rng, 200)
        seqs = [s for s in _contigs(rng, c) for _ in range(6)]
        out.append(Case(f"junk_contigs_{c}", K, ref, pack_reads(seqs), nsurv=4 * c, allcomp=c, refcomp=0, built=(True, True)))
    for i in range(400):                                              # where the reference component is numbered is the table's business: draw until it is above 32
        ref = _rand(rng, 200)
        seqs = [s for s in _contigs(rng, 39) + [ref[80:104]] for _ in range(6)]
        case = Case("ref_component_above_32", K, ref, pack_reads(seqs), nsurv=160, allcomp=40, refcomp=1, built=(True, True))
        dump = oracle.run(batch_of([case]), abi.default_params(**case.params), order_dump=True)[3]
        g = dump.get((0, K))
        if g and g["refcomp"] == 1 and g["touch_ref"].any() and int(g["comp"][g["touch_ref"]].min()) > 32:
            out.append(case)
            break
    else:
        raise AssertionError("no draw numbers the reference component above 32")
    return out


def _climbing(rng, name, dup, k1, k2, target=None, big=False, **kw):
    """a tumour haplotype with a tandem duplication of `dup` bases: every graph at k <= dup has a cycle (a read holds a k-mer twice), the one
    at k2 = the first odd k above dup is kept; junk tops the table of THAT graph up to `target`"""
    for _ in range(60):
        ref = _rand(rng, 400)
        hap = ref[:200] + ref[200 - dup:200] + ref[200:]
        have = kmers(ref, k2) | kmers(hap, k2)
        if len(kmers(ref, k1)) != 400 - k1 + 1 or len(kmers(ref, k2)) != 400 - k2 + 1 or len(kmers(hap, k2)) != len(hap) - k2 + 1:
            continue                                                  # (the base behind the duplication equals its first base: the repeat is one longer)
        junk = [_rand(rng, L) for L in junk_lengths(target - len(have), k2)] if target else []
        n_surv = len(have)
        for j in junk:
            have |= kmers(j, k2)
        if target and len(have) != target:
            continue
        # (the read that brings the duplicated k-mers into the table holds both copies: what the build kernel's `heavy` hint looks for)
        seqs = junk + [hap[150:250 + dup]] + perfect_reads(hap, k2) + perfect_reads(ref, k2)
        if big:                                                       # more than 512 reads: the 1024-lane configuration's window
            seqs += [ref[int(a):int(a) + k2 + 4] for a in rng.integers(0, 400 - (k2 + 4), size=520 - len(seqs))]
        return Case(name, k2, ref, pack_reads(seqs), N=len(have), nsurv=n_surv, params=dict(min_k=k1, max_k=k2), second=k1, big=big, **kw)
    raise AssertionError(f"{name}: no draw")


@functools.lru_cache(maxsize=None)
def family_later_graphs():
    """(f) the boundary at the SECOND k of a heavy window (k = 19 has a cycle, the graph at k = 21 has N = 541 | 542 | 1109 | 1110), and a
    window whose k climbs through twelve graphs.  Who builds the second graph: the build kernel builds ahead for a heavy window that has
    512 windows of the batch behind it (build_lds_impl.h BL_END_G) or that its 1024-lane configuration builds -- the `ahead_` cases, with
    more than 512 reads; the others' second graph is the build service's."""
    rng = np.random.default_rng(19)
    out = [_climbing(rng, f"second_k_N{t}", 20, 19, 21, target=t) for t in (541, 542, 1109, 1110)]
    out += [_climbing(rng, f"ahead_second_k_N{t}", 20, 19, 21, target=t, big=True) for t in (541, 542)]
    out.append(_climbing(rng, "many_k", 40, 19, 41))
    return out


FAMILIES = {"boundaries": family_boundaries, "switches_large": family_switches_large, "tiny": family_tiny, "all_survive": family_all_survive,
            "components": family_components, "later_graphs": family_later_graphs}


# ---------------------------------------------------------------- batches and the oracle

def batch_of(cases):
    wins, reads = [], []
    for w, c in enumerate(cases):
        start = 1000 + 3000 * w
        wins.append(frontend.Window(f"chr22:{start}-{start + len(c.ref)}", "chr22", start, start + len(c.ref), c.ref))
        reads.append(c.reads)
    return frontend.build_batch(wins, reads)


@functools.lru_cache(maxsize=None)
def groups(family):
    """the cases of a family by parameter set: [(params dict, [Case], batch)]"""
    by = {}
    for c in FAMILIES[family]():
        by.setdefault(tuple(sorted(c.params.items())), []).append(c)
    return [(dict(key), cases, batch_of(cases)) for key, cases in by.items()]


@functools.lru_cache(maxsize=None)
def oracle_of(family, gi):
    """(records, stats, -v trace, table dump) of group gi of the family"""
    params, _, batch = groups(family)[gi]
    return oracle.run(batch, abi.default_params(**params), verbose=True, order_dump=True)


def assert_oracle_side(family, gi):
    """what makes every case of the group its edge, on the oracle's dump alone"""
    _, cases, _ = groups(family)[gi]
    dump = oracle_of(family, gi)[3]
    for w, c in enumerate(cases):
        g = dump.get((w, c.k))
        assert g is not None and "hashes" in g, (c.name, "no graph at k", c.k, sorted(k for k in dump if k[0] == w))
        if c.N is not None:
            assert g["N"] == c.N, (c.name, "N", g["N"])
            assert g["buckets_built"] == buckets_for(c.N), (c.name, "bucket count", g["buckets_built"])
            # on both sides of the boundary: one k-mer more than a bucket count and the table has grown, at the bucket count it has not
            if c.N in CHAIN:
                assert g["buckets_built"] == c.N
            if c.N - 1 in CHAIN:
                assert g["buckets_built"] > c.N
        assert g["buckets"] == g["buckets_built"], c.name           # (erasing never shrinks the table)
        if c.nsurv is not None:
            assert len(g["hashes"]) == c.nsurv, (c.name, "nsurv", len(g["hashes"]))
        if c.allcomp is not None:
            assert g["allcomp"] == c.allcomp, (c.name, "allcomp", g["allcomp"])
        if c.refcomp is not None:
            assert g["refcomp"] == c.refcomp, (c.name, "refcomp", g["refcomp"])
        if c.ends_rehash is not None:
            assert (g["buckets_ends"] != g["buckets"]) == c.ends_rehash, (c.name, g["buckets"], g["buckets_ends"])
            if c.ends_rehash:
                assert g["buckets_ends"] == buckets_for(2 * g["buckets"])
        if c.second is not None:
            first = dump.get((w, c.second))
            assert first is not None and "hashes_ends" in first and "hashes_compressed" not in first, (c.name, "the graph at the first k is not one given up for a cycle")
            assert "hashes_compressed" in g, c.name
        if c.name == "many_k":
            assert len([k for k in dump if k[0] == w]) == 12, sorted(k for k in dump if k[0] == w)
        if c.name == "ref_component_above_32":
            assert int(g["comp"][g["touch_ref"]].min()) > 32


# ---------------------------------------------------------------- device values against the dump

def assert_orders_equal_oracle(family, gi, pre_orders, wide, what=""):
    """pre_orders[w]: the graphs of window w that the hand-off areas hold (engine.parse_pre_order), against the oracle's dump: per graph
    the build kernel built the hash sequence of the survivors, comp per position, numcomp, refcomp, the bucket count; with PreCmp::done the
    table after compress(1), and done only where markRefEnds(1) left the bucket count alone.  have_order exactly where the rule says: built,
    nsurv > 0 and N <= 4096, or the 1024-lane form and N <= 14336.  Returns how many graphs carried an order / a compressed table."""
    _, cases, _ = groups(family)[gi]
    dump = oracle_of(family, gi)[3]
    assert len(pre_orders) == len(cases)
    n_order = n_done = 0
    for w, c in enumerate(cases):
        graphs = pre_orders[w]
        assert graphs, (what, c.name, "no hand-off area read")
        if c.built is not None and c.built[1 if wide else 0] is not None:
            assert graphs[0]["built"] == c.built[1 if wide else 0], (what, c.name, "built", graphs[0])
        if c.big is not None and graphs[0]["built"]:
            assert bool(graphs[0]["big"]) == c.big, (what, c.name, "1024-lane configuration", graphs[0]["big"])
        for g in graphs:
            if not g["built"]:
                continue
            tag = (what, c.name, "k", g["K"])
            o = dump.get((w, g["K"]))
            assert o is not None, tag + ("a graph the reference never builds",)
            assert g["N"] == o["N"] and g["nsurv"] == len(o["hashes"]), tag + (g["N"], g["nsurv"], o["N"], len(o["hashes"]))
            expect = len(o["hashes"]) > 0 and (o["N"] <= ORDER_CAP or (bool(g["big"]) and o["N"] <= WIDE_CAP))
            assert bool(g["have_order"]) == expect, tag + ("have_order", g["have_order"], "N", o["N"], "nsurv", len(o["hashes"]), "big", g["big"])
            if not g["have_order"]:
                assert not g["done"], tag
                continue
            n_order += 1
            bad = np.nonzero(g["hashes"] != o["hashes"])[0]
            assert len(bad) == 0, tag + ("table order: %d of %d positions differ, the first %s" % (len(bad), len(o["hashes"]), bad[:4]),)
            bad = np.nonzero(g["comp"] != o["comp"])[0]
            assert len(bad) == 0, tag + ("comp: %d positions differ, the first %s: %s, the oracle's %s" % (len(bad), bad[:4], g["comp"][bad[:4]], o["comp"][bad[:4]]),)
            assert (g["numcomp"], g["refcomp"]) == (o["allcomp"], o["refcomp"]), tag + ("numcomp, refcomp", g["numcomp"], g["refcomp"], o["allcomp"], o["refcomp"])
            assert g["ht_bc"] == o["buckets"] and g["ht_next_resize"] == o["buckets"], tag + ("bucket count", g["ht_bc"], g["ht_next_resize"], o["buckets"])
            if g["done"]:
                assert o["buckets_ends"] == o["buckets"], tag + ("PreCmp::done where markRefEnds(1) rehashes",)
                if "hashes_compressed" in o:                          # (absent: the reference met a cycle before its compress -- the window kernel meets it behind this one)
                    n_done += 1
                    assert g["m_live"] == len(o["hashes_compressed"]) and (g["live_hashes"] == o["hashes_compressed"]).all(), tag + ("the table after compress(1)",)
    return n_order, n_done


KEY = lambda s: (s["status"], s["final_k"], s["n_builds"], s["n_variants"], s["n_kmers"], s["max_nodes"])


def assert_results_equal_oracle(family, gi, got, what=""):
    """records, per-window statistics and the -v trace (by its digest) against the oracle's"""
    import golden_util as gu
    (v, st, tr), (ov, ost, otr, _) = got, oracle_of(family, gi)
    bad = [(w, KEY(a), KEY(b)) for w, (a, b) in enumerate(zip(st, ost)) if KEY(a) != KEY(b)]
    assert not bad and len(st) == len(ost), (what, bad[:4])
    assert v == ov, what
    assert gu.digest_trace(tr) == gu.digest_trace(otr), what
