"""Hand-made windows around the rule by which the build kernel SETTLES a window (build_lds_impl.h, "settled windows"):
the graph after the first removeLowCov is the window reference's own k-mers in one chain and nothing else.  Every case states whether it
is settled, and every case is held against the oracle with settling on and with settling off.  Shared by test_settle_emu.py (host build
of the kernels) and test_settle_gpu.py (the device).

Windows of 240 bases, reads of 100 bases, k = 21 (min_k == max_k) unless the case says otherwise.  The helpers are those of
table_order_cases.py: perfect reads see every k-mer of a sequence at least four times, a junk read is random sequence seen once."""
from __future__ import annotations

import functools

import numpy as np

from lancet_amd import abi, frontend, workload
from oracle import oracle
from table_order_cases import _rand, batch_of, kmers, pack_reads, perfect_reads, rc

K = 21
REFLEN = 240
KEYS = ("status", "final_k", "n_builds", "n_variants", "n_kmers", "max_nodes")


class SCase:
    def __init__(self, name, ref, reads, settled, params=None, records=None, climbs=False):
        self.name, self.ref, self.reads = name, ref, reads
        self.settled = settled               # True / False: asserted ; None: either route (the case is about the result alone)
        self.params = params or dict(min_k=K, max_k=K)
        self.records = records               # None: not stated ; 0: none ; 1: at least one (asserted on the oracle's side)
        self.climbs = climbs                 # the oracle builds more than one graph
        self.k = self.params["min_k"]        # (table_order_cases.batch_of reads no more than ref and reads)


def _plain_ref(rng, n=REFLEN, k=K):
    """a random reference without a repeated canonical k-mer (no k-mer next to its reverse complement either)"""
    for _ in range(100):
        ref = _rand(rng, n)
        if len(kmers(ref, k)) == n - k + 1:
            return ref
    raise AssertionError("no reference without a repeated canonical k-mer")


def _snv(ref, at):
    return ref[:at] + {"A": "C", "C": "G", "G": "T", "T": "A"}[ref[at]] + ref[at + 1:]


def _junk(rng, n=6, rl=100):
    return [_rand(rng, rl) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(41)
    out = []
    # (a) perfect reads over the reference only, junk below the coverage cut
    ref = _plain_ref(rng)
    out.append(SCase("a_reference_only", ref, pack_reads(_junk(rng) + perfect_reads(ref, K)), True, records=0))
    # (b) the same plus a heterozygous SNV at full coverage
    ref = _plain_ref(rng)
    out.append(SCase("b_het_snv", ref, pack_reads(_junk(rng) + perfect_reads(ref, K) + perfect_reads(_snv(ref, 120), K)), False, records=1))
    # (c) every read carries the SNV: the reference k-mers over it are seen by the pseudo-read alone and go, the chain runs through non-reference nodes
    ref = _plain_ref(rng)
    out.append(SCase("c_hom_snv", ref, pack_reads(perfect_reads(_snv(ref, 120), K)), False, records=1))
    # (d) the reference's last (k - 1)-mer recurs earlier -- at its start, the one place where the reference passes the near-repeat test at this
    #     k (util.cc isAlmostRepeat compares windows of k + 1 bases, and none holds the first copy with a base in front of it) -- and reads that
    #     run from its end into its start add the back edge last node -> first node.  Default k range: k climbs over the exact repeat to 21.
    for _ in range(100):
        R = _rand(rng, K - 1)
        ref = R + _rand(rng, REFLEN - 2 * (K - 1)) + R
        if len(kmers(ref, K)) == REFLEN - K + 1:
            break
    back = ref[-60:] + ref[K - 1:K - 1 + 40]
    out.append(SCase("d_back_edge", ref, pack_reads(perfect_reads(ref, K) + [back] * 6), False, params=dict(min_k=11, max_k=101)))
    # (d2) the back edge that the reference's own clipping of the ends cannot remove: the reverse complement of an inner (k - 1)-mer further on,
    #      and reads that turn round at it.  Every node is a reference node at one offset, the near-repeat test (forward strings) passes, and
    #      hasCycle meets a grey node: the oracle climbs.
    for _ in range(100):
        R = _rand(rng, K - 1)
        ref = _rand(rng, 70) + R + _rand(rng, 60) + rc(R) + _rand(rng, REFLEN - 130 - 2 * (K - 1))
        if len(kmers(ref, K)) == REFLEN - K + 1:
            break
    p, q = 70, 70 + (K - 1) + 60
    turn = ref[p - 50:p + K - 1] + rc(ref[q - 30:q])
    out.append(SCase("d2_turn_round", ref, pack_reads(perfect_reads(ref, K) + [turn] * 6), False, params=dict(min_k=11, max_k=101), climbs=True))
    # (e) a k-mer and its reverse complement in the reference: one node at two offsets
    for _ in range(100):
        M = _rand(rng, K)
        ref = _rand(rng, 60) + M + _rand(rng, 70) + rc(M) + _rand(rng, REFLEN - 130 - 2 * K)
        if len(kmers(ref, K)) == REFLEN - K:
            break
    out.append(SCase("e_kmer_and_revcomp", ref, pack_reads(perfect_reads(ref, K)), False))
    # (f) no node reaches cov_threshold (5) though every one survives (2 .. 4 reads over each k-mer): no source
    ref = _plain_ref(rng)
    tile = [ref[a:a + 100] for a in range(0, REFLEN - 100 + 1, 50)] + [ref[-100:]]
    out.append(SCase("f_no_source", ref, pack_reads(tile + tile[:-1]), None, records=0))
    # (g) no read over the middle: two chains, two components
    ref = _plain_ref(rng)
    out.append(SCase("g_two_chains", ref, pack_reads(perfect_reads(ref[:110], K) + perfect_reads(ref[130:], K)), False))
    # (h) an N in the window reference
    ref = _plain_ref(rng)
    out.append(SCase("h_N_in_reference", ref[:120] + "N" + ref[121:], pack_reads(perfect_reads(ref, K)), False))
    # (i) survivors that stop short of both window ends, the outermost of them seen two to four times: the anchors lie inside the run
    ref = _plain_ref(rng)
    out.append(SCase("i_short_of_both_ends", ref, pack_reads(_junk(rng, 3) + perfect_reads(ref[20:220], K, edge_copies=1)), True, records=0))
    return out


@functools.lru_cache(maxsize=None)
def groups():
    """the cases by parameter set: [(params dict, [SCase], batch)]"""
    by = {}
    for c in cases():
        by.setdefault(tuple(sorted(c.params.items())), []).append(c)
    return [(dict(key), cs, batch_of(cs)) for key, cs in by.items()]


@functools.lru_cache(maxsize=None)
def oracle_of(gi):
    """(records, stats, -v trace) of group gi"""
    params, _, batch = groups()[gi]
    return oracle.run(batch, abi.default_params(**params), verbose=True)


def assert_oracle_side(gi):
    """what the cases state about the reference's own outcome, before a device value is looked at"""
    _, cs, _ = groups()[gi]
    ov, ost, _ = oracle_of(gi)
    for w, c in enumerate(cs):
        n = sum(1 for v in ov if v["window"] == w)
        if c.settled is not False:                                 # (a window that is not settled may end any way: (e) runs out of k on its cycle)
            assert ost[w]["status"] == 0, (c.name, ost[w])
        if c.records == 0:
            assert n == 0, (c.name, n)
        if c.records == 1:
            assert n >= 1, (c.name, "no record")
        if c.settled:
            assert ost[w]["n_builds"] == 1 and n == 0, (c.name, ost[w], n)
        if c.climbs:
            assert ost[w]["n_builds"] >= 2, (c.name, ost[w])


def assert_case_results(gi, on, off, settled_windows, device=False, what=""):
    """on / off: (records, stats) of the route with settling on and with it off; settled_windows: the windows the build kernel settled"""
    _, cs, _ = groups()[gi]
    ov, ost, _ = oracle_of(gi)
    keys = KEYS + (("sum_nodes",) if device else ())
    for tag, (v, st) in (("on", on), ("off", off)):
        bad = [(cs[w].name, [a[k] for k in keys], [b[k] for k in keys]) for w, (a, b) in enumerate(zip(st, ost)) if any(a[k] != b[k] for k in keys)]
        assert not bad and len(st) == len(ost), (what, tag, bad[:4])
        assert v == ov, (what, tag, "records")
    for w, c in enumerate(cs):
        if c.settled is not None:
            assert (w in settled_windows) == c.settled, (what, c.name, "settled" if w in settled_windows else "not settled")


# ---------------------------------------------------------------- the scan batch

SCAN = dict(n=400, cov_t=30, cov_n=30, seed=5)
P_EXPECTED = 99            # the plain reference chains of this batch, counted on the oracle's trace (below)


@functools.lru_cache(maxsize=None)
def scan_batch(n=None):
    b = workload.make_scan_batch(SCAN["n"], SCAN["cov_t"], SCAN["cov_n"], seed=SCAN["seed"])
    return b if n is None else workload.sub_batch(b, 0, n)


@functools.lru_cache(maxsize=None)
def scan_oracle(n=None):
    return oracle.run(scan_batch(n), abi.default_params(), verbose=True)


def plain_chains(trace, records, batch):
    """The windows P of the oracle's -v trace that are plain reference chains: a single build, `comp: 1`, edges == 2 * (nodes - 1) after the
    first removeLowCov, nodes <= reflen - k + 1, at most 5 nodes after the first compress, and no record."""
    import re
    blocks = trace.split("== Processing ")[1:]
    have_rec = {v["window"] for v in records}
    by_name = {}
    for blk in blocks:
        m = re.match(r"\d+: (\S+) ", blk)
        by_name[m.group(1)] = blk
    out = []
    for w in range(batch.n_windows):
        blk = by_name.get(batch.hdr[w])
        if blk is None or w in have_rec:
            continue
        reads = re.findall(r"^reads: \d+ reflen: (\d+) ", blk, re.M)
        if len(reads) != 1:                                          # one build
            continue
        reflen = int(reads[0])
        lines = blk.split("\n")
        try:
            i = next(j for j, ln in enumerate(lines) if ln.startswith("removing low coverage:"))
        except StopIteration:
            continue
        m = re.match(r"\s+0: nodes: (\d+) edges: (\d+) ", lines[i + 1])
        if not m:
            continue
        nodes, edges = int(m.group(1)), int(m.group(2))
        mc = re.search(r"^ nodes: \d+ refnodes: \d+ comp: (\d+) refcomp: (\d+)", blk, re.M)
        if not mc or int(mc.group(1)) != 1:
            continue
        k = _first_build_k(blk)
        if k is None or edges != 2 * (nodes - 1) or nodes > reflen - k + 1:
            continue
        try:
            j = next(j for j, ln in enumerate(lines) if ln.startswith("compressing graph:"))
        except StopIteration:
            continue
        m = re.match(r"\s+1: nodes: (\d+) ", lines[j + 1])
        if not m or int(m.group(1)) > 5:
            continue
        out.append(w)
    return out


def _first_build_k(blk):
    """k of the block's one graph: span of the whole table / its nodes (printStats: span = nodes * k before any compress)"""
    import re
    m = re.search(r"^\s+0: nodes: (\d+) edges: \d+ span: (\d+)", blk, re.M)
    if not m or int(m.group(1)) == 0:
        return None
    return int(m.group(2)) // int(m.group(1))


# ---------------------------------------------------------------- --linked-reads

@functools.lru_cache(maxsize=None)
def linked_group():
    """(params dict, [SCase], batch): the k = 21 cases with a barcode and a haplotype on every read, for a run with --linked-reads"""
    params, cs, _ = groups()[0]
    wins, reads = [], []
    for w, c in enumerate(cs):
        start = 1000 + 3000 * w
        wins.append(frontend.Window(f"chr22:{start}-{start + len(c.ref)}", "chr22", start, start + len(c.ref), c.ref))
        reads.append([r + ("ACGTACGTACGTAC%02d-1" % (i % 17), i % 3) for i, r in enumerate(c.reads)])
    return dict(params, lr_mode=1), cs, frontend.build_batch(wins, reads, linked=True)
