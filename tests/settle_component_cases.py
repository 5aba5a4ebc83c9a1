"""Hand-made windows around the WIDER rule by which the build kernel settles a window (build_lds_impl.h, "settled windows"; DESIGN.md
section 2): the reference chain may stand beside components that hold no reference k-mer of coverage >= cov_threshold -- such a component
has no source, sets no flag and emits nothing.  Every case states its outcome under the rule, and every case is held against the oracle
with the rule on, with LANCET_SETTLE_CHAIN_ONLY=1 (the rule before it: the chain is the whole graph) and with LANCET_NO_SETTLE=1.  Shared
by test_settle_components_emu.py (host builds of the kernels) and test_settle_components_gpu.py (the device).

Windows of 240 bases, reads of 100 bases, k = 21 (min_k == max_k), the helpers of settle_cases.py.  A junk COMPONENT is one random read
given six times (three tumour, three normal: its k-mers survive the first removeLowCov with coverage 6, at no reference offset)."""
from __future__ import annotations

import functools
import re

import numpy as np

import settle_cases as sc
from lancet_amd import abi
from oracle import oracle
from settle_cases import K, REFLEN, SCase, _junk, _plain_ref, _snv
from table_order_cases import _rand, batch_of, kmers, pack_reads, perfect_reads

JUNK_SEEDS = (0, 1, 2, 3, 4, 5)        # the junk-component case, once per seed: the component numbered before the chain in some, after it in others


class CCase(SCase):
    def __init__(self, name, ref, reads, settled, chain_only=False, ncomp=None, **kw):
        super().__init__(name, ref, reads, settled, **kw)
        self.chain_only = chain_only         # settled under LANCET_SETTLE_CHAIN_ONLY=1 too
        self.ncomp = ncomp                   # components of the oracle's first graph (asserted on its trace where not None)


def _free_of(ref, seq):
    """no canonical k-mer of seq is one of ref's, and seq repeats none of its own"""
    return not (kmers(ref, K) & kmers(seq, K)) and len(kmers(seq, K)) == len(seq) - K + 1


def _junk_read(rng, ref, n=100):
    for _ in range(100):
        s = _rand(rng, n)
        if _free_of(ref, s):
            return s
    raise AssertionError("no junk read free of the reference")


def _junk_component_case(seed):
    rng = np.random.default_rng(1000 + seed)
    ref = _plain_ref(rng)
    below, comp = _junk(rng), [_junk_read(rng, ref)] * 6
    # (the table's iteration order follows the order of insertion: the component's reads behind the reference's on even seeds, in front of them on odd ones)
    reads = below + perfect_reads(ref, K) + comp if seed % 2 == 0 else comp + below + perfect_reads(ref, K)
    return CCase("junk_component_s%d" % seed, ref, pack_reads(reads), True, ncomp=2, records=0)


def _low_cov_side(ref):
    """reads over ref[130:] that see each of its k-mers two to four times"""
    return [ref[130:230], ref[140:240]] * 2


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(43)
    out = [_junk_component_case(s) for s in JUNK_SEEDS]
    # a second component of reference k-mers below cov_threshold: no read over the middle, the right side seen two to four times
    ref = _plain_ref(rng)
    out.append(CCase("low_cov_reference_component", ref, pack_reads(perfect_reads(ref[:110], K) + _low_cov_side(ref)), True, ncomp=2, records=0))
    # ... and the same shape with both sides at full coverage (settle_cases.g_two_chains): both components have a source
    ref = _plain_ref(rng)
    out.append(CCase("two_full_chains", ref, pack_reads(perfect_reads(ref[:110], K) + perfect_reads(ref[130:], K)), False, ncomp=2))
    # a junk component with a cycle: a tandem repeat of a 30-base unit, longer than k
    ref = _plain_ref(rng)
    for _ in range(100):
        unit = _rand(rng, 30)
        loop = _rand(rng, 20) + unit + unit + _rand(rng, 20)
        if not (kmers(ref, K) & kmers(loop, K)) and len(kmers(unit + unit[:K - 1], K)) == 30:
            break
    out.append(CCase("junk_component_with_cycle", ref, pack_reads(perfect_reads(ref, K) + [loop] * 6), True, ncomp=2, records=0))
    # a junk read that starts with a reference k-mer: its first step links the chain's node to a junk node, the component touches the chain
    ref = _plain_ref(rng)
    for _ in range(100):
        tail = _rand(rng, 100 - K)
        touch = ref[90:90 + K] + tail
        if tail[0] != ref[90 + K] and len(kmers(ref, K) | kmers(touch, K)) == REFLEN - K + 1 + 100 - K:
            break
    out.append(CCase("junk_read_touches_chain", ref, pack_reads(perfect_reads(ref, K) + [touch] * 6), False, ncomp=1))
    # a heterozygous SNV beside a junk component
    ref = _plain_ref(rng)
    out.append(CCase("snv_beside_junk_component", ref, pack_reads(perfect_reads(ref, K) + perfect_reads(_snv(ref, 120), K) + [_junk_read(rng, ref)] * 6), False, ncomp=2, records=1))
    # a junk component one of whose k-mers is the reference's at offset 180, outside the run (reads over ref[:110] only), with coverage 6: rule (2') fails
    ref = _plain_ref(rng)
    for _ in range(100):
        hit = _rand(rng, 40) + ref[180:180 + K] + _rand(rng, 100 - 40 - K)
        if len(kmers(ref, K) | kmers(hit, K)) == REFLEN - K + 1 + 100 - K:
            break
    out.append(CCase("junk_kmer_is_reference_kmer", ref, pack_reads(perfect_reads(ref[:110], K) + [hit] * 6), False, ncomp=2))
    # no node reaches cov_threshold on a graph that branches: settle_cases.f_no_source's tiling, the two normal reads over base 120 carrying an
    # SNV allele (seen twice, like the reference allele: both survive).  No component has a source.
    ref = _plain_ref(rng)
    tile = [ref[a:a + 100] for a in range(0, REFLEN - 100 + 1, 50)] + [ref[-100:]]
    reads = tile + tile[:-1]
    alt = _snv(ref, 120)[50:150]
    assert reads[1] == ref[50:150] and reads[5] == ref[50:150]
    reads[1] = reads[5] = alt
    out.append(CCase("no_source_on_a_branching_graph", ref, pack_reads(reads), True, ncomp=1, records=0))
    return out


@functools.lru_cache(maxsize=None)
def batch():
    return batch_of(cases())


PARAMS = dict(min_k=K, max_k=K)
R_CASES = 8          # the -R run: the junk-component seeds, the low-coverage side and the two full chains (every base at quality 'I': recovery has nothing to lend, the reference's outcome is that without -R)


@functools.lru_cache(maxsize=None)
def oracle_out():
    """(records, stats, -v trace) of the cases"""
    return oracle.run(batch(), abi.default_params(**PARAMS), verbose=True)


def trace_blocks(trace, b):
    """the -v trace by window: {window index: text}"""
    by_name = {}
    for blk in trace.split("== Processing ")[1:]:
        by_name[re.match(r"\d+: (\S+) ", blk).group(1)] = blk
    return {w: by_name[b.hdr[w]] for w in range(b.n_windows) if b.hdr[w] in by_name}


def chain_component_ids():
    """per junk-component case: the number markConnectedComponents gave the chain's component (the one id on its `refcompids:` line)"""
    blocks = trace_blocks(oracle_out()[2], batch())
    out = {}
    for w, c in enumerate(cases()):
        if c.name.startswith("junk_component_s"):
            m = re.search(r"comp: 2 refcomp: 1 refcompids:\s+(\d+)\s*$", blocks[w], re.M)
            assert m, (c.name, "not two components of which one holds the reference's k-mers")
            out[c.name] = int(m.group(1))
    return out


def assert_oracle_side():
    """what the cases state about the reference's own outcome, before a value of the kernels is looked at"""
    cs = cases()
    ov, ost, tr = oracle_out()
    blocks = trace_blocks(tr, batch())
    for w, c in enumerate(cs):
        n = sum(1 for v in ov if v["window"] == w)
        if c.settled:
            assert ost[w]["status"] == 0 and ost[w]["n_builds"] == 1 and n == 0, (c.name, ost[w], n)
        if c.records == 0:
            assert n == 0, (c.name, n)
        if c.records == 1:
            assert n >= 1, (c.name, "no record")
        if c.ncomp is not None:
            m = re.search(r"^ nodes: \d+ refnodes: \d+ comp: (\d+) ", blocks[w], re.M)
            assert m and int(m.group(1)) == c.ncomp, (c.name, m and m.group(1))
    ids = chain_component_ids()
    assert 1 in ids.values() and 2 in ids.values(), ids                # the junk component numbered after the chain, and before it
    w = next(i for i, c in enumerate(cs) if c.name == "junk_component_with_cycle")
    assert "No match to reference for source" in blocks[w] and ost[w]["n_builds"] == 1      # a cycle in a component without a source makes nobody climb


def assert_results(routes, what="", keys=sc.KEYS, n=None):
    """routes: {"rule" | "chain_only" | "off": (records, stats, settled windows)} of the first n cases; every route equal to the oracle, the settled sets as the cases state"""
    cs = cases()[:n]
    ov, ost, _ = oracle_out()
    ov, ost = [v for v in ov if v["window"] < len(cs)], ost[:len(cs)]
    for tag, (v, st, settled) in routes.items():
        bad = [(cs[w].name, [a[k] for k in keys], [b[k] for k in keys]) for w, (a, b) in enumerate(zip(st, ost)) if any(a[k] != b[k] for k in keys)]
        assert not bad and len(st) == len(ost), (what, tag, bad[:4])
        assert v == ov, (what, tag, "records")
        want = {"rule": [w for w, c in enumerate(cs) if c.settled], "chain_only": [w for w, c in enumerate(cs) if c.chain_only], "off": []}[tag]
        assert sorted(settled) == want, (what, tag, [cs[w].name for w in set(settled) ^ set(want)])


# ---------------------------------------------------------------- the scan batch: the class the rule is for, counted on the oracle's trace

C_EXPECTED = 129           # windows of settle_cases.scan_batch() in source_chain_class (below)


def source_chain_class(trace, records, b):
    """The windows of the oracle's -v trace with
      one build, no record,
      every component of the first graph a tree: sum over the components of (edges // 2 + 1) == the `nodes:` of the `connected components`
        line, each component's edges from ITS first stats line after it (printStats(c) before markRefEnds(c): a link counts at both ends),
      exactly one `ref trim5` line (one component has a source),
      and at most 4 edges after the first compress of the component that has the source (a plain chain compresses to <= 3 nodes in a row)."""
    have_rec = {v["window"] for v in records}
    out = []
    for w, blk in sorted(trace_blocks(trace, b).items()):
        if w in have_rec or len(re.findall(r"^reads: \d+ reflen: \d+ ", blk, re.M)) != 1:
            continue
        if len(re.findall(r"^ref trim5: ", blk, re.M)) != 1:
            continue
        lines = blk.split("\n")
        try:
            i0 = next(j for j, ln in enumerate(lines) if ln.startswith("connected components"))
        except StopIteration:
            continue
        mc = re.match(r" nodes: (\d+) refnodes: \d+ comp: (\d+) ", lines[i0 + 1])
        if not mc:
            continue
        nodes, ncomp = int(mc.group(1)), int(mc.group(2))
        first, src_comp, after = {}, None, None
        cur = None
        for ln in lines[i0 + 2:]:
            m = re.match(r"\s*(\d+): nodes: (\d+) edges: (\d+) ", ln)
            if m:
                c = int(m.group(1))
                if c not in first:
                    first[c] = (int(m.group(2)), int(m.group(3)))
                    cur = c
                elif c == src_comp and after is None:
                    after = int(m.group(3))
            elif ln.startswith("ref trim5: "):
                src_comp = cur
        if len(first) != ncomp or 0 in first or src_comp is None or after is None:
            continue
        if sum(e // 2 + 1 for _, e in first.values()) != nodes:      # (whole halves: a lone node linked to itself counts its one edge once)
            continue
        if after > 4:
            continue
        out.append(w)
    return out
