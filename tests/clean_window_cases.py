"""Hand-made windows that take the three per-component cleaning passes (kernels.h remove_low_cov_wg, remove_tips_wg, remove_short_links_wg) to
their edges inside whole windows: 240 bases, k = 21 (min_k == max_k), reads cut by hand.  Every case states what the oracle's -v trace has to
show for it to be its case (trace_facts); assert_preconditions holds that before anything else is looked at.  Shared by
test_clean_passes_windows_emu.py (both host builds of the kernels) and test_clean_passes_gpu.py (the device).

The rules themselves, at every threshold, are held on hand-made graphs by test_clean_passes_emu.py; these windows put the same edges behind the
build kernels, the hand-off and the device's arithmetic."""
from __future__ import annotations

import functools
import re

import numpy as np

from lancet_amd import abi, frontend, synth, workload
from oracle import oracle
from table_order_cases import FWD, NML, REV, TMR, _rand, kmers, perfect_reads

K = 21
REFLEN = 240
TIP = 11                                                       # max_tip_len of the tip windows
N_GROUPS = 8                                                   # parameter sets of cases() (stated, so that collecting a test file builds no window)


class WCase:
    def __init__(self, name, ref, reads, params, expect):
        self.name, self.ref, self.reads, self.params = name, ref, reads, params
        self.expect = expect                                   # what trace_facts of the oracle's trace must hold: dict of key -> value
        self.k = K


def _plain_ref(rng, n=REFLEN):
    for _ in range(200):
        ref = _rand(rng, n)
        if len(kmers(ref, K)) == n - K + 1:
            return ref
    raise AssertionError("no reference without a repeated canonical k-mer")


def _pack(seqs):
    """seqs: strings (samples and strands alternate), (string, sample) or (string, sample, strand)"""
    out = []
    for i, s in enumerate(seqs):
        s, lab, strand = (s + (None,))[:3] if isinstance(s, tuple) else (s, TMR if i % 2 == 0 else NML, None)
        out.append((f"r{i:05d}", s, "I" * len(s), lab, strand if strand is not None else FWD if (i // 2) % 2 == 0 else REV, 1, True))
    return out


def _snv(ref, at):
    return ref[:at] + {"A": "C", "C": "G", "G": "T", "T": "A"}[ref[at]] + ref[at + 1:]


def _fresh(rng, ref, seqs, n):
    """n random bases that add no k-mer twice: the branch is a simple path"""
    for _ in range(200):
        t = _rand(rng, n)
        if all(len(kmers(s + t, K)) == len(s + t) - K + 1 and not (kmers(s[-(K - 1):] + t, K) & kmers(ref, K)) for s in seqs):
            return t
    raise AssertionError("no fresh tail")


def _almost_repeat(ref, k, max_mismatch=2):
    """util.cc isAlmostRepeat, as the oracle states it: a reference it holds for a near-perfect repeat at k is not assembled at k"""
    return bool(oracle.lib().lancet_oracle_is_almost_repeat(ref.encode(), k, max_mismatch))


def _drawn(make, seed0):
    """the first draw (generator seeds seed0, seed0 + 1, ..) whose window shows on the oracle's trace what the case states: the outcome
    hangs on the hash order of its k-mers or on float rounding, which no cut of the reads decides"""
    for seed in range(seed0, seed0 + 400):
        c = make(np.random.default_rng(seed))
        _, stats, trace = oracle.run(batch_of([c]), abi.default_params(**c.params), verbose=True)
        f = trace_facts(trace)
        if stats[0]["status"] == 0 and stats[0]["n_builds"] == 1 and all(f[key] == want for key, want in c.expect.items()):
            return c
    raise AssertionError("no draw shows what the case states")


def trace_facts(trace_of_window):
    """what the cleaning passes print in one window's -v trace"""
    t = trace_of_window
    m = re.search(r"reads: (\d+) reflen: (\d+) readlen: (\d+)", t)
    found = [int(x) for x in re.findall(r"removing low coverage: found (\d+)", t)]
    tips = [(int(r), int(n)) for r, n in re.findall(r"remove tips round: (\d+) removed: (\d+)", t)]
    links = [int(x) for x in re.findall(r"removed links: (\d+)", t)]
    nodes = [int(x) for x in re.findall(r"^  1: nodes: (\d+)", t, re.M)]
    return dict(totalreadbp=int(m.group(3)) if m else None, reflen=int(m.group(2)) if m else None, first_found=found[0] if found else None,
                component_found=found[1] if len(found) > 1 else None, tips=[n for _, n in tips], rounds=max([r for r, _ in tips], default=0),
                links=links[0] if links else None, nodes=nodes)


def split_trace(trace):
    parts = re.split(r"(?m)^(?=== Processing )", trace)
    return [p for p in parts if p.startswith("== Processing ")]


# ---------------------------------------------------------------- the windows

def _tip_window(rng, name, tail_len, removed):
    ref = _plain_ref(rng)
    stem = ref[60:120]
    tip = stem + _fresh(rng, ref, [stem], tail_len)              # tail_len k-mers that no other read holds: strlen - K + 1 == tail_len
    return WCase(name, ref, _pack(perfect_reads(ref, K) + [tip] * 4), dict(min_k=K, max_k=K, max_tip_len=TIP),
                 dict(tips=[1, 0] if removed else [0], component_found=0))


def _y_window(rng, name):
    """a stem of 4 k-mers on the reference with two ends of 3 and 5: which of the table orders it gets shows in the trace ([3, 0] or [2, 1, 0])"""
    ref = _plain_ref(rng)
    base = ref[60:120]
    s = _fresh(rng, ref, [base], 4)
    e1 = _fresh(rng, ref, [base + s], 3)
    e2 = _fresh(rng, ref, [base + s], 5)
    return WCase(name, ref, _pack(perfect_reads(ref, K) + [base + s + e1] * 4 + [base + s + e2] * 4), dict(min_k=K, max_k=K, max_tip_len=TIP), dict(component_found=0))


def _tree_window(rng, name, tips):
    """a stem with two branches of two ends each, every piece 2 k-mers long: leaves, branches, stem -- up to three rounds that remove"""
    ref = _plain_ref(rng)
    base = ref[60:120]
    s1 = _fresh(rng, ref, [base], 2)
    s2, s3 = _fresh(rng, ref, [base + s1], 2), _fresh(rng, ref, [base + s1], 2)
    ends = [_fresh(rng, ref, [base + s1 + p], 2) for p in (s2, s2, s3, s3)]
    seqs = [base + s1 + p + e for p, e in zip((s2, s2, s3, s3), ends)]
    return WCase(name, ref, _pack(perfect_reads(ref, K) + [x for q in seqs for x in [q] * 4]), dict(min_k=K, max_k=K, max_tip_len=TIP),
                 dict(component_found=0, **(dict(tips=tips) if tips else {})))


def _ratio_window(rng, name, ratio, avgcov, short_by):
    """avgcov exact (totalreadbp = avgcov * 240, less short_by bases) and an SNV branch seen by two reads: mincovqv 2 against ratio * avgcov == 2.0"""
    ref = _plain_ref(rng)
    alt = _snv(ref, 120)
    total = avgcov * REFLEN - short_by
    seqs = [(alt[70:170], TMR)] * 2                                        # (both tumour: one of each sample would be a (1, 1) node)
    left = total - 200
    full, rem = divmod(left, 100)
    if 0 < rem < K + 1:                                                      # (no read shorter than a k-mer and a base)
        full -= 1; rem += 100
    starts = [(i * 7) % (REFLEN - 100 + 1) for i in range(full)]
    seqs += [ref[a:a + 100] for a in starts]
    if rem:
        seqs.append(ref[:rem] if rem <= REFLEN else ref)
    assert sum(len(s[0] if isinstance(s, tuple) else s) for s in seqs) == total
    gone = short_by == 0
    # the branch's 21 k-mers go in the first removeLowCov (with whatever else is at or below the cut) or stay
    return WCase(name, ref, _pack(seqs), dict(min_k=K, max_k=K, min_cov_ratio=ratio, low_cov_threshold=1), dict(totalreadbp=total, reflen=REFLEN, branch_gone=gone))


def _one_one_window(rng, name, off_by_one, found):
    """an SNV branch of 21 k-mers whose tumour reads cover its left end and whose normal reads its right end: both sums are 21 (22 for the
    neighbour), no k-mer is (1, 1) on its own, every k-mer survives the first pass (low_cov_threshold 0, a ratio term far below 1).  The
    unitig's cov[] are compressNode's pairwise float averages per strand; found: whether their sums come out as exactly (1.0f, 1.0f)"""
    ref = _plain_ref(rng)
    x = 120
    alt = _snv(ref, x)
    # alt k-mer j starts at x - K + 1 + j.  A read alt[a:e] holds the alt k-mers with a <= start and start + K <= e
    first = x - K + 1
    tumour = [alt[first - 40:first + K + 10], alt[first - 40:first + K + 9]]                      # k-mers 0..10 and 0..9: 21, and the link 9 -> 10
    normal = [alt[first + 10:first + 20 + K + 40], alt[first + 10:first + 19 + K]]               # k-mers 10..20 and 10..19: 21 -- k-mer 10 is (1, 2), k-mer 20 (0, 1)
    if off_by_one:
        normal[1] = alt[first + 10:first + 20 + K]                                               # 10..20 twice: 22
    seqs = [(s, TMR, FWD) for s in tumour] + [(s, NML, REV) for s in normal]                     # (one strand per sample: one float average each)
    both = perfect_reads(ref, K)
    seqs += [(s, TMR if i % 2 == 0 else NML) for i, s in enumerate(both + both)]
    return WCase(name, ref, _pack(seqs), dict(min_k=K, max_k=K, low_cov_threshold=0, min_cov_ratio=0.0001),
                 dict(first_found=0, component_found=found))


def _link_window(rng, name, avgcov, short_by, links, in_str=False, d=5, k=K, **settings):
    """two SNVs d (five) bases apart on different haplotypes: the d reference k-mers over the first but not the second are a node of their own
    with three edges (getSize() d against floor(k / 2)), seen by the reference's reads and the second haplotype's -- sqrt(avgcov) of them.  avgcov is exact:
    totalreadbp = avgcov * 240, less short_by bases.  in_str: an (AC)n run under position K - 1 of that node's string"""
    x, root = 120, int(round(avgcov ** 0.5))
    assert root * root == avgcov
    for _ in range(200):
        ref = _rand(rng, REFLEN)
        if in_str:
            ref = ref[:x - 12] + "AC" * 8 + ref[x + 4:]
        hap_a, hap_b = _snv(ref, x), _snv(ref, x + d)
        if (len(kmers(ref, k)) == REFLEN - k + 1 and len(kmers(ref, k) | kmers(hap_a, k) | kmers(hap_b, k)) == REFLEN - k + 1 + 2 * k
                and not _almost_repeat(ref, k)):                              # (at k = 11 | 12 four in ten random references are near-repeats: the window would never be built)
            break
    else:
        raise AssertionError("no reference")
    mid = lambda g: g[70:170]
    seqs = [(mid(hap_a), TMR)] * 4 + [(mid(hap_b), TMR)] * 2 + [(mid(ref), NML)] * (root - 2)
    left = avgcov * REFLEN - short_by - 100 * len(seqs)
    n, rem = divmod(left, 100)
    assert n >= 12 and (rem == 0 or rem > k), (n, rem)
    seqs += [ref[:100] if i % 2 == 0 else ref[140:] for i in range(n)]               # (neither holds a k-mer over x or x + d)
    if rem:
        seqs.append(ref[:rem])
    return WCase(name, ref, _pack(seqs), dict(min_k=k, max_k=k, **settings), dict(totalreadbp=avgcov * REFLEN - short_by, reflen=REFLEN, links=links, component_found=0))


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(2768)
    out = [_tip_window(rng, "tip_of_max_tip_len_minus_1", TIP - 1, True), _tip_window(rng, "tip_of_max_tip_len", TIP, False)]
    out += [_y_window(rng, "y_%d" % i) for i in range(6)]
    # (which table order a window gets is the hash of its k-mers: drawn until the trace shows parents before children)
    out += [_drawn(lambda r: _tree_window(r, "tree_parents_first_a", [4, 2, 1, 0]), 9000), _drawn(lambda r: _tree_window(r, "tree_parents_first_b", [4, 2, 1, 0]), 9020),
            _tree_window(rng, "tree_any_order", None)]
    out += [_ratio_window(rng, "ratio_001_at_200", 0.01, 200, 0), _ratio_window(rng, "ratio_001_below_200", 0.01, 200, 1),
            _ratio_window(rng, "ratio_002_at_100", 0.02, 100, 0), _ratio_window(rng, "ratio_002_below_100", 0.02, 100, 1)]
    # the same cut of the reads on two references: the float sums of the averaged strand coverages come out as 1.0f on one and a step off on the other
    out += [_drawn(lambda r: _one_one_window(r, "one_one_by_average", False, 1), 7000), _drawn(lambda r: _one_one_window(r, "one_one_a_float_step_off", False, 0), 7000),
            _one_one_window(rng, "one_one_neighbour_22", True, 0)]
    # avgcov 16 | 25 on the square and one base below: the link's mincov is 4 | 5
    out += [_link_window(rng, "link_sqrt_at_16", 16, 0, 1), _link_window(rng, "link_sqrt_below_16", 16, 1, 0),
            _link_window(rng, "link_sqrt_at_25", 25, 0, 1), _link_window(rng, "link_sqrt_below_25", 25, 1, 0)]
    # the link of avgcov 16 in an STR (kept), and with the STR no longer reported (removed)
    in_str = _drawn(lambda r: _link_window(r, "link_in_str", 16, 0, 0, in_str=True), 830)
    out += [in_str, WCase("link_in_str_not_reported", in_str.ref, in_str.reads, dict(in_str.params, dist_from_str=0, min_report_len=40), dict(in_str.expect, links=1))]
    # getSize() at floor(k / 2) - 1 | floor(k / 2): k = 21, and min_k = max_k = 11 and 12 (floor(11 / 2) = 5 but (11 + 1) / 2 = 6; an even k goes through the general build)
    out += [_link_window(rng, "link_of_9_kmers", 16, 0, 1, d=9), _link_window(rng, "link_of_10_kmers", 16, 0, 0, d=10)]
    out += [_link_window(rng, "link_of_4_kmers_k11", 16, 0, 1, d=4, k=11), _link_window(rng, "link_of_5_kmers_k11", 16, 0, 0, d=5, k=11),
            _link_window(rng, "link_of_5_kmers_k12", 16, 0, 1, d=5, k=12), _link_window(rng, "link_of_6_kmers_k12", 16, 0, 0, d=6, k=12)]
    return out


def batch_of(cs):
    wins, reads = [], []
    for w, c in enumerate(cs):
        start = 1000 + 3000 * w
        wins.append(frontend.Window(f"chr22:{start}-{start + len(c.ref)}", "chr22", start, start + len(c.ref), c.ref))
        reads.append(c.reads)
    return frontend.build_batch(wins, reads)


@functools.lru_cache(maxsize=None)
def groups():
    """the cases by parameter set: [(params dict, [WCase], batch)]"""
    by = {}
    for c in cases():
        by.setdefault(tuple(sorted(c.params.items())), []).append(c)
    assert len(by) == N_GROUPS
    return [(dict(key), cs, batch_of(cs)) for key, cs in by.items()]


@functools.lru_cache(maxsize=None)
def oracle_of(gi):
    params, _, batch = groups()[gi]
    return oracle.run(batch, abi.default_params(**params), verbose=True)


def assert_preconditions(gi):
    """what makes every window of the group its case, on the oracle's -v trace alone"""
    _, cs, _ = groups()[gi]
    _, stats, trace = oracle_of(gi)
    parts = split_trace(trace)
    assert len(parts) == len(cs)
    facts = [trace_facts(p) for p in parts]
    for c, f, s in zip(cs, facts, stats):
        assert s["status"] == 0 and s["n_builds"] == 1, (c.name, s)
        for key, want in c.expect.items():
            if key == "branch_gone":
                # the component after the first pass: the reference's k-mers alone (at most 220), or the branch's 21 beside them
                assert (f["nodes"][0] <= REFLEN - K + 1) == want and (f["first_found"] >= K) == want, (c.name, f)
            else:
                assert f[key] == want, (c.name, key, f)
    return facts


def assert_group_wide(all_facts):
    """what the windows show between them, at least once each"""
    ys = [f["tips"] for c, f in all_facts if c.name.startswith("y_")]
    assert [3, 0] in ys and [2, 1, 0] in ys, ys                                  # both table orders of the Y
    trees = [f["tips"] for c, f in all_facts if c.name.startswith("tree_")]
    assert any(len(t) >= 4 and t[2] > 0 for t in trees), trees                   # a third round that removes
    assert any(f["component_found"] for _, f in all_facts)                       # the per-component removeLowCov finds a node
    by = {c.name: (c, f) for c, f in all_facts}
    assert by["link_in_str"][0].ref == by["link_in_str_not_reported"][0].ref and by["link_in_str"][1]["links"] == 0 and by["link_in_str_not_reported"][1]["links"] == 1      # kept only for its STR
    assert by["link_sqrt_at_16"][1]["links"] == 1 and by["link_sqrt_below_16"][1]["links"] == 0                                     # decided by a perfect-square avgcov
    assert by["ratio_001_at_200"][1]["first_found"] >= K > by["ratio_001_below_200"][1]["first_found"]                              # decided by the ratio term


# ---------------------------------------------------------------- one batch with a raised error rate

@functools.lru_cache(maxsize=None)
def noisy_batch():
    """(batch, the oracle's result): four synthetic windows of 300 bases at 60x / 60x with 12 % errors -- graphs of hundreds of unitigs when the
    passes run: pass_candidates_wg and clean_dead_flags_wg over tables of several lanes' worth, past 64 and past 512"""
    d = synth.make_tumor_normal(ref_len=3000, cov_t=60, cov_n=60, ref_seed=61, tumor_seed=161, normal_seed=261, error_rate=0.12, read_len=100,
                                insert_mean=300.0, insert_sd=30.0, somatic_every=400, germline_every=300)
    wins = frontend.tile_region(d["ref"], d["rname"], "chr22:400-2400", window_size=300)
    b, _ = frontend.batch_from_sam(wins, synth.pairs_to_sorted_reads(d["tumor"]), synth.pairs_to_sorted_reads(d["normal"]))
    b = workload.sub_batch(b, 0, 4)
    return b, oracle.run(b, abi.default_params(), verbose=True)


def assert_noisy_preconditions():
    """read off the oracle's statistics lines: the live nodes of a component after its first compress, which is what the passes walk"""
    _, (_, stats, trace) = noisy_batch()
    assert all(s["status"] == 0 for s in stats)
    live = [int(n) for p in split_trace(trace) for n in re.findall(r"compressing graph:  removing \d+ dead nodes\n  1: nodes: (\d+)[^\n]*\n\nremoving low coverage", p)]
    assert max(live) > 512 and sum(n > 64 for n in live) >= 2, live
    return live
