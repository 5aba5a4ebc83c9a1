"""Hand-made graphs for the three per-component cleaning passes (test_clean_passes_emu.py): each case states its outcome -- what every pass,
run alone from the start state, reports and which nodes it leaves dead -- and the settings it runs under.

The graphs stand on ANCHORS: long, well covered nodes with an edge to themselves.  compressNode never merges a node that has such an edge
(nor into one), no pass removes it, so whatever hangs between anchors is decided by the pass under test alone and the dead set of a case is
exactly the set of nodes its predicate took -- except where a case wants the compress that follows to have work, and says so."""
import numpy as np

from emu_graph import DEAD, FF, FR, NIL, NORMAL, SINK, SOURCE, TUMOR, Graph

CODE = {"A": 0, "C": 1, "G": 2, "T": 3}

# Lancet.hh's defaults, and an average coverage of 30 (floor(sqrt) = 5, ratio term 0.3) under which a node of the default coverages
# (minima 50) is no candidate of any pass unless it is a short tip
DEFAULTS = dict(totalreadbp=3000, reflen=100, low_cov_threshold=1, max_tip_len=11, max_unit_len=4, min_report_units=3, min_report_len=7,
                dist_from_str=1, path_cap=4096, comp=1, min_cov_ratio=0.01, precompress=0)


class CleanGraph(Graph):
    """nodes over k-mers that left the table, with stated minima, coverages and (where it matters) bases"""

    def __init__(self, K=11, seed=1, **settings):
        super().__init__(seed, K)
        self.settings = dict(DEFAULTS, **settings)
        assert set(self.settings) == set(DEFAULTS)
        self.stated_str = {}                # node -> the case's statement: findTandems reports an STR over position K-1 of its string
        self.expect = dict(lowcov=(0, set()), tips=([0], set()), links=(0, set()))      # pass alone: counts reported, nodes dead afterwards
        self.expect_seq = None              # the three in order: (found, [tips per round], links), where the case states it
        self.expect_overflow = set()        # passes (alone) that end with the overflow flag
        self.untouched = set()              # passes (alone) that leave the graph exactly as it was
        self.len_max = None

    def node(self, nk=12, mincov=50, mincovqv=50, cov=(9.0, 8.0, 7.0, 6.0), flags=TUMOR | NORMAL, comp=1, bases=None, table=True):
        """a node of nk k-mers (nk + K - 1 bases); its k-mers' counts are at least the stated minima and reach them at one k-mer"""
        K = self.K
        weak, weakq = int(self.rng.randint(nk)), int(self.rng.randint(nk))
        ks = []
        for j in range(nk):
            mc = mincov + (0 if j == weak else int(self.rng.randint(0, 4)))
            mq = mincovqv + (0 if j == weakq else int(self.rng.randint(0, 4)))
            row = len(self.qv)
            q = np.zeros((K, 4), np.int64); q[:, j % 4] = mq
            self.qv.append(q)
            kc = [0, 0, 0, 0]; kc[(j + 1) % 4] = mc
            ks.append(self._record(DEAD | (flags & 3), comp, kc=tuple(kc), nqv=row, nkm=1, nkmT=1 if flags & 3 == TUMOR else 0))
        length = nk + K - 1
        codes = [CODE[b] for b in bases] if bases is not None else [int(x) for x in self.rng.randint(0, 4, length)]
        assert len(codes) == length, (len(codes), length)
        desc = [ks[0] << 9 | i << 2 | codes[i] for i in range(K)] + [k << 9 | (K - 1) << 2 | codes[K + j] for j, k in enumerate(ks[1:])]
        lo = len(self.seq)
        self.seq += desc
        n = self._record(flags, comp, tuple(float(np.float32(x)) for x in cov), nqv=NIL, nkm=nk, nkmT=nk if flags & 3 == TUMOR else 0, lo=lo, hi=lo + length, clo=lo, chi=lo + length)
        if table:
            self.order.append(n)
        return n

    def anchor(self, comp=1):
        h = self.node(nk=25, mincov=60, mincovqv=60, comp=comp)
        self.link(h, h, FF)
        return h

    def between(self, n, anchors):
        """n hangs on the anchors: the first link arrives at its R side, the second leaves its F side, a third arrives reversed"""
        for i, h in enumerate(anchors):
            if i == 0:
                self.link(h, n, FF)
            elif i == 1:
                self.link(n, h, FF)
            else:
                self.link(h, n, FR)
        return n

    def string(self, n):
        r = self.rec[n]
        return "".join("ACGT"[d & 3] for d in self.seq[r["lo"]:r["hi"]])


def _anchors(g, count):
    return [g.anchor() for _ in range(count)]


def _probes(g, pass_name, probes, degree=2):
    """every probe is a node between `degree` anchors of its own choice of three; probe = (node keywords, removed?)"""
    hs = _anchors(g, 3)
    removed = set()
    for i, (kw, gone) in enumerate(probes):
        if i and i % 3 == 0:
            hs = _anchors(g, 3)                                            # (an anchor holds 12 edges, two of them its own)
        n = g.between(g.node(**kw), hs[:degree])
        if gone:
            removed.add(n)
    count = len(removed)
    g.expect[pass_name] = ([count, 0] if count else [0], removed) if pass_name == "tips" else (count, removed)
    return g


CASES = {}


def case(f):
    CASES[f.__name__] = f
    return f


# ---------------------------------------------------------------------------------------------------------------------------------------
# low coverage: mincovqv <= LOW_COV_THRESHOLD || mincovqv <= MIN_COV_RATIO * avgcov || (tumour total == 1 && normal total == 1)

def _lowcov_threshold(t):
    def f():
        # avgcov 30 at a ratio of 0.0001: the ratio term is 0.003 and only takes what the threshold takes anyway
        g = CleanGraph(seed=100 + t, low_cov_threshold=t, min_cov_ratio=0.0001)
        probes = [(dict(mincovqv=t), True), (dict(mincovqv=t + 1), False)] + ([(dict(mincovqv=t - 1), True)] if t else [])
        return _probes(g, "lowcov", probes)
    f.__name__ = "lowcov_threshold_%d" % t
    return f


for _t in (0, 1, 2):
    case(_lowcov_threshold(_t))


def _lowcov_ratio(name, ratio, totalreadbp, reflen, gone, kept):
    def f():
        # LOW_COV_THRESHOLD 0: only the ratio term can take a node whose minimum is above 0
        g = CleanGraph(seed=110, low_cov_threshold=0, min_cov_ratio=ratio, totalreadbp=totalreadbp, reflen=reflen)
        assert gone <= ratio * (totalreadbp / reflen) < kept                # (the statement, in the reference's own arithmetic)
        return _probes(g, "lowcov", [(dict(mincovqv=gone), True), (dict(mincovqv=kept), False)])
    f.__name__ = "lowcov_ratio_" + name
    return f


# ratio 0.01 at avgcov exactly 100, 200, 300: the product is 1.0, 2.0, 3.0; one base of totalreadbp less and it is just below
case(_lowcov_ratio("001_at_100", 0.01, 10000, 100, 1, 2))
case(_lowcov_ratio("001_below_100", 0.01, 9999, 100, 0, 1))
case(_lowcov_ratio("001_at_200", 0.01, 20000, 100, 2, 3))
case(_lowcov_ratio("001_below_200", 0.01, 19999, 100, 1, 2))
case(_lowcov_ratio("001_at_300", 0.01, 30000, 100, 3, 4))
case(_lowcov_ratio("001_below_300", 0.01, 29999, 100, 2, 3))
case(_lowcov_ratio("001_at_200_reflen_251", 0.01, 50200, 251, 2, 3))
case(_lowcov_ratio("001_below_200_reflen_251", 0.01, 50199, 251, 1, 2))
# 200 - 2^-21: a float quotient is 200.0
case(_lowcov_ratio("001_below_200_reflen_2097152", 0.01, 200 * 2097152 - 1, 2097152, 1, 2))
case(_lowcov_ratio("002_at_100", 0.02, 10000, 100, 2, 3))
case(_lowcov_ratio("002_below_100", 0.02, 9999, 100, 1, 2))
case(_lowcov_ratio("0015_at_200", 0.015, 20000, 100, 3, 4))
case(_lowcov_ratio("0015_below_200", 0.015, 19999, 100, 2, 3))


@case
def lowcov_reads_mincovqv_not_mincov():
    g = CleanGraph(seed=120)
    return _probes(g, "lowcov", [(dict(mincovqv=1, mincov=50), True), (dict(mincovqv=50, mincov=0), False), (dict(mincovqv=1, mincov=1), True)])


@case
def lowcov_one_one_term():
    g = CleanGraph(seed=121)
    third, two_thirds = np.float32(1.0) / np.float32(3.0), np.float32(2.0) / np.float32(3.0)
    up = np.nextafter(two_thirds, np.float32(1.0))
    assert np.float32(third + two_thirds) == np.float32(1.0) and np.float32(third + up) != np.float32(1.0)
    probes = [
        (dict(cov=(1.0, 0.0, 1.0, 0.0)), True),                            # totals exactly (1.0, 1.0)
        (dict(cov=(0.0, 1.0, 0.0, 1.0)), True),
        (dict(cov=(1.0, 0.0, 2.0, 0.0)), False),                           # (1.0, 2.0)
        (dict(cov=(2.0, 0.0, 1.0, 0.0)), False),
        (dict(cov=(0.5, 0.5, 1.0, 0.0)), True),                            # (0.5 + 0.5, 1.0)
        (dict(cov=(1.0, 0.0, 0.5, 0.5)), True),
        (dict(cov=(third, two_thirds, 1.0, 0.0)), True),                   # float thirds whose sum rounds to 1.0f
        (dict(cov=(third, up, 1.0, 0.0)), False),                          # ... and one float step further, where it does not
        (dict(cov=(1.0, 0.0, third, up)), False),
        (dict(cov=(1.0, 0.0, 0.0, 0.0)), False),                           # tumour only
        (dict(cov=(1.0, 1.0, 0.0, 0.0)), False),                           # forward strand (1, 1): cov[0] + cov[2] is not the term
        (dict(cov=(1.0, 0.0, 0.0, 1.0)), True),
    ]
    return _probes(g, "lowcov", probes)


def _lowcov_after_compress(name, tumour, normal, gone, nks=None):
    def f():
        # nodes that are not (1, 1) on their own; the unitig becomes (1, 1) only through compressNode's pairwise average (the rig compresses first)
        g = CleanGraph(seed=122, precompress=1)
        h = _anchors(g, 2)
        nk = nks or [1] * len(tumour)
        f32 = np.float32
        ks = [g.node(nk=k, cov=(float(f32(t)), 0.0, 0.0, float(f32(n)))) for k, t, n in zip(nk, tumour, normal)]
        g.link(h[0], ks[0], FF).chain(ks).link(ks[-1], h[1], FF)
        cov, amer = [f32(tumour[0]), f32(normal[0])], nk[0]
        for i in range(1, len(ks)):                                        # ((nc * amer) + (bc * bmer)) / (amer + bmer), in float
            cov = [f32(f32(f32(c * f32(amer)) + f32(f32(b) * f32(nk[i]))) / f32(amer + nk[i])) for c, b in zip(cov, (tumour[i], normal[i]))]
            amer += nk[i]
        assert (cov[0] == 1 and cov[1] == 1) == gone, cov
        g.expect["lowcov"] = (1, set(ks)) if gone else (0, set(ks[1:]))    # (the head absorbs the others; then it goes or stays)
        g.expect["tips"] = ([0], set(ks[1:]))
        g.expect["links"] = (0, set(ks[1:]))
        return g
    f.__name__ = "lowcov_one_one_by_average_" + name
    return f


case(_lowcov_after_compress("two_kmers", (2, 0), (0, 2), True))
case(_lowcov_after_compress("five_kmers", (2, 0, 3, 0, 0), (0, 2, 0, 3, 0), True))
case(_lowcov_after_compress("three_kmers_off", (2, 0, 2), (0, 2, 1), False))
case(_lowcov_after_compress("thirds_round_back", (1, 0, 0, 3), (0, 0, 1, 3), True))       # 1/3 in float, times 3, rounds back to 1.0f
case(_lowcov_after_compress("sevenths", (1, 1, 1, 1, 1, 1, 1), (0, 0, 0, 0, 0, 0, 7), True))
# the neighbours one float step from 1.0f: 14 / 13 (and 13 / 11) in float, times the k-mers, does not round back to the sum -- the exact mean is 1
case(_lowcov_after_compress("one_step_above", (np.float32(14) / np.float32(13), 0), (1, 1), False, nks=[13, 1]))
case(_lowcov_after_compress("one_step_below", (np.float32(13) / np.float32(11), 0), (1, 1), False, nks=[11, 2]))
case(_lowcov_after_compress("unitigs_exact", (np.float32(1.5), 0), (1, 1), True, nks=[8, 4]))


@case
def special_nodes_and_another_component():
    """nodes that meet a pass's predicate but are special, or of component 2: every pass keeps them"""
    g = CleanGraph(seed=123)
    h = _anchors(g, 2)
    s = g.special(SOURCE); t = g.special(SINK)                              # (their minima are 0 and they have no string)
    g.link(s, h[0], FF).link(s, h[1], FR).link(h[1], t, FF)                 # the source has two edges, the sink one
    h2 = [g.anchor(comp=2), g.anchor(comp=2)]
    g.node(mincovqv=0, cov=(1.0, 0.0, 1.0, 0.0), comp=2)                    # component 2: barely covered and (1, 1),
    g.between(g.node(nk=2, comp=2), h2[:1])                                 # a tip,
    g.between(g.node(nk=3, mincov=1, comp=2), h2)                           # a short link
    low = g.between(g.node(mincovqv=0), h)
    tip = g.between(g.node(nk=2), h[:1])
    link = g.between(g.node(nk=3, mincov=1), h)
    g.expect["lowcov"] = (1, {low})
    g.expect["tips"] = ([1, 0], {tip})
    g.expect["links"] = (1, {link})
    g.expect_seq = (1, [1, 0], 1)
    return g


@case
def lowcov_removal_makes_neighbours_mergeable():
    g = CleanGraph(seed=124)
    h = _anchors(g, 3)
    p, q, c = g.node(nk=14), g.node(nk=13), g.node(mincovqv=1)
    g.link(h[0], p, FF).link(p, q, FF).link(q, h[1], FF).link(p, c, FF).link(c, h[2], FF)
    g.expect["lowcov"] = (1, {c, q})                                        # c by the predicate, q absorbed by p in the compress that follows
    return g


@case
def lowcov_nothing_removed():
    g = CleanGraph(seed=125)
    h = _anchors(g, 2)
    p, q = g.node(nk=14, mincovqv=2), g.node(nk=13, mincovqv=2)
    g.link(h[0], p, FF).link(p, h[1], FF).link(h[0], q, FR).link(q, h[1], FR)
    g.untouched = {"lowcov", "tips", "links"}
    g.expect_seq = (0, [0], 0)
    return g


# ---------------------------------------------------------------------------------------------------------------------------------------
# tips: edges <= 1 && strlen - K + 1 < MAX_TIP_LEN, round after round until a round removes nothing

def _tips_length(L):
    def f():
        g = CleanGraph(seed=200 + L, max_tip_len=L)
        h = _anchors(g, 3)
        gone = {g.between(g.node(nk=L - 1), h[:1]), g.node(nk=L - 1), g.between(g.node(nk=1), h[1:2])}          # degree 1, 0, 1
        g.between(g.node(nk=L), h[:1]); g.node(nk=L)                        # at MAX_TIP_LEN: kept at degree 1 and 0
        g.between(g.node(nk=L - 1), h[:2]); g.between(g.node(nk=1), h[:3])  # short, degree 2 and 3: kept
        g.expect["tips"] = ([3, 0], gone)
        return g
    f.__name__ = "tips_length_%d" % L
    return f


for _L in (4, 11, 19):
    case(_tips_length(_L))


def _tips_y(stem_first):
    def f():
        g = CleanGraph(seed=210)
        h = g.anchor()
        s, e1, e2 = g.node(nk=2, table=False), g.node(nk=3, table=False), g.node(nk=2, table=False)
        g.order += [s, e1, e2] if stem_first else [e1, e2, s]
        g.link(h, s, FF).link(s, e1, FF).link(s, e2, FR)
        # the ends first: the stem is down to one edge when the walk reaches it, and goes in round 1; the stem first: it waits for round 2
        g.expect["tips"] = ([2, 1, 0] if stem_first else [3, 0], {s, e1, e2})
        return g
    f.__name__ = "tips_y_stem_%s" % ("first" if stem_first else "last")
    return f


case(_tips_y(True))
case(_tips_y(False))


def _tips_tree(depth):
    def f():
        # a binary tree of short nodes on an anchor, parents before children in the table: one level goes per round, leaves first
        g = CleanGraph(seed=220 + depth)
        h = g.anchor()
        levels = [[g.node(nk=1)]]
        g.link(h, levels[0][0], FF)
        for _ in range(depth):
            nxt = []
            for p in levels[-1]:
                a, b = g.node(nk=1), g.node(nk=1)
                g.link(p, a, FF).link(p, b, FR)
                nxt += [a, b]
            levels.append(nxt)
        g.expect["tips"] = ([len(l) for l in reversed(levels)] + [0], {n for l in levels for n in l})
        return g
    f.__name__ = "tips_tree_%d_rounds" % (depth + 2)
    return f


case(_tips_tree(1))         # 2 1 0
case(_tips_tree(2))         # 4 2 1 0
case(_tips_tree(3))         # 8 4 2 1 0


@case
def tips_third_round_after_a_merge():
    """s1 carries s2 and a leaf, s2 two leaves: round 1 takes the leaves, the compress merges s2 into s1, which is a tip in round 2 only
    because the merged node is still short (3 + 4 k-mers < 11)"""
    g = CleanGraph(seed=230)
    h = g.anchor()
    s1, s2 = g.node(nk=3), g.node(nk=4)
    e = [g.node(nk=1) for _ in range(3)]
    g.link(h, s1, FF).link(s1, s2, FF).link(s1, e[0], FR).link(s2, e[1], FF).link(s2, e[2], FR)
    g.expect["tips"] = ([3, 1, 0], {s1, s2, *e})
    return g


@case
def tips_merged_stem_reaches_max_tip_len():
    g = CleanGraph(seed=231)
    h = g.anchor()
    s1, s2 = g.node(nk=5), g.node(nk=6)                                     # 11 k-mers after the merge: no tip
    e = [g.node(nk=1) for _ in range(3)]
    g.link(h, s1, FF).link(s1, s2, FF).link(s1, e[0], FR).link(s2, e[1], FF).link(s2, e[2], FR)
    g.expect["tips"] = ([3, 0], {s2, *e})
    return g


@case
def tips_removal_leaves_a_self_loop_node():
    g = CleanGraph(seed=232)
    h = g.anchor()
    x, t = g.node(nk=2), g.node(nk=2)
    g.link(h, x, FF).link(x, x, FF).link(x, t, FF)
    g.expect["tips"] = ([1, 0], {t})                                        # x keeps three edges, two of them to itself
    return g


@case
def tips_special_node_of_degree_one():
    g = CleanGraph(seed=233)
    h = g.anchor()
    s = g.special(SOURCE); t = g.special(SINK)
    g.link(s, h, FF)
    return g                                                                # nothing goes: the source has one edge, the sink none


# ---------------------------------------------------------------------------------------------------------------------------------------
# short links: edges >= 2 && getSize() < floor(K / 2) && mincov <= floor(sqrt(avgcov)) && no STR over position K - 1

def _links_length(K):
    def f():
        g = CleanGraph(K=K, seed=300 + K, max_tip_len=K)
        half = K // 2
        return _probes(g, "links", [(dict(nk=half - 1, mincov=5), True), (dict(nk=half, mincov=5), False), (dict(nk=1, mincov=5), True)])
    f.__name__ = "links_length_k%d" % K
    return f


for _K in (11, 12, 13):
    case(_links_length(_K))


def _links_sqrt(name, totalreadbp, reflen, gone, kept):
    def f():
        g = CleanGraph(seed=310, totalreadbp=totalreadbp, reflen=reflen)
        return _probes(g, "links", [(dict(nk=3, mincov=gone), True), (dict(nk=3, mincov=kept), False)])
    f.__name__ = "links_sqrt_" + name
    return f


for _sq in (3, 4, 5, 7):
    case(_links_sqrt("at_%d" % (_sq * _sq), _sq * _sq * 100, 100, _sq, _sq + 1))
    case(_links_sqrt("below_%d" % (_sq * _sq), _sq * _sq * 100 - 1, 100, _sq - 1, _sq))
case(_links_sqrt("at_25_reflen_251", 25 * 251, 251, 5, 6))
case(_links_sqrt("below_25_reflen_251", 25 * 251 - 1, 251, 4, 5))
case(_links_sqrt("below_25_reflen_2097152", 25 * 2097152 - 1, 2097152, 4, 5))      # 25 - 2^-21: a float quotient is 25.0


@case
def links_reads_mincov_not_mincovqv():
    g = CleanGraph(seed=320)
    return _probes(g, "links", [(dict(nk=3, mincov=5, mincovqv=50), True), (dict(nk=3, mincov=6, mincovqv=2), False)])


@case
def links_degree():
    g = CleanGraph(seed=321)
    h = _anchors(g, 3)
    d1 = g.between(g.node(nk=3, mincov=2), h[:1])
    d2 = g.between(g.node(nk=3, mincov=2), h[:2])
    d3 = g.between(g.node(nk=3, mincov=2), h[:3])
    g.expect["links"] = (2, {d2, d3})
    g.expect["tips"] = ([1, 0], {d1})
    return g


def _links_neighbours(first):
    def f():
        g = CleanGraph(seed=322)
        h = _anchors(g, 2)
        l = [g.node(nk=3, mincov=2, table=False), g.node(nk=4, mincov=3, table=False)]
        g.order += [l[first], l[1 - first]]
        g.link(h[0], l[0], FF).link(l[0], l[1], FF).link(l[0], l[1], FR).link(l[1], h[1], FF)      # (two links between them: nothing to merge)
        g.expect["links"] = (1, {l[first]})                                 # the other is down to one edge when the walk reaches it
        return g
    f.__name__ = "links_neighbours_%s_first" % ("left" if first == 0 else "right")
    return f


case(_links_neighbours(0))
case(_links_neighbours(1))


# strings of 14 bases (K = 11, four k-mers), position K - 1 = 10
AC_RUN = "ACACACACACGTCT"                                                  # (AC)5, over positions 0 .. 9: position 10 is its end
AC_WHOLE = "ACACACACACACAC"                                                # the whole string one stretch: findTandems reports none (its end-of-string rule wants one more character)
AAG_RUN = "AAGAAGAAGAAGAA"
NO_REPEAT = "ACGTCAGTTGCATG"
AC_ENDS_AT_9 = "ACACACACAGTCTG"                                            # (AC)4 A: the stretch ends one base left of position 10


def _links_str(name, settings, strings):
    def f():
        g = CleanGraph(seed=330, **settings)
        hs = _anchors(g, 3)
        gone = set()
        for i, (bases, in_str) in enumerate(strings):
            n = g.between(g.node(nk=4, mincov=2, bases=bases), hs[:2])
            g.stated_str[n] = in_str
            if not in_str:
                gone.add(n)
        g.expect["links"] = (len(gone), gone)
        return g
    f.__name__ = "links_str_" + name
    return f


case(_links_str("defaults", {}, [(AC_RUN, True), (AAG_RUN, True), (NO_REPEAT, False), (AC_ENDS_AT_9, True), (AC_WHOLE, False)]))
case(_links_str("dist_0", dict(dist_from_str=0), [(AC_RUN, True), (AAG_RUN, True), (NO_REPEAT, False), (AC_ENDS_AT_9, False)]))
case(_links_str("min_report_len_15", dict(min_report_len=15), [(AC_RUN, False), (AAG_RUN, False), (NO_REPEAT, False), (AC_ENDS_AT_9, False)]))
case(_links_str("max_unit_len_2", dict(max_unit_len=2), [(AC_RUN, True), (AAG_RUN, False), (NO_REPEAT, False), (AC_ENDS_AT_9, True)]))


@case
def links_string_longer_than_path_cap():
    g = CleanGraph(seed=340, path_cap=12)                                   # a candidate of 3 k-mers is 13 bases long
    _probes(g, "links", [(dict(nk=3, mincov=2), True)])
    g.expect_overflow = {"links"}
    return g


@case
def links_string_of_path_cap():
    g = CleanGraph(seed=340, path_cap=13)
    return _probes(g, "links", [(dict(nk=3, mincov=2), True)])


# ---------------------------------------------------------------------------------------------------------------------------------------
# the three in order, with work for each

@case
def sequence_every_pass_has_work():
    g = CleanGraph(seed=400)
    h = _anchors(g, 3)
    low = g.between(g.node(mincovqv=1), h[:2])
    tip = g.between(g.node(nk=4), h[:1])
    link = g.between(g.node(nk=3, mincov=4), h[1:3])
    p, q, c = g.node(nk=2), g.node(nk=2), g.node(mincovqv=0)               # c goes for its coverage, p absorbs q (4 k-mers), a short link between two anchors
    g.link(h[0], p, FF).link(p, q, FF).link(q, h[2], FF).link(p, c, FF).link(c, h[1], FF)
    g.expect["lowcov"] = (2, {low, c, q})
    g.expect["tips"] = ([1, 0], {tip})
    g.expect["links"] = (1, {link})
    g.expect_seq = (2, [1, 0], 1)
    return g


# ---------------------------------------------------------------------------------------------------------------------------------------
# group edges of the compaction: tables of M nodes without edges, the candidates short (one k-mer) and barely covered, the others two k-mers long

GROUP_SIZES = [1, 63, 64, 65, 127, 128, 129]
GROUP_SIZES_FAT = [511, 512, 513, 1025]
GROUP_PATTERNS = ["none", "first", "last", "every", "every_second"]


def group_case(M, pattern):
    g = CleanGraph(K=5, seed=500 + M, max_tip_len=2)
    pick = {"none": lambda i: False, "first": lambda i: i == 0, "last": lambda i: i == M - 1, "every": lambda i: True, "every_second": lambda i: i % 2 == 1}[pattern]
    gone = set()
    for i in range(M):
        if pick(i):
            gone.add(g.node(nk=1, mincovqv=0))
        else:
            g.node(nk=2)
    g.expect["lowcov"] = (len(gone), gone)
    g.expect["tips"] = ([len(gone), 0] if gone else [0], gone)
    g.expect_seq = (len(gone), [0], 0)
    g.len_max = 8
    return g


def group_case_linked(M):
    """the same sizes with edges: anchors in a row with a one-k-mer node between each two; every second of those is barely covered -- a short
    link -- so that remove_short_links_wg's list, its walk and the compress_wg behind it run over a table of M nodes too"""
    g = CleanGraph(K=5, seed=600 + M, max_tip_len=2)
    n = (M - 1) // 2
    def anchor():
        h = g.node(nk=3, mincov=60, mincovqv=60)
        g.link(h, h, FF)
        return h
    gone = set()
    prev = anchor()
    for i in range(n):
        l = g.node(nk=1, mincov=2 if i % 2 == 1 else 50)
        nxt = anchor()
        g.link(prev, l, FF).link(l, nxt, FF)
        if i % 2 == 1:
            gone.add(l)
        prev = nxt
    if len(g.order) < M:
        g.node(nk=3)                                                        # (an even M: one more node, on its own)
    g.expect["links"] = (len(gone), gone)
    g.expect_seq = (0, [0], len(gone))
    g.len_max = 8
    return g
