"""Hand-made windows ON the edges of the code that carries the settle rule (build_lds_impl.h, "settled windows"): the
capacity of the test's words, the groups of the edge pass, the words of the three bitmaps over the reference offsets, the 1024-lane form,
the coverage threshold met exactly, survivors at two reference offsets by their survivor index, and the gates in front of the test.
settle_cases.py and settle_component_cases.py hold the RULE at one shape (240 bases, ~220 survivors, one group, bitmap words 0..6); the
windows here have up to 1024 bases and 2049 survivors.  Shared by test_settle_edges_emu.py (both host builds of the kernels) and
test_settle_edges_gpu.py (the device).

Every case states `settled` (True / False) for the default hand-off and for LANCET_PRE_WIDE=1 (`settled_wide`, the same unless given), and
whether LANCET_SETTLE_CHAIN_ONLY=1 settles it too (`chain_only`) -- derived from the rule and the gates, which the comments beside the
cases give.  Every case asserts on the oracle's side, before a value of the kernels is looked at, what makes it its edge: one build, status
0 and no record where settled; the survivors after the first removeLowCov (`nsurv`), the distinct k-mers (`N`) and the components where
stated (assert_oracle_side).  The sizes -- survivors per group `gmax`, the capacity `cap`, PB_SCAP, the quality rows of the hand-off -- are
read off the headers through tests/settle_emu (settle_emu.limits), never typed in.

How a window gets its survivors (k = 21, min_k == max_k, unless the case says otherwise; helpers of table_order_cases.py):
  the reads that cover the reference offsets [a, b] are copies of ref[a : b + k] (tiled in reads of 100 bases where longer): the run;
  a junk COMPONENT is one random read given six times (coverage 6, at no reference offset);
  a junk read given once adds k-mers that do not survive (they count in N alone);
  the reference pseudo-read is never counted: a reference k-mer no read holds does not survive.
The survivor index of a node follows its first occurrence in the order of the reads: what stands first in the list comes first."""
from __future__ import annotations

import functools
import os
import re
import sys

import numpy as np

from lancet_amd import abi
from oracle import oracle
from settle_cases import KEYS, SCase, _plain_ref, _snv
from table_order_cases import _rand, batch_of, junk_lengths, kmers, pack_reads, perfect_reads, rc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "settle_emu"))
import settle_emu  # noqa: E402

K = 21
BLW_K, BLW_NODES, BLW_TRACKED, BLW_QV = 4, 6, 7, 9          # build_lds.h: why the build kernel turns a window away (asserted on the emulator where a case states it)


@functools.lru_cache(maxsize=None)
def limits(large=False):
    return settle_emu.limits(large)


class ECase(SCase):
    def __init__(self, name, ref, reads, settled, chain_only, nsurv, settled_wide=None, N=None, ncomp=None, big=False, why=None, why_wide=None,
                 final_k=None, params=None, records=None):
        super().__init__(name, ref, pack_reads(reads), settled, params=params or dict(min_k=K, max_k=K), records=records)
        self.settled_wide = settled if settled_wide is None else settled_wide
        self.chain_only = chain_only         # settled under LANCET_SETTLE_CHAIN_ONLY=1 (under either hand-off)
        self.nsurv, self.N, self.ncomp = nsurv, N, ncomp      # asserted on the oracle's trace where not None
        self.big = big                       # more than 512 reads: the 1024-lane form's window
        self.why, self.why_wide = why, why if why_wide is None else why_wide     # BLW_* where the build kernel does not build it (0: it does)
        self.final_k = final_k


def survivors(reads, k):
    """the k-mers that survive the first removeLowCov (Graph.cc): seen twice or more over the reads, but not once in the tumour and once in the
    normal (every base at full quality, min_cov_ratio * coverage < 2; pack_reads gives the reads to tumour and normal in turn)"""
    cnt = {}
    for j, s in enumerate(reads):
        for i in range(len(s) - k + 1 if len(s) > k else 0):
            c = s[i:i + k]
            r = rc(c)
            c = c if c < r else r
            cnt.setdefault(c, [0, 0])[j % 2] += 1
    return {c for c, (t, n) in cnt.items() if t + n >= 2 and (t, n) != (1, 1)}


def _cover(ref, a, b, k=K, copies=None):
    """reads over exactly the reference offsets [a, b]: `copies` of the stretch (one read of 100 bases has to hold it); not given: ten of them,
    or the stretch tiled where it is longer (every k-mer five times or more)"""
    seq = ref[a:b + k]
    assert copies is None or len(seq) <= 100, (a, b, copies)
    return [seq] * (copies or 10) if len(seq) <= 100 else perfect_reads(seq, k)


def _components(rng, count, k=K):
    """random reads of up to 100 bases that hold `count` k-mers between them"""
    return [_rand(rng, L) for L in junk_lengths(count, k, rl=100)] if count else []


def _more_than_512(reads, unit):
    """reads enough for the 512-lane form to turn the window away for its size (more than its BL_RMAX): the 1024-lane form's window"""
    while len(reads) <= limits(False)["rmax"]:
        reads = reads + unit
    return reads


def _counted(rng, name, nsurv, settled, reflen=600, big=False, N=None, snv=False, k=K, junk_first=True, **kw):
    """a chain over the whole reference beside junk components, nsurv survivors in all (and N distinct k-mers); the junk first in the read order
    (junk_first=False: behind the chain, so that the last survivor is a junk node).
    snv: a heterozygous SNV in the middle of the chain, whose nodes then lie behind all the junk in the survivor order"""
    for _ in range(60):
        ref = _plain_ref(rng, reflen, k)
        chain = perfect_reads(ref, k) + (perfect_reads(_snv(ref, reflen // 2), k) if snv else [])
        n_chain = reflen - k + 1 + (k if snv else 0)
        comps = _components(rng, nsurv - n_chain, k)
        once = [_rand(rng, L) for L in junk_lengths(N - nsurv, k)] if N else []
        junk, chain = [c for c in comps for _ in range(6)] + once, _more_than_512(chain, chain) if big else chain
        reads = junk + chain if junk_first else chain + junk
        have = set()
        for s in reads:
            have |= kmers(s, k)
        if len(survivors(reads, k)) != nsurv or (N and len(have) != N):
            continue
        assert (len(reads) > limits(False)["rmax"]) == big and len(reads) <= limits(True)["rmax"]
        return ECase(name, ref, reads, settled, False, nsurv, N=N, ncomp=1 + len(comps), big=big, **kw)
    raise AssertionError(name + ": no draw")


# ---------------------------------------------------------------- (a) survivor counts, 512-lane form

@functools.lru_cache(maxsize=None)
def family_counts():
    """nsurv on both sides of a group of the edge pass and of the capacity of the test's words; the chain's nodes in the second group; tables
    the build kernel would not have ordered; and, because this batch is not a deep one (narrow hand-off), the 1024-lane form's quality rows"""
    rng = np.random.default_rng(101)
    L, LL = limits(False), limits(True)
    gmax, cap = L["gmax"], L["cap"]
    assert gmax + 1 < cap - 1 and cap < L["scap"] and LL["gmax"] + 1 < LL["scap"] <= LL["cap"]
    out = [_counted(rng, "nsurv_%d" % n, n, n <= cap) for n in (gmax - 1, gmax, gmax + 1, cap - 1, cap, cap + 1)]
    # the same edge with the chain first: the last survivor, whose word st_own[nsurv - 1] is the last in front of the edge slots at nsurv = cap and
    # the first of them one further, is then a junk node
    out += [_counted(rng, "nsurv_%d_chain_first" % n, n, n <= cap, junk_first=False) for n in (cap, cap + 1)]
    # the chain behind gmax + 3 junk survivors: its nodes are in the second group.  Settled as it is; with a heterozygous SNV on it not, and the
    # record is the oracle's -- a verdict that looked at the first group alone would settle both.
    out.append(_counted(rng, "chain_in_second_group", gmax + 3 + 280, True, reflen=300))
    out.append(_counted(rng, "snv_in_second_group", gmax + 3 + 280 + K, False, reflen=300, snv=True, records=1))
    # a settled chain in a table of N distinct k-mers: the 512-lane form has no gate on N (its order would stop at 4096), up to its BL_NCAP;
    # one more and the build kernel does not build the window at all
    for n in (4096, 4097, L["ncap"]):
        out.append(_counted(rng, "N_%d" % n, 700, True, N=n))
    out.append(_counted(rng, "N_%d" % (L["ncap"] + 1), 700, False, N=L["ncap"] + 1, why=BLW_NODES))
    # the 1024-lane form under the NARROW hand-off (this batch has few reads per window): candidates * k has to fit its quality rows.  Every
    # survivor is a candidate and no other node is (a junk read given once is decided by its count).  Under LANCET_PRE_WIDE=1 both fit.
    q = L["qvcap"] // K
    assert LL["gmax"] < q < q + 1 <= LL["scap"] and (q + 1) * K <= L["qvcap_wide"]
    out.append(_counted(rng, "large_narrow_rows_%d" % q, q, True, reflen=1024, big=True, why=0))
    out.append(_counted(rng, "large_narrow_rows_%d" % (q + 1), q + 1, False, settled_wide=True, reflen=1024, big=True, why=BLW_QV, why_wide=0))
    assert sum(len(c.reads) for c in out) <= 400 * len(out)          # (not deep: host_common.h lc_pre_layout_for_sizes)
    return out


# ---------------------------------------------------------------- (b) the 1024-lane form

@functools.lru_cache(maxsize=None)
def family_large():
    """more than 512 reads per window (a deep batch: the wide hand-off, with LANCET_PRE_WIDE=1 or without): the 1024-lane form's group, its gate
    on the table size, and its upper edge -- PB_SCAP survivors.  One more and the tracked nodes exceed BL_TCAP (= PB_SCAP): not built at all."""
    rng = np.random.default_rng(102)
    LL = limits(True)
    gmax, scap = LL["gmax"], LL["scap"]
    out = [_counted(rng, "large_nsurv_%d" % n, n, True, reflen=1024, big=True) for n in (gmax - 1, gmax, gmax + 1, scap - 1, scap)]
    out.append(_counted(rng, "large_nsurv_%d" % (scap + 1), scap + 1, False, reflen=1024, big=True, why=BLW_TRACKED))
    out.append(_counted(rng, "large_chain_in_second_group", gmax + 3 + 280, True, reflen=300, big=True))
    out.append(_counted(rng, "large_snv_in_second_group", gmax + 3 + 280 + K, False, reflen=300, big=True, snv=True, records=1))
    t = LL["wide_table_from"]
    out.append(_counted(rng, "large_N_%d" % t, 1100, True, reflen=1024, big=True, N=t))
    out.append(_counted(rng, "large_N_%d" % (t + 1), 1100, False, reflen=1024, big=True, N=t + 1, why=0))      # (built, in its wide table form: not tested)
    assert sum(len(c.reads) for c in out) > 400 * len(out)
    return out


# ---------------------------------------------------------------- (c) run positions

RUNS = [(0, 31), (0, 32), (32, 63), (31, 64), (33, 95), (960, 991), (961, 1003), (992, 1003), (1, 1002), (0, 1003)]


def _touch(rng, ref, at, n, k=K):
    """a read that starts with the reference k-mer at offset `at` and leaves the reference behind it: n new k-mers, a third link on that node"""
    for _ in range(100):
        tail = _rand(rng, n)
        t = ref[at:at + k] + tail
        if tail[0] != ref[at + k] and len(kmers(ref, k) | kmers(t, k)) == len(ref) - k + 1 + n:
            return t
    raise AssertionError("no touching read")


@functools.lru_cache(maxsize=None)
def family_runs():
    """reads over exactly the offsets [a, b] of a reference of 1024 bases (1004 offsets: bits 0..11 of word 31): the run is all there is"""
    rng = np.random.default_rng(103)
    out = []
    for a, b in RUNS:
        ref = _plain_ref(rng, 1024, K)
        out.append(ECase("run_%d_%d" % (a, b), ref, _cover(ref, a, b), True, True, b - a + 1, ncomp=1, records=0))
    # one covered offset: its reads have exactly k bases, and a sequence of k bases or fewer makes no node (Graph.cc loadSequence).  No read
    # holds a k-mer, nothing survives, and a graph without survivors is not tested (nsurv > 0).
    ref = _plain_ref(rng, 1024, K)
    out.append(ECase("run_512_512", ref, _cover(ref, 512, 512), False, False, 0, records=0))
    # a run of one whole word beside a second stretch at full coverage: from 64 on it continues the run (the pseudo-read's step 63 -> 64 links
    # them: one chain [32, 100]), from 65 on offset 64 is missing and there are two chains with a source each
    ref = _plain_ref(rng, 1024, K)
    out.append(ECase("word_run_then_64", ref, _cover(ref, 32, 63) + _cover(ref, 64, 100), True, True, 69, ncomp=1, records=0))
    ref = _plain_ref(rng, 1024, K)
    out.append(ECase("word_run_then_65", ref, _cover(ref, 32, 63) + _cover(ref, 65, 100), False, False, 68, ncomp=2))
    # min Q at bit 31 and at bit 0 of a word: the run starts at 20 with offsets seen three times (they survive, below cov_threshold = 5)
    for q0 in (31, 32, 64):
        ref = _plain_ref(rng, 1024, K)
        out.append(ECase("min_q_%d" % q0, ref, _cover(ref, 20, q0 + 14, copies=3) + _cover(ref, q0, q0 + 60), True, True, q0 + 61 - 20, ncomp=1, records=0))
    # max Q in a later word than b: a second chain at full coverage further on
    ref = _plain_ref(rng, 1024, K)
    out.append(ECase("max_q_in_a_later_word", ref, _cover(ref, 0, 31) + _cover(ref, 40, 70), False, False, 63, ncomp=2))
    # ... in the LAST word that holds an offset, which is where the search for max Q starts: bits 0..11 of word 31 here, and bit 0 alone of word 3
    # on a reference of k + 96 bases (97 offsets)
    ref = _plain_ref(rng, 1024, K)
    out.append(ECase("max_q_in_the_last_word", ref, _cover(ref, 0, 31) + _cover(ref, 992, 1003), False, False, 44, ncomp=2))
    # (offsets 90..96 seen three times; five reads more start with the k-mer at 96 and run on past the reference's end: 96 alone is in Q there)
    for _ in range(100):
        ref, tail = _plain_ref(rng, K + 96, K), _rand(rng, 10)
        if len(kmers(ref + tail, K)) == 97 + 10:
            break
    out.append(ECase("max_q_at_bit_0_of_the_last_word", ref, _cover(ref, 0, 31) + _cover(ref, 90, 96, copies=3) + [ref[96:] + tail] * 5, False, False, 49, ncomp=2))
    # a run node with a third link: the run search from min Q = 0 stops AT that offset (e1), and a survivor stands there
    for at in (31, 32, 63):
        ref = _plain_ref(rng, 1024, K)
        out.append(ECase("third_link_at_%d" % at, ref, _cover(ref, 0, 79) + [_touch(rng, ref, at, 40)] * 6, False, False, 120, ncomp=1))
    # ... and below min Q: offsets 0..40 seen three times, a touching read three times on the node at `at` (coverage 6, cov_threshold 8: not in
    # Q), ten reads over every offset from 41 on.  The search down from min Q = 41 stops above `at` (a = at + 1), and a survivor stands at a - 1.
    for at in (31, 32):
        ref = _plain_ref(rng, 1024, K)
        out.append(ECase("third_link_below_min_q_at_%d" % at, ref, _cover(ref, 0, 40, copies=3) + [_touch(rng, ref, at, 30)] * 3 + _cover(ref, 41, 110), False, False, 141, ncomp=1,
                         params=dict(min_k=K, max_k=K, cov_threshold=8)))
    # ... and above max Q: ten reads over every offset of [10, e1 - 1], offsets e1 .. e1 + 40 seen three times and a touching read three times on
    # the node at e1 (coverage 6, cov_threshold 8).  Q ends with the run; what stops the run is a survivor at e1 with a third link, and no
    # later Q says so a second time.
    for e1 in (63, 64):
        ref = _plain_ref(rng, 1024, K)
        out.append(ECase("third_link_above_max_q_at_%d" % e1, ref, _cover(ref, 10, e1 - 1) + _cover(ref, e1, e1 + 40, copies=3) + [_touch(rng, ref, e1, 30)] * 3, False, False,
                         e1 - 10 + 41 + 30, ncomp=1, params=dict(min_k=K, max_k=K, cov_threshold=8)))
    return out


@functools.lru_cache(maxsize=None)
def family_runs_k11():
    """a reference of 1024 bases without a repeated 11-mer: 1014 offsets, bits 0..21 of word 31 (max_mismatch 0: with two mismatches allowed
    1024 random bases hold a near-repeat of 12 bases and k = 11 is passed over)"""
    rng = np.random.default_rng(111)
    params = dict(min_k=11, max_k=11, max_mismatch=0)
    out = []
    for a, b in ((0, 1013), (992, 1013), (961, 1013)):
        for _ in range(400):
            ref = _rand(rng, 1024)
            if len(kmers(ref, 11)) == 1014:
                break
        else:
            raise AssertionError("no reference of 1024 bases without a repeated 11-mer")
        out.append(ECase("k11_run_%d_%d" % (a, b), ref, _cover(ref, a, b, k=11), True, True, b - a + 1, ncomp=1, records=0, params=params, final_k=11))
    return out


# ---------------------------------------------------------------- (d) the threshold met exactly

def _threshold_cases(rng, thr, params=None):
    out = []
    tag = "" if params is None else "_thr%d" % thr
    # a second stretch of reference k-mers beside a run at full coverage (every offset of [0, 600] in ten or more reads... at its two ends in
    # five): seen cov_threshold - 1 times it has no source (settled), seen cov_threshold times it has one (not settled)
    for a, b in ((640, 703), (639, 704), (64, 100), (65, 100)):
        run = (0, 600) if a > 600 else (32, 63)
        for copies in (thr - 1, thr):
            ref = _plain_ref(rng, 1024, K)
            joined = a == run[1] + 1                                    # (from 64 on it continues the run [32, 63]: one chain whatever its coverage)
            reads = _cover(ref, run[0], run[1]) + _cover(ref, a, b, copies=copies)
            out.append(ECase("stretch_%d_%d_x%d%s" % (a, b, copies, tag), ref, reads, joined or copies < thr, joined, run[1] - run[0] + 1 + b - a + 1,
                             ncomp=1 if joined else 2, records=0 if joined or copies < thr else None, params=params))
    # a chain whose own nodes sit at exactly the threshold (Q is all of it), and one below (no Q at all: no component has a source; the rule
    # before this one starts from the first survivor instead and finds the run to be all there is)
    for copies in (thr, thr - 1):
        ref = _plain_ref(rng, 1024, K)
        out.append(ECase("chain_x%d%s" % (copies, tag), ref, _cover(ref, 300, 360, copies=copies), True, True, 61, ncomp=1, records=0, params=params))
    return out


@functools.lru_cache(maxsize=None)
def family_threshold():
    rng = np.random.default_rng(104)
    return _threshold_cases(rng, 5) + _threshold_cases(rng, 8, params=dict(min_k=K, max_k=K, cov_threshold=8))


# ---------------------------------------------------------------- (e) survivors at two reference offsets

TWO_PARAMS = dict(min_k=K, max_k=K, cov_threshold=7)


def _two_offsets(rng, name, index, copies, junk_before):
    """A k-mer M at offset 700 + index and its reverse complement at 850 + index: one node at two offsets.  Reads over [700, 779] and over
    [850, 929], `copies` each, stand first (behind `junk_before` junk survivors), so M is survivor junk_before + index; a run at full coverage
    over [100, 199].  M is seen 2 * copies times, cov_threshold is 7: with copies = 3 it is below -- the two stretches are a component without
    a source beside the run: settled -- with copies = 4 it is in Q at two offsets: not settled."""
    for _ in range(400):
        ref = _rand(rng, 1024)
        M = ref[700 + index:700 + index + K]
        ref = ref[:850 + index] + rc(M) + ref[850 + index + K:]
        if len(kmers(ref, K)) == 1024 - K:
            break
    else:
        raise AssertionError(name + ": no draw")
    comps = _components(rng, junk_before)
    reads = [c for c in comps for _ in range(6)] + _cover(ref, 700, 779, copies=copies) + _cover(ref, 850, 929, copies=copies) + _cover(ref, 100, 199)
    nsurv = junk_before + 80 + 80 - 1 + 100
    assert len(survivors(reads, K)) == nsurv and len(kmers(ref[700:700 + index + K], K)) == index + 1
    return ECase(name, ref, reads, copies == 3, False, nsurv, records=0 if copies == 3 else None, params=dict(TWO_PARAMS))


def _two_offsets_in_run(rng, name, index, copies, junk_before):
    """The run [100, 179] alone (and junk components in front of it), the k-mer M at offset 100 + index, its reverse complement at offset 600
    where no read lies: the node survives for the run's reads and has exactly the run's two links -- the graph is the chain -- but it stands
    at two offsets.  In Q (ten reads, cov_threshold 7) the test gives up on it (ST[0]: one of the offsets is no run node's first); with four
    reads nothing is in Q and the window is settled whatever its graph.  The rule before this one (LANCET_SETTLE_CHAIN_ONLY=1) does not look
    at the bit: it settles both where the run is all the survivors (no junk), and the oracle, which finds the sink ambiguous, has no record."""
    for _ in range(400):
        ref = _rand(rng, 1024)
        ref = ref[:600] + rc(ref[100 + index:100 + index + K]) + ref[600 + K:]
        if len(kmers(ref, K)) == 1024 - K:
            break
    else:
        raise AssertionError(name + ": no draw")
    comps = _components(rng, junk_before)
    reads = [c for c in comps for _ in range(6)] + _cover(ref, 100, 179, copies=copies)
    return ECase(name, ref, reads, copies < 7, junk_before == 0, junk_before + 80, ncomp=1 + len(comps), records=0, params=dict(TWO_PARAMS))


@functools.lru_cache(maxsize=None)
def family_two_offsets():
    """the st_multi bitmap has one bit per SURVIVOR: index 31, 32 and 1024 + 31 (behind 1024 junk survivors; 1283 survivors would be over the
    capacity of the 512-lane form, so the junk is 960 there: word 30 of the bitmap -- and the full 1024 in a window of the 1024-lane form, below)"""
    rng = np.random.default_rng(105)
    cap = limits(False)["cap"]
    out = []
    for index, junk in ((31, 0), (32, 0), (31, 960)):
        assert junk + 259 <= cap
        for copies in (3, 4):
            out.append(_two_offsets(rng, "two_offsets_si%d_x%d" % (junk + index, copies), index, copies, junk))
    # the node in the run itself, where the bit is all that keeps the window from being settled: survivor 31, 32 and 1024 + 31 (word 32 of the
    # bitmap: 1104 survivors fit the 512-lane form)
    for index, junk in ((31, 0), (32, 0), (31, 1024)):
        assert junk + 80 <= cap
        for copies in (4, 10):
            out.append(_two_offsets_in_run(rng, "two_offsets_in_run_si%d_x%d" % (junk + index, copies), index, copies, junk))
    return out


@functools.lru_cache(maxsize=None)
def family_two_offsets_large():
    rng = np.random.default_rng(106)
    out = []
    for copies in (3, 4):
        c = _two_offsets(rng, "large_two_offsets_si%d_x%d" % (1024 + 31, copies), 31, copies, 1024)
        reads = [r[1] for r in c.reads]
        run = reads[-10:]
        c2 = ECase(c.name, c.ref, _more_than_512(reads, run), c.settled, False, c.nsurv, big=True, records=c.records, params=dict(TWO_PARAMS))
        out.append(c2)
    return out


# ---------------------------------------------------------------- (f) the gates

@functools.lru_cache(maxsize=None)
def family_gates():
    rng = np.random.default_rng(107)
    out = []
    # k = 29 and 31 are tested (one-word k-mers); k = 33 is the 1024-lane form's (BL_KMAX of the 512-lane form is 31), and it does not test
    # above 31.  Under the narrow hand-off (one-word keys) the build kernel does not build a window at k = 33 at all.
    for k in (29, 31, 33):
        ref = _plain_ref(rng, 400, k)
        out.append(ECase("k%d" % k, ref, perfect_reads(ref, k), k <= 31, k <= 31, 400 - k + 1, ncomp=1, records=0, params=dict(min_k=k, max_k=k), final_k=k,
                         why=BLW_K if k > 31 else 0, why_wide=0))
    # a reference of K + 1 bases has two k-mers and is tested; one of K bases has none (reflen - K > 0 fails) -- and no k for the oracle either
    ref = _plain_ref(rng, K + 1, K)
    out.append(ECase("reference_of_k_plus_1_bases", ref, [ref] * 10, True, True, 2, ncomp=1, records=0))
    ref = _rand(rng, K)
    out.append(ECase("reference_of_k_bases", ref, [_rand(rng, 60)] * 6, False, False, None, records=0))
    # the first graph at a k above min_k: the reference's first 20 bases recur at its end, every k up to 19 is passed over for the exact repeat
    # and the window's FIRST graph is the one at 21.  The test does not ask for min_k (it asks that the build kernel's own repeat scan chose the
    # k: `rep == nullptr`, which holds for every first graph): it may settle, and the oracle builds once.
    for _ in range(100):
        R = _rand(rng, K - 1)
        ref = R + _rand(rng, 400 - 2 * (K - 1)) + R
        if len(kmers(ref, K)) == 400 - K + 1:
            break
    out.append(ECase("first_graph_above_min_k", ref, perfect_reads(ref, K), True, True, 400 - K + 1, ncomp=1, records=0, params=dict(min_k=11, max_k=101), final_k=K))
    return out


FAMILIES = {"counts": family_counts, "large": family_large, "runs": family_runs, "runs_k11": family_runs_k11, "threshold": family_threshold,
            "two_offsets": family_two_offsets, "two_offsets_large": family_two_offsets_large, "gates": family_gates}


# ---------------------------------------------------------------- batches, the oracle, the assertions

@functools.lru_cache(maxsize=None)
def groups(family):
    """the cases of a family by parameter set: [(params dict, [ECase], batch)]"""
    by = {}
    for c in FAMILIES[family]():
        by.setdefault(tuple(sorted(c.params.items())), []).append(c)
    return [(dict(key), cs, batch_of(cs)) for key, cs in by.items()]


def all_groups():
    return [(f, gi) for f in FAMILIES for gi in range(len(groups(f)))]


@functools.lru_cache(maxsize=None)
def oracle_of(family, gi):
    """(records, stats, -v trace) of group gi of the family"""
    params, _, batch = groups(family)[gi]
    return oracle.run(batch, abi.default_params(**params), verbose=True)


def _blocks(trace, b):
    by_name = {}
    for blk in trace.split("== Processing ")[1:]:
        by_name[re.match(r"\d+: (\S+) ", blk).group(1)] = blk
    return {w: by_name.get(b.hdr[w], "") for w in range(b.n_windows)}


def trace_counts(blk):
    """(N, nsurv, components) of a window's first graph in the oracle's -v trace; None where the trace has no such line"""
    n = re.search(r"^reads: \d+ reflen: \d+ .*\n\s+0: nodes: (\d+) ", blk, re.M)
    s = re.search(r"^removing low coverage:.*\n\s+0: nodes: (\d+) ", blk, re.M)
    c = re.search(r"^ nodes: \d+ refnodes: \d+ comp: (\d+) ", blk, re.M)
    return tuple(int(m.group(1)) if m else None for m in (n, s, c))


def assert_oracle_side(family, gi):
    """what makes every case its edge, on the oracle's output alone"""
    _, cs, batch = groups(family)[gi]
    ov, ost, tr = oracle_of(family, gi)
    blocks = _blocks(tr, batch)
    for w, c in enumerate(cs):
        n = sum(1 for v in ov if v["window"] == w)
        N, nsurv, ncomp = trace_counts(blocks[w])
        if c.settled or c.settled_wide or c.chain_only:
            assert ost[w]["status"] == 0 and ost[w]["n_builds"] == 1 and n == 0, (c.name, ost[w], n)
        if c.records == 0:
            assert n == 0, (c.name, n)
        if c.records == 1:
            assert n >= 1, (c.name, "no record")
        if c.nsurv is not None:
            assert (nsurv or 0) == c.nsurv, (c.name, "nsurv", nsurv)
        if c.N is not None:
            assert N == c.N, (c.name, "N", N)
        if c.ncomp is not None:
            assert ncomp == c.ncomp, (c.name, "components", ncomp)
        if c.final_k is not None and c.final_k <= 31:
            assert ost[w]["final_k"] == c.final_k and ost[w]["n_builds"] == 1, (c.name, ost[w])
        assert (len(c.reads) > limits(False)["rmax"]) == c.big, (c.name, len(c.reads))
        assert len(c.ref) <= 1024


def expected(family, gi, route, wide):
    """the windows of the group that are settled on a route ("rule" | "chain_only" | "off"), under LANCET_PRE_WIDE=1 (wide) or not"""
    _, cs, _ = groups(family)[gi]
    if route == "off":
        return []
    return [w for w, c in enumerate(cs) if (c.chain_only if route == "chain_only" else c.settled_wide if wide else c.settled)]


def assert_results(family, gi, routes, wide, what="", keys=KEYS):
    """routes: {route: (records, stats, settled windows)}: every route equal to the oracle in records and statistics, the settled sets as stated"""
    _, cs, _ = groups(family)[gi]
    ov, ost, _ = oracle_of(family, gi)
    for tag, (v, st, settled) in routes.items():
        bad = [(cs[w].name, [a[k] for k in keys], [b[k] for k in keys]) for w, (a, b) in enumerate(zip(st, ost)) if any(a[k] != b[k] for k in keys)]
        assert not bad and len(st) == len(ost), (what, tag, bad[:4])
        assert v == ov, (what, tag, "records")
        want = expected(family, gi, tag, wide)
        assert sorted(settled) == want, (what, tag, "settled and should not be", [cs[w].name for w in set(settled) - set(want)],
                                         "not settled and should be", [cs[w].name for w in set(want) - set(settled)])
