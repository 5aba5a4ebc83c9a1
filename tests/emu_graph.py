"""The hand-made graph of the rigs that run one graph stage of kernels.h beside a plain model (tests/emu/emu_graph_model.h): the builder, and
the packing of its records into the words the rigs read.  Used by test_compress_emu.py and test_clean_passes_emu.py."""
import numpy as np

FF, FR, RF, RR = 0, 1, 2, 3
TWIN = {FF: RR, RR: FF, FR: FR, RF: RF}
TUMOR, NORMAL, DEAD, SOURCE, SINK = 1, 2, 4, 8, 16
NIL = 0xFFFFFFFF
IN_WORDS, OUT_HEAD = 28, 24


class Graph:
    """k-mer nodes (one k-mer each, descriptors at id * K, no room in the deque) and unitigs made of k-mers that are no longer in the table.
    link(u, v, d) adds the edge and its twin at v (Edge.hh: FF <-> RR, FR and RF are their own)."""

    def __init__(self, seed=1, K=5):
        self.K = K
        self.rng = np.random.RandomState(seed)
        self.rec = []           # dicts
        self.order = []
        self.seq = []
        self.qv = []            # rows of K * 4

    def _record(self, flags, comp, cov=(0, 0, 0, 0), kc=(0, 0, 0, 0), nqv=NIL, nkm=0, nkmT=0, lo=0, hi=0, clo=0, chi=0):
        self.rec.append(dict(flags=flags, comp=comp, edges=[], cov=cov, kc=kc, nqv=nqv, nkm=nkm, nkmT=nkmT, lo=lo, hi=hi, clo=clo, chi=chi))
        return len(self.rec) - 1

    def _kmer_record(self, flags, comp, cov):
        n, row, lo = len(self.rec), len(self.qv), len(self.seq)
        kc = tuple(int(x) for x in self.rng.randint(0, 9, 4))
        self.qv.append(self.rng.randint(0, 6, (self.K, 4)))
        self.seq += [n << 9 | i << 2 | int(self.rng.randint(4)) for i in range(self.K)]
        return self._record(flags, comp, cov, kc, nqv=row, nkm=1, nkmT=1 if flags & 3 == TUMOR else 0, lo=lo, hi=lo + self.K, clo=lo, chi=lo + self.K)

    def kmers(self, count, cov=None, flags=None, comp=1, table=True):
        ids = []
        for i in range(count):
            c = cov[i] if cov else tuple(float(x) for x in self.rng.randint(0, 40, 4))
            ids.append(self._kmer_record(flags[i] if flags else (TUMOR, NORMAL, TUMOR | NORMAL)[i % 3], comp, c))
        if table:
            self.order += ids
        return ids

    def special(self, flag):
        n = self._record(flag, 1)
        self.order.append(n)
        return n

    def unitig(self, length, room=(0, 0), flags=TUMOR, cov=(3.0, 1.0, 0.0, 2.0), weak_last=False):
        """a node of `length` bases over length - self.K + 1 k-mers that left the table (their records keep the counts); room: free descriptor
        slots before / behind its deque; weak_last: its last k-mer has the smallest counts, so that the minima sit on the last descriptor"""
        ks = self.ghosts[self.ghost_at:self.ghost_at + length - self.K + 1]
        self.ghost_at += length - self.K + 1
        assert len(ks) == length - self.K + 1
        if weak_last:
            self.rec[ks[-1]]["kc"] = (0, 0, 0, 0)
            self.qv[self.rec[ks[-1]]["nqv"]][self.K - 1] = 0
        desc = [ks[0] << 9 | i << 2 | int(self.rng.randint(4)) for i in range(self.K)] + [k << 9 | (self.K - 1) << 2 | int(self.rng.randint(4)) for k in ks[1:]]
        clo = len(self.seq); lo = clo + room[0]
        self.seq += [0] * room[0] + desc + [0] * room[1]
        n = self._record(flags, 1, cov, nqv=NIL, nkm=len(ks), nkmT=len(ks) if flags & 3 == TUMOR else 0, lo=lo, hi=lo + length, clo=clo, chi=len(self.seq))
        self.order.append(n)
        return n

    def with_ghosts(self, count):
        """k-mer records that are dead and out of the table, for unitigs to be made of"""
        self.ghosts = self.kmers(count, flags=[DEAD | TUMOR] * count, comp=1, table=False)
        for g in self.ghosts:
            self.rec[g]["kc"] = tuple(int(x) for x in self.rng.randint(2, 9, 4))
            self.qv[self.rec[g]["nqv"]][:] = self.rng.randint(2, 6, (self.K, 4))
        self.ghost_at = 0
        return self

    def link(self, u, v, d=FF, used=False):
        self.rec[u]["edges"].append(v | d << 28 | int(used) << 30)
        if not (u == v and TWIN[d] == d):
            self.rec[v]["edges"].append(u | TWIN[d] << 28 | int(used) << 30)
        return self

    def half_edge(self, u, v, d):
        self.rec[u]["edges"].append(v | d << 28)
        return self

    def chain(self, nodes, dirs=None):
        """links along the list; dirs[i] is the direction of link i in travel orientation (a node entered reversed is left through R)"""
        rev = False
        for i, (u, v) in enumerate(zip(nodes, nodes[1:])):
            d = dirs[i] if dirs else FF
            arrives_rev = rev ^ (d in (FR, RF))
            self.link(u, v, {(False, False): FF, (False, True): FR, (True, False): RF, (True, True): RR}[(rev, arrives_rev)])
            rev = arrives_rev
        return self


def pack(g, seq_cap=None, len_max=None):
    """the records, the descriptor arena and the quality rows as the rigs take them: (n, order, rec, seq, seq_top, seq_cap, qv, len_max)"""
    n = len(g.rec)
    rec = np.zeros((n, IN_WORDS), np.uint32)
    for i, r in enumerate(g.rec):
        assert len(r["edges"]) <= 12
        rec[i, 0:3] = (r["flags"], r["comp"], len(r["edges"]))
        rec[i, 3:3 + len(r["edges"])] = r["edges"]
        rec[i, 15:19] = np.asarray(r["cov"], np.float32).view(np.uint32)
        rec[i, 19] = r["kc"][0] | r["kc"][1] << 16
        rec[i, 20] = r["kc"][2] | r["kc"][3] << 16
        rec[i, 21:28] = (r["nqv"], r["nkm"], r["nkmT"], r["lo"], r["hi"], r["clo"], r["chi"])
    total = sum(r["hi"] - r["lo"] for r in g.rec if not r["flags"] & DEAD)
    len_max = len_max or total + 8
    seq_top = len(g.seq)
    seq_cap = seq_cap or seq_top + 8 * total + 256
    seq = np.zeros(max(seq_cap, seq_top), np.uint32); seq[:seq_top] = g.seq
    qv = np.ascontiguousarray(np.asarray(g.qv, np.uint16).reshape(-1))
    order = np.asarray(g.order, np.uint32)
    return n, order, rec, seq, seq_top, seq_cap, qv, len_max
