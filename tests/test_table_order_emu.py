"""The node table's iteration order and the component numbering alone and without a GPU: the drivers of kernels.h that reproduce
libstdc++'s unordered_map (ht_insert / ht_rehash, first_lowcov -> order_stage, clean_dead_wg in both forms, mark_connected_components_wg,
order_insert, clean_dead) run one script on made-up 64-bit hashes beside a real std::unordered_map whose hasher returns those hashes
(tests/emu/emu_table_order.cc), in the single-wave build and in the re-run tier's (-DLANCET_FAT=1).

Per script and stage, rig against model, exact and whole: the order, the bucket count, the rehash threshold, the element count; after the
numbering the component of every node, numcomp and refcomp.  Nothing here restates the container's rules: the helper `final_buckets`
below only AIMS inputs (survivor counts next to a bucket count, hashes that are multiples of it) and every aim is checked on the
model's own bucket_count() before a rig is looked at."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle

CHAIN = [13, 29, 59, 127, 257, 541, 1109, 2357, 5087, 10273, 20753]
NS = sorted(set(list(range(1, 16)) + [b + d for b in CHAIN for d in (-2, -1, 0, 1, 2)] +
                [1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 5631, 5632, 5633, 14335, 14336, 14337]))
ONE_BUCKET_CAP = 1200                     # families that put all nodes into one or two runs: the in-run insertion sort is quadratic
STAGES, HEAD, SPECIAL, EMAX = 6, 5, 4, 8
NIL = 0xFFFFFFFF
STAGE_NAMES = ["insert 0..N-1", "erase non-survivors", "markConnectedComponents", "insert N, N+1", "erase the given set", "insert N+2, N+3"]


@pytest.fixture(scope="module", params=["plain", "fat"])
def rig(request, tmp_path_factory):
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
    so = os.path.join(str(tmp_path_factory.mktemp("emu_table_order_" + request.param)), "libemu_table_order.so")
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-strict-aliasing", "-w"]
    cmd += ["-DLANCET_FAT=1"] if request.param == "fat" else []
    header = os.environ.get("LANCET_EMU_KERNELS_H")                # (to hold the rig against another revision of the headers)
    cmd += ['-DLANCET_EMU_KERNELS_H="%s"' % header] if header else []
    subprocess.run(cmd + ["-o", so, os.path.join(here, "emu_table_order.cc")], check=True)
    L = ctypes.CDLL(so)
    L.lancet_emu_table_order.restype = None
    L.lancet_emu_table_order_words.restype = ctypes.c_uint32
    return L


def final_buckets(n):
    """where N inserts are expected to leave the bucket count -- an aim for the generators, asserted on the model"""
    return next(b for b in CHAIN + [42043] if b >= n)


class Script:
    def __init__(self, nhash, surv=None, edges=(), touch=None, erase2=None):
        self.N = len(nhash) - SPECIAL
        self.nhash = np.asarray(nhash, dtype=np.uint64)
        self.surv = np.ones(self.N, np.uint8) if surv is None else np.asarray(surv, np.uint8)
        self.touch = np.zeros(self.N, np.uint8) if touch is None else np.asarray(touch, np.uint8)
        self.erase2 = np.zeros(self.N + 2, np.uint8) if erase2 is None else np.asarray(erase2, np.uint8)
        self.necnt = np.zeros(self.N, np.uint32)
        self.edges = np.zeros((self.N, EMAX), np.uint32)
        for u, v in edges:
            self.link(u, v)

    def link(self, u, v):
        assert self.surv[u] and self.surv[v]
        for a, b in ((u, v),) if u == v else ((u, v), (v, u)):
            assert self.necnt[a] < EMAX
            self.edges[a, self.necnt[a]] = b
            self.necnt[a] += 1


class Result:
    def __init__(self, N, words):
        self.N = N
        w = HEAD + N + SPECIAL
        self.stages = [words[s * w:(s + 1) * w] for s in range(STAGES)]
        tail = words[STAGES * w:]
        self.numcomp, self.refcomp, self.comp = int(tail[0]), int(tail[1]), tail[2:2 + N]

    def M(self, s): return int(self.stages[s][0])
    def buckets(self, s): return int(self.stages[s][1])
    def order(self, s): return self.stages[s][HEAD:HEAD + self.M(s)]


def run(L, sc):
    bw = int(L.lancet_emu_table_order_words(ctypes.c_uint32(sc.N)))
    out = np.zeros(3 * bw, np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    L.lancet_emu_table_order(ctypes.c_uint32(sc.N), p(sc.nhash), p(sc.surv), p(sc.touch), p(sc.necnt), p(np.ascontiguousarray(sc.edges)), p(sc.erase2), p(out))
    return [Result(sc.N, out[i * bw:(i + 1) * bw]) for i in range(3)]


def model_of(L, sc):
    return run(L, sc)[2]


def check(L, sc, what, aim=None):
    """aim(model): what makes the script its edge, asserted on the model before a rig is looked at"""
    a, b, m = run(L, sc)
    assert m.M(0) == sc.N and m.M(1) == int(sc.surv.sum()), what
    if aim:
        aim(m)
    for name, r in (("ht_insert + flags form", a), ("first_lowcov + survb form", b)):
        for s in range(STAGES):
            if not np.array_equal(r.stages[s], m.stages[s]):
                head = "M, buckets, next_resize, elements, overflow: %s, the model's %s" % (list(r.stages[s][:HEAD]), list(m.stages[s][:HEAD]))
                diff = np.nonzero(r.stages[s][HEAD:] != m.stages[s][HEAD:])[0]
                pytest.fail("%s: %s, stage %d (%s): %s; the order differs at %d positions, the first %s" % (what, name, s, STAGE_NAMES[s], head, len(diff), diff[:4]))
        assert (r.numcomp, r.refcomp) == (m.numcomp, m.refcomp), "%s: %s: numcomp, refcomp" % (what, name)
        bad = np.nonzero(r.comp != m.comp)[0]
        assert len(bad) == 0, "%s: %s: the component of %d nodes, the first %s: %s, the model's %s" % (what, name, len(bad), bad[:4], r.comp[bad[:4]], m.comp[bad[:4]])
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# hash families
# ---------------------------------------------------------------------------------------------------------------------------------
_POOL = None


def kmer_hash_pool():
    global _POOL
    if _POOL is None:
        rng = np.random.RandomState(20753)
        seqs = rng.randint(0, 4, (21000, 21))
        _POOL = np.array([oracle.std_hash("".join("ACGT"[c] for c in row)) for row in seqs], dtype=np.uint64)
    return _POOL


# all primes of the chain that a table of up to ONE_BUCKET_CAP + 4 nodes goes through; 17 multiples of their product fit into 64 bits
_L = 13 * 29 * 59 * 127 * 257 * 541 * 1109 * 2357


def fam_std_hash(n, rng):
    pool = kmer_hash_pool()
    at = int(rng.randint(0, len(pool) - n))
    return pool[at:at + n]


def fam_id(n, rng): return np.arange(n, dtype=np.uint64)
def fam_equal(n, rng): return np.full(n, 0x1234567, np.uint64)
def fam_equal_mod_primes(n, rng): return np.uint64(7) + np.uint64(_L) * (np.arange(n, dtype=np.uint64) % np.uint64(17))


def fam_high(n, rng):
    h = (rng.randint(0, 2 ** 62, n).astype(np.uint64) * np.uint64(2) + rng.randint(0, 2, n).astype(np.uint64)) | np.uint64(1 << 63)
    h[rng.rand(n) < 0.1] = np.uint64(2 ** 64 - 1)
    h[rng.rand(n) < 0.05] = np.uint64(1 << 63)
    return h


def fam_multiples(n, rng):
    """multiples of the bucket count that is current when the node goes in (and of the one before and after): bucket 0, again and again"""
    chain = np.array(CHAIN, dtype=np.int64)
    at = np.minimum(np.searchsorted(chain, np.arange(1, n + 1)), len(CHAIN) - 1)
    b = chain[np.clip(at + rng.randint(-1, 2, n), 0, len(CHAIN) - 1)]
    return np.where(np.arange(n) % 3 != 0, b * rng.randint(0, 2 ** 40, n), rng.randint(0, 2 ** 62, n)).astype(np.uint64)


def fam_two(n, rng): return np.where(np.arange(n) % 2 == 0, np.uint64(5), np.uint64(2 ** 64 - 3)).astype(np.uint64)


FAMILIES = {"std_hash": fam_std_hash, "id": fam_id, "equal": fam_equal, "equal_mod_primes": fam_equal_mod_primes, "high": fam_high,
            "multiples": fam_multiples, "two_values": fam_two}
CAPPED = {"equal", "equal_mod_primes", "two_values"}


# ---------------------------------------------------------------------------------------------------------------------------------
# survivor sets
# ---------------------------------------------------------------------------------------------------------------------------------
def runs_of(nhash, N):
    b = (nhash[:N] % np.uint64(final_buckets(N))).astype(np.int64)
    runs = {}
    for n in range(N):
        runs.setdefault(int(b[n]), []).append(n)
    return runs.values()


def surv_all(h, N, rng): return np.ones(N, np.uint8)
def surv_one(h, N, rng): s = np.zeros(N, np.uint8); s[int(rng.randint(N))] = 1; return s
def surv_second(h, N, rng): return (np.arange(N) % 2 == 0).astype(np.uint8)


def surv_of_run(pick):
    def f(h, N, rng):
        s = np.zeros(N, np.uint8)
        for r in runs_of(h, N):
            s[pick(r)] = 1                         # (a run lists its nodes latest first: the largest id is its first element)
        return s
    return f


def surv_random(p):
    def f(h, N, rng):
        s = (rng.rand(N) < p).astype(np.uint8)
        s[int(rng.randint(N))] = 1
        return s
    return f


SURVIVORS = {"all": surv_all, "one": surv_one, "every_second": surv_second, "run_first": surv_of_run(lambda r: r[-1]),
             "run_middle": surv_of_run(lambda r: r[len(r) // 2]), "run_last": surv_of_run(lambda r: r[0]), "random_5": surv_random(0.05), "random_50": surv_random(0.5)}


# ---------------------------------------------------------------------------------------------------------------------------------
# graphs over the survivors
# ---------------------------------------------------------------------------------------------------------------------------------
def chains(groups):
    return [(u, v) for g in groups for u, v in zip(g, g[1:])]


def graph_chain_ids(ids, rng): return chains([list(ids)])


def graph_components(k):
    def f(ids, rng):
        ids = list(rng.permutation(ids))
        k1 = min(k, len(ids))
        return chains([ids[i::k1] for i in range(k1)])
    return f


def graph_self_edges(ids, rng):
    e = graph_components(3)(ids, rng)
    return e + [(int(u), int(u)) for u in ids[::4]]


def graph_stars(ids, rng):
    """hubs of degree up to 8 (more neighbours than the three the numbering keeps beside the table position)"""
    ids = list(rng.permutation(ids))
    e = []
    for i in range(0, len(ids) - 8, 9):
        e += [(ids[i], v) for v in ids[i + 1:i + 9]]
    return e


GRAPHS = {"chain_ids": graph_chain_ids, "c1": graph_components(1), "c2": graph_components(2), "c31": graph_components(31), "c32": graph_components(32),
          "c33": graph_components(33), "c200": graph_components(200), "self_edges": graph_self_edges, "stars": graph_stars}


def random_erase2(sc, rng):
    e = np.zeros(sc.N + 2, np.uint8)
    e[:sc.N] = (rng.rand(sc.N) < 0.3) & (sc.surv != 0)
    e[sc.N:] = rng.randint(0, 2, 2)
    return e


def make_script(fam, N, survivors, graph, seed, touch="some"):
    rng = np.random.RandomState(seed)
    h = FAMILIES[fam](N + SPECIAL, rng)
    surv = SURVIVORS[survivors](h, N, rng)
    ids = np.nonzero(surv)[0]
    sc = Script(h, surv, GRAPHS[graph](ids, rng))
    if touch == "some":
        sc.touch = ((rng.rand(N) < 0.02) & (surv != 0)).astype(np.uint8)
    elif touch == "all":
        sc.touch = surv.copy()
    sc.erase2 = random_erase2(sc, rng)
    return sc


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_every_size_and_family(rig, fam):
    """every N of the list under every hash family; the survivor sets and the graphs take turns"""
    sv, gr = sorted(SURVIVORS), sorted(GRAPHS)
    for i, N in enumerate(NS):
        if fam in CAPPED and N > ONE_BUCKET_CAP:
            continue
        sc = make_script(fam, N, sv[i % len(sv)], gr[(i // 2) % len(gr)], 1000 + i)
        def aim(m):
            assert m.buckets(0) == final_buckets(N)
        check(rig, sc, "%s N=%d %s %s" % (fam, N, sv[i % len(sv)], gr[(i // 2) % len(gr)]), aim)


@pytest.mark.parametrize("survivors", sorted(SURVIVORS))
def test_every_survivor_set(rig, survivors):
    for fam in sorted(FAMILIES):
        for N in (14, 30, 59, 128, 542, 1111, 4097, 10275):
            if fam in CAPPED and N > ONE_BUCKET_CAP:
                continue
            check(rig, make_script(fam, N, survivors, "c2", 7 * N), "%s N=%d %s" % (fam, N, survivors))


@pytest.mark.parametrize("B", CHAIN)
def test_special_inserts_cross_the_threshold(rig, B):
    """N <= B nodes of which B - 2, B - 1 or B survive: the two special-node insertions rehash at the second, at the first, or not at all;
    then the second pair does (or the erasures in between make room)"""
    nxt = final_buckets(2 * B)
    for fam in sorted(FAMILIES):
        if fam in CAPPED and B > ONE_BUCKET_CAP:
            continue
        for N in (B - 1, B):
            for nsurv in (B - 2, B - 1, B):
                if nsurv > N:
                    continue
                for erase in ("none", "random"):
                    rng = np.random.RandomState(B + N + nsurv)
                    h = FAMILIES[fam](N + SPECIAL, rng)
                    surv = np.ones(N, np.uint8)
                    surv[rng.permutation(N)[:N - nsurv]] = 0
                    sc = Script(h, surv, GRAPHS["c2"](np.nonzero(surv)[0], rng))
                    if erase == "random":
                        sc.erase2 = random_erase2(sc, rng)
                    what = "%s B=%d N=%d nsurv=%d erase=%s" % (fam, B, N, nsurv, erase)

                    def aim(m):
                        assert m.buckets(1) == B and m.M(1) == nsurv, what
                        assert m.buckets(3) == (B if nsurv == B - 2 else nxt), what
                        if erase == "none":
                            assert m.buckets(5) == nxt, what
                    check(rig, sc, what, aim)


@pytest.mark.parametrize("graph", sorted(GRAPHS))
def test_component_numbering(rig, graph):
    for fam in ("std_hash", "id", "high", "equal_mod_primes"):
        for N in (9, 257, 1109, 2500):
            if fam in CAPPED and N > ONE_BUCKET_CAP:
                continue
            for survivors in ("all", "random_50"):
                for touch in ("none", "some", "all"):
                    check(rig, make_script(fam, N, survivors, graph, N + 3, touch), "%s N=%d %s %s touchRef %s" % (fam, N, survivors, graph, touch))


def test_chain_in_reverse_table_order(rig):
    """one component whose links run against the table: the label of the last position has to travel to the first"""
    for fam in ("std_hash", "multiples", "two_values"):
        for N in (61, 600, 1200):
            rng = np.random.RandomState(N)
            h = FAMILIES[fam](N + SPECIAL, rng)
            surv = SURVIVORS["random_50"](h, N, rng)
            order = [int(x) for x in model_of(rig, Script(h, surv)).order(1)]
            sc = Script(h, surv, chains([order[::-1]]), touch=(np.arange(N) == order[-1]).astype(np.uint8))
            m = check(rig, sc, "%s N=%d" % (fam, N))
            assert (m.numcomp, m.refcomp) == (1, 1)


def test_first_node_is_not_the_smallest_id(rig):
    """components numbered by their first node in TABLE order: ones whose first node is not their smallest id, and whose numbers are
    therefore not in the order of their smallest ids"""
    for N in (300, 1500):
        sc = make_script("std_hash", N, "all", "c33", N)
        m = check(rig, sc, "N=%d" % N)
        order = [int(x) for x in m.order(1)]
        first, smallest = {}, {}
        for n in order:
            first.setdefault(int(m.comp[n]), n)
            smallest[int(m.comp[n])] = min(smallest.get(int(m.comp[n]), n), n)
        assert m.numcomp == 33 and sum(first[c] != smallest[c] for c in first) > 16
        by_id = sorted(smallest, key=lambda c: smallest[c])
        assert by_id != sorted(smallest)


def test_reference_only_in_components_above_32(rig):
    """touchRef on none of the first 32 components: whatever keeps the reference components as a 32-bit mask would lose these"""
    for graph, N in (("c33", 400), ("c200", 2000)):
        sc = make_script("std_hash", N, "all", graph, N, touch="none")
        m = model_of(rig, sc)
        sc.touch = (m.comp > 32).astype(np.uint8)
        m = check(rig, sc, "%s N=%d" % (graph, N))
        assert m.refcomp == m.numcomp - 32 and m.refcomp >= 1
        comp1 = np.nonzero(m.comp == 1)[0]
        sc.erase2[:] = 0
        sc.erase2[comp1] = 1                       # all of component 1 goes, as after a component that was given up
        check(rig, sc, "%s N=%d, component 1 erased" % (graph, N))
