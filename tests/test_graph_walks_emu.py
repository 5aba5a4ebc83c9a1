"""The two graph walks whose visiting order must be the reference's, alone and without a GPU: kernels.h cycle_dfs (Graph_t::hasCycle,
reference src/Graph.cc:593-681) and path_fifo (Graph_t::bfs, :1299-1425) run on hand-made cleaned graphs through the view of the node
records and through the view of graph_cache_wg's copy, and beside a plain model of the reference lines (tests/emu/emu_walks.cc).

Per graph: the same answer and the same colour of every node from both views and the model; the same queue entry by entry, the same
best path.  The build kernel's third view of cycle_dfs is covered where it can be observed, by the graphs-built-ahead counts of
test_emu_kernels.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

FF, FR, RF, RR = 0, 1, 2, 3
SOURCE, SINK = 8, 16                     # NF_SOURCE, NF_SINK
NIL = 0xFFFFFFFF
GC_MAX = 48                              # kernels.h: the longest table graph_cache_wg takes
PATTERN = 0xCDCDCDCD
K = 5


@pytest.fixture(scope="module")
def walks(tmp_path_factory):
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
    so = os.path.join(str(tmp_path_factory.mktemp("emu_walks")), "libemu_walks.so")
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-strict-aliasing", "-w",
                    "-o", so, os.path.join(here, "emu_walks.cc")], check=True)
    L = ctypes.CDLL(so)
    L.lancet_emu_walks.restype = ctypes.c_int
    return L


class Graph:
    """Node records by id + table order.  link(u, v, d) adds the edge and its twin at v (Edge.hh: FF <-> RR, FR and RF are their own)."""

    def __init__(self, order, special, length=9):
        self.order = list(order)
        self.n = max(order) + 1
        self.flags = [0] * self.n
        self.len = [0] * self.n
        self.edges = [[] for _ in range(self.n)]
        for n in order:
            self.flags[n] = special.get(n, 1)                      # NF_TUMOR on the ordinary ones
            self.len[n] = 0 if n in special else length
        self.source = next(n for n, f in special.items() if f == SOURCE)
        self.sink = next(n for n, f in special.items() if f == SINK)

    def link(self, u, v, d=FF, used=False):
        self.edges[u].append(v | d << 28 | int(used) << 30)
        self.edges[v].append(u | {FF: RR, RR: FF, FR: FR, RF: RF}[d] << 28 | int(used) << 30)
        return self

    def chain(self, nodes, used=False):
        for u, v in zip(nodes, nodes[1:]):
            self.link(u, v, FF, used)
        return self


def run(L, g, reflen=60, max_indel=20, dfs_limit=0, tracing=False, queue_cap=256):
    M = len(g.order)
    u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)
    edges = np.zeros((g.n, 12), np.uint32)
    for n, el in enumerate(g.edges):
        assert len(el) <= 12
        edges[n, :len(el)] = el
    order, flags, necnt, length = u32(g.order), u32(g.flags), u32([len(e) for e in g.edges]), u32(g.len)
    cyc = np.zeros(3, np.int32); col = np.zeros((3, M), np.uint32); bfs = np.zeros((3, 3), np.uint32); queue = np.zeros((3, queue_cap, 5), np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    cached = L.lancet_emu_walks(ctypes.c_uint32(g.n), ctypes.c_uint32(M), p(order), p(flags), p(necnt), p(edges), p(length),
                                ctypes.c_uint32(g.source), ctypes.c_uint32(g.sink), K, reflen, max_indel, dfs_limit, ctypes.c_uint32(int(tracing)),
                                ctypes.c_uint32(queue_cap), p(cyc), p(col), p(bfs), p(queue))
    return dict(cached=bool(cached), cyc=cyc.tolist(), col=col, bfs=bfs, queue=queue, tracing=tracing, order=g.order)


def path_of(r, view=0):
    """nodes of the best path of a view, source first"""
    q, i, out = r["queue"][view], int(r["bfs"][view][0]), []
    while i != NIL:
        out.append(int(q[i][1])); i = int(q[i][0])
    return out[::-1]


def check(r, cycle, cached=True):
    HBM, GC, MODEL = 0, 1, 2
    assert r["cached"] == cached
    assert r["cyc"][HBM] == r["cyc"][MODEL] == int(cycle)
    assert (r["col"][HBM] == r["col"][MODEL]).all(), (r["col"][HBM], r["col"][MODEL])
    model_q = r["queue"][MODEL].copy()
    n_model = int(r["bfs"][MODEL][2])
    assert (model_q[n_model:] == PATTERN).all() and n_model >= 1
    if not r["tracing"]:                                           # Path_t::hasCycle (bit 1 of `bits`, the top byte of word 4) is evaluated only for the trace
        assert not (r["queue"][HBM][:n_model, 4] >> 25 & 1).any()
        model_q[:n_model, 4] &= ~np.uint32(2 << 24)
    assert (r["queue"][HBM] == model_q).all()                      # entry by entry; what the model did not push, nobody wrote
    assert int(r["bfs"][HBM][0]) == int(r["bfs"][MODEL][0])        # best path
    assert int(r["bfs"][HBM][1]) == int(r["bfs"][MODEL][1])        # DFS_LIMIT hit
    assert int(r["bfs"][HBM][2]) == 0                              # no overflow
    if cached:
        assert r["cyc"][GC] == r["cyc"][HBM]
        assert (r["col"][GC] == r["col"][HBM]).all(), (r["col"][GC], r["col"][HBM])
        assert (r["queue"][GC] == r["queue"][HBM]).all()
        assert (r["bfs"][GC] == r["bfs"][HBM]).all()
    else:
        assert r["cyc"][GC] == -1


SRC, SNK = 40, 41
SPECIAL = {SRC: SOURCE, SNK: SINK}


def bubble(first, second, used_first=False):
    """source - 7 - (first | second) - 9 - sink; node 7 lists the edge to `first` first"""
    g = Graph([9, SRC, second, 7, first, SNK], SPECIAL)
    g.link(SRC, 7, FF, used_first).link(7, first, FF, used_first).link(7, second).link(first, 9, FF, used_first).link(second, 9).link(9, SNK, FF, used_first)
    return g


def test_chain_from_source_to_sink(walks):
    r = run(walks, Graph([9, SRC, 3, 7, SNK], SPECIAL).chain([SRC, 7, 3, 9, SNK]))
    check(r, cycle=False)
    assert path_of(r) == [SRC, 7, 3, 9, SNK]
    assert r["col"][0].tolist() == [3, 3, 3, 3, 0]                 # every node that was entered is done; the sink never is


@pytest.mark.parametrize("first,second", [(3, 5), (5, 3)])
def test_bubble_of_two_equal_paths_the_first_dequeued_wins(walks, first, second):
    r = run(walks, bubble(first, second))
    check(r, cycle=False)
    assert path_of(r, 0) == path_of(r, 1) == [SRC, 7, first, 9, SNK]      # the branch node 7 lists first: an expansion in another order picks the other


def test_cycle_reachable_only_in_direction_R(walks):
    # forwards: source - 7 - 9 - sink, no cycle.  Backwards out of the source: 11 -> 12 -> 11.
    g = Graph([12, 9, SRC, 11, 7, SNK], SPECIAL).chain([SRC, 7, 9, SNK])
    g.link(SRC, 11, RF).link(11, 12, FF)
    g.edges[12].append(11 | FF << 28); g.edges[11].append(12 | RR << 28)
    r = run(walks, g)
    check(r, cycle=True)
    by_node = dict(zip(g.order, r["col"][0].tolist()))
    assert by_node[7] == 3 and by_node[9] == 3                     # direction F was walked to its end first
    assert by_node[11] == 2 and by_node[12] == 2                   # ... then R met a node on the stack
    assert path_of(r) == [SRC, 7, 9, SNK]


@pytest.mark.parametrize("tracing", [False, True], ids=["plain", "traced"])
def test_self_loop_on_a_tandem_node(walks, tracing):
    g = Graph([7, SNK, SRC], SPECIAL).link(SRC, 7)
    g.edges[7].append(7 | FF << 28); g.edges[7].append(7 | RR << 28)
    g.link(7, SNK)
    r = run(walks, g, reflen=30, max_indel=10, tracing=tracing)
    check(r, cycle=True)
    p = path_of(r)
    assert p[0] == SRC and p[-1] == SNK and set(p[1:-1]) == {7} and len(p) > 3      # every turn of the loop is one more unused edge: the longest scores highest
    if tracing:
        assert (r["queue"][0][:int(r["bfs"][2][2]), 4] >> 25 & 1).any()      # Path_t::hasCycle was seen, on both views (check compared them)


def test_edge_into_a_special_node_is_skipped(walks):
    # 3 has an edge back into the source, which is on the stack all along: hasCycle does not look at special nodes, the path search follows it
    g = Graph([3, SRC, SNK, 7], SPECIAL).chain([SRC, 7, 3, SNK])
    g.edges[3].append(SRC | FF << 28); g.edges[SRC].append(3 | RR << 28)
    r = run(walks, g, reflen=30, max_indel=10)
    check(r, cycle=False)
    p = path_of(r)
    assert p[:4] == [SRC, 7, 3, SRC] and p[-1] == SNK              # (going round through the source scores higher than the direct path)


def test_node_with_twelve_edges_is_still_cached(walks):
    mids = list(range(20, 31))                                     # 11 parallel branches: 7 has 1 + 11 edges, 9 has 11 + 1
    g = Graph([9] + mids[::-1] + [SRC, 7, SNK], SPECIAL).link(SRC, 7)
    for m in mids:
        g.link(7, m)
    for m in mids:
        g.link(m, 9)
    g.link(9, SNK)
    assert len(g.edges[7]) == 12 and len(g.edges[9]) == 12
    r = run(walks, g)
    check(r, cycle=False)
    assert path_of(r) == [SRC, 7, mids[0], 9, SNK]


def test_table_of_one_node_more_than_the_cache_takes(walks):
    inner = [200 - 2 * i for i in range(GC_MAX - 1)]               # GC_MAX + 1 nodes with the two special ones
    g = Graph(inner[::2] + [SNK] + inner[1::2] + [SRC], SPECIAL).chain([SRC] + inner + [SNK])
    assert len(g.order) == GC_MAX + 1
    r = run(walks, g, reflen=400)
    check(r, cycle=False, cached=False)                            # graph_cache_wg declines: the node records' view alone, against the model
    assert path_of(r) == [SRC] + inner + [SNK]
    g2 = Graph(inner[2::2] + [SNK] + inner[1::2] + [SRC], SPECIAL).chain([SRC] + inner[1:] + [SNK])
    check(run(walks, g2, reflen=400), cycle=False, cached=True)    # ... and GC_MAX nodes are taken


def test_dfs_limit_hit_mid_search(walks):
    r = run(walks, bubble(3, 5), dfs_limit=4)
    check(r, cycle=False)
    assert int(r["bfs"][0][1]) == 1 and int(r["bfs"][1][1]) == 1 and int(r["bfs"][0][0]) == NIL
    full = run(walks, bubble(3, 5))
    assert 1 < int(r["bfs"][2][2]) < int(full["bfs"][2][2])        # a partial queue


def test_edge_used_by_an_earlier_path_changes_score_and_bits(walks):
    r = run(walks, bubble(3, 5, used_first=True))
    check(r, cycle=False)
    assert path_of(r, 0) == path_of(r, 1) == [SRC, 7, 5, 9, SNK]   # the branch listed first is all used edges: its path is no complete path
    q = r["queue"][0]
    ends = [e for e in q[:int(r["bfs"][2][2])] if int(e[1]) == SNK]
    assert sorted((int(e[4]) & 0xFFFF, int(e[4]) >> 24 & 1) for e in ends) == [(0, 1), (2, 0)]      # (score, still-all-used flag)
