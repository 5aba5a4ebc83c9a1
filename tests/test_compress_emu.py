"""Unitig compression alone and without a GPU: the four drivers of kernels.h that state Graph_t::compressNode / compress / cleanDead
(reference src/Graph.cc:2486-2762) run on hand-made graphs, each from the same start state -- compress (the literal loop),
compress_prepare -> compress_fast, compress_prepare -> compress_rank, compress_wg -- beside a plain model of the reference lines
(tests/emu/emu_compress.cc), in the single-wave build and in the re-run tier's (-DLANCET_FAT=1, where compress_wg runs the one-lane body).

Per graph and driver against the model: the live table order, which nodes are dead, and per live node the edge list word for word
(bit 30 included), every descriptor of its string, cov[4] by bit pattern, mincov, mincovqv, nkm, nkmT, the colour flags; the overflow
flag; for compress_rank whether it declined (and that it then left the graph untouched).

The build kernel's bl_compress_first shares the link rule, the port arithmetic and the edge adoption with these drivers; it needs a whole
hand-off area and is held where it can be observed, by the records and the counts of test_emu_kernels.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from emu_graph import DEAD, FF, FR, NORMAL, OUT_HEAD, RF, RR, SINK, SOURCE, TUMOR, Graph, pack

K = 5                                                              # (the builder's default)
DRIVERS = ["compress", "compress_fast", "compress_rank", "compress_wg"]


@pytest.fixture(scope="module", params=["plain", "fat"])
def rig(request, tmp_path_factory):
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
    so = os.path.join(str(tmp_path_factory.mktemp("emu_compress_" + request.param)), "libemu_compress.so")
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-strict-aliasing", "-w"]
    cmd += ["-DLANCET_FAT=1"] if request.param == "fat" else []
    header = os.environ.get("LANCET_EMU_KERNELS_H")                # (to hold the rig against another revision of the headers)
    cmd += ['-DLANCET_EMU_KERNELS_H="%s"' % header] if header else []
    subprocess.run(cmd + ["-o", so, os.path.join(here, "emu_compress.cc")], check=True)
    L = ctypes.CDLL(so)
    L.lancet_emu_compress.restype = None
    return L


def run(L, g, seq_cap=None, len_max=None):
    n, order, rec, seq, seq_top, seq_cap, qv, len_max = pack(g, seq_cap, len_max)
    bw = 3 + n + n * (OUT_HEAD + len_max)
    out = np.zeros((5, bw), np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    L.lancet_emu_compress(ctypes.c_uint32(n), ctypes.c_uint32(len(order)), p(order), p(rec), p(seq), ctypes.c_uint32(seq_top), ctypes.c_uint32(seq_cap),
                          p(qv), ctypes.c_uint32(len(g.qv)), K, ctypes.c_uint32(len_max), p(out))
    res = []
    for b in out:
        m = int(b[2])
        res.append(dict(ovf=int(b[0]), aux=int(b[1]), order=b[3:3 + m].tolist(), rec=b[3 + n:].reshape(n, OUT_HEAD + len_max)))
    return res


def check(res, overflow=False, cmp_ok=1, ranked=1, drivers=(0, 1, 2, 3)):
    """every driver against the model; returns the model's block"""
    model = res[4]
    for d in drivers:
        r, name = res[d], DRIVERS[d]
        if d == 2 and not (cmp_ok and ranked):
            continue                                                        # (compress_rank stood aside: the graph is as it was, see the aux word below)
        assert r["ovf"] == int(overflow), name
        if overflow:
            continue
        assert model["ovf"] == 0
        assert r["order"] == model["order"], name
        dead = lambda x: [i for i, w in enumerate(x["rec"]) if w[0] & DEAD]
        assert dead(r) == dead(model), name
        for n in model["order"]:
            a, b = r["rec"][n], model["rec"][n]
            assert a[0] & 31 == b[0] & 31, (name, n, "flags")
            assert a[1:14].tolist() == b[1:14].tolist(), (name, n, "edges", [hex(x) for x in a[1:14]], [hex(x) for x in b[1:14]])
            assert a[14:18].tolist() == b[14:18].tolist(), (name, n, "cov", a[14:18].view(np.float32), b[14:18].view(np.float32))
            assert a[18:23].tolist() == b[18:23].tolist(), (name, n, "mincov mincovqv nkm nkmT length", a[18:23], b[18:23])
            assert a[OUT_HEAD:].tolist() == b[OUT_HEAD:].tolist(), (name, n, "descriptors")
    if 1 in drivers:
        assert res[1]["aux"] == cmp_ok
    if 2 in drivers:
        assert res[2]["aux"] == (3 if not cmp_ok else ranked), "compress_rank: 1 ranked, 0 declined and untouched, 2 declined but touched"
    return model


def length(model, n):
    return int(model["rec"][n][22])


# ---- the first compress: every node one k-mer

def test_chain_head_in_the_middle(rig):
    g = Graph()
    a = g.kmers(9, cov=[(1, 65535, 3, 7), (65535, 1, 2, 1), (3, 3, 65535, 0), (7, 2, 1, 65535), (1, 1, 1, 1), (40000, 3, 9, 2), (5, 50000, 7, 3), (2, 8, 4, 60000), (9, 9, 9, 9)])
    g.chain(a)
    g.order = [a[4], a[0], a[8], a[2], a[6], a[1], a[3], a[5], a[7]]     # the head is the table-first member: merges on its F, then on its R side
    m = check(run(rig, g))
    assert m["order"] == [a[4]] and length(m, a[4]) == K + 8


@pytest.mark.parametrize("dirs,order", [
    ([FF, FR, FF, FF, FF, FF], None), ([FF, FR, FF, FF, RF, FF], None), ([FR, FF, FF, FF, FF, FR], None),
    ([FF, FF, FF, FF, FF, FF], [6, 5, 4, 3, 2, 1, 0]),                    # entered from its R end
    ([FF, RF, FF, FR, FF, FF], [3, 0, 6, 1, 5, 2, 4]),
])
def test_chain_with_frame_flips(rig, dirs, order):
    g = Graph(seed=3)
    a = g.kmers(7)
    g.chain(a, dirs)
    if order:
        g.order = [a[i] for i in order]
    m = check(run(rig, g))
    assert len(m["order"]) == 1 and length(m, m["order"][0]) == K + 6


def test_ring_beside_a_chain(rig):
    g = Graph(seed=4)
    r = g.kmers(4); a = g.kmers(5)
    g.chain(r).link(r[3], r[0])
    g.chain(a)
    res = run(rig, g)
    m = check(res, ranked=0)                                                # compress_rank declines and touches nothing; compress_fast hands the ring to the literal loop
    assert m["order"] == [r[0], a[0]]
    assert m["rec"][r[0]][1] == 2 and all(int(e) & 0x0FFFFFFF == r[0] for e in m["rec"][r[0]][2:4])      # the ring ends as a node with an edge to itself


def test_self_loop_and_tandem_buddy(rig):
    g = Graph(seed=5)
    a = g.kmers(8)
    g.chain(a).link(a[3], a[3], FF)                                         # a[3] is a tandem: merging stops on both of its sides
    m = check(run(rig, g))
    assert m["order"] == [a[0], a[3], a[4]]


@pytest.mark.parametrize("dirs,head", [([FF, FF, FR, FF, FF], 2), ([FF, FR, FF, FF, FF], 0), ([FR, FF, FF, RF, FF], 0), ([FF, FR, FF, FR, FR], 4), ([FF, FF, FF, FF, FF], 5)])
def test_fork_at_both_ends(rig, dirs, head):
    """The head adopts the outward edges of the F-side end, then of the R-side end (erase / push_back order), flipped with the end's frame
    -- the parity of FR / RF links between the head and the end, wherever along the chain they stand; the neighbours' twins in place."""
    g = Graph(seed=6)
    a = g.kmers(6); f = g.kmers(2); b = g.kmers(2)
    g.order = [a[head]] + [x for x in a if x != a[head]] + f + b
    g.chain(a, dirs)
    if sum(d in (FR, RF) for d in dirs) % 2:
        g.link(a[5], f[0], RF, used=True).link(a[5], f[1], RR)             # a[5] is entered reversed: it is left through R
    else:
        g.link(a[5], f[0], FF, used=True).link(a[5], f[1], FR)
    g.link(b[0], a[0], FF).link(b[1], a[0], RF, used=True)
    m = check(run(rig, g))
    assert m["order"] == [a[head]] + f + b and m["rec"][a[head]][1] == 4


def test_far_end_points_back_at_the_head(rig):
    g = Graph(seed=7)
    a = g.kmers(4); x = g.kmers(1)
    g.chain(a).link(a[3], a[0], FF).link(a[3], x[0], FF)                   # arrives on the head's R side: the head becomes a tandem after the merge
    m = check(run(rig, g))
    h = m["rec"][a[0]]
    assert m["order"] == [a[0], x[0]] and any(int(e) & 0x0FFFFFFF == a[0] for e in h[2:2 + int(h[1])])


def test_thirteenth_edge(rig):
    g = Graph(seed=8)
    a = g.kmers(2); x = g.kmers(12)
    g.link(a[0], a[1], FF)
    for i in range(6):
        g.link(x[i], a[0], FF)                                              # six more edges on the head's R side,
        g.link(a[1], x[6 + i], FF)
    g.link(a[1], x[0], FR)                                                  # seven to adopt: 6 + 7 = 13
    res = run(rig, g)
    assert res[4]["ovf"] == 1
    check(res, overflow=True)


def test_source_and_sink_next_to_mergeable_nodes(rig):
    g = Graph(seed=9)
    s = g.special(SOURCE); a = g.kmers(6); t = g.special(SINK)
    g.chain(a).link(s, a[0], FF).link(a[5], t, FF)
    m = check(run(rig, g))
    assert m["order"] == [s, a[0], t] and length(m, a[0]) == K + 5


def test_second_component_and_dead_node(rig):
    g = Graph(seed=10)
    a = g.kmers(5); b = g.kmers(3, comp=2); d = g.kmers(1, flags=[DEAD | TUMOR])
    g.chain(a).chain(b)
    g.order = [b[0], a[0], d[0], a[1], b[1], a[2], a[3], b[2], a[4]]
    res = run(rig, g)
    for r in res:
        r["order"] = [n for n in r["order"] if n != d[0]]                   # (cleanDead drops the dead node from the table in some routes, compaction by marks in others: not compared)
        r["rec"][d[0]][0] |= DEAD
    m = check(res)
    assert m["order"] == [b[0], a[0], b[1], b[2]]


def test_irregular_link(rig):
    g = Graph(seed=11)
    a = g.kmers(5); x = g.kmers(1)
    g.chain(a[:3]).chain(a[3:])
    g.half_edge(a[2], a[3], FF).half_edge(a[3], x[0], RR).half_edge(x[0], a[3], FF)      # a[3]'s one edge in R goes elsewhere
    check(run(rig, g), cmp_ok=0)


def test_merge_order_of_the_coverages(rig):
    cov = [(1, 65535, 3, 7), (65535, 1, 7, 3), (3, 7, 1, 65535), (7, 3, 65535, 1), (0, 0, 0, 0), (11, 13, 17, 19), (65535, 65535, 1, 1), (2, 3, 5, 7), (1, 1, 1, 2)]
    for order in ([0, 1, 2, 3, 4, 5, 6, 7, 8], [8, 7, 6, 5, 4, 3, 2, 1, 0], [3, 5, 1, 7, 0, 8, 2, 6, 4]):
        g = Graph(seed=12)
        a = g.kmers(9, cov=cov)
        g.chain(a)
        g.order = [a[i] for i in order]
        m = check(run(rig, g))
        assert len(m["order"]) == 1


# ---- later compresses: unitigs (compress_prepare finds no first compress: cmp_ok = 0, the literal route)

@pytest.mark.parametrize("blen", [K, K + 63, K + 64, K + 70])              # the lane-strided loop's one-trip and two-trip edges
@pytest.mark.parametrize("link", [FF, FR, RR, RF])                         # dir F and R, brev off and on
def test_unitig_merge(rig, blen, link):
    g = Graph(seed=20 + blen).with_ghosts(200)
    h = g.unitig(30, room=(90, 90)); b = g.unitig(blen, flags=NORMAL, cov=(0.5, 7.25, 1.0, 3.0), weak_last=True)
    x = g.kmers(2, table=False); g.order += x
    g.link(h, b, link)
    g.link(b, x[0], FF if link in (FF, RF) else RF).link(b, x[1], FR if link in (FF, RF) else RR)
    m = check(run(rig, g), cmp_ok=0)
    assert m["order"] == [h] + x and length(m, h) == 30 + blen - (K - 1)


@pytest.mark.parametrize("link", [FF, RR])
def test_deque_without_room_moves(rig, link):
    g = Graph(seed=30).with_ghosts(200)
    h = g.unitig(40, room=(3, 3)); b = g.unitig(80)
    g.link(h, b, link)
    m = check(run(rig, g), cmp_ok=0)
    assert m["order"] == [h] and length(m, h) == 40 + 80 - (K - 1)


def test_arena_too_small_for_the_move(rig):
    g = Graph(seed=31).with_ghosts(200)
    h = g.unitig(40, room=(3, 3)); b = g.unitig(80)
    g.link(h, b, FF)
    check(run(rig, g, seq_cap=len(g.seq) + 100, len_max=200), overflow=True, cmp_ok=0)      # the move needs 2 * (40 + 76) + 16 slots


def test_three_unitigs_in_one_call(rig):
    g = Graph(seed=32).with_ghosts(300)
    u = [g.unitig(70, room=(10, 10)), g.unitig(20), g.unitig(90, weak_last=True)]
    g.order = [u[1], u[0], u[2]]
    g.chain(u, [FR, FF])
    m = check(run(rig, g), cmp_ok=0)
    assert m["order"] == [u[1]] and length(m, u[1]) == 70 + 20 + 90 - 2 * (K - 1)
