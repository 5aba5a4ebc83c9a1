"""The three per-component cleaning passes alone and without a GPU: remove_low_cov_wg, remove_tips_wg and remove_short_links_wg of kernels.h
(pass_candidates_wg, clean_dead_flags_wg and compress_wg under them), which state Graph_t::removeLowCov(true, comp), removeTips and
removeShortLinks (reference src/Graph.cc:2768-2926), run on hand-made graphs (clean_cases.py) -- each pass alone from the same start state and
the three in process_window's order -- beside a plain model of the reference lines (tests/emu/emu_graph_model.h), in the single-wave build and in
the re-run tier's (-DLANCET_FAT=1).

Every case states its outcome (what each pass reports, which nodes it leaves dead); that is asserted on the model before the kernels are looked
at.  findTandems is not modelled a third time: the model takes its answer per node from the oracle's findTandems, and a case that is about
an STR states the answer, which is held against the oracle's first.

Per case and pass, kernel against model, exact and whole: the live table order, the dead set, per live node the edge words, every descriptor,
cov[4] by bit pattern, mincov, mincovqv, nkm, nkmT and the flags; the counts the passes report (found, tips per round, rounds, links); the
overflow flag."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import clean_cases as cc
from emu_graph import DEAD, OUT_HEAD, SINK, SOURCE, pack
from oracle import oracle

PASSES = ["lowcov", "tips", "links", "sequence"]
IP = ["totalreadbp", "reflen", "low_cov_threshold", "max_tip_len", "max_unit_len", "min_report_units", "min_report_len", "dist_from_str", "path_cap", "comp", "precompress"]
CNT_WORDS = 16
PRE_LINKS, START = 8, 9


_BUILT = {}                                                        # (one compile per build, however pytest orders the parameters)


@pytest.fixture(scope="module", params=["plain", "fat"])
def rig(request, tmp_path_factory):
    if request.param in _BUILT:
        return _BUILT[request.param]
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
    so = os.path.join(str(tmp_path_factory.mktemp("emu_clean_" + request.param)), "libemu_clean.so")
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-strict-aliasing", "-w"]
    cmd += ["-DLANCET_FAT=1"] if request.param == "fat" else []
    header = os.environ.get("LANCET_EMU_KERNELS_H")                # (to hold the rig against another revision of the headers)
    cmd += ['-DLANCET_EMU_KERNELS_H="%s"' % header] if header else []
    subprocess.run(cmd + ["-o", so, os.path.join(here, "emu_clean.cc")], check=True)
    # A pass that loses count of its list walks off it: every case once in a child process first, so that such a kernel fails here, within a
    # time limit, and is never called in this process.
    child = "import sys; sys.path.insert(0, %r); import test_clean_passes_emu as t; t.every_case_once(%r)" % (os.path.dirname(os.path.abspath(__file__)), so)
    done = subprocess.run([sys.executable, "-c", child], timeout=60, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert done.returncode == 0, "the rig did not get through its cases in a child process"
    _BUILT[request.param] = load(so)
    return _BUILT[request.param]


def load(so):
    L = ctypes.CDLL(so)
    L.lancet_emu_clean.restype = None
    return L


def every_case_once(so):
    L = load(so)
    for name in sorted(cc.CASES):
        run(L, cc.CASES[name]())
    for M in cc.GROUP_SIZES:
        run(L, cc.group_case(M, "every_second"))
        run(L, cc.group_case_linked(M))


def call(L, g, packed, in_str, in_str_seq):
    n, order, rec, seq, seq_top, seq_cap, qv, len_max = packed
    s = g.settings
    ip = np.asarray([s[k] for k in IP], np.int32)
    bw = 3 + n + n * (OUT_HEAD + len_max)
    out = np.zeros((10, bw), np.uint32)
    cnt = np.zeros((10, CNT_WORDS), np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    L.lancet_emu_clean(ctypes.c_uint32(n), ctypes.c_uint32(len(order)), p(order), p(rec), p(seq), ctypes.c_uint32(seq_top), ctypes.c_uint32(seq_cap),
                       p(qv), ctypes.c_uint32(len(g.qv)), ctypes.c_int(g.K), ctypes.c_uint32(len_max), p(ip), ctypes.c_double(s["min_cov_ratio"]),
                       p(in_str), p(in_str_seq), p(out), p(cnt))
    res = []
    for b, c in zip(out, cnt):
        m = int(b[2])
        rounds = int(c[2])
        res.append(dict(ovf=int(b[0]), order=b[3:3 + m].tolist(), rec=b[3 + n:].reshape(n, OUT_HEAD + len_max),
                        found=int(c[0]), links=int(c[1]), tips=c[3:3 + rounds].tolist(), rounds_in_order=int(c[CNT_WORDS - 1]) == 0))
    return res


def strings_in_an_str(g, block):
    """the oracle's findTandems over position K - 1, for the string of every live node of the block that has one"""
    s = g.settings
    flags = np.zeros(len(g.rec), np.uint8)
    for n in block["order"]:
        w = block["rec"][n]
        if w[0] & (SOURCE | SINK):
            continue
        text = "".join("ACGT"[int(d) & 3] for d in w[OUT_HEAD:OUT_HEAD + int(w[22])])
        flags[n] = oracle.find_tandems(text, g.K - 1, s["max_unit_len"], s["min_report_units"], s["min_report_len"], s["dist_from_str"])[0]
    return flags


def run(L, g):
    s = g.settings
    for n, stated in g.stated_str.items():                                  # the case's statement first, on the string the case wrote
        assert oracle.find_tandems(g.string(n), g.K - 1, s["max_unit_len"], s["min_report_units"], s["min_report_len"], s["dist_from_str"])[0] == stated, (n, g.string(n))
    packed = pack(g, len_max=g.len_max)
    none = np.zeros(len(g.rec), np.uint8)
    res = call(L, g, packed, none, none)
    if res[START]["ovf"] or res[PRE_LINKS]["ovf"]:
        return res
    in_str, in_str_seq = strings_in_an_str(g, res[START]), strings_in_an_str(g, res[PRE_LINKS])
    for n, stated in g.stated_str.items():
        assert bool(in_str[n]) == stated
    if in_str.any() or in_str_seq.any():
        res = call(L, g, packed, in_str, in_str_seq)
    return res


def dead(block, g):
    return {n for n in g.order if block["rec"][n][0] & DEAD}


def counts(block):
    return dict(found=block["found"], tips=block["tips"], links=block["links"])


def check_model(res, g):
    """the case's statement, on the model alone"""
    start = res[START]
    assert start["ovf"] == 0
    absorbed = dead(start, g)                                               # (by the first compress, where the case asks for one)
    for i, name in enumerate(PASSES[:3]):
        m = res[4 + i]
        assert m["ovf"] == int(name in g.expect_overflow), name
        if m["ovf"]:
            continue
        want, gone = g.expect[name]
        assert (m["tips"] if name == "tips" else m["found"] if name == "lowcov" else m["links"]) == want, (name, counts(m))
        assert dead(m, g) == set(gone) | absorbed, (name, dead(m, g), gone)
        assert m["order"] == [n for n in start["order"] if n not in gone], name      # the start order without the dead nodes
        if name in g.untouched:
            assert gone == set() and m["order"] == start["order"] and np.array_equal(m["rec"], start["rec"]), name
        # a pass alone reports nothing of the others
        assert (m["found"] == -1) == (name != "lowcov") and (m["links"] == -1) == (name != "links") and (m["tips"] == []) == (name != "tips"), (name, counts(m))
    m = res[7]
    assert m["ovf"] == int(bool(g.expect_overflow))
    if g.expect_seq is not None:
        assert (m["found"], m["tips"], m["links"]) == tuple(g.expect_seq), counts(m)
    if g.untouched == set(PASSES[:3]):
        assert m["order"] == start["order"] and np.array_equal(m["rec"], start["rec"])


def check_kernels(res, g):
    """every pass of kernels.h against the model's"""
    for i, name in enumerate(PASSES):
        k, m = res[i], res[4 + i]
        assert k["ovf"] == m["ovf"], name
        assert k["rounds_in_order"], name
        if m["ovf"]:
            continue
        assert counts(k) == counts(m), name
        assert k["order"] == m["order"], name
        assert dead(k, g) == dead(m, g), name
        live = np.asarray(m["order"], np.int64)
        a, b = k["rec"][live], m["rec"][live]
        if np.array_equal(a[:, 1:23], b[:, 1:23]) and np.array_equal(a[:, OUT_HEAD:], b[:, OUT_HEAD:]) and np.array_equal(a[:, 0] & 31, b[:, 0] & 31):
            continue
        for n, x, y in zip(live, a, b):                                     # (say where)
            assert x[0] & 31 == y[0] & 31, (name, n, "flags")
            assert x[1:14].tolist() == y[1:14].tolist(), (name, n, "edges", [hex(v) for v in x[1:14]], [hex(v) for v in y[1:14]])
            assert x[14:18].tolist() == y[14:18].tolist(), (name, n, "cov", x[14:18].view(np.float32), y[14:18].view(np.float32))
            assert x[18:23].tolist() == y[18:23].tolist(), (name, n, "mincov mincovqv nkm nkmT length", x[18:23], y[18:23])
            assert x[OUT_HEAD:].tolist() == y[OUT_HEAD:].tolist(), (name, n, "descriptors")


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_case(rig, name):
    g = cc.CASES[name]()
    res = run(rig, g)
    check_model(res, g)
    check_kernels(res, g)


@pytest.mark.parametrize("pattern", cc.GROUP_PATTERNS)
@pytest.mark.parametrize("rig,M", [("plain", M) for M in cc.GROUP_SIZES] + [("fat", M) for M in cc.GROUP_SIZES + cc.GROUP_SIZES_FAT], indirect=["rig"])
def test_group_edges_of_the_compaction(rig, M, pattern):
    g = cc.group_case(M, pattern)
    assert len(g.order) == M
    res = run(rig, g)
    check_model(res, g)
    check_kernels(res, g)
    gone = g.expect["lowcov"][1]
    for i in (0, 1, 3):                                                     # after the pass the table order is the start order without the dead nodes
        assert res[i]["order"] == [n for n in g.order if n not in gone], PASSES[i]


@pytest.mark.parametrize("rig,M", [("plain", M) for M in cc.GROUP_SIZES] + [("fat", M) for M in cc.GROUP_SIZES + cc.GROUP_SIZES_FAT], indirect=["rig"])
def test_group_edges_with_short_links(rig, M):
    g = cc.group_case_linked(M)
    assert len(g.order) == M
    res = run(rig, g)
    check_model(res, g)
    check_kernels(res, g)


def test_the_cases_cover_what_they_claim():
    """the shapes the issue names are in the list, with the outcomes that make them what they are"""
    rounds = {name: len(cc.CASES[name]().expect["tips"][0]) for name in cc.CASES if name.startswith("tips_")}
    assert {3, 4, 5} <= set(rounds.values())                                # two, three and four rounds that remove, then one that does not
    assert cc.CASES["tips_y_stem_first"]().expect["tips"][0] == [2, 1, 0] and cc.CASES["tips_y_stem_last"]().expect["tips"][0] == [3, 0]
    assert {11, 12, 13} == {cc.CASES[n]().K for n in cc.CASES if n.startswith("links_length_")}
    assert {4, 11, 19} == {cc.CASES[n]().settings["max_tip_len"] for n in cc.CASES if n.startswith("tips_length_")}
