"""The --linked-reads replay alone and without a GPU: lr_node_replay (one lane, 16-bit fields: runs of fewer than 3 or more than 192
occurrences) and lr_replay_batches (the whole wave, 8-bit fields, LDS batches of up to 32 nodes and 192 staged occurrences, a 64-entry list
refill) of kernels.h run on hand-made csr runs (tests/emu/emu_lr_replay.cc), in the single-wave build and in the re-run tier's
(-DLANCET_FAT=1, 64-bit csr words), beside a plain model of the reference lines that shares no code with them.

The model (reference src/Graph.cc:239-317, src/Node.cc:30-118, 470-520), per node: four sets of barcode strings (sample x strand), three
haplotype counters per sample.  loadSequence visits the reads in order and a read's k-mers by offset; every visit of the node is an LR
event -- unless the node has the read's barcode in either set of the read's sample (hasBX), the barcode goes into the set of (sample,
strand) and the read's haplotype counter goes up; "null" is never stored, so a read without barcode adds its haplotype every time; the
reference pseudo-read (label REF) has no effect -- and, unless the occurrence is an overlapping mate's (csr state != 0) or the reference's,
a coverage event: the size of the set of (sample, strand) and the sample's three counters are stored (last writer wins), and haplotype h
"had grown" when the stored counter was below the current one.  At offset 0 the LR events of positions 0 and 1 both precede the coverage
events of positions 0 and 1.

Three drivers per node list -- lr_node_replay per node; lr_replay_batches over the list as build_gather and load_prebuilt_lr make it;
the same with every run reversed on arrival (EngineCaps::debug_stop = 141) -- each against the model, exactly: the ten values (and mincov,
their first four summed), the run as left in the csr (sorted by read and position, state and orientation bits kept) and each occurrence's
grown bits.  Nodes of 3..192 occurrences reach the wave in drivers 1 and 2; the others take the one-lane route there too, as at the call
sites.  Every case runs with its runs stored in visiting order and stored shuffled (the order in which the lanes' atomics arrive on the
device)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

T, N = 0, 1
FWD, REV = 0, 1
REF = -1                       # the reference pseudo-read in a case's occurrence lists (the window's last read)
COOP_MIN, COOP_MAX, COOP_SEGS = 3, 192, 32
DRIVERS = ["lr_node_replay", "lr_replay_batches", "lr_replay_batches_reversed"]
NODE_WORDS, OCC_WORDS = 12, 3


@pytest.fixture(scope="module", params=["plain", "fat"])
def rig(request, tmp_path_factory):
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
    so = os.path.join(str(tmp_path_factory.mktemp("emu_lr_replay_" + request.param)), "libemu_lr_replay.so")
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-strict-aliasing", "-w"]
    cmd += ["-DLANCET_FAT=1"] if request.param == "fat" else []
    header = os.environ.get("LANCET_EMU_KERNELS_H")                # (to hold the rig against another revision of the headers)
    cmd += ['-DLANCET_EMU_KERNELS_H="%s"' % header] if header else []
    subprocess.run(cmd + ["-o", so, os.path.join(here, "emu_lr_replay.cc")], check=True)
    L = ctypes.CDLL(so)
    L.lancet_emu_lr_replay.restype = None
    L.lancet_emu_lr_limits.restype = None
    lim = (ctypes.c_uint32 * 4)()
    L.lancet_emu_lr_limits(lim)
    assert tuple(lim) == (COOP_MIN, COOP_MAX, COOP_SEGS, 8 if request.param == "fat" else 4)      # the cases below are placed at these
    return L


# ---------------------------------------------------------------- a window's reads and its nodes' runs

class Win:
    def __init__(self, seed=0):
        self.rng = np.random.RandomState(seed)
        self.reads = []                                            # (sample, strand, barcode or "null", haplotype)
        self.nodes = []                                            # lists of (read, position, state) in visiting order
        self._bx = 0

    def read(self, sample=T, strand=FWD, bx="null", hp=0):
        self.reads.append((sample, strand, bx, hp))
        return len(self.reads) - 1

    def fresh_bx(self):
        self._bx += 1
        return "BX%05d" % self._bx

    def node(self, occs):
        self.nodes.append(list(occs))
        return len(self.nodes) - 1

    def fill(self, count, pool=None, null=0.0, samples=(T, N), strands=(FWD, REV), hps=(0, 1, 2), st=(0,), pos=(2, 90)):
        """count occurrences of new reads (one each, at a position past 1): barcodes fresh, or drawn from pool; a share without barcode"""
        out = []
        for _ in range(count):
            bx = "null" if self.rng.rand() < null else (self.fresh_bx() if pool is None else pool[self.rng.randint(len(pool))])
            r = self.read(samples[self.rng.randint(len(samples))], strands[self.rng.randint(len(strands))], bx, hps[self.rng.randint(len(hps))])
            out.append((r, int(self.rng.randint(pos[0], pos[1])), st[self.rng.randint(len(st))]))
        return out

    @property
    def refr(self):
        return len(self.reads)

    def runs(self):
        """the nodes' runs in visiting order, the reference pseudo-read as the window's last read"""
        out = []
        for occs in self.nodes:
            run = sorted((self.refr if r == REF else r, p, s) for r, p, s in occs)
            assert len({(r, p) for r, p, _ in run}) == len(run)
            out.append(run)
        return out


def model(win):
    """Per node: (the ten values, {(read, position): grown bits of a counted occurrence})."""
    res = []
    for run in win.runs():
        sets = {(s, d): set() for s in (T, N) for d in (FWD, REV)}
        hpc = {T: [0, 0, 0], N: [0, 0, 0]}
        cov = {(s, d): 0 for s in (T, N) for d in (FWD, REV)}
        hpw = {T: [0, 0, 0], N: [0, 0, 0]}
        grown = {}

        def lr_event(r):
            if r == win.refr:                                      # BX "null", label REF: neither set, neither counter
                return
            s, d, bx, hp = win.reads[r]
            if bx in sets[(s, FWD)] or bx in sets[(s, REV)]:       # Node_t::hasBX
                return
            if bx != "null":                                       # Node_t::addBX
                sets[(s, d)].add(bx)
            hpc[s][hp] += 1                                        # Node_t::addHP

        def cov_event(r, p, st):
            if r == win.refr or st != 0:                           # !isRef ; !isOvlMate
                return
            s, d, _, _ = win.reads[r]
            cov[(s, d)] = len(sets[(s, d)])                        # updateCovDistr(BXcnt(strand, sample))
            grown[(r, p)] = sum(1 << h for h in range(3) if hpw[s][h] < hpc[s][h])      # updateHPCovDistr
            hpw[s] = list(hpc[s])

        by_read = {}
        for r, p, st in run:
            by_read.setdefault(r, {})[p] = st
        for r in sorted(by_read):                                  # loadSequence per read, offsets in order
            at = by_read[r]
            for p in (0, 1):                                       # offset 0: u's and v's LR events ...
                if p in at:
                    lr_event(r)
            for p in (0, 1):                                       # ... then u's and v's coverage events
                if p in at:
                    cov_event(r, p, at[p])
            for p in sorted(q for q in at if q > 1):               # offset p - 1: v's LR event, v's coverage event
                lr_event(r)
                cov_event(r, p, at[p])
        vals = [cov[(T, FWD)], cov[(T, REV)], cov[(N, FWD)], cov[(N, REV)]] + hpw[T] + hpw[N]
        res.append((vals, grown))
    return res


def replay(L, win, arrival):
    """-> per driver: (per node (values, mincov, listed), per node the run as left: (read, position, state, grown, orientation))"""
    runs = win.runs()
    rng = np.random.RandomState(99)
    stored = []
    for i, run in enumerate(runs):
        if arrival == "shuffled":
            run = [run[j] for j in rng.permutation(len(run))]
        elif arrival == "as_given":
            run = [(win.refr if r == REF else r, p, s) for r, p, s in win.nodes[i]]
        stored.append(run)
    nocc = np.cumsum([0] + [len(r) for r in stored]).astype(np.uint32)
    flat = [o for r in stored for o in r]
    o_read = np.array([o[0] for o in flat], np.uint32); o_pos = np.array([o[1] for o in flat], np.uint32); o_st = np.array([o[2] for o in flat], np.uint32)
    names = sorted({bx for _, _, bx, _ in win.reads if bx != "null"})
    rank = {bx: i for i, bx in enumerate(names)}
    R = win.refr + 1
    rinfo = np.array([100 | s << 16 | d << 17 for s, d, _, _ in win.reads] + [100], np.uint32)
    bxr = np.array([0xFFFFFFFF if bx == "null" else rank[bx] for _, _, bx, _ in win.reads] + [0xFFFFFFFF], np.uint32)
    hp = np.array([h for _, _, _, h in win.reads] + [0], np.uint8)
    nn, total = len(runs), int(nocc[-1])
    BW = NODE_WORDS * nn + OCC_WORDS * total
    out = np.full(3 * BW, 0xDDDDDDDD, np.uint32)
    p = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
    L.lancet_emu_lr_replay(ctypes.c_uint32(nn), p(nocc, ctypes.c_uint32), p(o_read, ctypes.c_uint32), p(o_pos, ctypes.c_uint32), p(o_st, ctypes.c_uint32),
                           ctypes.c_uint32(R), p(rinfo, ctypes.c_uint32), p(bxr, ctypes.c_uint32), p(hp, ctypes.c_uint8), p(out, ctypes.c_uint32))
    res = []
    for d in range(3):
        blk = out[d * BW:(d + 1) * BW]
        nodes = [([int(x) for x in blk[NODE_WORDS * n:NODE_WORDS * n + 10]], int(blk[NODE_WORDS * n + 10]), int(blk[NODE_WORDS * n + 11])) for n in range(nn)]
        occ = blk[NODE_WORDS * nn:].reshape(total, OCC_WORDS)
        left = [[(int(r), int(q), int(w) & 3, (int(w) >> 8) & 7, (int(w) >> 16) & 1) for r, q, w in occ[int(nocc[n]):int(nocc[n + 1])]] for n in range(nn)]
        res.append((nodes, left))
    return res


def hold(L, win, arrivals=("sorted", "shuffled")):
    want = model(win)
    runs = win.runs()
    assert runs and all(runs)
    for arrival in arrivals:
        got = replay(L, win, arrival)
        for d, (nodes, left) in enumerate(got):
            for n, run in enumerate(runs):
                what = (DRIVERS[d], arrival, "node", n, "occurrences", len(run))
                vals, mincov, listed = nodes[n]
                if d > 0:
                    assert listed == int(COOP_MIN <= len(run) <= COOP_MAX), what
                assert vals == want[n][0], what
                assert mincov == sum(want[n][0][:4]), what
                assert left[n] == [(r, p, st, want[n][1].get((r, p), 0), (r + p) & 1) for r, p, st in run], what
    return want


# ---------------------------------------------------------------- the cases

COUNTS = [1, 2, 3, 4, 191, 192, 193]


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("barcodes", ["distinct", "three"])
def test_run_lengths(rig, count, barcodes):
    """the routes' limits from both sides: 2 | 3 and 192 | 193"""
    w = Win(count)
    w.node(w.fill(count, pool=None if barcodes == "distinct" else ["BXA", "BXB", "BXC"]))
    (vals, grown), = hold(rig, w)
    assert len(grown) == count
    if barcodes == "distinct":
        assert sum(vals[:4]) == count and sum(vals[4:]) == count   # every occurrence adds: a class's last writer sees the class whole
    else:
        assert 1 <= sum(vals[:4]) <= 6 and sum(vals[4:]) == sum(vals[:4])


@pytest.mark.parametrize("count", [2, 4, 8, 200])
def test_one_barcode_in_both_samples_and_on_both_strands(rig, count):
    """hasBX looks at both strands of ONE sample: the barcode is new to the other sample"""
    w = Win()
    classes = [(T, FWD), (N, REV), (T, REV), (N, FWD)]
    w.node([(w.read(*classes[i % 4], "BXSAME", i % 3), 5 + i % 7, 0) for i in range(count)])
    (vals, grown), = hold(rig, w)
    assert vals[:4] == [1, 0, 0, 1] and sum(vals[4:7]) == 1 and sum(vals[7:]) == 1
    assert sum(1 for g in grown.values() if g) == 2                # (the first occurrence of either sample adds, no other)


@pytest.mark.parametrize("count", [1, 2, 5, 200])
def test_all_reads_without_barcode(rig, count):
    """"null" is never stored: no barcode count, every occurrence adds its haplotype"""
    w = Win(3)
    w.node(w.fill(count, null=1.0))
    (vals, grown), = hold(rig, w)
    assert vals[:4] == [0, 0, 0, 0] and sum(vals[4:]) == count and all(grown.values())


@pytest.mark.parametrize("count", [2, 6, 60, 200])
def test_null_mixed_with_barcodes(rig, count):
    w = Win(4)
    w.node(w.fill(count, pool=["BXA", "BXB", "BXC"], null=0.5) + w.fill(1, null=1.0) + w.fill(1, pool=["BXA"]))
    (vals, grown), = hold(rig, w)
    assert 0 < sum(vals[:4]) < sum(vals[4:])


# a (position 0, position 1) pair of one read in one node: loadSequence's offset 0 makes both LR events before both coverage events.  With a
# barcode the second event never adds (the first one stored it); without one both add, and the pair's first coverage event sees both.
PAIRS = ["barcode", "null", "null_last", "null_then_2", "null_overlapping_mate", "null_second_not_counted", "null_first_not_counted", "null_twice"]


@pytest.mark.parametrize("around", [0, 3, 60, 195], ids=lambda a: "with_%d_others" % a)
@pytest.mark.parametrize("kind", PAIRS)
def test_pair_at_positions_0_and_1(rig, kind, around):
    w = Win(7)
    before = w.fill(around // 2, pool=["BXA", "BXB"], null=0.3, hps=(0,))
    bx = "BXPAIR" if kind == "barcode" else "null"
    r = w.read(N, REV, bx, 1)
    st0, st1 = {"null_overlapping_mate": (1, 1), "null_second_not_counted": (0, 2), "null_first_not_counted": (1, 0)}.get(kind, (0, 0))
    pair = [(r, 0, st0), (r, 1, st1)] + ([(r, 2, 0)] if kind == "null_then_2" else [])
    if kind == "null_twice":
        r2 = w.read(N, FWD, "null", 1)
        pair += [(r2, 0, 0), (r2, 1, 0)]
    after = [] if kind == "null_last" else w.fill(around - around // 2, pool=["BXA", "BXB"], null=0.3, hps=(0,))
    w.node(before + pair + after)
    (vals, grown), = hold(rig, w)
    run = w.runs()[0]
    if kind == "null_last":
        assert run[-2:] == [(r, 0, 0), (r, 1, 0)]
    if kind == "barcode":
        assert grown[(r, 0)] == 2 and grown[(r, 1)] == 0
    elif st0 == 0 and st1 == 0:
        assert grown[(r, 0)] == 2 and grown[(r, 1)] == 0           # (one event after the other: the second would have grown too)
    elif kind == "null_second_not_counted":
        assert grown == {**grown, (r, 0): 2} and (r, 1) not in grown
        if not after:
            assert vals[8] == 2                                    # the stored counter holds BOTH events of the pair
    elif kind == "null_first_not_counted":
        assert grown[(r, 1)] == 2 and (r, 0) not in grown
    else:
        assert (r, 0) not in grown and (r, 1) not in grown


def test_pair_alone_leaves_both_events_in_the_stored_counter(rig):
    """the pair's first occurrence is the node's last counted one: what it stores is the value the node keeps"""
    for extra in (0, 2, 200):
        w = Win(8)
        r = w.read(T, FWD, "null", 2)
        w.node(w.fill(extra, samples=(N,), pool=["BXA"]) + [(r, 0, 0), (r, 1, 1)])
        (vals, _), = hold(rig, w)
        assert vals[4:7] == [0, 0, 2]


@pytest.mark.parametrize("count,cls", [(128, 0), (150, 1), (192, 2), (192, 3)])
def test_more_than_127_barcodes_in_one_class_wave_route(rig, count, cls):
    w = Win(9)
    w.node(w.fill(count, samples=(cls >> 1,), strands=(cls & 1,)) + w.fill(COOP_MAX - count, pool=["BXA", "BXB"]))
    (vals, _), = hold(rig, w)
    assert len(w.nodes[0]) == COOP_MAX and vals[cls] >= count > 127 and max(vals[4:]) > 42


@pytest.mark.parametrize("cls", [0, 3])
def test_more_than_255_barcodes_in_one_class_lane_route(rig, cls):
    w = Win(10)
    w.node(w.fill(300, samples=(cls >> 1,), strands=(cls & 1,), hps=(1,)))
    (vals, _), = hold(rig, w)
    assert vals[cls] == 300 and vals[4 + 3 * (cls >> 1) + 1] == 300


@pytest.mark.parametrize("count", [2, 6, 194])
@pytest.mark.parametrize("which", ["first", "last", "none"])
def test_few_counted_occurrences(rig, which, count):
    """overlapping mates make LR events and no coverage event: the one counted occurrence stores what the others added before it"""
    w = Win(11)
    occ = w.fill(count, pool=["BXA", "BXB", "BXC", "BXD"], null=0.2, st=(1, 2))
    if which != "none":
        i = 0 if which == "first" else count - 1
        occ[i] = (occ[i][0], occ[i][1], 0)
    w.node(occ)
    (vals, grown), = hold(rig, w)
    run = w.runs()[0]
    if which == "none":
        assert vals == [0] * 10 and not grown
    else:
        assert list(grown) == [run[0 if which == "first" else -1][:2]]
        s = w.reads[list(grown)[0][0]][0]
        assert sum(vals[4 + 3 * s:7 + 3 * s]) == (1 if which == "first" else sum(1 for r, _, _ in run if w.reads[r][0] == s and w.reads[r][2] == "null") +
                                                  len({w.reads[r][2] for r, _, _ in run if w.reads[r][0] == s and w.reads[r][2] != "null"}))


@pytest.mark.parametrize("count", [1, 2, 4, 194])
@pytest.mark.parametrize("ref_at", ["first", "middle", "last"])
def test_haplotypes_and_the_reference_pseudo_read(rig, ref_at, count):
    """HP 0, 1 and 2 of both samples; the reference pseudo-read has no effect wherever the csr pass left it in the run"""
    w = Win(12)
    occ = []
    for i in range(count - 1):
        occ.append((w.read((T, N)[i % 2], (FWD, REV)[(i // 2) % 2], w.fresh_bx() if i % 5 else "null", (i // 2) % 3), 3 + i % 11, 0))
    at = {"first": 0, "middle": len(occ) // 2, "last": len(occ)}[ref_at]
    occ.insert(at, (REF, 40, 0))
    w.node(occ)
    (vals, grown), = hold(rig, w, arrivals=("as_given", "sorted", "shuffled"))
    assert (w.refr, 40) not in grown and sum(vals[4:]) == count - 1
    if count >= 7:
        assert all(vals[4:])
    # without the pseudo-read: the same values
    w2 = Win(12)
    w2.reads = list(w.reads)
    w2.node([o for o in occ if o[0] != REF] or [(w2.read(), 9, 1)])
    if count > 1:
        assert model(w2)[0][0] == vals


def _small_nodes(w, sizes):
    for m in sizes:
        w.node(w.fill(m, pool=["BXA", "BXB", "BXC", "BXD", "BXE"], null=0.3, st=(0, 0, 0, 1)))


@pytest.mark.parametrize("name,sizes", [
    ("33_nodes_of_3", [3] * 33), ("64_nodes_of_3", [3] * 64),                                  # the 32-segment cut
    ("192_staged", [100, 92, 5]), ("193_staged", [100, 93, 5]), ("192_staged_by_3", [3] * 31 + [99, 4]),      # the cut at LR_COOP_MAX
    ("192_after_3", [3, 192, 3, 192]), ("192_twice", [192, 192]),
    ("one_lane_between", [3, 2, 193, 4, 1, 192, 3]),                                          # nodes the wave does not take, between listed ones
], ids=lambda x: x if isinstance(x, str) else "")
def test_batches(rig, name, sizes):
    w = Win(len(sizes))
    _small_nodes(w, sizes)
    want = hold(rig, w)
    assert len(want) == len(sizes) and any(any(v[0]) for v in want)


@pytest.mark.parametrize("listed", [63, 64, 65, 80, 130])
def test_list_refills(rig, listed):
    """the list reaches LDS 64 entries at a time, again when fewer than 16 are left: batches of 32 three-occurrence nodes, of ~10 larger ones
    and of single 192-occurrence nodes move the cursor across the refill points differently"""
    for seed, sizes in enumerate(([3] * listed, [3 + (7 * i) % 40 for i in range(listed)], [(192 if i % 9 == 8 else 3 + i % 5) for i in range(listed)])):
        w = Win(100 + seed)
        _small_nodes(w, sizes)
        assert len(hold(rig, w, arrivals=("sorted",) if seed else ("sorted", "shuffled"))) == listed


def test_random_nodes(rig):
    """40 nodes over small pools: 1..6 barcodes, 40 % null, random state bits, reads that meet a node at several positions (0 and 1 among them)"""
    rng = np.random.RandomState(5)
    w = Win(5)
    pairs = 0
    for n in range(40):
        pool = ["BX%d" % i for i in range(int(rng.randint(1, 7)))]
        reads = [w.read(int(rng.randint(2)), int(rng.randint(2)), "null" if rng.rand() < 0.4 else pool[rng.randint(len(pool))], int(rng.randint(3))) for _ in range(int(rng.randint(1, 14)))]
        size = int(rng.randint(1, 30)) if n % 8 else int(rng.randint(193, 230))
        size = min(size, 4 * len(reads)) if n % 8 else size
        if n % 8 == 0:
            reads += [w.read(int(rng.randint(2)), int(rng.randint(2)), "null" if rng.rand() < 0.4 else pool[rng.randint(len(pool))], int(rng.randint(3))) for _ in range(60)]
        keys = set()
        while len(keys) < size:
            keys.add((reads[rng.randint(len(reads))], int(rng.randint(0, 4))))
        occ = [(r, p, int(rng.choice([0, 0, 0, 1, 2]))) for r, p in sorted(keys)]
        if rng.rand() < 0.3:
            occ.append((REF, int(rng.randint(0, 50)), 0))
        pairs += sum(1 for r, p in keys if p == 0 and (r, 1) in keys)
        w.node(occ)
    want = hold(rig, w)
    assert pairs > 20 and sum(1 for run in w.runs() if len(run) > COOP_MAX) == 5 and sum(1 for run in w.runs() if len(run) < COOP_MIN) >= 1
    assert any(g not in (0, 7) for _, grown in want for g in grown.values())
