"""Windows whose reference contains N, at the smallest shapes at which the LDS build kernel's handling of them can go wrong
(build_lds_impl.h: the N mask, the N nodes as out-of-band entries of the node table, their edges in the graph statistics, the reference
bookkeeping).  Shared by test_nref_lds_emu.py (both host builds of the kernels) and test_nref_lds_gpu.py (the device).

The checker is the oracle, which names k-mers by std::string and so handles N like the reference does (reference src/util.cc:204-217:
N <-> N under reverse complement, A < C < G < N < T); the reference's own output on N windows is tests/golden/nref.* and
tests/golden/recovery/rec_nref.*.  Every batch here has an N-free twin -- the same reads, every N replaced by the base the sequenced
genome has there -- that the LDS build kernel builds whole without this feature (twin()); the hand-made windows are drawn at 30x / 30x."""
from __future__ import annotations

import functools

import numpy as np

from lancet_amd import abi, frontend, synth, workload
from lancet_amd.frontend import FWD, NML, REV, TMR
from oracle import oracle

KEY = lambda s: (s["status"], s["final_k"], s["n_builds"], s["n_variants"], s["n_kmers"], s["max_nodes"])
K0 = 11                                   # default min_k: the k of a window's first graph unless its reference is a repeat there
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def rc(s: str) -> str:
    return "".join(_COMP[c] for c in reversed(s))


def _rand(rng, n: int) -> str:
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def assert_equal_to_oracle(got, want, what=""):
    """(records, stats, trace) of a run against the oracle's: records and statistics bit for bit, the -v trace by its digest (node
    counts, edge counts and the table order show there)."""
    import golden_util as gu
    (v, st, tr), (ov, ost, otr) = got, want
    bad = [(w, KEY(a), KEY(b)) for w, (a, b) in enumerate(zip(st, ost)) if KEY(a) != KEY(b)]
    assert not bad and len(st) == len(ost), (what, bad[:4])
    assert v == ov, what
    assert gu.digest_trace(tr) == gu.digest_trace(otr), what


# ---------------------------------------------------------------- hand-made windows

def _window(rng, w: int, ref: str, genome: str, cov: int = 30, read_len: int = 100, extra=()):
    """One window: `ref` (with N) is what the FASTA shows, `genome` (same length, no N) what was sequenced.  cov x tumour reads (half of
    them carry a substitution 40 bases from the window's middle, where no case puts its N) and cov x normal reads, all inside the window, all
    bases Q40.  extra: further (sequence, quality string, label) reads, appended to their sample."""
    L = len(ref)
    assert len(genome) == L and "N" not in genome
    at = L // 2 + 40
    hap = genome[:at] + "ACGT"[("ACGT".index(genome[at]) + 1) % 4] + genome[at + 1:]
    rl = min(read_len, L)
    n = max(4, cov * L // rl)
    per = {TMR: [], NML: []}
    for lab in (TMR, NML):
        for i in range(n):
            src = hap if (lab == TMR and i % 2 == 0) else genome
            a = int(rng.integers(0, L - rl + 1))
            if i < 2:
                a = 0 if i == 0 else L - rl                                   # (both window edges are covered)
            per[lab].append((src[a:a + rl], "I" * rl))
        per[lab] += [(s, q) for s, q, l in extra if l == lab]
    reads = []
    for lab in (TMR, NML):
        for i, (s, q) in enumerate(per[lab]):
            reads.append((f"{'T' if lab == TMR else 'N'}{i:05d}", s, q, lab, FWD if i & 1 else REV, 1 + (i & 1), True))
    start = 1000 + 2000 * w
    return frontend.Window(f"chr22:{start}-{start + L}", "chr22", start, start + L, ref), reads, genome


def _put(s: str, at: int, what: str) -> str:
    return s[:at] + what + s[at + len(what):]


def _runs_case(rng, w, run: int, at: int = 150, L: int = 300, genome_base=None):
    genome = _rand(rng, L)
    if genome_base is not None:
        genome = _put(genome, at, "".join(genome_base(genome[at + i]) for i in range(run)))
    return _window(rng, w, _put(genome, at, "N" * run), genome)


def _self_complementary(rng, w, L: int = 300, at: int = 140):
    """...s N rc(s)... with |s| = (K0 - 1) / 2: the k-mer of K0 bases around the N is its own reverse complement at odd k."""
    h = (K0 - 1) // 2
    genome = _rand(rng, L)
    s = genome[at:at + h]
    genome = _put(genome, at + h + 1, rc(s))
    ref = _put(genome, at + h, "N")
    assert ref[at:at + K0] == rc(ref[at:at + K0])
    return _window(rng, w, ref, genome)


def _inverted_repeat(rng, w, L: int = 300, a: int = 90, b: int = 200):
    """u N v at offset a and rc(v) N rc(u) at offset b: two N k-mers of K0 bases that are reverse complements of each other."""
    h = (K0 - 1) // 2
    genome = _rand(rng, L)
    x = genome[a:a + K0]
    genome = _put(genome, b, rc(x))
    ref = _put(_put(genome, a + h, "N"), b + h, "N")
    assert ref[a:a + K0] == rc(ref[b:b + K0])
    return _window(rng, w, ref, genome)


HAND = ["one", "run_k-1", "run_k", "run_k+1", "run_2k", "at_0", "at_last", "in_last_k", "two_ends", "self_rc", "inverted", "alias_A", "alias_other"]
# (graphs built, k of the last one).  One graph at K0, unless the N run makes the reference a repeat there: N equals N (reference
# src/util.cc:295-315), so a run of r N is an exact repeat of r - 1 bases one base on and, with the two mismatches isAlmostRepeat allows,
# a near-repeat of r + 1: the loop skips every k <= r.  The inverted repeat is a cycle at K0 (its node is met in both directions): that
# graph -- the one the case is about -- is rejected and a second one built at K0 + 2.
HAND_K = {name: (1, K0) for name in HAND}
HAND_K.update({"run_k": (1, K0 + 2), "run_k+1": (1, K0 + 2), "run_2k": (1, 2 * K0 + 1), "inverted": (2, K0 + 2)})


def _hand_draw(rng, w: int, name: str):
    if name == "one":
        return _runs_case(rng, w, 1)
    if name.startswith("run_"):
        return _runs_case(rng, w, {"k-1": K0 - 1, "k": K0, "k+1": K0 + 1, "2k": 2 * K0}[name[4:]])
    if name == "at_0":
        return _runs_case(rng, w, 1, at=0)
    if name == "at_last":
        return _runs_case(rng, w, 1, at=299)
    if name == "in_last_k":
        return _runs_case(rng, w, 2, at=300 - K0 + 3)
    if name == "two_ends":
        g = _rand(rng, 300)
        return _window(rng, w, _put(_put(_put(g, 0, "NN"), 298, "NN"), 120, "N"), g)
    if name == "self_rc":
        return _self_complementary(rng, w)
    if name == "inverted":
        return _inverted_repeat(rng, w)
    if name == "alias_A":                                             # the reads carry A where the reference shows N: the 2-bit image of every N k-mer is a read's k-mer
        g = _rand(rng, 300)
        g = _put(_put(_put(g, 100, "A"), 150, "AAA"), 220, "AAAAA")
        return _window(rng, w, _put(_put(_put(g, 100, "N"), 150, "NNN"), 220, "NNNNN"), g)
    assert name == "alias_other"                                      # ... and the other three bases there
    g = _rand(rng, 300)
    g = _put(_put(_put(g, 100, "C"), 150, "GTC"), 220, "T")
    return _window(rng, w, _put(_put(_put(g, 100, "N"), 150, "NNN"), 220, "N"), g)


def _draw_until(rng, draw, want=None):
    """Draws until the oracle builds want = (graphs, k of the last one) for the window -- one graph at any k when not given (a random
    300-base reference is a near-repeat at k = 11 now and then, and a graph can have a cycle: the cases aim at one k)."""
    for _ in range(400):
        m = draw(rng)
        _, ost, _ = oracle.run(frontend.build_batch([m[0]], [m[1]]), abi.default_params())
        if ost[0]["status"] == 0 and ((ost[0]["n_builds"], ost[0]["final_k"]) == want if want else ost[0]["n_builds"] == 1):
            return m
    raise AssertionError("no draw builds one graph at the k the case is about")


@functools.lru_cache(maxsize=None)
def hand_made():
    """(batch, twin batch): one window per name of HAND, with the graphs HAND_K[name] says."""
    rng = np.random.default_rng(2611)
    return _batches([_draw_until(rng, lambda r, w=w, name=name: _hand_draw(r, w, name), HAND_K[name]) for w, name in enumerate(HAND)])


def _batches(made):
    wins = [m[0] for m in made]
    twins = [frontend.Window(m[0].hdr, m[0].chrom, m[0].start, m[0].end, m[2]) for m in made]
    reads = [m[1] for m in made]
    return frontend.build_batch(wins, reads), frontend.build_batch(twins, reads)


@functools.lru_cache(maxsize=None)
def recovery_window():
    """(batch, twin) for -R: the reference shows N at x where the genome has C, and T at x + 3 where both samples have G.  One tumour read
    carries A at x (a sequencing error at full quality) and its G at x + 3 below MIN_QUAL_CALL: the k-mers of that read over both positions
    are tumour singletons -- donors -- and turning their low-quality base into T gives exactly the 2-bit image (N read as A) of the
    reference's N k-mers.  No node of the graph is that k-mer (the N nodes are their strings, and no read holds the image), so the pass
    must find no acceptor: the run with -R equals the run without it."""
    rng = np.random.default_rng(77)
    L, x = 300, 150
    def draw(r):
        genome = _put(_put(_rand(r, L), x, "C"), x + 3, "G")
        donor = _put(genome[x - 50:x + 50], 50, "A")
        m = _window(r, 0, _put(_put(genome, x, "N"), x + 3, "T"), genome, extra=[(donor, _put("I" * 100, 53, "+"), TMR)])
        return m[0], m[1], _put(genome, x + 3, "T")
    win, reads, twin_ref = _draw_until(rng, draw)
    return frontend.build_batch([win], [reads]), frontend.build_batch([frontend.Window(win.hdr, win.chrom, win.start, win.end, twin_ref)], [reads])


# ---------------------------------------------------------------- drawn batches (synth, with n_runs)

def _synth_batch(region: str, linked: bool = False, max_windows: int = 24, **kw):
    data = synth.make_tumor_normal(linked=linked, **kw)
    out = []
    for ref in (data["ref"], synth.make_tumor_normal(linked=linked, **{**kw, "n_runs": ()})["ref"]):
        windows = frontend.tile_region(ref, data["rname"], region)
        batch, _ = frontend.batch_from_sam(windows, synth.pairs_to_sorted_reads(data["tumor"]), synth.pairs_to_sorted_reads(data["normal"]), linked=linked)
        out.append(batch)
    # (the front end drops a window whose reference is a repeat at max_k, which an N can decide either way: the windows both have)
    both = [h for h in out[0].hdr if h in set(out[1].hdr)][:max_windows]
    if out[0].hdr == out[1].hdr:
        out = [workload.sub_batch(b, 0, len(both)) for b in out]
    else:                                                             # (short reads only: concat_batches carries no barcodes)
        assert not linked
        out = [workload.concat_batches([workload.sub_batch(b, b.hdr.index(h), b.hdr.index(h) + 1) for h in both]) for b in out]
    assert out[0].n_windows == out[1].n_windows >= 4 and out[0].n_reads == out[1].n_reads
    assert (out[0].ref_bases == ord("N")).any() and not (out[1].ref_bases == ord("N")).any()
    return out[0], out[1]


@functools.lru_cache(maxsize=None)
def climbing():
    """Tandem duplications next to N: k climbs through several graphs per window (graphs built ahead, the build service, Ref_t::seq
    trimmed by a rejected k and applied again to the next graph's reference bookkeeping)."""
    return _synth_batch("chr22:700-2600", ref_len=3400, cov_t=30, cov_n=30, ref_seed=75, tumor_seed=175, normal_seed=275, dup_prob=1.0,
                        somatic_every=350, germline_every=260, read_len=100, insert_mean=330.0, insert_sd=30.0,
                        n_runs=((905, 1), (1290, 3), (1513, 1), (1822, 9), (2204, 2), (2391, 1)))


@functools.lru_cache(maxsize=None)
def linked():
    """--linked-reads with N (barcodes, haplotypes: the replay over the tracked nodes' runs, where an N node has none)."""
    return _synth_batch("chr22:700-2200", linked=True, ref_len=3000, cov_t=30, cov_n=30, ref_seed=93, tumor_seed=193, normal_seed=293,
                        somatic_every=400, germline_every=300, read_len=120,
                        n_runs=((940, 1), (1312, 4), (1650, 1), (1905, 12)))


@functools.lru_cache(maxsize=None)
def deep_str():
    """STR-rich 100x / 40x with N: the 1024-lane configuration, k above 31 (keys of more than one word)."""
    return _synth_batch("chr22:800-1900", max_windows=8, ref_len=2800, cov_t=100, cov_n=40, ref_seed=41, tumor_seed=141, normal_seed=241,
                        str_fraction=0.3, lowcomplex_fraction=0.05, read_len=150,
                        n_runs=((1010, 1), (1333, 2), (1571, 1), (1702, 7)))


@functools.lru_cache(maxsize=None)
def many_reads():
    """One hand-made window of more than 512 reads (short reads at 30x / 30x of a 640-base window): the 1024-lane configuration."""
    rng = np.random.default_rng(513)
    def draw(r):
        g = _rand(r, 640)
        return _window(r, 0, _put(_put(_put(g, 200, "N"), 333, "NNN"), 500, "N" * (K0 - 1)), g, read_len=60)
    b, t = _batches([_draw_until(rng, draw)])
    assert b.n_reads > 512
    return b, t


@functools.lru_cache(maxsize=None)
def mixed():
    """N windows and ordinary ones in one batch."""
    plain = workload.make_scan_batch(6, 30, 30, seed=19)
    b, t = hand_made()
    pick = lambda x: workload.concat_batches([workload.sub_batch(plain, 0, 3), workload.sub_batch(x, 0, 4), workload.sub_batch(plain, 3, 6), workload.sub_batch(x, 8, 12)])
    return pick(b), pick(t)


@functools.lru_cache(maxsize=None)
def oracle_of(name: str, lr: bool = False):
    batch = {"hand": hand_made, "recovery": recovery_window, "climbing": climbing, "linked": linked, "deep_str": deep_str, "many_reads": many_reads,
             "mixed": mixed}[name]()[0]
    return oracle.run(batch, abi.default_params(lr_mode=1 if lr else 0), verbose=True)


def hand_preconditions():
    """What makes the hand-made windows tests of what they are named after, stated on the oracle's output and on the windows."""
    b, _ = hand_made()
    _, ost, _ = oracle_of("hand")
    assert [(s["status"], s["n_builds"], s["final_k"]) for s in ost] == [(0,) + HAND_K[name] for name in HAND]
    ref = lambda name: b.ref_bases[int(b.ref_off[HAND.index(name)]):int(b.ref_off[HAND.index(name) + 1])].tobytes().decode()
    assert ref("at_0")[0] == "N" and ref("at_last")[-1] == "N" and "N" in ref("in_last_k")[-K0:] and "N" not in ref("in_last_k")[:-K0]
    assert any(ref("self_rc")[i:i + K0] == rc(ref("self_rc")[i:i + K0]) for i in range(300 - K0 + 1))
    r = ref("inverted")
    nk = {r[i:i + K0]: i for i in range(300 - K0 + 1) if "N" in r[i:i + K0]}
    assert any(rc(x) in nk and nk[rc(x)] != i for x, i in nk.items())
