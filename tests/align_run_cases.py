"""The (S, T) pairs on which a traceback that consumes whole runs of cells (kernels.h align_traceback_runs: the diagonal between two
gaps, a gap being extended) can go wrong and at which tests/align_cases.py does not aim, shared by tests/test_align_runs_emu.py and
tests/test_align_runs_gpu.py.  Strings of at most 300 bases, drawn from fixed seeds; the expected rows are oracle.align's, asked once.
The oracle also decides, while the table is drawn, whether a pair shows what its family is about (a homopolymer next to an indel lets
the tie rules move the gap): a draw that does not is drawn again.

Families
  diag1  one single-base deletion / insertion, placed so that the walk's first run along the diagonal (from the end of the alignment
         to the gap) has exactly 1, 62, 63, 64, 65, 127, 128 or 129 cells: a run that ends with the last cell of a 64-cell fetch, a
         gap that is the first cell of a fresh one
  diag2  two single-base indels, the run between them of those lengths (the fetch behind a gap starts at the run's first cell).
         A run of 1 between two gaps is never the best alignment under the reference's scores (two gaps around one match: -9 - 9 + 2;
         one gap of two bases and a mismatch: -10 - 4; two mismatches where the gaps are opposite: -8), so the shortest run the
         scores leave stands in for it: 2 between two gaps of a kind, 3 between opposite ones
  gaprun one deletion / insertion of 1, 2, 63, 64, 65 bases: the lines fetched along a column / a row while a gap is extended
  turn   a deletion directly followed by an insertion, or the reverse, no diagonal cell between the two
  head   an indel at the head of the strings: the walk ends on a border (i == 0 with j > 0, j == 0 with i > 0)
  seam   n in 60..67, m in {n - 1, n, n + 1}: every residue of n + m modulo 4, a substitution in the first and in the last column
"""
import numpy as np

from oracle import oracle

RUNS = (1, 62, 63, 64, 65, 127, 128, 129)
GAPS = (1, 2, 63, 64, 65)
FAMILIES = ("diag1", "diag2", "gaprun", "turn", "head", "seam")
SINGLE_INDEL = ("diag1", "gaprun")            # one indel and nothing else: the band has to certify (nearly) all of them
MAX_BASES = 300


def _rs(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def _other(rng, ch):
    return "ACGT"[("ACGT".index(ch) + 1 + int(rng.integers(0, 3))) % 4]


def ops(a, b):
    """[(kind, length)] of the aligned rows, M / D (a base of S against '-') / I ('-' against a base of T), from the head."""
    out = []
    for x, y in zip(a, b):
        k = "I" if x == "-" else ("D" if y == "-" else "M")
        if out and out[-1][0] == k:
            out[-1][1] += 1
        else:
            out.append([k, 1])
    return [(k, r) for k, r in out]


def _draw(rng, make, want_ops):
    """A pair from make(rng) whose oracle alignment has the run-length shape want_ops (a predicate on ops())."""
    for _ in range(200):
        s, t = make(rng)
        al = oracle.align(s, t)
        if al is not None and want_ops(ops(*al)):
            return s, t
    raise AssertionError("no draw with the intended alignment in 200 tries")


def _indel(rng, s, p, kind, size=1):
    """s with `size` bases taken out at p (D) or `size` random bases put in before p (I)."""
    return s[:p] + s[p + size:] if kind == "D" else s[:p] + _rs(rng, size) + s[p:]


def _diag1(rng):
    out = []
    for r in RUNS:
        for kind in ("D", "I"):
            def make(rng, r=r, kind=kind):
                s = _rs(rng, r + 1 + int(rng.integers(20, 60)))
                return s, _indel(rng, s, len(s) - r - (1 if kind == "D" else 0), kind)
            s, t = _draw(rng, make, lambda o, r=r, kind=kind: len(o) == 3 and o[1] == (kind, 1) and o[2] == ("M", r))
            out.append((f"diag1/{kind}_run{r}", s, t))
    return out


def diag2_shortest(k1, k2):
    return 2 if k1 == k2 else 3


def _diag2(rng):
    out = []
    for r0 in RUNS:
        for k1 in ("D", "I"):            # the gap nearer the end of the strings (the walk meets it first)
            for k2 in ("D", "I"):
                r = r0 if r0 > 1 else diag2_shortest(k1, k2)
                def make(rng, r=r, k1=k1, k2=k2):
                    tail = int(rng.integers(3, 12))
                    s = _rs(rng, int(rng.integers(20, 60)) + 1 + r + 1 + tail)
                    p1 = len(s) - tail - (1 if k1 == "D" else 0)
                    p2 = p1 - r - (1 if k2 == "D" else 0)
                    return s, _indel(rng, _indel(rng, s, p1, k1), p2, k2)
                s, t = _draw(rng, make, lambda o, r=r, k1=k1, k2=k2: len(o) == 5 and o[1] == (k2, 1) and o[2] == ("M", r) and o[3] == (k1, 1))
                out.append((f"diag2/{k2}{k1}_run{r}", s, t))
    return out


def _gaprun(rng):
    out = []
    for g in GAPS:
        for kind in ("D", "I"):
            def make(rng, g=g, kind=kind):
                s = _rs(rng, int(rng.integers(150, 220)) + (g if kind == "D" else 0))
                return s, _indel(rng, s, int(rng.integers(40, 100)), kind, g)
            s, t = _draw(rng, make, lambda o, g=g, kind=kind: len(o) == 3 and o[1] == (kind, g))
            out.append((f"gaprun/{kind}{g}", s, t))
    return out


def _turn(rng):
    """A stretch of S replaced by unrelated bases, long enough that two gaps beat the mismatches (-4 a column against -8 - length a gap);
    the tie rules decide which gap comes first, so the draws are sorted by what the oracle answered and both orders are asked for."""
    out = []
    need = {("D", "I"): 4, ("I", "D"): 4}
    k = 0
    for _ in range(400):
        if not any(need.values()):
            break
        s = _rs(rng, int(rng.integers(120, 200)))
        p, a, b = int(rng.integers(30, 80)), int(rng.integers(10, 40)), int(rng.integers(10, 40))
        t = s[:p] + _rs(rng, b) + s[p + a:]
        al = oracle.align(s, t)
        if al is None:
            continue
        o = ops(*al)
        for x in range(len(o) - 1):
            key = (o[x][0], o[x + 1][0])
            if key in need and need[key] > 0:
                need[key] -= 1
                out.append((f"turn/{key[0]}{key[1]}_{k}", s, t))
                k += 1
                break
    return out, need


def _head(rng):
    out = []
    for g in (1, 5, 30):
        for kind in ("D", "I"):
            def make(rng, g=g, kind=kind):
                s = _rs(rng, int(rng.integers(80, 160)))
                return s, (s[g:] if kind == "D" else _rs(rng, g) + s)
            s, t = _draw(rng, make, lambda o, g=g, kind=kind: len(o) == 2 and o[0] == (kind, g))
            out.append((f"head/{kind}{g}", s, t))
    return out


def _seam(rng):
    out = []
    for n in range(60, 68):
        for dm in (-1, 0, 1):
            def make(rng, n=n, dm=dm):
                s = _rs(rng, n)
                t = list(s)
                t[0] = _other(rng, t[0]); t[-1] = _other(rng, t[-1])
                p = int(rng.integers(20, 40))
                if dm < 0:
                    del t[p]
                elif dm > 0:
                    t[p:p] = [_rs(rng, 1)]
                return s, "".join(t)
            want = {-1: ["M", "D", "M"], 0: ["M"], 1: ["M", "I", "M"]}[dm]
            s, t = _draw(rng, make, lambda o, want=want: [k for k, _ in o] == want)
            out.append((f"seam/n{n}_m{n + dm}", s, t))
    return out


_CASES = None
TURN_MISSING = {}


def cases():
    """[(id, S, T)]"""
    global _CASES
    if _CASES is None:
        out = []
        for k, fam in enumerate((_diag1, _diag2, _gaprun, _turn, _head, _seam)):
            got = fam(np.random.default_rng(9300 + k))
            if fam is _turn:
                got, need = got
                TURN_MISSING.update({"".join(key): v for key, v in need.items() if v})
            out += got
        ids = [c[0] for c in out]
        assert len(set(ids)) == len(ids)
        assert all(1 <= len(s) <= MAX_BASES and 1 <= len(t) <= MAX_BASES for _, s, t in out)
        _CASES = out
    return _CASES


def family(cid):
    return cid.split("/", 1)[0]


_EXPECTED = None


def expected():
    """{id: oracle.align(S, T)}, asked once (every pair of the table has an alignment: the draw kept only such pairs)."""
    global _EXPECTED
    if _EXPECTED is None:
        _EXPECTED = {cid: oracle.align(s, t) for cid, s, t in cases()}
        assert all(v is not None for v in _EXPECTED.values())
    return _EXPECTED
