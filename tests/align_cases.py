"""The (S, T) pairs the alignment (global_align_aff, reference src/align.cc:235-364) is checked on where its kernels are most likely
to go wrong, shared by the CPU tests (oracle, emulator) and the GPU tests (the device forms of the fill and the traceback), and the
reader of tests/golden/align_edge_ref.tsv, which holds what the reference's own align.cc answers for each of them
(tools/make_align_golden.py).  A plain helper module: the table is drawn from fixed seeds, every pair has an id `family/name`.

Families
  len    length seams: n = 64 g - 1, 64 g, 64 g + 1 (row blocks of the systolic full-matrix fill, 64-cell fetches of the wave
         traceback, the last partial store of its notes), 640 -> 641 (the full matrix moves from registers to the work space), 1024
  str    homopolymer / STR expansion and contraction (units A, AC, ACG, AAT, ACGT, AAAC) at the head, in the interior and at the tail:
         many equally good alignments, decided by the reference's tie rules
  gap    one insertion or deletion of 8..400 bases at the head, in the middle, at the tail: gap runs around 64 cells, |m - n| around
         the limit of the band (111)
  edge   two opposite indels that take the best path w - 1, w, w + 1 and w + 2 diagonals off the corner diagonals: along the last lanes
         inside the band, its edge lane, and just outside (the band must refuse)
  tiny   n in {1, 2, 3}
  unrel  unrelated strings: the band must not certify; the only family where the reference's traceback may leave its matrix
  lowc   two-letter strings with many edits
"""
import hashlib
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "align_edge_ref.tsv")
FAMILIES = ("len", "str", "gap", "edge", "tiny", "unrel", "lowc")
UNDEFINED = "undefined"
# pairs the band must certify per family, on the emulator and on the device (90 % of what the emulated band certified on the first table
# of these families: 62, 108, 324), so that no test passes by refusing everything; the device decision must also equal the emulator's
CERTIFY_FLOOR = {"len": 55, "str": 97, "gap": 290}


def _rs(rng, n, alphabet="ACGT"):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), size=n))


def _other(rng, ch):
    return "ACGT"[("ACGT".index(ch) + 1 + int(rng.integers(0, 3))) % 4]


def _len_family(rng):
    out = []
    ns = [64 * g + d for g in range(1, 11) for d in (-1, 0, 1)] + [642, 1024]
    for n in ns:
        s = _rs(rng, n)
        # (a) substitutions only, one of them in the last row and one in the first: the alignment has exactly n columns
        t = list(s)
        for p in {0, n - 1, n // 2, int(rng.integers(0, n))}:
            t[p] = _other(rng, t[p])
        out.append((f"len/n{n}_sub", s, "".join(t)))
        # (b) one base more or less next to a seam: n + 1 columns, the path changes diagonal in the last row block
        p = max(1, n - 1 - int(rng.integers(0, 8)))
        t = s[:p] + (_other(rng, s[p]) if n % 2 else "") + s[p + (0 if n % 2 else 1):]
        out.append((f"len/n{n}_indel", s, t))
    return out


def _str_family(rng):
    out = []
    for unit in ("A", "AC", "ACG", "AAT", "ACGT", "AAAC"):
        u = len(unit)
        for where in ("head", "mid", "tail"):
            for sign in (+1, -1):
                for bases in (u, 16, 60):
                    dunits = max(1, bases // u)
                    r = 10 + dunits + int(rng.integers(0, 6))          # copies in S; T has r +- dunits (at least 4 stay)
                    fl, fr = int(rng.integers(120, 260)), int(rng.integers(120, 260))
                    left = "" if where == "head" else _rs(rng, fl)
                    right = "" if where == "tail" else _rs(rng, fr)
                    if where == "head":
                        right = _rs(rng, fl + fr)
                    if where == "tail":
                        left = _rs(rng, fl + fr)
                    s = left + unit * r + right
                    t = left + unit * (r + sign * dunits) + right
                    out.append((f"str/{unit}_{where}_{'exp' if sign > 0 else 'con'}{dunits}", s, t))
    return out


GAP_SIZES = (8, 12, 16, 24, 31, 32, 33, 48, 62, 63, 64, 65, 66, 80, 96, 100, 108, 109, 110, 111, 112, 113, 114, 127, 128, 129, 160, 200,
             256, 300, 350, 400)


def _gap_family(rng):
    out = []
    for size in GAP_SIZES:
        for where in ("head", "mid", "tail"):
            for kind in ("ins", "del"):
                for base in (200, 450, 600):
                    n = base + int(rng.integers(0, 40))
                    if kind == "del":
                        n = max(n, size + 60 + int(rng.integers(0, 40)))
                    s = _rs(rng, n)
                    p = {"head": 0, "mid": (n - (size if kind == "del" else 0)) // 2, "tail": n - (size if kind == "del" else 0)}[where]
                    t = s[:p] + _rs(rng, size) + s[p:] if kind == "ins" else s[:p] + s[p + size:]
                    out.append((f"gap/{kind}{size}_{where}_n{n}", s, t))
    return out


def _edge_family(rng):
    """T = S with x random bases put in at a third and y bases taken out at two thirds (up), or the other way round (down): the best
    path leaves the main diagonal by x offsets and comes back to offset d = x - y (resp. -x, y - x).  With w = (127 - |d|) / 2 the band
    holds the offsets [min(d, 0) - w, min(d, 0) - w + 127]."""
    out = []
    for d in (0, 20):
        w = (127 - d) // 2
        for direction in ("up", "down"):
            lo = -w if direction == "up" else -d - w             # up: m - n = d ; down: m - n = -d
            last = lo + 127 if direction == "up" else -lo         # how far from the main diagonal the band still reaches on that side
            for x in (last - 2, last - 1, last, last + 1, last + 2):
                for n in (420, 600):
                    n += int(rng.integers(0, 30))
                    s = _rs(rng, n)
                    y = x - d
                    a, b = n // 3, 2 * n // 3
                    if direction == "up":        # T longer by d
                        t = s[:a] + _rs(rng, x) + s[a:b] + s[b + y:]
                    else:                        # T shorter by d
                        t = s[:a] + s[a + x:b + x] + _rs(rng, y) + s[b + x:]
                    out.append((f"edge/d{d}_{direction}_x{x}_n{n}", s, t))
    return out


def _tiny_family(rng):
    out = []
    for s, t in (("A", "A"), ("A", "C"), ("A", "AA"), ("A", "ACGT"), ("AC", "AC"), ("AC", "A"), ("AC", "ACC"), ("AC", "GACGT"), ("ACG", "ACG"),
                 ("ACG", "AG"), ("ACG", "ACTG"), ("AAA", "AAAAAA"), ("ACG", "ACGACGACG"), ("G", "G" * 70), ("AC", "AC" * 40), ("ACG", "ACG" + "T" * 130)):
        out.append((f"tiny/{s}_{t if len(t) < 10 else len(t)}", s, t))
    for n in (1, 2, 3):
        s = _rs(rng, n)
        out.append((f"tiny/n{n}_m200", s, s + _rs(rng, 200 - n)))
    return out


def _unrel_family(rng):
    out = []
    for k, (n, m) in enumerate(((446, 151), (151, 446), (64, 64), (65, 63), (300, 300), (640, 640), (641, 600), (128, 900), (600, 40), (40, 600),
                                (200, 210), (500, 389), (389, 500), (90, 91), (1000, 300), (257, 255), (320, 640), (639, 641), (77, 400), (512, 512))):
        out.append((f"unrel/{k}_{n}x{m}", _rs(rng, n), _rs(rng, m)))
    return out


def _lowc_family(rng):
    out = []
    for k, (ab, n) in enumerate((("AC", 120), ("AT", 250), ("GT", 400), ("AG", 600), ("CT", 640), ("AC", 641), ("CG", 333), ("AT", 64), ("AC", 500), ("GT", 200))):
        s = _rs(rng, n, ab)
        t = list(s)
        for _ in range(n // 10):
            p = int(rng.integers(1, len(t) - 1))
            r = rng.random()
            if r < 0.4:
                t[p] = ab[1 - ab.index(t[p])]
            elif r < 0.7:
                t[p:p] = list(_rs(rng, int(rng.integers(1, 6)), ab))
            else:
                del t[p:p + int(rng.integers(1, 6))]
        out.append((f"lowc/{k}_{ab}{n}", s, "".join(t)))
    return out


_CASES = None


def cases():
    """[(id, S, T)], in the order of the fixture."""
    global _CASES
    if _CASES is None:
        out = []
        for k, fam in enumerate((_len_family, _str_family, _gap_family, _edge_family, _tiny_family, _unrel_family, _lowc_family)):
            out += fam(np.random.default_rng(7100 + k))
        ids = [c[0] for c in out]
        assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
        assert all(1 <= len(s) <= 1024 and len(t) >= 1 and set(s + t) <= set("ACGT") for _, s, t in out)
        _CASES = out
    return _CASES


def family(cid):
    return cid.split("/", 1)[0]


def by_family(fam):
    return [c for c in cases() if family(c[0]) == fam]


def pair_hash(s, t):
    return hashlib.sha1((s + "\t" + t).encode()).hexdigest()[:12]


# ---- the alignment as a run-length string of column kinds: M both characters, D a character of S against '-', I '-' against one of T
def encode_ops(a, b):
    assert len(a) == len(b)
    out, prev, run = [], None, 0
    for x, y in zip(a, b):
        k = "I" if x == "-" else ("D" if y == "-" else "M")
        if k == prev:
            run += 1
        else:
            if prev:
                out.append(f"{run}{prev}")
            prev, run = k, 1
    if prev:
        out.append(f"{run}{prev}")
    return "".join(out) or "-"


def decode_ops(ops, s, t):
    """The two aligned rows the op string stands for."""
    a, b, i, j, num = [], [], 0, 0, ""
    for ch in ("" if ops == "-" else ops):
        if ch.isdigit():
            num += ch
            continue
        r = int(num)
        num = ""
        if ch == "M":
            a.append(s[i:i + r]); b.append(t[j:j + r]); i += r; j += r
        elif ch == "D":
            a.append(s[i:i + r]); b.append("-" * r); i += r
        elif ch == "I":
            a.append("-" * r); b.append(t[j:j + r]); j += r
        else:
            raise ValueError(ops)
    return "".join(a), "".join(b)


_GOLDEN = None


def golden():
    """{id: (aligned S, aligned T) or UNDEFINED} from the fixture; checks that the table drawn here is the one the fixture was made from."""
    global _GOLDEN
    if _GOLDEN is None:
        rows = {}
        with open(FIXTURE) as fh:
            for line in fh:
                cid, n, m, h, ops = line.rstrip("\n").split("\t")
                rows[cid] = (int(n), int(m), h, ops)
        out = {}
        cs = cases()
        assert len(rows) == len(cs), (len(rows), len(cs))
        for cid, s, t in cs:
            n, m, h, ops = rows[cid]
            assert (n, m, h) == (len(s), len(t), pair_hash(s, t)), f"{cid}: the generator no longer draws the pair the fixture was made from"
            if ops == UNDEFINED:
                out[cid] = UNDEFINED
            else:
                a, b = decode_ops(ops, s, t)
                assert a.replace("-", "") == s and b.replace("-", "") == t and len(a) == len(b), cid
                out[cid] = (a, b)
        _GOLDEN = out
    return _GOLDEN


REFUSED = "refused"


def emu_align(L, s, t, mode):
    """lancet_emu_align of an emulator build L (tests/emu): the aligned rows, None (mode 2: the band did not certify itself),
    UNDEFINED (the reference's traceback leaves its matrix) or REFUSED (a string too long for the hook)."""
    import ctypes
    f = L.lancet_emu_align
    f.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    f.restype = ctypes.c_int
    cap = len(s) + len(t) + 8
    a, b = ctypes.create_string_buffer(cap), ctypes.create_string_buffer(cap)
    r = f(s.encode(), t.encode(), a, b, cap, mode)
    if r < 0:
        return {-1: UNDEFINED, -2: None, -3: REFUSED}[r]
    return a.value.decode(), b.value.decode()
