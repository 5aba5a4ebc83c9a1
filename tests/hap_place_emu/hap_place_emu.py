"""TEST INFRASTRUCTURE ONLY -- loader for tests/hap_place_emu/libemu.so (and libemu_fat.so): tests/hap_sup_emu's library with the emulated
placement kernel behind the windows and the support kernel (see emu_hap_place.cc).  The library exports everything tests/emu/libemu.so
does and is named like it, so tests/emu/emu.py drives it: run() puts it in emu's place for the length of one run and then fetches
haplotypes, CIGARs, support counts and the reads' placement records.  hand() runs the placement kernel over one hand-written window."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

from lancet_amd import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "emu"))
import emu  # noqa: E402

_LIBS = {}
_U32P = C.POINTER(C.c_uint32)
_U16P = C.POINTER(C.c_uint16)
_PLP = C.POINTER(abi.LancetReadPlacement)


def lib():
    """The library of the form emu.FAT selects, set up as emu.lib() sets up its own."""
    fat = bool(emu.FAT[0])
    if fat not in _LIBS:
        saved, here = dict(emu._LIBS), emu._HERE
        try:                                                   # emu.lib() builds, loads and declares the emulator's entry points: here, from this directory
            emu._LIBS.pop(fat, None)
            emu._HERE = _HERE
            L = emu.lib()
        finally:
            emu._HERE = here
            emu._LIBS.clear()
            emu._LIBS.update(saved)
        L.lancet_happlace_emu_set.argtypes = [C.c_uint32] + [C.c_int] * 7
        L.lancet_happlace_emu_results.argtypes = [C.POINTER(C.POINTER(abi.LancetHaplotype)), _U32P, C.POINTER(_U32P), _U32P, C.POINTER(C.POINTER(C.c_uint8))]
        L.lancet_happlace_emu_cigars.argtypes = [C.POINTER(_U32P), C.POINTER(_U32P), _U32P]
        L.lancet_happlace_emu_support.argtypes = [C.POINTER(_U32P)]
        L.lancet_happlace_emu_raw.argtypes = [C.POINTER(_U32P), C.POINTER(_U32P)]
        L.lancet_happlace_emu_raw.restype = C.c_uint32
        L.lancet_happlace_emu_placements.argtypes = [C.POINTER(_PLP), _U32P, C.POINTER(_U32P), C.POINTER(_U16P)]
        L.lancet_happlace_emu_hand.argtypes = [_U32P, C.c_uint32, C.c_uint32, _U32P, _U32P, _U32P, C.c_uint32, C.c_uint32, _PLP, _U16P]
        L.lancet_happlace_emu_read_cigar.argtypes = [C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, _U32P, C.c_uint32, _U32P, _U32P, C.c_uint32, _U32P]
        L.lancet_happlace_emu_struct_size.restype = C.c_uint32
        L.lancet_happlace_emu_consts.argtypes = [C.c_uint32 * 6]
        _LIBS[fat] = L
    return _LIBS[fat]


def consts() -> dict:
    """What the emulated kernel was compiled with."""
    out = (C.c_uint32 * 6)()
    lib().lancet_happlace_emu_consts(out)
    return dict(zip(("ents", "stage", "count_max", "waves", "idx_max", "min_words"), (int(x) for x in out)))


def set_switches(words_per_window: int, place, mm, max_indel_len: int = 500) -> int:
    """The return code of the set call (capture without its other switches)."""
    return int(lib().lancet_happlace_emu_set(words_per_window, 0, 0, 0, 5, place, mm, max_indel_len))


LAST_RAW = [None]      # (length words, buffers as [n_windows, cap]) of the last run with the capture on


def run(batch, params=None, evt_cap: int = 0, hap_words: int = 0, aln: bool = False, sup: bool = False, sup_mm: int = 5, place: bool = True, mm: int = 5):
    """(variants, stats, trace text, haplotypes, truncated, placements): emu.run's three, abi.haplotypes_to_py's dicts -- each with "cigar"
    when aln and "support" when sup -- the per-window marks and abi.placements_to_py's (records, read_begin, tlen)."""
    L = lib()
    fat = bool(emu.FAT[0])
    rc = L.lancet_happlace_emu_set(hap_words, 1 if aln else 0, 0, 1 if sup else 0, sup_mm, 1 if place else 0, mm, int(params.max_indel_len) if params is not None else 500)
    assert rc == 0, rc
    saved = emu._LIBS.get(fat)
    emu._LIBS[fat] = L
    try:
        v, st, text = emu.run(batch, params, evt_cap=evt_cap)
        hp, n, wp, nwd, tp = C.POINTER(abi.LancetHaplotype)(), C.c_uint32(), _U32P(), C.c_uint32(), C.POINTER(C.c_uint8)()
        assert L.lancet_happlace_emu_results(C.byref(hp), C.byref(n), C.byref(wp), C.byref(nwd), C.byref(tp)) == 0
        words = np.ctypeslib.as_array(wp, shape=(nwd.value,)).copy() if nwd.value else np.zeros(0, np.uint32)
        haps = abi.haplotypes_to_py(hp, n.value, words)
        if aln:
            op, cp, nc = _U32P(), _U32P(), C.c_uint32()
            assert L.lancet_happlace_emu_cigars(C.byref(op), C.byref(cp), C.byref(nc)) == 0
            for i, h in enumerate(haps):
                h["cigar"] = abi.cigar_to_py(cp[op[i]:op[i + 1]])
        if sup:
            sp = _U32P()
            assert L.lancet_happlace_emu_support(C.byref(sp)) == 0 and bool(sp) == bool(haps)
            for i, h in enumerate(haps):
                h["support"] = abi.support_to_py(sp[8 * i:8 * i + 8])
        trunc = [int(tp[w]) for w in range(batch.n_windows)]
        lp, bp = _U32P(), _U32P()
        cap = L.lancet_happlace_emu_raw(C.byref(lp), C.byref(bp))
        LAST_RAW[0] = None if not cap else (np.ctypeslib.as_array(lp, shape=(batch.n_windows,)).copy(),
                                            np.ctypeslib.as_array(bp, shape=(batch.n_windows, cap)).copy())
        pp, nr, rb, tl = _PLP(), C.c_uint32(), _U32P(), _U16P()
        assert L.lancet_happlace_emu_placements(C.byref(pp), C.byref(nr), C.byref(rb), C.byref(tl)) == 0
        assert place or not pp
        pl = abi.placements_to_py(pp, nr.value, rb, batch.n_windows, tl)
    finally:
        L.lancet_happlace_emu_set(0, 0, 0, 0, 0, 0, 0, 500)
        if saved is None:
            emu._LIBS.pop(fat, None)
        else:
            emu._LIBS[fat] = saved
    return v, st, text, haps, trunc, pl


def pack(seq: str) -> list:
    """A string over ACGT as the kernels' words: 2 bits per base, first base in the low bits."""
    words = [0] * ((len(seq) + 15) // 16)
    for i, c in enumerate(seq):
        words[i // 16] |= "ACGT".index(c) << (2 * (i % 16))
    return words


def hand(entries, reads, max_mm: int = 5, cap: int = None, len_word: int = None):
    """The placement kernel over one hand-written window.  entries: [(path string, k)] or [(path string, k, component)], laid out one behind
    the other as the window kernels lay them out (header, path words; no CIGAR, coverage or support words); reads: [(string, cls)], taken as
    trimmed.  cap / len_word: the buffer's size and the window's length word where they are not simply the entries' words.
    Returns (records, tlen) as numpy arrays."""
    L = lib()
    buf = []
    for e in entries:
        s, k, comp = (e + (0,))[:3]
        buf += [k | comp << 16, 0, len(s), len(s), 0, 0, 0, 0] + pack(s)
    used = len(buf)
    cap = used + 3 if cap is None else cap
    buf = (buf + [0xCDCDCDCD] * max(0, cap - used))[:max(cap, 1)]
    ri, bw, bases = [], [], []
    for s, cls in reads:
        ri.append(len(s) | (cls >> 1) << 16 | (cls & 1) << 17)
        bw.append(len(bases))
        bases += pack(s)
    bases += [0, 0]
    n = len(reads)
    out, tl = (abi.LancetReadPlacement * max(1, n))(), (C.c_uint16 * max(1, n))()
    arr = lambda x: (C.c_uint32 * max(1, len(x)))(*x)
    assert L.lancet_happlace_emu_hand(arr(buf), used if len_word is None else len_word, cap, arr(ri), arr(bw), arr(bases), n, max_mm, out, tl) == 0
    recs = np.frombuffer(bytes(out), dtype=abi.PLACEMENT_DTYPE)[:n].copy()
    return recs, np.array(list(tl)[:n], np.uint16)


_OPS = {0: "M", 1: "I", 2: "D", 4: "S"}
_HOPS = {"I": 1, "D": 2, "=": 7, "X": 8}


def read_cigar(o: int, t: int, length: int, ref_off: int, cigar) -> tuple:
    """lc_read_cigar (host_common.h) in abi.read_cigar's form: (start, [(n, op)], has_m)."""
    L = lib()
    cw = [n << 4 | _HOPS[op] for n, op in (cigar or [])]
    out, start, n_out = (C.c_uint32 * 64)(), C.c_uint32(), C.c_uint32()
    rc = L.lancet_happlace_emu_read_cigar(o, t, length, ref_off, (C.c_uint32 * max(1, len(cw)))(*cw), len(cw), C.byref(start), out, 64, C.byref(n_out))
    assert rc >= 0
    return int(start.value), [(int(out[i]) >> 4, _OPS[int(out[i]) & 15]) for i in range(n_out.value)], bool(rc)
