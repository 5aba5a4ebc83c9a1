"""TEST INFRASTRUCTURE ONLY -- loader for tests/hap_evid_emu/libemu.so (and libemu_fat.so): tests/hap_sup_emu's library with the emulated
evidence kernel behind the windows and the support kernel (see emu_hap_evid.cc).  The library exports everything tests/emu/libemu.so
does and is named like it, so tests/emu/emu.py drives it: run() puts it in emu's place for the length of one run and then fetches
haplotypes, CIGARs, support counts and the events' records.  hand() runs the evidence kernel over one hand-written window."""
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
_EVP = C.POINTER(abi.LancetVariantEvidence)
_HOPS = {"I": 1, "D": 2, "=": 7, "X": 8}


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
        L.lancet_hapevid_emu_set.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int]
        L.lancet_hapevid_emu_results.argtypes = [C.POINTER(C.POINTER(abi.LancetHaplotype)), _U32P, C.POINTER(_U32P), _U32P, C.POINTER(C.POINTER(C.c_uint8))]
        L.lancet_hapevid_emu_cigars.argtypes = [C.POINTER(_U32P), C.POINTER(_U32P), _U32P]
        L.lancet_hapevid_emu_support.argtypes = [C.POINTER(_U32P)]
        L.lancet_hapevid_emu_evidence.argtypes = [C.POINTER(_EVP), _U32P, C.POINTER(_U32P), C.POINTER(C.POINTER(C.c_uint8))]
        L.lancet_hapevid_emu_hand.argtypes = [_U32P, C.c_uint32, C.c_uint32, _U32P, _U32P, _U32P, C.c_uint32, C.c_uint32, C.c_uint32, _EVP, C.c_uint32, _U32P, _U32P, C.c_uint32, _U32P]
        L.lancet_hapevid_emu_join.argtypes = [C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_int32]
        L.lancet_hapevid_emu_struct_size.restype = C.c_uint32
        L.lancet_hapevid_emu_consts.argtypes = [C.c_uint32 * 5]
        _LIBS[fat] = L
    return _LIBS[fat]


def consts() -> dict:
    """What the emulated kernel was compiled with."""
    out = (C.c_uint32 * 5)()
    lib().lancet_hapevid_emu_consts(out)
    return dict(zip(("ents", "events", "pool", "waves", "words"), (int(x) for x in out)))


def set_switches(words_per_window: int, evid, mm, max_indel_len: int = 500) -> int:
    """The return code of the set call (capture with its alignments, without its other switches)."""
    return int(lib().lancet_hapevid_emu_set(words_per_window, 1, 0, 5, evid, mm, max_indel_len))


def run(batch, params=None, evt_cap: int = 0, hap_words: int = 0, aln: bool = True, sup: bool = False, sup_mm: int = 5, evid: int = 64, mm: int = 5):
    """(variants, stats, trace text, haplotypes, truncated, marked): emu.run's three, abi.haplotypes_to_py's dicts -- each with "cigar" when
    aln, "support" when sup and "events" when evid -- and the two per-window marks."""
    L = lib()
    fat = bool(emu.FAT[0])
    rc = L.lancet_hapevid_emu_set(hap_words, 1 if aln else 0, 1 if sup else 0, sup_mm, evid, mm, int(params.max_indel_len) if params is not None else 500)
    assert rc == 0, rc
    saved = emu._LIBS.get(fat)
    emu._LIBS[fat] = L
    try:
        v, st, text = emu.run(batch, params, evt_cap=evt_cap)
        hp, n, wp, nwd, tp = C.POINTER(abi.LancetHaplotype)(), C.c_uint32(), _U32P(), C.c_uint32(), C.POINTER(C.c_uint8)()
        assert L.lancet_hapevid_emu_results(C.byref(hp), C.byref(n), C.byref(wp), C.byref(nwd), C.byref(tp)) == 0
        words = np.ctypeslib.as_array(wp, shape=(nwd.value,)).copy() if nwd.value else np.zeros(0, np.uint32)
        haps = abi.haplotypes_to_py(hp, n.value, words)
        if aln:
            op, cp, nc = _U32P(), _U32P(), C.c_uint32()
            assert L.lancet_hapevid_emu_cigars(C.byref(op), C.byref(cp), C.byref(nc)) == 0
            for i, h in enumerate(haps):
                h["cigar"] = abi.cigar_to_py(cp[op[i]:op[i + 1]])
        if sup:
            sp = _U32P()
            assert L.lancet_hapevid_emu_support(C.byref(sp)) == 0 and bool(sp) == bool(haps)
            for i, h in enumerate(haps):
                h["support"] = abi.support_to_py(sp[8 * i:8 * i + 8])
        trunc = [int(tp[w]) for w in range(batch.n_windows)]
        ep, ne, eo, mp = _EVP(), C.c_uint32(), _U32P(), C.POINTER(C.c_uint8)()
        assert L.lancet_hapevid_emu_evidence(C.byref(ep), C.byref(ne), C.byref(eo), C.byref(mp)) == 0
        assert (evid and aln) or not ep
        if evid:
            for h, evs in zip(haps, abi.evidence_to_py(ep, ne.value, eo, len(haps))):
                h["events"] = evs
        marked = [int(mp[w]) for w in range(batch.n_windows)] if hap_words else [0] * batch.n_windows
    finally:
        L.lancet_hapevid_emu_set(0, 0, 0, 0, 0, 0, 500)
        if saved is None:
            emu._LIBS.pop(fat, None)
        else:
            emu._LIBS[fat] = saved
    return v, st, text, haps, trunc, marked


def pack(seq: str) -> list:
    """A string over ACGT as the kernels' words: 2 bits per base, first base in the low bits."""
    words = [0] * ((len(seq) + 15) // 16)
    for i, c in enumerate(seq):
        words[i // 16] |= "ACGT".index(c) << (2 * (i % 16))
    return words


def hand(entries, reads, max_mm: int = 5, cap: int = 256, len_word: int = None):
    """The evidence kernel over one hand-written window.  entries: [(path string, k, component, [(n, op)])], laid out one behind the other as
    the window kernels lay them out with the alignments on (header, path words, CIGAR words); reads: [(string, cls)], taken as trimmed.
    cap: records kept; len_word: the window's length word where it is not simply the entries' words.
    Returns (events per whole entry, marked): abi.evidence_to_py's lists."""
    L = lib()
    buf = []
    for s, k, comp, cigar in entries:
        ref_len = sum(n for n, op in cigar if op != "I")
        buf += [k | comp << 16, 0, ref_len, len(s), 0, 0, 0, len(cigar)] + pack(s) + [n << 4 | _HOPS[op] for n, op in cigar]
    used = len(buf)
    ri, bw, bases = [], [], []
    for s, cls in reads:
        ri.append(len(s) | (cls >> 1) << 16 | (cls & 1) << 17)
        bw.append(len(bases))
        bases += pack(s)
    bases += [0, 0]
    arr = lambda x: (C.c_uint32 * max(1, len(x)))(*x)
    out_cap, off_cap = 4096, len(entries) + 2
    out, off, ne, nh = (abi.LancetVariantEvidence * out_cap)(), (C.c_uint32 * off_cap)(), C.c_uint32(), C.c_uint32()
    rc = L.lancet_hapevid_emu_hand(arr(buf), used if len_word is None else len_word, used, arr(ri), arr(bw), arr(bases), len(reads), max_mm, cap, out, out_cap,
                                   C.byref(ne), off, off_cap, C.byref(nh))
    assert rc >= 0, rc
    return abi.evidence_to_py(out, ne.value, off, nh.value), rc


def join(first_variant: int, n_variants: int, ref_off: int, rb: int, ref_start: int, seq_in_window: int, pos: int) -> bool:
    """lc_evid_join (host_common.h) over one record."""
    return lib().lancet_hapevid_emu_join(first_variant, n_variants, ref_off, rb, ref_start, seq_in_window, pos) == 0
