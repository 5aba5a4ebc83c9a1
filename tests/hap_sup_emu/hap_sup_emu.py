"""TEST INFRASTRUCTURE ONLY -- loader for tests/hap_sup_emu/libemu.so (and libemu_fat.so): the host emulation of the kernels (tests/emu) with the
haplotype capture and all its switches around it, and the emulated support kernel behind the windows (see emu_hap_sup.cc).  The library
exports everything tests/emu/libemu.so does and is named like it, so tests/emu/emu.py drives it: run() puts it in emu's place for the length
of one run and then fetches haplotypes, CIGARs, coverages and support counts."""
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
        L.lancet_hapsup_emu_set.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int]
        L.lancet_hapsup_emu_results.argtypes = [C.POINTER(C.POINTER(abi.LancetHaplotype)), _U32P, C.POINTER(_U32P), _U32P, C.POINTER(C.POINTER(C.c_uint8))]
        L.lancet_hapsup_emu_cigars.argtypes = [C.POINTER(_U32P), C.POINTER(_U32P), _U32P]
        L.lancet_hapsup_emu_coverage.argtypes = [C.POINTER(_U32P), C.POINTER(_U16P), _U32P]
        L.lancet_hapsup_emu_support.argtypes = [C.POINTER(_U32P)]
        L.lancet_hapsup_emu_raw.argtypes = [C.POINTER(_U32P), C.POINTER(_U32P)]
        L.lancet_hapsup_emu_raw.restype = C.c_uint32
        L.lancet_hapsup_emu_struct_size.restype = C.c_uint32
        L.lancet_hapsup_emu_flag.restype = C.c_uint32
        _LIBS[fat] = L
    return _LIBS[fat]


def set_switches(words_per_window: int, aln, cov, sup, mm) -> int:
    """The return code the set calls share."""
    return int(lib().lancet_hapsup_emu_set(words_per_window, aln, cov, sup, mm))


LAST_RAW = [None]      # (length words, buffers as [n_windows, cap]) of the last run with the capture on
LAST_NULL = [True]     # the support call of the last run returned NULL


def run(batch, params=None, evt_cap: int = 0, hap_words: int = 0, aln: bool = False, cov: bool = False, sup: bool = True, mm: int = 5):
    """(variants, stats, trace text, haplotypes, truncated): emu.run's three, abi.haplotypes_to_py's dicts -- each with "cigar" when aln,
    "cov" when cov and "support" when sup -- and the per-window marks."""
    L = lib()
    fat = bool(emu.FAT[0])
    rc = L.lancet_hapsup_emu_set(hap_words, 1 if aln else 0, 1 if cov else 0, 1 if sup else 0, mm)
    assert rc == 0, rc
    saved = emu._LIBS.get(fat)
    emu._LIBS[fat] = L
    try:
        v, st, text = emu.run(batch, params, evt_cap=evt_cap)
        hp, n, wp, nwd, tp = C.POINTER(abi.LancetHaplotype)(), C.c_uint32(), _U32P(), C.c_uint32(), C.POINTER(C.c_uint8)()
        assert L.lancet_hapsup_emu_results(C.byref(hp), C.byref(n), C.byref(wp), C.byref(nwd), C.byref(tp)) == 0
        words = np.ctypeslib.as_array(wp, shape=(nwd.value,)).copy() if nwd.value else np.zeros(0, np.uint32)
        haps = abi.haplotypes_to_py(hp, n.value, words)
        assert sum(h["n_words"] for h in haps) == nwd.value        # `words` stays dense: path words only
        op, cp, nc = _U32P(), _U32P(), C.c_uint32()
        assert L.lancet_hapsup_emu_cigars(C.byref(op), C.byref(cp), C.byref(nc)) == 0
        assert op[0] == 0 and op[n.value] == nc.value and (aln or nc.value == 0)
        if aln:
            for i, h in enumerate(haps):
                h["cigar"] = abi.cigar_to_py(cp[op[i]:op[i + 1]])
        vo, vp, nv = _U32P(), _U16P(), C.c_uint32()
        assert L.lancet_hapsup_emu_coverage(C.byref(vo), C.byref(vp), C.byref(nv)) == 0
        assert vo[0] == 0 and vo[n.value] == nv.value and (cov or nv.value == 0)
        if cov:
            vals = np.ctypeslib.as_array(vp, shape=(nv.value,)).copy() if nv.value else np.zeros(0, np.uint16)
            for i, h in enumerate(haps):
                h["cov"] = abi.coverage_to_py(vals[vo[i]:vo[i + 1]], h["len"], h["ref_len"])
        sp = _U32P()
        assert L.lancet_hapsup_emu_support(C.byref(sp)) == 0
        LAST_NULL[0] = not sp
        assert sup or not sp
        if sup:
            assert bool(sp) == bool(haps)
            for i, h in enumerate(haps):
                h["support"] = abi.support_to_py(sp[8 * i:8 * i + 8])
        trunc = [int(tp[w]) for w in range(batch.n_windows)]
        lp, bp = _U32P(), _U32P()
        cap = L.lancet_hapsup_emu_raw(C.byref(lp), C.byref(bp))
        LAST_RAW[0] = None if not cap else (np.ctypeslib.as_array(lp, shape=(batch.n_windows,)).copy(),
                                            np.ctypeslib.as_array(bp, shape=(batch.n_windows, cap)).copy())
    finally:
        L.lancet_hapsup_emu_set(0, 0, 0, 0, 0)
        if saved is None:
            emu._LIBS.pop(fat, None)
        else:
            emu._LIBS[fat] = saved
    return v, st, text, haps, trunc
