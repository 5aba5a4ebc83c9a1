"""TEST INFRASTRUCTURE ONLY -- loader for tests/hap_emu/libemu.so (and libemu_fat.so): the host emulation of the kernels (tests/emu) with the haplotype
capture around it (see emu_hap.cc).  The library exports everything tests/emu/libemu.so does and is named like it, so tests/emu/emu.py drives it: run() puts it
in emu's place for the length of one run and then fetches the haplotypes."""
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
        L.lancet_hap_emu_set.argtypes = [C.c_uint32]
        L.lancet_hap_emu_results.argtypes = [C.POINTER(C.POINTER(abi.LancetHaplotype)), C.POINTER(C.c_uint32), C.POINTER(C.POINTER(C.c_uint32)),
                                             C.POINTER(C.c_uint32), C.POINTER(C.POINTER(C.c_uint8))]
        L.lancet_hap_emu_struct_size.restype = C.c_uint32
        _LIBS[fat] = L
    return _LIBS[fat]


def set_words(words_per_window: int) -> int:
    """lancet_engine_set_haplotypes' return code."""
    return int(lib().lancet_hap_emu_set(words_per_window))


def run(batch, params=None, evt_cap: int = 0, hap_words: int = 0):
    """(variants, stats, trace text, haplotypes, truncated): emu.run's three, abi.haplotypes_to_py's dicts and the per-window marks."""
    L = lib()
    fat = bool(emu.FAT[0])
    rc = L.lancet_hap_emu_set(hap_words)
    assert rc == 0, rc
    saved = emu._LIBS.get(fat)
    emu._LIBS[fat] = L
    try:
        v, st, text = emu.run(batch, params, evt_cap=evt_cap)
        hp, n, wp, nwd, tp = C.POINTER(abi.LancetHaplotype)(), C.c_uint32(), C.POINTER(C.c_uint32)(), C.c_uint32(), C.POINTER(C.c_uint8)()
        assert L.lancet_hap_emu_results(C.byref(hp), C.byref(n), C.byref(wp), C.byref(nwd), C.byref(tp)) == 0
        words = np.ctypeslib.as_array(wp, shape=(nwd.value,)).copy() if nwd.value else np.zeros(0, np.uint32)
        haps = abi.haplotypes_to_py(hp, n.value, words)
        assert sum(h["n_words"] for h in haps) == nwd.value
        trunc = [int(tp[w]) for w in range(batch.n_windows)]
    finally:
        L.lancet_hap_emu_set(0)
        if saved is None:
            emu._LIBS.pop(fat, None)
        else:
            emu._LIBS[fat] = saved
    return v, st, text, haps, trunc
