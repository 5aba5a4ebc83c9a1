"""TEST INFRASTRUCTURE ONLY -- loader for tests/settle_emu/libemu.so (and libemu_fat.so): the host emulation of the kernels with the haplotype
capture (tests/hap_emu) plus the read-back of the windows the build kernel settled (see emu_settle.cc).  The library exports everything
tests/hap_emu's does and is named like it, so hap_emu.run drives it: run() puts it in hap_emu's place for the length of one run, with
LANCET_EMU_SETTLE in the environment as asked, and then fetches the settled windows."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "emu"))
sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "hap_emu"))
import emu  # noqa: E402
import hap_emu  # noqa: E402

_LIBS = {}
LAST_SETTLED = []            # windows of the last run that the build kernel settled
LAST_WHY = []                # per window of the last run: why the build kernel turned it away (build_lds.h BLW_*), 0 where it built it
LIMIT_NAMES = ("gmax", "cap", "st_fixed", "scap", "ccap", "ncap", "maxw", "rmax", "qvcap", "qvcap_wide", "wide_table_from")


def lib():
    """The library of the form emu.FAT selects, set up as hap_emu.lib() sets up its own."""
    fat = bool(emu.FAT[0])
    if fat not in _LIBS:
        saved, here = dict(hap_emu._LIBS), hap_emu._HERE
        try:                                                   # hap_emu.lib() builds, loads and declares the entry points: here, from this directory
            hap_emu._LIBS.pop(fat, None)
            hap_emu._HERE = _HERE
            L = hap_emu.lib()
        finally:
            hap_emu._HERE = here
            hap_emu._LIBS.clear()
            hap_emu._LIBS.update(saved)
        L.lancet_settle_emu_flags.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.lancet_settle_emu_why.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.lancet_settle_emu_limits.argtypes = [C.c_int, C.c_void_p, C.c_int]
        _LIBS[fat] = L
    return _LIBS[fat]


def limits(large: bool = False):
    """The sizes the settled test is written for, as the headers have them (emu_settle.cc lancet_settle_emu_limits): a dict over LIMIT_NAMES for
    the 512-lane form or, with large, the 1024-lane form."""
    buf = np.zeros(len(LIMIT_NAMES), np.uint32)
    n = int(lib().lancet_settle_emu_limits(1 if large else 0, buf.ctypes.data_as(C.c_void_p), len(buf)))
    assert n == len(LIMIT_NAMES), n
    return {k: int(v) for k, v in zip(LIMIT_NAMES, buf)}


def run(batch, params=None, settle: bool = True, evt_cap: int = 0, hap_words: int = 0, pre_order: bool = False):
    """(variants, stats, trace text, haplotypes, settled windows): hap_emu.run's first four and the sorted list of the windows settled."""
    L = lib()
    fat = bool(emu.FAT[0])
    got = {}
    free = L.lancet_emu_free

    class _Spy:                                                # the run's handle is freed inside emu.run: the flags are read just before
        def __getattr__(self, name):
            return getattr(L, name)

        def lancet_emu_free(self, h):
            buf = np.zeros(max(1, batch.n_windows), np.uint8)
            n = int(L.lancet_settle_emu_flags(C.c_void_p(h), buf.ctypes.data_as(C.c_void_p), len(buf)))
            got["n"], got["flags"] = n, buf
            why = np.zeros(max(1, batch.n_windows), np.uint32)
            got["why"] = why if int(L.lancet_settle_emu_why(C.c_void_p(h), why.ctypes.data_as(C.c_void_p), len(why))) >= 0 else None
            free(h)

    spy = _Spy()
    saved_lib = hap_emu._LIBS.get(fat)
    saved_env = os.environ.get("LANCET_EMU_SETTLE")
    hap_emu._LIBS[fat] = spy
    os.environ["LANCET_EMU_SETTLE"] = "1" if settle else "0"
    try:
        if pre_order:
            rc = L.lancet_hap_emu_set(hap_words)
            assert rc == 0, rc
            savede = emu._LIBS.get(fat)
            emu._LIBS[fat] = spy
            try:
                v, st, text = emu.run(batch, params, evt_cap=evt_cap, pre_order=True)
            finally:
                L.lancet_hap_emu_set(0)
                if savede is None:
                    emu._LIBS.pop(fat, None)
                else:
                    emu._LIBS[fat] = savede
            haps = []
        else:
            v, st, text, haps, _trunc = hap_emu.run(batch, params, evt_cap=evt_cap, hap_words=hap_words)
    finally:
        if saved_env is None:
            os.environ.pop("LANCET_EMU_SETTLE", None)
        else:
            os.environ["LANCET_EMU_SETTLE"] = saved_env
        if saved_lib is None:
            hap_emu._LIBS.pop(fat, None)
        else:
            hap_emu._LIBS[fat] = saved_lib
    n = got.get("n", -6)
    LAST_SETTLED[:] = [w for w in range(batch.n_windows) if n >= 0 and got["flags"][w]]
    assert n < 0 or n == len(LAST_SETTLED), (n, len(LAST_SETTLED))
    LAST_WHY[:] = [int(x) for x in got["why"][:batch.n_windows]] if got.get("why") is not None else []
    return v, st, text, haps, list(LAST_SETTLED)
