"""TEST INFRASTRUCTURE ONLY -- loader for tests/select_emu/libemu_select.so (the device read selection's rules and planning, lanes run
one after the other on the host; see emu_select.cc)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from lancet_amd import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
_ARRAYS = (("summaries", 0, np.uint32), ("kept", 1, np.int32), ("chr_id", 2, np.int32), ("ref_start", 3, np.int32), ("ref_off", 4, np.uint32),
           ("ref_codes", 5, np.uint8), ("read_begin", 6, np.uint32), ("rinfo", 7, np.uint32), ("name_rank", 8, np.uint32),
           ("base_woff", 9, np.uint32), ("good_woff", 10, np.uint32))


def lib():
    global _LIB
    if _LIB is None:
        subprocess.run(["make", "-s", "-C", _HERE, "all"], check=True)
        L = C.CDLL(os.path.join(_HERE, "libemu_select.so"))
        L.lancet_select_emu.restype = C.c_void_p
        L.lancet_select_emu.argtypes = [C.POINTER(abi.LancetAlignmentTable), C.POINTER(abi.LancetWindowSlice), C.c_void_p, C.c_uint32, C.c_uint32]
        L.lancet_select_emu_free.argtypes = [C.c_void_p]
        L.lancet_select_emu_rc.argtypes = [C.c_void_p]
        L.lancet_select_emu_reason.restype = C.c_char_p
        L.lancet_select_emu_reason.argtypes = [C.c_void_p]
        L.lancet_select_emu_need_large.argtypes = [C.c_void_p]
        L.lancet_select_emu_array.restype = C.c_void_p
        L.lancet_select_emu_array.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
        _LIB = L
    return _LIB


def caps():
    """(reads of one window the second pass stages, evidence counters of one window)"""
    a, b = C.c_int(), C.c_int()
    lib().lancet_select_emu_caps(C.byref(a), C.byref(b))
    return a.value, b.value


def run(table, slice_, opts, lds_reads: int = 512, lds_bases: int = 32768) -> dict:
    """What lancet_engine_upload_windows would leave on the device: dict(rc, reason, need_large, summaries [n, 6], kept, chr_id, ref_start,
    ref_off, ref_codes, read_begin, rinfo, name_rank, base_woff, good_woff).  rc 1 = not taken (reason says why; only summaries may be set)."""
    L = lib()
    h = L.lancet_select_emu(C.byref(table), C.byref(slice_), C.addressof(opts), lds_reads, lds_bases)
    try:
        out = dict(rc=int(L.lancet_select_emu_rc(h)), reason=L.lancet_select_emu_reason(h).decode(), need_large=int(L.lancet_select_emu_need_large(h)))
        for name, which, dt in _ARRAYS:
            nb = C.c_uint64()
            p = L.lancet_select_emu_array(h, which, C.byref(nb))
            out[name] = np.frombuffer(C.string_at(p, nb.value), dtype=dt).copy() if nb.value else np.zeros(0, dtype=dt)
        out["summaries"] = out["summaries"].reshape(-1, 6)
    finally:
        L.lancet_select_emu_free(h)
    return out
