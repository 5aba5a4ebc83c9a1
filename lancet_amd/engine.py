"""Python binding of the C-ABI in include/lancet_engine.h (ctypes; plain pointers only).

`Engine` is the drop-in for the reference seam `Microassembler::processGraph` (reference
src/Microassembler.cc:837) applied to a whole batch of windows; `VariantDB` is the host side below it
(reference src/VariantDB.cc).  There is no CPU fallback: a missing library or a missing GPU raises."""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np

from . import abi, trace as _trace

_LIBPATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "liblancet_engine.so")
_LIB = None

ERRORS = {0: "OK", -1: "bad argument", -2: "no HIP device", -3: "HIP error", -4: "unsupported", -5: "out of memory", -6: "bad state"}


PRE_ORDER_WORDS = 64 * (13 + 3 * 2048 + 2 * 834)      # room for Engine.pre_order: a chain of 64 graphs at the hand-off limits


def parse_pre_order(words):
    """The words of lancet_debug_pre_order (csrc/host_common.h lc_pre_order_words) as one dict per graph: K, built, N, nsurv, have_order,
    ht_bc, ht_next_resize, numcomp, refcomp, big, done, m_live, settled; with have_order `hashes` (uint64 per table position) and `comp`; with
    done `live_hashes` (the table after markRefEnds(1) and compress(1), special nodes included)."""
    import numpy as np
    graphs, at = [], 0
    names = ("K", "status", "N", "nsurv", "have_order", "ht_bc", "ht_next_resize", "numcomp", "refcomp", "big", "done", "m_live", "settled")
    while at < len(words):
        g = {k: int(v) for k, v in zip(names, words[at:at + 13])}
        g["built"] = g.pop("status") == 1
        at += 13
        if g["have_order"]:
            rows = np.asarray(words[at:at + 3 * g["nsurv"]], dtype=np.uint64).reshape(g["nsurv"], 3)
            g["hashes"] = rows[:, 0] | (rows[:, 1] << np.uint64(32))
            g["comp"] = rows[:, 2].astype(np.int64)
            at += 3 * g["nsurv"]
        if g["done"]:
            rows = np.asarray(words[at:at + 2 * g["m_live"]], dtype=np.uint64).reshape(g["m_live"], 2)
            g["live_hashes"] = rows[:, 0] | (rows[:, 1] << np.uint64(32))
            at += 2 * g["m_live"]
        graphs.append(g)
    return graphs


class EngineError(RuntimeError):
    pass


def lib():
    global _LIB
    if _LIB is None:
        path = _LIBPATH
        if not os.path.exists(path):
            raise EngineError(f"{_LIBPATH} is missing: build it with `python -m lancet_amd.build` (there is no CPU fallback)")
        L = C.CDLL(path)
        L.lancet_params_default.argtypes = [C.POINTER(abi.LancetParams)]
        L.lancet_engine_create.argtypes = [C.POINTER(abi.LancetParams), C.c_int, C.POINTER(C.c_void_p)]
        L.lancet_engine_destroy.argtypes = [C.c_void_p]
        L.lancet_engine_last_error.restype = C.c_char_p
        L.lancet_engine_last_error.argtypes = [C.c_void_p]
        L.lancet_engine_upload.argtypes = [C.c_void_p, C.POINTER(abi.LancetWindowBatch)]
        L.lancet_engine_run.argtypes = [C.c_void_p]
        L.lancet_engine_submit.argtypes = [C.c_void_p]
        L.lancet_engine_submit_after.argtypes = [C.c_void_p, C.c_void_p]
        L.lancet_engine_wait.argtypes = [C.c_void_p]
        L.lancet_engine_process.argtypes = [C.c_void_p, C.POINTER(abi.LancetWindowBatch)]
        L.lancet_engine_results.argtypes = [C.c_void_p, C.POINTER(C.POINTER(abi.LancetVariant)), C.POINTER(C.c_uint32),
                                            C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.POINTER(C.POINTER(abi.LancetWindowStats))]
        L.lancet_engine_last_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float * 2)]
        L.lancet_engine_results_lr.argtypes = [C.c_void_p, C.POINTER(C.POINTER(abi.LancetVariantLR)), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint32)]
        L.lancet_engine_set_trace.argtypes = [C.c_void_p, C.c_uint32]
        L.lancet_engine_set_haplotypes.argtypes = [C.c_void_p, C.c_uint32]
        L.lancet_engine_results_haplotypes.argtypes = [C.c_void_p, C.POINTER(C.POINTER(abi.LancetHaplotype)), C.POINTER(C.c_uint32), C.POINTER(C.POINTER(C.c_uint32)),
                                                       C.POINTER(C.c_uint32), C.POINTER(C.POINTER(C.c_uint8))]
        L.lancet_engine_set_haplotype_alignments.argtypes = [C.c_void_p, C.c_int]
        L.lancet_engine_results_haplotype_alignments.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint32)]
        L.lancet_engine_set_haplotype_coverage.argtypes = [C.c_void_p, C.c_int]
        L.lancet_engine_results_haplotype_coverage.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_uint16)), C.POINTER(C.c_uint32)]
        L.lancet_engine_set_haplotype_support.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.lancet_engine_results_haplotype_support.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint32))]
        L.lancet_engine_haplotype_support_ms.restype = C.c_float
        L.lancet_engine_haplotype_support_ms.argtypes = [C.c_void_p]
        L.lancet_engine_set_haplotype_placements.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.lancet_engine_results_haplotype_placements.argtypes = [C.c_void_p, C.POINTER(C.POINTER(abi.LancetReadPlacement)), C.POINTER(C.c_uint32),
                                                                 C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_uint16))]
        L.lancet_engine_haplotype_placement_ms.restype = C.c_float
        L.lancet_engine_haplotype_placement_ms.argtypes = [C.c_void_p]
        L.lancet_engine_set_haplotype_evidence.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
        L.lancet_engine_results_haplotype_evidence.argtypes = [C.c_void_p, C.POINTER(C.POINTER(abi.LancetVariantEvidence)), C.POINTER(C.c_uint32),
                                                               C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_uint8))]
        L.lancet_engine_haplotype_evidence_ms.restype = C.c_float
        L.lancet_engine_haplotype_evidence_ms.argtypes = [C.c_void_p]
        L.lancet_engine_haplotype_evidence_readback_ms.restype = C.c_float
        L.lancet_engine_haplotype_evidence_readback_ms.argtypes = [C.c_void_p]
        L.lancet_engine_haplotype_readback_ms.restype = C.c_float
        L.lancet_engine_haplotype_readback_ms.argtypes = [C.c_void_p]
        L.lancet_engine_set_trace_level.argtypes = [C.c_void_p, C.c_uint32, C.c_int32]
        L.lancet_engine_trace_level.argtypes = [C.c_void_p]
        L.lancet_engine_trace.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint32)]
        L.lancet_engine_rerun_count.argtypes = [C.c_void_p]
        L.lancet_engine_prebuilt_count.argtypes = [C.c_void_p]
        L.lancet_engine_settled_count.argtypes = [C.c_void_p]
        L.lancet_engine_ahead_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.lancet_engine_svc_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint32 * 4)]
        L.lancet_engine_build_phase_times.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint64))]
        L.lancet_engine_kernel_times.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int]
        L.lancet_engine_kernel_name.restype = C.c_char_p
        L.lancet_engine_kernel_name.argtypes = [C.c_int]
        L.lancet_engine_geometry.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
        L.lancet_debug_align.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
        L.lancet_debug_align_mode.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int]
        L.lancet_engine_phase_times.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint64))]
        # device read selection (opts is host.LancetHostOpts: passed by address)
        L.lancet_device_reads_create.argtypes = [C.c_int, C.POINTER(abi.LancetAlignmentTable), C.POINTER(C.c_void_p)]
        L.lancet_device_reads_destroy.argtypes = [C.c_void_p]
        L.lancet_device_reads_bytes.restype = C.c_uint64
        L.lancet_device_reads_bytes.argtypes = [C.c_void_p]
        L.lancet_engine_upload_windows.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(abi.LancetWindowSlice), C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.lancet_engine_debug_select.argtypes = [C.c_void_p, C.POINTER(C.POINTER(abi.LancetSelectSummary)), C.POINTER(C.c_int32)]
        L.lancet_engine_debug_batch.restype = C.c_longlong
        L.lancet_engine_debug_batch.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_size_t]
        L.lancet_filters_default.argtypes = [C.POINTER(abi.LancetFilters)]
        L.lancet_vdb_create.restype = C.c_void_p
        L.lancet_vdb_create.argtypes = [C.POINTER(abi.LancetFilters)]
        L.lancet_vdb_destroy.argtypes = [C.c_void_p]
        L.lancet_vdb_add.argtypes = [C.c_void_p, C.POINTER(abi.LancetVariant), C.c_uint32, C.c_char_p, C.POINTER(C.c_char_p), C.c_int32]
        L.lancet_vdb_add_lr.argtypes = [C.c_void_p, C.POINTER(abi.LancetVariant), C.POINTER(abi.LancetVariantLR), C.c_uint32, C.c_char_p,
                                        C.POINTER(C.c_uint32), C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_char_p), C.c_int32]
        L.lancet_vdb_keys.argtypes = [C.POINTER(abi.LancetVariant), C.c_uint32, C.c_char_p, C.POINTER(C.c_char_p), C.c_int32, C.c_void_p]
        L.lancet_vdb_add_keyed.argtypes = [C.c_void_p, C.POINTER(abi.LancetVariant), C.POINTER(abi.LancetVariantLR), C.c_void_p, C.c_uint32, C.c_char_p,
                                           C.POINTER(C.c_uint32), C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_char_p), C.c_int32]
        L.lancet_vdb_reduce.argtypes = [C.POINTER(abi.LancetVariant), C.c_void_p, C.c_uint32, C.c_void_p]
        L.lancet_vdb_size.restype = C.c_uint32
        L.lancet_vdb_size.argtypes = [C.c_void_p]
        L.lancet_vdb_vcf.restype = C.c_void_p
        L.lancet_vdb_vcf.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]
        L.lancet_free.argtypes = [C.c_void_p]
        L.lancet_trace_format.restype = C.c_void_p
        L.lancet_trace_format.argtypes = [C.POINTER(C.c_uint32), C.c_uint32, C.c_int32, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, C.c_int32]
        _LIB = L
    return _LIB


class DeviceReads:
    """lancet_device_reads: the alignment table of a scan (host.NativeHost.alignment_table) resident on one device, shared by every
    engine on it.  There is no CPU path: without a GPU creation raises."""

    def __init__(self, table: "abi.LancetAlignmentTable", device: int = 0):
        self.L = lib()
        h = C.c_void_p()
        rc = self.L.lancet_device_reads_create(device, C.byref(table), C.byref(h))
        if rc != 0:
            why = self.L.lancet_engine_last_error(None).decode()
            raise EngineError(f"lancet_device_reads_create failed: {ERRORS.get(rc, rc)}" + (f" ({why})" if rc not in (-2,) and why != "null engine" else ""))
        self.h = h
        self.device = device

    @property
    def nbytes(self) -> int:
        return int(self.L.lancet_device_reads_bytes(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.L.lancet_device_reads_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class Engine:
    def __init__(self, params: Optional[abi.LancetParams] = None, device: int = 0, trace_words: int = 0, trace_level: int = 1, haplotype_words: int = 0,
                 haplotype_alignments: bool = False, haplotype_coverage: bool = False, haplotype_support: bool = False,
                 haplotype_support_mismatches: int = 5, haplotype_placements: bool = False, haplotype_placement_mismatches: int = 5,
                 haplotype_evidence: int = 0, haplotype_evidence_mismatches: int = 5):
        """trace_words: 32-bit words of trace events kept per window (0: no trace).  trace_level 1: the reference's -v lines; 2: its -V
        (--more-verbose) lines as well -- a diagnostics mode in which every graph takes the general build (lancet_engine_set_trace_level).
        haplotype_words: 32-bit words kept per window for its assembled haplotypes (0: none; lancet_engine_set_haplotypes, haplotypes()).
        haplotype_alignments: each of them with its CIGAR against its reference stretch, out of the same words (set_haplotype_alignments).
        haplotype_coverage: each of them with the reads' support of every base of path and stretch, out of the same words (set_haplotype_coverage).
        haplotype_support: each of them with the numbers of reads that fit it, and fit it alone among the haplotypes of its (k, component), within
        haplotype_support_mismatches mismatches, by class Tf Tr Nf Nr; eight more words each (set_haplotype_support).
        haplotype_placements: per read of the batch the haplotype it fits best, where it lies on it and with how many mismatches, within
        haplotype_placement_mismatches (set_haplotype_placements, placements()); no words of the windows' buffers.
        haplotype_evidence: records kept per window for the events of its haplotypes -- per allele the reads that carry it, the reference allele
        or something else at its site, within haplotype_evidence_mismatches (set_haplotype_evidence; needs haplotype_alignments; haplotypes()
        then gives every dict its "events"); no words of the windows' buffers either."""
        self.L = lib()
        self.params = params or abi.default_params()
        h = C.c_void_p()
        rc = self.L.lancet_engine_create(C.byref(self.params), device, C.byref(h))
        if rc != 0:
            raise EngineError(f"lancet_engine_create failed: {ERRORS.get(rc, rc)}")
        self.h = h
        self._batch = None
        if trace_level not in (1, 2):
            raise EngineError(f"trace_level {trace_level}: 1 or 2")
        if trace_words and trace_level == 2:
            self._chk(self.L.lancet_engine_set_trace_level(self.h, trace_words, 2))
        elif trace_words:
            self.L.lancet_engine_set_trace(self.h, trace_words)
        self._hap_aln = False
        self._hap_cov = False
        if haplotype_words:
            self.set_haplotypes(haplotype_words)
        if haplotype_alignments:
            self.set_haplotype_alignments(True)
        if haplotype_coverage:
            self.set_haplotype_coverage(True)
        self._hap_sup = False
        if haplotype_support:
            self.set_haplotype_support(True, haplotype_support_mismatches)

        if haplotype_placements:
            self.set_haplotype_placements(True, haplotype_placement_mismatches)

        self._evid = 0
        if haplotype_evidence:
            self.set_haplotype_evidence(haplotype_evidence, haplotype_evidence_mismatches)

    def set_haplotype_evidence(self, events_per_window: int, max_mismatches: int = 5) -> None:
        """lancet_engine_set_haplotype_evidence: for the uploads that follow (0: off); nothing while the capture or its alignments are off.
        EngineError between an upload and its run, and for max_mismatches outside 0 .. 255."""
        self._chk(self.L.lancet_engine_set_haplotype_evidence(self.h, int(events_per_window), int(max_mismatches)))
        self._evid = int(events_per_window)

    def evidence_marked(self) -> list:
        """Per window of the last run 1 where it had more events than haplotype_evidence records (the first ones are kept, whole)."""
        ep, n, op, mp = C.POINTER(abi.LancetVariantEvidence)(), C.c_uint32(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint8)()
        self._chk(self.L.lancet_engine_results_haplotype_evidence(self.h, C.byref(ep), C.byref(n), C.byref(op), C.byref(mp)))
        nw = self._batch.n_windows if self._batch is not None else 0
        return [int(mp[w]) for w in range(nw)]

    def haplotype_evidence_ms(self) -> float:
        """HIP-event milliseconds of the evidence kernel in the last run (0 with the switch off)."""
        return float(self.L.lancet_engine_haplotype_evidence_ms(self.h))

    def haplotype_evidence_readback_ms(self) -> float:
        return float(self.L.lancet_engine_haplotype_evidence_readback_ms(self.h))

    def set_haplotype_placements(self, on: bool, max_mismatches: int = 5) -> None:
        """lancet_engine_set_haplotype_placements: for the uploads that follow; nothing while the capture is off.  EngineError between an
        upload and its run, and for max_mismatches outside 0 .. 255."""
        self._chk(self.L.lancet_engine_set_haplotype_placements(self.h, 1 if on else 0, int(max_mismatches)))

    def placements(self):
        """(records, read_begin, tlen) of the last run: a numpy structured array (abi.PLACEMENT_DTYPE: haplotype = index_in_window or -1,
        offset, mismatches, n_offsets, n_haplotypes, cls 0..3 = Tf Tr Nf Nr) with one record per read in the batch's read order, window w's
        at read_begin[w] .. read_begin[w + 1], and every read's trimmed length.  Empty with the switch off (include/lancet_engine.h)."""
        pp, n, rb, tl = C.POINTER(abi.LancetReadPlacement)(), C.c_uint32(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint16)()
        self._chk(self.L.lancet_engine_results_haplotype_placements(self.h, C.byref(pp), C.byref(n), C.byref(rb), C.byref(tl)))
        nw = len(self.results()[1]) if n.value else 0            # (one statistics record per window of the run, whatever route uploaded it)
        return abi.placements_to_py(pp, n.value, rb, nw, tl)

    def haplotype_placement_ms(self) -> float:
        """HIP-event milliseconds of the placement kernel in the last run (0 with the switch off)."""
        return float(self.L.lancet_engine_haplotype_placement_ms(self.h))

    def set_haplotypes(self, words_per_window: int) -> None:
        """lancet_engine_set_haplotypes: for the uploads that follow (0: off).  EngineError between an upload and its run."""
        self._chk(self.L.lancet_engine_set_haplotypes(self.h, words_per_window))

    def set_haplotype_alignments(self, on: bool) -> None:
        """lancet_engine_set_haplotype_alignments: for the uploads that follow; nothing while the capture is off.  EngineError between an
        upload and its run."""
        self._chk(self.L.lancet_engine_set_haplotype_alignments(self.h, 1 if on else 0))
        self._hap_aln = bool(on)

    def set_haplotype_coverage(self, on: bool) -> None:
        """lancet_engine_set_haplotype_coverage: for the uploads that follow; nothing while the capture is off.  EngineError between an
        upload and its run."""
        self._chk(self.L.lancet_engine_set_haplotype_coverage(self.h, 1 if on else 0))
        self._hap_cov = bool(on)

    def set_haplotype_support(self, on: bool, max_mismatches: int = 5) -> None:
        """lancet_engine_set_haplotype_support: for the uploads that follow; nothing while the capture is off.  EngineError between an
        upload and its run, and for max_mismatches outside 0 .. 255."""
        self._chk(self.L.lancet_engine_set_haplotype_support(self.h, 1 if on else 0, int(max_mismatches)))
        self._hap_sup = bool(on)

    def haplotype_support_ms(self) -> float:
        """HIP-event milliseconds of the support kernel in the last run (0 with the switch off)."""
        return float(self.L.lancet_engine_haplotype_support_ms(self.h))

    def haplotypes(self):
        """(haplotypes, truncated) of the last run: abi.haplotypes_to_py's dicts ordered by (window, index), and per window 1 where some of its
        haplotypes did not fit.  Both empty / all zero with the capture off.  With haplotype_alignments every dict also has "cigar": (length, op)
        pairs, op one of = X I D (I: bases the reference stretch does not have).  With haplotype_coverage every dict has "cov": {"path": len x 4
        uint16 (an+ an- at+ at-), "ref": ref_len x 4 uint16 (rn+ rn- rt+ rt-)}, the cells of the reference's vertical alignment.  With
        haplotype_support every dict has "support": {"fit": [Tf, Tr, Nf, Nr], "alone": [Tf, Tr, Nf, Nr]}, the reads that fit it (include/lancet_engine.h).
        With haplotype_evidence every dict has "events": its events in CIGAR order, each a dict rb rs pb ps variant flags alt ref other -- the
        last three [Tf, Tr, Nf, Nr], `variant` the index in results()'s records of the one the event emitted or -1 (evidence_marked(): the
        windows that had more events than were kept)."""
        hp, n, wp, nwd, tp = C.POINTER(abi.LancetHaplotype)(), C.c_uint32(), C.POINTER(C.c_uint32)(), C.c_uint32(), C.POINTER(C.c_uint8)()
        self._chk(self.L.lancet_engine_results_haplotypes(self.h, C.byref(hp), C.byref(n), C.byref(wp), C.byref(nwd), C.byref(tp)))
        words = np.ctypeslib.as_array(wp, shape=(nwd.value,)).copy() if nwd.value else np.zeros(0, np.uint32)
        nw = self._batch.n_windows if self._batch is not None else 0
        haps = abi.haplotypes_to_py(hp, n.value, words)
        if self._hap_aln:
            op, cp, nc = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.c_uint32()
            self._chk(self.L.lancet_engine_results_haplotype_alignments(self.h, C.byref(op), C.byref(cp), C.byref(nc)))
            for i, h in enumerate(haps):
                h["cigar"] = abi.cigar_to_py(cp[op[i]:op[i + 1]])
        if self._hap_cov:
            op, vp, nv = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint16)(), C.c_uint32()
            self._chk(self.L.lancet_engine_results_haplotype_coverage(self.h, C.byref(op), C.byref(vp), C.byref(nv)))
            vals = np.ctypeslib.as_array(vp, shape=(nv.value,)).copy() if nv.value else np.zeros(0, np.uint16)
            for i, h in enumerate(haps):
                h["cov"] = abi.coverage_to_py(vals[op[i]:op[i + 1]], h["len"], h["ref_len"])
        if self._hap_sup:
            sp = C.POINTER(C.c_uint32)()
            self._chk(self.L.lancet_engine_results_haplotype_support(self.h, C.byref(sp)))
            for i, h in enumerate(haps):
                h["support"] = abi.support_to_py(sp[8 * i:8 * i + 8] if sp else [0] * 8)
        if self._evid:
            ep, ne, op, mp = C.POINTER(abi.LancetVariantEvidence)(), C.c_uint32(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint8)()
            self._chk(self.L.lancet_engine_results_haplotype_evidence(self.h, C.byref(ep), C.byref(ne), C.byref(op), C.byref(mp)))
            for h, evs in zip(haps, abi.evidence_to_py(ep, ne.value, op, len(haps))):
                h["events"] = evs
        return haps, [int(tp[w]) for w in range(nw)]

    def haplotype_readback_ms(self) -> float:
        return float(self.L.lancet_engine_haplotype_readback_ms(self.h))

    def _chk(self, rc):
        if rc != 0:
            raise EngineError(f"{ERRORS.get(rc, rc)}: {self.L.lancet_engine_last_error(self.h).decode()}")

    def upload(self, batch) -> None:
        self._batch = batch
        cb = abi.batch_to_c(batch)
        self._chk(self.L.lancet_engine_upload(self.h, C.byref(cb)))

    def upload_packed(self, batch, packed) -> None:
        """lancet_engine_upload_packed: `batch` without bases / qualities (host.NativeHost.batch(..., pack_params=...)), `packed` the dict of
        arrays that call returned (packed with THIS engine's parameters)."""
        self._batch = batch
        cb = abi.batch_to_c(batch)
        keep = {k: np.ascontiguousarray(packed[k], dtype=np.uint32) for k in ("rinfo", "base_woff", "good_woff", "bases", "good")}
        pk = abi.LancetPackedReads(C.sizeof(abi.LancetPackedReads), 0, *[keep[k].ctypes.data_as(C.POINTER(C.c_uint32)) for k in ("rinfo", "base_woff", "good_woff", "bases", "good")])
        # the thresholds the producer packed with (host.NativeHost.batch records them): required -- a dict without them would claim this
        # engine's own and walk past the C side's check against reads packed with other thresholds
        for k in ("min_qual_trim", "min_qual_call"):
            if k not in packed:
                raise EngineError(f"upload_packed: the packed dict has no '{k}' (the thresholds the reads were trimmed / masked with)")
        pk.min_qual_trim = int(packed["min_qual_trim"]); pk.min_qual_call = int(packed["min_qual_call"])
        if packed.get("read_index") is not None:              # the reads stored once per batch (include/lancet_engine.h)
            keep["read_index"] = np.ascontiguousarray(packed["read_index"], dtype=np.uint32)
            pk.read_index = keep["read_index"].ctypes.data_as(C.POINTER(C.c_uint32)); pk.n_distinct = int(packed["n_distinct"])
        self._packed_keep = keep
        self.L.lancet_engine_upload_packed.restype = C.c_int
        self.L.lancet_engine_upload_packed.argtypes = [C.c_void_p, C.POINTER(abi.LancetWindowBatch), C.POINTER(abi.LancetPackedReads)]
        self._chk(self.L.lancet_engine_upload_packed(self.h, C.byref(cb), C.byref(pk)))

    def upload_windows(self, reads: DeviceReads, slice_, opts, host=None):
        """lancet_engine_upload_windows: the engine's batch from the windows of `slice_` (host.NativeHost.windows), their reads picked on
        the device from `reads`.  Returns the tiled indices of the kept windows, or None when the batch is NOT TAKEN and has to go through
        upload_packed (why: last_error()).  `host` (the NativeHost of the slice) names the windows for trace_text()."""
        n = max(1, int(slice_.n_windows))
        kept = (C.c_int32 * n)()
        nk = C.c_int32()
        rc = self.L.lancet_engine_upload_windows(self.h, reads.h, C.byref(slice_), C.byref(opts), kept, C.byref(nk))
        if rc == abi.LANCET_NOT_TAKEN:
            return None
        self._chk(rc)
        idx = [int(kept[i]) for i in range(nk.value)]
        import types
        b = types.SimpleNamespace(n_windows=nk.value, hdr=[], chrom=[], ref_start=np.zeros(nk.value, np.int32), ref_off=np.zeros(nk.value + 1, np.uint32))
        if host is not None:
            for k, w in enumerate(idx):
                hdr, chrom, s, e = host.window_info(w)
                b.hdr.append(hdr); b.chrom.append(chrom); b.ref_start[k] = s; b.ref_off[k + 1] = b.ref_off[k] + (e - s)
        self._batch = b
        return idx

    def last_error(self) -> str:
        return self.L.lancet_engine_last_error(self.h).decode()

    def select_summaries(self):
        """test hook: the per-window summaries of the last upload_windows (one per window of the slice)."""
        p = C.POINTER(abi.LancetSelectSummary)()
        n = C.c_int32()
        self._chk(self.L.lancet_engine_debug_select(self.h, C.byref(p), C.byref(n)))
        return [tuple(getattr(p[i], f) for f in ("status", "reads_t", "reads_n", "bases", "tw16", "tw32")) for i in range(n.value)]

    def debug_batch(self):
        """test hook: the uploaded batch read back from the device, as a dict of arrays (lancet_engine_debug_batch)."""
        nw = self._batch.n_windows
        out = {}

        def get(which, count, dt, arg=0):
            a = np.zeros(max(1, count), dtype=dt)
            got = self.L.lancet_engine_debug_batch(self.h, which, arg, a.ctypes.data, count * a.itemsize)
            if got < 0:
                self._chk(int(got))
            return a[:got // a.itemsize]
        out["read_begin"] = get(4, nw + 1, np.uint32)
        out["ref_off"] = get(2, nw + 1, np.uint32)
        R = int(out["read_begin"][-1])
        out["chr_id"] = get(0, nw, np.int32); out["ref_start"] = get(1, nw, np.int32)
        out["ref_codes"] = get(3, int(out["ref_off"][-1]), np.uint8)
        for name, which in (("rinfo", 5), ("name_rank", 6), ("base_woff", 7), ("good_woff", 8)):
            out[name] = get(which, R, np.uint32)
        out["words"] = lambda r, nb, ng: (get(9, nb, np.uint32, r), get(10, ng, np.uint32, r))      # of one read
        for name, which in (("bases", 11), ("good", 12)):                                          # the arrays the offsets point into
            out[name] = get(which, int(self.L.lancet_engine_debug_batch(self.h, which, 0, None, 0)) // 4, np.uint32)
        return out

    def run(self) -> None:
        self._chk(self.L.lancet_engine_run(self.h))

    def submit(self, after: "Engine | None" = None) -> None:
        """Launch the kernels of the uploaded batch and return at once (collect with wait()).  `after`: another engine on the same
        device whose batch is in flight -- this batch's kernels then start when that one's build kernel is through."""
        if after is not None and after is not self:
            self._chk(self.L.lancet_engine_submit_after(self.h, after.h))
        else:
            self._chk(self.L.lancet_engine_submit(self.h))

    def wait(self) -> None:
        self._chk(self.L.lancet_engine_wait(self.h))

    def process(self, batch):
        self.upload(batch)
        self.run()
        return self.results()

    def raw_results(self):
        vp = C.POINTER(abi.LancetVariant)()
        n = C.c_uint32()
        blob = C.c_void_p()
        bl = C.c_uint32()
        sp = C.POINTER(abi.LancetWindowStats)()
        self._chk(self.L.lancet_engine_results(self.h, C.byref(vp), C.byref(n), C.byref(blob), C.byref(bl), C.byref(sp)))
        return vp, n.value, (C.string_at(blob, bl.value) if bl.value else b""), sp

    def raw_results_lr(self):
        """(lancet_variant_lr*, bx_blob*, bx_blob_len) of the last run; the first is NULL unless lr_mode."""
        lp = C.POINTER(abi.LancetVariantLR)()
        bp = C.POINTER(C.c_uint32)()
        bl = C.c_uint32()
        self._chk(self.L.lancet_engine_results_lr(self.h, C.byref(lp), C.byref(bp), C.byref(bl)))
        return lp, bp, bl.value

    def results(self):
        vp, n, blob, sp = self.raw_results()
        variants = abi.variants_to_py(vp, n, blob)
        if self.params.lr_mode:
            lp, bp, _ = self.raw_results_lr()
            abi.variants_lr_to_py(variants, lp, bp)
        nw = self._batch.n_windows
        stats = [dict(status=sp[i].status, final_k=sp[i].final_k, n_builds=sp[i].n_builds, n_variants=sp[i].n_variants,
                      n_kmers=sp[i].n_kmers, max_nodes=sp[i].max_nodes, sum_nodes=sp[i].sum_nodes) for i in range(nw)]
        return variants, stats

    def timing_ms(self):
        t = (C.c_float * 2)()
        self._chk(self.L.lancet_engine_last_timing(self.h, C.byref(t)))
        return float(t[0]), float(t[1])

    def kernel_names(self):
        out = []
        i = 0
        while True:
            n = self.L.lancet_engine_kernel_name(i)
            if not n:
                return out
            out.append(n.decode()); i += 1

    def kernel_times(self):
        """HIP-event duration (ms) of every kernel of the last run, in kernel_names() order."""
        buf = (C.c_float * 8)()
        n = self.L.lancet_engine_kernel_times(self.h, buf, 8)
        if n < 0:
            self._chk(n)
        return [float(buf[i]) for i in range(n)]

    def build_phase_times(self):
        """Workgroup-seconds of the LDS build kernel per phase (profiling aid)."""
        p = C.POINTER(C.c_uint64)()
        self._chk(self.L.lancet_engine_build_phase_times(self.h, C.byref(p)))
        return [p[i] * 1e-8 for i in range(16)]

    def prebuilt_count(self) -> int:
        return int(self.L.lancet_engine_prebuilt_count(self.h))

    def settled_count(self) -> int:
        """Windows of the last run that the build kernel settled (reference-only chains: no record, nothing loaded by the window kernel)."""
        return int(self.L.lancet_engine_settled_count(self.h))

    def pre_headers(self):
        """test hook: per window of the last run (built in LDS, K, nodes, table order + components came along) from the hand-off headers"""
        import numpy as np
        nw = self._batch.n_windows
        out = np.zeros(8 * max(1, nw), dtype=np.uint32)
        self.L.lancet_debug_pre_headers.argtypes = [C.c_void_p, C.c_void_p]
        if self.L.lancet_debug_pre_headers(self.h, out.ctypes.data) != 0:
            return []
        o = out.reshape(-1, 8)[:nw]
        return [dict(built=int(r[0] & 0xFF) == 1, K=int(r[1]), nodes=int(r[3]), order=bool(r[0] >> 16 & 1)) for r in o]

    def pre_order(self, w):
        """test hook: the table order of every graph of window w that the last run left in a hand-off area -- the window's first graph, then
        the graphs built ahead and the build service's (PreHdr::next) -- as parse_pre_order returns them"""
        import numpy as np
        out = np.zeros(PRE_ORDER_WORDS, dtype=np.uint32)
        self.L.lancet_debug_pre_order.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        n = self.L.lancet_debug_pre_order(self.h, int(w), out.ctypes.data, len(out))
        if n < 0:
            self._chk(n)
        return parse_pre_order(out[:n])

    def ahead_counts(self):
        """(graphs the build kernel built ahead at a later k, how many the window kernel took)"""
        b, u = C.c_int32(), C.c_int32()
        self._chk(self.L.lancet_engine_ahead_counts(self.h, C.byref(b), C.byref(u)))
        return b.value, u.value

    def svc_counts(self):
        """Build service of the last run: (requests posted, served in LDS, not buildable there, taken back by the window kernel)"""
        a = (C.c_uint32 * 4)()
        self._chk(self.L.lancet_engine_svc_counts(self.h, C.byref(a)))
        return tuple(int(x) for x in a)

    def rerun_count(self) -> int:
        return int(self.L.lancet_engine_rerun_count(self.h))

    def geometry(self):
        s = C.c_int32()
        b = C.c_uint64()
        self._chk(self.L.lancet_engine_geometry(self.h, C.byref(s), C.byref(b)))
        return s.value, b.value

    def trace_text(self) -> str:
        """The trace of the last run as the reference prints it: the -v lines, at trace_level 2 the -V lines among them (and, for a window whose
        events did not fit trace_words, a line that says so)."""
        lp = C.POINTER(C.c_uint32)()
        ep = C.POINTER(C.c_uint32)()
        wpw = C.c_uint32()
        self._chk(self.L.lancet_engine_trace(self.h, C.byref(lp), C.byref(ep), C.byref(wpw)))
        if not wpw.value:
            return ""
        b = self._batch
        lens = np.ctypeslib.as_array(lp, shape=(b.n_windows,))
        ev = np.ctypeslib.as_array(ep, shape=(b.n_windows * wpw.value,))
        parts = []
        for w in range(b.n_windows):
            words = ev[w * wpw.value: w * wpw.value + int(lens[w])]
            end = int(b.ref_start[w]) + int(b.ref_off[w + 1] - b.ref_off[w])
            if self.L.lancet_engine_trace_level(self.h) == 2:
                rawseq = bytes(b.ref_bases[int(b.ref_off[w]):int(b.ref_off[w + 1])]).decode()
                parts.append(_trace.format_window2(words, wpw.value, w + 1, b.hdr[w], b.chrom[w], int(b.ref_start[w]), end,
                                                   dfs_limit=int(self.params.dfs_limit), rawseq=rawseq))
            else:
                parts.append(_trace.format_window(words, w + 1, b.hdr[w], b.chrom[w], int(b.ref_start[w]), end, dfs_limit=int(self.params.dfs_limit)))
        return "".join(parts)

    def phase_times(self):
        """[n_windows, 16] array of per-phase times in seconds (profiling aid)."""
        p = C.POINTER(C.c_uint64)()
        self._chk(self.L.lancet_engine_phase_times(self.h, C.byref(p)))
        return np.ctypeslib.as_array(p, shape=(self._batch.n_windows, 16)).astype(np.float64) * 1e-8

    def debug_align(self, s: str, t: str, mode: int = 0, fat: bool = False):
        """Test hook: the device global_align_aff on one pair of strings.  mode 0: banded matrix with the full one as fall-back (what
        the window kernel runs), 1: full matrix only, 2: band only -- returns None when the band could not be certified.  fat: through
        the 512-lane build of the kernels (the re-run tier's).  EngineError where the reference's traceback is undefined on the pair."""
        cap = len(s) + len(t) + 8
        a = C.create_string_buffer(cap)
        b = C.create_string_buffer(cap)
        rc = self.L.lancet_debug_align_mode(self.h, s.encode(), t.encode(), a, b, cap, mode + (4 if fat else 0))
        if rc == -6 and mode == 2:
            return None
        self._chk(rc)
        return a.value.decode(), b.value.decode()

    def close(self):
        if getattr(self, "h", None):
            self.L.lancet_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def record_keys(vptr, n: int, blob: bytes, chr_names: Sequence[str]):
    """lancet_vdb_keys: the 32-byte addVar key (sha256 of Variant_t::getSignature) of each of n records -> uint8[n, 32]."""
    import numpy as np
    keys = np.zeros((max(1, n), 32), dtype=np.uint8)
    names = abi.c_string_array(list(chr_names))
    rc = lib().lancet_vdb_keys(vptr, n, blob, names, len(chr_names), keys.ctypes.data)
    if rc != 0:
        raise EngineError(f"lancet_vdb_keys: {ERRORS.get(rc, rc)}")
    return keys[:n]


def records_that_matter(vptr, keys, n: int):
    """lancet_vdb_reduce: bool[n], the records of a keyed stream (in adding order) that can change a VariantDB."""
    import numpy as np
    keep = np.zeros(max(1, n), dtype=np.uint8)
    rc = lib().lancet_vdb_reduce(vptr, keys.ctypes.data, n, keep.ctypes.data)
    if rc != 0:
        raise EngineError(f"lancet_vdb_reduce: {ERRORS.get(rc, rc)}")
    return keep[:n].astype(bool)


class VariantDB:
    """reference src/VariantDB.cc: addVar + printToVCF (host)."""

    def __init__(self, filters: Optional[abi.LancetFilters] = None):
        self.L = lib()
        self.h = C.c_void_p(self.L.lancet_vdb_create(C.byref(filters) if filters is not None else None))

    def add_raw(self, vptr, n: int, blob: bytes, chr_names: Sequence[str]) -> None:
        names = abi.c_string_array(list(chr_names))
        rc = self.L.lancet_vdb_add(self.h, vptr, n, blob, names, len(chr_names))
        if rc != 0:
            raise EngineError(f"lancet_vdb_add: {ERRORS.get(rc, rc)}")

    def add_raw_lr(self, vptr, lrptr, n: int, blob: bytes, bx_blob, bx_names: Sequence[str], chr_names: Sequence[str]) -> None:
        names = abi.c_string_array(list(chr_names))
        bxn = abi.c_string_array(list(bx_names))
        rc = self.L.lancet_vdb_add_lr(self.h, vptr, lrptr, n, blob, bx_blob, bxn, len(bx_names), names, len(chr_names))
        if rc != 0:
            raise EngineError(f"lancet_vdb_add_lr: {ERRORS.get(rc, rc)}")

    def add_raw_keyed(self, vptr, lrptr, keys, n: int, blob: bytes, bx_blob, bx_names: Optional[Sequence[str]], chr_names: Sequence[str]) -> None:
        """The records with their addVar keys (record_keys, computed where the records were made): rank 0 of a multi-GPU run only inserts.
        keys: numpy uint8 array of 32 * n bytes; lrptr / bx_blob / bx_names None without --linked-reads."""
        names = abi.c_string_array(list(chr_names))
        bxn = abi.c_string_array(list(bx_names)) if bx_names is not None else None
        rc = self.L.lancet_vdb_add_keyed(self.h, vptr, lrptr, keys.ctypes.data, n, blob, bx_blob, bxn, len(bx_names) if bx_names is not None else 0,
                                         names, len(chr_names))
        if rc != 0:
            raise EngineError(f"lancet_vdb_add_keyed: {ERRORS.get(rc, rc)}")

    def add_records(self, records: List[dict], chr_names: Sequence[str], bx_names: Optional[Sequence[str]] = None) -> None:
        """records: dicts as produced by abi.variants_to_py (any source); with bx_names: linked-read records
        (abi.variants_lr_to_py) for a --linked-reads database."""
        arr = (abi.LancetVariant * len(records))()
        blob = bytearray()
        if bx_names is not None:
            lr = (abi.LancetVariantLR * max(1, len(records)))()
            ids: List[int] = []
            for i, r in enumerate(records):
                for q in range(12):
                    lr[i].hp[q] = r["hp"][q]
                for q in range(4):
                    lr[i].bx_off[q], lr[i].bx_len[q] = len(ids), len(r["bx"][q])
                    ids += list(r["bx"][q])
            bxb = (C.c_uint32 * max(1, len(ids)))(*ids)
        for i, r in enumerate(records):
            v = arr[i]
            v.window, v.seq_in_window, v.chr_id, v.pos = r["window"], r["seq"], r["chr_id"], r["pos"]
            v.code, v.prev_bp_ref, v.prev_bp_alt, v.kmer = ord(r["code"]), ord(r["prev_bp_ref"]), ord(r["prev_bp_alt"]), r["kmer"]
            for q in range(8):
                v.cov[q] = r["cov"][q]
            v.ref_off, v.ref_len = len(blob), len(r["ref"]); blob += r["ref"].encode()
            v.alt_off, v.alt_len = len(blob), len(r["alt"]); blob += r["alt"].encode()
            v.str_off, v.str_len = len(blob), len(r["str"]); blob += r["str"].encode()
        if bx_names is not None:
            self.add_raw_lr(arr, lr, len(records), bytes(blob) + b"\0", bxb, bx_names, chr_names)
        else:
            self.add_raw(arr, len(records), bytes(blob) + b"\0", chr_names)

    def size(self) -> int:
        return int(self.L.lancet_vdb_size(self.h))

    def vcf(self, version: Optional[str] = None, cmdline: Optional[str] = None, reference: Optional[str] = None,
            date_line: Optional[str] = None, sample_normal: str = "NORMAL", sample_tumor: str = "TUMOR") -> str:
        enc = lambda s: s.encode() if s is not None else None
        p = self.L.lancet_vdb_vcf(self.h, enc(version), enc(cmdline), enc(reference), enc(date_line), enc(sample_normal), enc(sample_tumor))
        if not p:
            raise EngineError("lancet_vdb_vcf failed")
        try:
            return C.string_at(p).decode()
        finally:
            self.L.lancet_free(p)

    def close(self):
        if getattr(self, "h", None):
            self.L.lancet_vdb_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
