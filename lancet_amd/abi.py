"""ctypes mirror of include/lancet_engine.h (struct layouts only; no logic)."""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

import numpy as np


class _RecoverySlot(C.Union):
    """The 16th word of lancet_params: `kmer_recovery`; `reserved` is the name the slot had before (still accepted, same word)."""
    _fields_ = [("kmer_recovery", C.c_int32), ("reserved", C.c_int32)]


class LancetParams(C.Structure):
    _anonymous_ = ("_slot16",)
    _fields_ = [(n, C.c_int32) for n in (
        "min_k", "max_k", "max_tip_len", "cov_threshold", "low_cov_threshold", "dfs_limit", "max_indel_len",
        "max_mismatch", "min_qual_trim", "min_qual_call", "max_unit_len", "min_report_units", "min_report_len",
        "dist_from_str", "lr_mode")] + [("_slot16", _RecoverySlot), ("min_cov_ratio", C.c_double)]


def default_params(**over) -> LancetParams:
    """Reference defaults, src/Lancet.hh:33-81."""
    p = LancetParams(min_k=11, max_k=101, max_tip_len=11, cov_threshold=5, low_cov_threshold=1, dfs_limit=1000000,
                     max_indel_len=500, max_mismatch=2, min_qual_trim=10 + 33, min_qual_call=17 + 33,
                     max_unit_len=4, min_report_units=3, min_report_len=7, dist_from_str=1, lr_mode=0, kmer_recovery=0,
                     min_cov_ratio=0.01)
    for k, v in over.items():
        setattr(p, k, v)
    return p


class LancetWindowBatch(C.Structure):
    _fields_ = [
        ("n_windows", C.c_int32),
        ("chr_id", C.POINTER(C.c_int32)), ("ref_start", C.POINTER(C.c_int32)),
        ("ref_off", C.POINTER(C.c_uint32)), ("ref_bases", C.c_char_p),
        ("read_begin", C.POINTER(C.c_uint32)), ("seq_off", C.POINTER(C.c_uint32)),
        ("seq", C.c_char_p), ("qual", C.c_char_p),
        ("label", C.POINTER(C.c_uint8)), ("strand", C.POINTER(C.c_uint8)), ("mate", C.POINTER(C.c_uint8)),
        ("mapped", C.POINTER(C.c_uint8)), ("name_rank", C.POINTER(C.c_uint32)),
        ("bx_rank", C.POINTER(C.c_uint32)), ("hp", C.POINTER(C.c_uint8)),
    ]


class LancetPackedReads(C.Structure):
    """include/lancet_engine.h lancet_packed_reads: the reads of a batch trimmed and packed by the caller."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32),
                ("rinfo", C.POINTER(C.c_uint32)), ("base_woff", C.POINTER(C.c_uint32)), ("good_woff", C.POINTER(C.c_uint32)),
                ("bases", C.POINTER(C.c_uint32)), ("good", C.POINTER(C.c_uint32)), ("min_qual_trim", C.c_int32), ("min_qual_call", C.c_int32),
                ("read_index", C.POINTER(C.c_uint32)), ("n_distinct", C.c_uint32), ("reserved2", C.c_uint32)]


# ---- device read selection (include/lancet_engine.h)
LANCET_NOT_TAKEN = 1
ALN_SEL_OK, ALN_AR_OK = 1, 2


class LancetAlignmentTable(C.Structure):
    """lancet_alignment_table: the alignments of a scan, handed to the device once (lancet_device_reads_create)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_chroms", C.c_uint32), ("n_aln", C.c_uint32 * 2),
                ("span", C.POINTER(C.c_uint32)), ("pos0", C.POINTER(C.c_int32)), ("ref_len", C.POINTER(C.c_int32)), ("l_seq", C.POINTER(C.c_uint32)),
                ("flags", C.POINTER(C.c_uint8)), ("rinfo", C.POINTER(C.c_uint32)), ("evt_off", C.POINTER(C.c_uint32)), ("evt_kind", C.POINTER(C.c_uint8)),
                ("evt_pos", C.POINTER(C.c_int32)), ("name_off", C.POINTER(C.c_uint32)), ("names", C.POINTER(C.c_char)), ("names_len", C.c_uint64),
                ("base_woff", C.POINTER(C.c_uint32)), ("good_woff", C.POINTER(C.c_uint32)), ("bases", C.POINTER(C.c_uint32)), ("good", C.POINTER(C.c_uint32)),
                ("n_base_words", C.c_uint32), ("n_good_words", C.c_uint32), ("min_qual_trim", C.c_int32), ("min_qual_call", C.c_int32), ("load_id", C.c_uint64)]


class LancetWindowSlice(C.Structure):
    """lancet_window_slice: the windows of a range that pass the host-side window filters (lancet_host_windows)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_windows", C.c_int32), ("widx", C.POINTER(C.c_int32)), ("start", C.POINTER(C.c_int32)), ("end", C.POINTER(C.c_int32)),
                ("chr_id", C.POINTER(C.c_int32)), ("ref_off", C.POINTER(C.c_uint32)), ("ref_bases", C.POINTER(C.c_char)), ("leak_reads", C.c_uint32),
                ("host_reason", C.c_int32), ("load_id", C.c_uint64)]


class LancetSelectSummary(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("status", "reads_t", "reads_n", "bases", "tw16", "tw32")]


class LancetVariantLR(C.Structure):
    _fields_ = [("hp", C.c_uint16 * 12), ("bx_off", C.c_uint32 * 4), ("bx_len", C.c_uint32 * 4), ("reserved", C.c_uint32 * 2)]


class LancetVariant(C.Structure):
    _fields_ = [
        ("window", C.c_int32), ("seq_in_window", C.c_int32), ("chr_id", C.c_int32), ("pos", C.c_int32),
        ("code", C.c_uint8), ("prev_bp_ref", C.c_uint8), ("prev_bp_alt", C.c_uint8), ("reserved", C.c_uint8),
        ("kmer", C.c_uint16), ("cov", C.c_uint16 * 8), ("reserved2", C.c_uint16),
        ("ref_off", C.c_uint32), ("ref_len", C.c_uint32), ("alt_off", C.c_uint32), ("alt_len", C.c_uint32),
        ("str_off", C.c_uint32), ("str_len", C.c_uint32),
    ]


class LancetHaplotype(C.Structure):
    """lancet_haplotype: one path the window kernel compared with the window reference (lancet_engine_results_haplotypes)."""
    _fields_ = [("window", C.c_int32), ("index_in_window", C.c_int32), ("kmer", C.c_uint16), ("component", C.c_uint16),
                ("ref_off", C.c_uint32), ("ref_len", C.c_uint32), ("len", C.c_uint32), ("word_off", C.c_uint32),
                ("first_variant", C.c_int32), ("n_variants", C.c_int32), ("flags", C.c_uint32)]


HAP_HEADER_WORDS = 8          # LANCET_HAP_HEADER_WORDS: a haplotype of n bases takes this + (n + 15) // 16 words of its window's buffer
HAP_UNALIGNED, HAP_IS_REF = 1, 2
HAP_HAS_COVERAGE = 4          # LANCET_HAP_HAS_COVERAGE: the entry carries its per-base coverages (lancet_engine_set_haplotype_coverage)
HAP_HAS_SUPPORT = 8           # LANCET_HAP_HAS_SUPPORT: the entry carries the counts of the reads that fit it (lancet_engine_set_haplotype_support)
HAP_W_NCIGAR = 7              # LANCET_HAP_W_NCIGAR: the header word that counts an entry's CIGAR words (lancet_engine_set_haplotype_alignments)
HAP_OPS = {1: "I", 2: "D", 7: "=", 8: "X"}      # LANCET_HAP_OP_*: BAM's codes, SAM's extended letters


def cigar_to_py(words) -> List[tuple]:
    """CIGAR words (length << 4 | op) as (length, op_char) pairs."""
    return [(int(w) >> 4, HAP_OPS[int(w) & 15]) for w in words]


def coverage_to_py(vals: np.ndarray, length: int, ref_len: int) -> dict:
    """The 4 * (length + ref_len) 16-bit counts of one haplotype as {"path": length x 4 (an+ an- at+ at-), "ref": ref_len x 4 (rn+ rn- rt+ rt-)}."""
    v = np.asarray(vals, dtype=np.uint16)
    if v.size != 4 * (length + ref_len):          # (a haplotype of a run without the switch: none)
        return {"path": np.zeros((0, 4), np.uint16), "ref": np.zeros((0, 4), np.uint16)}
    return {"path": v[:4 * length].reshape(length, 4).copy(), "ref": v[4 * length:].reshape(ref_len, 4).copy()}


def support_to_py(vals) -> dict:
    """The eight counts of one haplotype as {"fit": [Tf, Tr, Nf, Nr], "alone": [Tf, Tr, Nf, Nr]}."""
    v = [int(x) for x in vals]
    return {"fit": v[:4], "alone": v[4:8]}


class LancetReadPlacement(C.Structure):
    """lancet_read_placement: where one read lies on the haplotype it fits best (lancet_engine_results_haplotype_placements)."""
    _fields_ = [("haplotype", C.c_int32), ("offset", C.c_int32), ("mismatches", C.c_uint16), ("n_offsets", C.c_uint16),
                ("n_haplotypes", C.c_uint16), ("cls", C.c_uint16)]


PLACEMENT_DTYPE = np.dtype([("haplotype", "<i4"), ("offset", "<i4"), ("mismatches", "<u2"), ("n_offsets", "<u2"), ("n_haplotypes", "<u2"), ("cls", "<u2")])
PLACEMENT_COUNT_MAX = 127     # LANCET_PLACEMENT_COUNT_MAX: n_offsets and n_haplotypes saturate here


def placements_to_py(pptr, n: int, read_begin_ptr, n_windows: int, tlen_ptr):
    """(records, read_begin, tlen): the lancet_read_placement records as a numpy structured array (PLACEMENT_DTYPE) in the batch's read order,
    read_begin[n_windows + 1] and the trimmed length of every read.  No records (a NULL pointer): three empty arrays but read_begin = [0]."""
    if not pptr or not n:
        return np.zeros(0, PLACEMENT_DTYPE), np.zeros(1, np.uint32), np.zeros(0, np.uint16)
    assert C.sizeof(LancetReadPlacement) == PLACEMENT_DTYPE.itemsize
    recs = np.frombuffer(C.string_at(pptr, n * PLACEMENT_DTYPE.itemsize), dtype=PLACEMENT_DTYPE).copy()
    rb = np.ctypeslib.as_array(read_begin_ptr, shape=(n_windows + 1,)).copy()
    tl = np.ctypeslib.as_array(tlen_ptr, shape=(n,)).copy()
    return recs, rb, tl


def read_cigar(o: int, t: int, length: int, ref_off: int, cigar) -> tuple:
    """(start, [(n, op)], has_m): a placed read's alignment on the window reference through its haplotype's -- the rule of lc_read_cigar
    (lancet_amd/csrc/host_common.h), restated column by column.  o, t: the placement's offset and the read's trimmed length; length, ref_off,
    cigar: the haplotype's len, ref_off and (n, op_char) pairs (none: the path lies on its stretch base for base).  start is 0-based on the
    window reference; ops are M I D S; has_m is False for a read that lies wholly inside an I run (start: the column behind the run)."""
    cols, pp, rc = [], 0, 0          # one (op, path position or None, stretch column -- for an I the one behind it) per alignment column
    for n, op in (cigar or [(length, "=")]):
        for _ in range(n):
            if op == "D":
                cols.append(("D", None, rc))
                rc += 1
            else:
                cols.append(("I" if op == "I" else "M", pp, rc))
                pp += 1
                rc += 0 if op == "I" else 1
    a, b = max(0, o), min(length, o + t)
    on_path = [i for i, c in enumerate(cols) if c[1] is not None and a <= c[1] < b]
    kept = cols[on_path[0]:on_path[-1] + 1]            # (the D columns in between stay, those in front and behind go)
    ops = [[a - o, "S"]]
    for c in kept:
        if ops[-1][1] == c[0]:
            ops[-1][0] += 1
        else:
            ops.append([1, c[0]])
    if ops[-1][1] == "S":
        ops[-1][0] += o + t - b
    else:
        ops.append([o + t - b, "S"])
    return ref_off + kept[0][2], [(n, op) for n, op in ops if n], any(c[0] == "M" for c in kept)


class LancetVariantEvidence(C.Structure):
    """lancet_variant_evidence: one event of a haplotype with the reads for and against its allele (lancet_engine_results_haplotype_evidence)."""
    _fields_ = [("haplotype", C.c_int32), ("variant", C.c_int32), ("rb", C.c_uint32), ("rs", C.c_uint32), ("pb", C.c_uint32), ("ps", C.c_uint32),
                ("flags", C.c_uint32), ("alt", C.c_uint32 * 4), ("ref", C.c_uint32 * 4), ("other", C.c_uint32 * 4)]


EVID_UNEVALUATED = 1          # LANCET_EVID_UNEVALUATED: the event's group is beyond the kernel's lists, all its counts are 0
EVID_GROUP_ENTRIES, EVID_GROUP_EVENTS = 32, 64      # LANCET_EVID_GROUP_ENTRIES / _EVENTS


def evidence_to_py(evptr, n: int, event_off, n_haplotypes: int) -> List[list]:
    """Per haplotype the list of its events' dicts: rb rs pb ps variant flags alt ref other (the three: [Tf, Tr, Nf, Nr]); `variant` is the
    index in the run's records, -1 without one.  No records (a NULL pointer): an empty list each."""
    out = []
    for i in range(n_haplotypes):
        a, b = (int(event_off[i]), int(event_off[i + 1])) if evptr and n else (0, 0)
        out.append([dict(rb=int(x.rb), rs=int(x.rs), pb=int(x.pb), ps=int(x.ps), variant=int(x.variant), flags=int(x.flags),
                         alt=list(x.alt), ref=list(x.ref), other=list(x.other)) for x in (evptr[j] for j in range(a, b))])
    return out


def evidence_variant(h: dict, rb: int, ref_start: int, variants: Sequence[dict]) -> int:
    """The index in `variants` (variants_to_py's dicts of one run) of the record the event at `rb` of haplotype h (haplotypes_to_py's dict)
    emitted, -1 without one -- the rule of lc_evid_join (lancet_amd/csrc/host_common.h), restated: a transcript opens at the event's first
    column, its position is the 1-based window start plus the stretch's offset plus the stretch bases in front, and a record holds that - 1."""
    mine = range(h["first_variant"], h["first_variant"] + h["n_variants"])
    for i, v in enumerate(variants):
        if v["window"] == h["window"] and v["seq"] in mine and v["pos"] + 1 - ref_start - h["ref_off"] == rb:
            return i
    return -1


def haplotypes_to_py(hptr, n: int, words: np.ndarray) -> List[dict]:
    """lancet_haplotype records as dicts, `seq` = the path string (2 bits per base, first base in the low bits of a word)."""
    out = []
    for i in range(n):
        h = hptr[i]
        nw = (h.len + 15) // 16
        w = words[h.word_off:h.word_off + nw].astype(np.uint32)
        codes = ((w[:, None] >> (2 * np.arange(16, dtype=np.uint32))[None, :]) & 3).reshape(-1)
        out.append(dict(window=h.window, index=h.index_in_window, kmer=h.kmer, component=h.component, ref_off=h.ref_off, ref_len=h.ref_len,
                        len=h.len, first_variant=h.first_variant, n_variants=h.n_variants, flags=h.flags,
                        seq="".join("ACGT"[c] for c in codes[:h.len]), n_words=int(len(w)),
                        # the bits of the last word above the last base (0 by contract)
                        pad_bits=int(w[-1] >> np.uint32(2 * (h.len % 16))) if len(w) and h.len % 16 else 0))
    return out


class LancetWindowStats(C.Structure):
    _fields_ = [("status", C.c_int32), ("final_k", C.c_int32), ("n_builds", C.c_int32), ("n_variants", C.c_int32),
                ("n_kmers", C.c_uint64), ("max_nodes", C.c_uint32), ("sum_nodes", C.c_uint32)]


class LancetFilters(C.Structure):
    _fields_ = [("min_phred_fisher_str", C.c_double), ("min_phred_fisher", C.c_double),
                ("max_vaf_normal", C.c_double), ("min_vaf_tumor", C.c_double),
                ("min_cov_normal", C.c_int32), ("max_cov_normal", C.c_int32), ("min_cov_tumor", C.c_int32),
                ("max_cov_tumor", C.c_int32), ("min_alt_cnt_tumor", C.c_int32), ("max_alt_cnt_normal", C.c_int32),
                ("min_strand_bias", C.c_int32), ("reserved", C.c_int32)]


def _p(a: np.ndarray, t):
    return a.ctypes.data_as(C.POINTER(t))


def batch_to_c(b) -> LancetWindowBatch:
    """b: lancet_amd.frontend.WindowBatch (numpy SoA).  The returned struct borrows b's arrays."""
    cb = LancetWindowBatch()
    cb.n_windows = b.n_windows
    cb.chr_id = _p(b.chr_id, C.c_int32)
    cb.ref_start = _p(b.ref_start, C.c_int32)
    cb.ref_off = _p(b.ref_off, C.c_uint32)
    cb.ref_bases = b.ref_bases.ctypes.data_as(C.c_char_p)
    cb.read_begin = _p(b.read_begin, C.c_uint32)
    cb.seq_off = _p(b.seq_off, C.c_uint32)
    cb.seq = b.seq.ctypes.data_as(C.c_char_p)
    cb.qual = b.qual.ctypes.data_as(C.c_char_p)
    cb.label = _p(b.label, C.c_uint8)
    cb.strand = _p(b.strand, C.c_uint8)
    cb.mate = _p(b.mate, C.c_uint8)
    cb.mapped = _p(b.mapped, C.c_uint8)
    cb.name_rank = _p(b.name_rank, C.c_uint32)
    if getattr(b, "bx_rank", None) is not None:
        cb.bx_rank = _p(b.bx_rank, C.c_uint32)
        cb.hp = _p(b.hp, C.c_uint8)
    cb._keep = b
    return cb


def variants_to_py(vptr, n: int, blob: bytes) -> List[dict]:
    out = []
    for i in range(n):
        v = vptr[i]
        out.append(dict(
            window=v.window, seq=v.seq_in_window, chr_id=v.chr_id, pos=v.pos, code=chr(v.code),
            prev_bp_ref=chr(v.prev_bp_ref), prev_bp_alt=chr(v.prev_bp_alt), kmer=v.kmer, cov=tuple(v.cov),
            ref=blob[v.ref_off:v.ref_off + v.ref_len].decode(), alt=blob[v.alt_off:v.alt_off + v.alt_len].decode(),
            str=blob[v.str_off:v.str_off + v.str_len].decode()))
    return out


def variants_lr_to_py(out: List[dict], lrptr, bx_blob) -> List[dict]:
    """Adds the linked-read annotations (hp: 12 counts, bx: 4 tuples of barcode ranks) to variants_to_py's dicts."""
    for i, d in enumerate(out):
        l = lrptr[i]
        d["hp"] = tuple(l.hp)
        d["bx"] = tuple(tuple(int(bx_blob[l.bx_off[q] + j]) for j in range(l.bx_len[q])) for q in range(4))
    return out


def c_string_array(strs: Sequence[str]):
    arr = (C.c_char_p * len(strs))(*[s.encode() for s in strs])
    return arr
