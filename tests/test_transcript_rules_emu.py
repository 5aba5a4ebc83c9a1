"""The rules of the transcript walk alone and without a GPU: kernels.h walk_column (which transcript an alignment column opens, extends
or turns complex), walk_extend (one of the K + 1 positions behind an indel / complex transcript) and ts_record_cov (the coverages of
the record), fed through tests/emu/emu_transcript.cc with hand-made lists of column values -- what the two walk drivers share, without
either driver.  Beside them a plain model of the reference's lines (src/Graph.cc processPath, the loop over the alignment columns and
the loop over the transcripts; src/Transcript.hh computeStats and the getters), written here in Python on the reference's own terms:
every alignment column is visited, a transcript keeps the vectors of its coverages and the statistics are taken at the end.

Compared: the returned status, the number of transcripts, every field of every transcript (the model's vectors reduced to the
accumulators' first / minimum / non-zero minimum / sums / counts), the eight coverages and the twelve haplotype counts of each record.
The lists need not be alignments an aligner would produce: "delete extended" cannot come out of one (see the case)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

GO, END, OVF, FULL = 0, 1, 2, 3
RRBASE = 1000                                  # refstart + trim5
U16 = 0xFFFF


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
    so = os.path.join(str(tmp_path_factory.mktemp("emu_transcript")), "libemu_transcript.so")
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-strict-aliasing", "-w",
                    "-o", so, os.path.join(here, "emu_transcript.cc")], check=True)
    return ctypes.CDLL(so)


def pos(col, code, P, ref, an=(0, 0, 0, 0), at=(0, 0, 0, 0), rn=(0, 0), rt=(0, 0), tumor=False, no_spanner=False, p_outside=False,
        hp_an=(0, 0, 0), hq_an=(0, 0, 0), hp_at=(0, 0, 0), hq_at=(0, 0, 0), hp_rn=(0, 0, 0), hp_rt=(0, 0, 0)):
    """One position's values.  an / at: the path's coverage (fwd, rev, minqv_fwd, minqv_rev), normal / tumor; rn / rt: the reference's (fwd, rev)."""
    return dict(col=col, code=code, P=P, ref=ref, an=an, at=at, rn=rn, rt=rt, tumor=tumor, no_spanner=no_spanner, p_outside=p_outside,
                hp_an=hp_an, hq_an=hq_an, hp_at=hp_at, hq_at=hq_at, hp_rn=hp_rn, hp_rt=hp_rt)


def _flat(v):
    return ([v["col"], ord(v["code"]), v["P"], v["ref"], int(v["tumor"]) | 2 * int(v["no_spanner"]) | 4 * int(v["p_outside"])]
            + list(v["an"]) + list(v["at"]) + list(v["rn"]) + list(v["rt"])
            + list(v["hp_an"]) + list(v["hq_an"]) + list(v["hp_at"]) + list(v["hq_at"]) + list(v["hp_rn"]) + list(v["hp_rt"]))


def run_kernel_rules(L, cols, ext, ra, pa, cap, lr):
    maxts, words = L.lancet_emu_transcript_maxts(), L.lancet_emu_transcript_words()
    c = np.ascontiguousarray([_flat(v) for v in cols], dtype=np.int32).reshape(-1)
    off = np.zeros(maxts + 1, np.int32)
    flat_ext = []
    for ti in range(maxts):
        flat_ext += [_flat(v) for v in ext.get(ti, [])]
        off[ti + 1] = len(flat_ext)
    e = np.ascontiguousarray(flat_ext if flat_ext else [[0] * 35], dtype=np.int32).reshape(-1)
    out = np.zeros((maxts, words), np.uint32)
    nts, ovf = ctypes.c_int(0), ctypes.c_int(0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    status = L.lancet_emu_transcript(p(c), len(cols), p(e), p(off), ra.encode(), pa.encode(), ctypes.c_uint32(RRBASE), cap, int(lr), p(out),
                                     ctypes.byref(nts), ctypes.byref(ovf))
    assert (ovf.value != 0) == (status == OVF)
    return status, nts.value, out[:nts.value].tolist() if status in (GO, END) else None


# ---- the model: the reference's lines
def _cov(four, hp, hq):
    return dict(fwd=four[0], rev=four[1], minqv_fwd=four[2] if len(four) > 2 else 0, minqv_rev=four[3] if len(four) > 3 else 0, hp=list(hp), hq=list(hq))


def model(cols, ext, ra, pa, cap, lr, maxts):
    listed = {v["col"]: v for v in cols}
    ts, code, status = [], "?", GO
    for i in range(len(ra)):
        prev_code = code
        code = "^" if ra[i] == "-" else ("v" if pa[i] == "-" else ("x" if ra[i] != pa[i] else "="))
        if code == "=":
            continue
        v = listed.get(i)
        if v is None:                                       # the list ends before the alignment does
            break
        assert v["code"] == code
        if v["no_spanner"]:                                 # pathcontig() == NULL: break
            status = END
            break
        if v["p_outside"]:                                  # coverageN[P] outside the vector
            status = OVF
            break
        COVn, COVt = _cov(v["an"], v["hp_an"], v["hq_an"]), _cov(v["at"], v["hp_at"], v["hq_at"])
        REFn, REFt = _cov(v["rn"], v["hp_rn"], (0, 0, 0)), _cov(v["rt"], v["hp_rt"], (0, 0, 0))
        rrpos = v["ref"] + RRBASE
        pr = pq = i - 1
        while pr >= 0 and ra[pr] not in "ACGT":
            pr -= 1
        while pq >= 0 and pa[pq] not in "ACGT":
            pq -= 1
        if pr < 0 or pq < 0:                                # assert(pr >= 0) / reading before the string
            status = OVF
            break
        if ts and prev_code != "=":
            t = ts[-1]
            if v["tumor"]:
                t["somatic"] = True
            t["ref"] += ra[i]
            t["qry"] += pa[i]
            t["end_pos"], t["ref_end_pos"] = v["P"], v["ref"]
            if code == "^" and t["code"] == code and t["pos"] == rrpos:
                t["alt_N"].append(COVn); t["alt_T"].append(COVt)
            elif code == "v" and t["code"] == code and t["pos"] + len(t["ref"]) == rrpos:
                t["ref_N"].append(REFn); t["ref_T"].append(REFt)
            elif code == "x" or t["code"] != code:
                t["code"] = "c"
                t["alt_N"].append(COVn); t["alt_T"].append(COVt); t["ref_N"].append(REFn); t["ref_T"].append(REFt)
        else:
            if len(ts) >= maxts:                            # the project's limit of transcripts per path
                status = OVF
                break
            if len(ts) >= cap:
                status = FULL
                break
            ts.append(dict(pos=rrpos, ref_pos=v["ref"], start_pos=v["P"] + 1, code=code, ref=ra[i], qry=pa[i], col0=i, alt_N=[COVn], alt_T=[COVt],
                           ref_N=[REFn], ref_T=[REFt], prev_bp_ref=ra[pr], prev_bp_alt=pa[pq], end_pos=v["P"], ref_end_pos=v["ref"], somatic=v["tumor"]))
    if status in (OVF, FULL):
        return status, len(ts), None
    for ti, t in enumerate(ts):
        if t["code"] != "x":
            for v in ext.get(ti, []):
                if not v["p_outside"]:                      # idx1 < coverageN.size()
                    if v["no_spanner"]:
                        break
                    if v["tumor"]:
                        t["somatic"] = True
                    t["alt_N"].append(_cov(v["an"], v["hp_an"], v["hq_an"])); t["alt_T"].append(_cov(v["at"], v["hp_at"], v["hq_at"]))
                t["ref_N"].append(_cov(v["rn"], v["hp_rn"], (0, 0, 0))); t["ref_T"].append(_cov(v["rt"], v["hp_rt"], (0, 0, 0)))
    return status, len(ts), [_dump(t, lr) for t in ts]


def _stats(vals):
    """computeStats over one field: first, min, min_non0 (starts at the first value, zero or not), the u16 sums, the non-zero count, n."""
    mn = mnz = vals[0]
    s = snz = nnz = 0
    for x in vals:
        s = (s + x) & U16
        if x != 0:
            snz = (snz + x) & U16
            nnz += 1
        mn = min(mn, x)
        if x < mnz and x != 0:
            mnz = x
    return [vals[0], mn, mnz, s, snz, nnz, len(vals)]


def _mean(s, n):
    return int(np.float32(s) / np.float32(n)) & U16 if n > 0 else 0


def _dump(t, lr):
    x = t["code"] == "x"
    out = [t["pos"], t["ref_pos"], t["start_pos"], t["end_pos"], t["ref_end_pos"], t["col0"], t["col0"] + len(t["ref"]) - 1,
           ord(t["code"]), ord(t["prev_bp_ref"]), ord(t["prev_bp_alt"]), int(t["somatic"])]
    acc = {}
    for name, fields in (("alt_N", ("fwd", "rev", "minqv_fwd", "minqv_rev")), ("alt_T", ("fwd", "rev", "minqv_fwd", "minqv_rev")), ("ref_N", ("fwd", "rev")), ("ref_T", ("fwd", "rev"))):
        for f in fields:
            acc[name, f] = _stats([c[f] for c in t[name]])
            out += acc[name, f]
    hp = lambda name, key, j: [c[key][j] for c in t[name]]
    hrmn = {s: [min(hp("ref_" + s, "hp", j)) for j in range(3)] for s in "NT"}
    hrsum = {s: [sum(hp("ref_" + s, "hp", j)) & U16 for j in range(3)] for s in "NT"}
    hamn = {s: [min(hp("alt_" + s, "hp", j)) for j in range(3)] for s in "NT"}
    haq = {s: [min(hp("alt_" + s, "hq", j)) for j in range(3)] for s in "NT"}
    out += hrmn["N"] + hrmn["T"] + hrsum["N"] + hrsum["T"] + hamn["N"] + hamn["T"] + haq["N"] + haq["T"]
    # the record (Graph.cc, the loop over the transcripts)
    MIN, MNZ, SUM, N = 1, 2, 3, 6
    RCNF, RCNR, RCTF, RCTR = acc["ref_N", "fwd"][MIN], acc["ref_N", "rev"][MIN], acc["ref_T", "fwd"][MIN], acc["ref_T", "rev"][MIN]
    qf, qr = ("minqv_fwd", "minqv_rev") if x else ("fwd", "rev")
    ACNF, ACNR = acc["alt_N", qf][MIN], acc["alt_N", qr][MIN]
    if not x:
        ACNF, ACNR = acc["alt_N", qf][MNZ], acc["alt_N", qr][MNZ]
    ACTF, ACTR = acc["alt_T", qf][MIN], acc["alt_T", qr][MIN]
    HPRN, HPRT = list(hrmn["N"]), list(hrmn["T"])
    HPAN, HPAT = (list(haq["N"]), list(haq["T"])) if x else (list(hamn["N"]), list(hamn["T"]))
    if t["somatic"]:
        n = len(t["ref_N"])
        RCNF, RCNR = _mean(acc["ref_N", "fwd"][SUM], n), _mean(acc["ref_N", "rev"][SUM], n)
        RCTF, RCTR = _mean(acc["ref_T", "fwd"][SUM], n), _mean(acc["ref_T", "rev"][SUM], n)
        ACNF = ACNR = 0
        HPRT = [_mean(hrsum["T"][j], n) for j in range(3)]
        HPRN = [_mean(hrsum["N"][j], n) for j in range(3)]
        HPAN = [0, 0, 0]
    out += [RCNF, RCNR, RCTF, RCTR, ACNF, ACNR, ACTF, ACTR]
    order = lambda h: [h[1], h[2], h[0]]                   # {HP1, HP2, HP0}
    out += order(HPRN) + order(HPRT) + order(HPAN) + order(HPAT) if lr else [0] * 12
    return out


# ---- the hand-made lists.  (name, ra, pa, columns, {transcript: extension positions}, lr, cap or None, expected status, expected codes)
A, B = "ACGTACGTAC", "ACGTACGTAC"
_X = lambda col, **kw: pos(col, "x", col, col, an=(5, 6, 3, 4), at=(7, 8, 5, 6), rn=(9, 10), rt=(11, 12), **kw)
_many = lambda n: [_X(1 + 2 * j) for j in range(n)]
_many_aln = lambda n: ("A" * (2 * n + 1), "".join("AC"[j % 2] for j in range(2 * n + 1)))
_EXT3 = [pos(0, "\0", 5, 0, an=(0, 4, 0, 0), at=(6, 0, 1, 1), rn=(3, 3), rt=(2, 8)), pos(1, "\0", 6, 0, an=(2, 0, 0, 0), at=(9, 5, 1, 1), rn=(1, 0), rt=(4, 4)),
         pos(2, "\0", -1, 0, p_outside=True, rn=(7, 7), rt=(0, 6))]
LISTS = [
    ("insert_extended", "ACGT--ACGT", "ACGTGGACGT",                       # t.pos == rrpos: the alternative's side only
     [pos(4, "^", 4, 4, an=(3, 4, 1, 2), at=(5, 6, 2, 3), rn=(8, 9), rt=(7, 6)), pos(5, "^", 5, 4, an=(2, 5, 1, 1), at=(4, 7, 2, 2), rn=(1, 1), rt=(1, 1))],
     {0: _EXT3}, False, None, GO, "^"),
    ("delete_extended", "ACGTGGACGT", "ACGT--ACGT",                       # t.pos + ref.length() == rrpos with the length read after the append: the second
     [pos(4, "v", 3, 4, an=(3, 4, 1, 2), at=(5, 6, 2, 3), rn=(8, 9), rt=(7, 6)),      # column's reference position is 6, which no alignment gives
      pos(5, "v", 3, 6, an=(9, 9, 9, 9), at=(9, 9, 9, 9), rn=(2, 3), rt=(4, 1))], {0: _EXT3}, False, None, GO, "v"),
    ("delete_as_aligned", "ACGTGGACGT", "ACGT--ACGT",                     # what an alignment gives (position 5): no arm fires, only the strings grow
     [pos(4, "v", 3, 4, an=(3, 4, 1, 2), at=(5, 6, 2, 3), rn=(8, 9), rt=(7, 6)), pos(5, "v", 3, 5, an=(9, 9, 9, 9), at=(9, 9, 9, 9), rn=(2, 3), rt=(4, 1))],
     {0: _EXT3}, False, None, GO, "v"),
    ("delete_not_adjacent", "ACGTGAGACGT", "ACGT-A-ACGT",                 # a match between the two: the second opens a transcript of its own
     [pos(4, "v", 3, 4, an=(3, 4, 1, 2), at=(5, 6, 2, 3), rn=(8, 9), rt=(7, 6)), pos(6, "v", 4, 6, an=(1, 2, 3, 4), at=(4, 3, 2, 1), rn=(2, 3), rt=(4, 1))],
     {0: _EXT3, 1: _EXT3[:1]}, False, None, GO, "vv"),
    ("x_after_x", "ACGTACGT", "ACGTTAGT", [_X(4), pos(5, "x", 5, 5, an=(1, 9, 0, 7), at=(2, 2, 2, 2), rn=(3, 30), rt=(1, 40))], {0: _EXT3}, False, None, GO, "c"),
    ("ins_after_del", "ACGTG-ACGT", "ACGT-CACGT",                         # t.code != code
     [pos(4, "v", 3, 4, an=(3, 4, 1, 2), at=(5, 6, 2, 3), rn=(8, 9), rt=(7, 6)), pos(5, "^", 4, 5, an=(2, 5, 1, 1), at=(4, 7, 2, 2), rn=(6, 1), rt=(1, 5))],
     {0: _EXT3}, False, None, GO, "c"),
    # nothing but gaps before the column in one string: that string has a gap in column 0, so column 0 is listed and is where it shows
    ("first_column_ins", "-ACGT", "GACGT", [pos(0, "^", 0, 0)], {}, False, None, OVF, ""),            # the reference's assert(pr >= 0)
    ("first_column_del", "GACGT", "-ACGT", [pos(0, "v", -1, 0, p_outside=False)], {}, False, None, OVF, ""),
    ("p_outside", A, "ACGTTCGTAC", [pos(4, "x", -1, 4, p_outside=True)], {}, False, None, OVF, ""),
    ("no_spanner_third", "AAAAAAA", "ACACACA", [_X(1), _X(3), _X(5, no_spanner=True)], {}, False, None, END, "xx"),
    ("no_spanner_in_extension", "ACGT--ACGT", "ACGTGGACGT",               # the loop over j is left before the reference's side of that position
     [pos(4, "^", 4, 4, an=(3, 4, 1, 2), at=(5, 6, 2, 3), rn=(8, 9), rt=(7, 6))], {0: [_EXT3[0], pos(1, "\0", 6, 0, no_spanner=True, rn=(1, 1), rt=(1, 1)), _EXT3[1]]}, False, None, GO, "^"),
    ("maxts_exact", *_many_aln(64), _many(64), {}, False, None, GO, "x" * 64),
    ("maxts_plus_one", *_many_aln(65), _many(65), {}, False, None, OVF, ""),
    ("staging_area_full", *_many_aln(4), _many(4), {}, False, 3, FULL, ""),
    ("staging_area_exact", *_many_aln(3), _many(3), {}, False, 3, GO, "xxx"),
    ("u16_sum_wraps", "ACGTACGT", "ACGTTAGT",                             # 40000 + 30000 in 16 bits; somatic, so the wrapped sum shows in the mean
     [pos(4, "x", 4, 4, an=(1, 1, 1, 1), at=(2, 2, 2, 2), rn=(40000, 65535), rt=(40000, 1), tumor=True), pos(5, "x", 5, 5, an=(1, 1, 1, 1), at=(2, 2, 2, 2), rn=(30000, 2), rt=(30000, 65535))],
     {0: _EXT3}, False, None, GO, "c"),
    ("somatic_by_extension", "ACGT--ACGT", "ACGTGGACGT",                  # means of the reference's side, ACNF = ACNR = 0
     [pos(4, "^", 4, 4, an=(3, 4, 1, 2), at=(5, 6, 2, 3), rn=(8, 9), rt=(7, 6))], {0: [_EXT3[0], dict(_EXT3[1], tumor=True), _EXT3[2]]}, False, None, GO, "^"),
    ("zero_and_nonzero_minimum", "ACGT--ACGT", "ACGTGGACGT",              # fwd: 3, 0, 2 -> minimum 0, non-zero minimum 2; rev: 0 first, then 4, 0 -> both stay 0
     [pos(4, "^", 4, 4, an=(3, 0, 1, 2), at=(5, 6, 2, 3), rn=(8, 9), rt=(7, 6))], {0: _EXT3}, False, None, GO, "^"),
    ("linked_reads_indel", "ACGT--ACGT", "ACGTGGACGT",
     [pos(4, "^", 4, 4, an=(3, 4, 1, 2), at=(5, 6, 2, 3), rn=(8, 9), rt=(7, 6), hp_an=(4, 5, 6), hq_an=(1, 2, 3), hp_at=(7, 8, 9), hq_at=(3, 2, 1), hp_rn=(10, 11, 12), hp_rt=(13, 14, 15)),
      pos(5, "^", 5, 4, an=(2, 5, 1, 1), at=(4, 7, 2, 2), rn=(1, 1), rt=(1, 1), hp_an=(3, 6, 6), hq_an=(0, 9, 3), hp_at=(8, 7, 9), hq_at=(4, 1, 1), hp_rn=(1, 1, 1), hp_rt=(1, 1, 1))],
     {0: [dict(_EXT3[0], hp_an=(9, 1, 9), hq_an=(5, 5, 5), hp_at=(1, 9, 9), hq_at=(6, 6, 6), hp_rn=(2, 40000, 3), hp_rt=(65535, 2, 2)), dict(_EXT3[2], hp_rn=(5, 30000, 1), hp_rt=(3, 3, 0))]},
     True, None, GO, "^"),
    ("linked_reads_snv_somatic", A, "ACGTTCGTAC",                         # 'x': the minqv haplotype counts; somatic: means, HPAN = 0
     [pos(4, "x", 4, 4, an=(3, 4, 1, 2), at=(5, 6, 2, 3), rn=(8, 9), rt=(7, 6), tumor=True, hp_an=(4, 5, 6), hq_an=(1, 2, 3), hp_at=(7, 8, 9), hq_at=(3, 2, 1), hp_rn=(10, 11, 12), hp_rt=(13, 14, 15))],
     {}, True, None, GO, "x"),
    ("linked_reads_complex_somatic", "ACGTACGT", "ACGTTAGT",
     [pos(4, "x", 4, 4, an=(3, 4, 1, 2), at=(5, 6, 2, 3), rn=(8, 9), rt=(7, 6), hp_an=(4, 5, 6), hq_an=(1, 2, 3), hp_at=(7, 8, 9), hq_at=(3, 2, 1), hp_rn=(10, 11, 12), hp_rt=(13, 14, 15)),
      pos(5, "x", 5, 5, an=(2, 2, 2, 2), at=(1, 1, 1, 1), rn=(3, 3), rt=(4, 4), tumor=True, hp_an=(1, 9, 9), hq_an=(9, 1, 9), hp_at=(9, 9, 1), hq_at=(1, 9, 9), hp_rn=(60000, 3, 4), hp_rt=(7, 7, 60000))],
     {0: [dict(_EXT3[0], hp_rn=(6000, 1, 1), hp_rt=(2, 2, 6000))]}, True, None, GO, "c"),
]


@pytest.mark.parametrize("case", LISTS, ids=[c[0] for c in LISTS])
def test_rules_equal_the_model_of_the_reference(rules, case):
    name, ra, pa, cols, ext, lr, cap, want_status, want_codes = case
    maxts = rules.lancet_emu_transcript_maxts()
    cap = maxts if cap is None else cap
    status, nts, ts = run_kernel_rules(rules, cols, ext, ra, pa, cap, lr)
    m_status, m_nts, m_ts = model(cols, ext, ra, pa, cap, lr, maxts)
    assert m_status == want_status and status == m_status                      # the list does what it was made for, and the rule says the same
    assert nts == m_nts
    if ts is not None:
        assert "".join(chr(t[7]) for t in m_ts) == want_codes
        for ti, (got, want) in enumerate(zip(ts, m_ts)):
            assert got == want, (name, ti, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w])


def test_the_lists_show_what_they_are_named_for(rules):
    """By eye, on the model's side: the figures each list was made to produce."""
    maxts = rules.lancet_emu_transcript_maxts()

    def dump(name):
        _, ra, pa, cols, ext, lr, _, _, _ = next(c for c in LISTS if c[0] == name)
        return model(cols, ext, ra, pa, maxts, lr, maxts)[2][0]

    cov8 = lambda name: dump(name)[-20:-12]
    assert cov8("u16_sum_wraps")[0] == ((40000 + 30000 + 3 + 1 + 7) & U16) // 5         # RCNF: the mean of a sum that wrapped
    assert cov8("somatic_by_extension")[4:6] == [0, 0]                                  # ACNF = ACNR = 0
    assert cov8("zero_and_nonzero_minimum")[4:6] == [2, 0]                              # non-zero minimum 2 beside a minimum of 0 ; a first value of 0 stays
    assert cov8("delete_extended")[0] == 1 and cov8("delete_as_aligned")[0] == 1        # RCNF: min(8, 2, 3, 1, 7) and min(8, 3, 1, 7)
    n_ref = 11 + 8 * 7 + 6                                                              # the count of the reference's side (normal, fwd)
    assert dump("delete_extended")[n_ref] == dump("delete_as_aligned")[n_ref] + 1       # the extended delete took one value more
