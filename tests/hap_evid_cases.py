"""Shared by test_haplotype_evidence_emu.py / test_haplotype_evidence_gpu.py: what a run with the variant evidence
(lancet_engine_set_haplotype_evidence) has to return.  There is no reference value for the quantity: include/lancet_engine.h defines it, and
model() below restates that definition as plain loops over strings and lists -- it shares nothing with the kernel (no packed words, no
masks, no lanes, no entry buffers) and nothing with abi.py's join.  The hand-made windows carry numbers that are known from how their reads
were cut, not from the model.  A haplotype is one of abi.haplotypes_to_py's dicts with "cigar" and "events"."""
from __future__ import annotations

import hap_place_cases as pc
import hap_sup_cases as sc
from hap_sup_cases import _OTHER, _rand, _sub  # noqa: F401

ENTS, EVENTS = 32, 64                 # LANCET_EVID_GROUP_ENTRIES, LANCET_EVID_GROUP_EVENTS
UNEVALUATED = 1                       # LANCET_EVID_UNEVALUATED
KEYS = ("rb", "rs", "pb", "ps", "flags", "alt", "ref", "other")


# ---------------------------------------------------------------- the definition, restated

def events_of(cigar) -> list:
    """[(rb, rs, pb, ps)] of an entry: its maximal runs of CIGAR pairs whose op is not '='."""
    out, rb, pb, cur = [], 0, 0, None
    for n, op in cigar:
        if op == "=":
            if cur:
                out.append(tuple(cur))
                cur = None
        else:
            if cur is None:
                cur = [rb, 0, pb, 0]
            cur[1] += n if op in "DX" else 0
            cur[3] += n if op in "IX" else 0
        rb += n if op != "I" else 0
        pb += n if op != "D" else 0
    if cur:
        out.append(tuple(cur))
    return out


def stand(e, bases: str, evs2, seq2: str):
    """(class, left, right): how an entry with the events evs2 and the path seq2 stands to the event e whose path bases are `bases`."""
    rb, rs, pb, ps = e
    touch = [x for x in evs2 if x[0] <= rb + rs and x[0] + x[1] >= rb]
    if not touch:
        cls = "ref"
    elif len(touch) == 1 and (touch[0][0], touch[0][1], touch[0][3]) == (rb, rs, ps) and seq2[touch[0][2]:touch[0][2] + ps] == bases:
        cls = "alt"
    else:
        cls = "other"
    lo = min([rb] + [x[0] for x in touch])
    hi = max([rb + rs] + [x[0] + x[1] for x in touch])
    shift = sum(x[3] - x[1] for x in evs2 if x not in touch and x[0] + x[1] <= lo)
    return cls, lo + shift, hi + shift + sum(x[3] - x[1] for x in touch)


def model_group(entries, reads, max_mm: int) -> list:
    """Per entry of one group the list of its events' dicts (KEYS).  entries: [(path string, k, [(n, op)])]; reads: [(string, class)]."""
    evs = [events_of(c) for _, _, c in entries]
    out = [[dict(rb=e[0], rs=e[1], pb=e[2], ps=e[3], flags=0, alt=[0] * 4, ref=[0] * 4, other=[0] * 4) for e in ev] for ev in evs]
    if len(entries) > ENTS or sum(len(e) for e in evs) > EVENTS:
        for ev in out:
            for d in ev:
                d["flags"] = UNEVALUATED
        return out
    table = {}
    for i, (seq, _, _) in enumerate(entries):
        for j, e in enumerate(evs[i]):
            for i2, (seq2, _, _) in enumerate(entries):
                table[i, j, i2] = stand(e, seq[e[2]:e[2] + e[3]], evs[i2], seq2)
    for read, rc in reads:
        got = [pc.place_one(read, seq, k) if read else None for seq, k, _ in entries]
        have = [g[0] for g in got if g is not None]
        if not have or min(have) > max_mm:
            continue
        best = [i2 for i2, g in enumerate(got) if g is not None and g[0] == min(have)]
        for i in range(len(entries)):
            for j in range(len(evs[i])):
                on = set()
                for i2 in best:
                    cls, left, right = table[i, j, i2]
                    o, t, m = got[i2][1], len(read), len(entries[i2][0])
                    if left >= 1 and right + 1 <= m and o <= left - 1 and o + t >= right + 1:
                        on.add(cls)
                if on:
                    out[i][j]["alt" if on == {"alt"} else ("ref" if on == {"ref"} else "other")][rc] += 1
    return out


def model(batch, p, haps, max_mm: int) -> list:
    """Per haplotype, in order, the list of its events' dicts."""
    out = [None] * len(haps)
    byw = {}
    for i, h in enumerate(haps):
        byw.setdefault(h["window"], {}).setdefault((h["kmer"], h["component"]), []).append(i)
    for w, groups in byw.items():
        reads = sc.trimmed_reads(batch, p, w)
        for (k, _), members in groups.items():
            assert members == list(range(members[0], members[0] + len(members)))          # a group is a run of entries
            for i, ev in zip(members, model_group([(haps[i]["seq"], k, haps[i]["cigar"]) for i in members], reads, max_mm)):
                out[i] = ev
    return out


def strip(events) -> list:
    return [{k: e[k] for k in KEYS} for e in events]


def check_model(batch, p, haps, max_mm: int, cap: int = None):
    """Every event of every haplotype against the model; cap: the records a window keeps (the first ones, whole)."""
    want = model(batch, p, haps, max_mm)
    kept = {}
    for h, x in zip(haps, want):
        n = kept.get(h["window"], 0)
        room = len(x) if cap is None else max(0, min(len(x), cap - n))
        assert strip(h["events"]) == x[:room], (h["window"], h["index"], h["cigar"], strip(h["events"]), x[:room])
        kept[h["window"]] = n + len(x)
    return want, kept


def check_invariants(haps, with_support: bool):
    """Item 3 of the issue: events of two entries of a group with equal (rb, rs, ps, bases) have equal counts; the events' spans plus the '='
    lengths give len and ref_len; per event and class alt <= `fit` (support on at the same limit).
    The last one holds as the issue states it -- against the event's own entry -- where that entry is the group's only ALT carrier of the
    event.  Where several entries carry it the definition itself, and the invariant of equal counts, make a read that fits only ANOTHER carrier
    count alt for this entry's event too (more_verbose fixture mv_nref, window 0, entry 0, the event at rb 313: alt Tr = 8, the entry's own
    fit Tr = 6).  What the definition implies there: every read that counts alt fits at least one ALT carrier, so alt <= the sum of the
    carriers' fit.  That is what is asserted; with one carrier it is the issue's bound."""
    same = {}
    groups = {}
    for h in haps:
        groups.setdefault((h["window"], h["kmer"], h["component"]), []).append(h)
    for h in haps:
        eq = sum(n for n, op in h["cigar"] if op == "=")
        assert eq + sum(e["ps"] for e in h["events"]) == h["len"] and eq + sum(e["rs"] for e in h["events"]) == h["ref_len"], (h["window"], h["index"])
        for e in h["events"]:
            if with_support and not e["flags"]:
                ev = (e["rb"], e["rs"], e["pb"], e["ps"])
                carriers = [g for g in groups[h["window"], h["kmer"], h["component"]]
                            if stand(ev, h["seq"][e["pb"]:e["pb"] + e["ps"]], events_of(g["cigar"]), g["seq"])[0] == "alt"]
                assert any(g is h for g in carriers)
                bound = [sum(g["support"]["fit"][c] for g in carriers) for c in range(4)]
                assert all(a <= f for a, f in zip(e["alt"], bound)), (h["window"], h["index"], e, bound, len(carriers))
            key = (h["window"], h["kmer"], h["component"], e["rb"], e["rs"], e["ps"], h["seq"][e["pb"]:e["pb"] + e["ps"]])
            counts = (e["alt"], e["ref"], e["other"], e["flags"])
            assert same.setdefault(key, counts) == counts, (key, counts, same[key])


def check_join(batch, haps, variants, marked, join=None):
    """Item 2: every record's ref and alt strings without '-' are the stretch bases [rb, rb + rs) and the path bases [pb, pb + ps) of the event
    it is joined to; every haplotype's n_variants records are joined, each to another event (but in a marked window, which lost events).  join: a second statement of the rule to hold
    `variant` to as well (abi.evidence_variant)."""
    for h in haps:
        w = h["window"]
        ref = bytes(batch.ref_bases[int(batch.ref_off[w]):int(batch.ref_off[w + 1])]).decode()
        stretch = ref[h["ref_off"]:h["ref_off"] + h["ref_len"]]
        joined = [e["variant"] for e in h["events"] if e["variant"] >= 0]
        assert len(set(joined)) == len(joined)
        if not marked[w]:
            assert sorted(variants[i]["seq"] for i in joined) == list(range(h["first_variant"], h["first_variant"] + h["n_variants"])), (w, h["index"], joined)
        for e in h["events"]:
            if join is not None:
                assert e["variant"] == join(h, e["rb"], int(batch.ref_start[w]), variants), (w, h["index"], e)
            if e["variant"] >= 0:
                v = variants[e["variant"]]
                assert v["window"] == w and v["kmer"] == h["kmer"]
                assert v["ref"].replace("-", "") == stretch[e["rb"]:e["rb"] + e["rs"]], (v, e)
                assert v["alt"].replace("-", "") == h["seq"][e["pb"]:e["pb"] + e["ps"]], (v, e)


# ---------------------------------------------------------------- counts known without the model

def check_basic(variant, batch, st, haps, trunc, marked):
    """sc.basic_batch: first that the window assembled into exactly the two paths, in one group, then: the reference path has no event; the alt
    path has one, the planted one, with alt = the tumour reads cut from the alt allele over the site ([5, 4, 0, 0]), ref = the reads cut from
    the reference over it ([2, 3, 4, 6]) and other = 0 -- every one of those reads has at least 20 own bases on either side of SITE.  The
    end reads and the three overhanging ones do not reach the site and count nothing."""
    _, _, alt, ref, _ = sc.basic_batch(variant)
    assert all(s["status"] == 0 for s in st) and not any(trunc) and not any(marked)
    assert sorted(h["seq"] for h in haps) == sorted([alt, ref]) and len({(h["kmer"], h["component"]) for h in haps}) == 1
    (hr,) = [h for h in haps if h["seq"] == ref]
    (ha,) = [h for h in haps if h["seq"] == alt]
    assert hr["events"] == [] and len(ha["events"]) == 1
    (e,) = ha["events"]
    if variant == "snv":
        assert (e["rb"], e["rs"], e["pb"], e["ps"]) == (sc.SITE, 1, sc.SITE, 1)
    else:
        assert (e["rs"], e["ps"]) == (3, 0) and abs(e["rb"] - sc.SITE) <= 19, e       # (the aligner may shift the deletion inside a repeat; the reads keep 20 bases)
    fa, fr = sc.OVER[(sc.TMR, True)]
    tf, tr = sc.OVER[(sc.TMR, False)]
    nf, nr = sc.OVER[(sc.NML, False)]
    assert e["flags"] == 0 and e["alt"] == [fa, fr, 0, 0] and e["ref"] == [tf, tr, nf, nr] and e["other"] == [0] * 4, e
    assert e["variant"] >= 0


# ---------------------------------------------------------------- hand-written windows (the emulator's call)

def edit(ref: str, edits):
    """(path string, [(n, op)]): ref with edits applied, and the path's CIGAR against it.  edits, ascending and apart or touching:
    (pos, "X", base) / (pos, "I", bases) in front of ref[pos] / (pos, "D", n)."""
    path, cols, at = [], [], 0
    for pos, op, arg in edits:
        path.append(ref[at:pos]); cols += ["="] * (pos - at); at = pos
        if op == "X":
            assert arg != ref[pos]
            path.append(arg); cols.append("X"); at += 1
        elif op == "I":
            path.append(arg); cols += ["I"] * len(arg)
        else:
            cols += ["D"] * arg; at += arg
    path.append(ref[at:]); cols += ["="] * (len(ref) - at)
    cigar = []
    for c in cols:
        if cigar and cigar[-1][1] == c:
            cigar[-1][0] += 1
        else:
            cigar.append([1, c])
    return "".join(path), [(n, op) for n, op in cigar]


def entry(ref: str, edits, k: int = 15, comp: int = 0):
    s, c = edit(ref, edits)
    return (s, k, comp, c)


def model_hand(entries, reads, max_mm: int) -> list:
    """Per entry the events' dicts; the groups are the runs of entries with one (k, component)."""
    out, i = [], 0
    while i < len(entries):
        j = i
        while j < len(entries) and entries[j][1:3] == entries[i][1:3]:
            j += 1
        out += model_group([(s, k, c) for s, k, _, c in entries[i:j]], reads, max_mm)
        i = j
    return out


def tile(hap: str, lo: int, hi: int, t: int = 40, step: int = 3, cls0: int = 0) -> list:
    """Reads of t bases cut from hap at lo, lo + step, ... (at most hi), their classes in turn."""
    return [(hap[s:s + t], (cls0 + n) & 3) for n, s in enumerate(range(max(0, lo), min(hi, len(hap) - t) + 1, step))]
