"""Fixtures of -V / --more-verbose: tests/golden/more_verbose/* (tools/make_more_verbose_goldens.py), written by the reference itself.
They live beside, not among, the cases golden_util.py collects."""
from __future__ import annotations

import functools
import gzip
import json
import os
import re

import numpy as np

import golden_util as gu
from lancet_amd import frontend
from lancet_amd.synth import SamRead

DIR = os.path.join(gu.GOLDEN, "more_verbose")
CASES = sorted(f[:-5] for f in os.listdir(DIR) if f.endswith(".json"))
_KEYS = ("qname", "flag", "pos", "mapq", "cigar", "seq", "qual", "as", "xs", "md")
# the lines only -V prints (tools/make_more_verbose_goldens.py V_PREFIXES)
V_PREFIXES = ("cycle detected in read ", "refid: ", "Looking at ", "checking for other ", "  removing node ", "alignment", "r:  ", "p:  ")


def meta(name: str) -> dict:
    """The case's json; `flags` without the switches golden_util's helpers do not pair with a value (recovery is in `recovery`)."""
    m = json.load(open(os.path.join(DIR, f"{name}.json")))
    m["recovery"] = "--kmer-recovery" in m["flags"]
    m["flags"] = [f for f in m["flags"] if f != "--kmer-recovery"]
    return m


def digest(text: str) -> str:
    """golden_util.digest_trace's lines plus the -V lines, in order (what the generator kept of the reference's stderr)."""
    return "\n".join(l.rstrip() for l in text.splitlines() if l.startswith(V_PREFIXES) or gu._DIGEST.match(l)) + "\n"


def digest_v(text: str) -> str:
    """The -v part of a digest: what a run without -V prints."""
    return "\n".join(l.rstrip() for l in text.splitlines() if not l.startswith(V_PREFIXES) and gu._DIGEST.match(l)) + "\n"


@functools.lru_cache(maxsize=None)
def case_batch(name: str):
    """(meta, window batch, kept windows) of a case, made the way golden_util.case_batch makes them."""
    m = meta(name)
    z = np.load(os.path.join(DIR, f"{name}.reads.npz"))
    ref, rname = str(z["ref"]), str(z["rname"])
    reads = {}
    for rg in ("tumor", "normal"):
        a = {k: z[f"{rg}_{k}"].tolist() for k in _KEYS}
        reads[rg] = [SamRead(a["qname"][i], a["flag"][i], rname, a["pos"][i], a["mapq"][i], a["cigar"][i], a["seq"][i], a["qual"][i],
                             {"AS": a["as"][i], "XS": a["xs"][i], "MD": a["md"][i]}) for i in range(len(a["qname"]))]
        if f"{rg}_bx" in z.files:
            bx, hp = z[f"{rg}_bx"].tolist(), z[f"{rg}_hp"].tolist()
            for i, r in enumerate(reads[rg]):
                if bx[i] != "":
                    r.tags["BX"] = bx[i]
                if hp[i] >= 0:
                    r.tags["HP"] = hp[i]
    padding, _, max_k = gu.case_params(m)
    windows = frontend.tile_region(ref, rname, m["region"], padding=padding, window_size=gu.case_window(m))
    batch, kept = frontend.batch_from_sam(windows, reads["tumor"], reads["normal"], max_k=max_k, linked=gu.case_lr(m),
                                          active_region=gu.case_active_region(m))
    return m, batch, kept


def params(m: dict, **over):
    return gu.params(m, kmer_recovery=1 if m["recovery"] else 0, **over)


def golden_vcf(name: str, full: bool = False) -> str:
    return open(os.path.join(DIR, f"{name}.{'full.' if full else ''}vcf")).read()


def golden_trace(name: str, level: str = "V") -> str:
    """level "V": the digest of the reference's -V stderr; "v" (the command-line case only): of its -v stderr."""
    return gzip.open(os.path.join(DIR, f"{name}.{level}.trace.txt.gz"), "rt").read()


def trace_words(batch, p, paths: int = 32) -> int:
    """Trace words per window for a level-2 run, sized from the batch as lancet_gpu sizes them (lancet_main.cc trace_words_for): 512 words,
    `paths` path strings of (longest window reference + --max-indel-len + 256) bases at a quarter word per base (+ event and padding), 16 words
    per reference base for the cycle lines; a multiple of 8."""
    longest = max(int(batch.ref_off[w + 1] - batch.ref_off[w]) for w in range(batch.n_windows)) if batch.n_windows else 0
    return (512 + paths * ((longest + int(p.max_indel_len) + 256 + 3) // 4 + 16) + 16 * longest + 7) // 8 * 8


def records_vcf(batch, variants, lr: bool = False, bx_names=None) -> str:
    """VCF (without ##fileDate / ##cmdline / ##reference) of a run's records, through the restatement of VariantDB the other parity tests use."""
    from oracle import vcf_oracle
    db = vcf_oracle.VariantDB(lr=lr)
    for rec in variants:
        db.add(vcf_oracle.Variant(batch.chrom[rec["window"]], rec, lr=lr, bx_names=bx_names))
    return db.vcf()


_TS = re.compile(r" (\d+):([ACGTN-]+)\|([ACGTN-]+)\|")


def window_texts(batch, events, words_per_window, p):
    """Per window, the level-2 text of its raw event words (lancet_amd.trace.format_window2)."""
    from lancet_amd import trace
    out = []
    for w in range(batch.n_windows):
        raw = bytes(batch.ref_bases[int(batch.ref_off[w]):int(batch.ref_off[w + 1])]).decode()
        end = int(batch.ref_start[w]) + len(raw)
        out.append(trace.format_window2(events[w], words_per_window, w + 1, batch.hdr[w], batch.chrom[w], int(batch.ref_start[w]), end,
                                        dfs_limit=int(p.dfs_limit), rawseq=raw))
    return out


def replay_paths(text: str):
    """For every path of a -V text: (its p: line, what the transcripts of its `>p_` line make of its r: line).  A transcript
    ` <pos>:<ref>|<qry>|...` starts at offset pos - (window start + trim5) of r (reference src/Graph.cc:977: rrpos = pos_in_ref + refstart + trim5,
    trim5 as the last `ref trim5:` line printed it) and puts qry without its '-' in place of ref without its '-'."""
    out = []
    start = trim5 = r = p = None
    for l in text.splitlines():
        if l.startswith("== Processing"):
            start = int(re.match(r"== Processing \d+: \S+:(\d+)-", l).group(1))
        elif l.startswith("ref trim5: "):
            trim5 = int(l.split()[2])
        elif l.startswith("r:  "):
            r = l[4:]
        elif l.startswith("p:  "):
            p = l[4:]
        elif l.startswith(">p_"):
            made, at = [], 0
            for m in _TS.finditer(l):
                o = int(m.group(1)) - start - trim5
                ref, qry = m.group(2).replace("-", ""), m.group(3).replace("-", "")
                assert o >= at and r[o:o + len(ref)] == ref, l[:120]
                made += [r[at:o], qry]
                at = o + len(ref)
            out.append((p, "".join(made) + r[at:]))
            p = None
    return out
