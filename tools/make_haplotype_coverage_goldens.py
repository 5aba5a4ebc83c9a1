#!/usr/bin/env python3
"""Generates tests/golden/hap_cov/*: the coverage tables the REFERENCE ITSELF prints for every path under -V.

Graph_t::printVerticalAlignment (reference src/Graph.cc:749-783) writes, for every processPath call, the line
`Pos  r  p  d  an+ an- at+ at- rn+ rn- rt+ rt-` and one row per alignment column: the path's normal / tumour coverage per strand at
its position and the reference's at its position.  tools/make_golden.py digest_trace drops these lines, so the -V fixtures of
tests/golden/more_verbose/ do not have them.  This tool runs the same unmodified reference binary (tools/REFERENCE_BUILD.md) with -V
on the same five inputs (tools/make_more_verbose_goldens.py CASES; the reads are regenerated from the committed synth parameters),
asserts that the `r:  ` / `p:  ` lines of the run are those of the committed <case>.V.trace.txt.gz -- the same run -- and stores

  tests/golden/hap_cov/<case>.tables.txt.gz      per processPath call, in order: the `Pos...` line and its rows exactly as printed

Usage:  python tools/make_haplotype_coverage_goldens.py [case ...]
"""
from __future__ import annotations

import gzip
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden as mg  # noqa: E402
import make_more_verbose_goldens as mv  # noqa: E402
from lancet_amd import synth  # noqa: E402

OUT = os.path.join(mg.GOLDEN, "hap_cov")
HEADER = "Pos\tr\tp\td\tan+\tan-\tat+\tat-\trn+\trn-\trt+\trt-"
ROW = re.compile(r"^\d+\t[ACGTN-]\t[ACGTN-]\t[ xv^]\t")


def tables_of(stderr: str):
    """[(r, p, [row, ...])] per processPath call of a -V stderr: the strings of its r: / p: lines and the rows below its Pos line."""
    out, r, p = [], None, None
    lines = stderr.splitlines()
    i = 0
    while i < len(lines):
        l = lines[i]
        if l.startswith("r:  "):
            r = l[4:]
        elif l.startswith("p:  "):
            p = l[4:]
        elif l == HEADER:
            rows = []
            while i + 1 < len(lines) and ROW.match(lines[i + 1]):
                rows.append(lines[i + 1])
                i += 1
            out.append((r, p, rows))
        i += 1
    return out


def parse_tables(text: str):
    """The stored file back into [[row fields, ...], ...]: one list of rows per table, each row its 12 tab-separated cells."""
    tabs = []
    for l in text.splitlines():
        if l == HEADER:
            tabs.append([])
        else:
            tabs[-1].append(l.split("\t"))
    return tabs


def run_case(name: str) -> str:
    kwargs, region, flags, cli = mv.CASES[name]
    data = synth.make_tumor_normal(**kwargs)
    ref, rname = data["ref"], data["rname"]
    with tempfile.TemporaryDirectory(prefix="lancet_hap_cov_") as td:
        synth.write_fasta(os.path.join(td, "ref.fa"), rname, ref)
        for sample, rg, pairs in (("TUMOR", "tumor", data["tumor"]), ("NORMAL", "normal", data["normal"])):
            sam = os.path.join(td, f"{rg}.sam")
            synth.write_sam(sam, rname, len(ref), sample, rg, pairs)
            mg.run([mg.TEST_VIEW, "-b", "-p", os.path.join(td, f"{rg}.bam"), sam], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            mg.run([mg.BAMTOOLS, "index", "-in", os.path.join(td, f"{rg}.bam")])
        cmd = [mg.REF_BIN, "--tumor", "tumor.bam", "--normal", "normal.bam", "--ref", "ref.fa", "--reg", region, "--num-threads", "1"] + \
              ([] if cli else ["--active-region-off"]) + flags + ["-V"]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=td, errors="replace")
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-3000:])
            raise SystemExit(f"reference failed on case {name}")
    return r.stderr


def make_case(name: str) -> dict:
    err = run_case(name)
    with gzip.open(os.path.join(mv.OUT, f"{name}.V.trace.txt.gz"), "rt") as f:
        committed = [l for l in f.read().splitlines() if l.startswith(("r:  ", "p:  "))]
    mine = [l.rstrip() for l in err.splitlines() if l.startswith(("r:  ", "p:  "))]
    if mine != committed:
        raise SystemExit(f"{name}: the r: / p: lines of this run are not those of the committed -V trace")
    tabs = tables_of(err)
    if 2 * len(tabs) != len(committed):
        raise SystemExit(f"{name}: {len(tabs)} tables for {len(committed) // 2} processPath calls")
    for r, p, rows in tabs:
        if sum(1 for x in rows if x.split("\t")[1] != "-") != len(r) or sum(1 for x in rows if x.split("\t")[2] != "-") != len(p):
            raise SystemExit(f"{name}: a table's rows do not spell its r: / p: lines")
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"{name}.tables.txt.gz")
    mv.write_gz(path, "".join(HEADER + "\n" + "".join(x + "\n" for x in rows) for _, _, rows in tabs))
    n = counts(tabs)
    print(f"{name}: {n}; {os.path.getsize(path)} bytes")
    return n


def counts(tabs) -> dict:
    """What check_set asks of the set, counted per case."""
    n = {"aligned": 0, "hamming": 0, "ref_spelling": 0, "ins_cols": 0, "del_cols": 0, "strand_rows": 0, "ref_strand_rows": 0}
    for r, p, rows in tabs:
        if len(p) != len(r):
            n["aligned"] += 1
        elif p == r:
            n["ref_spelling"] += 1
        elif sum(a != b for a, b in zip(p, r)) <= 5:
            n["hamming"] += 1
        else:
            n["aligned"] += 1
        for x in rows:
            c = x.split("\t")
            n["ins_cols"] += c[3] == "^"
            n["del_cols"] += c[3] == "v"
            n["strand_rows"] += c[3] != "v" and (c[4] != c[5] or c[6] != c[7])
            n["ref_strand_rows"] += c[3] != "^" and (c[8] != c[9] or c[10] != c[11])
    return n


def stretch_offsets(name: str):
    """ref_off of every path of the committed trace: the `ref trim5:` line (src/Graph.cc:2145) that precedes its p: line."""
    off, cur = [], 0
    with gzip.open(os.path.join(mv.OUT, f"{name}.V.trace.txt.gz"), "rt") as f:
        for l in f.read().splitlines():
            m = re.match(r"ref trim5: (\d+)", l)
            if m:
                cur = int(m.group(1))
            elif l.startswith("p:  "):
                off.append(cur)
    return off


def check_set(per_case: dict) -> None:
    """Conditions on the reference's own output, not measurements of the engine."""
    tot = {k: sum(n[k] for n in per_case.values()) for k in next(iter(per_case.values()))}
    for k, least, what in (("aligned", 20, "aligned paths"), ("hamming", 20, "paths of the Hamming short-cut"), ("ref_spelling", 50, "reference-spelling paths"),
                           ("ins_cols", 1, "insertion columns"), ("del_cols", 1, "deletion columns"),
                           ("strand_rows", 1, "rows with an+ != an- or at+ != at-")):
        if tot[k] < least:
            raise SystemExit(f"{tot[k]} {what} in the set ({least} at least)")
    if not any(o > 0 for c in per_case for o in stretch_offsets(c)):
        raise SystemExit("no path whose stretch has ref_off > 0")
    for f in os.listdir(OUT):
        if os.path.getsize(os.path.join(OUT, f)) > (1 << 20):
            raise SystemExit(f"{f} is larger than 1 MiB")
    print("set ok:", tot)


if __name__ == "__main__":
    mg.check_reference_is_unmodified()
    done = {c: make_case(c) for c in (sys.argv[1:] or list(mv.CASES))}
    if not sys.argv[1:]:
        check_set(done)
