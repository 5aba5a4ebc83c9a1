#!/usr/bin/env python3
"""Generates tests/golden/more_verbose/*: what the REFERENCE ITSELF prints under -V / --more-verbose.

Same unmodified reference binary, same helper programs and the same check as tools/make_golden.py (tools/REFERENCE_BUILD.md).  The
fixtures live in their own directory, so that tests/golden_util.py (which turns every tests/golden/*.json into a case of the parity
tests) does not see them.  Per case:

  <case>.reads.npz          the simulated reads (SAM fields) + contig sequence (inputs)
  <case>.json               synth parameters, region, reference flags, counts of the -V lines
  <case>.vcf                the reference's VCF (no ##fileDate / ##cmdline / ##reference); -V does not change it
  <case>.V.trace.txt.gz     the digest of the reference's -V stderr (gzipped): the lines of make_golden.digest_trace plus the -V lines
  <case>.v.trace.txt.gz, .{tumor,normal}.bam, .fa, .full.vcf
                            (the case marked cli) the digest of the plain -v run, the inputs as files, and the VCF of the -V run whole but
                            for ##fileDate: the reference run from the directory that holds tumor.bam / normal.bam / ref.fa

The -V lines (reference src/Graph.cc:328-332, :539 / :2042, :2030-2034, :2168-2213, :800-802) print whole reads and whole paths, so the
cases are small: 8-20 windows at 6-30x.  The script itself checks what the set must cover (see check_set).

Usage:  python tools/make_more_verbose_goldens.py [case ...]
"""
from __future__ import annotations

import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden as mg  # noqa: E402
from lancet_amd import synth  # noqa: E402

OUT = os.path.join(mg.GOLDEN, "more_verbose")

V_PREFIXES = ("cycle detected in read ", "refid: ", "Looking at ", "checking for other ", "  removing node ", "alignment", "r:  ", "p:  ")

CASES = {
    # name: (synth kwargs, region, extra reference flags, keep the BAM / FASTA inputs for the command-line test)
    # a thin normal under a 7x tumour, as a user would type it (active regions on); the command-line fixture
    "mv_low": (dict(ref_len=3600, cov_t=7, cov_n=3, ref_seed=400, tumor_seed=500, normal_seed=600, error_rate=0.015,
                    somatic_every=350, germline_every=500), "chr22:900-2700", [], True),
    # duplications on 100-base reads: windows rebuilt at several k, reads that run through a k-mer twice
    "mv_dups": (dict(ref_len=3600, cov_t=6, cov_n=2, ref_seed=400, tumor_seed=500, normal_seed=600, error_rate=0.015, dup_prob=1.0,
                     somatic_every=350, germline_every=500, read_len=100), "chr22:900-2700", [], False),
    # N in the window reference: nodes identified by their strings
    "mv_nref": (dict(ref_len=3600, cov_t=12, cov_n=8, ref_seed=401, tumor_seed=501, normal_seed=601, error_rate=0.01,
                     somatic_every=350, germline_every=500, n_runs=((1410, 1), (1833, 3), (2305, 14))), "chr22:900-2700", [], False),
    # --linked-reads
    "mv_lr": (dict(ref_len=3600, cov_t=20, cov_n=16, ref_seed=61, tumor_seed=161, normal_seed=261, linked=True,
                   insert_mean=300.0, insert_sd=40.0, somatic_every=700, germline_every=600), "chr22:900-2400", ["--linked-reads"], False),
    # --kmer-recovery
    "mv_rec": (dict(ref_len=3600, cov_t=7, cov_n=3, ref_seed=402, tumor_seed=502, normal_seed=602, error_rate=0.015,
                    somatic_every=350, germline_every=500), "chr22:900-2400", ["--kmer-recovery"], False),
}


def digest_more_verbose(stderr: str) -> str:
    """The lines of make_golden.digest_trace plus the lines only -V prints, in the order the reference printed them."""
    keep = [line.rstrip() for line in stderr.splitlines() if line.startswith(V_PREFIXES) or mg.digest_trace(line) != "\n"]
    return "\n".join(keep) + "\n"


def _strip(vcf_text: str, keep_header: bool) -> str:
    drop = ("##fileDate",) if keep_header else ("##fileDate", "##cmdline", "##reference")
    return "".join(l + "\n" for l in vcf_text.splitlines() if not l.startswith(drop))


def write_gz(path: str, text: str) -> None:
    """(no name, no time stamp in the header: the same bytes every time)"""
    with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0, compresslevel=9) as f:
        f.write(text.encode())


def line_counts(digest: str) -> dict:
    """What check_set asks of the set, counted per case."""
    lines = digest.splitlines()
    n = {"cycle": 0, "before_source": 0, "after_sink": 0, "aligned": 0, "ref_spelling": 0, "mismatch_1_5": 0, "n_node": 0, "rebuilds": 0}
    r = None
    for l in lines:
        if l.startswith("cycle detected in read "):
            n["cycle"] += 1
        elif l.startswith("  removing node before source: "):
            n["before_source"] += 1
            n["n_node"] += "N" in l.split(": ", 1)[1]
        elif l.startswith("  removing node after sink: "):
            n["after_sink"] += 1
            n["n_node"] += "N" in l.split(": ", 1)[1]
        elif l.startswith("Cycle found") or l.startswith(" Found repeat in assembly"):
            n["rebuilds"] += 1
        elif l.startswith("r:  "):
            r = l[4:]
        elif l.startswith("p:  "):
            p = l[4:]
            if len(p) != len(r):
                n["aligned"] += 1
            elif p == r:
                n["ref_spelling"] += 1
            elif sum(a != b for a, b in zip(p, r)) <= 5:
                n["mismatch_1_5"] += 1
    return n


def make_case(name: str) -> dict:
    kwargs, region, flags, cli = CASES[name]
    data = synth.make_tumor_normal(**kwargs)
    ref, rname = data["ref"], data["rname"]
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory(prefix="lancet_more_verbose_") as td:
        synth.write_fasta(os.path.join(td, "ref.fa"), rname, ref)
        for sample, rg, pairs in (("TUMOR", "tumor", data["tumor"]), ("NORMAL", "normal", data["normal"])):
            sam = os.path.join(td, f"{rg}.sam")
            synth.write_sam(sam, rname, len(ref), sample, rg, pairs)
            mg.run([mg.TEST_VIEW, "-b", "-p", os.path.join(td, f"{rg}.bam"), sam], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            mg.run([mg.BAMTOOLS, "index", "-in", os.path.join(td, f"{rg}.bam")])
        base = [mg.REF_BIN, "--tumor", "tumor.bam", "--normal", "normal.bam", "--ref", "ref.fa", "--reg", region, "--num-threads", "1"] + \
               ([] if cli else ["--active-region-off"]) + flags
        runs = {}
        for tag, extra in (("V", ["-V"]), ("v", ["-v"])):
            r = subprocess.run(base + extra, capture_output=True, text=True, cwd=td, errors="replace")
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-3000:])
                raise SystemExit(f"reference failed on case {name} ({tag})")
            runs[tag] = (r.stdout, r.stderr)
        if cli:
            for rg in ("tumor", "normal"):
                shutil.copy(os.path.join(td, f"{rg}.bam"), os.path.join(OUT, f"{name}.{rg}.bam"))
            shutil.copy(os.path.join(td, "ref.fa"), os.path.join(OUT, f"{name}.fa"))
    vcf, err = runs["V"]
    if _strip(vcf, False) != _strip(runs["v"][0], False):
        raise SystemExit(f"{name}: -V changed the reference's VCF")
    digest = digest_more_verbose(err)
    if "".join(l + "\n" for l in digest.splitlines() if not l.startswith(V_PREFIXES)) != mg.digest_trace(runs["v"][1]):
        raise SystemExit(f"{name}: the -v lines of the -V run are not those of the -v run")
    with open(os.path.join(OUT, f"{name}.vcf"), "w") as f:
        f.write(_strip(vcf, False))
    write_gz(os.path.join(OUT, f"{name}.V.trace.txt.gz"), digest)
    if cli:
        write_gz(os.path.join(OUT, f"{name}.v.trace.txt.gz"), mg.digest_trace(runs["v"][1]))
        with open(os.path.join(OUT, f"{name}.full.vcf"), "w") as f:      # (##cmdline starts with argv[0]: the program as `lancet`, not where it was built)
            f.write(_strip(vcf, True).replace("##cmdline=" + mg.REF_BIN + " ", "##cmdline=lancet ", 1))
    reads = {}
    for rg in ("tumor", "normal"):
        rs = synth.pairs_to_sorted_reads(data[rg])
        for key, get, dt in (("qname", lambda x: x.qname, None), ("flag", lambda x: x.flag, np.int32), ("pos", lambda x: x.pos, np.int32),
                             ("mapq", lambda x: x.mapq, np.int32), ("cigar", lambda x: x.cigar, None), ("seq", lambda x: x.seq, None),
                             ("qual", lambda x: x.qual, None), ("as", lambda x: x.tags["AS"], np.int32), ("xs", lambda x: x.tags["XS"], np.int32),
                             ("md", lambda x: x.tags["MD"], None)):
            reads[f"{rg}_{key}"] = np.array([get(x) for x in rs], dtype=dt) if dt else np.array([get(x) for x in rs])
        if kwargs.get("linked"):
            reads[f"{rg}_bx"] = np.array([x.tags.get("BX", "") for x in rs])
            reads[f"{rg}_hp"] = np.array([x.tags.get("HP", -1) for x in rs], dtype=np.int32)
    np.savez_compressed(os.path.join(OUT, f"{name}.reads.npz"), ref=np.array(ref), rname=np.array(rname), **reads)
    info = {"synth": kwargs, "region": region, "flags": flags + (["--active-region-on"] if cli else []), "cli": cli,
            "reference_cmd": "lancet " + " ".join(base[1:]) + " -V",
            "n_vcf_records": sum(1 for l in vcf.splitlines() if not l.startswith("#")),
            "n_windows": sum(1 for l in digest.splitlines() if l.startswith("== Processing")), "lines": line_counts(digest)}
    with open(os.path.join(OUT, f"{name}.json"), "w") as f:
        json.dump(info, f, indent=1)
    print(f"{name}: {info['n_vcf_records']} records, {info['n_windows']} windows, {info['lines']}; "
          f"{len(reads['tumor_qname'])}+{len(reads['normal_qname'])} reads")
    return info


def check_set():
    """What the committed set must cover: conditions on the reference's own output, not measurements of the engine."""
    infos = {c: json.load(open(os.path.join(OUT, c + ".json"))) for c in CASES}
    tot = {k: sum(i["lines"][k] for i in infos.values()) for k in next(iter(infos.values()))["lines"]}
    for k, what in (("before_source", "`removing node before source` line"), ("after_sink", "`removing node after sink` line"),
                    ("aligned", "p: line whose length differs from its r: line"), ("ref_spelling", "p: line equal to its r: line"),
                    ("mismatch_1_5", "p: line of the r: line's length with 1..5 mismatches")):
        if tot[k] < 1:
            raise SystemExit(f"no {what} in the set")
    if not any(i["synth"].get("read_len") == 100 and i["synth"].get("dup_prob") and i["lines"]["rebuilds"] >= 3 and i["lines"]["cycle"] >= 20
               for i in infos.values()):
        raise SystemExit("no duplication case rebuilt at three or more k with 20 `cycle detected in read` lines")
    if not any(i["synth"].get("n_runs") for i in infos.values()):
        raise SystemExit("no case with N in the window reference")
    if not any("--linked-reads" in i["flags"] for i in infos.values()):
        raise SystemExit("no case with --linked-reads")
    if not any("--kmer-recovery" in i["flags"] for i in infos.values()):
        raise SystemExit("no case with --kmer-recovery")
    if sum(1 for i in infos.values() if i["cli"]) != 1:
        raise SystemExit("exactly one case keeps its BAMs and FASTA")
    for c, i in infos.items():
        if not 8 <= i["n_windows"] <= 20:
            raise SystemExit(f"{c}: {i['n_windows']} windows (8-20)")
    for f in os.listdir(OUT):
        if os.path.getsize(os.path.join(OUT, f)) > (1 << 20):
            raise SystemExit(f"{f} is larger than 1 MiB")
    print("set ok:", tot)


if __name__ == "__main__":
    mg.check_reference_is_unmodified()
    for c in (sys.argv[1:] or list(CASES)):
        make_case(c)
    if not sys.argv[1:]:
        check_set()
