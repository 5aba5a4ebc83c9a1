#!/usr/bin/env python3
"""Generates tests/golden/recovery/*: what the REFERENCE ITSELF writes with and without -R / --kmer-recovery on the same inputs.

Same unmodified reference binary, same helper programs and the same check as tools/make_golden.py (tools/REFERENCE_BUILD.md).  The
fixtures live in their own directory: tests/golden_util.py turns every tests/golden/*.json into a case of the parity tests against the
oracle, which knows nothing of recovery.  Per case:

  <case>.reads.npz                  the simulated reads (SAM fields) + contig sequence (inputs)
  <case>.json                       synth parameters, region, reference flags (without the recovery switch), record counts
  <case>.R.vcf / .R.trace.txt.gz    the reference's VCF (no ##fileDate / ##cmdline / ##reference) and -v digest (gzipped) WITH --kmer-recovery
  <case>.noR.vcf / .noR.trace.txt.gz  the same WITHOUT it
  <case>.{tumor,normal}.bam, .fa,   (cases marked cli) the inputs as files, and the VCFs whole but for ##fileDate: the reference run from
  <case>.R.full.vcf, .noR.full.vcf   the directory that holds tumor.bam / normal.bam / ref.fa, so that ##cmdline carries no directory

Inputs on which recovery matters: tumour at 4-8x, substitution errors with base qualities below --min-base-qual next to k-mers with
support, anchors near --cov-thr.  The script itself checks what the set must cover (see check_set).

Usage:  python tools/make_recovery_goldens.py [case ...]
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

OUT = os.path.join(mg.GOLDEN, "recovery")

CASES = {
    # name: (synth kwargs, region, extra reference flags, keep the BAM / FASTA inputs for the command-line test)
    # (seeds and depths were picked by running the reference over a few dozen candidates and keeping inputs on which -R changes its output)
    # a thin normal under a 7x tumour, anchors near --cov-thr: windows of the 512-lane LDS build; also the command-line fixture
    "rec_low": (dict(ref_len=3600, cov_t=7, cov_n=3, ref_seed=400, tumor_seed=500, normal_seed=600, error_rate=0.015,
                     somatic_every=350, germline_every=500), "chr22:900-2700", [], True),
    # even k (--min-k 12: 12, 14, ...): the general build; palindromes planted so that a mutated k-mer can be its own reverse complement
    "rec_even": (dict(ref_len=4200, cov_t=7, cov_n=20, ref_seed=302, tumor_seed=312, normal_seed=322, error_rate=0.012,
                      somatic_every=450, germline_every=600,
                      palindromes=((1300, 6), (1600, 7), (1900, 6), (2200, 8), (2500, 6), (2800, 7))), "chr22:1000-3200",
                 ["--min-k", "12", "--max-k", "60"], False),
    # N in the window reference: the general build, k-mers of the reference that are identified by their strings
    "rec_nref": (dict(ref_len=3600, cov_t=7, cov_n=3, ref_seed=401, tumor_seed=501, normal_seed=601, error_rate=0.015,
                      somatic_every=350, germline_every=500, n_runs=((1410, 1), (1833, 3), (2305, 14))), "chr22:900-2700", [], False),
    # a deep normal under the thin tumour: more than 512 reads per window -> the 1024-lane configuration
    "rec_deep": (dict(ref_len=3000, cov_t=7, cov_n=150, ref_seed=400, tumor_seed=500, normal_seed=600, error_rate=0.015,
                      somatic_every=350, germline_every=500), "chr22:1100-1900", [], False),
    # duplications: k climbs through several graphs per window (graphs built ahead, the build service)
    "rec_dups": (dict(ref_len=3600, cov_t=6, cov_n=2, ref_seed=400, tumor_seed=500, normal_seed=600, error_rate=0.015, dup_prob=1.0,
                      somatic_every=350, germline_every=500, read_len=100), "chr22:900-2700", [], False),
}


def _strip(vcf_text: str, keep_header: bool) -> str:
    drop = ("##fileDate",) if keep_header else ("##fileDate", "##cmdline", "##reference")
    return "".join(l + "\n" for l in vcf_text.splitlines() if not l.startswith(drop))


def write_trace(path: str, digest: str) -> None:
    """The -v digests run to thousands of lines per case: kept gzipped (no name, no time stamp in the header: the same bytes every time)."""
    with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0, compresslevel=9) as f:
        f.write(digest.encode())


def _records(vcf: str):
    return [l for l in vcf.splitlines() if not l.startswith("#")]


def make_case(name: str) -> dict:
    kwargs, region, flags, cli = CASES[name]
    data = synth.make_tumor_normal(**kwargs)
    ref, rname = data["ref"], data["rname"]
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory(prefix="lancet_recovery_") as td:
        synth.write_fasta(os.path.join(td, "ref.fa"), rname, ref)
        for sample, rg, pairs in (("TUMOR", "tumor", data["tumor"]), ("NORMAL", "normal", data["normal"])):
            sam = os.path.join(td, f"{rg}.sam")
            synth.write_sam(sam, rname, len(ref), sample, rg, pairs)
            mg.run([mg.TEST_VIEW, "-b", "-p", os.path.join(td, f"{rg}.bam"), sam], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            mg.run([mg.BAMTOOLS, "index", "-in", os.path.join(td, f"{rg}.bam")])
        # the command-line case runs as a user would type it (active regions on, the reference's default); the others as tools/make_golden.py runs them
        base = [mg.REF_BIN, "--tumor", "tumor.bam", "--normal", "normal.bam", "--ref", "ref.fa", "--reg", region, "--num-threads", "1"] + \
               ([] if cli else ["--active-region-off"]) + flags
        runs = {}
        for tag, extra in (("R", ["--kmer-recovery"]), ("noR", [])):
            r = subprocess.run(base + extra + ["-v"], capture_output=True, text=True, cwd=td)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-3000:])
                raise SystemExit(f"reference failed on case {name} ({tag})")
            runs[tag] = (r.stdout, mg.digest_trace(r.stderr))
        if cli:
            for rg in ("tumor", "normal"):
                shutil.copy(os.path.join(td, f"{rg}.bam"), os.path.join(OUT, f"{name}.{rg}.bam"))
            shutil.copy(os.path.join(td, "ref.fa"), os.path.join(OUT, f"{name}.fa"))
    for tag, (vcf, digest) in runs.items():
        with open(os.path.join(OUT, f"{name}.{tag}.vcf"), "w") as f:
            f.write(_strip(vcf, False))
        write_trace(os.path.join(OUT, f"{name}.{tag}.trace.txt.gz"), digest)
        if cli:
            with open(os.path.join(OUT, f"{name}.{tag}.full.vcf"), "w") as f:      # (##cmdline starts with argv[0]: the program as `lancet`, not where it was built)
                f.write(_strip(vcf, True).replace("##cmdline=" + mg.REF_BIN + " ", "##cmdline=lancet ", 1))
    reads = {}
    for rg in ("tumor", "normal"):
        rs = synth.pairs_to_sorted_reads(data[rg])
        for key, get, dt in (("qname", lambda x: x.qname, None), ("flag", lambda x: x.flag, np.int32), ("pos", lambda x: x.pos, np.int32),
                             ("mapq", lambda x: x.mapq, np.int32), ("cigar", lambda x: x.cigar, None), ("seq", lambda x: x.seq, None),
                             ("qual", lambda x: x.qual, None), ("as", lambda x: x.tags["AS"], np.int32), ("xs", lambda x: x.tags["XS"], np.int32),
                             ("md", lambda x: x.tags["MD"], None)):
            reads[f"{rg}_{key}"] = np.array([get(x) for x in rs], dtype=dt) if dt else np.array([get(x) for x in rs])
    np.savez_compressed(os.path.join(OUT, f"{name}.reads.npz"), ref=np.array(ref), rname=np.array(rname), **reads)
    rec_r, rec_n = _records(runs["R"][0]), _records(runs["noR"][0])
    info = {"synth": kwargs, "region": region, "flags": flags + (["--active-region-on"] if cli else []), "cli": cli,
            "reference_cmd": "lancet " + " ".join(base[1:]) + " [--kmer-recovery] -v",
            "n_vcf_records_R": len(rec_r), "n_vcf_records_noR": len(rec_n),
            "vcf_records_differ": rec_r != rec_n, "trace_differs": runs["R"][1] != runs["noR"][1]}
    with open(os.path.join(OUT, f"{name}.json"), "w") as f:
        json.dump(info, f, indent=1)
    print(f"{name}: {len(rec_r)} records with -R, {len(rec_n)} without; records differ: {info['vcf_records_differ']}, "
          f"trace differs: {info['trace_differs']}; {len(reads['tumor_qname'])}+{len(reads['normal_qname'])} reads")
    return info


def check_set():
    """What the committed set must cover (the parity tests cannot fail on an engine that ignores the flag otherwise)."""
    infos = {c: json.load(open(os.path.join(OUT, c + ".json"))) for c in CASES}
    differ = [c for c, i in infos.items() if i["vcf_records_differ"] or i["trace_differs"]]
    if len(differ) < 3:
        raise SystemExit(f"only {differ} differ between -R and no -R: need three")
    if not any(i["vcf_records_differ"] for i in infos.values()):
        raise SystemExit("no case whose VCF records differ between -R and no -R")
    if not any("--min-k" in i["flags"] and int(i["flags"][i["flags"].index("--min-k") + 1]) % 2 == 0 for i in infos.values()):
        raise SystemExit("no case with even k")
    if not any(i["synth"].get("n_runs") for i in infos.values()):
        raise SystemExit("no case with N in the window reference")
    for c in CASES:
        t = gzip.open(os.path.join(OUT, c + ".R.trace.txt.gz"), "rt").read()
        if c == "rec_dups" and t.count("Cycle found") + t.count(" Found repeat in assembly") < 3:
            raise SystemExit("rec_dups: the windows are not rebuilt at several k")
    for f in os.listdir(OUT):
        if os.path.getsize(os.path.join(OUT, f)) > (1 << 20):
            raise SystemExit(f"{f} is larger than 1 MiB")
    print("set ok:", ", ".join(differ), "differ")


if __name__ == "__main__":
    mg.check_reference_is_unmodified()
    for c in (sys.argv[1:] or list(CASES)):
        make_case(c)
    if not sys.argv[1:]:
        check_set()
