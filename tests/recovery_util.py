"""Fixtures of -R / --kmer-recovery: tests/golden/recovery/* (tools/make_recovery_goldens.py), written by the reference itself
with and without the option on the same inputs.  They live beside, not among, the cases golden_util.py collects."""
from __future__ import annotations

import functools
import gzip
import json
import os

import numpy as np

import golden_util as gu
from lancet_amd import frontend
from lancet_amd.synth import SamRead

DIR = os.path.join(gu.GOLDEN, "recovery")
CASES = sorted(f[:-5] for f in os.listdir(DIR) if f.endswith(".json"))
_KEYS = ("qname", "flag", "pos", "mapq", "cigar", "seq", "qual", "as", "xs", "md")


def meta(name: str) -> dict:
    return json.load(open(os.path.join(DIR, f"{name}.json")))


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
    padding, _, max_k = gu.case_params(m)
    windows = frontend.tile_region(ref, rname, m["region"], padding=padding, window_size=gu.case_window(m))
    batch, kept = frontend.batch_from_sam(windows, reads["tumor"], reads["normal"], max_k=max_k, linked=False,
                                          active_region=gu.case_active_region(m))
    return m, batch, kept


def params(m: dict, recovery: bool, **over):
    return gu.params(m, kmer_recovery=1 if recovery else 0, **over)


def tag(recovery: bool) -> str:
    return "R" if recovery else "noR"


def golden_vcf(name: str, recovery: bool, full: bool = False) -> str:
    return open(os.path.join(DIR, f"{name}.{tag(recovery)}.{'full.' if full else ''}vcf")).read()


def golden_trace(name: str, recovery: bool) -> str:
    return gzip.open(os.path.join(DIR, f"{name}.{tag(recovery)}.trace.txt.gz"), "rt").read()


def records_vcf(batch, variants) -> str:
    """VCF (without ##fileDate / ##cmdline / ##reference) of a run's records, through the restatement of VariantDB the other parity tests use."""
    from oracle import vcf_oracle
    db = vcf_oracle.VariantDB(lr=False)
    for rec in variants:
        db.add(vcf_oracle.Variant(batch.chrom[rec["window"]], rec, lr=False, bx_names=None))
    return db.vcf()
