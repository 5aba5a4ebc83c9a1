"""One-window inputs for the transcript walk's three routes (kernels.h count_ref_path): a path that spells the reference (Hamming
distance 0: nothing of the walk runs), a path of the reference's length with 1..5 mismatches (not aligned: the columns come straight
from the mismatch positions) and a path that is aligned.  Shared by tests/test_walk_unaligned_emu.py and tests/test_walk_unaligned_gpu.py.

A window of 200 bases of lancet_amd.synth's random reference, 32 reads of 80 bases cut from haplotypes built with
synth.build_haplotype, a third of them on the window's two ends so that the first and the last k-mer are anchors.  k = 15, except
for the two cases that name their own k (and read length).

The cases from many_ts on reach the places where the rules the two walk drivers share can go wrong: more transcripts on a path than the
LDS staging area holds (the one-lane driver redoes the path) and exactly as many, a transcript carried over the boundary between two
rounds of columns, a deletion turned complex by the column behind it, and K + 1 extension positions that need a second round."""
import numpy as np

from lancet_amd import abi, frontend, synth

W, READ_LEN, K = 200, 80, 15
# cases with a k and a read length of their own (the window stays at 200 bases): k + 1 extension positions that need a second round
_OWN = {"ins3_k33_lr": (80, 33), "ins3_k65": (150, 65)}
_COMP = {"A": "C", "C": "G", "G": "T", "T": "A"}


def _snv(ref, pos):
    return synth.PlantedVariant(pos, ref[pos], _COMP[ref[pos]], True)


def _variants(name, ref):
    if name in ("perfect",):
        return []
    if name in ("snv1", "snv1_lr", "het_ref_first", "het_alt_first"):
        return [_snv(ref, 101)]
    if name == "snv6":                                   # six mismatches: one more than the short-cut takes, so the path is aligned
        return [_snv(ref, p) for p in (70, 78, 86, 94, 102, 110)]
    if name == "snv5_ends":                              # the first and the last column a path can differ at: right behind the source
        return [_snv(ref, p) for p in (K, 60, 100, 140, W - 1 - K)]      # k-mer and right before the sink k-mer (both are reference k-mers)
    if name == "snv2_adjacent":
        return [_snv(ref, 100), _snv(ref, 101)]
    if name in ("many_ts", "ts_exact"):                  # 12 / 11 separate transcripts on one aligned path: one more than the LDS staging area
        return [_snv(ref, 22 + 13 * j) for j in range(12 if name == "many_ts" else 11)]      # of the window kernel holds, and exactly as many
    if name in ("del70", "del40_lr"):                    # one transcript over more listed columns than a round takes (64; 32 with linked reads)
        n = 70 if name == "del70" else 40
        return [synth.PlantedVariant(65, ref[65:65 + n], "", True)]
    if name == "del_then_snv":                           # the mismatch right behind the deletion turns the transcript complex (t.code != code)
        return [synth.PlantedVariant(100, ref[100:103], "", True), _snv(ref, 103)]
    if name.startswith("ins3"):
        return [synth.PlantedVariant(100, "", "GAT" if ref[100:103] != "GAT" else "CTA", True)]
    if name == "del3":
        return [synth.PlantedVariant(100, ref[100:103], "", True)]
    raise KeyError(name)


CASES = ["perfect", "snv1", "snv6", "snv5_ends", "snv2_adjacent", "ins3", "del3", "het_ref_first", "het_alt_first", "snv1_lr",
         "many_ts", "ts_exact", "del70", "del40_lr", "del_then_snv", "ins3_k33_lr", "ins3_k65"]
# (match, snp, ins, del) of every path of the window in the order eka meets them: what each case is made to exercise.  The normal sample
# is on the reference everywhere, so a case with a variant has the reference's path too (second, unless the case says otherwise).
_REF = (200, 0, 0, 0)
PATHS = {"perfect": [_REF], "snv1": [(199, 1, 0, 0), _REF], "snv6": [(194, 6, 0, 0), _REF], "snv5_ends": [(195, 5, 0, 0), _REF],
         "snv2_adjacent": [(198, 2, 0, 0), _REF], "ins3": [(200, 0, 3, 0), _REF], "del3": [(197, 0, 0, 3), _REF],
         "het_ref_first": [_REF, (199, 1, 0, 0)], "het_alt_first": [(199, 1, 0, 0), _REF], "snv1_lr": [(199, 1, 0, 0), _REF],
         "many_ts": [(188, 12, 0, 0), _REF], "ts_exact": [(189, 11, 0, 0), _REF], "del70": [(130, 0, 0, 70), _REF], "del40_lr": [(160, 0, 0, 40), _REF],
         "del_then_snv": [(196, 1, 0, 3), _REF], "ins3_k33_lr": [(200, 0, 3, 0), _REF], "ins3_k65": [(200, 0, 3, 0), _REF]}
N_RECORDS = {"perfect": 0, "snv1": 1, "snv6": 6, "snv5_ends": 5, "snv2_adjacent": 1, "ins3": 1, "del3": 1, "het_ref_first": 1, "het_alt_first": 1, "snv1_lr": 1,
             "many_ts": 12, "ts_exact": 11, "del70": 1, "del40_lr": 1, "del_then_snv": 1, "ins3_k33_lr": 1, "ins3_k65": 1}


def paths_of(trace_text):
    import re
    return [tuple(int(x) for x in m) for m in re.findall(r"cycle: \d+ match: (\d+) snp: (\d+) ins: (\d+) del: (\d+)", trace_text)]


def read_len_k(name):
    return _OWN.get(name, (READ_LEN, K))


def params(name):
    k = read_len_k(name)[1]
    return abi.default_params(min_k=k, max_k=k, lr_mode=1 if name.endswith("_lr") else 0)


def make(name, seed=0):
    """(batch, params) of the case."""
    ref = synth.random_reference(W, 400 + seed)
    linked = name.endswith("_lr")
    alt_b, _ = synth.build_haplotype(ref, _variants(name, ref))
    ref_b, _ = synth.build_haplotype(ref, [])
    alt, rf = alt_b.tobytes().decode(), ref_b.tobytes().decode()
    het = name.startswith("het")
    rng = np.random.default_rng(7 + seed)
    read_len = read_len_k(name)[0]
    reads = []                                           # (name, seq, qual, label, strand, mate, mapped[, bx, hp])

    def add(hap, label, i, start_frac):
        start = int(round(start_frac * (len(hap) - read_len)))
        q = "".join(chr(33 + int(v)) for v in rng.choice([37, 30, 25], size=read_len, p=[0.8, 0.15, 0.05]))
        rec = (f"{'T' if label == frontend.TMR else 'N'}{i:04d}", hap[start:start + read_len], q, label, frontend.FWD if i % 2 == 0 else frontend.REV, 1, True)
        if linked:
            rec += (f"ACGTACGTACGT{i % 7:04d}-1" if i % 5 else "null", i % 3)
        reads.append(rec)

    fracs = [0.0] * 3 + [1.0] * 3 + [j / 9.0 for j in range(10)]                   # 16 reads per sample
    for i, f in enumerate(fracs):
        # het_ref_first: more reads on the reference allele, so that its path scores first; het_alt_first: the other way round
        if het:
            on_alt = (i % 3 == 0) if name == "het_ref_first" else (i % 3 != 0)
        else:
            on_alt = True
        add(alt if on_alt else rf, frontend.TMR, i, f)
    for i, f in enumerate(fracs):
        add(rf, frontend.NML, 100 + i, f)
    win = frontend.Window(f"chr22:1001-{1001 + W}", "chr22", 1001, 1001 + W, ref)
    return frontend.build_batch([win], [reads], linked=linked), params(name)
