"""python tools/haplotype_cost.py [windows] [--alignments] [--coverage] [--support] [--placements] [--evidence] [--once] -- cost of the haplotype capture on the bench batch (workload.make_scan_batch(32768, 30, 30, seed=22), the batch resident): wall time of
lancet_engine_run per step with the capture off and on (lancet_gpu's size for the batch), the kernels' time, and the read-back.
--alignments: also with every haplotype's CIGAR (lancet_engine_set_haplotype_alignments; lancet_gpu --haplotype-sam's size for the batch), and the CIGAR words per batch.
--coverage: also with every base's coverages on top of the CIGARs (lancet_engine_set_haplotype_coverage; lancet_gpu --haplotype-coverage's size for the batch): the window kernel's own time,
the read-back, the words per window that are used, the truncated windows; every haplotype's arrays are checked for their shape.
--support: also with the reads that fit every haplotype (lancet_engine_set_haplotype_support; lancet_gpu --haplotype-support's size for the batch, 5 mismatches): the support kernel's
HIP-event time (not one of the run's kernels: it runs in the wait), the window kernel with and without the switch, the read-back; the counts are checked for their invariants.
--placements: also with the reads' placements (lancet_engine_set_haplotype_placements; lancet_gpu --haplotype-reads' size for the batch, 5 mismatches) and, as the yardstick, the
support run: the placement kernel's HIP-event time beside the support kernel's on the same batch, the records' bytes (8 per read; their read-back and decoding is what the
`place` step's wall time has beyond the `aln` step's and the kernel), reads placed / not placed / with n_haplotypes > 1.
--evidence: also with the variant evidence (lancet_engine_set_haplotype_evidence; lancet_gpu --variant-evidence's size and records per window for the batch, 5 mismatches, support on
beside it for the invariants) and, as the yardsticks, the support and the placement run: the evidence kernel's HIP-event time beside theirs on the same batch, the records' read-back
(bytes and host-clock time), and the totals over the batch: events, events with a record, unevaluated events, marked windows, the most events of a window, the sums of alt / ref / other;
the invariants of tests/hap_evid_cases.py are checked on every haplotype.
--once: every configuration once, not twice."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from lancet_amd import abi, engine, workload
import hap_cases as hc

args = [a for a in sys.argv[1:] if a not in ("--alignments", "--coverage", "--support", "--placements", "--evidence", "--once")]
evd = "--evidence" in sys.argv[1:]
EVID_EVENTS = 128                       # lancet_gpu's records per window (lancet_main.cc EVID_EVENTS)
plc = "--placements" in sys.argv[1:] or evd
sup = "--support" in sys.argv[1:] or plc
aln = "--alignments" in sys.argv[1:]
cov = "--coverage" in sys.argv[1:]
n = int(args[0]) if args else 32768
t = time.time(); batch = workload.make_scan_batch(n, 30.0, 30.0, seed=22); print("batch s", round(time.time() - t, 1), flush=True)
p = abi.default_params(min_k=11, max_k=101)
words = hc.ample_words(batch, p)
longest = max(int(batch.ref_off[w + 1] - batch.ref_off[w]) for w in range(batch.n_windows))
cov_words = words + 32 * 64 + 32 * 2 * (2 * longest + int(p.max_indel_len) + 256)
res = {}
once = ([("off", 0, False, False, False, False, 0), ("on", words, False, False, False, False, 0)] + ([("aln", words + 32 * 64, True, False, False, False, 0)] if aln or cov or plc else [])
        + ([("cov", cov_words, True, True, False, False, 0)] if cov else []) + ([("sup", words + 32 * 8, False, False, True, False, 0)] if sup else [])
        + ([("place", words + 32 * 64, True, False, False, True, 0)] if plc else [])
        + ([("evid", words + 32 * 64 + 32 * 8, True, False, True, False, EVID_EVENTS)] if evd else []))
runs = once + ([] if "--once" in sys.argv[1:] else [(l + "2", hw, al, cv, sp, pl, ev) for l, hw, al, cv, sp, pl, ev in once])
for label, hw, al, cv, sp, pl, ev in runs:
    eng = engine.Engine(p, haplotype_words=hw, haplotype_alignments=al, haplotype_coverage=cv, haplotype_support=sp, haplotype_support_mismatches=5,
                        haplotype_placements=pl, haplotype_placement_mismatches=5, haplotype_evidence=ev, haplotype_evidence_mismatches=5)
    eng.upload(batch)
    names = eng.kernel_names()
    wi = names.index("window_kernel") if "window_kernel" in names else None
    wall, kern, rb, wk, sk, pk, ek, erb = [], [], [], [], [], [], [], []
    for it in range(12):
        t = time.perf_counter(); eng.run(); wall.append(1000 * (time.perf_counter() - t))
        kern.append(eng.timing_ms()[0]); rb.append(eng.haplotype_readback_ms())
        wk.append(eng.kernel_times()[wi] if wi is not None else eng.timing_ms()[1])
        sk.append(eng.haplotype_support_ms()); pk.append(eng.haplotype_placement_ms()); ek.append(eng.haplotype_evidence_ms()); erb.append(eng.haplotype_evidence_readback_ms())
    v, st = eng.results()
    haps, trunc = ([], []) if not hw else eng.haplotypes()
    res[label] = (v, st)
    med = lambda a: float(np.median(a[2:]))
    used = sum(hc.words_of(h) + len(h.get("cigar", ())) + (2 * (h["len"] + h["ref_len"]) if "cov" in h else 0) + (8 if "support" in h else 0) for h in haps)
    print(f"{label}: words/window {hw} wall ms/step median {med(wall):.2f} (min {min(wall[2:]):.2f} max {max(wall[2:]):.2f}) kernels ms {med(kern):.2f} window kernel ms {med(wk):.2f} "
          f"support kernel ms {med(sk):.2f} placement kernel ms {med(pk):.2f} evidence kernel ms {med(ek):.2f} evidence read-back ms {med(erb):.2f} read-back ms {med(rb):.2f} read-back bytes {4 * used} haplotypes {len(haps)} bases {sum(h['len'] for h in haps)} cigar words {sum(len(h.get('cigar', ())) for h in haps)} "
          f"used words/window {used / max(1, batch.n_windows):.1f} truncated windows {sum(trunc)} records {len(v)} "
          f"bad {sum(1 for s in st if s['status'] < 0)} rerun {eng.rerun_count()}", flush=True)
    if cv:
        import hap_cov_cases as hcc
        haps_plain = hcc.strip_cov(haps)
        if label == "cov":
            hcc.check_shape(haps)
            print("coverage shape ok on", len(haps), "haplotypes;", sum(1 for h in haps if (h["cov"]["path"][:, 0] != h["cov"]["path"][:, 1]).any()), "with an+ != an- somewhere", flush=True)
        haps = haps_plain
    if ev:
        import hap_evid_cases as hec
        marked = eng.evidence_marked()
        evs = [e for h in haps for e in h["events"]]
        per = {}
        for h in haps:
            per[h["window"]] = per.get(h["window"], 0) + len(h["events"])
        grp = {}
        for h in haps:
            g = grp.setdefault((h["window"], h["kmer"], h["component"]), [0, 0])
            g[0] += 1; g[1] += len(h["events"])
        print(f"{label}: events {len(evs)} ({72 * len(evs)} bytes read back per run, 72 per event) with a record {sum(1 for e in evs if e['variant'] >= 0)} unevaluated {sum(1 for e in evs if e['flags'] & 1)} "
              f"marked windows {sum(marked)} of {batch.n_windows} (records per window {ev}) most events of a window {max(per.values()) if per else 0} most entries of a group {max(g[0] for g in grp.values())} "
              f"most events of a group {max(g[1] for g in grp.values())} sum alt {sum(sum(e['alt']) for e in evs)} ref {sum(sum(e['ref']) for e in evs)} other {sum(sum(e['other']) for e in evs)}", flush=True)
        if label == "evid":
            hec.check_invariants(haps, True)
            hec.check_join(batch, haps, v, marked)
            print("evidence invariants and join ok on", len(haps), "haplotypes", flush=True)
        haps = [{k: x for k, x in h.items() if k != "events"} for h in haps]
    if sp:
        import hap_sup_cases as hsc
        if label == "sup":
            hsc.check_invariants(batch, haps)
            print("support invariants ok on", len(haps), "haplotypes; reads that fit", sum(sum(h["support"]["fit"]) for h in haps), "alone", sum(sum(h["support"]["alone"]) for h in haps),
                  "of", batch.n_reads, "reads", flush=True)
        haps = hsc.strip_support(haps)
    if pl:
        recs, rbeg, tl = eng.placements()
        placed = recs["haplotype"] >= 0
        print(f"{label}: placement records {len(recs)} ({recs.nbytes // 2} bytes read back per run, 8 per read) placed {int(placed.sum())} not placed {int((~placed).sum())} "
              f"with n_haplotypes > 1 {int((recs['n_haplotypes'] > 1).sum())} with n_offsets > 1 {int((recs['n_offsets'] > 1).sum())} mismatches 0 {int((placed & (recs['mismatches'] == 0)).sum())}", flush=True)
        assert len(recs) == batch.n_reads and (recs["haplotype"][~placed] == -1).all() and (recs["mismatches"][placed] <= 5).all()
    if hw and label in ("on", "aln", "cov", "sup", "place", "evid"):
        import hap_align_cases as hac
        hc.check_shape(batch, st, hac.strip_cigar(haps), trunc); hc.check_link(batch, v, st, haps, windows=[w for w in range(batch.n_windows) if not trunc[w]])
        print("link check ok on", batch.n_windows, "windows", flush=True)
    if label in ("aln", "cov", "place", "evid"):
        hac.check_cigars(batch, haps, v)
        print("cigar check ok on", len(haps), "haplotypes", flush=True)
    eng.close()
assert all(r == res["off"] for r in res.values()), "records / stats differ with the capture on"
print("records and stats identical with and without the capture")
