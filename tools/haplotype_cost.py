"""python tools/haplotype_cost.py [windows] [--alignments] -- cost of the haplotype capture on the bench batch (workload.make_scan_batch(32768, 30, 30, seed=22), the batch resident): wall time of
lancet_engine_run per step with the capture off and on (lancet_gpu's size for the batch), the kernels' time, and the read-back.
--alignments: also with every haplotype's CIGAR (lancet_engine_set_haplotype_alignments; lancet_gpu --haplotype-sam's size for the batch), and the CIGAR words per batch."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from lancet_amd import abi, engine, workload
import hap_cases as hc

args = [a for a in sys.argv[1:] if a != "--alignments"]
aln = "--alignments" in sys.argv[1:]
n = int(args[0]) if args else 32768
t = time.time(); batch = workload.make_scan_batch(n, 30.0, 30.0, seed=22); print("batch s", round(time.time() - t, 1), flush=True)
p = abi.default_params(min_k=11, max_k=101)
words = hc.ample_words(batch, p)
res = {}
runs = [("off", 0, False), ("on", words, False)] + ([("aln", words + 32 * 64, True)] if aln else []) + [("off2", 0, False), ("on2", words, False)] + ([("aln2", words + 32 * 64, True)] if aln else [])
for label, hw, al in runs:
    eng = engine.Engine(p, haplotype_words=hw, haplotype_alignments=al)
    eng.upload(batch)
    wall, kern, rb = [], [], []
    for it in range(12):
        t = time.perf_counter(); eng.run(); wall.append(1000 * (time.perf_counter() - t))
        kern.append(eng.timing_ms()[0]); rb.append(eng.haplotype_readback_ms())
    v, st = eng.results()
    haps, trunc = ([], []) if not hw else eng.haplotypes()
    res[label] = (v, st)
    med = lambda a: float(np.median(a[2:]))
    print(f"{label}: words/window {hw} wall ms/step median {med(wall):.2f} (min {min(wall[2:]):.2f} max {max(wall[2:]):.2f}) kernels ms {med(kern):.2f} read-back ms {med(rb):.2f} "
          f"haplotypes {len(haps)} bases {sum(h['len'] for h in haps)} cigar words {sum(len(h.get('cigar', ())) for h in haps)} truncated windows {sum(trunc)} records {len(v)} "
          f"bad {sum(1 for s in st if s['status'] < 0)} rerun {eng.rerun_count()}", flush=True)
    if hw and label in ("on", "aln"):
        hc.check_shape(batch, st, haps, trunc); hc.check_link(batch, v, st, haps, windows=[w for w in range(batch.n_windows) if not trunc[w]])
        print("link check ok on", batch.n_windows, "windows", flush=True)
    if label == "aln":
        import hap_align_cases as hac
        hac.check_cigars(batch, haps, v)
        print("cigar check ok on", len(haps), "haplotypes", flush=True)
    eng.close()
assert all(r == res["off"] for r in res.values()), "records / stats differ with the capture on"
print("records and stats identical with and without the capture")
