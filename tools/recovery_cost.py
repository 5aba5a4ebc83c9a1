#!/usr/bin/env python3
"""What -R / --kmer-recovery costs on the headline batch (the workload bench.py measures): per-kernel times from
lancet_engine_kernel_times with kmer_recovery 0 and 1, and the share of windows whose records changed.

Usage:  python tools/recovery_cost.py [--windows N] [--steps K]      (needs the GPU; prints a small report)"""
import argparse
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lancet_amd import abi, engine, workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    batch = workload.make_scan_batch(a.windows, 30, 30, seed=22)
    try:
        rev = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip()
    except OSError:
        rev = ""
    print(f"commit {rev or 'unknown'} (+ working tree); {a.windows} windows 30x/30x, seed 22 (the batch bench.py measures, a quarter of its windows by default); best of {a.steps} runs per setting")
    res = {}
    for rec in (0, 1):
        eng = engine.Engine(abi.default_params(kmer_recovery=rec))
        best, out = None, None
        for _ in range(a.steps + 1):
            out = eng.process(batch)
            t = eng.kernel_times()
            if best is None or sum(t) < sum(best):
                best = t
        names = eng.kernel_names()
        res[rec] = (names, best, out, eng.prebuilt_count())
        eng.close()
    print(f"{'kernel':<28}{'-R off ms':>12}{'-R on ms':>12}")
    for i, n in enumerate(res[0][0]):
        print(f"{n:<28}{res[0][1][i]:>12.3f}{res[1][1][i]:>12.3f}")
    print(f"{'all kernels':<28}{sum(res[0][1]):>12.3f}{sum(res[1][1]):>12.3f}")
    print(f"windows first built in LDS: {res[0][3]} without -R, {res[1][3]} with")
    per = [{}, {}]
    for rec in (0, 1):
        for v in res[rec][2][0]:
            per[rec].setdefault(v["window"], []).append(v)
    changed = sum(1 for w in range(batch.n_windows) if per[0].get(w) != per[1].get(w))
    print(f"windows whose records changed with -R: {changed} of {batch.n_windows} ({100.0 * changed / batch.n_windows:.2f} %)")


if __name__ == "__main__":
    main()
