"""The transcript walk's three routes on the GPU (kernels.h count_ref_path; tests/test_walk_unaligned_emu.py has the same cases on the
emulated kernels): the cases of tests/walk_cases.py as one small batch through the engine, and 256 windows of the kind bench.py
measures, against the oracle -- records, window statistics and, for the small batch, every event of the -v trace."""
import pytest

import golden_util as gu
import walk_cases as wc
from lancet_amd import abi, engine, workload
from oracle import oracle

pytestmark = pytest.mark.gpu

_KEY = lambda s: (s["status"], s["final_k"], s["n_builds"], s["n_variants"], s["n_kmers"], s["max_nodes"])


def _engine_equals_oracle(batch, p, trace):
    ov, ost, otr = oracle.run(batch, p, verbose=True)
    eng = engine.Engine(p, device=0, trace_words=(1 << 16) if trace else 0)
    try:
        first = eng.process(batch)
        v, st = first
        assert all(s["status"] >= 0 for s in st)
        assert v == ov
        assert [_KEY(s) for s in st] == [_KEY(s) for s in ost]
        if trace:
            assert gu.digest_trace(eng.trace_text()) == gu.digest_trace(otr)
        assert eng.process(batch) == first                                           # deterministic
    finally:
        eng.close()
    return ov, otr


def test_walk_cases_as_one_batch():
    """The short-read cases, one small batch per (k, read length): one engine means one set of parameters."""
    names = [c for c in wc.CASES if not c.endswith("_lr")]
    groups = {}
    for c in names:
        groups.setdefault(wc.read_len_k(c), []).append(c)
    assert sorted(c for g in groups.values() for c in g) == sorted(names) and len(groups) > 1
    for group in groups.values():
        batch = workload.concat_batches([wc.make(c)[0] for c in group])
        ov, otr = _engine_equals_oracle(batch, wc.params(group[0]), trace=True)
        assert wc.paths_of(otr) == [p for c in group for p in wc.PATHS[c]]           # every case still reaches its route
        assert len(ov) == sum(wc.N_RECORDS[c] for c in group)


@pytest.mark.parametrize("case", [c for c in wc.CASES if c.endswith("_lr")])
def test_walk_case_with_linked_reads(case):
    batch, p = wc.make(case)
    ov, otr = _engine_equals_oracle(batch, p, trace=True)
    assert wc.paths_of(otr) == wc.PATHS[case] and len(ov) == wc.N_RECORDS[case]


def test_scan_batch_of_256_windows():
    batch = workload.make_scan_batch(256, 30, 30, seed=31)
    ov, otr = _engine_equals_oracle(batch, abi.default_params(), trace=False)
    kinds = [("perfect" if s + i + d == 0 else ("unaligned" if i + d == 0 and s <= 5 else "aligned")) for m, s, i, d in wc.paths_of(otr)]
    assert len(ov) > 0 and {"perfect", "unaligned", "aligned"} <= set(kinds)
