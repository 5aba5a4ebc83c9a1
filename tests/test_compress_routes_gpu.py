"""The lane-dependent routes of unitig compression on the device, through engine.Engine: what the emulator (tests/test_compress_emu.py,
lanes one after the other) cannot show -- a race between the lanes that share the descriptor loops of compress_node_wv, a barrier
missing between the passes of compress_rank or of the build kernel's bl_compress_first, a miscompile of the shared rules.

One batch of 8 synthetic windows of 300 bases at 20x / 20x with a raised error rate (3 %): tips and short links make the passes after the
first compress merge unitigs of more than 64 k-mers -- under the emulator windows 1, 2, 3, 4 and 6 of the batch do, with merges of 95, 72,
81, 115 and 74 descriptors, the lane-strided copy's second trip.  Records, per-window statistics and the digest of the -v trace equal the
oracle's under three settings: the default (the build kernel does the first compress, compress_node_wv the later ones), without the LDS
build (the window kernel's compress_rank), and with a 64-entry tier-1 node table (the re-run tier: the one-lane body).

compress_fast and the ring route have no lane-dependent code (one lane walks records) and stay with the CPU rig."""
import functools
import os

import pytest

import nref_cases as nc
from lancet_amd import abi, engine, frontend, synth, workload
from oracle import oracle

pytestmark = pytest.mark.gpu

# (tools/fat_check.sh runs the suite with a 64-entry tier-1 node table: what tier 1 itself served is not counted then)
TIER1 = "LANCET_NODE_CAP1" not in os.environ
EVT = 1 << 18


@functools.lru_cache(maxsize=None)
def _batch_and_oracle():
    d = synth.make_tumor_normal(ref_len=3000, cov_t=20, cov_n=20, ref_seed=61, tumor_seed=161, normal_seed=261, error_rate=0.03, read_len=100,
                                insert_mean=300.0, insert_sd=30.0, somatic_every=400, germline_every=300)
    wins = frontend.tile_region(d["ref"], d["rname"], "chr22:400-2400", window_size=300)
    b, _ = frontend.batch_from_sam(wins, synth.pairs_to_sorted_reads(d["tumor"]), synth.pairs_to_sorted_reads(d["normal"]))
    b = workload.sub_batch(b, 0, 8)
    assert b.n_windows == 8 and int(b.ref_off[1] - b.ref_off[0]) == 300
    return b, oracle.run(b, abi.default_params(), verbose=True)


@pytest.mark.parametrize("env", [{}, {"LANCET_NO_PREBUILD": "1"}, {"LANCET_NODE_CAP1": "64"}], ids=["lds-build", "window-kernel-rank", "rerun-tier"])
def test_compression_routes(env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    batch, want = _batch_and_oracle()
    assert want[0] and all(s["status"] == 0 for s in want[1])
    eng = engine.Engine(abi.default_params(), device=0, trace_words=EVT)
    v, st = eng.process(batch)
    nc.assert_equal_to_oracle((v, st, eng.trace_text()), want, what=env)
    if "LANCET_NODE_CAP1" in env:
        assert eng.rerun_count() > 0
    elif TIER1:
        assert (eng.prebuilt_count() == 0) if "LANCET_NO_PREBUILD" in env else (eng.prebuilt_count() > 0)
    eng.close()
