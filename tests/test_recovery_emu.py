"""-R / --kmer-recovery without a GPU: the emulated kernels (tests/emu) against what the REFERENCE ITSELF wrote with and without the
option (tests/golden/recovery/, tools/make_recovery_goldens.py), the parameter block, and the command line's parser.

The pass: reference src/ErrorCorrector.hh:38-134, called at src/Microassembler.cc:137-140; kernels.h build_recover (general build, also
the re-run tier's source) and the recovery section of build_lds_impl.h (both configurations of the LDS build, the build service, graphs
built ahead)."""
import ctypes
import os
import sys

import pytest

import golden_util as gu
import recovery_util as ru
from lancet_amd import abi, cli

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402

_KEY = lambda s: (s["status"], s["final_k"], s["n_builds"], s["n_variants"], s["n_kmers"], s["max_nodes"])


@pytest.fixture
def build(request, monkeypatch):
    """wave: the LDS build kernel + service + window kernel; fat: the re-run tier's source with every graph from the general build."""
    if request.param == "fat":
        monkeypatch.setenv("LANCET_NO_PREBUILD", "1")
        emu.FAT[0] = True
    yield request.param
    emu.FAT[0] = False


@pytest.mark.parametrize("build", ["wave", "fat"], indirect=True)
@pytest.mark.parametrize("recovery", [True, False], ids=["R", "noR"])
@pytest.mark.parametrize("case", ru.CASES)
def test_emulated_kernels_reproduce_the_reference_with_and_without_recovery(case, recovery, build):
    m, batch, kept = ru.case_batch(case)
    v, st, tr = emu.run(batch, ru.params(m, recovery), evt_cap=1 << 17)
    assert all(s["status"] >= 0 for s in st)
    assert ru.records_vcf(batch, v) == ru.golden_vcf(case, recovery)             # record for record: the VCF the reference wrote
    assert gu.digest_trace(tr) == ru.golden_trace(case, recovery)                # every stage of its -v trace


def test_fixture_set_can_tell_an_engine_that_ignores_the_flag():
    metas = {c: ru.meta(c) for c in ru.CASES}
    assert sum(1 for m in metas.values() if m["vcf_records_differ"] or m["trace_differs"]) >= 3
    differ = [c for c, m in metas.items() if m["vcf_records_differ"]]
    assert differ
    for c in differ:
        assert ru.golden_vcf(c, True) != ru.golden_vcf(c, False)
    assert any("--min-k" in m["flags"] and int(m["flags"][m["flags"].index("--min-k") + 1]) % 2 == 0 for m in metas.values())
    assert any(m["synth"].get("n_runs") for m in metas.values())


@pytest.mark.parametrize("case", ru.CASES)
def test_recovery_does_not_change_which_route_builds_a_graph(case):
    """Scheduling is the same with the flag on and off: LDS-built windows, the 1024-lane list, the service's requests."""
    m, batch, kept = ru.case_batch(case)
    routes = []
    for recovery in (False, True):
        _, st, _ = emu.run(batch, ru.params(m, recovery))
        routes.append((emu.LAST_PREBUILT[0], emu.LAST_BIGLIST[0], emu.LAST_SVC[0], emu.LAST_SVC[1], [s["max_nodes"] for s in st]))
    assert routes[0] == routes[1]


def test_fixture_set_reaches_every_build_route():
    seen = {"lds": 0, "large": 0, "svc": 0, "ahead": 0, "general": 0}
    for case in ru.CASES:
        m, batch, kept = ru.case_batch(case)
        emu.run(batch, ru.params(m, True))
        seen["lds"] += emu.LAST_PREBUILT[0]
        seen["large"] += emu.LAST_BIGLIST[0]
        seen["svc"] += emu.LAST_SVC[1]
        seen["ahead"] += emu.LAST_AHEAD[1]
        seen["general"] += batch.n_windows - emu.LAST_PREBUILT[0] - emu.LAST_BIGLIST[0] > 0
    assert all(seen.values()), seen


def test_params_block_keeps_its_size_and_the_old_name_of_the_slot():
    assert ctypes.sizeof(abi.LancetParams) == 72
    assert abi.LancetParams.min_cov_ratio.offset == 64 and abi.LancetParams.lr_mode.offset == 56
    p = abi.default_params()
    assert p.kmer_recovery == 0
    assert abi.default_params(kmer_recovery=1).kmer_recovery == 1
    q = abi.default_params(reserved=0)                                         # callers that still name the slot `reserved`
    assert q.kmer_recovery == 0 and q.reserved == 0
    raw = (ctypes.c_int32 * 18).from_buffer_copy(bytes(abi.default_params(kmer_recovery=1)))
    assert raw[15] == 1 and raw[14] == 0


def test_engine_create_refuses_other_values_and_linked_reads():
    from lancet_amd import engine
    L = engine.lib()
    L.lancet_engine_create.restype = ctypes.c_int
    h = ctypes.c_void_p()
    assert L.lancet_engine_create(ctypes.byref(abi.default_params(kmer_recovery=2)), 0, ctypes.byref(h)) == -1      # LANCET_E_ARG
    assert L.lancet_engine_create(ctypes.byref(abi.default_params(kmer_recovery=-1)), 0, ctypes.byref(h)) == -1
    assert L.lancet_engine_create(ctypes.byref(abi.default_params(kmer_recovery=1, lr_mode=1)), 0, ctypes.byref(h)) == -4   # LANCET_E_UNSUPPORTED
    assert not h.value
    msg = L.lancet_engine_last_error(None)
    assert b"kmer_recovery" in msg and b"lr_mode" in msg


def test_cli_parser_takes_the_option_in_both_spellings():
    base = ["--tumor", "t.bam", "--normal", "n.bam", "--ref", "r.fa", "--reg", "chr22:1-10"]
    ap = cli.build_parser()
    assert ap.parse_args(base).kmer_recovery is False
    assert ap.parse_args(base + ["--kmer-recovery"]).kmer_recovery is True
    assert ap.parse_args(base + ["-R"]).kmer_recovery is True
    with pytest.raises(SystemExit) as e:                                        # refused before a BAM is opened or an engine made
        cli.run(base + ["--linked-reads", "-R"])
    assert "--linked-reads" in str(e.value)
    for opt in ("--print-graph", "--more-verbose", "--print-config-file"):      # these stay not offered
        with pytest.raises(SystemExit):
            ap.parse_args(base + [opt])


# ---- the pass alone, on a hand-made table ------------------------------------------------------------------------------------
# One window through the emulated general build up to the end of build_graph (tests/emu/emu_recovery.cc), with the flag off and on;
# the float coverages of every k-mer are compared with a model that restates the rule over a dict of strings.

_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
_rc = lambda s: "".join(_COMP[b] for b in reversed(s))
GOOD, LOW = "I", "-"                     # phred 40; phred 12: above --trim-lowqual 10, below --min-base-qual 17


def _probe_lib(tmp_path_factory):
    import subprocess
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
    so = os.path.join(str(tmp_path_factory.mktemp("emu_recovery")), "libemu_recovery.so")
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-strict-aliasing", "-w",
                    "-o", so, os.path.join(here, "emu_recovery.cc")], check=True)
    L = ctypes.CDLL(so)
    L.lancet_emu_table_probe.restype = ctypes.c_int
    return L


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return _probe_lib(tmp_path_factory)


def _hand_made_window():
    import numpy as np
    from lancet_amd import frontend
    rng = np.random.default_rng(7)
    ref = "".join("ACGT"[i] for i in rng.integers(0, 4, 230))
    pal = "ACCTGATCAGGT"                                                    # its own reverse complement (even k = 12)
    ref = ref[:190] + pal + ref[202:]
    reads = []                                                              # (seq, qual, tumour?, reverse strand?)
    def add(lo, hi, tumour, rev, sub=None, low=()):
        s, q = list(ref[lo:hi]), [GOOD] * (hi - lo)
        if sub is not None:
            s[sub - lo] = _COMP[s[sub - lo]]
        for p in low:
            q[p - lo] = LOW
        reads.append(("".join(s), "".join(q), tumour, rev))
    for rev in (False, True, False):
        add(20, 120, True, rev, low=(58,))                                  # support 3; its tumour quality count is 0 at reference base 58
    add(20, 120, True, True, sub=60, low=(60,))                             # donor on the reverse strand, error at 60: lends to the k-mers over 60
    add(25, 115, True, False, sub=58, low=(58,))                            # donor, error at 58: the acceptors' quality count there is 0 -> nothing
    add(120, 180, True, False)                                              # support 1 only ...
    add(120, 180, True, False, sub=150, low=(150,))                         # ... so this donor's targets have tumour coverage 1 -> nothing
    add(20, 180, False, False); add(20, 180, False, True)                   # normal reads: never donors, never counted as support
    add(180, 225, True, False); add(180, 225, True, True)                   # support 2 over the palindrome
    add(180, 225, True, False, sub=195, low=(195,))                         # donor whose corrected 12-mer is the palindrome: found twice
    reads = [r for r in reads if r[2]] + [r for r in reads if not r[2]]          # tumour reads first, then the normal ones (lancet_window_batch)
    seq = "".join(r[0] for r in reads).encode(); qual = "".join(r[1] for r in reads).encode()
    n = len(reads)
    batch = frontend.WindowBatch(
        n_windows=1, hdr=["chrH:1-230"], chrom=["chrH"], chr_id=np.zeros(1, np.int32), ref_start=np.ones(1, np.int32),
        ref_off=np.array([0, len(ref)], np.uint32), ref_bases=np.frombuffer(ref.encode(), np.uint8).copy(), read_begin=np.array([0, n], np.uint32),
        seq_off=np.cumsum([0] + [len(r[0]) for r in reads]).astype(np.uint32), seq=np.frombuffer(seq, np.uint8).copy(),
        qual=np.frombuffer(qual, np.uint8).copy(), label=np.array([4 if r[2] else 5 for r in reads], np.uint8),
        strand=np.array([2 if r[3] else 1 for r in reads], np.uint8), mate=np.zeros(n, np.uint8), mapped=np.ones(n, np.uint8),
        name_rank=np.arange(n, dtype=np.uint32))
    return ref, reads, batch


def _model(ref, reads, K):
    """k-mer table as the issue words it: counts, per-position quality counts, then what recovery lends (Tf, Tr per k-mer)."""
    tab = {}
    node = lambda key: tab.setdefault(key, {"cov": [0, 0, 0, 0], "q": [[0, 0, 0, 0] for _ in range(K)]})
    for p in range(len(ref) - K + 1):
        km = ref[p:p + K]; node(min(km, _rc(km)))
    for s, q, tumour, rev in reads:
        cls = (0 if tumour else 2) + (1 if rev else 0)
        for p in range(len(s) - K + 1):
            km = s[p:p + K]; r = _rc(km); fwd = km < r
            nd = node(km if fwd else r)
            nd["cov"][cls] += 1
            for j in range(K):
                if q[p + j] == GOOD:
                    nd["q"][j if fwd else K - 1 - j][cls] += 1
    lent = {k: [0, 0] for k in tab}
    for key, a in tab.items():
        if a["cov"][0] + a["cov"][1] != 1:
            continue
        strand = 0 if a["cov"][0] > 0 else 1
        for i in range(K):
            if a["q"][i][0] + a["q"][i][1] != 0:
                continue
            for b in "ACGT":
                if b == key[i]:
                    continue
                m = key[:i] + b + key[i + 1:]
                for hit, pos in ((m, i), (_rc(m), K - 1 - i)):
                    t = tab.get(hit)
                    if t is not None and t is not a and t["cov"][0] + t["cov"][1] >= 2 and t["q"][pos][0] + t["q"][pos][1] > 0:
                        lent[hit][strand] += 1
    return tab, lent


@pytest.mark.parametrize("K", [15, 12])
def test_recovery_pass_alone_on_a_hand_made_table(probe, K):
    ref, reads, batch = _hand_made_window()
    tab, lent = _model(ref, reads, K)
    keys = sorted(tab)
    got = {}
    for rec in (0, 1):
        p = abi.default_params(min_k=K, max_k=K, kmer_recovery=rec)
        cb = abi.batch_to_c(batch)
        n = len(keys)
        nodes = (ctypes.c_int32 * n)(); cov = (ctypes.c_float * (4 * n))(); kc = (ctypes.c_uint16 * (4 * n))()
        assert probe.lancet_emu_table_probe(ctypes.byref(p), ctypes.byref(cb), "".join(keys).encode(), n, nodes, cov, kc) == K
        assert all(x >= 0 for x in nodes)
        got[rec] = ([list(cov[4 * i:4 * i + 4]) for i in range(n)], [list(kc[4 * i:4 * i + 4]) for i in range(n)])
    for i, key in enumerate(keys):
        want = tab[key]["cov"]
        assert got[0][0][i] == [float(x) for x in want], key                                   # the table itself, flag off
        assert got[0][1][i] == want and got[1][1][i] == want, key                              # the cov_t counts never move
        assert got[1][0][i] == [float(want[0] + lent[key][0]), float(want[1] + lent[key][1]), float(want[2]), float(want[3])], key
    total = [sum(l[0] for l in lent.values()), sum(l[1] for l in lent.values())]
    if K == 15:
        # the donor on the reverse strand lends K times, all on Tr; the donor at the acceptors' dead position and the one whose targets have
        # support 1 lend nothing; the k-mer over 52..66 has base 60 at 8 and base 58 at the mirrored 6: the position must follow the hit's orientation
        assert total[1] >= K and lent[min(ref[52:67], _rc(ref[52:67]))] == [0, 1]
        assert all(l == [0, 0] for k, l in lent.items() if any(k in (ref[s:s + K], _rc(ref[s:s + K])) for s in range(120, 180 - K + 1)))
    else:
        pal = "ACCTGATCAGGT"
        assert lent[pal] == [2, 0]                                                             # found by both look-ups: two increments
