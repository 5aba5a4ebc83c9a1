"""Windows whose reference contains N through the LDS build kernel (tests/nref_cases.py), on the host builds of the kernels: records,
per-window statistics and the digest of the -v trace equal the oracle's, and every window's first graph comes from the LDS build
(emu.LAST_PREBUILT) -- as it does for the N-free twin of every batch.  Until the build kernel took N, that count was 0 for these batches.
The same cases run on the device in test_nref_lds_gpu.py."""
import os
import sys

import pytest

import golden_util as gu
import nref_cases as nc
from lancet_amd import abi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402

EVT = 1 << 18


@pytest.fixture
def build_of():
    """Yields the setter of emu.FAT; the thin build is selected again afterwards."""
    def use(fat):
        emu.FAT[0] = fat
    yield use
    emu.FAT[0] = False


def _run_both(build_of, batch, p, want, what, n_built=None):
    """The batch on both host builds against the oracle; the route on the thin one (the re-run tier builds N windows by the general build)."""
    for fat in (False, True):
        build_of(fat)
        got = emu.run(batch, p, evt_cap=EVT)
        built = emu.LAST_PREBUILT[0]
        nc.assert_equal_to_oracle(got, want, what=(what, fat))
        if not fat:
            assert built == (batch.n_windows if n_built is None else n_built), (what, built, batch.n_windows)
    build_of(False)


def _twin_is_built_whole(twin, p, n_built=None):
    emu.FAT[0] = False
    emu.run(twin, p)
    assert emu.LAST_PREBUILT[0] == (twin.n_windows if n_built is None else n_built), emu.LAST_PREBUILT


def test_hand_made_windows(build_of):
    """One N, runs of k - 1, k, k + 1 and 2k, N at the window's edges, the k-mer that is its own reverse complement at odd k, the inverted
    repeat across N (one node, two offsets), reads that carry A -- or the other three bases -- where the reference shows N."""
    nc.hand_preconditions()
    batch, twin = nc.hand_made()
    p = abi.default_params()
    _twin_is_built_whole(twin, p)
    _run_both(build_of, batch, p, nc.oracle_of("hand"), "hand")


def test_every_hand_made_window_on_its_own():
    """... one window per batch: a failure names its case (and nothing carries over from the window before)."""
    from lancet_amd import workload
    from oracle import oracle
    batch, _ = nc.hand_made()
    p = abi.default_params()
    for w, name in enumerate(nc.HAND):
        one = workload.sub_batch(batch, w, w + 1)
        got = emu.run(one, p, evt_cap=EVT)
        assert emu.LAST_PREBUILT[0] == 1, name
        nc.assert_equal_to_oracle(got, oracle.run(one, p, verbose=True), what=name)


@pytest.mark.parametrize("wide", [False, True], ids=["default", "wide"])
def test_a_window_of_more_than_512_reads(wide, build_of, monkeypatch):
    """The 1024-lane configuration (a window of 640 reads), with the narrow and the wide hand-off areas."""
    if wide:
        monkeypatch.setenv("LANCET_PRE_WIDE", "1")
    batch, twin = nc.many_reads()
    p = abi.default_params()
    _twin_is_built_whole(twin, p)
    _run_both(build_of, batch, p, nc.oracle_of("many_reads"), ("many_reads", wide))
    assert emu.LAST_BIGLIST[0] == 1


@pytest.mark.parametrize("wide", [False, True], ids=["default", "wide"])
def test_deep_str_rich_windows_climb_past_k_31(wide, build_of, monkeypatch):
    """100x / 40x, STR-rich, N in every window: keys of more than one word.  With the default hand-off areas (one key word) the graphs
    above k = 31 are the general build's -- which has to know of the N: PreHdr::hasN; with the wide ones the 1024-lane configuration builds
    them.  The twin leaves out as many windows as the batch does: none."""
    if wide:
        monkeypatch.setenv("LANCET_PRE_WIDE", "1")
    batch, twin = nc.deep_str()
    p = abi.default_params()
    want = nc.oracle_of("deep_str")
    assert max(s["final_k"] for s in want[1]) > 63 and sum(s["n_builds"] for s in want[1]) > batch.n_windows
    _twin_is_built_whole(twin, p)
    _run_both(build_of, batch, p, want, ("deep_str", wide))


def test_graphs_built_ahead_and_by_the_service_next_to_n(build_of, monkeypatch):
    """Duplications next to N: k climbs through several graphs per window.  With the service, without it, with nothing built ahead and
    with no LDS build at all the records are the same; every graph a window takes from the LDS build has N nodes in it."""
    batch, twin = nc.climbing()
    p = abi.default_params()
    want = nc.oracle_of("climbing")
    assert max(s["n_builds"] for s in want[1]) >= 5
    _twin_is_built_whole(twin, p)
    _run_both(build_of, batch, p, want, "climbing")
    emu.run(batch, p)
    assert emu.LAST_AHEAD[1] >= 10 and emu.LAST_SVC[1] >= 10, (emu.LAST_AHEAD, emu.LAST_SVC)
    for env in ({"LANCET_NO_SVC": "1"}, {"LANCET_AHEAD_DEPTH": "0", "LANCET_SVC_DEPTH": "0"}, {"LANCET_NO_PREBUILD": "1"}):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            got = emu.run(batch, p, evt_cap=EVT)
            built = emu.LAST_PREBUILT[0]
        nc.assert_equal_to_oracle(got, want, what=env)
        assert built == (0 if "LANCET_NO_PREBUILD" in env else batch.n_windows), (env, built)


@pytest.mark.parametrize("route", ["small", "large"])
def test_linked_reads_with_n(route, build_of, monkeypatch):
    """--linked-reads: the records carry the haplotype counts and barcode sets; an N node has no run to replay."""
    if route == "large":
        monkeypatch.setenv("LANCET_EMU_FORCE_LARGE", "1")
    batch, twin = nc.linked()
    p = abi.default_params(lr_mode=1)
    want = nc.oracle_of("linked", True)
    assert any(any(len(x) for x in r["bx"]) for r in want[0]) and any(any(r["hp"]) for r in want[0])
    _twin_is_built_whole(twin, p)
    _run_both(build_of, batch, p, want, ("linked", route))


def test_recovery_finds_no_acceptor_in_an_n_node(build_of):
    """-R on the hand-made window whose donor k-mers, mutated, are the 2-bit image of the reference's N k-mers: same records, statistics
    and route with and without the flag (and without it, the oracle's)."""
    batch, twin = nc.recovery_window()
    want = nc.oracle_of("recovery")
    _twin_is_built_whole(twin, abi.default_params())
    for fat in (False, True):
        build_of(fat)
        runs = []
        for flag in (0, 1):
            v, st, tr = emu.run(batch, abi.default_params(kmer_recovery=flag), evt_cap=EVT)
            runs.append((v, [nc.KEY(s) for s in st], gu.digest_trace(tr), emu.LAST_PREBUILT[0]))
            if flag == 0:
                nc.assert_equal_to_oracle((v, st, tr), want, what=("recovery", fat))
        assert runs[0] == runs[1], fat
        if not fat:
            assert runs[0][3] == 1


def test_mixed_batch_twice_through_one_library(build_of):
    """N windows between ordinary ones, the batch twice in a row."""
    batch, twin = nc.mixed()
    p = abi.default_params()
    _twin_is_built_whole(twin, p)
    for _ in range(2):
        _run_both(build_of, batch, p, nc.oracle_of("mixed"), "mixed")


@pytest.mark.parametrize("case", ["nref"])
def test_the_reference_made_golden_takes_the_new_route(case):
    """tests/golden/nref.* (N runs of 1, 2, 3 and 17 bases): all of its windows are built in LDS; its parity with the reference's own
    trace is test_emu_kernels.py's."""
    meta, batch, kept, (min_k, max_k) = gu.case_batch(case)
    emu.run(batch, gu.params(meta))
    assert emu.LAST_PREBUILT[0] == batch.n_windows


def test_the_recovery_golden_with_n_takes_the_new_route():
    import recovery_util as ru
    m, batch, kept = ru.case_batch("rec_nref")
    for flag in (False, True):
        emu.run(batch, ru.params(m, flag))
        assert emu.LAST_PREBUILT[0] == batch.n_windows, flag
