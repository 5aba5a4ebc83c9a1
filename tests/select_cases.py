"""Shared by test_device_select_emu.py / test_device_select_gpu.py: the device read selection (emulated, or read back from the GPU) held
against lancet_host_batch_packed on the same windows -- kept[], read_begin and per read rinfo, name_rank and the packed words reached
through its offsets; the reference codes; the per-window summaries.  Equality is exact everywhere."""
import os
import zlib

import numpy as np

import bam_writer
import golden_util as gu
from lancet_amd import abi, host, synth

G = gu.GOLDEN
_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _i
    _CODE[ord(_c.lower())] = _i


def fixture_paths(case):
    d = os.path.join(G, "recovery") if case.startswith("rec_") else G
    return [os.path.join(d, f"{case}.tumor.bam"), os.path.join(d, f"{case}.normal.bam"), os.path.join(d, f"{case}.fa")]


def table_arrays(tab):
    """The packed words and the per-alignment arrays of a lancet_alignment_table as numpy views (valid while the host object lives)."""
    n = int(tab.n_aln[0]) + int(tab.n_aln[1])

    def view(ptr, count, dt):
        if count == 0:
            return np.zeros(0, dtype=dt)
        return np.ctypeslib.as_array(abi.C.cast(ptr, abi.C.POINTER(abi.C.c_uint8)), shape=(count * np.dtype(dt).itemsize,)).view(dt)
    return dict(n=n, bases=view(tab.bases, int(tab.n_base_words) + 4, np.uint32), good=view(tab.good, int(tab.n_good_words) + 1, np.uint32),
                flags=view(tab.flags, n, np.uint8), rinfo=view(tab.rinfo, n, np.uint32), l_seq=view(tab.l_seq, n, np.uint32),
                evt_off=view(tab.evt_off, n + 1 if n else 0, np.uint32))


def _gather(words, off, cnt):
    """words[off[r] : off[r] + cnt[r]] for every r, concatenated"""
    cnt = cnt.astype(np.int64)
    total = int(cnt.sum())
    if total == 0:
        return np.zeros(0, dtype=words.dtype)
    starts = np.repeat(off.astype(np.int64), cnt)
    within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return words[starts + within]


def host_expectation(H, lo, hi, o, P):
    """lancet_host_batch_packed on [lo, hi) -> dict of what the device route must reproduce (and it advances the host object)."""
    b, idx, pk = H.batch(lo, hi, o, pack_params=P)
    R = int(b.read_begin[-1]) if b.n_windows else 0
    ln = np.diff(b.seq_off.astype(np.int64)).astype(np.int64) if R else np.zeros(0, np.int64)
    u = pk["read_index"] if "read_index" in pk else np.arange(R, dtype=np.uint32)
    rinfo = pk["rinfo"][u] if R else np.zeros(0, np.uint32)
    return dict(batch=b, kept=list(idx), read_begin=b.read_begin, ref_off=b.ref_off, ref_codes=_CODE[b.ref_bases], chr_id=b.chr_id, ref_start=b.ref_start,
                rinfo=rinfo, name_rank=b.name_rank, lens=ln,
                base_words=_gather(pk["bases"], pk["base_woff"][u], (ln + 15) // 16) if R else np.zeros(0, np.uint32),
                good_words=_gather(pk["good"], pk["good_woff"][u], (ln + 31) // 32) if R else np.zeros(0, np.uint32))


def need_large(want, lds_reads, lds_bases):
    """engine.hip's size test of the 512-lane build configuration, window by window over the host batch"""
    n = 0
    for w in range(len(want["kept"])):
        r0, r1 = int(want["read_begin"][w]), int(want["read_begin"][w + 1])
        rl = int(want["ref_off"][w + 1] - want["ref_off"][w])
        tl = (want["rinfo"][r0:r1] & 0xFFFF).astype(np.int64)
        wb, wg = (rl + 15) // 16 + int(((tl + 15) // 16).sum()), (rl + 31) // 32 + int(((tl + 31) // 32).sum())
        n += int(r1 - r0 > lds_reads or wb > lds_bases // 16 or wg > lds_bases // 32)
    return n


def assert_same(got, want, words):
    """got: the device route's arrays (select_emu.run / Engine.debug_batch + kept), words(base_woff, good_woff, lens) -> (base words, good words)"""
    assert list(got["kept"]) == want["kept"]
    for f in ("read_begin", "ref_off", "ref_codes", "chr_id", "ref_start", "rinfo", "name_rank"):
        assert np.array_equal(np.asarray(got[f]), np.asarray(want[f])), f
    bw, gw = words(got["base_woff"], got["good_woff"], want["lens"])
    assert np.array_equal(bw, want["base_words"]), "packed bases"
    assert np.array_equal(gw, want["good_words"]), "quality masks"


def table_words(tab):
    t = table_arrays(tab)
    return lambda bo, go, ln: (_gather(t["bases"], bo, (ln + 15) // 16), _gather(t["good"], go, (ln + 31) // 32))


def assert_summaries(summaries, sl, want):
    """Per window of the slice: kept exactly the host's windows, with its reads, untrimmed bases, trimmed word sums and mapped flag."""
    widx = [int(sl.widx[i]) for i in range(sl.n_windows)]
    kept = [widx[i] for i in range(sl.n_windows) if (int(summaries[i][0]) & 3) == 1]
    assert kept == want["kept"]
    rows = [summaries[i] for i in range(sl.n_windows) if (int(summaries[i][0]) & 3) == 1]
    for w, s in enumerate(rows):
        r0, r1 = int(want["read_begin"][w]), int(want["read_begin"][w + 1])
        ri = want["rinfo"][r0:r1]
        tl = (ri & 0xFFFF).astype(np.int64)
        n_t = int(((ri >> 16) & 1 == 0).sum())
        assert (int(s[1]), int(s[2])) == (n_t, r1 - r0 - n_t) and int(s[3]) == int(want["lens"][r0:r1].sum())
        assert (int(s[4]), int(s[5])) == (int(((tl + 15) // 16).sum()), int(((tl + 31) // 32).sum()))
        assert bool(int(s[0]) & 4) == bool(((ri >> 20) & 1).any())


# ---- small synthetic inputs through the test-side BAM writer: one window each ----------------------------------------------------
WIN_START, WIN_END = 501, 900          # the one window of region chrS:501-900 with --padding 0 (its reference has 399 bases)
REGION = "chrS:501-900"


def _ref(seed=7, n=2000):
    rng = np.random.default_rng(seed)
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def read(name, pos, cigar="100M", flag=0, mapq=60, md=None, qual="I", **tags):
    """A SamRead at 1-based `pos`; the bases are taken from nowhere in particular (selection does not look at them)."""
    import re
    l_seq = sum(int(n) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar) if op in "MIS=X")
    rng = np.random.default_rng(zlib.crc32(name.encode()) ^ pos)
    seq = "".join("ACGT"[i] for i in rng.integers(0, 4, l_seq))
    t = dict(tags)
    if md is not None:
        t["MD"] = md
    return synth.SamRead(qname=name, flag=flag, rname="chrS", pos=pos, mapq=mapq, cigar=cigar, seq=seq, qual=(qual * l_seq)[:l_seq], tags=t)


def write_case(tmp, tumor, normal):
    os.makedirs(tmp, exist_ok=True)
    ref = _ref()
    fa = os.path.join(tmp, "r.fa")
    synth.write_fasta(fa, "chrS", ref)
    tb, nb = os.path.join(tmp, "t.bam"), os.path.join(tmp, "n.bam")
    bam_writer.write_bam(tb, [("chrS", len(ref))], sorted(tumor, key=lambda r: r.pos), sample="TT")
    bam_writer.write_bam(nb, [("chrS", len(ref))], sorted(normal, key=lambda r: r.pos), sample="NN")
    return [tb, nb, fa]


def _clipped(j, pos0):
    # leading soft clip: isActiveRegion's `pos` runs 20 ahead of the genome, so the insertion is counted at pos0 + 90 for every j
    # although the reads start at pos0 + j (their soft clips are keyed by the genome position: all different)
    return read(f"sc{j}", pos0 + j + 1, cigar=f"20S{70 - j}M2I{8 + j}M", md="78")


def synthetic_cases():
    """name -> (tumor reads, normal reads, host options, expectation: 'kept' | 'filtered' | 'skipped')"""
    four = [read(f"c{i}", 520 + 60 * i) for i in range(4)]                # starts (0-based) 519 .. 699, 100 bases each, inside [501, 900]
    near_end = WIN_END - 78 - 2                                            # 0-based start: ends at 898, the CIGAR position reaches 910
    c = {}
    # coverage: 399 reference bases, --max-avg-cov 1 -> skipped iff the reads selected BEFORE the last candidate hold more than 399 bases
    c["cov_crossed_by_last_only"] = (four, [], dict(active_region=0, max_avg_cov=1), "kept")
    c["cov_crossed_by_the_one_before"] = (four + [read("c4", 790)], [], dict(active_region=0, max_avg_cov=1), "skipped")
    c["cov_last_candidate_not_contained"] = (four + [read("c4", 850)], [], dict(active_region=0, max_avg_cov=1), "skipped")   # (starts inside, ends behind the window)
    c["cov_normal_side"] = ([read("t0", 600)], four + [read("c4", 790)], dict(active_region=0, max_avg_cov=1), "skipped")
    c["names_r1_r10_r2"] = ([read("r10", 520), read("r2", 560), read("r1", 600)], [read("r2", 530), read("r1", 640)], dict(active_region=0), "kept")
    c["names_equal_in_8_bytes"] = ([read("readname_b", 520), read("readname", 540), read("readname_a", 560), read("readnameXYZ", 580), read("readname_", 600)],
                                   [read("readname_a", 530), read("readname_ab", 570)], dict(active_region=0), "kept")
    c["three_reads_of_one_name"] = ([read("m", 520), read("a", 530), read("m", 560), read("z", 580), read("m", 600)], [read("m", 610)], dict(active_region=0), "kept")
    c["soft_clips_past_the_end_min_evidence"] = ([_clipped(j, near_end - 2) for j in range(3)], [read("n0", 600, md="100")], dict(min_evidence=3), "kept")
    c["soft_clips_past_the_end_one_fewer"] = ([_clipped(j, near_end - 2) for j in range(2)], [read("n0", 600, md="100")], dict(min_evidence=3), "filtered")
    c["md_mismatch_at_the_last_base"] = ([read(f"x{i}", 600, md="99A") for i in range(3)], [], dict(min_evidence=3), "filtered")
    c["md_mismatch_one_before_the_last"] = ([read(f"x{i}", 600, md="98A0") for i in range(3)], [], dict(min_evidence=3), "kept")
    c["no_candidate"] = ([read("far", 1200)], [read("far2", 100)], dict(active_region=0), "kept")
    c["reads_in_one_sample_only"] = ([], [read("n1", 520), read("n0", 640)], dict(active_region=0), "kept")
    return c


def open_case(paths, o):
    H = host.NativeHost(*paths)
    hdrs = H.tile(REGION, o)
    assert hdrs == [f"chrS:{WIN_START}-{WIN_END}"]
    return H
