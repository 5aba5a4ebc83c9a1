// emu_hap_sup.cc -- TEST INFRASTRUCTURE ONLY.
//
// The host emulation of the kernels (tests/emu/emu_engine.cc, included as it is) with the haplotype capture, its CIGAR, coverage and
// support words (EngineCaps::hap_aln / hap_cov / hap_sup) AND the emulated support kernel (lancet_amd/csrc/hap_support.h, the same
// source the engine compiles for the device) over the buffers the window kernels left, as lancet_engine_wait runs it: behind the
// re-run tier, in front of the read-back.  As in tests/hap_cov_emu the emulator's driver knows nothing of any of them: buffers, size
// and switches reach the window kernels through the sink of layout.h (LcEmuHapSink).  lancet_emu_run here is the emulator's with the
// capture around it; everything else the library exports is the emulator's own, so tests/emu/emu.py drives it unchanged
// (hap_sup_emu.py puts this library in its place for the length of a run).
//
// The engine's two tiers: with LANCET_EMU_TIER1 in the environment the batch runs twice over the SAME buffers -- first with the tier-1
// work space the variable asks for, then with the re-run tier's -- and only the first run starts from cleared length words, as an
// upload leaves them.  The support kernel runs once, after both.
#define lancet_emu_run lancet_emu_run_plain
#include "../emu/emu_engine.cc"
#undef lancet_emu_run
#include "../../lancet_amd/csrc/hap_support.h"
#include <string>

static thread_local uint32_t hap_words_set = 0, hap_aln_set = 0, hap_cov_set = 0, hap_sup_set = 0, hap_mm_set = 0;
static thread_local LcHapResult hap_result;
static thread_local std::vector<uint32_t> raw_len, raw_out;       // the windows' length words and buffers as the last run left them

// lancet_engine_set_haplotypes (0 = off), _set_haplotype_alignments, _set_haplotype_coverage and _set_haplotype_support: the same argument rules
extern "C" int lancet_hapsup_emu_set(uint32_t words_per_window, int aln, int cov, int sup, int max_mismatches) {
  if (words_per_window && words_per_window < LC_HAP_MIN_WORDS) return LANCET_E_ARG;
  if (aln != 0 && aln != 1) return LANCET_E_ARG;
  if (cov != 0 && cov != 1) return LANCET_E_ARG;
  if (sup != 0 && sup != 1) return LANCET_E_ARG;
  if (max_mismatches < 0 || max_mismatches > 255) return LANCET_E_ARG;
  hap_words_set = words_per_window; hap_aln_set = (uint32_t)aln; hap_cov_set = (uint32_t)cov; hap_sup_set = (uint32_t)sup; hap_mm_set = (uint32_t)max_mismatches;
  return LANCET_OK;
}

extern "C" void *lancet_emu_run(const lancet_params *P, const lancet_window_batch *b, uint32_t evt_cap) {
  const int nw = b->n_windows > 0 ? b->n_windows : 0;
  hap_result.h.clear(); hap_result.words.clear(); hap_result.truncated.assign((size_t)nw, 0);
  hap_result.cigar_off.assign(1, 0u); hap_result.cigar.clear();
  hap_result.cov_off.assign(1, 0u); hap_result.cov.clear(); hap_result.sup.clear();
  raw_len.clear(); raw_out.clear();
  if (!hap_words_set) return lancet_emu_run_plain(P, b, evt_cap);
  const uint32_t cap = hap_words_set;
  // (HBM is not zeroed; the lengths are cleared per upload.  One spare word in front when the size is odd keeps window 0's buffer 8-byte
  //  aligned as a device allocation is, so that the kernels' choice between one 8-byte store and two 4-byte ones falls as it does there)
  raw_len.assign((size_t)nw + 1, 0); raw_out.assign((size_t)nw * cap + 2, 0xCDCDCDCDu);
  uint32_t *out0 = raw_out.data() + ((reinterpret_cast<uintptr_t>(raw_out.data()) & 7u) ? 1 : 0);
  lc_emu_hap_sink.cap = cap; lc_emu_hap_sink.len = raw_len.data(); lc_emu_hap_sink.out = out0; lc_emu_hap_sink.aln = hap_aln_set; lc_emu_hap_sink.cov = hap_cov_set;
  lc_emu_hap_sink.sup = hap_sup_set;
  void *h = nullptr;
  if (const char *t1 = getenv("LANCET_EMU_TIER1")) {
    const std::string keep = t1;
    lancet_emu_free(lancet_emu_run_plain(P, b, evt_cap));
    unsetenv("LANCET_EMU_TIER1");
    h = lancet_emu_run_plain(P, b, evt_cap);
    setenv("LANCET_EMU_TIER1", keep.c_str(), 1);
  } else h = lancet_emu_run_plain(P, b, evt_cap);
  lc_emu_hap_sink.cap = 0; lc_emu_hap_sink.len = nullptr; lc_emu_hap_sink.out = nullptr; lc_emu_hap_sink.aln = 0; lc_emu_hap_sink.cov = 0; lc_emu_hap_sink.sup = 0;
  // ---- the support kernel, one emulated workgroup per window, over the resident batch as the driver lays it out (emu_engine.cc: the words of
  // every read, trimmed and packed by prep_read) and the buffers as they are
  if (hap_sup_set && nw > 0) {
    const uint32_t R = b->read_begin[nw];
    std::vector<uint32_t> rinfo(R + 1), bw(R + 1), gw(R + 1);
    uint32_t bo = 0, go = 0;
    for (uint32_t r = 0; r < R; ++r) { const uint32_t len = b->seq_off[r + 1] - b->seq_off[r]; bw[r] = bo; gw[r] = go; bo += (len + 15) / 16; go += (len + 31) / 32; }
    std::vector<uint32_t> bases(bo + 4), good(go + 1);
    for (uint32_t r = 0; r < R; ++r)
      prep_read(P, b->seq, b->qual, b->seq_off[r], (int)(b->seq_off[r + 1] - b->seq_off[r]), b->label[r], b->strand[r], b->mate[r], b->mapped[r],
                &rinfo[r], bases.data(), bw[r], good.data(), gw[r]);
    DevBatch B; memset(&B, 0, sizeof(B));
    B.n_windows = nw; B.read_begin = b->read_begin; B.rinfo = rinfo.data(); B.base_woff = bw.data(); B.bases = bases.data();
    static thread_local SupShared SS;
    memset(&SS, 0xCD, sizeof(SS));
    for (int w = 0; w < nw; ++w) hap_support_window(&B, raw_len.data(), out0, cap, hap_mm_set, w, &SS);
  }
  if (out0 != raw_out.data()) raw_out.erase(raw_out.begin());
  // what lancet_engine_wait does: the used words of every window, dense, then the entries
  const lancet_window_stats *st = lancet_emu_stats(h);
  std::vector<uint32_t> off((size_t)nw + 1, 0), dense;
  for (int w = 0; w < nw; ++w) {
    const uint32_t u = lc_hap_used(raw_len[(size_t)w], cap, st[w].status);
    off[(size_t)w + 1] = off[(size_t)w] + u;
    dense.insert(dense.end(), raw_out.begin() + (size_t)w * cap, raw_out.begin() + (size_t)w * cap + u);
  }
  dense.push_back(0);
  lc_hap_collect(nw, raw_len.data(), off.data(), dense.data(), st, &hap_result);
  return h;
}

// lancet_engine_results_haplotypes / _haplotype_alignments / _haplotype_coverage / _haplotype_support of the last run on this thread
extern "C" int lancet_hapsup_emu_results(const lancet_haplotype **h, uint32_t *n, const uint32_t **words, uint32_t *n_words, const uint8_t **truncated) {
  *h = hap_result.h.data(); *n = (uint32_t)hap_result.h.size(); *words = hap_result.words.data(); *n_words = (uint32_t)hap_result.words.size();
  *truncated = hap_result.truncated.data();
  return LANCET_OK;
}
extern "C" int lancet_hapsup_emu_cigars(const uint32_t **cigar_off, const uint32_t **cigar, uint32_t *n_cigar) {
  *cigar_off = hap_result.cigar_off.data(); *cigar = hap_result.cigar.data(); *n_cigar = (uint32_t)hap_result.cigar.size();
  return LANCET_OK;
}
extern "C" int lancet_hapsup_emu_coverage(const uint32_t **cov_off, const uint16_t **cov, uint32_t *n_cov) {
  if (hap_result.cov_off.size() != hap_result.h.size() + 1) hap_result.cov_off.assign(hap_result.h.size() + 1, (uint32_t)hap_result.cov.size());
  *cov_off = hap_result.cov_off.data(); *cov = hap_result.cov.data(); *n_cov = (uint32_t)hap_result.cov.size();
  return LANCET_OK;
}
extern "C" int lancet_hapsup_emu_support(const uint32_t **support) {
  *support = (hap_result.sup.size() == (size_t)HP_SUP_WORDS * hap_result.h.size() && !hap_result.sup.empty()) ? hap_result.sup.data() : nullptr;
  return LANCET_OK;
}
// the windows' length words ([n_windows]) and buffers ([n_windows * cap]) of the last run with the capture on
extern "C" uint32_t lancet_hapsup_emu_raw(const uint32_t **len, const uint32_t **out) { *len = raw_len.data(); *out = raw_out.data(); return hap_words_set; }
extern "C" uint32_t lancet_hapsup_emu_struct_size() { return (uint32_t)sizeof(lancet_haplotype); }
extern "C" uint32_t lancet_hapsup_emu_flag() { return (uint32_t)LANCET_HAP_HAS_SUPPORT; }
