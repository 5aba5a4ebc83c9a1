// emu_hap_cov.cc -- TEST INFRASTRUCTURE ONLY.
//
// The host emulation of the kernels (tests/emu/emu_engine.cc, included as it is) with the haplotype capture, the alignment of every
// haplotype (EngineCaps::hap_aln) AND the read support of every base (EngineCaps::hap_cov, lancet_engine_set_haplotype_coverage).  As in
// tests/hap_align_emu the emulator's driver knows nothing of any of them: buffers, size and switches reach the kernels through the sink
// of layout.h (LcEmuHapSink).  lancet_emu_run here is the emulator's with the capture around it; everything else the library exports is
// the emulator's own, so tests/emu/emu.py drives it unchanged (hap_cov_emu.py puts this library in its place for the length of a run).
//
// The engine's two tiers: with LANCET_EMU_TIER1 in the environment the batch runs twice over the SAME buffers -- first with the tier-1
// work space the variable asks for, then with the re-run tier's -- and only the first run starts from cleared length words, as an
// upload leaves them.
#define lancet_emu_run lancet_emu_run_plain
#include "../emu/emu_engine.cc"
#undef lancet_emu_run
#include <string>

static thread_local uint32_t hap_words_set = 0, hap_aln_set = 0, hap_cov_set = 0;
static thread_local LcHapResult hap_result;
static thread_local std::vector<uint32_t> raw_len, raw_out;       // the windows' length words and buffers as the last run left them

// lancet_engine_set_haplotypes (0 = off), lancet_engine_set_haplotype_alignments and lancet_engine_set_haplotype_coverage: the same argument rules
extern "C" int lancet_hapcov_emu_set(uint32_t words_per_window, int aln, int cov) {
  if (words_per_window && words_per_window < LC_HAP_MIN_WORDS) return LANCET_E_ARG;
  if (aln != 0 && aln != 1) return LANCET_E_ARG;
  if (cov != 0 && cov != 1) return LANCET_E_ARG;
  hap_words_set = words_per_window; hap_aln_set = (uint32_t)aln; hap_cov_set = (uint32_t)cov;
  return LANCET_OK;
}

extern "C" void *lancet_emu_run(const lancet_params *P, const lancet_window_batch *b, uint32_t evt_cap) {
  const int nw = b->n_windows > 0 ? b->n_windows : 0;
  hap_result.h.clear(); hap_result.words.clear(); hap_result.truncated.assign((size_t)nw, 0);
  hap_result.cigar_off.assign(1, 0u); hap_result.cigar.clear();
  hap_result.cov_off.assign(1, 0u); hap_result.cov.clear();
  raw_len.clear(); raw_out.clear();
  if (!hap_words_set) return lancet_emu_run_plain(P, b, evt_cap);
  const uint32_t cap = hap_words_set;
  // (HBM is not zeroed; the lengths are cleared per upload.  One spare word in front when the size is odd keeps window 0's buffer 8-byte
  //  aligned as a device allocation is, so that the kernels' choice between one 8-byte store and two 4-byte ones falls as it does there)
  raw_len.assign((size_t)nw + 1, 0); raw_out.assign((size_t)nw * cap + 2, 0xCDCDCDCDu);
  uint32_t *out0 = raw_out.data() + ((reinterpret_cast<uintptr_t>(raw_out.data()) & 7u) ? 1 : 0);
  lc_emu_hap_sink.cap = cap; lc_emu_hap_sink.len = raw_len.data(); lc_emu_hap_sink.out = out0; lc_emu_hap_sink.aln = hap_aln_set; lc_emu_hap_sink.cov = hap_cov_set;
  void *h = nullptr;
  if (const char *t1 = getenv("LANCET_EMU_TIER1")) {
    const std::string keep = t1;
    lancet_emu_free(lancet_emu_run_plain(P, b, evt_cap));
    unsetenv("LANCET_EMU_TIER1");
    h = lancet_emu_run_plain(P, b, evt_cap);
    setenv("LANCET_EMU_TIER1", keep.c_str(), 1);
  } else h = lancet_emu_run_plain(P, b, evt_cap);
  lc_emu_hap_sink.cap = 0; lc_emu_hap_sink.len = nullptr; lc_emu_hap_sink.out = nullptr; lc_emu_hap_sink.aln = 0; lc_emu_hap_sink.cov = 0;
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

// lancet_engine_results_haplotypes / _haplotype_alignments / _haplotype_coverage of the last run on this thread
extern "C" int lancet_hapcov_emu_results(const lancet_haplotype **h, uint32_t *n, const uint32_t **words, uint32_t *n_words, const uint8_t **truncated) {
  *h = hap_result.h.data(); *n = (uint32_t)hap_result.h.size(); *words = hap_result.words.data(); *n_words = (uint32_t)hap_result.words.size();
  *truncated = hap_result.truncated.data();
  return LANCET_OK;
}
extern "C" int lancet_hapcov_emu_cigars(const uint32_t **cigar_off, const uint32_t **cigar, uint32_t *n_cigar) {
  *cigar_off = hap_result.cigar_off.data(); *cigar = hap_result.cigar.data(); *n_cigar = (uint32_t)hap_result.cigar.size();
  return LANCET_OK;
}
extern "C" int lancet_hapcov_emu_coverage(const uint32_t **cov_off, const uint16_t **cov, uint32_t *n_cov) {
  if (hap_result.cov_off.size() != hap_result.h.size() + 1) hap_result.cov_off.assign(hap_result.h.size() + 1, (uint32_t)hap_result.cov.size());
  *cov_off = hap_result.cov_off.data(); *cov = hap_result.cov.data(); *n_cov = (uint32_t)hap_result.cov.size();
  return LANCET_OK;
}
// the windows' length words ([n_windows]) and buffers ([n_windows * cap]) of the last run with the capture on
extern "C" uint32_t lancet_hapcov_emu_raw(const uint32_t **len, const uint32_t **out) { *len = raw_len.data(); *out = raw_out.data(); return hap_words_set; }
extern "C" uint32_t lancet_hapcov_emu_struct_size() { return (uint32_t)sizeof(lancet_haplotype); }
extern "C" uint32_t lancet_hapcov_emu_flag() { return (uint32_t)LANCET_HAP_HAS_COVERAGE; }
