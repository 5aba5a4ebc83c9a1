// emu_hap.cc -- TEST INFRASTRUCTURE ONLY.
//
// The host emulation of the kernels (tests/emu/emu_engine.cc, included as it is) with the haplotype capture: the emulator's driver knows
// nothing of it, so the buffers reach the kernels through the sink of layout.h (LcEmuHapSink), which lc_caps_for_sizes and the kernels
// read in an emulation build.  lancet_emu_run here is the emulator's with the capture around it; everything else the library exports is
// the emulator's own, so tests/emu/emu.py drives it unchanged (hap_emu.py puts this library in its place for the length of a run).
//
// The engine's two tiers: with LANCET_EMU_TIER1 in the environment the batch runs twice over the SAME buffers -- first with the tier-1
// work space the variable asks for, then with the re-run tier's -- and only the first run starts from cleared length words, as an
// upload leaves them.  The second run starts every window over (kernels.h process_window), as the engine's re-run tier does for the
// windows it takes: a window must come out with each of its haplotypes once.
#define lancet_emu_run lancet_emu_run_plain
#include "../emu/emu_engine.cc"
#undef lancet_emu_run
#include <string>

static thread_local uint32_t hap_words_set = 0;
static thread_local LcHapResult hap_result;

// lancet_engine_set_haplotypes: 0 = off
extern "C" int lancet_hap_emu_set(uint32_t words_per_window) {
  if (words_per_window && words_per_window < LC_HAP_MIN_WORDS) return LANCET_E_ARG;
  hap_words_set = words_per_window;
  return LANCET_OK;
}

extern "C" void *lancet_emu_run(const lancet_params *P, const lancet_window_batch *b, uint32_t evt_cap) {
  const int nw = b->n_windows > 0 ? b->n_windows : 0;
  hap_result.h.clear(); hap_result.words.clear(); hap_result.truncated.assign((size_t)nw, 0);
  if (!hap_words_set) return lancet_emu_run_plain(P, b, evt_cap);
  const uint32_t cap = hap_words_set;
  std::vector<uint32_t> len((size_t)nw + 1, 0), out((size_t)nw * cap + 1, 0xCDCDCDCDu);      // (HBM is not zeroed; the lengths are cleared per upload)
  lc_emu_hap_sink.cap = cap; lc_emu_hap_sink.len = len.data(); lc_emu_hap_sink.out = out.data();
  void *h = nullptr;
  if (const char *t1 = getenv("LANCET_EMU_TIER1")) {
    const std::string keep = t1;
    lancet_emu_free(lancet_emu_run_plain(P, b, evt_cap));
    unsetenv("LANCET_EMU_TIER1");
    h = lancet_emu_run_plain(P, b, evt_cap);
    setenv("LANCET_EMU_TIER1", keep.c_str(), 1);
  } else h = lancet_emu_run_plain(P, b, evt_cap);
  lc_emu_hap_sink.cap = 0; lc_emu_hap_sink.len = nullptr; lc_emu_hap_sink.out = nullptr;
  // what lancet_engine_wait does: the used words of every window, dense, then the entries
  const lancet_window_stats *st = lancet_emu_stats(h);
  std::vector<uint32_t> off((size_t)nw + 1, 0), dense;
  for (int w = 0; w < nw; ++w) {
    const uint32_t u = lc_hap_used(len[(size_t)w], cap, st[w].status);
    off[(size_t)w + 1] = off[(size_t)w] + u;
    dense.insert(dense.end(), out.begin() + (size_t)w * cap, out.begin() + (size_t)w * cap + u);
  }
  dense.push_back(0);
  lc_hap_collect(nw, len.data(), off.data(), dense.data(), st, &hap_result);
  return h;
}

// lancet_engine_results_haplotypes of the last run on this thread
extern "C" int lancet_hap_emu_results(const lancet_haplotype **h, uint32_t *n, const uint32_t **words, uint32_t *n_words, const uint8_t **truncated) {
  *h = hap_result.h.data(); *n = (uint32_t)hap_result.h.size(); *words = hap_result.words.data(); *n_words = (uint32_t)hap_result.words.size();
  *truncated = hap_result.truncated.data();
  return LANCET_OK;
}
extern "C" uint32_t lancet_hap_emu_struct_size() { return (uint32_t)sizeof(lancet_haplotype); }
