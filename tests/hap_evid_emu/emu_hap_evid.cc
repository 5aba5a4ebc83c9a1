// emu_hap_evid.cc -- TEST INFRASTRUCTURE ONLY.
//
// The host emulation of the kernels (tests/emu/emu_engine.cc, included as it is) with the haplotype capture, its CIGAR and support words,
// the emulated support kernel (lancet_amd/csrc/hap_support.h) AND the emulated evidence kernel (lancet_amd/csrc/hap_evidence.h, the same
// source the engine compiles for the device) over the buffers the window kernels left, as lancet_engine_wait runs them: behind the re-run
// tier, in front of the read-back.  The pattern is tests/hap_place_emu's: buffers, size and switches reach the window kernels through the
// sink of layout.h (LcEmuHapSink); lancet_emu_run here is the emulator's with the capture around it; everything else the library exports
// is the emulator's own, so tests/emu/emu.py drives it unchanged.  With LANCET_EMU_TIER1 in the environment the batch runs twice over the
// SAME buffers, as there; both kernels run once, after both.
//
// lancet_hapevid_emu_hand runs the evidence kernel over ONE hand-written window -- an entry buffer with CIGAR words and a set of packed
// reads the caller lays out -- for the shapes no assembly produces; lancet_hapevid_emu_join is lc_evid_join (host_common.h).
#define lancet_emu_run lancet_emu_run_plain
#include "../emu/emu_engine.cc"
#undef lancet_emu_run
#include "../../lancet_amd/csrc/hap_evidence.h"      // (includes hap_place.h and hap_support.h)
#include <string>

static thread_local uint32_t hap_words_set = 0, hap_aln_set = 0, hap_sup_set = 0, hap_mm_set = 0;
static thread_local LcHapResult hap_result;
static thread_local uint32_t evid_set = 0, evid_mm_set = 0;
static thread_local LcEvidResult evid_result;

// the capture's switches (lancet_hapsup_emu_set's rules) and lancet_engine_set_haplotype_evidence: the same argument rules
extern "C" int lancet_hapevid_emu_set(uint32_t words_per_window, int aln, int sup, int sup_mm, uint32_t evid, int evid_mm, int max_indel_len) {
  if (evid > LC_EVID_CAP_MAX) return LANCET_E_ARG;
  if (evid_mm < 0 || evid_mm > 255) return LANCET_E_ARG;
  lancet_params p; memset(&p, 0, sizeof(p)); p.max_indel_len = max_indel_len;
  if (evid && !lc_place_params_ok(&p)) return LANCET_E_ARG;
  if (words_per_window && words_per_window < LC_HAP_MIN_WORDS) return LANCET_E_ARG;
  if ((aln != 0 && aln != 1) || (sup != 0 && sup != 1) || sup_mm < 0 || sup_mm > 255) return LANCET_E_ARG;
  hap_words_set = words_per_window; hap_aln_set = (uint32_t)aln; hap_sup_set = (uint32_t)sup; hap_mm_set = (uint32_t)sup_mm;
  evid_set = evid; evid_mm_set = (uint32_t)evid_mm;
  return LANCET_OK;
}

// what lancet_engine_wait does behind the kernel: the kept records of every window, dense, then the join
static void collect_evidence(int nw, const std::vector<uint32_t> &ev_len, const uint32_t *rec, uint32_t cap, const lancet_window_stats *st, const int32_t *ref_start,
                             const std::vector<lancet_haplotype> &haps, const lancet_variant *v, size_t nv, LcEvidResult *out) {
  std::vector<uint32_t> off((size_t)nw + 1, 0), dense;
  for (int w = 0; w < nw; ++w) {
    const uint32_t u = lc_evid_used(ev_len[(size_t)w], cap, st[w].status);
    off[(size_t)w + 1] = off[(size_t)w] + u;
    dense.insert(dense.end(), rec + (size_t)w * cap * EV_WORDS, rec + ((size_t)w * cap + u) * EV_WORDS);
  }
  dense.push_back(0);
  lc_evid_collect(nw, ev_len.data(), off.data(), dense.data(), cap, st, ref_start, haps, v, nv, out);
}

extern "C" void *lancet_emu_run(const lancet_params *P, const lancet_window_batch *b, uint32_t evt_cap) {
  const int nw = b->n_windows > 0 ? b->n_windows : 0;
  hap_result.h.clear(); hap_result.words.clear(); hap_result.truncated.assign((size_t)nw, 0);
  hap_result.cigar_off.assign(1, 0u); hap_result.cigar.clear(); hap_result.cov_off.assign(1, 0u); hap_result.cov.clear(); hap_result.sup.clear();
  evid_result.ev.clear(); evid_result.event_off.assign(1, 0u); evid_result.marked.assign((size_t)nw, 0);
  if (!hap_words_set) return lancet_emu_run_plain(P, b, evt_cap);
  const uint32_t cap = hap_words_set;
  std::vector<uint32_t> raw_len((size_t)nw + 1, 0), raw_out((size_t)nw * cap + 2, 0xCDCDCDCDu);      // (HBM is not zeroed; the lengths are cleared per upload)
  uint32_t *out0 = raw_out.data() + ((reinterpret_cast<uintptr_t>(raw_out.data()) & 7u) ? 1 : 0);
  lc_emu_hap_sink.cap = cap; lc_emu_hap_sink.len = raw_len.data(); lc_emu_hap_sink.out = out0; lc_emu_hap_sink.aln = hap_aln_set; lc_emu_hap_sink.cov = 0;
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
  const lancet_window_stats *st = lancet_emu_stats(h);
  const bool evid_on = evid_set && hap_aln_set;                    // (the engine's rule: nothing without the alignments)
  std::vector<uint32_t> ev_len((size_t)nw + 1, 0u), rec;
  if ((hap_sup_set || evid_on) && nw > 0) {
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
    if (hap_sup_set) {
      static thread_local SupShared SS;
      memset(&SS, 0xCD, sizeof(SS));
      for (int w = 0; w < nw; ++w) hap_support_window(&B, raw_len.data(), out0, cap, hap_mm_set, w, &SS);
    }
    if (evid_on) {
      rec.assign((size_t)nw * evid_set * EV_WORDS + 1, 0u);                          // (zeroed per run, as the engine's)
      static thread_local EvShared ES;
      memset(&ES, 0xCD, sizeof(ES));
      for (int w = 0; w < nw; ++w) hap_evidence_window(&B, raw_len.data(), out0, cap, evid_mm_set, rec.data(), ev_len.data(), evid_set, w, &ES);
    }
  }
  if (out0 != raw_out.data()) raw_out.erase(raw_out.begin());
  std::vector<uint32_t> off((size_t)nw + 1, 0), dense;
  for (int w = 0; w < nw; ++w) {
    const uint32_t u = lc_hap_used(raw_len[(size_t)w], cap, st[w].status);
    off[(size_t)w + 1] = off[(size_t)w] + u;
    dense.insert(dense.end(), raw_out.begin() + (size_t)w * cap, raw_out.begin() + (size_t)w * cap + u);
  }
  dense.push_back(0);
  lc_hap_collect(nw, raw_len.data(), off.data(), dense.data(), st, &hap_result);
  if (evid_on && nw > 0) {
    // the records in the engine's order, as tests/emu/emu.py returns them: those of windows with a result, by (window, seq_in_window)
    std::vector<lancet_variant> vs;
    const lancet_variant *raw = lancet_emu_variants(h);
    for (uint32_t i = 0; i < lancet_emu_n_variants(h); ++i) if (st[raw[i].window].status >= 0) vs.push_back(raw[i]);
    std::stable_sort(vs.begin(), vs.end(), [](const lancet_variant &a, const lancet_variant &c) { return a.window != c.window ? a.window < c.window : a.seq_in_window < c.seq_in_window; });
    collect_evidence(nw, ev_len, rec.data(), evid_set, st, b->ref_start, hap_result.h, vs.data(), vs.size(), &evid_result);
  }
  return h;
}

extern "C" int lancet_hapevid_emu_results(const lancet_haplotype **h, uint32_t *n, const uint32_t **words, uint32_t *n_words, const uint8_t **truncated) {
  *h = hap_result.h.data(); *n = (uint32_t)hap_result.h.size(); *words = hap_result.words.data(); *n_words = (uint32_t)hap_result.words.size();
  *truncated = hap_result.truncated.data();
  return LANCET_OK;
}
extern "C" int lancet_hapevid_emu_cigars(const uint32_t **cigar_off, const uint32_t **cigar, uint32_t *n_cigar) {
  *cigar_off = hap_result.cigar_off.data(); *cigar = hap_result.cigar.data(); *n_cigar = (uint32_t)hap_result.cigar.size();
  return LANCET_OK;
}
extern "C" int lancet_hapevid_emu_support(const uint32_t **support) {
  *support = (hap_result.sup.size() == (size_t)HP_SUP_WORDS * hap_result.h.size() && !hap_result.sup.empty()) ? hap_result.sup.data() : nullptr;
  return LANCET_OK;
}
// lancet_engine_results_haplotype_evidence of the last run on this thread
extern "C" int lancet_hapevid_emu_evidence(const lancet_variant_evidence **ev, uint32_t *n_events, const uint32_t **event_off, const uint8_t **marked) {
  if (evid_result.event_off.size() != hap_result.h.size() + 1) evid_result.event_off.assign(hap_result.h.size() + 1, 0u);
  *ev = evid_result.ev.empty() ? nullptr : evid_result.ev.data(); *n_events = (uint32_t)evid_result.ev.size();
  *event_off = evid_result.event_off.data(); *marked = evid_result.marked.data();
  return LANCET_OK;
}

// One hand-written window: buf[hcap] its buffer, len_word its length word (HP_TRUNC and all); n_reads reads with their info words, word
// offsets and packed bases; cap records.  The entries are collected as the read-back collects them, the records as the results call
// returns them (status 0, no records of variants: every `variant` is -1).  out[out_cap], event_off[off_cap]; *n_events / *n_haps: how many
// there are; returns the window's mark, or -1 when an array is too small.
extern "C" int lancet_hapevid_emu_hand(const uint32_t *buf, uint32_t len_word, uint32_t hcap, const uint32_t *rinfo, const uint32_t *base_woff, const uint32_t *bases,
                                       uint32_t n_reads, uint32_t max_mm, uint32_t cap, lancet_variant_evidence *out, uint32_t out_cap, uint32_t *n_events,
                                       uint32_t *event_off, uint32_t off_cap, uint32_t *n_haps) {
  const uint32_t read_begin[2] = {0u, n_reads};
  DevBatch B; memset(&B, 0, sizeof(B));
  B.n_windows = 1; B.read_begin = read_begin; B.rinfo = rinfo; B.base_woff = base_woff; B.bases = bases;
  std::vector<uint32_t> rec((size_t)cap * EV_WORDS + 1, 0u), ev_len(2, 0u);
  static thread_local EvShared ES;
  memset(&ES, 0xCD, sizeof(ES));
  hap_evidence_window(&B, &len_word, buf, hcap, max_mm, rec.data(), ev_len.data(), cap, 0, &ES);
  lancet_window_stats st; memset(&st, 0, sizeof(st));
  const uint32_t used = lc_hap_used(len_word, hcap, 0);
  const uint32_t off[2] = {0u, used};
  std::vector<uint32_t> dense(buf, buf + used); dense.push_back(0);
  LcHapResult hr;
  lc_hap_collect(1, &len_word, off, dense.data(), &st, &hr);
  const int32_t ref_start = 1;
  LcEvidResult r;
  collect_evidence(1, ev_len, rec.data(), cap, &st, &ref_start, hr.h, nullptr, 0, &r);
  *n_events = (uint32_t)r.ev.size(); *n_haps = (uint32_t)hr.h.size();
  if (r.ev.size() > out_cap || r.event_off.size() > off_cap) return -1;
  for (size_t i = 0; i < r.ev.size(); ++i) out[i] = r.ev[i];
  for (size_t i = 0; i < r.event_off.size(); ++i) event_off[i] = r.event_off[i];
  return (int)r.marked[0];
}

// lc_evid_join over one record: the haplotype's first_variant, n_variants and ref_off, the event's rb, the window's start; the record's
// seq_in_window and pos.  Returns 0 where they are joined, -1 where not.
extern "C" int lancet_hapevid_emu_join(int32_t first_variant, int32_t n_variants, uint32_t ref_off, uint32_t rb, int32_t ref_start, int32_t seq_in_window, int32_t pos) {
  lancet_haplotype h; memset(&h, 0, sizeof(h)); h.first_variant = first_variant; h.n_variants = n_variants; h.ref_off = ref_off;
  lancet_variant v; memset(&v, 0, sizeof(v)); v.seq_in_window = seq_in_window; v.pos = pos;
  return lc_evid_join(h, rb, ref_start, &v, 0, 1);
}
extern "C" uint32_t lancet_hapevid_emu_struct_size() { return (uint32_t)sizeof(lancet_variant_evidence); }
// LC_EV_ENTS, LC_EV_EVENTS, LC_EV_POOL, LC_SUP_WAVES, EV_WORDS: what the kernel was compiled with
extern "C" void lancet_hapevid_emu_consts(uint32_t out[5]) { out[0] = LC_EV_ENTS; out[1] = LC_EV_EVENTS; out[2] = LC_EV_POOL; out[3] = LC_SUP_WAVES; out[4] = EV_WORDS; }
