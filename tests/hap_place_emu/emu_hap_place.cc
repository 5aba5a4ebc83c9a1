// emu_hap_place.cc -- TEST INFRASTRUCTURE ONLY.
//
// The host emulation of the kernels (tests/emu/emu_engine.cc, included as it is) with the haplotype capture, its CIGAR and support words,
// the emulated support kernel (lancet_amd/csrc/hap_support.h) AND the emulated placement kernel (lancet_amd/csrc/hap_place.h, the same
// source the engine compiles for the device) over the buffers the window kernels left, as lancet_engine_wait runs them: behind the re-run
// tier, in front of the read-back.  The pattern is tests/hap_sup_emu's: buffers, size and switches reach the window kernels through the
// sink of layout.h (LcEmuHapSink); lancet_emu_run here is the emulator's with the capture around it; everything else the library exports
// is the emulator's own, so tests/emu/emu.py drives it unchanged.  With LANCET_EMU_TIER1 in the environment the batch runs twice over the
// SAME buffers, as there; both kernels run once, after both.
//
// lancet_happlace_emu_hand runs the placement kernel over ONE hand-written window -- an entry buffer and a set of packed reads the caller
// lays out -- for the shapes no assembly produces; lancet_happlace_emu_read_cigar is lc_read_cigar (host_common.h).
#define lancet_emu_run lancet_emu_run_plain
#include "../emu/emu_engine.cc"
#undef lancet_emu_run
#include "../../lancet_amd/csrc/hap_place.h"      // (includes hap_support.h)
#include <string>

static thread_local uint32_t hap_words_set = 0, hap_aln_set = 0, hap_sup_set = 0, hap_mm_set = 0;
static thread_local LcHapResult hap_result;
static thread_local std::vector<uint32_t> raw_len, raw_out;       // the windows' length words and buffers as the last run left them
static thread_local uint32_t place_set = 0, place_mm_set = 0;
static thread_local LcPlaceResult place_result;

// the capture's switches (lancet_hapsup_emu_set's rules) and lancet_engine_set_haplotype_placements: the same argument rules
extern "C" int lancet_happlace_emu_set(uint32_t words_per_window, int aln, int cov, int sup, int sup_mm, int place, int place_mm, int max_indel_len) {
  if (place != 0 && place != 1) return LANCET_E_ARG;
  if (place_mm < 0 || place_mm > 255) return LANCET_E_ARG;
  lancet_params p; memset(&p, 0, sizeof(p)); p.max_indel_len = max_indel_len;
  if (place && (!lc_place_words_ok(words_per_window) || !lc_place_params_ok(&p))) return LANCET_E_ARG;
  if (words_per_window && words_per_window < LC_HAP_MIN_WORDS) return LANCET_E_ARG;
  if ((aln != 0 && aln != 1) || cov != 0 || (sup != 0 && sup != 1) || sup_mm < 0 || sup_mm > 255) return LANCET_E_ARG;      // (coverage words: tests/hap_cov_emu, hap_sup_emu)
  hap_words_set = words_per_window; hap_aln_set = (uint32_t)aln; hap_sup_set = (uint32_t)sup; hap_mm_set = (uint32_t)sup_mm;
  place_set = (uint32_t)place; place_mm_set = (uint32_t)place_mm;
  return LANCET_OK;
}

extern "C" void *lancet_emu_run(const lancet_params *P, const lancet_window_batch *b, uint32_t evt_cap) {
  const int nw = b->n_windows > 0 ? b->n_windows : 0;
  hap_result.h.clear(); hap_result.words.clear(); hap_result.truncated.assign((size_t)nw, 0);
  hap_result.cigar_off.assign(1, 0u); hap_result.cigar.clear(); hap_result.cov_off.assign(1, 0u); hap_result.cov.clear(); hap_result.sup.clear();
  place_result.p.clear(); place_result.tlen.clear(); place_result.read_begin.assign(1, 0u);
  raw_len.clear(); raw_out.clear();
  if (!hap_words_set) return lancet_emu_run_plain(P, b, evt_cap);
  const uint32_t cap = hap_words_set;
  // (HBM is not zeroed; the lengths are cleared per upload.  One spare word in front when the size is odd keeps window 0's buffer 8-byte
  //  aligned as a device allocation is)
  raw_len.assign((size_t)nw + 1, 0); raw_out.assign((size_t)nw * cap + 2, 0xCDCDCDCDu);
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
  // ---- the two kernels, one emulated workgroup per window each, over the resident batch as the driver lays it out (emu_engine.cc: the words
  // of every read, trimmed and packed by prep_read) and the buffers as they are
  if ((hap_sup_set || place_set) && nw > 0) {
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
    if (place_set) {
      std::vector<uint32_t> rec((size_t)PL_WORDS * R + 2, 0u);                      // (zeroed per run, as the engine's)
      uint32_t *rec0 = rec.data() + ((reinterpret_cast<uintptr_t>(rec.data()) & 7u) ? 1 : 0);
      static thread_local PlShared PS;
      memset(&PS, 0xCD, sizeof(PS));
      for (int w = 0; w < nw; ++w) hap_placement_window(&B, raw_len.data(), out0, cap, place_mm_set, rec0, w, &PS);
      lc_place_collect(nw, b->read_begin, rinfo.data(), rec0, st, &place_result);
    }
  }
  if (out0 != raw_out.data()) raw_out.erase(raw_out.begin());
  // what lancet_engine_wait does: the used words of every window, dense, then the entries
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

// lancet_engine_results_haplotypes / _haplotype_alignments / _haplotype_support of the last run on this thread, and its raw buffers
extern "C" int lancet_happlace_emu_results(const lancet_haplotype **h, uint32_t *n, const uint32_t **words, uint32_t *n_words, const uint8_t **truncated) {
  *h = hap_result.h.data(); *n = (uint32_t)hap_result.h.size(); *words = hap_result.words.data(); *n_words = (uint32_t)hap_result.words.size();
  *truncated = hap_result.truncated.data();
  return LANCET_OK;
}
extern "C" int lancet_happlace_emu_cigars(const uint32_t **cigar_off, const uint32_t **cigar, uint32_t *n_cigar) {
  *cigar_off = hap_result.cigar_off.data(); *cigar = hap_result.cigar.data(); *n_cigar = (uint32_t)hap_result.cigar.size();
  return LANCET_OK;
}
extern "C" int lancet_happlace_emu_support(const uint32_t **support) {
  *support = (hap_result.sup.size() == (size_t)HP_SUP_WORDS * hap_result.h.size() && !hap_result.sup.empty()) ? hap_result.sup.data() : nullptr;
  return LANCET_OK;
}
extern "C" uint32_t lancet_happlace_emu_raw(const uint32_t **len, const uint32_t **out) { *len = raw_len.data(); *out = raw_out.data(); return hap_words_set; }

// lancet_engine_results_haplotype_placements of the last run on this thread
extern "C" int lancet_happlace_emu_placements(const lancet_read_placement **p, uint32_t *n_reads, const uint32_t **read_begin, const uint16_t **tlen) {
  const bool have = !place_result.p.empty();
  if (place_result.read_begin.empty()) place_result.read_begin.assign(1, 0u);
  *p = have ? place_result.p.data() : nullptr; *n_reads = (uint32_t)place_result.p.size();
  *read_begin = place_result.read_begin.data(); *tlen = have ? place_result.tlen.data() : nullptr;
  return LANCET_OK;
}

// One hand-written window: buf[cap] its buffer, len_word its length word (HP_TRUNC and all); n_reads reads with their info words, word
// offsets and packed bases.  out[n_reads]: the records as the results call would return them (status 0).
extern "C" int lancet_happlace_emu_hand(const uint32_t *buf, uint32_t len_word, uint32_t cap, const uint32_t *rinfo, const uint32_t *base_woff, const uint32_t *bases,
                                        uint32_t n_reads, uint32_t max_mm, lancet_read_placement *out, uint16_t *tlen) {
  const uint32_t read_begin[2] = {0u, n_reads};
  DevBatch B; memset(&B, 0, sizeof(B));
  B.n_windows = 1; B.read_begin = read_begin; B.rinfo = rinfo; B.base_woff = base_woff; B.bases = bases;
  std::vector<uint32_t> rec((size_t)PL_WORDS * n_reads + 2, 0u);
  uint32_t *rec0 = rec.data() + ((reinterpret_cast<uintptr_t>(rec.data()) & 7u) ? 1 : 0);
  static thread_local PlShared PS;
  memset(&PS, 0xCD, sizeof(PS));
  hap_placement_window(&B, &len_word, buf, cap, max_mm, rec0, 0, &PS);
  lancet_window_stats st; memset(&st, 0, sizeof(st));
  LcPlaceResult r;
  lc_place_collect(1, read_begin, rinfo, rec0, &st, &r);
  for (uint32_t i = 0; i < n_reads; ++i) { out[i] = r.p[i]; tlen[i] = r.tlen[i]; }
  return LANCET_OK;
}

// lc_read_cigar: the ops into out[out_cap] (length << 4 | BAM op), *n_out of them; returns 1 with an M, 0 without, -1 when out is too small
extern "C" int lancet_happlace_emu_read_cigar(int32_t o, uint32_t t, uint32_t M, uint32_t ref_off, const uint32_t *cig, uint32_t ncig, uint32_t *start, uint32_t *out, uint32_t out_cap,
                                              uint32_t *n_out) {
  std::vector<uint32_t> v;
  const bool m = lc_read_cigar(o, t, M, ref_off, cig, ncig, start, &v);
  *n_out = (uint32_t)v.size();
  if (v.size() > out_cap) return -1;
  for (size_t i = 0; i < v.size(); ++i) out[i] = v[i];
  return m ? 1 : 0;
}
extern "C" uint32_t lancet_happlace_emu_struct_size() { return (uint32_t)sizeof(lancet_read_placement); }
// LC_PL_ENTS, LC_PL_STAGE, PL_CNT_MAX, LC_SUP_WAVES, PL_IDX_MAX, LC_HAP_MIN_WORDS: what the kernel was compiled with
extern "C" void lancet_happlace_emu_consts(uint32_t out[6]) { out[0] = LC_PL_ENTS; out[1] = LC_PL_STAGE; out[2] = PL_CNT_MAX; out[3] = LC_SUP_WAVES; out[4] = PL_IDX_MAX; out[5] = LC_HAP_MIN_WORDS; }
