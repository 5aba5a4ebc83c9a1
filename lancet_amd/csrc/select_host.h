// select_host.h -- host side of the device read selection, between its two passes: which slices the route takes at all, and from the
// per-window summaries of pass 1 the batch's kept[], read_begin and sizes.  Plain C++, shared by engine.hip and the emulation build
// (tests/select_emu), so that what is "not taken" is decided by the same lines with and without a GPU.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>
#include "select_rules.h"
#include "../../include/lancet_host.h"

// why a slice goes through the host route before anything is looked at on the device ("" = no reason)
static inline std::string sel_precheck(uint64_t table_load_id, const lancet_window_slice *s, const lancet_host_opts *o) {
  if (o->linked) return "linked reads: barcodes and haplotypes are assembled on the host";
  if (s->host_reason == LANCET_SLICE_RG_FILE) return "rg-file: the read-group filter of the active-region test is sequential state";
  if (s->host_reason == LANCET_SLICE_NOT_LOADED) return "not loaded: the range's alignments are loaded batch by batch";
  if (s->host_reason) return "host reason " + std::to_string(s->host_reason);
  if (table_load_id && s->load_id != table_load_id) return "not loaded: the resident table is of another load than the range";
  if (s->leak_reads) return "leak: " + std::to_string(s->leak_reads) + " reads of earlier windows are still in the graph";
  return "";
}

struct SelPlan {
  std::vector<int32_t> kslice;                    // kept window k -> its place in the slice
  std::vector<uint32_t> read_begin, ref_off;      // [nk + 1]
  std::vector<uint32_t> wbases;                   // [nk] untrimmed bases of the window's reads
  int need_large = 0;                             // windows beyond the 512-lane LDS build configuration (lds_reads / lds_bases: its limits)
  std::string reason;                             // not taken when set
};
static inline SelPlan sel_plan(const lancet_window_slice *s, const lancet_select_summary *sum, uint32_t lds_reads, uint32_t lds_bases) {
  SelPlan p; p.read_begin.assign(1, 0); p.ref_off.assign(1, 0);
  uint64_t R = 0;
  for (int32_t i = 0; i < s->n_windows; ++i) {
    const lancet_select_summary &m = sum[i];
    const uint32_t st = m.status & 3u, n = m.reads_t + m.reads_n;
    if (m.status & SEL_ST_EVT_OVERFLOW) { p.reason = "oversize: a window has more evidence positions than the selection kernel counts"; return p; }
    if (st != SEL_ST_KEPT) continue;               // filtered, or skipped for coverage (the graph is cleared: nothing leaks either way)
    if (n > SEL_CAP) { p.reason = "oversize: a window selects " + std::to_string(n) + " reads, the selection kernel stages " + std::to_string(SEL_CAP); return p; }
    if (n > 0 && !(m.status & SEL_ST_MAPPED)) { p.reason = "leak: a kept window has reads but no mapped read, they stay in the graph"; return p; }
    R += n;
    if (R > 0xFFFFFFF0ull) { p.reason = "oversize: more than 2^32 reads in the batch"; return p; }
    const uint32_t rl = s->ref_off[i + 1] - s->ref_off[i];
    p.kslice.push_back(i); p.read_begin.push_back((uint32_t)R); p.ref_off.push_back(p.ref_off.back() + rl); p.wbases.push_back(m.bases);
    const uint64_t wb = (rl + 15u) / 16u + (uint64_t)m.tw16, wg = (rl + 31u) / 32u + (uint64_t)m.tw32;
    if (n > lds_reads || wb > lds_bases / 16u || wg > lds_bases / 32u) ++p.need_large;
  }
  return p;
}
static inline SelTable sel_table_of(const lancet_alignment_table *t) {       // (host pointers: the emulation; the engine fills device pointers in)
  SelTable T; T.n_chroms = t->n_chroms; T.n_aln[0] = t->n_aln[0]; T.n_aln[1] = t->n_aln[1];
  T.span = t->span; T.pos0 = t->pos0; T.ref_len = t->ref_len; T.l_seq = t->l_seq; T.flags = t->flags; T.rinfo = t->rinfo; T.evt_off = t->evt_off;
  T.evt_kind = t->evt_kind; T.evt_pos = t->evt_pos; T.name_off = t->name_off; T.names = t->names; T.base_woff = t->base_woff; T.good_woff = t->good_woff;
  return T;
}
static inline SelOpts sel_opts_of(const lancet_host_opts *o) { SelOpts O; O.active_region = o->active_region; O.min_evidence = o->min_evidence; O.max_avg_cov = o->max_avg_cov; O.reserved = 0; return O; }

// What the kernels index with values of the table is checked here, once: spans inside the sample, CSR offsets monotone and inside the
// event arrays, name offsets inside the blob and the blob terminated.  "" when the table is sound.
static inline const char *sel_table_check(const lancet_alignment_table *t) {
  const uint64_t N = (uint64_t)t->n_aln[0] + t->n_aln[1];
  if (N + 1 > 0xFFFFFFFFull) return "too many alignments";
  if (N && (!t->pos0 || !t->ref_len || !t->l_seq || !t->flags || !t->rinfo || !t->evt_off || !t->name_off || !t->names || !t->base_woff || !t->good_woff)) return "an array is missing";
  if (!t->bases || !t->good) return "the packed words are missing";
  if (t->n_chroms && !t->span) return "span is missing";
  for (uint32_t s = 0; s < 2; ++s) for (uint32_t c = 0; c < t->n_chroms; ++c) {
    const uint32_t a = t->span[(s * t->n_chroms + c) * 2], b = t->span[(s * t->n_chroms + c) * 2 + 1];
    const uint32_t lo = s ? t->n_aln[0] : 0u, hi = lo + t->n_aln[s];
    if (a > b || a < lo || b > hi) return "a contig's span lies outside its sample";
  }
  if (N) {
    if (t->evt_off[0] != 0) return "evt_off does not start at 0";
    for (uint64_t i = 0; i < N; ++i) if (t->evt_off[i + 1] < t->evt_off[i]) return "evt_off is not monotone";
    if (t->evt_off[N] && (!t->evt_kind || !t->evt_pos)) return "the event arrays are missing";
    if (t->names_len == 0 || t->names[t->names_len - 1] != 0) return "the name blob is not terminated";
    for (uint64_t i = 0; i < N; ++i) {
      if (t->name_off[i] >= t->names_len) return "a name offset lies outside the blob";
      if ((uint64_t)t->base_woff[i] + (t->l_seq[i] + 15u) / 16u > t->n_base_words || (uint64_t)t->good_woff[i] + (t->l_seq[i] + 31u) / 32u > t->n_good_words) return "a read's words lie outside the packed arrays";
    }
  }
  return "";
}
