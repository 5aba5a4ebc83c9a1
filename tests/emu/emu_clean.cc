// emu_clean.cc -- TEST INFRASTRUCTURE ONLY (tests/test_clean_passes_emu.py compiles it on its own, once plain and once with -DLANCET_FAT=1;
// the Makefile's libraries do not hold it).
//
// The three per-component cleaning passes alone, on a hand-made graph: remove_low_cov_wg, remove_tips_wg and remove_short_links_wg of
// kernels.h (with pass_candidates_wg, clean_dead_flags_wg and compress_wg under them), which state Graph_t::removeLowCov(true, comp),
// removeTips and removeShortLinks (reference src/Graph.cc:2768-2926) -- each pass alone from the same start state, and the three in
// process_window's order -- next to the plain model of those lines in emu_graph_model.h.  The model takes the answer of findTandems per node
// from the case (the test holds it against the oracle's findTandems first); the kernels compute it from the node's string.
#define LANCET_WAVE_EMU 1
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#ifndef LANCET_EMU_KERNELS_H
#define LANCET_EMU_KERNELS_H "../../lancet_amd/csrc/kernels.h"
#endif
#include LANCET_EMU_KERNELS_H

#include "emu_graph_model.h"

namespace {
// settings of a case: ip[] = totalreadbp, reflen, low_cov_threshold, max_tip_len, max_unit_len, min_report_units, min_report_len, dist_from_str, path_cap, comp,
// precompress (1: compress_wg / the model's compress run first, as process_window's first compress does: the start state of every block is its result)
enum { IP_TOTALREADBP, IP_REFLEN, IP_LOW_COV, IP_MAX_TIP, IP_MAX_UNIT, IP_MIN_UNITS, IP_MIN_LEN, IP_DIST, IP_PATH_CAP, IP_COMP, IP_PRECOMPRESS, IP_WORDS };
// counts of a block: 0 low coverage found (-1: the pass did not run)  1 links removed (-1)  2 tip rounds  3.. tips removed per round
enum { CNT_WORDS = 16, EVT_WORDS = 8 * 1024 };

struct CleanRig : Rig {
  CleanRig(const Input &in, const int32_t *ip, double ratio) : Rig(in) {
    P.low_cov_threshold = ip[IP_LOW_COV]; P.max_tip_len = ip[IP_MAX_TIP]; P.min_cov_ratio = ratio;
    P.max_unit_len = ip[IP_MAX_UNIT]; P.min_report_units = ip[IP_MIN_UNITS]; P.min_report_len = ip[IP_MIN_LEN]; P.dist_from_str = ip[IP_DIST];
    C.path_cap = (uint32_t)ip[IP_PATH_CAP]; C.evt_cap = EVT_WORDS; C.evt_level = 1;
    pseq.assign((size_t)ip[IP_PATH_CAP] + 64, 0); evt.assign(EVT_WORDS, 0);
    W.pseq = pseq.data(); W.evt = evt.data();
    S.totalreadbp = ip[IP_TOTALREADBP]; S.reflen = ip[IP_REFLEN];
  }
  void counts(int32_t *cnt) const {                                   // what the passes reported, read off their trace events
    for (int i = 0; i < CNT_WORDS; ++i) cnt[i] = 0;
    cnt[0] = -1; cnt[1] = -1;
    for (uint32_t at = 0; at + 8 <= S.evt_len; at += 8) {
      const uint32_t code = evt[at], a = evt[at + 1];
      if (code == EV_LOWCOV) cnt[0] = (int32_t)a;
      else if (code == EV_LINKS) cnt[1] = (int32_t)a;
      else if (code == EV_TIPS_ROUND) { if ((int)a != cnt[2] + 1) cnt[CNT_WORDS - 1] = -1; cnt[2] = (int32_t)a; }      // (rounds count 1, 2, 3 ..)
      else if (code == EV_TIPS_REMOVED && cnt[2] >= 1 && 2 + cnt[2] < CNT_WORDS - 1) cnt[2 + cnt[2]] = (int32_t)a;
    }
  }
};
void model_counts(const Model &m, int32_t *cnt) {
  for (int i = 0; i < CNT_WORDS; ++i) cnt[i] = 0;
  cnt[0] = m.counts.lowcov; cnt[1] = m.counts.links; cnt[2] = (int32_t)m.counts.tips.size();
  for (size_t r = 0; r < m.counts.tips.size() && 3 + r < (size_t)CNT_WORDS - 1; ++r) cnt[3 + r] = m.counts.tips[r];
}
Model clean_model(const Input &in, const int32_t *ip, double ratio, const uint8_t *in_str) {
  Model m = make_model(in);
  m.totalreadbp = ip[IP_TOTALREADBP]; m.reflen = (size_t)ip[IP_REFLEN]; m.LOW_COV_THRESHOLD = ip[IP_LOW_COV]; m.MAX_TIP_LEN = ip[IP_MAX_TIP]; m.MIN_COV_RATIO = ratio;
  m.path_cap = (size_t)ip[IP_PATH_CAP];
  for (uint32_t n = 0; n < in.n_rec; ++n) m.nodes[n].in_str = in_str[n] != 0;
  return m;
}
}  // namespace

// out: ten blocks of 3 + n_rec + n_rec * (24 + len_max) words, cnt: ten blocks of 16 --
//   0 remove_low_cov_wg  1 remove_tips_wg  2 remove_short_links_wg  3 the three in process_window's order      (the kernels)
//   4 removeLowCov       5 removeTips      6 removeShortLinks       7 the three in that order                  (the model)
//   8 the model after removeLowCov and removeTips: the graph its removeShortLinks of block 7 starts from
//   9 the model's start state (after the first compress, where the case asks for one)
// in_str / in_str_seq [n_rec]: findTandems' answer for the node's string at the start (blocks 6) and in the state of block 8 (block 7); the test reads both states
// off a first call and asks the oracle.
extern "C" void lancet_emu_clean(uint32_t n_rec, uint32_t M, const uint32_t *order, const uint32_t *rec, const uint32_t *seq, uint32_t seq_top, uint32_t seq_cap,
                                 const uint16_t *qv, uint32_t qv_rows, int K, uint32_t len_max, const int32_t *ip, double min_cov_ratio,
                                 const uint8_t *in_str, const uint8_t *in_str_seq, uint32_t *out, int32_t *cnt) {
  Input in; in.n_rec = n_rec; in.M = M; in.order = order; in.rec = rec; in.seq = seq; in.seq_top = seq_top; in.seq_cap = seq_cap; in.qv = qv; in.qv_rows = qv_rows; in.K = K; in.len_max = len_max;
  const size_t BW = 3 + (size_t)n_rec + (size_t)n_rec * (OUT_HEAD + len_max);
  const int comp = ip[IP_COMP];
  for (int pass = 0; pass < 4; ++pass) {
    CleanRig r(in, ip, min_cov_ratio);
    if (ip[IP_PRECOMPRESS]) { compress_wg(r.c, comp); r.S.evt_len = 0; }
    if (pass == 0 || pass == 3) remove_low_cov_wg(r.c, comp);
    if (pass == 1 || (pass == 3 && !r.S.overflow)) remove_tips_wg(r.c, comp);
    if (pass == 2 || (pass == 3 && !r.S.overflow)) remove_short_links_wg(r.c, comp);
    r.dump(in, 0, out + pass * BW);
    r.counts(cnt + pass * CNT_WORDS);
  }
  {
    Model m = clean_model(in, ip, min_cov_ratio, in_str);
    if (ip[IP_PRECOMPRESS]) m.compress(comp);
    dump_model(in, m, out + 9 * BW); model_counts(m, cnt + 9 * CNT_WORDS);
  }
  for (int pass = 0; pass < 4; ++pass) {
    Model m = clean_model(in, ip, min_cov_ratio, pass == 3 ? in_str_seq : in_str);
    if (ip[IP_PRECOMPRESS]) m.compress(comp);
    if (pass == 0 || pass == 3) m.remove_low_cov(comp);
    if (pass == 1 || (pass == 3 && !m.overflow)) m.remove_tips(comp);
    if (pass == 3) { dump_model(in, m, out + 8 * BW); model_counts(m, cnt + 8 * CNT_WORDS); }
    if (pass == 2 || (pass == 3 && !m.overflow)) m.remove_short_links(comp);
    dump_model(in, m, out + (4 + pass) * BW);
    model_counts(m, cnt + (4 + pass) * CNT_WORDS);
  }
}
