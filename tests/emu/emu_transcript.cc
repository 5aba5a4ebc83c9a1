// emu_transcript.cc -- TEST INFRASTRUCTURE ONLY (tests/test_transcript_rules_emu.py compiles it on its own; the Makefile's libraries do not hold it).
//
// The rules of the transcript walk alone (kernels.h walk_column, walk_extend, ts_record_cov), fed with hand-made lists of column values
// instead of a path: what the two walk drivers share, without either driver.  The model they are compared with is the test's.
#define LANCET_WAVE_EMU 1
#include <cstdio>
#include <cstdlib>
#include "../../lancet_amd/csrc/kernels.h"

namespace {
const int REC = 35;            // ints per position: col code P pos_in_ref flags | cn4 ct4 rn2 rt2 | path hp nh nq th tq | reference hp nh th
WalkPos pos_of(const int32_t *r) {
  WalkPos v;
  v.col = r[0]; v.code = (char)r[1]; v.P = r[2]; v.pos_in_ref = (uint32_t)r[3];
  v.tumor = (r[4] & 1) != 0; v.no_spanner = (r[4] & 2) != 0; v.p_outside = (r[4] & 4) != 0;
  for (int q = 0; q < 4; ++q) { v.cn4[q] = (uint16_t)r[5 + q]; v.ct4[q] = (uint16_t)r[9 + q]; }
  for (int q = 0; q < 2; ++q) { v.rn2[q] = (uint16_t)r[13 + q]; v.rt2[q] = (uint16_t)r[15 + q]; }
  hp_zero(v.ha); hp_zero(v.hr);
  for (int j = 0; j < 3; ++j) { v.ha.nh[j] = (uint16_t)r[17 + j]; v.ha.nq[j] = (uint16_t)r[20 + j]; v.ha.th[j] = (uint16_t)r[23 + j]; v.ha.tq[j] = (uint16_t)r[26 + j]; v.hr.nh[j] = (uint16_t)r[29 + j]; v.hr.th[j] = (uint16_t)r[32 + j]; }
  return v;
}
void put_acc(uint32_t *&o, const Acc &a) { *o++ = a.first; *o++ = a.mn; *o++ = a.mnz; *o++ = a.sum; *o++ = a.sumnz; *o++ = a.nnz; *o++ = a.n; }
}

extern "C" int lancet_emu_transcript_maxts() { return LC_MAXTS; }
extern "C" int lancet_emu_transcript_words() { return 11 + 12 * 7 + 24 + 8 + 12; }

// cols: ncols positions, the listed (non-match) columns in order.  ext: the extension positions of transcript ti are ext_off[ti] .. ext_off[ti + 1].
// out: per transcript its fields, the twelve accumulators, the haplotype fields, cov[8], hp12[12].  Returns the column rule's last status.
extern "C" int lancet_emu_transcript(const int32_t *cols, int ncols, const int32_t *ext, const int32_t *ext_off, const uint8_t *ra, const uint8_t *pa,
                                     uint32_t rrbase, int cap, int lr, uint32_t *out, int *nts_out, int *ovf_out) {
  static WinShared S; memset(&S, 0, sizeof(S));
  static TS ts[LC_MAXTS]; memset(ts, 0xCD, sizeof(ts));
  Ctx c; c.P = nullptr; c.B = nullptr; c.C = nullptr; c.W = nullptr; c.OUT = nullptr; c.S = &S;
  WalkState st = {0, -2, '?'};
  int status = WALK_GO;
  for (int i = 0; i < ncols && status == WALK_GO; ++i) {
    const WalkPos v = pos_of(cols + REC * i);
    status = walk_column(c, ts, st, cap, v, ra, pa, v.pos_in_ref + rrbase, lr != 0);
  }
  *nts_out = st.nts; *ovf_out = S.overflow;
  if (status == WALK_OVF || status == WALK_FULL) return status;
  for (int ti = 0; ti < st.nts; ++ti) {
    TS &t = ts[ti];
    if (t.code != 'x') for (int e = ext_off[ti]; e < ext_off[ti + 1]; ++e) if (!walk_extend(t, pos_of(ext + REC * e), lr != 0)) break;
    uint16_t cov[8], hp12[12];
    ts_record_cov(t, lr != 0, cov, hp12);
    uint32_t *o = out + (size_t)lancet_emu_transcript_words() * ti;
    *o++ = t.pos; *o++ = t.ref_pos; *o++ = t.start_pos; *o++ = t.end_pos; *o++ = t.ref_end_pos; *o++ = (uint32_t)t.col0; *o++ = (uint32_t)t.col1;
    *o++ = (uint8_t)t.code; *o++ = (uint8_t)t.prev_bp_ref; *o++ = (uint8_t)t.prev_bp_alt; *o++ = t.somatic ? 1u : 0u;
    for (int q = 0; q < 4; ++q) put_acc(o, t.aN[q]);
    for (int q = 0; q < 4; ++q) put_acc(o, t.aT[q]);
    for (int q = 0; q < 2; ++q) put_acc(o, t.rN[q]);
    for (int q = 0; q < 2; ++q) put_acc(o, t.rT[q]);
    for (int j = 0; j < 3; ++j) *o++ = t.hrmnN[j];
    for (int j = 0; j < 3; ++j) *o++ = t.hrmnT[j];
    for (int j = 0; j < 3; ++j) *o++ = t.hrsumN[j];
    for (int j = 0; j < 3; ++j) *o++ = t.hrsumT[j];
    for (int j = 0; j < 3; ++j) *o++ = t.hamnN[j];
    for (int j = 0; j < 3; ++j) *o++ = t.hamnT[j];
    for (int j = 0; j < 3; ++j) *o++ = t.haqN[j];
    for (int j = 0; j < 3; ++j) *o++ = t.haqT[j];
    for (int q = 0; q < 8; ++q) *o++ = cov[q];
    for (int q = 0; q < 12; ++q) *o++ = hp12[q];
  }
  return status;
}
