// emu_compress.cc -- TEST INFRASTRUCTURE ONLY (tests/test_compress_emu.py compiles it on its own, once plain and once with -DLANCET_FAT=1;
// the Makefile's libraries do not hold it).
//
// Unitig compression alone, on a hand-made graph: the four drivers of kernels.h that state Graph_t::compressNode / compress / cleanDead
// (reference src/Graph.cc:2486-2762) -- compress (the literal loop), compress_prepare -> compress_fast (record replay), compress_prepare ->
// compress_rank (pointer jumping over ports) and compress_wg (the whole-wave loop; its one-lane form in the FAT build) -- each from the
// same start state, next to a plain model of the reference lines (strings, per-position coverage entries, edge vectors) that shares no
// code with them.  The build kernel's bl_compress_first needs a whole hand-off area and is held where it can be observed: by the counts of
// test_emu_kernels.py, and -- the table it leaves, position by position -- by test_table_order_windows_emu.py, which reads CLIVE back
// (lancet_debug_pre_order) and holds it against the oracle's unordered_map after compress(1).  The build kernel's tail in front of it
// (table order, cleanDead, components) has a rig of its own: emu_table_order.cc for the rules, table_order_cases.py for whole windows.
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

#include "emu_graph_model.h"      // the input record, the work space (Rig) and the plain model of the reference lines

// out: five blocks of 3 + n_rec + n_rec * (24 + len_max) words -- drivers 0 compress, 1 compress_prepare -> compress_fast (its fallbacks included),
// 2 compress_prepare -> compress_rank, 3 compress_wg, 4 the model.  Word 1 of a block (aux): driver 1: compress_prepare's cmp_ok;
// driver 2: 1 ranked, 0 compress_rank declined and left the graph untouched, 2 declined but touched it, 3 not asked (cmp_ok == 0).
extern "C" void lancet_emu_compress(uint32_t n_rec, uint32_t M, const uint32_t *order, const uint32_t *rec, const uint32_t *seq, uint32_t seq_top, uint32_t seq_cap,
                                    const uint16_t *qv, uint32_t qv_rows, int K, uint32_t len_max, uint32_t *out) {
  Input in; in.n_rec = n_rec; in.M = M; in.order = order; in.rec = rec; in.seq = seq; in.seq_top = seq_top; in.seq_cap = seq_cap; in.qv = qv; in.qv_rows = qv_rows; in.K = K; in.len_max = len_max;
  const size_t BW = 3 + (size_t)n_rec + (size_t)n_rec * (OUT_HEAD + len_max);
  const int comp = 1;
  {
    Rig r(in);
    compress(r.c, comp, true);
    r.dump(in, 0, out);
  }
  {
    Rig r(in);
    compress_prepare(r.c, comp);
    const uint32_t ok = (uint32_t)r.S.cmp_ok;
    if (ok) compress_fast(r.c, comp, true); else compress(r.c, comp, true);
    if (r.S.tmp2) compact_absorbed_wg(r.c);
    r.dump(in, ok, out + BW);
  }
  {
    Rig r(in), start(in);
    compress_prepare(r.c, comp);
    uint32_t aux = 3;
    if (r.S.cmp_ok) {
      if (compress_rank(r.c, comp)) { aux = 1; if (r.S.tmp2) compact_absorbed_wg(r.c); }
      else aux = r.same_graph(start) ? 0 : 2;
    }
    r.dump(in, aux, out + 2 * BW);
  }
  {
    Rig r(in);
    compress_wg(r.c, comp);
    r.dump(in, 0, out + 3 * BW);
  }
  {
    Model m = make_model(in);
    m.compress(comp);
    dump_model(in, m, out + 4 * BW);
  }
}
