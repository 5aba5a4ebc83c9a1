// emu_recovery.cc -- TEST INFRASTRUCTURE ONLY (tests/test_recovery_emu.py compiles it on its own; the Makefile's libraries do not hold it).
//
// The node table right after build_graph, by k-mer: one window goes through the emulated general build (kernels.h build_graph, which
// ends with build_recover when lancet_params::kmer_recovery is set) and stops there (EngineCaps::debug_stop = 6); the caller then asks
// for the float coverages and the cov_t counts of the k-mers it names.  This is how the recovery pass is looked at alone: the same
// table built with the flag off and on, and nothing of the graph passes behind it.
#include "emu_engine.cc"

// kmers: n strings of K characters, back to back.  node_out[i] = node id or -1; cov_out[4 i ..] = Tf Tr Nf Nr (float); kc_out likewise (counts).
// Returns K of the build, or -1 when the window did not reach one.
extern "C" int lancet_emu_table_probe(const lancet_params *P, const lancet_window_batch *b, const char *kmers, int n, int32_t *node_out, float *cov_out,
                                      uint16_t *kc_out) {
  if (b->n_windows != 1) return -1;
  EngineCaps C = lc_caps_for_batch(b, P, 0, 65536);
  C.pl = lc_pre_layout_for_batch(b, 1, (size_t)1 << 40, -1, false);
  C.wide_ids = LC_WIDE_IDS;
  C.debug_stop = 6u;                                                   // (STOP_RET(c, 6) at the end of build_graph)
  const uint32_t R = b->read_begin[1];
  std::vector<uint8_t> ref_codes(b->ref_off[1]);
  for (size_t i = 0; i < ref_codes.size(); ++i) ref_codes[i] = (uint8_t)base_code(b->ref_bases[i]);
  std::vector<uint32_t> rinfo(R), bw(R + 1), gw(R + 1);
  uint32_t bo = 0, go = 0;
  for (uint32_t r = 0; r < R; ++r) { uint32_t len = b->seq_off[r + 1] - b->seq_off[r]; bw[r] = bo; gw[r] = go; bo += (len + 15) / 16; go += (len + 31) / 32; }
  std::vector<uint32_t> bases(bo + 4), good(go + 1);
  for (uint32_t r = 0; r < R; ++r)
    prep_read(P, b->seq, b->qual, b->seq_off[r], (int)(b->seq_off[r + 1] - b->seq_off[r]), b->label[r], b->strand[r], b->mate[r], b->mapped[r],
              &rinfo[r], bases.data(), bw[r], good.data(), gw[r]);
  DevBatch B;
  B.n_windows = 1; B.chr_id = b->chr_id; B.ref_start = b->ref_start; B.ref_off = b->ref_off; B.ref_codes = ref_codes.data();
  B.read_begin = b->read_begin; B.rinfo = rinfo.data(); B.name_rank = b->name_rank; B.base_woff = bw.data(); B.good_woff = gw.data();
  B.bases = bases.data(); B.good = good.data(); B.bx_rank = nullptr; B.hp = nullptr;
  size_t wbytes = lc_work_carve(nullptr, nullptr, C);
  std::vector<char> wmem(wbytes + 256, (char)0xCD);
  Work work; lc_work_carve(&work, wmem.data(), C);
  std::vector<lancet_variant> variants(C.var_cap); std::vector<char> blob(C.blob_cap); std::vector<lancet_window_stats> stats(1);
  std::vector<lancet_variant_lr> lr(C.var_cap); std::vector<uint32_t> bxb(C.bx_cap + 1), evl(1, 0), ev(1, 0);
  uint32_t nv = 0, nb = 0, qh = 0, nx = 0, nau = 0;
  DevOut O; memset(&O, 0, sizeof(O));
  O.variants = variants.data(); O.blob = blob.data(); O.n_variants = &nv; O.n_blob = &nb; O.stats = stats.data();
  O.variants_lr = lr.data(); O.bx_blob = bxb.data(); O.n_bx = &nx; O.queue_head = &qh; O.evt_len = evl.data(); O.evt_out = ev.data(); O.n_ahead_used = &nau;
  static thread_local WinShared S;
  memset(&S, 0xCD, sizeof(S));
  window_kernel_body(P, &B, &C, &work, &O, &S, 0);
  const int K = S.K;
  if (K < 3 || K > 127) return -1;
  Ctx c; c.P = P; c.B = &B; c.C = &C; c.W = &work; c.OUT = &O; c.S = &S;
  for (int i = 0; i < n; ++i) {
    uint8_t codes[128];
    for (int j = 0; j < K; ++j) codes[j] = (uint8_t)base_code(kmers[(size_t)i * K + j]);
    const uint32_t node = kmer_lookup(c, codes, nullptr);
    node_out[i] = node == LC_NIL ? -1 : (int32_t)node;
    for (int q = 0; q < 4; ++q) { cov_out[4 * i + q] = node == LC_NIL ? 0.0f : work.gr[node].cov[q]; kc_out[4 * i + q] = node == LC_NIL ? (uint16_t)0 : work.gr[node].kc[q]; }
  }
  return K;
}
