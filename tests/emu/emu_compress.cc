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

namespace {
// one node record of the input: 28 words
//   0 flags  1 comp  2 necnt  3..14 edges  15..18 cov (float bits)  19 kc Tf|Tr<<16  20 kc Nf|Nr<<16  21 nqv  22 nkm  23 nkmT
//   24 seq_lo  25 seq_hi  26 seq_clo  27 seq_chi
enum { IN_WORDS = 28 };
struct Input {
  uint32_t n_rec, M; const uint32_t *order, *rec; const uint32_t *seq; uint32_t seq_top, seq_cap; const uint16_t *qv; uint32_t qv_rows; int K; uint32_t len_max;
};
// one node record of the output: 24 + len_max words
//   0 flags  1 necnt  2..13 edges  14..17 cov bits  18 mincov  19 mincovqv  20 nkm  21 nkmT  22 length  23 (unused)  24.. descriptors
enum { OUT_HEAD = 24 };

// ---- position data behind a descriptor, in plain words (the model's and the start state's Node_t::computeMinCov operands)
void position_totals(const Input &in, uint32_t d, int *tot, int *totqv) {
  const uint32_t km = d >> 9, off = (d >> 2) & 0x7Fu;
  const uint32_t *r = in.rec + (size_t)IN_WORDS * km;
  *tot = (int)(r[19] & 0xFFFFu) + (int)(r[19] >> 16) + (int)(r[20] & 0xFFFFu) + (int)(r[20] >> 16);
  *totqv = 0;
  if (r[21] != 0xFFFFFFFFu) { const uint16_t *q = in.qv + ((size_t)r[21] * in.K + off) * 4; *totqv = q[0] + q[1] + q[2] + q[3]; }
}

// ---- the drivers of kernels.h on a work space that holds just what they touch
struct Rig {
  lancet_params P; EngineCaps C; Work W; WinShared S; Ctx c;
  std::vector<NodeGr> gr; std::vector<CmpRec> cmp; std::vector<uint32_t> order, seq, todo, mv, scratch, pnodes, pedges; std::vector<uint16_t> qv;
  explicit Rig(const Input &in) : gr(in.n_rec), cmp(in.n_rec), order(in.order, in.order + in.M), seq(in.seq, in.seq + in.seq_cap), todo(in.n_rec + 8), mv(64 * (size_t)in.n_rec + 64),
                                  scratch(8 * (size_t)in.n_rec + 64), pnodes(2 * (size_t)in.n_rec + 8), pedges(2 * (size_t)in.n_rec + 8), qv(in.qv, in.qv + 4 * (size_t)in.qv_rows * in.K) {
    memset(&P, 0, sizeof(P)); memset(&C, 0, sizeof(C)); memset(&W, 0, sizeof(W)); memset(&S, 0, sizeof(S));
    memset(gr.data(), 0, gr.size() * sizeof(NodeGr)); memset(cmp.data(), 0, cmp.size() * sizeof(CmpRec));
    order.resize(in.n_rec + 8);
    for (uint32_t n = 0; n < in.n_rec; ++n) {
      const uint32_t *r = in.rec + (size_t)IN_WORDS * n; NodeGr &g = gr[n];
      g.flags = r[0]; g.comp = (int)r[1]; g.necnt = r[2];
      for (int e = 0; e < LC_EMAX; ++e) g.edges[e] = r[3 + e];
      memcpy(g.cov, r + 15, 16);
      g.kc[0] = (uint16_t)(r[19] & 0xFFFFu); g.kc[1] = (uint16_t)(r[19] >> 16); g.kc[2] = (uint16_t)(r[20] & 0xFFFFu); g.kc[3] = (uint16_t)(r[20] >> 16);
      g.nqv = r[21]; g.nkm = r[22]; g.nkmT = r[23]; g.seq_lo = r[24]; g.seq_hi = r[25]; g.seq_clo = r[26]; g.seq_chi = r[27];
      int mn = 10000000, mq = 10000000;
      for (uint32_t i = g.seq_lo; i < g.seq_hi; ++i) { int t, tq; position_totals(in, in.seq[i], &t, &tq); mn = std::min(mn, t); mq = std::min(mq, tq); }
      g.mincov = g.seq_hi > g.seq_lo ? mn : 0; g.mincovqv = g.seq_hi > g.seq_lo ? mq : 0;
    }
    P.max_tip_len = 11;
    C.node_cap = in.n_rec; C.special_cap = 2; C.seq_cap = in.seq_cap; C.occ_cap = 16 * in.n_rec + 64; C.evt_cap = 0;
    W.gr = gr.data(); W.cmp = cmp.data(); W.order = order.data(); W.seq = seq.data(); W.todo = todo.data(); W.mv = mv.data(); W.scratch = scratch.data();
    W.pnodes = pnodes.data(); W.pedges = pedges.data(); W.qv = qv.data(); W.qv_own = qv.data();
    S.M = in.M; S.K = in.K; S.QS = 4; S.seq_top = in.seq_top; S.ht_elt = in.M; S.reflen = 100; S.totalreadbp = 1000;
    c.P = &P; c.B = nullptr; c.C = &C; c.W = &W; c.OUT = nullptr; c.S = &S;
  }
  // out: overflow, aux, live nodes, the table order [n_rec], then the records
  void dump(const Input &in, uint32_t aux, uint32_t *out) const {
    const size_t RW = OUT_HEAD + in.len_max;
    out[0] = (uint32_t)S.overflow; out[1] = aux; out[2] = S.M;
    for (uint32_t i = 0; i < in.n_rec; ++i) out[3 + i] = i < S.M ? order[i] : 0xFFFFFFFFu;
    uint32_t *o = out + 3 + in.n_rec;
    for (uint32_t n = 0; n < in.n_rec; ++n, o += RW) {
      const NodeGr &g = gr[n];
      o[0] = g.flags; o[1] = g.necnt;
      for (int e = 0; e < LC_EMAX; ++e) o[2 + e] = (uint32_t)e < g.necnt ? g.edges[e] : 0u;
      memcpy(o + 14, g.cov, 16);
      o[18] = (uint32_t)g.mincov; o[19] = (uint32_t)g.mincovqv; o[20] = g.nkm; o[21] = g.nkmT;
      const uint32_t len = g.seq_hi - g.seq_lo;
      o[22] = len; o[23] = 0;
      for (uint32_t i = 0; i < in.len_max; ++i) o[OUT_HEAD + i] = (i < len && !S.overflow) ? seq[g.seq_lo + i] : 0u;
    }
  }
  bool same_graph(const Rig &o) const {                       // node records, table and descriptor arena
    return S.M == o.S.M && S.seq_top == o.S.seq_top && !memcmp(gr.data(), o.gr.data(), gr.size() * sizeof(NodeGr)) &&
           std::equal(order.begin(), order.begin() + S.M, o.order.begin()) && seq == o.seq;
  }
};

// ---- the model: Node_t / Graph_t as the reference has them, reduced to what compression touches
struct MEdge { uint32_t to, dir, flag; };
struct MPos { uint32_t kmer, off; int tot, totqv; };                  // a cov_t entry, and whose it is
struct MNode {
  uint32_t id; bool special = false, dead = false, tumor = false, normal = false; int comp = 0;
  std::string str;                                                    // codes 0..3 as characters
  std::vector<MPos> dist; std::string status;
  float cov[4]; int mincov = 0, mincovqv = 0;
  std::vector<MEdge> edges;
};
bool m_isdir(uint32_t d, char dir) { return dir == 'F' ? (d == 0 || d == 1) : (d == 2 || d == 3); }      // Edge_t::isDir
char m_dest(uint32_t d) { return (d == 0 || d == 2) ? 'F' : 'R'; }                                       // Edge_t::destdir
uint32_t m_flipme(uint32_t d) { switch (d) { case 0: return 2; case 1: return 3; case 2: return 0; default: return 1; } }      // FF<->RF, FR<->RR
uint32_t m_fliplink(uint32_t d) { return d == 0 ? 3u : d == 3 ? 0u : d; }                                // FF<->RR
std::string m_rc(const std::string &s) { std::string r(s.rbegin(), s.rend()); for (auto &ch : r) ch = (char)(3 - ch); return r; }
struct Model {
  int K; std::vector<MNode> nodes; std::vector<uint32_t> order; bool overflow = false;
  int buddy(const MNode &n, char dir) const {                         // Node_t::getBuddy
    int ret = -1;
    if (n.special) return ret;
    for (size_t i = 0; i < n.edges.size(); ++i) if (m_isdir(n.edges[i].dir, dir)) { if (ret != -1) return -1; ret = (int)i; }
    if (ret != -1 && n.edges[ret].to == n.id) return -1;
    return ret;
  }
  static bool tandem(const MNode &n) { for (auto &e : n.edges) if (e.to == n.id) return true; return false; }
  static void min_cov(MNode &n) { int mn = 10000000, mq = 10000000; for (auto &p : n.dist) { mn = std::min(mn, p.tot); mq = std::min(mq, p.totqv); } n.mincov = mn; n.mincovqv = mq; }
  void compress_node(MNode &node, char dir) {                         // Graph_t::compressNode
    while (!overflow) {
      const int uid = buddy(node, dir);
      if (uid == -1) return;
      if (tandem(node)) return;
      const uint32_t edir = node.edges[uid].dir;
      const char bdir = (edir == 0 || edir == 2) ? 'R' : 'F';
      MNode &b = nodes[node.edges[uid].to];
      if (tandem(b)) return;
      const int buid = buddy(b, bdir);
      if (buid == -1) return;
      std::string astr = node.str;
      if (dir == 'R') { astr = m_rc(astr); std::reverse(node.dist.begin(), node.dist.end()); }
      std::string bstr = b.str;
      if (m_dest(edir) == 'R') { bstr = m_rc(bstr); std::reverse(b.dist.begin(), b.dist.end()); }
      std::string mstr = astr + bstr.substr(K - 1);
      if (dir == 'R') mstr = m_rc(mstr);
      node.str = mstr;
      const int amer = (int)astr.length() - K + 1, bmer = (int)bstr.length() - K + 1;
      for (size_t j = K - 1; j < b.dist.size(); ++j) { node.dist.push_back(b.dist[j]); node.status.push_back(b.status[j]); }
      min_cov(node);
      for (int q = 0; q < 4; ++q) { const float nc = node.cov[q], bc = b.cov[q]; node.cov[q] = ((nc * amer) + (bc * bmer)) / (amer + bmer); }
      if (dir == 'R') std::reverse(node.dist.begin(), node.dist.end());
      b.dead = true;
      if (b.normal) node.normal = true;
      if (b.tumor) node.tumor = true;
      node.edges.erase(node.edges.begin() + uid);
      for (int i = 0; i < (int)b.edges.size(); ++i) {
        if (i == buid) continue;
        MEdge ne = b.edges[i];
        if (edir == 1 || edir == 2) ne.dir = m_flipme(ne.dir);
        if (ne.to == b.id) { ne.to = node.id; node.edges.push_back(ne); }
        else {
          node.edges.push_back(ne);
          for (auto &e : nodes[ne.to].edges) if (e.to == b.id && e.dir == m_fliplink(b.edges[i].dir)) { e.to = node.id; e.dir = m_fliplink(ne.dir); break; }      // Node_t::updateEdge
        }
        if (node.edges.size() > (size_t)LC_EMAX) { overflow = true; return; }      // (the work space holds 12 edges per node)
      }
    }
  }
  void compress(int comp) {                                           // Graph_t::compress + cleanDead
    for (size_t i = 0; i < order.size() && !overflow; ++i) {
      MNode &n = nodes[order[i]];
      if (n.comp != comp || n.dead || n.special) continue;
      compress_node(n, 'F');
      compress_node(n, 'R');
    }
    std::vector<uint32_t> live;
    for (uint32_t n : order) if (!nodes[n].dead) live.push_back(n);
    order = live;
  }
};
Model make_model(const Input &in) {
  Model m; m.K = in.K; m.nodes.resize(in.n_rec); m.order.assign(in.order, in.order + in.M);
  for (uint32_t n = 0; n < in.n_rec; ++n) {
    const uint32_t *r = in.rec + (size_t)IN_WORDS * n; MNode &x = m.nodes[n];
    x.id = n; x.special = (r[0] & (NF_SOURCE | NF_SINK)) != 0; x.dead = (r[0] & NF_DEAD) != 0; x.tumor = (r[0] & NF_TUMOR) != 0; x.normal = (r[0] & NF_NORMAL) != 0;
    x.comp = (int)r[1];
    for (uint32_t e = 0; e < r[2]; ++e) x.edges.push_back(MEdge{r[3 + e] & 0x0FFFFFFFu, (r[3 + e] >> 28) & 3u, (r[3 + e] >> 30) & 1u});
    memcpy(x.cov, r + 15, 16);
    for (uint32_t i = r[24]; i < r[25]; ++i) { const uint32_t d = in.seq[i]; MPos p; p.kmer = d >> 9; p.off = (d >> 2) & 0x7Fu; position_totals(in, d, &p.tot, &p.totqv); x.dist.push_back(p); x.str.push_back((char)(d & 3u)); }
    x.status.assign(x.str.size(), 'E');                               // positions K-1 .. : one per constituent k-mer, 'T' for the tumor-only ones
    for (uint32_t j = 0; j < r[22] && (size_t)(in.K - 1) + j < x.status.size(); ++j) x.status[(size_t)(in.K - 1) + j] = j < r[23] ? 'T' : 'N';
    if (!x.dist.empty()) Model::min_cov(x);
  }
  return m;
}
void dump_model(const Input &in, const Model &m, uint32_t *out) {
  const size_t RW = OUT_HEAD + in.len_max;
  out[0] = m.overflow ? 1u : 0u; out[1] = 0; out[2] = (uint32_t)m.order.size();
  for (uint32_t i = 0; i < in.n_rec; ++i) out[3 + i] = i < m.order.size() ? m.order[i] : 0xFFFFFFFFu;
  uint32_t *o = out + 3 + in.n_rec;
  for (uint32_t n = 0; n < in.n_rec; ++n, o += RW) {
    const MNode &x = m.nodes[n];
    o[0] = (in.rec[(size_t)IN_WORDS * n] & ~(uint32_t)(NF_DEAD | NF_TUMOR | NF_NORMAL)) | (x.dead ? NF_DEAD : 0u) | (x.tumor ? NF_TUMOR : 0u) | (x.normal ? NF_NORMAL : 0u);
    o[1] = (uint32_t)x.edges.size();
    for (size_t e = 0; e < (size_t)LC_EMAX; ++e) o[2 + e] = e < x.edges.size() ? (x.edges[e].to | (x.edges[e].dir << 28) | (x.edges[e].flag << 30)) : 0u;
    memcpy(o + 14, x.cov, 16);
    o[18] = (uint32_t)x.mincov; o[19] = (uint32_t)x.mincovqv;
    uint32_t nkm = 0, nkmT = 0;
    for (size_t j = (size_t)(in.K - 1); j < x.status.size(); ++j) { ++nkm; if (x.status[j] == 'T') ++nkmT; }
    o[20] = x.special ? 0u : nkm; o[21] = x.special ? 0u : nkmT; o[22] = (uint32_t)x.str.size(); o[23] = 0;
    for (uint32_t i = 0; i < in.len_max; ++i) o[OUT_HEAD + i] = (i < x.str.size() && !m.overflow) ? ((x.dist[i].kmer << 9) | (x.dist[i].off << 2) | (uint32_t)x.str[i]) : 0u;
  }
}
}  // namespace

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
