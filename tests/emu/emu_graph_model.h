// emu_graph_model.h -- TEST INFRASTRUCTURE ONLY: what the rigs that run graph stages of kernels.h on a hand-made graph share
// (emu_compress.cc, emu_clean.cc; each includes kernels.h first: the record types, NF_* and LC_EMAX are its).
//
//   Input      the hand-made graph as the tests pack it (tests/emu_graph.py)
//   Rig        a work space that holds just what the graph stages touch, and the dump of its state
//   Model      Node_t / Graph_t as the reference has them, reduced to what compression and the three cleaning passes touch:
//              compressNode / compress / cleanDead (reference src/Graph.cc:2486-2762) and removeNode / removeLowCov / removeShortLinks /
//              removeTips (src/Graph.cc:2768-2926), over strings, per-position coverage entries and edge vectors.  It shares no code with
//              kernels.h or the oracle.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

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
  std::vector<uint8_t> pseq; std::vector<uint32_t> evt;                // (the cleaning passes: the string of a short link; the counts the passes report)
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

// ---- the model: Node_t / Graph_t as the reference has them, reduced to what compression and the cleaning passes touch
struct MEdge { uint32_t to, dir, flag; };
struct MPos { uint32_t kmer, off; int tot, totqv; };                  // a cov_t entry, and whose it is
struct MNode {
  uint32_t id; bool special = false, dead = false, tumor = false, normal = false; int comp = 0;
  std::string str;                                                    // codes 0..3 as characters
  std::vector<MPos> dist; std::string status;
  float cov[4]; int mincov = 0, mincovqv = 0;
  std::vector<MEdge> edges;
  bool in_str = false;                                                // removeShortLinks: findTandems reports an STR over position K-1 of str (stated by the case)
};
bool m_isdir(uint32_t d, char dir) { return dir == 'F' ? (d == 0 || d == 1) : (d == 2 || d == 3); }      // Edge_t::isDir
char m_dest(uint32_t d) { return (d == 0 || d == 2) ? 'F' : 'R'; }                                       // Edge_t::destdir
uint32_t m_flipme(uint32_t d) { switch (d) { case 0: return 2; case 1: return 3; case 2: return 0; default: return 1; } }      // FF<->RF, FR<->RR
uint32_t m_fliplink(uint32_t d) { return d == 0 ? 3u : d == 3 ? 0u : d; }                                // FF<->RR
std::string m_rc(const std::string &s) { std::string r(s.rbegin(), s.rend()); for (auto &ch : r) ch = (char)(3 - ch); return r; }
struct MCounts { int lowcov = -1, links = -1; std::vector<int> tips; };      // what the passes print: found N ; removed: n per round ; removed links: n
struct Model {
  int K; std::vector<MNode> nodes; std::vector<uint32_t> order; bool overflow = false;
  // the members and settings the cleaning passes read (Graph.hh: int totalreadbp_m, ref_m->rawseq.length(), int / double settings)
  int totalreadbp = 1000; size_t reflen = 100; int LOW_COV_THRESHOLD = 1, MAX_TIP_LEN = 11; double MIN_COV_RATIO = 0.01; size_t path_cap = 1u << 30;
  MCounts counts;
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
  void clean_dead() {                                                 // Graph_t::cleanDead
    std::vector<uint32_t> live;
    for (uint32_t n : order) if (!nodes[n].dead) live.push_back(n);
    order = live;
  }
  void compress(int comp) {                                           // Graph_t::compress + cleanDead
    for (size_t i = 0; i < order.size() && !overflow; ++i) {
      MNode &n = nodes[order[i]];
      if (n.comp != comp || n.dead || n.special) continue;
      compress_node(n, 'F');
      compress_node(n, 'R');
    }
    clean_dead();
  }

  // ---- the cleaning passes.  Each walks the table in table order (nodes_m.begin() .. end()); a node removed during a walk stays in the table,
  // dead, until the cleanDead of the compress that follows -- and is met at most once, so no walk removes a dead node.
  void remove_edge(MNode &n, uint32_t to, uint32_t dir) {            // Node_t::removeEdge: the first edge that matches
    for (size_t i = 0; i < n.edges.size(); ++i) if (n.edges[i].to == to && n.edges[i].dir == dir) { n.edges.erase(n.edges.begin() + i); return; }
  }
  void remove_node(MNode &node) {                                     // Graph_t::removeNode, :2768-2784
    node.dead = true;
    for (size_t i = 0; i < node.edges.size(); ++i) {
      MNode &nn = nodes[node.edges[i].to];
      if (nn.id != node.id) remove_edge(nn, node.id, m_fliplink(node.edges[i].dir));
    }
  }
  void remove_low_cov(int compid) {                                   // Graph_t::removeLowCov(true, compid), :2790-2827
    int lowcovnodes = 0;
    const double avgcov = ((double)totalreadbp) / ((double)reflen);
    for (size_t i = 0; i < order.size(); ++i) {
      MNode &node = nodes[order[i]];
      if (node.comp != compid) continue;
      if (node.special) continue;
      const int mq = node.mincovqv;
      const float tot_tmr = node.cov[0] + node.cov[1], tot_nml = node.cov[2] + node.cov[3];      // float getTotTmrCov() / getTotNmlCov()
      if ((mq <= LOW_COV_THRESHOLD) || (mq <= (MIN_COV_RATIO * avgcov)) || (tot_tmr == 1 && tot_nml == 1)) { ++lowcovnodes; remove_node(node); }
    }
    counts.lowcov = lowcovnodes;
    clean_dead();
    compress(compid);
  }
  void remove_short_links(int compid) {                               // Graph_t::removeShortLinks, :2833-2880
    int links = 0;
    const double avgcov = ((double)totalreadbp) / ((double)reflen);
    const int MAX_LINK_LEN = (int)floor((double)K / 2.0);             // Graph.hh setK
    for (size_t i = 0; i < order.size() && !overflow; ++i) {
      MNode &cur = nodes[order[i]];
      if (cur.comp != compid) continue;
      if (cur.special) continue;
      const int deg = (int)cur.edges.size();
      const int len = (int)cur.str.size() - K + 1;                    // getSize()
      if ((deg >= 2) && (len < MAX_LINK_LEN) && (cur.mincov <= floor(sqrt(avgcov)))) {
        if (cur.str.size() > path_cap) { overflow = true; break; }    // (the work space: the string of a candidate has to fit the path buffer)
        if (!cur.in_str) { remove_node(cur); ++links; }               // findTandems(cur->str_m, .., K-1, LEN, MOTIF); LEN == 0
      }
    }
    counts.links = links;
    if (links && !overflow) compress(compid);
  }
  void remove_tips(int compid) {                                      // Graph_t::removeTips, :2885-2926
    int tips = 0;
    do {
      tips = 0;
      for (size_t i = 0; i < order.size(); ++i) {
        MNode &cur = nodes[order[i]];
        if (cur.comp != compid) continue;
        if (cur.special) continue;
        const int deg = (int)cur.edges.size();
        const int len = (int)cur.str.size() - K + 1;                  // strlen() - K + 1
        if ((deg <= 1) && (len < MAX_TIP_LEN)) { remove_node(cur); ++tips; }
      }
      counts.tips.push_back(tips);
      if (tips) compress(compid);
    } while (tips && !overflow);
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
