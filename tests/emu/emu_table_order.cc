// emu_table_order.cc -- TEST INFRASTRUCTURE ONLY (tests/test_table_order_emu.py compiles it on its own, once plain and once with
// -DLANCET_FAT=1; the Makefile's libraries do not hold it).
//
// The node table's iteration order and the numbering of the components alone, on made-up 64-bit hashes: the drivers of kernels.h that
// state libstdc++'s _M_insert_bucket_begin / _M_rehash_aux / _Prime_rehash_policy and Graph_t::cleanDead / markConnectedComponents
// (reference src/Graph.cc:2252-2336, 2737-2762) -- ht_insert (the sequential replay), first_lowcov -> order_stage (the closed form per
// growth stage), clean_dead_wg in its flags and its survb form, mark_connected_components_wg, order_insert, clean_dead -- run one script,
// next to a model that shares no code with them: a real std::unordered_map whose hasher returns the made-up hash of its key, driven by
// the same script.  The model's own iteration is the order, its bucket_count() the bucket count; its components are the reference's
// breadth-first walk over that iteration.
//
// The script (a stage is what the output holds a block for):
//   0  insert ids 0 .. N-1                          rig A: ht_insert one by one ; rig B: first_lowcov
//   1  erase the non-survivors                      rig A: clean_dead_wg reading the node flags ; rig B: clean_dead_wg reading survb
//   2  markConnectedComponents                      (the order is unchanged; comp per node, numcomp, refcomp)
//   3  insert nodes N, N+1                          order_insert (markRefEnds' source and sink)
//   4  erase a given set of nodes 0 .. N+1          clean_dead
//   5  insert nodes N+2, N+3                        order_insert (the second component's special nodes)
// With -DTABLE_ORDER_MAIN the file is a stand-alone program that runs the script on cases of its own (for a sanitizer build).
#define LANCET_WAVE_EMU 1
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <set>
#include <unordered_map>
#include <vector>
#ifndef LANCET_EMU_KERNELS_H
#define LANCET_EMU_KERNELS_H "../../lancet_amd/csrc/kernels.h"
#endif
#include LANCET_EMU_KERNELS_H

namespace {
enum { TO_STAGES = 6, TO_HEAD = 5, TO_SPECIAL = 4, TO_EMAX = 8 };
struct Input {
  uint32_t N; const unsigned long long *nhash;      // [N + 4]
  const uint8_t *surv, *touch;                      // [N]
  const uint32_t *necnt, *edges;                    // [N], [N * 8]: neighbours (survivors only)
  const uint8_t *erase2;                            // [N + 2]
};
size_t block_words(uint32_t N) { return (size_t)TO_STAGES * (TO_HEAD + N + TO_SPECIAL) + 2 + N; }
// a block: per stage M, bucket count, next resize, elements, overflow, order[N + 4] (LC_NIL behind M); then numcomp, refcomp, comp[N] (0: erased)
struct Block {
  uint32_t N; uint32_t *out;
  void stage(int s, uint32_t M, uint32_t bc, uint32_t nr, uint32_t elt, uint32_t ovf, const uint32_t *order) {
    uint32_t *o = out + (size_t)s * (TO_HEAD + N + TO_SPECIAL);
    o[0] = M; o[1] = bc; o[2] = nr; o[3] = elt; o[4] = ovf;
    for (uint32_t i = 0; i < N + TO_SPECIAL; ++i) o[TO_HEAD + i] = i < M ? order[i] : 0xFFFFFFFFu;
  }
  uint32_t *comps() { return out + (size_t)TO_STAGES * (TO_HEAD + N + TO_SPECIAL); }
};

// ---- the drivers of kernels.h on a work space that holds just what they touch
struct Rig {
  lancet_params P; EngineCaps C; Work W; WinShared S; Ctx c;
  std::vector<NodeGr> gr; std::vector<unsigned long long> nhash;
  std::vector<uint32_t> ht_next, ht_bucket, ht_cnt, ht_start, order, scratch, pnodes, pedges, nfill, mv; std::vector<uint8_t> survb;
  explicit Rig(const Input &in) {
    const uint32_t N = in.N, nodes = N + TO_SPECIAL, BC = 42043u;
    memset(&P, 0, sizeof(P)); memset(&C, 0, sizeof(C)); memset(&W, 0, sizeof(W)); memset(&S, 0, sizeof(S));
    gr.resize(nodes); memset(gr.data(), 0, gr.size() * sizeof(NodeGr));
    nhash.assign(in.nhash, in.nhash + nodes);
    ht_next.assign(nodes + 8, 0); ht_bucket.assign(BC, 0); ht_cnt.assign(BC, 0); ht_start.assign(BC, 0);
    order.assign(nodes + 8, 0); scratch.assign(2 * (size_t)nodes + 16, 0); pnodes.assign(nodes + 8, 0); pedges.assign(nodes + 8, 0);
    nfill.assign(nodes + 8, 0); mv.assign(4 * (size_t)nodes + 16, 0); survb.assign(nodes, 0);
    for (uint32_t n = 0; n < N; ++n) {
      NodeGr &g = gr[n];
      g.flags = (in.surv[n] ? NF_SURV : 0u) | (in.touch[n] ? NF_INMER : 0u);
      survb[n] = in.surv[n];
      g.necnt = in.surv[n] ? in.necnt[n] : 0u;
      for (uint32_t e = 0; e < g.necnt; ++e) g.edges[e] = ED_MAKE(in.edges[(size_t)TO_EMAX * n + e], 0u);
    }
    C.node_cap = N; C.special_cap = TO_SPECIAL; C.bucket_cap = BC; C.evt_cap = 0;
    W.gr = gr.data(); W.nhash = nhash.data(); W.ht_next = ht_next.data(); W.ht_bucket = ht_bucket.data(); W.ht_cnt = ht_cnt.data(); W.ht_start = ht_start.data();
    W.order = order.data(); W.scratch = scratch.data(); W.pnodes = pnodes.data(); W.pedges = pedges.data(); W.nfill = nfill.data(); W.mv = mv.data(); W.survb = survb.data();
    S.N = N;
    c.P = &P; c.B = nullptr; c.C = &C; c.W = &W; c.OUT = nullptr; c.S = &S;
  }
  void stage(Block &b, int s) { b.stage(s, S.M, S.ht_bc, S.ht_next_resize, S.ht_elt, (uint32_t)S.overflow, order.data()); }
  void run(const Input &in, bool closed_form, Block b) {
    const uint32_t N = in.N;
    if (closed_form) first_lowcov(c);
    else {
      ht_reset(c);
      for (uint32_t n = 0; n < N && !S.overflow; ++n) ht_insert(c, n);
      uint32_t m = 0;
      for (uint32_t p = S.ht_head; p != LC_NIL; p = W.ht_next[p]) W.order[m++] = p;
      S.M = m;
    }
    stage(b, 0);
    S.prebuilt = closed_form ? 1 : 0;
    if (closed_form) for (uint32_t n = 0; n < N; ++n) gr[n].flags &= ~(uint32_t)NF_SURV;       // (the survb form never reads the records' flags: they are stale there)
    clean_dead_wg(c);
    if (closed_form) for (uint32_t n = 0; n < N; ++n) if (survb[n]) gr[n].flags |= NF_SURV;
    stage(b, 1);
    mark_connected_components_wg(c);
    stage(b, 2);
    uint32_t *cp = b.comps();
    cp[0] = (uint32_t)S.numcomp; cp[1] = (uint32_t)S.refcomp;
    for (uint32_t n = 0; n < N; ++n) cp[2 + n] = in.surv[n] ? (uint32_t)gr[n].comp : 0u;
    order_insert(c, N); order_insert(c, N + 1);
    stage(b, 3);
    for (uint32_t n = 0; n < N + 2; ++n) if (in.erase2[n]) gr[n].flags |= NF_DEAD;
    clean_dead(c, true);
    stage(b, 4);
    order_insert(c, N + 2); order_insert(c, N + 3);
    stage(b, 5);
  }
};

// ---- the model: the reference's container itself
struct Hasher { const unsigned long long *h; size_t operator()(uint32_t k) const { return (size_t)h[k]; } };
}  // namespace
#ifdef __GLIBCXX__
namespace std { template <> struct __is_fast_hash<Hasher> : public std::false_type {}; }     // hash codes cached in the nodes, as for std::string keys
#endif
namespace {
typedef std::unordered_map<uint32_t, int, Hasher> Table;
void model_stage(Block &b, int s, const Table &t) {
  std::vector<uint32_t> order;
  for (Table::const_iterator it = t.begin(); it != t.end(); ++it) order.push_back(it->first);
  // _Prime_rehash_policy keeps _M_next_resize == floor(bucket_count * max_load_factor) from the first insert on (the only observable of it)
  b.stage(s, (uint32_t)t.size(), (uint32_t)t.bucket_count(), (uint32_t)((float)t.bucket_count() * t.max_load_factor()), (uint32_t)t.size(), 0u, order.data());
}
void model_erase(Table &t, const std::set<uint32_t> &dead) {                      // Graph_t::cleanDead: collect, then erase by key
  for (std::set<uint32_t>::const_iterator d = dead.begin(); d != dead.end(); ++d) { Table::iterator it = t.find(*d); if (it != t.end()) t.erase(it); }
}
void model_run(const Input &in, Block b) {
  const uint32_t N = in.N;
  Table t(0, Hasher{in.nhash});
  for (uint32_t n = 0; n < N; ++n) t.insert(std::make_pair(n, 0));
  model_stage(b, 0, t);
  std::set<uint32_t> dead;
  for (Table::iterator it = t.begin(); it != t.end(); ++it) if (!in.surv[it->first]) dead.insert(it->first);
  model_erase(t, dead);
  model_stage(b, 1, t);
  int comp = 0, refcomp = 0;                                                      // Graph_t::markConnectedComponents
  for (Table::iterator it = t.begin(); it != t.end(); ++it) it->second = 0;
  for (Table::iterator it = t.begin(); it != t.end(); ++it) {
    if (it->second != 0) continue;
    ++comp;
    std::deque<uint32_t> Q; Q.push_back(it->first);
    int touches = 0;
    while (!Q.empty()) {
      const uint32_t cur = Q.front(); Q.pop_front();
      int &cc = t.find(cur)->second;
      if (cc == 0) {
        cc = comp;
        if (in.touch[cur]) ++touches;
        for (uint32_t e = 0; e < in.necnt[cur]; ++e) Q.push_back(in.edges[(size_t)TO_EMAX * cur + e]);
      }
    }
    if (touches) ++refcomp;
  }
  model_stage(b, 2, t);
  uint32_t *cp = b.comps();
  cp[0] = (uint32_t)comp; cp[1] = (uint32_t)refcomp;
  for (uint32_t n = 0; n < N; ++n) { Table::iterator it = t.find(n); cp[2 + n] = it == t.end() ? 0u : (uint32_t)it->second; }
  t.insert(std::make_pair(N, 0)); t.insert(std::make_pair(N + 1, 0));
  model_stage(b, 3, t);
  dead.clear();
  for (uint32_t n = 0; n < N + 2; ++n) if (in.erase2[n]) dead.insert(n);
  model_erase(t, dead);
  model_stage(b, 4, t);
  t.insert(std::make_pair(N + 2, 0)); t.insert(std::make_pair(N + 3, 0));
  model_stage(b, 5, t);
}
}  // namespace

// out: three blocks of 6 * (5 + N + 4) + 2 + N words -- rig A (ht_insert, flags form), rig B (first_lowcov, survb form), the model
extern "C" void lancet_emu_table_order(uint32_t N, const unsigned long long *nhash, const uint8_t *surv, const uint8_t *touch, const uint32_t *necnt,
                                       const uint32_t *edges, const uint8_t *erase2, uint32_t *out) {
  Input in; in.N = N; in.nhash = nhash; in.surv = surv; in.touch = touch; in.necnt = necnt; in.edges = edges; in.erase2 = erase2;
  const size_t BW = block_words(N);
  { Rig r(in); r.run(in, false, Block{N, out}); }
  { Rig r(in); r.run(in, true, Block{N, out + BW}); }
  model_run(in, Block{N, out + 2 * BW});
}
extern "C" uint32_t lancet_emu_table_order_words(uint32_t N) { return (uint32_t)block_words(N); }

#ifdef TABLE_ORDER_MAIN
// stand-alone: a few hundred scripts on hashes of a small generator; exit status 1 on the first block that differs from the model's
int main() {
  unsigned long long x = 0x9E3779B97F4A7C15ULL;
  auto rnd = [&x]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  const uint32_t sizes[] = {1, 2, 11, 12, 13, 14, 28, 29, 30, 31, 58, 59, 60, 127, 128, 257, 258, 541, 542, 1109, 1110, 2357, 2358, 4097, 5087, 5088, 10273, 10274, 14337, 20753, 20755};
  int cases = 0;
  for (uint32_t N : sizes) for (int fam = 0; fam < 5; ++fam) for (int sv = 0; sv < 3; ++sv) {
    if (fam == 2 && N > 1200) continue;
    std::vector<unsigned long long> h(N + 4); std::vector<uint8_t> surv(N), touch(N), erase2(N + 2); std::vector<uint32_t> necnt(N, 0), edges((size_t)TO_EMAX * N, 0);
    for (uint32_t n = 0; n < N + 4; ++n) h[n] = fam == 0 ? rnd() : fam == 1 ? n : fam == 2 ? 7ULL : fam == 3 ? ~0ULL - (rnd() & 0xFFFF) : (n & 1 ? 5ULL : 18ULL) + 29ULL * (rnd() % 3);
    if (fam == 4 && N > 1200) for (uint32_t n = 0; n < N + 4; ++n) h[n] = rnd() % 97;
    for (uint32_t n = 0; n < N; ++n) { surv[n] = sv == 0 ? 1 : sv == 1 ? (n & 1) : (rnd() % 20 == 0); touch[n] = rnd() % 7 == 0; }
    if (sv != 0) surv[N / 2] = 1;
    uint32_t prev = 0xFFFFFFFFu;
    for (uint32_t n = 0; n < N; ++n) {                                            // chains of survivors, broken at random
      if (!surv[n]) continue;
      if (prev != 0xFFFFFFFFu && rnd() % 9 != 0) { edges[(size_t)TO_EMAX * n + necnt[n]++] = prev; edges[(size_t)TO_EMAX * prev + necnt[prev]++] = n; }
      prev = n;
    }
    for (uint32_t n = 0; n < N + 2; ++n) erase2[n] = rnd() % 3 == 0;
    const size_t BW = block_words(N);
    std::vector<uint32_t> out(3 * BW);
    lancet_emu_table_order(N, h.data(), surv.data(), touch.data(), necnt.data(), edges.data(), erase2.data(), out.data());
    for (int r = 0; r < 2; ++r) if (!std::equal(out.begin() + r * BW, out.begin() + (r + 1) * BW, out.begin() + 2 * BW)) { printf("N=%u family=%d survivors=%d rig %c differs from the model\n", N, fam, sv, 'A' + r); return 1; }
    ++cases;
  }
  printf("%d scripts, every block equal to the model's\n", cases);
  return 0;
}
#endif
