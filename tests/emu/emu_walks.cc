// emu_walks.cc -- TEST INFRASTRUCTURE ONLY (tests/test_graph_walks_emu.py compiles it on its own; the Makefile's libraries do not hold it).
//
// The two graph walks of the window kernel alone, on a hand-made cleaned graph: kernels.h cycle_dfs and path_fifo through the view of the
// node records (has_cycle / bfs) and through the view of graph_cache_wg's copy in LDS (has_cycle_cached / bfs_cached), next to a plain
// model of Graph_t::hasCycle / hasCycleRec (reference src/Graph.cc:593-681) and Graph_t::bfs (:1299-1425) that shares no code with them.
#define LANCET_WAVE_EMU 1
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <vector>
#include "../../lancet_amd/csrc/kernels.h"

namespace {
static_assert(sizeof(BfsEntry) == 20, "a queue entry is five words");
const uint32_t PATTERN = 0xCDCDCDCDu;                                   // what a queue entry nobody wrote holds

struct Graph {
  uint32_t n_rec, M; const uint32_t *order, *flags, *necnt, *edges, *len;      // records by node id (edges: 12 words each), the table order
  uint32_t source, sink; int K, reflen, max_indel, dfs_limit; uint32_t tracing, queue_cap;
};

// ---- the walks of kernels.h on a work space that holds just what they touch
struct Rig {
  lancet_params P; EngineCaps C; Work W; WinShared S; Ctx c;
  std::vector<NodeGr> gr; std::vector<uint32_t> order, scratch, evt; std::vector<BfsEntry> queue;
  explicit Rig(const Graph &g) : gr(g.n_rec), order(g.order, g.order + g.M), scratch(2 * (g.n_rec + 2)), evt(64), queue(g.queue_cap) {
    memset(&P, 0, sizeof(P)); memset(&C, 0, sizeof(C)); memset(&W, 0, sizeof(W)); memset(&S, 0, sizeof(S));
    memset(gr.data(), 0, gr.size() * sizeof(NodeGr)); memset(queue.data(), 0xCD, queue.size() * sizeof(BfsEntry));
    for (uint32_t n = 0; n < g.n_rec; ++n) {
      gr[n].flags = g.flags[n]; gr[n].necnt = g.necnt[n]; gr[n].seq_lo = 100; gr[n].seq_hi = 100 + g.len[n];
      for (int e = 0; e < LC_EMAX; ++e) gr[n].edges[e] = g.edges[LC_EMAX * n + e];
    }
    P.dfs_limit = g.dfs_limit; P.max_indel_len = g.max_indel;
    C.node_cap = g.n_rec; C.special_cap = 2; C.queue_cap = g.queue_cap; C.evt_cap = g.tracing ? (uint32_t)evt.size() : 0u;
    W.gr = gr.data(); W.order = order.data(); W.scratch = scratch.data(); W.queue = queue.data(); W.evt = evt.data();
    S.M = g.M; S.source = g.source; S.sink = g.sink; S.K = g.K; S.seq_len = g.reflen;
    c.P = &P; c.B = nullptr; c.C = &C; c.W = &W; c.OUT = nullptr; c.S = &S;
  }
};

// ---- the model: recursion and a deque of whole paths, as the reference has them
enum { WHITE = 1, GREY = 2, BLACK = 3 };
bool is_special(const Graph &g, uint32_t n) { return (g.flags[n] & (NF_SOURCE | NF_SINK)) != 0; }
bool edge_is_dir(uint32_t d, char dir) { return dir == 'F' ? (d == 0 || d == 1) : (d == 2 || d == 3); }      // Edge_t::isDir: FF FR leave forwards, RF RR backwards
char edge_destdir(uint32_t d) { return (d == 0 || d == 2) ? 'F' : 'R'; }                                     // Edge_t::destdir: FF RF arrive forwards
struct CycleModel {
  const Graph &g; std::vector<uint32_t> color, at_hit; bool hit = false;
  void rec(uint32_t node, char dir, bool *ans) {                                          // hasCycleRec
    if (*ans) return;
    color[node] = GREY;
    for (uint32_t i = 0; i < g.necnt[node]; ++i) {
      const uint32_t e = g.edges[LC_EMAX * node + i];
      if (!edge_is_dir((e >> 28) & 3u, dir)) continue;
      const uint32_t other = e & 0x0FFFFFFFu;
      if (is_special(g, other)) continue;
      if (color[other] == GREY) { *ans = true; if (!hit) { hit = true; at_hit = color; } break; }
      if (color[other] == WHITE) rec(other, edge_destdir((e >> 28) & 3u), ans);
    }
    color[node] = BLACK;
  }
  bool run() {                                                                            // hasCycle
    color.assign(g.n_rec, 0);
    if (g.source == LC_NIL || g.sink == LC_NIL) return false;
    for (uint32_t i = 0; i < g.M; ++i) if (!is_special(g, g.order[i])) color[g.order[i]] = WHITE;
    bool ans1 = false, ans2 = false;
    rec(g.source, 'F', &ans1);
    rec(g.source, 'R', &ans2);
    return ans1 || ans2;
  }
  // the colours when the first cycle was met (the kernels stop there: what the reference does afterwards changes no answer), else at the end
  const std::vector<uint32_t> &colors() const { return hit ? at_hit : color; }
};
struct PathModel { std::vector<uint32_t> nodes; char dir; int len, flag, score, has_cycle; uint32_t entry; };
// returns the best path's queue entry (LC_NIL: none); q[0 .. *nq) are the paths in the order they were pushed, *limit = DFS_LIMIT was hit
uint32_t bfs_model(const Graph &g, std::vector<BfsEntry> &q, uint32_t *nq, int *limit) {
  std::deque<PathModel> Q;
  auto note = [&](const PathModel &p, uint32_t parent, uint32_t edge) {
    BfsEntry &e = q[p.entry];
    e.parent = parent; e.node = p.nodes.back(); e.edge = edge; e.len = p.len; e.score = (uint16_t)p.score; e.dir = (uint8_t)p.dir; e.bits = (uint8_t)(p.flag | (p.has_cycle << 1));
  };
  uint32_t pushed = 0, best = LC_NIL; int best_score = 0, complete = 0, visit = 0;
  *limit = 0;
  PathModel root; root.nodes.push_back(g.source); root.dir = 'F'; root.len = g.K; root.flag = 1; root.score = 0; root.has_cycle = 0; root.entry = pushed++;
  note(root, LC_NIL, LC_NIL);
  Q.push_back(root);
  while (!Q.empty()) {
    ++visit;
    if (g.dfs_limit && visit > g.dfs_limit) { *limit = 1; break; }
    PathModel path = Q.front(); Q.pop_front();
    const uint32_t cur = path.nodes.back();
    if (cur == g.sink && path.flag == 0) {
      ++complete;
      if (best == LC_NIL) { best = path.entry; best_score = path.score; }
      else if (path.score > best_score) { best = path.entry; best_score = path.score; }
    } else if (path.len > g.reflen + g.max_indel) {
    } else {
      for (uint32_t i = 0; i < g.necnt[cur]; ++i) {
        const uint32_t e = g.edges[LC_EMAX * cur + i], d = (e >> 28) & 3u, eflag = (e >> 30) & 1u;
        if (!edge_is_dir(d, path.dir)) continue;
        const uint32_t other = e & 0x0FFFFFFFu;
        if (!path.has_cycle) for (uint32_t x : path.nodes) if (x == other) { path.has_cycle = 1; q[path.entry].bits |= 2; break; }      // Path_t::hasCycle
        PathModel np = path;
        np.nodes.push_back(other); np.dir = edge_destdir(d);
        np.len = path.len + (is_special(g, other) ? 0 : (int)g.len[other]) - g.K + 1;
        np.flag = path.flag * (int)eflag;
        if (eflag == 0) np.score = path.score + 1;
        np.entry = pushed++;
        if (np.entry >= q.size()) { *nq = pushed - 1; return LC_NIL; }
        note(np, path.entry, (cur << 4) | i);
        Q.push_back(np);
      }
    }
  }
  *nq = pushed;
  return complete ? best : LC_NIL;
}
}  // namespace

// Views 0 / 1 / 2 = node records in HBM / graph_cache_wg's copy / the model.  Per view v:
//   cyc[v]            hasCycle's answer (the cache view: -1 when graph_cache_wg declined)
//   col[v * M + i]    colour of the node at table position i afterwards
//   bfs[3 v ..]       best path's queue entry, the DFS_LIMIT flag, the overflow flag
//   queue[v * 5 * queue_cap ..]   the queue, five words per entry; entries nobody wrote hold 0xCDCDCDCD
// Returns 1 when graph_cache_wg took the graph.
extern "C" int lancet_emu_walks(uint32_t n_rec, uint32_t M, const uint32_t *order, const uint32_t *flags, const uint32_t *necnt, const uint32_t *edges, const uint32_t *len,
                                uint32_t source, uint32_t sink, int K, int reflen, int max_indel, int dfs_limit, uint32_t tracing, uint32_t queue_cap,
                                int32_t *cyc, uint32_t *col, uint32_t *bfs_out, uint32_t *queue) {
  Graph g; g.n_rec = n_rec; g.M = M; g.order = order; g.flags = flags; g.necnt = necnt; g.edges = edges; g.len = len;
  g.source = source; g.sink = sink; g.K = K; g.reflen = reflen; g.max_indel = max_indel; g.dfs_limit = dfs_limit; g.tracing = tracing; g.queue_cap = queue_cap;
  const size_t qwords = 5 * (size_t)queue_cap;
  int cached;
  {
    Rig r(g);
    cyc[0] = has_cycle(r.c) ? 1 : 0;
    for (uint32_t i = 0; i < M; ++i) col[i] = r.gr[order[i]].color;
  }
  {
    Rig r(g);
    const uint32_t best = bfs(r.c);
    bfs_out[0] = best; bfs_out[1] = (uint32_t)r.S.bfs_dfs; bfs_out[2] = (uint32_t)r.S.overflow;
    memcpy(queue, r.queue.data(), 4 * qwords);
  }
  {
    Rig r(g);
    cached = graph_cache_wg(r.c) ? 1 : 0;
    cyc[1] = cached ? (has_cycle_cached(r.c) ? 1 : 0) : -1;
    for (uint32_t i = 0; i < M; ++i) col[M + i] = cached ? (uint32_t)r.S.lbytes[GC_OFF_COL + i] : 0u;
  }
  {
    Rig r(g);
    uint32_t best = LC_NIL;
    if (graph_cache_wg(r.c)) best = bfs_cached(r.c);
    bfs_out[3] = best; bfs_out[4] = (uint32_t)r.S.bfs_dfs; bfs_out[5] = (uint32_t)r.S.overflow;
    memcpy(queue + qwords, r.queue.data(), 4 * qwords);
  }
  {
    CycleModel m{g};
    cyc[2] = m.run() ? 1 : 0;
    for (uint32_t i = 0; i < M; ++i) col[2 * M + i] = m.colors()[order[i]];
    std::vector<BfsEntry> q(queue_cap);
    memset(q.data(), 0xCD, q.size() * sizeof(BfsEntry));
    uint32_t nq = 0; int limit = 0;
    bfs_out[6] = bfs_model(g, q, &nq, &limit); bfs_out[7] = (uint32_t)limit; bfs_out[8] = nq;
    memcpy(queue + 2 * qwords, q.data(), 4 * qwords);
    (void)PATTERN;
  }
  return cached;
}
