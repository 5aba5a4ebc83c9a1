// evid_asan.cc -- TEST INFRASTRUCTURE ONLY.  A stand-alone program for the address / undefined-behaviour sanitizers (`make asan`): the
// emulated evidence kernel (lancet_amd/csrc/hap_evidence.h under LANCET_WAVE_EMU) and the host side behind it (lc_evid_collect with
// lc_evid_join, host_common.h) over hand-written buffers allocated to their exact sizes, so that a word read or written past an end is
// seen: groups at and one beyond the entry list and the event list, paths on both sides of the staging pool's end, reads hanging over
// either end of a path, 1 / 4 / 5 reads, a truncated length word, one record fewer than the window has events.  Every count is held to
// a plain loop over the strings.  Nothing is loaded into Python.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../lancet_amd/csrc/host_common.h"
#include "../../lancet_amd/csrc/hap_evidence.h"

static std::string rnd(uint32_t &s, int n) { std::string r; for (int i = 0; i < n; ++i) { s = s * 1664525u + 1013904223u; r += "ACGT"[(s >> 24) & 3u]; } return r; }
static void pack(const std::string &s, std::vector<uint32_t> *out) {
  const size_t at = out->size(); out->resize(at + (s.size() + 15) / 16, 0u);
  for (size_t i = 0; i < s.size(); ++i) (*out)[at + i / 16] |= (uint32_t)(std::string("ACGT").find(s[i])) << (2 * (i % 16));
}
static char other(char c) { return c == 'A' ? 'C' : c == 'C' ? 'G' : c == 'G' ? 'T' : 'A'; }
struct Op { uint32_t n; char op; };
struct Ent { std::string s; int k, comp; std::vector<Op> cig; };
struct Evt { int rb, rs, pb, ps; };
// an entry: ref with substitutions at `at` (ascending, apart), an insertion of `ins` bases in front of ref[ipos] and a deletion of del bases at dpos (both behind the substitutions)
static Ent make(const std::string &ref, int k, int comp, std::vector<int> at, int ipos = -1, int ins = 0, int dpos = -1, int del = 0) {
  Ent e; e.k = k; e.comp = comp;
  std::string cols;
  for (int i = 0; i < (int)ref.size(); ++i) {
    if (i == ipos) { e.s += std::string((size_t)ins, other(ref[(size_t)i])); cols += std::string((size_t)ins, 'I'); }
    if (dpos >= 0 && i >= dpos && i < dpos + del) { cols += 'D'; continue; }
    bool x = false; for (int a : at) x = x || a == i;
    e.s += x ? other(ref[(size_t)i]) : ref[(size_t)i]; cols += x ? 'X' : '=';
  }
  for (char c : cols) { if (!e.cig.empty() && e.cig.back().op == c) ++e.cig.back().n; else e.cig.push_back(Op{1u, c}); }
  return e;
}
// the definition, in plain loops
static std::vector<Evt> events(const Ent &e) {
  std::vector<Evt> out; int rb = 0, pb = 0; bool open = false;
  for (const Op &o : e.cig) {
    if (o.op == '=') open = false;
    else { if (!open) { out.push_back(Evt{rb, 0, pb, 0}); open = true; } if (o.op != 'I') out.back().rs += (int)o.n; if (o.op != 'D') out.back().ps += (int)o.n; }
    if (o.op != 'I') rb += (int)o.n;
    if (o.op != 'D') pb += (int)o.n;
  }
  return out;
}
static bool place(const std::string &r, const Ent &e, int *d, int *o0) {
  const int t = (int)r.size(), M = (int)e.s.size(); *d = -1;
  for (int o = -t; o <= M; ++o) {
    const int lo = o < 0 ? -o : 0, hi = t < M - o ? t : M - o;
    if (hi - lo < e.k) continue;
    int mm = 0; for (int i = lo; i < hi; ++i) mm += r[(size_t)i] != e.s[(size_t)(o + i)];
    if (*d < 0 || mm < *d) { *d = mm; *o0 = o; }
  }
  return *d >= 0;
}
static int stand(const Evt &e, const std::string &bases, const Ent &h2, int *left, int *right) {
  int lo = e.rb, hi = e.rb + e.rs, shift = 0, tsum = 0, nt = 0; bool same = false;
  for (const Evt &x : events(h2)) {
    if (x.rb <= e.rb + e.rs && x.rb + x.rs >= e.rb) { ++nt; lo = x.rb < lo ? x.rb : lo; hi = x.rb + x.rs > hi ? x.rb + x.rs : hi; tsum += x.ps - x.rs;
      same = x.rb == e.rb && x.rs == e.rs && x.ps == e.ps && h2.s.substr((size_t)x.pb, (size_t)x.ps) == bases; }
  }
  for (const Evt &x : events(h2)) if (!(x.rb <= e.rb + e.rs && x.rb + x.rs >= e.rb) && x.rb + x.rs <= lo) shift += x.ps - x.rs;
  *left = lo + shift; *right = hi + shift + tsum;
  return nt == 0 ? 0 : (nt == 1 && same ? 1 : 2);      // ref, alt, other
}
struct Want { uint32_t idx; Evt e; uint32_t flags; uint32_t c[12]; };
static std::vector<Want> model(const std::vector<Ent> &es, const std::vector<std::string> &reads, int max_mm) {
  std::vector<Want> out;
  for (size_t g0 = 0; g0 < es.size();) {
    size_t g1 = g0; while (g1 < es.size() && es[g1].k == es[g0].k && es[g1].comp == es[g0].comp) ++g1;
    const size_t first = out.size();
    for (size_t i = g0; i < g1; ++i) for (const Evt &e : events(es[i])) out.push_back(Want{(uint32_t)i, e, 0u, {0}});
    if (g1 - g0 > LC_EV_ENTS || out.size() - first > LC_EV_EVENTS) for (size_t q = first; q < out.size(); ++q) out[q].flags = LANCET_EVID_UNEVALUATED;
    else for (const std::string &r : reads) {
      std::vector<int> d(g1 - g0), o(g1 - g0); int best = -1;
      for (size_t i = g0; i < g1; ++i) if (place(r, es[i], &d[i - g0], &o[i - g0]) && (best < 0 || d[i - g0] < best)) best = d[i - g0];
      if (best < 0 || best > max_mm) continue;
      for (size_t q = first; q < out.size(); ++q) {
        int on = 0;
        for (size_t i = g0; i < g1; ++i) if (d[i - g0] == best) {
          int left, right; const Ent &own = es[out[q].idx];
          const int cls = stand(out[q].e, own.s.substr((size_t)out[q].e.pb, (size_t)out[q].e.ps), es[i], &left, &right);
          if (left >= 1 && right + 1 <= (int)es[i].s.size() && o[i - g0] <= left - 1 && o[i - g0] + (int)r.size() >= right + 1) on |= 1 << cls;
        }
        if (on) ++out[q].c[on == 2 ? 0 : on == 1 ? 4 : 8];      // class Tf: the reads here are tumour, forward
      }
    }
    g0 = g1;
  }
  return out;
}
static int failures = 0;
static void run(const char *what, const std::vector<Ent> &es, const std::vector<std::string> &reads, int max_mm, uint32_t trunc_after = 0, uint32_t short_by = 0) {
  std::vector<uint32_t> buf;
  uint32_t len_word = 0, n = 0;
  for (const Ent &e : es) {
    uint32_t ref_len = 0; for (const Op &o : e.cig) if (o.op != 'I') ref_len += o.n;
    const uint32_t hdr[HP_HDR] = {(uint32_t)e.k | (uint32_t)e.comp << 16, 0u, ref_len, (uint32_t)e.s.size(), 0u, 0u, 0u, (uint32_t)e.cig.size()};
    buf.insert(buf.end(), hdr, hdr + HP_HDR); pack(e.s, &buf);
    for (const Op &o : e.cig) buf.push_back(o.n << 4 | (o.op == '=' ? HP_OP_EQ : o.op == 'X' ? HP_OP_X : o.op == 'I' ? HP_OP_I : HP_OP_D));
    if (trunc_after && ++n == trunc_after) len_word = (uint32_t)buf.size() | HP_TRUNC;
  }
  if (!trunc_after) len_word = (uint32_t)buf.size();
  std::vector<uint32_t> heap_buf(buf);                                   // exact size: the sanitizer sees a word past the end
  std::vector<uint32_t> ri, bw, bases;
  for (const std::string &r : reads) { ri.push_back((uint32_t)r.size()); bw.push_back((uint32_t)bases.size()); pack(r, &bases); }
  const uint32_t rb[2] = {0u, (uint32_t)reads.size()};
  DevBatch B; memset(&B, 0, sizeof(B));
  B.n_windows = 1; B.read_begin = rb; B.rinfo = ri.data(); B.base_woff = bw.data(); B.bases = bases.data();
  const std::vector<Ent> whole(es.begin(), trunc_after ? es.begin() + trunc_after : es.end());
  const std::vector<Want> want = model(whole, reads, max_mm);
  const uint32_t cap = (uint32_t)want.size() > short_by ? (uint32_t)want.size() - short_by : 0u;
  std::vector<uint32_t> rec((size_t)cap * EV_WORDS, 0u), ev_len(1, 0u);     // exact sizes again
  static EvShared S;
  memset(&S, 0xCD, sizeof(S));
  hap_evidence_window(&B, &len_word, heap_buf.data(), (uint32_t)heap_buf.size(), (uint32_t)max_mm, rec.data(), ev_len.data(), cap, 0, &S);
  lancet_window_stats st; memset(&st, 0, sizeof(st));
  const uint32_t used = lc_hap_used(len_word, (uint32_t)heap_buf.size(), 0), hoff[2] = {0u, used};
  std::vector<uint32_t> dense(heap_buf.begin(), heap_buf.begin() + used); dense.push_back(0u);
  LcHapResult hr; lc_hap_collect(1, &len_word, hoff, dense.data(), &st, &hr);
  const uint32_t kept = lc_evid_used(ev_len[0], cap, 0), eoff[2] = {0u, kept};
  // a record per event, as if every event had emitted one at its own place: the join finds each its own
  std::vector<lancet_variant> vs; const int32_t ref_start = 1000;
  for (const Want &w : want) { lancet_variant v; memset(&v, 0, sizeof(v)); v.window = 0; v.seq_in_window = (int32_t)vs.size(); v.pos = ref_start + w.e.rb - 1; vs.push_back(v); }
  for (lancet_haplotype &h : hr.h) { h.first_variant = 0; h.n_variants = 0; }
  { size_t q = 0; for (lancet_haplotype &h : hr.h) { h.first_variant = (int32_t)q; while (q < want.size() && want[q].idx == (uint32_t)h.index_in_window) ++q; h.n_variants = (int32_t)q - h.first_variant; } }
  LcEvidResult out;
  std::vector<uint32_t> rec1(rec); rec1.push_back(0u);
  lc_evid_collect(1, ev_len.data(), eoff, rec1.data(), cap, &st, &ref_start, hr.h, vs.data(), vs.size(), &out);
  if (ev_len[0] != want.size() || out.ev.size() != kept || out.marked[0] != (want.size() > cap ? 1 : 0) || out.event_off.size() != hr.h.size() + 1 || hr.h.size() != whole.size()) {
    printf("FAIL %s: %u events of %zu, %zu records of %u, %zu entries of %zu\n", what, ev_len[0], want.size(), out.ev.size(), kept, hr.h.size(), whole.size()); ++failures;
  }
  for (size_t q = 0; q < out.ev.size() && q < want.size(); ++q) {
    const lancet_variant_evidence &g = out.ev[q]; const Want &w = want[q];
    bool ok = g.haplotype == (int32_t)w.idx && (int)g.rb == w.e.rb && (int)g.rs == w.e.rs && (int)g.pb == w.e.pb && (int)g.ps == w.e.ps && g.flags == w.flags && g.variant == (int32_t)q;
    for (int c = 0; c < 4; ++c) ok = ok && g.alt[c] == w.c[c] && g.ref[c] == w.c[4 + c] && g.other[c] == w.c[8 + c];
    if (!ok) { printf("FAIL %s event %zu: got entry %d rb %u flags %u variant %d alt %u ref %u other %u, want entry %u rb %d flags %u alt %u ref %u other %u\n", what, q, g.haplotype, g.rb, g.flags, g.variant,
                      g.alt[0], g.ref[0], g.other[0], w.idx, w.e.rb, w.flags, w.c[0], w.c[4], w.c[8]); ++failures; }
  }
  printf("%s: %zu entries, %zu events, %zu reads\n", what, es.size(), want.size(), reads.size());
}

int main() {
  uint32_t s = 4711u;
  const std::string ref = rnd(s, 200);
  auto tiles = [&](const Ent &e, int lo, int hi) { std::vector<std::string> r; for (int a = lo; a <= hi; a += 6) r.push_back(e.s.substr((size_t)a, 45)); return r; };
  {   // one site, ALT / REF / OTHER carriers; an insertion and a deletion beside a substitution; reads over either end
    const std::vector<Ent> es = {make(ref, 15, 0, {}), make(ref, 15, 0, {60}), make(ref, 15, 0, {60, 62}), make(ref, 15, 0, {100}, 101, 3), make(ref, 15, 0, {100}, -1, 0, 101, 4)};
    std::vector<std::string> rs;
    for (const Ent &e : es) { const auto t = tiles(e, 20, 90); rs.insert(rs.end(), t.begin(), t.end()); }
    rs.push_back(rnd(s, 20) + ref.substr(0, 20)); rs.push_back(ref.substr(180) + rnd(s, 25)); rs.push_back(rnd(s, 40));
    run("carriers", es, rs, 5);
    run("carriers, one record short", es, rs, 5, 0, 1);
    run("carriers, no record", es, rs, 5, 0, 1000);
    run("carriers, truncated", es, rs, 5, 3);
  }
  for (int extra : {0, 1}) {   // the entry list and the event list, at and one beyond; a group in front and one behind
    std::vector<Ent> es = {make(ref, 15, 0, {30}), make(ref, 15, 0, {})};
    for (int i = 0; i < LC_EV_ENTS + extra; ++i) es.push_back(make(ref, 15, 1, {40 + 2 * (i % 40)}));
    es.push_back(make(ref, 17, 1, {50}));
    run(extra ? "entry list, one beyond" : "entry list, full", es, tiles(es[2], 10, 60), 5);
    es.resize(2);
    for (int i = 0; i < 4; ++i) { std::vector<int> at; for (int q = 0; q < 16 + (i == 3 ? extra : 0); ++q) at.push_back(20 + 3 * q + (i & 1)); es.push_back(make(ref, 15, 1, at)); }
    es.push_back(make(ref, 17, 1, {50}));
    run(extra ? "event list, one beyond" : "event list, full", es, tiles(es[2], 0, 60), 255);
  }
  for (int extra : {-1, 0, 1}) {   // the end of the staging pool: the second path fits with its two zero words, exactly, or not
    const int m = 16 * (LC_EV_POOL / 2 - 2) + 16 * extra;
    const std::string p = rnd(s, m);
    const std::vector<Ent> es = {make(p, 15, 0, {}), make(p, 15, 0, {m - 30})};
    run("staging", es, {es[1].s.substr((size_t)m - 60), p.substr((size_t)m - 60), es[1].s.substr((size_t)m - 40) + rnd(s, 10), rnd(s, 10) + p.substr(0, 30)}, 5);
  }
  for (int n : {1, 4, 5}) {
    const Ent a = make(ref, 15, 0, {75});
    std::vector<std::string> rs;
    for (int i = 0; i < n; ++i) rs.push_back(a.s.substr((size_t)(40 + 5 * i), 60));
    run("reads", {make(ref, 15, 0, {}), a}, rs, 5);
  }
  run("site at the ends", {make(ref, 15, 0, {0}), make(ref, 15, 0, {1}), make(ref, 15, 0, {198}), make(ref, 15, 0, {199}), make(ref, 15, 0, {})}, {ref.substr(0, 50), ref.substr(150), rnd(s, 10) + ref.substr(0, 30)}, 5);
  run("no entries", {}, {rnd(s, 40)}, 5);
  run("no reads", {make(ref, 15, 0, {60})}, {}, 5);
  printf(failures ? "FAILED\n" : "ok\n");
  return failures ? 1 : 0;
}
