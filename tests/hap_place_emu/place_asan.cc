// place_asan.cc -- TEST INFRASTRUCTURE ONLY.  A stand-alone program for the address / undefined-behaviour sanitizers (`make asan`): the
// emulated placement kernel (lancet_amd/csrc/hap_place.h under LANCET_WAVE_EMU) and lc_read_cigar (host_common.h) over hand-written
// buffers allocated to their exact sizes, so that a word read or written past an end is seen: one more entry than the LDS list holds,
// path words on both sides of the staging boundary, reads hanging over either end of a path, 1 / 4 / 5 reads, a truncated length word,
// both counts saturating.  Every record is held to a plain loop over the strings.  Nothing is loaded into Python.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../lancet_amd/csrc/host_common.h"
#include "../../lancet_amd/csrc/hap_place.h"

static std::string rnd(uint32_t &s, int n) { std::string r; for (int i = 0; i < n; ++i) { s = s * 1664525u + 1013904223u; r += "ACGT"[(s >> 24) & 3u]; } return r; }
static void pack(const std::string &s, std::vector<uint32_t> *out) {
  const size_t at = out->size(); out->resize(at + (s.size() + 15) / 16, 0u);
  for (size_t i = 0; i < s.size(); ++i) (*out)[at + i / 16] |= (uint32_t)(std::string("ACGT").find(s[i])) << (2 * (i % 16));
}
struct Ent { std::string s; int k; };
struct Rec { int hap, off, mm, noff, nhap; };
// the definition, in plain loops
static Rec model(const std::string &r, const std::vector<Ent> &es, int max_mm) {
  Rec best{-1, 0, 0, 0, 0};
  for (size_t e = 0; e < es.size(); ++e) {
    const int t = (int)r.size(), M = (int)es[e].s.size(), k = es[e].k;
    int d = -1, o0 = 0, n = 0;
    for (int o = -t; o <= M; ++o) {
      const int lo = o < 0 ? -o : 0, hi = t < M - o ? t : M - o;
      if (hi - lo < k) continue;
      int mm = 0;
      for (int i = lo; i < hi; ++i) mm += r[(size_t)i] != es[e].s[(size_t)(o + i)];
      if (d < 0 || mm < d) { d = mm; o0 = o; n = 1; } else if (mm == d) ++n;
    }
    if (d < 0 || d > max_mm) continue;
    if (best.hap < 0 || d < best.mm) best = Rec{(int)e, o0, d, n > (int)PL_CNT_MAX ? (int)PL_CNT_MAX : n, 1};
    else if (d == best.mm && best.nhap < (int)PL_CNT_MAX) ++best.nhap;
  }
  if (best.hap < 0) best = Rec{-1, 0, 0, 0, 0};
  return best;
}
static int failures = 0;
static void run(const char *what, const std::vector<Ent> &es, const std::vector<std::string> &reads, int max_mm, uint32_t trunc_after = 0) {
  std::vector<uint32_t> buf;
  uint32_t len_word = 0, n = 0;
  for (const Ent &e : es) {
    const uint32_t hdr[HP_HDR] = {(uint32_t)e.k, 0u, (uint32_t)e.s.size(), (uint32_t)e.s.size(), 0u, 0u, 0u, 0u};
    buf.insert(buf.end(), hdr, hdr + HP_HDR); pack(e.s, &buf);
    if (trunc_after && ++n == trunc_after) len_word = (uint32_t)buf.size() | HP_TRUNC;
  }
  if (!trunc_after) len_word = (uint32_t)buf.size();
  std::vector<uint32_t> heap_buf(buf);                                   // exact size: the sanitizer sees a word past the end
  std::vector<uint32_t> ri, bw, bases;
  for (const std::string &r : reads) { ri.push_back((uint32_t)r.size()); bw.push_back((uint32_t)bases.size()); pack(r, &bases); }
  const uint32_t rb[2] = {0u, (uint32_t)reads.size()};
  DevBatch B; memset(&B, 0, sizeof(B));
  B.n_windows = 1; B.read_begin = rb; B.rinfo = ri.data(); B.base_woff = bw.data(); B.bases = bases.data();
  std::vector<uint64_t> rec(reads.size() + 1, 0);
  static PlShared S;
  memset(&S, 0xCD, sizeof(S));
  hap_placement_window(&B, &len_word, heap_buf.data(), (uint32_t)heap_buf.size(), (uint32_t)max_mm, (uint32_t *)rec.data(), 0, &S);
  lancet_window_stats st; memset(&st, 0, sizeof(st));
  LcPlaceResult out;
  lc_place_collect(1, rb, ri.data(), (const uint32_t *)rec.data(), &st, &out);
  std::vector<Ent> whole(es.begin(), trunc_after ? es.begin() + trunc_after : es.end());
  for (size_t i = 0; i < reads.size(); ++i) {
    const Rec w = model(reads[i], whole, max_mm);
    const lancet_read_placement &g = out.p[i];
    if (g.haplotype != w.hap || g.offset != w.off || g.mismatches != w.mm || g.n_offsets != w.noff || g.n_haplotypes != w.nhap) {
      printf("FAIL %s read %zu: got %d %d %u %u %u, want %d %d %d %d %d\n", what, i, g.haplotype, g.offset, g.mismatches, g.n_offsets, g.n_haplotypes, w.hap, w.off, w.mm, w.noff, w.nhap);
      ++failures;
    }
    if (g.haplotype >= 0) {                                              // ... and the read's CIGAR through a path with an insertion and a deletion
      const uint32_t M = (uint32_t)whole[(size_t)g.haplotype].s.size();
      const uint32_t cig[5] = {(M / 4) << 4 | HP_OP_EQ, 3u << 4 | HP_OP_D, (M / 4) << 4 | HP_OP_I, 1u << 4 | HP_OP_X, (M - 2 * (M / 4) - 1) << 4 | HP_OP_EQ};
      uint32_t start = 0; std::vector<uint32_t> ops;
      lc_read_cigar(g.offset, out.tlen[i], M, 5u, cig, 5u, &start, &ops);
      uint32_t q = 0;
      for (uint32_t op : ops) if ((op & 15u) != LC_RC_D) q += op >> 4;
      if (q != out.tlen[i]) { printf("FAIL %s read %zu: CIGAR of %u query bases for a read of %u\n", what, i, q, (unsigned)out.tlen[i]); ++failures; }
    }
  }
  printf("%s: %zu entries, %zu reads\n", what, es.size(), reads.size());
}

int main() {
  uint32_t s = 12345u;
  {   // one more entry than the list holds, each with its own k; reads on the last ones and over their ends
    std::vector<Ent> es;
    for (int i = 0; i < LC_PL_ENTS + 2; ++i) es.push_back(Ent{rnd(s, 70 + i), 12 + i % 5});
    std::vector<std::string> rs = {es.back().s.substr(20, 40), es[LC_PL_ENTS].s.substr(0, 30), rnd(s, 20) + es.back().s.substr(0, 16), es[3].s.substr(50) + rnd(s, 25), rnd(s, 40)};
    run("entry list", es, rs, 5);
    run("entry list, truncated", es, rs, 5, LC_PL_ENTS + 1);
  }
  for (int extra : {0, 1, 16}) {   // the staging boundary
    const int m = 16 * LC_PL_STAGE + extra;
    const std::string p = rnd(s, m);
    run("staging", {Ent{p, 15}}, {p.substr(m - 50), p.substr(m - 20) + rnd(s, 30), rnd(s, 30) + p.substr(0, 20), p.substr(100, 33), p.substr(m - 16)}, 5);
  }
  for (int n : {1, 4, 5}) {
    const std::string p = rnd(s, 150);
    std::vector<std::string> rs;
    for (int i = 0; i < n; ++i) rs.push_back(p.substr(10 * i, 60));
    run("reads", {Ent{p, 15}, Ent{p.substr(0, 75) + "A" + p.substr(76), 15}}, rs, 5);
  }
  run("saturation of n_offsets", {Ent{std::string(300, 'A'), 15}}, {std::string(20, 'A')}, 5);
  { const std::string p = rnd(s, 60); run("saturation of n_haplotypes", std::vector<Ent>(PL_CNT_MAX + 3, Ent{p, 15}), {p.substr(5, 40)}, 5); }
  run("no entries", {}, {rnd(s, 40)}, 5);
  run("no reads", {Ent{rnd(s, 60), 15}}, {}, 5);
  printf(failures ? "FAILED\n" : "ok\n");
  return failures ? 1 : 0;
}
