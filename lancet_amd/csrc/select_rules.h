// select_rules.h -- read selection over the resident alignment table: the rules of extractReads (reference src/Microassembler.cc:436-655)
// and isActiveRegion (:253-432) for one window, written once.  hipcc compiles them into the two selection kernels of select.hip, one
// 64-lane wave per window; with LANCET_WAVE_EMU (tests/select_emu only, never the product build) the same source is plain C++ that runs
// the lanes of a loop one after the other, so that the rules are held against lancet_host_batch_packed without a GPU.
//
// What belongs to the alignment whatever the window was worked out once by lancet_host_alignment_table: the two filter bits, the evidence
// events, the per-read word (trimmed length, sample, strand, mate, mapped), the name, the packed words.  Left to do per window:
//   pass 1  [lo, hi) by binary search in the sample's contig, containment, the coverage cut-off, evidence counts -> lancet_select_summary
//   pass 2  for a kept window: its reads in file order (tumor, then normal) -> rinfo, word offsets, dense name rank
#pragma once
#include "wave.h"
#include "../../include/lancet_engine.h"

#define SEL_WAVES 4                 /* windows (= waves) per workgroup */
#define SEL_CAP 1024                /* selected reads of one window the second pass stages in LDS (more: the batch is not taken) */
#define SEL_HASH 1024               /* (sample, kind, position) counters of one window in LDS (full: the batch is not taken) */
#define SEL_ST_KEPT 1u
#define SEL_ST_SKIPPED 2u
#define SEL_ST_MAPPED 4u
#define SEL_ST_EVT_OVERFLOW 8u

struct SelTable {                   // lancet_alignment_table with pointers the kernels can follow (device memory; host memory in the emulation)
  uint32_t n_chroms, n_aln[2];
  const uint32_t *span;
  const int32_t *pos0, *ref_len;
  const uint32_t *l_seq;
  const uint8_t *flags;
  const uint32_t *rinfo, *evt_off;
  const uint8_t *evt_kind;
  const int32_t *evt_pos;
  const uint32_t *name_off;
  const char *names;
  const uint32_t *base_woff, *good_woff;
};
struct SelWin { int32_t start, end, chr; uint32_t ref_len; };        // one window of the slice
struct SelOpts { int32_t active_region, min_evidence, max_avg_cov, reserved; };
struct SelLds1 { unsigned long long hkey[SEL_HASH]; uint32_t hcnt[SEL_HASH]; };
struct SelLds2 { unsigned long long key[SEL_CAP]; uint32_t sel[SEL_CAP], ord[SEL_CAP]; };      // staged read j: its name key, its alignment; ord: the sort's permutation
struct SelOut { uint32_t *rinfo, *name_rank, *base_woff, *good_woff; };

#ifndef LANCET_WAVE_EMU
#define SEL_LANE ((uint32_t)(threadIdx.x & 63u))
#define SEL_FOR(i, n) for (uint32_t i = SEL_LANE; i < (uint32_t)(n); i += 64u)
// a loop every lane of the wave goes through together, 64 consecutive items per trip (`act`: this lane has one): ballots inside are whole
#define SEL_ORDERED_BEGIN(i, act, lo, hi) for (uint32_t _b = (lo); _b < (hi); _b += 64u) { const uint32_t i = _b + SEL_LANE; const bool act = i < (hi);
#define SEL_ORDERED_END }
// the waves of a workgroup work on different windows and never meet: what one wave's lanes hand each other through LDS is ordered by
// the wave's own instruction stream (LDS operations of a wave complete in order); the fence keeps the compiler from moving them
#define SEL_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
DEV uint32_t sel_sum(uint32_t v) { for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64); return v; }
DEV unsigned long long sel_sum(unsigned long long v) { for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64); return v; }
DEV bool sel_any(bool p) { return __ballot(p) != 0; }
struct SelRank { uint32_t cnt; };
// place of this lane's item among the items with `p` so far, in item order (ballot + prefix); every lane of the wave calls it
DEV uint32_t sel_rank(SelRank &s, bool p) {
  const unsigned long long b = __ballot(p);
  const uint32_t r = s.cnt + (uint32_t)__popcll(b & ((1ull << SEL_LANE) - 1ull));
  s.cnt += (uint32_t)__popcll(b);
  return r;
}
#else
#define SEL_FOR(i, n) for (uint32_t i = 0; i < (uint32_t)(n); ++i)
#define SEL_ORDERED_BEGIN(i, act, lo, hi) for (uint32_t i = (lo); i < (hi); ++i) { const bool act = true;
#define SEL_ORDERED_END }
#define SEL_SYNC() ((void)0)
DEV uint32_t sel_sum(uint32_t v) { return v; }                       // (the lanes of a loop share the accumulator: it already holds the sum)
DEV unsigned long long sel_sum(unsigned long long v) { return v; }
DEV bool sel_any(bool p) { return p; }
struct SelRank { uint32_t cnt; };
DEV uint32_t sel_rank(SelRank &s, bool p) { const uint32_t r = s.cnt; if (p) ++s.cnt; return r; }
#endif

// [lo, hi) of sample s in the window's contig: the first start >= win.start up to the first start > win.end (extractReads seeks to the
// window and stops at the first alignment that starts behind it)
DEV void sel_range(const SelTable &T, const SelWin &W, int s, uint32_t *lo, uint32_t *hi) {
  uint32_t a = 0, b = 0;
  if (W.chr >= 0 && (uint32_t)W.chr < T.n_chroms) { a = T.span[((uint32_t)s * T.n_chroms + (uint32_t)W.chr) * 2u]; b = T.span[((uint32_t)s * T.n_chroms + (uint32_t)W.chr) * 2u + 1u]; }
  uint32_t l = a, r = b;
  while (l < r) { const uint32_t m = l + (r - l) / 2u; if (T.pos0[m] < W.start) l = m + 1u; else r = m; }
  *lo = l; r = b;
  while (l < r) { const uint32_t m = l + (r - l) / 2u; if (T.pos0[m] <= W.end) l = m + 1u; else r = m; }
  *hi = l;
}
// (alstart >= win.start holds for every alignment of [lo, hi))
DEV bool sel_contained(const SelTable &T, const SelWin &W, uint32_t i) { return T.pos0[i] + T.ref_len[i] <= W.end; }

// One more event at (sample, kind, position); true when its count has reached `thr`.  Open addressing over 64-bit keys that are never 0.
DEV bool sel_count(SelLds1 *L, unsigned long long key, int thr, uint32_t *overflow) {
  unsigned long long x = key * 0x9E3779B97F4A7C15ULL;
  uint32_t h = (uint32_t)(x >> 40) & (SEL_HASH - 1u);
  for (uint32_t probes = 0; probes < SEL_HASH; ++probes) {
    const unsigned long long old = dev_atomic_cas64(&L->hkey[h], 0ull, key);
    if (old == 0ull || old == key) return (int)(dev_atomic_add(&L->hcnt[h], 1u) + 1u) >= thr;
    h = (h + 1u) & (SEL_HASH - 1u);
  }
  *overflow = 1u;
  return false;
}

DEV void sel_pass1(const SelTable &T, const SelWin &W, const SelOpts &O, SelLds1 *L, lancet_select_summary *out) {
  const bool ar = O.active_region != 0;
  if (ar) { SEL_FOR(q, SEL_HASH) { L->hkey[q] = 0ull; L->hcnt[q] = 0u; } SEL_SYNC(); }
  uint32_t n_sel[2] = {0, 0}, bases = 0, tw16 = 0, tw32 = 0, mapped = 0, overflow = 0, active = 0, skip = 0;
  for (int s = 0; s < 2; ++s) {
    uint32_t lo, hi; sel_range(T, W, s, &lo, &hi);
    unsigned long long before_last = 0;            // bases of the reads selected before index hi - 1: what extractReads' last coverage test sees
    uint32_t cnt = 0, nb = 0;
    SEL_FOR(q, hi - lo) {
      const uint32_t i = lo + q;
      if (!sel_contained(T, W, i)) continue;
      const uint32_t f = T.flags[i];
      if (f & LANCET_ALN_SEL_OK) {
        const uint32_t l = T.l_seq[i], ri = T.rinfo[i], tl = RI_TLEN(ri);
        ++cnt; nb += l; tw16 += (tl + 15u) / 16u; tw32 += (tl + 31u) / 32u; mapped |= (ri >> 20) & 1u;
        if (i + 1u < hi) before_last += l;
      }
      if (ar && (f & LANCET_ALN_AR_OK)) {
        for (uint32_t e = T.evt_off[i]; e < T.evt_off[i + 1u]; ++e) {
          const unsigned long long key = ((unsigned long long)((uint32_t)s * 4u + T.evt_kind[e] + 1u) << 32) | (uint32_t)T.evt_pos[e];
          if (sel_count(L, key, O.min_evidence, &overflow)) active = 1u;
        }
      }
    }
    n_sel[s] = sel_sum(cnt); bases += sel_sum(nb);
    before_last = sel_sum(before_last);
    // the cut-off is tested at the top of every iteration over [lo, hi), before containment: the sum only grows, so the window is skipped
    // iff the last test fires (:491-496; the same double division)
    if (hi > lo && W.ref_len > 0u && ((double)(long long)before_last / (double)W.ref_len) > (double)O.max_avg_cov) skip = 1u;
  }
  tw16 = sel_sum(tw16); tw32 = sel_sum(tw32);
  const bool is_mapped = sel_any(mapped != 0u), is_active = sel_any(active != 0u), is_over = sel_any(overflow != 0u);
  uint32_t st = 0;
  if (!ar || is_active) st = skip ? SEL_ST_SKIPPED : SEL_ST_KEPT;                // (both samples are read before the skip, :833-836)
  else if (is_over) st = SEL_ST_EVT_OVERFLOW;                                    // not seen active with counts missing: unknown
  if (is_mapped) st |= SEL_ST_MAPPED;
#ifndef LANCET_WAVE_EMU
  if (SEL_LANE == 0u)
#endif
  { out->status = st; out->reads_t = n_sel[0]; out->reads_n = n_sel[1]; out->bases = bases; out->tw16 = tw16; out->tw32 = tw32; }
}

// the first eight bytes of a name, big-endian, zero after its end: ordered like strcmp (unsigned bytes) over those bytes
DEV unsigned long long sel_name_key(const char *nm) {
  unsigned long long k = 0; bool end = false;
  for (int b = 0; b < 8; ++b) { uint32_t c = 0; if (!end) { c = (uint8_t)nm[b]; if (!c) end = true; } k = (k << 8) | c; }
  return k;
}
// strcmp of the names of two staged reads (0xFFFFFFFF: padding, behind every name): < 0, 0, > 0
DEV int sel_name_cmp(const SelTable &T, const SelLds2 *L, uint32_t a, uint32_t b) {
  if (a == 0xFFFFFFFFu || b == 0xFFFFFFFFu) return a == b ? 0 : (a == 0xFFFFFFFFu ? 1 : -1);
  const unsigned long long ka = L->key[a], kb = L->key[b];
  if (ka != kb) return ka < kb ? -1 : 1;
  if (!(ka & 0xFFull)) return 0;                                                  // both end inside the eight bytes
  const char *x = T.names + T.name_off[L->sel[a]] + 8, *y = T.names + T.name_off[L->sel[b]] + 8;
  for (;; ++x, ++y) { const uint32_t cx = (uint8_t)*x, cy = (uint8_t)*y; if (cx != cy) return cx < cy ? -1 : 1; if (!cx) return 0; }
}

// Reads of a kept window: rows r0 .. r0 + expect - 1 of the batch's per-read arrays (expect: what pass 1 counted; nothing is written otherwise).
DEV void sel_pass2(const SelTable &T, const SelWin &W, uint32_t r0, uint32_t expect, SelLds2 *L, const SelOut &out) {
  SelRank rk; rk.cnt = 0;
  for (int s = 0; s < 2; ++s) {
    uint32_t lo, hi; sel_range(T, W, s, &lo, &hi);
    SEL_ORDERED_BEGIN(i, act, lo, hi)
      const bool p = act && sel_contained(T, W, i) && (T.flags[i] & LANCET_ALN_SEL_OK);
      const uint32_t at = sel_rank(rk, p);
      if (p && at < SEL_CAP) L->sel[at] = i;
    SEL_ORDERED_END
  }
  const uint32_t n = rk.cnt;
  if (n > SEL_CAP || n != expect) return;          // (the host does not launch the pass for such a batch)
  uint32_t n2 = 1; while (n2 < n) n2 <<= 1;
  SEL_SYNC();
  SEL_FOR(j, n2) {
    if (j < n) {
      const uint32_t a = L->sel[j];
      out.rinfo[r0 + j] = T.rinfo[a]; out.base_woff[r0 + j] = T.base_woff[a]; out.good_woff[r0 + j] = T.good_woff[a];
      L->key[j] = sel_name_key(T.names + T.name_off[a]);
      L->ord[j] = j;
    } else L->ord[j] = 0xFFFFFFFFu;
  }
  // bitonic sort of the permutation by name
  for (uint32_t k = 2; k <= n2; k <<= 1) for (uint32_t j = k >> 1; j > 0; j >>= 1) {
    SEL_SYNC();
    SEL_FOR(t, n2 / 2u) {
      const uint32_t x = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), y = x | j;
      const uint32_t a = L->ord[x], b = L->ord[y];
      const int c = sel_name_cmp(T, L, a, b);
      if (((x & k) == 0u) ? c > 0 : c < 0) { L->ord[x] = b; L->ord[y] = a; }
    }
  }
  SEL_SYNC();
  // dense rank: names in order, one more for every name that differs from the one before it
  SelRank nr; nr.cnt = 0;
  SEL_ORDERED_BEGIN(j, act, 0u, n)
    const bool isnew = act && j > 0u && sel_name_cmp(T, L, L->ord[j - 1u], L->ord[j]) != 0;
    const uint32_t before = sel_rank(nr, isnew);
    if (act) out.name_rank[r0 + L->ord[j]] = before + (isnew ? 1u : 0u);
  SEL_ORDERED_END
}
