// hap_support.h -- the support kernel: how many reads of a window fit each of its haplotypes (lancet_engine_set_haplotype_support).
//
// It runs after the batch's windows are through (engine.hip lancet_engine_wait, behind the re-run tier): the window's haplotype entries
// (layout.h, "haplotype capture") are final then, and the batch's trimmed, 2-bit packed reads are still resident.  One workgroup of
// LC_SUP_WG lanes per window; it counts into the HP_SUP_WORDS words the window kernels reserved behind every entry (kernels.h hap_sup).
//
// The quantity (include/lancet_engine.h states it for callers).  An entry h of M bases at k, a read of t >= k bases: a placement is an
// offset o in [k - t, M - k] -- the read may hang over either end, the overlap v(o) = min(t, M - o) - max(0, -o) is at least k -- mm(o)
// the overlap positions at which read and path differ, d(r, h) the smallest mm(o).  The GROUP of an entry is its HP_W_KC word,
// (k, component); a window visits each k once and each component of it once, so the entries of a group lie one behind the other and a
// group is a run of entries with one HP_W_KC.  The read FITS h iff d(r, h) is the smallest d of the run and <= max_mm; ALONE iff no
// other entry of the run has that d.  fit[4] and alone[4] count such reads by class Tf Tr Nf Nr (NodeGr::kc's order).
//
// Shape.  A wave takes a read at a time (the workgroup LC_SUP_WAVES reads), its lanes take offsets, 64 to a trip.  Per 16 read bases a
// lane forms the path's bases at its offset from two neighbouring path words (a 64-bit shift; words outside the path read as 0), XORs,
// folds each base's two difference bits into one, masks the bases outside the overlap and adds the popcount.  A wave reduction and an
// LDS word per wave give d.  Per run a wave keeps the smallest d, how many entries have it and where the first one is: a read that is
// alone is counted there and then; only for a tie the run is walked a second time to find who shares it.  Nothing is kept per entry or
// per read, so neither their number nor their lengths are limited.  Counts go to the entries with vector atomics.
//
// Phase style (wave.h): every lane runs every loop, control values are read from HBM or LDS alike by all lanes, phases end at a
// barrier.  With LANCET_WAVE_EMU the same source runs the lanes one after the other on the host (tests/hap_sup_emu).
#pragma once
#include "wave.h"
#include "layout.h"
#include "../../include/lancet_engine.h"

#define LC_SUP_WAVES 4
#define LC_SUP_WG (64 * LC_SUP_WAVES)
#define LC_SUP_NONE 0xFFFFFFFFu       /* no placement: t < k or M < k */

struct SupShared {
  uint32_t dmin[LC_SUP_WAVES];        /* d of the wave's read on the entry at hand                                          */
  uint32_t best[LC_SUP_WAVES];        /* the smallest d of the run so far, ...                                               */
  uint32_t nbest[LC_SUP_WAVES];       /* ... how many entries of the run have it, ...                                        */
  uint32_t arg[LC_SUP_WAVES];         /* ... and the first of them (word offset of the entry in the window's buffer)          */
  uint32_t tie[LC_SUP_WAVES];         /* the read fits several entries of the run: the second walk finds them                */
};

#ifndef LANCET_WAVE_EMU
DEV uint32_t sup_wave_min(uint32_t v, bool *lead) {
  for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, d, 64); v = o < v ? o : v; }
  *lead = (threadIdx.x & 63u) == 0;
  return v;
}
#else
DEV uint32_t sup_wave_min(uint32_t v, bool *lead) { *lead = true; return v; }      // (lanes one after the other: each brings its own)
#endif

// mm(o): read positions [lo, hi) lie on the path.  The rule is stated here once, for this kernel and for the placement kernel (hap_place.h).
// PAD: pw is a copy of the path words with a zero word in front and one behind (pw[-1], pw[npw]) -- every q below lies in -1 .. npw - 1 (the
// first word's p is >= -15, the last word's p <= M - 1), so the two words are taken without the bounds tests.
template <bool PAD, class PW>
DEV uint32_t sup_mm_at(LC_GLOBAL const uint32_t *rw, int t, PW pw, int M, int o) {
  const int lo = o < 0 ? -o : 0, hi = t < M - o ? t : M - o;
  const int npw = (M + 15) >> 4;
  uint32_t mm = 0;
  for (int wi = lo >> 4; wi < ((hi + 15) >> 4); ++wi) {
    const int p = o + 16 * wi;                                   // path position under the word's first base (negative: in front of the path)
    const int q = p >> 4, s = p & 15;
    const uint32_t a = PAD ? pw[q] : ((q >= 0 && q < npw) ? pw[q] : 0u), b = PAD ? pw[q + 1] : ((q + 1 >= 0 && q + 1 < npw) ? pw[q + 1] : 0u);
    const uint32_t at = (uint32_t)(((((unsigned long long)b) << 32) | (unsigned long long)a) >> (2 * s));
    uint32_t x = rw[wi] ^ at;
    x = (x | (x >> 1)) & 0x55555555u;                             // one bit per base that differs
    const int b0 = lo > 16 * wi ? lo - 16 * wi : 0, b1 = hi - 16 * wi < 16 ? hi - 16 * wi : 16;      // 0 <= b0 < b1 <= 16
    const uint32_t m1 = b1 >= 16 ? 0xFFFFFFFFu : ((1u << (2 * b1)) - 1u), m0 = (1u << (2 * b0)) - 1u;
    mm += (uint32_t)dev_popc(x & m1 & ~m0);
  }
  return mm;
}
DEV uint32_t sup_mm(LC_GLOBAL const uint32_t *rw, int t, LC_GLOBAL const uint32_t *pw, int M, int o) { return sup_mm_at<false>(rw, t, pw, M, o); }

// A whole entry at word `at` of a window's buffer of which `used` words count: its length, group, where its support words are and where
// the next entry starts.  false: no (further) whole entry -- the bounds lc_hap_collect (host_common.h) checks.
DEV bool sup_entry(LC_GLOBAL const uint32_t *buf, uint32_t used, uint32_t at, uint32_t *kc, uint32_t *sup, uint32_t *next) {
  if (at > used || HP_HDR > used - at) return false;
  LC_GLOBAL const uint32_t *e = buf + at;
  uint32_t room = used - at - HP_HDR;
  const uint32_t nw = (e[HP_W_LEN] + 15u) / 16u;
  if (nw > room) return false;
  room -= nw;
  const uint32_t nc = e[HP_W_NCIG];
  if (nc > room) return false;
  room -= nc;
  const uint32_t nv = (e[HP_W_FLAGS] & LANCET_HAP_HAS_COVERAGE) ? 2u * (e[HP_W_LEN] + e[HP_W_REFLEN]) : 0u;
  if (nv > room) return false;
  room -= nv;
  if (!(e[HP_W_FLAGS] & LANCET_HAP_HAS_SUPPORT) || HP_SUP_WORDS > room) return false;      // (an entry without the words: a run without the switch)
  *kc = e[HP_W_KC]; *sup = at + HP_HDR + nw + nc + nv; *next = *sup + HP_SUP_WORDS;
  return true;
}

// d of reads r0 .. r0 + LC_SUP_WAVES - 1 of the window on the entry at e, into S->dmin (cleared by the caller); ties: only for the waves
// that are looking for the entries that share their smallest d
DEV void sup_dist(LC_GLOBAL const DevBatch *B, uint32_t g0, int R, int r0, LC_GLOBAL const uint32_t *e, LC_LDS SupShared *S, bool ties) {
  const int M = (int)e[HP_W_LEN], k = (int)(e[HP_W_KC] & 0xFFFFu);
  LC_GLOBAL const uint32_t *pw = e + HP_HDR;
  WG_FOR(l, LC_SUP_WG) {
    const int wv = l >> 6, r = r0 + wv;
    if (r < R && (!ties || S->tie[wv])) {
      const int t = (int)RI_TLEN(B->rinfo[g0 + (uint32_t)r]);
      LC_GLOBAL const uint32_t *rw = B->bases + B->base_woff[g0 + (uint32_t)r];
      uint32_t m = LC_SUP_NONE;
      if (t >= k && M >= k)
        for (int o = k - t + (l & 63); o <= M - k; o += 64) { const uint32_t x = sup_mm(rw, t, pw, M, o); m = x < m ? x : m; }
      bool lead;
      m = sup_wave_min(m, &lead);
      if (lead && m != LC_SUP_NONE) dev_atomic_min((LC_LDS uint32_t *)&S->dmin[wv], m);
    }
  }
  WG_SYNC();
}

// one window
DEV void hap_support_window(LC_GLOBAL const DevBatch *B, LC_GLOBAL const uint32_t *hap_len, LC_GLOBAL uint32_t *hap_out, uint32_t cap, uint32_t max_mm,
                            int w, LC_LDS SupShared *S) {
  const uint32_t lw = hap_len[w] & ~HP_TRUNC, used = lw < cap ? lw : cap;      // (a truncated window: its whole entries)
  LC_GLOBAL uint32_t *buf = hap_out + (size_t)w * cap;
  const uint32_t g0 = B->read_begin[w];
  const int R = (int)(B->read_begin[w + 1] - g0);
  uint32_t kc, sup, next;
  if (R <= 0 || !sup_entry(buf, used, 0u, &kc, &sup, &next)) return;
  for (int r0 = 0; r0 < R; r0 += LC_SUP_WAVES) {
    uint32_t at = 0;
    while (sup_entry(buf, used, at, &kc, &sup, &next)) {
      // ---- the run of entries of this group: every wave's smallest d, how often, where first
      const uint32_t key = kc;
      WG_FOR(l, LC_SUP_WG) { if ((l & 63) == 0) { const int wv = l >> 6; S->best[wv] = LC_SUP_NONE; S->nbest[wv] = 0; S->arg[wv] = 0; S->tie[wv] = 0; S->dmin[wv] = LC_SUP_NONE; } }
      WG_SYNC();
      uint32_t end = at;
      while (sup_entry(buf, used, end, &kc, &sup, &next) && kc == key) {
        sup_dist(B, g0, R, r0, buf + end, S, false);
        WG_FOR(l, LC_SUP_WG) {
          if ((l & 63) == 0) {
            const int wv = l >> 6; const uint32_t d = S->dmin[wv];
            if (d < S->best[wv]) { S->best[wv] = d; S->nbest[wv] = 1; S->arg[wv] = end; }
            else if (d == S->best[wv] && d != LC_SUP_NONE) ++S->nbest[wv];
            S->dmin[wv] = LC_SUP_NONE;
          }
        }
        WG_SYNC();
        end = next;
      }
      // ---- a read that fits one entry is counted there; one that fits several asks for the second walk
      WG_FOR(l, LC_SUP_WG) {
        if ((l & 63) == 0) {
          const int wv = l >> 6, r = r0 + wv;
          if (r < R && S->best[wv] <= max_mm) {
            if (S->nbest[wv] == 1) {
              const uint32_t ri = B->rinfo[g0 + (uint32_t)r], cls = (RI_NML(ri) ? 2u : 0u) + (RI_REV(ri) ? 1u : 0u);
              uint32_t ksup, knext, kkc;
              if (sup_entry(buf, used, S->arg[wv], &kkc, &ksup, &knext)) { dev_atomic_add(buf + ksup + cls, 1u); dev_atomic_add(buf + ksup + 4u + cls, 1u); }
            } else S->tie[wv] = 1;
          }
        }
      }
      WG_SYNC();
      uint32_t any = 0;
      for (int wv = 0; wv < LC_SUP_WAVES; ++wv) any |= S->tie[wv];
      WG_SYNC();                                                  // (every lane has read the marks before the next run clears them)
      if (any) {
        for (uint32_t x = at; x != end && sup_entry(buf, used, x, &kc, &sup, &next); x = next) {
          sup_dist(B, g0, R, r0, buf + x, S, true);
          WG_FOR(l, LC_SUP_WG) {
            if ((l & 63) == 0) {
              const int wv = l >> 6, r = r0 + wv;
              if (r < R && S->tie[wv] && S->dmin[wv] == S->best[wv]) {
                const uint32_t ri = B->rinfo[g0 + (uint32_t)r], cls = (RI_NML(ri) ? 2u : 0u) + (RI_REV(ri) ? 1u : 0u);
                dev_atomic_add(buf + sup + cls, 1u);
              }
              S->dmin[wv] = LC_SUP_NONE;
            }
          }
          WG_SYNC();
        }
      }
      at = end;
    }
  }
}

#ifndef LANCET_WAVE_EMU
// grid: one workgroup per window of the batch
__global__ void __launch_bounds__(LC_SUP_WG) hap_support_kernel(const DevBatch *B, const uint32_t *hap_len, uint32_t *hap_out, uint32_t cap, uint32_t max_mm, int n_windows) {
  __shared__ SupShared sh;
  const int w = (int)blockIdx.x;
  if (w >= n_windows) return;
  hap_support_window((LC_GLOBAL const DevBatch *)B, (LC_GLOBAL const uint32_t *)hap_len, (LC_GLOBAL uint32_t *)hap_out, cap, max_mm, w, (LC_LDS SupShared *)&sh);
}
#endif
