// hap_place.h -- the placement kernel: where each read of a window lies on the haplotype it fits best (lancet_engine_set_haplotype_placements).
//
// It runs where the support kernel runs (engine.hip lancet_engine_wait, behind the re-run tier): the windows' entries are final, the batch's
// trimmed, packed reads are resident.  One workgroup of LC_SUP_WG lanes per window; it writes one record of PL_WORDS words per read
// (layout.h, "read placements") into a buffer of its own and touches no entry.
//
// The quantity (include/lancet_engine.h states it for callers) reuses the support kernel's terms: offsets o in [k - t, M - k], mm(o), d(r, h)
// the smallest mm(o) on entry h.  Over all whole entries of the window, whatever their group: mismatches = the smallest d; haplotype = the
// first entry that has it; offset = the smallest o on that entry with mm(o) = d; n_offsets = how many offsets of that entry have it;
// n_haplotypes = how many entries have that d.  The read is placed iff mismatches <= max_mm.
//
// Shape.  Lane 0 parses the window's entries once into an LDS list (word offset, M, k, index); entries beyond its LC_PL_ENTS are parsed in
// place as the walk reaches them.  The entries are the outer loop: the workgroup copies an entry's path words into LDS once, a zero word
// in front and one behind, so that the inner loop takes pw[q] and pw[q + 1] without bounds tests (sup_mm_at<true>, hap_support.h: the one
// statement of the mask arithmetic); a path of more than LC_PL_STAGE words is read in place with the tests.  Then a wave takes a read at a
// time, its lanes the offsets, 64 to a trip, each lane keeping its smallest mm, the first offset that reached it and how many of its
// offsets did.  A wave reduction on the pair (mm, o) gives d and the smallest offset, a second one sums the counts of the lanes whose own
// smallest mm is d.  The running best of a read over the entries IS its record: the wave that owns the read (read r of the window: wave
// r % LC_SUP_WAVES, always) folds an entry's result into it with plain vector loads and stores -- a smaller d replaces it, an equal d
// counts one more haplotype, so the first entry wins.  One walk, no atomics.
//
// Phase style (wave.h): every lane runs every loop, control values are read from LDS alike by all lanes.  The per-wave words key[] / cnt[]
// are written and read by the wave's first lane only, so the two phases of a read need no barrier between them; barriers stand around the
// staging.  With LANCET_WAVE_EMU the lanes run one after the other and each brings its own pair to the same fold (tests/hap_place_emu).
#pragma once
#include "hap_support.h"

#define LC_PL_ENTS 32                  /* entries of the LDS list (lancet_gpu sizes a window's buffer for 32 paths) */
#define LC_PL_STAGE 128                /* path words staged: 2048 bases (the longest path of a default run, max_w + max_indel_len + 256 = 1780 bases, takes 112) */
#define LC_PL_NONE 0xFFFFFFFFu         /* no placement */
#define LC_PL_MM_CLAMP 0x3FFEu         /* (mm, o) pairs are ordered as mm << PL_OFF_BITS | o + PL_OFF_BIAS: 14 bits of mm, far above any limit */

struct PlEnt { uint32_t at, M, k, idx; };
struct PlShared {
  uint32_t n_ent;                      /* whole entries of the window                                                        */
  uint32_t over_at;                    /* where entry number LC_PL_ENTS starts: from there on the entries are parsed in place */
  PlEnt ent[LC_PL_ENTS];
  uint32_t key[LC_SUP_WAVES];          /* the wave's read on the entry at hand: (d, smallest offset) ...                      */
  uint32_t cnt[LC_SUP_WAVES];          /* ... and how many offsets have that d                                               */
  uint32_t stage[LC_PL_STAGE + 2];     /* 0, the entry's path words, 0                                                       */
};

#ifndef LANCET_WAVE_EMU
DEV uint32_t pl_wave_sum(uint32_t v) {
  for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
  return v;
}
#else
DEV uint32_t pl_wave_sum(uint32_t v) { return v; }      // (lanes one after the other: each brings its own)
#endif

// A whole entry at word `at` of a window's buffer of which `used` words count, and where the next one starts: lc_hap_collect's bounds
// (host_common.h), so the n-th entry here is the haplotype with index_in_window n.
DEV bool pl_entry(LC_GLOBAL const uint32_t *buf, uint32_t used, uint32_t at, uint32_t *next) {
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
  const uint32_t ns = (e[HP_W_FLAGS] & LANCET_HAP_HAS_SUPPORT) ? HP_SUP_WORDS : 0u;
  if (ns > room) return false;
  *next = at + HP_HDR + nw + nc + nv + ns;
  return true;
}

// one window; rec: the batch's records, PL_WORDS per read, zeroed
DEV void hap_placement_window(LC_GLOBAL const DevBatch *B, LC_GLOBAL const uint32_t *hap_len, LC_GLOBAL const uint32_t *hap_out, uint32_t cap, uint32_t max_mm,
                              LC_GLOBAL uint32_t *rec, int w, LC_LDS PlShared *S) {
  const uint32_t lw = hap_len[w] & ~HP_TRUNC, used = lw < cap ? lw : cap;      // (a truncated window: its whole entries)
  LC_GLOBAL const uint32_t *buf = hap_out + (size_t)w * cap;
  const uint32_t g0 = B->read_begin[w];
  const int R = (int)(B->read_begin[w + 1] - g0);
  if (R <= 0) return;
  // ---- the entries, once
  WG_FOR(l, LC_SUP_WG) {
    if (l == 0) {
      uint32_t n = 0, at = 0, next = 0, over = 0;
      while (n < PL_IDX_MAX && pl_entry(buf, used, at, &next)) {
        if (n < LC_PL_ENTS) { S->ent[n].at = at; S->ent[n].M = buf[at + HP_W_LEN]; S->ent[n].k = buf[at + HP_W_KC] & 0xFFFFu; S->ent[n].idx = n; }
        else if (n == LC_PL_ENTS) over = at;
        ++n; at = next;
      }
      S->n_ent = n; S->over_at = over;
      for (int wv = 0; wv < LC_SUP_WAVES; ++wv) { S->key[wv] = LC_PL_NONE; S->cnt[wv] = 0; }
    }
  }
  WG_SYNC();
  const uint32_t n_ent = S->n_ent;
  uint32_t at_cur = S->over_at;
  for (uint32_t ei = 0; ei < n_ent; ++ei) {
    uint32_t at, idx; int M, k;
    if (ei < LC_PL_ENTS) { at = S->ent[ei].at; M = (int)S->ent[ei].M; k = (int)S->ent[ei].k; idx = S->ent[ei].idx; }
    else { at = at_cur; M = (int)buf[at + HP_W_LEN]; k = (int)(buf[at + HP_W_KC] & 0xFFFFu); idx = ei; uint32_t nx = at; (void)pl_entry(buf, used, at, &nx); at_cur = nx; }
    // ---- its path words into LDS, a zero word on either side
    const int npw = (M + 15) >> 4;
    const bool staged = npw <= LC_PL_STAGE;
    if (staged) { WG_FOR(i, npw + 2) S->stage[i] = (i == 0 || i == npw + 1) ? 0u : buf[at + HP_HDR + (uint32_t)(i - 1)]; }
    WG_SYNC();
    for (int r0 = 0; r0 < R; r0 += LC_SUP_WAVES) {
      // ---- every wave its read: d, the smallest offset that has it, how many have it
      WG_FOR(l, LC_SUP_WG) {
        const int wv = l >> 6, r = r0 + wv;
        if (r < R) {
          const int t = (int)RI_TLEN(B->rinfo[g0 + (uint32_t)r]);
          uint32_t m = LC_PL_NONE, c = 0; int mo = 0;
          if (t >= k && M >= k) {
            LC_GLOBAL const uint32_t *rw = B->bases + B->base_woff[g0 + (uint32_t)r];
            for (int o = k - t + (l & 63); o <= M - k; o += 64) {
              const uint32_t x = staged ? sup_mm_at<true>(rw, t, (LC_LDS const uint32_t *)S->stage + 1, M, o) : sup_mm_at<false>(rw, t, buf + at + HP_HDR, M, o);
              if (x < m) { m = x; mo = o; c = 1; } else if (x == m) ++c;      // (a lane's offsets ascend: the first one is its smallest)
            }
          }
          const uint32_t key = m == LC_PL_NONE ? LC_PL_NONE : ((m < LC_PL_MM_CLAMP ? m : LC_PL_MM_CLAMP) << PL_OFF_BITS) | (uint32_t)(mo + PL_OFF_BIAS);
          bool lead;
          const uint32_t kmin = sup_wave_min(key, &lead);
          const uint32_t csum = pl_wave_sum((key != LC_PL_NONE && (key >> PL_OFF_BITS) == (kmin >> PL_OFF_BITS)) ? c : 0u);
          if (lead && kmin != LC_PL_NONE) {
            const uint32_t have = S->key[wv];
            if (have == LC_PL_NONE || (kmin >> PL_OFF_BITS) < (have >> PL_OFF_BITS)) { S->key[wv] = kmin; S->cnt[wv] = csum; }
            else if ((kmin >> PL_OFF_BITS) == (have >> PL_OFF_BITS)) { S->key[wv] = kmin < have ? kmin : have; S->cnt[wv] += csum; }
          }
        }
      }
      // ---- ... folded into the read's record by the wave that owns it
      WG_FOR(l, LC_SUP_WG) {
        if ((l & 63) == 0) {
          const int wv = l >> 6, r = r0 + wv;
          const uint32_t key = S->key[wv];
          if (r < R && key != LC_PL_NONE && (key >> PL_OFF_BITS) <= max_mm) {
            const uint32_t d = key >> PL_OFF_BITS, off = ((key & PL_OFF_MASK) - (uint32_t)PL_OFF_BIAS) & PL_OFF_MASK;
            const uint32_t n_off = S->cnt[wv] < PL_CNT_MAX ? S->cnt[wv] : PL_CNT_MAX;
            LC_GLOBAL uint32_t *q = rec + (size_t)PL_WORDS * (g0 + (uint32_t)r);
            const uint32_t w0 = q[0], w1 = q[1];
            if (!(w0 & PL_IDX_MAX) || d < (w0 >> PL_MM_SHIFT)) stg2(q, (idx + 1u) | (d << PL_MM_SHIFT), off | (n_off << PL_NOFF_SHIFT) | (1u << PL_NHAP_SHIFT));
            else if (d == (w0 >> PL_MM_SHIFT) && (w1 >> PL_NHAP_SHIFT) < PL_CNT_MAX) q[1] = w1 + (1u << PL_NHAP_SHIFT);
          }
          S->key[wv] = LC_PL_NONE; S->cnt[wv] = 0;
        }
      }
    }
    WG_SYNC();                                                    // (every wave is through with the staged words before the next entry's replace them)
  }
}

#ifndef LANCET_WAVE_EMU
// grid: one workgroup per window of the batch
__global__ void __launch_bounds__(LC_SUP_WG) hap_placement_kernel(const DevBatch *B, const uint32_t *hap_len, const uint32_t *hap_out, uint32_t cap, uint32_t max_mm,
                                                                  uint32_t *rec, int n_windows) {
  __shared__ PlShared sh;
  const int w = (int)blockIdx.x;
  if (w >= n_windows) return;
  hap_placement_window((LC_GLOBAL const DevBatch *)B, (LC_GLOBAL const uint32_t *)hap_len, (LC_GLOBAL const uint32_t *)hap_out, cap, max_mm, (LC_GLOBAL uint32_t *)rec, w,
                       (LC_LDS PlShared *)&sh);
}
#endif
