// hap_evidence.h -- the evidence kernel: per allele of a window, the reads that carry it, the reference allele or something else at its
// site, judged by the haplotypes they fit (lancet_engine_set_haplotype_evidence).
//
// It runs where the support and placement kernels run (engine.hip lancet_engine_wait, behind the re-run tier and behind those two): the
// windows' entries with their CIGAR words are final, the batch's trimmed, packed reads are resident.  One workgroup of LC_SUP_WG lanes per
// window; it writes records of EV_WORDS words (layout.h, "variant evidence") into a buffer of its own and touches no entry.
//
// The quantity (include/lancet_engine.h states it for callers) reuses the support kernel's terms: offsets o in [k - t, M - k], mm(o),
// d(r, h), the group of an entry.  An EVENT of an entry is a maximal run of CIGAR words that are not '='; (rb, rs) its place on the group's
// reference stretch, (pb, ps) on the path.  Another entry of the group CARRIES the event's alt allele, the reference allele or something
// else there (EV_ALT / EV_REF / EV_OTHER) and has a SITE [left, right) on its own path; a read is INFORMATIVE on an entry it fits when its
// best placement there (the smallest offset that reaches d) covers the site and one path base on either side.
//
// Shape.  The groups of a window are taken one behind the other; every entry is parsed once, by lane 0, into the group's LDS list.
//   1. a lane per entry counts its events, lane 0 sums, a lane per entry writes them to the group's event list (a path's CIGAR is a few
//      words: the parallelism is across the entries, and the list comes out in entry order without a sort);
//   2. a lane per (event, entry) pair fills the table of carrier class and site; the entries' path words go into one LDS pool, each with a
//      zero word on either side (sup_mm_at<true>, hap_support.h: the one statement of the mask arithmetic);
//   3. a wave takes a read, its lanes the offsets of an entry, 64 to a trip; a wave reduction on the pair (mm, o) gives d and the smallest
//      offset that has it (hap_place.h's key); the wave keeps one key per entry of the group in LDS -- one walk, none for ties;
//   4. behind the group's last entry the wave's lanes take the group's events, each classifies the read against its event from the keys
//      and the table and adds to the event's counts in LDS;
//   5. behind the window's last read the counts go to the records with plain vector stores.  No atomics on HBM.
// The list holds LC_EV_ENTS entries, the event list LC_EV_EVENTS events.  A group beyond either is not evaluated: lane 0 writes its
// events with LANCET_EVID_UNEVALUATED and all counts 0, walking the entries in place.  A path that does not fit what is left of the pool
// is read in place, with the bounds tests.
//
// Phase style (wave.h): every lane runs every loop, control values are read from LDS alike by all lanes, phases end at a barrier.  The
// keys of a wave are written by its first lane and read by all its lanes: a barrier stands between the walk and the classification, and
// the keys alternate between two sets, so that the set the next walk writes is cleared a barrier before and a barrier after anyone reads
// it.  With LANCET_WAVE_EMU the lanes run one after the other and each folds its own pair into the same key (tests/hap_evid_emu).
#pragma once
#include "hap_place.h"

#define LC_EV_ENTS 32                  /* entries of a group's LDS list (lancet_gpu sizes a window's buffer for 32 paths) */
#define LC_EV_EVENTS 64                /* events of a group's LDS list */
#define LC_EV_POOL 4096                /* words of staged paths: 32 paths of 2016 bases, or fewer, longer ones */
#define LC_EV_NONE 0xFFFFFFFFu
enum { EV_REF = 0, EV_ALT = 1, EV_OTHER = 2 };
static_assert(LC_EV_ENTS == LANCET_EVID_GROUP_ENTRIES && LC_EV_EVENTS == LANCET_EVID_GROUP_EVENTS, "the capacities the public header states");

struct EvEnt { uint32_t at, M, cig, ncig, ev0, nev, stage; };       /* stage: the zero word in front of its words in the pool, LC_EV_NONE: not staged */
struct EvEvt { uint32_t ent, rb, rs, pb, ps; };
struct EvCur { uint32_t i, rb, pb; };                                /* a walk over an entry's CIGAR words: the next word, stretch and path bases in front of it */
struct EvShared {
  uint32_t g_at, g_idx, g_out;         /* the group at hand: where it starts, index_in_window of its first entry, events of the window in front of it */
  uint32_t g_next, more, ok;           /* where the next one starts; there is a group; it fits the lists */
  uint32_t n_ent, n_evt, k;            /* its entries (all of them), its events, its k */
  EvEnt ent[LC_EV_ENTS];
  EvEvt evt[LC_EV_EVENTS];
  uint32_t site[LC_EV_EVENTS * LC_EV_ENTS][2];      /* (event, entry): left | class << 30, right */
  uint32_t key[2][LC_SUP_WAVES][LC_EV_ENTS];        /* the wave's read on every entry of the group: (d, smallest offset) */
  uint32_t cnt[LC_EV_EVENTS][EV_COUNTS];
  uint32_t pool[LC_EV_POOL];
};

// The next event of an entry: a maximal run of words that are not '='.  D and X span stretch bases, I and X path bases.
template <class CP>
DEV bool ev_next(CP cig, uint32_t nc, EvCur *c, EvEvt *o) {
  while (c->i < nc && (cig[c->i] & 15u) == (uint32_t)HP_OP_EQ) { const uint32_t L = cig[c->i] >> 4; c->rb += L; c->pb += L; ++c->i; }
  if (c->i >= nc) return false;
  o->rb = c->rb; o->pb = c->pb; o->rs = 0; o->ps = 0;
  while (c->i < nc && (cig[c->i] & 15u) != (uint32_t)HP_OP_EQ) {
    const uint32_t L = cig[c->i] >> 4, op = cig[c->i] & 15u;
    if (op != (uint32_t)HP_OP_I) o->rs += L;
    if (op != (uint32_t)HP_OP_D) o->ps += L;
    ++c->i;
  }
  c->rb += o->rs; c->pb += o->ps;
  return true;
}
DEV uint32_t ev_base(LC_GLOBAL const uint32_t *pw, uint32_t i) { return (pw[i >> 4] >> (2u * (i & 15u))) & 3u; }

// one record's first words; the counts stay as the engine zeroed them until the window's reads are through
DEV void ev_record(LC_GLOBAL uint32_t *q, uint32_t idx, const EvEvt &x, uint32_t flags) {
  q[EV_W_IDX] = idx; q[EV_W_RB] = x.rb; q[EV_W_RS] = x.rs; q[EV_W_PB] = x.pb; q[EV_W_PS] = x.ps; q[EV_W_FLAGS] = flags;
}

// one window; rec: the batch's records, cap * EV_WORDS words per window, zeroed; ev_len[w]: the events the window has, kept or not
DEV void hap_evidence_window(LC_GLOBAL const DevBatch *B, LC_GLOBAL const uint32_t *hap_len, LC_GLOBAL const uint32_t *hap_out, uint32_t hcap, uint32_t max_mm,
                             LC_GLOBAL uint32_t *rec, LC_GLOBAL uint32_t *ev_len, uint32_t cap, int w, LC_LDS EvShared *S) {
  const uint32_t lw = hap_len[w] & ~HP_TRUNC, used = lw < hcap ? lw : hcap;      // (a truncated window: its whole entries)
  LC_GLOBAL const uint32_t *buf = hap_out + (size_t)w * hcap;
  LC_GLOBAL uint32_t *out = rec + (size_t)w * cap * EV_WORDS;
  const uint32_t g0 = B->read_begin[w];
  const int R = (int)(B->read_begin[w + 1] - g0);
  WG_FOR(l, LC_SUP_WG) { if (l == 0) { S->g_at = 0; S->g_idx = 0; S->g_out = 0; } }
  WG_SYNC();
  for (;;) {
    // ---- the group's entries, once
    WG_FOR(l, LC_SUP_WG) {
      if (l == 0) {
        uint32_t a = S->g_at, next = 0, n = 0, pool = 0;
        if (!pl_entry(buf, used, a, &next)) S->more = 0;
        else {
          const uint32_t kc = buf[a + HP_W_KC];
          while (pl_entry(buf, used, a, &next) && buf[a + HP_W_KC] == kc) {
            if (n < LC_EV_ENTS) {
              const uint32_t M = buf[a + HP_W_LEN], npw = (M + 15u) >> 4;
              S->ent[n].at = a; S->ent[n].M = M; S->ent[n].cig = a + HP_HDR + npw; S->ent[n].ncig = buf[a + HP_W_NCIG]; S->ent[n].ev0 = 0; S->ent[n].nev = 0;
              if (pool + npw + 2u <= LC_EV_POOL) { S->ent[n].stage = pool; pool += npw + 2u; } else S->ent[n].stage = LC_EV_NONE;
            }
            ++n; a = next;
          }
          S->more = 1; S->n_ent = n; S->g_next = a; S->k = kc & 0xFFFFu; S->n_evt = 0;
        }
      }
    }
    WG_SYNC();
    if (!S->more) break;
    const uint32_t n_ent = S->n_ent, n_list = n_ent < LC_EV_ENTS ? n_ent : LC_EV_ENTS, idx0 = S->g_idx, out0 = S->g_out;
    // ---- its events: counted, summed, listed
    WG_FOR(i, n_list) {
      EvCur c = {0u, 0u, 0u}; EvEvt x; uint32_t n = 0;
      while (ev_next(buf + S->ent[i].cig, S->ent[i].ncig, &c, &x)) ++n;
      S->ent[i].nev = n;
    }
    WG_SYNC();
    WG_FOR(l, LC_SUP_WG) {
      if (l == 0) {
        uint32_t n = 0;
        for (uint32_t i = 0; i < n_list; ++i) { S->ent[i].ev0 = n; n += S->ent[i].nev; }
        S->n_evt = n; S->ok = (n_ent <= LC_EV_ENTS && n <= LC_EV_EVENTS) ? 1u : 0u;
      }
    }
    WG_SYNC();
    if (S->ok) {
      const uint32_t n_evt = S->n_evt;
      WG_FOR(i, n_ent) {
        EvCur c = {0u, 0u, 0u}; EvEvt x; uint32_t j = S->ent[i].ev0;
        while (ev_next(buf + S->ent[i].cig, S->ent[i].ncig, &c, &x)) { x.ent = (uint32_t)i; S->evt[j++] = x; }
      }
      for (uint32_t i = 0; i < n_ent; ++i) {                       // the paths into the pool, a zero word on either side
        const uint32_t st = S->ent[i].stage, npw = (S->ent[i].M + 15u) >> 4, at = S->ent[i].at;
        if (st != LC_EV_NONE) { WG_FOR(j, npw + 2u) S->pool[st + (uint32_t)j] = (j == 0 || (uint32_t)j == npw + 1u) ? 0u : buf[at + HP_HDR + (uint32_t)(j - 1)]; }
      }
      WG_FOR(x, n_evt * EV_COUNTS) S->cnt[x / EV_COUNTS][x % EV_COUNTS] = 0u;
      WG_FOR(x, 2 * LC_SUP_WAVES * LC_EV_ENTS) ((LC_LDS uint32_t *)S->key)[x] = LC_PL_NONE;
      WG_SYNC();
      // ---- how every entry stands to every event, and where
      WG_FOR(x, n_evt * n_ent) {
        const uint32_t ei = (uint32_t)x / n_ent, hi = (uint32_t)x % n_ent;
        const EvEvt E = S->evt[ei];
        const uint32_t ev0 = S->ent[hi].ev0, nev = S->ent[hi].nev;
        LC_GLOBAL const uint32_t *pe = buf + S->ent[E.ent].at + HP_HDR, *ph = buf + S->ent[hi].at + HP_HDR;
        uint32_t lo = E.rb, hi_r = E.rb + E.rs, n_touch = 0;
        int shift = 0, tsum = 0;
        bool same = false;
        for (uint32_t j = 0; j < nev; ++j) {
          const EvEvt X = S->evt[ev0 + j];
          if (X.rb <= E.rb + E.rs && X.rb + X.rs >= E.rb) {        // closed intervals: an insertion at either edge touches
            ++n_touch;
            lo = X.rb < lo ? X.rb : lo; hi_r = X.rb + X.rs > hi_r ? X.rb + X.rs : hi_r;
            tsum += (int)X.ps - (int)X.rs;
            same = X.rb == E.rb && X.rs == E.rs && X.ps == E.ps && E.pb + E.ps <= S->ent[E.ent].M && X.pb + X.ps <= S->ent[hi].M;
            for (uint32_t b = 0; same && b < E.ps; ++b) same = ev_base(pe, E.pb + b) == ev_base(ph, X.pb + b);
          } else if (X.rb + X.rs < E.rb) shift += (int)X.ps - (int)X.rs;      // (wholly in front of the site: the events of an entry lie a '=' column apart)
        }
        const uint32_t cls = n_touch == 0 ? (uint32_t)EV_REF : ((n_touch == 1 && same) ? (uint32_t)EV_ALT : (uint32_t)EV_OTHER);
        S->site[ei * LC_EV_ENTS + hi][0] = ((uint32_t)((int)lo + shift) & 0x3FFFFFFFu) | cls << 30;
        S->site[ei * LC_EV_ENTS + hi][1] = (uint32_t)((int)hi_r + shift + tsum);
      }
      WG_FOR(x, n_evt) { if (out0 + (uint32_t)x < cap) ev_record(out + (size_t)(out0 + (uint32_t)x) * EV_WORDS, idx0 + S->evt[x].ent, S->evt[x], 0u); }
      WG_SYNC();
      // ---- the reads
      const int k = (int)S->k;
      int par = 0;
      for (int r0 = 0; r0 < R && n_evt; r0 += LC_SUP_WAVES, par ^= 1) {
        // every wave its read: on every entry d and the smallest offset that has it
        WG_FOR(l, LC_SUP_WG) {
          const int wv = l >> 6, r = r0 + wv;
          if (r < R) {
            const int t = (int)RI_TLEN(B->rinfo[g0 + (uint32_t)r]);
            LC_GLOBAL const uint32_t *rw = B->bases + B->base_woff[g0 + (uint32_t)r];
            for (uint32_t hi = 0; hi < n_ent; ++hi) {
              const int M = (int)S->ent[hi].M;
              const uint32_t st = S->ent[hi].stage, at = S->ent[hi].at;
              uint32_t m = LC_PL_NONE; int mo = 0;
              if (t >= k && M >= k) {
                for (int o = k - t + (l & 63); o <= M - k; o += 64) {
                  const uint32_t x = st != LC_EV_NONE ? sup_mm_at<true>(rw, t, (LC_LDS const uint32_t *)S->pool + st + 1, M, o) : sup_mm_at<false>(rw, t, buf + at + HP_HDR, M, o);
                  if (x < m) { m = x; mo = o; }                     // (a lane's offsets ascend: the first one is its smallest)
                }
              }
              const uint32_t key = m == LC_PL_NONE ? LC_PL_NONE : ((m < LC_PL_MM_CLAMP ? m : LC_PL_MM_CLAMP) << PL_OFF_BITS) | (uint32_t)(mo + PL_OFF_BIAS);
              bool lead;
              const uint32_t kmin = sup_wave_min(key, &lead);
              if (lead && kmin < S->key[par][wv][hi]) S->key[par][wv][hi] = kmin;
            }
          }
        }
        WG_SYNC_LDS();
        // ... and, the group's smallest d known, every lane of the wave an event
        WG_FOR(l, LC_SUP_WG) {
          const int wv = l >> 6, r = r0 + wv;
          if (r < R) {
            uint32_t best = LC_PL_NONE;
            for (uint32_t hi = 0; hi < n_ent; ++hi) { const uint32_t key = S->key[par][wv][hi]; if (key != LC_PL_NONE && (key >> PL_OFF_BITS) < best) best = key >> PL_OFF_BITS; }
            if (best != LC_PL_NONE && best <= max_mm) {
              const uint32_t ri = B->rinfo[g0 + (uint32_t)r], rc = (RI_NML(ri) ? 2u : 0u) + (RI_REV(ri) ? 1u : 0u);
              const int t = (int)RI_TLEN(ri);
              for (uint32_t ei = (uint32_t)(l & 63); ei < n_evt; ei += 64u) {
                uint32_t on = 0;                                    // bit c: informative on a carrier of class c
                for (uint32_t hi = 0; hi < n_ent; ++hi) {
                  const uint32_t key = S->key[par][wv][hi];
                  if (key == LC_PL_NONE || (key >> PL_OFF_BITS) != best) continue;
                  const int o = (int)(key & PL_OFF_MASK) - PL_OFF_BIAS, M = (int)S->ent[hi].M;
                  const uint32_t s0 = S->site[ei * LC_EV_ENTS + hi][0];
                  const int left = (int)(s0 & 0x3FFFFFFFu), right = (int)S->site[ei * LC_EV_ENTS + hi][1];
                  if (left >= 1 && right + 1 <= M && o <= left - 1 && o + t >= right + 1) on |= 1u << (s0 >> 30);
                }
                if (on) {
                  const uint32_t what = on == (1u << EV_ALT) ? 0u : (on == (1u << EV_REF) ? 1u : 2u);      // alt, ref, other: the record's order
                  dev_atomic_add((LC_LDS uint32_t *)&S->cnt[ei][4u * what + rc], 1u);
                }
              }
            }
          }
          if ((l & 63) < LC_EV_ENTS) S->key[par ^ 1][wv][l & 63] = LC_PL_NONE;      // the other set, for the next walk
        }
        WG_SYNC_LDS();
      }
      WG_SYNC();
      // ---- the counts
      WG_FOR(x, n_evt * EV_COUNTS) {
        const uint32_t ei = (uint32_t)x / EV_COUNTS;
        if (out0 + ei < cap) out[(size_t)(out0 + ei) * EV_WORDS + EV_W_CNT + (uint32_t)x % EV_COUNTS] = S->cnt[ei][(uint32_t)x % EV_COUNTS];
      }
    } else {
      // ---- a group beyond the lists: its events, unevaluated, from the entries in place
      WG_FOR(l, LC_SUP_WG) {
        if (l == 0) {
          uint32_t a = S->g_at, next = 0, n = 0;
          for (uint32_t i = 0; i < n_ent && pl_entry(buf, used, a, &next); ++i, a = next) {
            const uint32_t npw = (buf[a + HP_W_LEN] + 15u) >> 4;
            EvCur c = {0u, 0u, 0u}; EvEvt x;
            while (ev_next(buf + a + HP_HDR + npw, buf[a + HP_W_NCIG], &c, &x)) {
              if (out0 + n < cap) ev_record(out + (size_t)(out0 + n) * EV_WORDS, idx0 + i, x, LANCET_EVID_UNEVALUATED);
              ++n;
            }
          }
          S->n_evt = n;
        }
      }
    }
    WG_SYNC();
    WG_FOR(l, LC_SUP_WG) { if (l == 0) { S->g_at = S->g_next; S->g_idx = idx0 + n_ent; S->g_out = out0 + S->n_evt; } }
    WG_SYNC();
  }
  WG_FOR(l, LC_SUP_WG) { if (l == 0) ev_len[w] = S->g_out; }
}

#ifndef LANCET_WAVE_EMU
// grid: one workgroup per window of the batch
__global__ void __launch_bounds__(LC_SUP_WG) hap_evidence_kernel(const DevBatch *B, const uint32_t *hap_len, const uint32_t *hap_out, uint32_t hcap, uint32_t max_mm,
                                                                 uint32_t *rec, uint32_t *ev_len, uint32_t cap, int n_windows) {
  __shared__ EvShared sh;
  const int w = (int)blockIdx.x;
  if (w >= n_windows) return;
  hap_evidence_window((LC_GLOBAL const DevBatch *)B, (LC_GLOBAL const uint32_t *)hap_len, (LC_GLOBAL const uint32_t *)hap_out, hcap, max_mm, (LC_GLOBAL uint32_t *)rec,
                      (LC_GLOBAL uint32_t *)ev_len, cap, w, (LC_LDS EvShared *)&sh);
}
#endif
