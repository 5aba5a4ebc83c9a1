// host_common.h -- host-side sizing of the HBM work space (shared by engine.hip and the test-side emulator).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "layout.h"
#include "../../include/lancet_engine.h"

static inline uint32_t lc_pow2_ge(uint32_t x) { uint32_t p = 1; while (p < x) p <<= 1; return p; }
static inline uint32_t lc_bucket_cap_for(uint32_t nodes) {
  const uint32_t chain[] = {13u, 29u, 59u, 127u, 257u, 541u, 1109u, 2357u, 5087u, 10273u, 20753u, 42043u,
                            85229u, 172933u, 351061u, 712697u, 1447153u, 2938679u};
  for (int i = 0; i < 18; ++i) if (chain[i] >= nodes + 2) return chain[i] + 1;
  return 2938680u;
}

// Layout of one hand-off area of the LDS build kernel (layout.h PreLayout): `ncap` distinct k-mers, `qvcap` (candidate, position)
// quality rows, `kw` words per candidate key.
static inline PreLayout lc_pre_layout(uint32_t ncap, uint32_t qvcap, uint32_t kw, uint32_t maxw = LC_MAXW_DEFAULT, uint32_t lrcap = 0) {
  PreLayout L; memset(&L, 0, sizeof(L));
  L.ncap = ncap; L.qvcap = qvcap; L.kw = kw; L.maxw = maxw;
  uint32_t o = PRE_OFF_OCCREF + 4u * maxw;
  auto take = [&](uint32_t bytes, uint32_t align) { o = (o + align - 1u) & ~(align - 1u); const uint32_t at = o; o += bytes; return at; };
  L.refcov = take(8u * maxw, 64u);
  L.nhash = take(8u * ncap, 64u); L.surv = take(ncap, 64u);
  L.snode = take(4u * PB_CCAP, 64u); L.skey = take(8u * kw * PB_CCAP, 64u); L.sid = take(4u * PB_SCAP, 64u);
  L.pgr = take(128u * PB_SCAP, 128u); L.order = take(4u * PB_SCAP, 64u); L.qv = take(8u * qvcap, 64u);
  L.chdr = take(64u, 64u); L.clive = take(4u * (PB_CMAX + 2u), 64u); L.cseq = take(4u * PB_CSEQ, 64u);
  L.cord = take(8u * PB_CMAX, 64u); L.chl = take(12u * PB_CHEADS, 64u);
  if (lrcap) { L.lrnocc = take(4u * (ncap + 2u), 64u); L.lrcsr = take(4u * lrcap, 64u); L.lrcap = lrcap; }      // --linked-reads
  L.stride = (o + 255u) & ~255u;
  return L;
}
// Which form a batch gets: the wide one (PB_NCAP_WIDE k-mers, keys of 4 words, PB_QVCAP_WIDE rows: windows of 100x / 40x build at
// k = 31..101 with 9-12 k distinct k-mers) when its windows are deep (more than 400 reads on average: 60x / 60x windows, ~360 reads, all fit the narrow form) and `n_areas` of them stay
// within `budget` bytes; else the narrow one.  LANCET_PRE_WIDE=0 / 1 forces either (read by the caller, passed as `force`).
// What the sizing below needs of a batch: per window its reads, the untrimmed bases of its reads and its reference length.  A host batch
// has them in read_begin / seq_off / ref_off (lc_sizes_of_batch); the device read selection has them from its per-window summaries.
struct LcBatchSizes { int n_windows; const uint32_t *read_begin, *ref_off, *wbases; uint64_t total_bases; };
static inline LcBatchSizes lc_sizes_of_batch(const lancet_window_batch *b, std::vector<uint32_t> *wbases) {
  const int nw = b->n_windows > 0 ? b->n_windows : 0;
  wbases->resize((size_t)nw);
  for (int w = 0; w < nw; ++w) (*wbases)[(size_t)w] = b->seq_off[b->read_begin[w + 1]] - b->seq_off[b->read_begin[w]];
  return LcBatchSizes{b->n_windows, b->read_begin, b->ref_off, wbases->data(), nw ? (uint64_t)b->seq_off[b->read_begin[nw]] : 0ull};
}
static inline uint32_t lc_max_w_for_sizes(const LcBatchSizes &b) {      // EngineCaps::max_w
  uint32_t m = LC_MAXW_DEFAULT;
  for (int w = 0; w < b.n_windows; ++w) { const uint32_t l = b.ref_off[w + 1] - b.ref_off[w]; if (l > m && l <= LC_MAXW) m = l; }
  m = (m + 63u) & ~63u;
  return m > LC_MAXW ? (uint32_t)LC_MAXW : m;
}
static inline uint32_t lc_max_w_for_batch(const lancet_window_batch *b) { std::vector<uint32_t> wb; return lc_max_w_for_sizes(lc_sizes_of_batch(b, &wb)); }
static inline PreLayout lc_pre_layout_for_sizes(const LcBatchSizes &b, size_t n_areas, size_t budget, int force = -1, bool lr = false) {
  const uint32_t mw = lc_max_w_for_sizes(b);
  const PreLayout narrow = lc_pre_layout(PB_NCAP, PB_QVCAP, 1u, mw, lr ? PB_LRCAP : 0u), wide = lc_pre_layout(PB_NCAP_WIDE, PB_QVCAP_WIDE, LC_NWMAX, mw, lr ? PB_LRCAP_WIDE : 0u);
  if (force == 0 || b.n_windows <= 0) return narrow;
  if (force == 1) return wide;
  const uint32_t R = b.read_begin[b.n_windows];
  const bool deep = R / (uint32_t)b.n_windows > 400u;
  return (deep && n_areas * (size_t)wide.stride <= budget) ? wide : narrow;
}
static inline PreLayout lc_pre_layout_for_batch(const lancet_window_batch *b, size_t n_areas, size_t budget, int force = -1, bool lr = false) {
  std::vector<uint32_t> wb; return lc_pre_layout_for_sizes(lc_sizes_of_batch(b, &wb), n_areas, budget, force, lr);
}

// Test hook (engine.hip lancet_debug_pre_order and its twin in tests/emu/emu_engine.cc): what ONE hand-off area -- a host copy of it -- says
// about the table order, appended to `out`:
//   K, status, N, nsurv, have_order, ht_bc, ht_next_resize, numcomp, refcomp, big, PreCmp::done, m_live, settled (13 words)
//   with have_order, per table position i < nsurv: nhash[order[i]] (low, high word), the comp of that survivor's record
//   with done, per position i < m_live of CLIVE: the hash of the node there (low, high; a special node's is PreCmp::spec_hash)
// Returns PreHdr::next (0: the last graph of the window's chain), -1 when an index in the area points outside its array.
static inline int lc_pre_order_words(const uint8_t *area, const PreLayout &pl, std::vector<uint32_t> *out) {
  const PreHdr *H = (const PreHdr *)(area + PRE_OFF_HDR);
  const PreCmp *CH = (const PreCmp *)(area + pl.chdr);
  const bool built = H->status == PB_BUILT, ord = built && H->have_order == 1u, done = ord && CH->done == 1u;
  const uint32_t hdr[13] = {(uint32_t)H->K, H->status, built ? H->N : 0u, built ? H->nsurv : 0u, ord ? 1u : 0u, ord ? H->ht_bc : 0u, ord ? H->ht_next_resize : 0u,
                            ord ? H->numcomp : 0u, ord ? H->refcomp : 0u, built ? H->big : 0u, done ? 1u : 0u, done ? CH->m_live : 0u, (built && H->settled == 1u) ? 1u : 0u};
  out->insert(out->end(), hdr, hdr + 13);
  if (!ord) return (int)H->next;
  const unsigned long long *nhash = (const unsigned long long *)(area + pl.nhash);
  const uint32_t *sid = (const uint32_t *)(area + pl.sid), *order = (const uint32_t *)(area + pl.order), *clive = (const uint32_t *)(area + pl.clive);
  const NodeGr *pgr = (const NodeGr *)(area + pl.pgr);
  const uint32_t nsurv = H->nsurv;
  if (nsurv > PB_SCAP || H->N > pl.ncap) return -1;
  std::vector<uint32_t> si_of(H->N, LC_NIL);
  for (uint32_t si = 0; si < nsurv; ++si) { if (sid[si] >= H->N) return -1; si_of[sid[si]] = si; }
  for (uint32_t i = 0; i < nsurv; ++i) {
    const uint32_t n = order[i];
    if (n >= H->N || si_of[n] == LC_NIL) return -1;
    out->push_back((uint32_t)nhash[n]); out->push_back((uint32_t)(nhash[n] >> 32)); out->push_back((uint32_t)pgr[si_of[n]].comp);
  }
  if (!done) return (int)H->next;
  if (CH->m_live > PB_CMAX + 2u) return -1;
  for (uint32_t i = 0; i < CH->m_live; ++i) {
    const uint32_t idx = clive[i];
    unsigned long long h;
    if (idx & 0x80000000u) { if ((idx & 0xFFu) > 1u) return -1; h = CH->spec_hash[idx & 0xFFu]; }
    else { if (idx >= nsurv) return -1; h = nhash[sid[idx]]; }
    out->push_back((uint32_t)h); out->push_back((uint32_t)(h >> 32));
  }
  return (int)H->next;
}

// Node limit of the re-run tier: `limit` (65 536 unless LANCET_MAX_NODES says otherwise), 2^20 when `grow` and a window has 65 535 reads or more.
static inline uint32_t lc_tier2_nodes_for_sizes(const LcBatchSizes &b, uint32_t limit, bool grow) {
  if (grow) for (int w = 0; w < b.n_windows; ++w) if (b.read_begin[w + 1] - b.read_begin[w] >= 0xFFFFu) return limit > (1u << 20) ? limit : (1u << 20);
  return limit;
}
static inline uint32_t lc_tier2_nodes_for_batch(const lancet_window_batch *b, uint32_t limit, bool grow) {
  std::vector<uint32_t> wb; return lc_tier2_nodes_for_sizes(lc_sizes_of_batch(b, &wb), limit, grow);
}
// Work-space caps for a batch: the largest window decides.
// tier 1 = the common case (small tables: cheap to clear, cache/TLB friendly); tier 2 = worst case for the window
// shapes in the batch, used to re-run the windows that overflowed tier 1.
static inline EngineCaps lc_caps_for_sizes(const LcBatchSizes &bs, const lancet_params *p, uint32_t evt_cap,
                                           uint32_t max_nodes_limit, int tier = 2) {
  const LcBatchSizes *b = &bs;
  EngineCaps c; memset(&c, 0, sizeof(c));
  uint32_t max_reads = 0; uint64_t max_bases = 0;
  for (int w = 0; w < b->n_windows; ++w) {
    uint32_t r0 = b->read_begin[w], r1 = b->read_begin[w + 1];
    if (r1 - r0 > max_reads) max_reads = r1 - r0;
    uint64_t bases = (uint64_t)b->wbases[w] + (b->ref_off[w + 1] - b->ref_off[w]);
    if (bases > max_bases) max_bases = bases;
  }
  if (tier == 1 && b->n_windows > 0) {
    // coverage pile-ups: a window far above the batch's typical size would size every slot's work space; tier 1 is laid
    // out for windows up to 4x the mean (they overflow at once and run in tier 2, whose limits are the true maxima)
    const uint32_t R = b->read_begin[b->n_windows];
    const uint64_t mean_reads = R / (uint32_t)b->n_windows, mean_bases = (b->total_bases + b->ref_off[b->n_windows]) / (uint64_t)b->n_windows;
    // (round 5: bases 2x the mean + 16 Ki instead of 4x + 32 Ki -- the occurrence-sized arrays are a third of a slot, and what lies between
    //  is a handful of windows per scan that run in the re-run tier like the pile-ups above them)
    const uint64_t lim_reads = 4 * mean_reads + 256, lim_bases = 2 * mean_bases + 16384;
    if (max_reads > lim_reads) max_reads = (uint32_t)lim_reads;
    if (max_bases > lim_bases) max_bases = lim_bases;
  }
  c.reads_cap = max_reads + 2;
  c.occ_cap = (uint32_t)max_bases + 64;           // every base starts at most one k-mer
  uint32_t nodes = c.occ_cap;
  if (nodes > max_nodes_limit) nodes = max_nodes_limit;
  c.node_cap = nodes;
  c.table_cap = lc_pow2_ge(2 * nodes);
  // The flagged occurrences of the mate-overlap replay share todo[] with the slot -> node table.  Tier 1 keeps that size (its windows re-run
  // when the list fills up); the re-run tier holds one entry per occurrence: a short-insert library at a few hundred x flags more
  // occurrences than a 65 536-node window has slots (8 windows of ~3 200 overlapping 150-base reads: 165 k of 400 k).
  c.todo_cap = tier == 1 || c.occ_cap < c.table_cap ? c.table_cap : c.occ_cap;
  c.bucket_cap = lc_bucket_cap_for(nodes);
  c.special_cap = tier == 1 ? 64u : 4096u;     /* source + sink per component that touches the reference, per build */
  uint32_t maxk = (uint32_t)(p->max_k > 0 ? p->max_k : 101);
  c.max_k = maxk;
  if (tier == 1) {
    c.surv_cap = nodes < 4096 ? nodes : 4096;
    c.qv_cap = 4096u * 32u;                    // (survivor, position) entries: 4096 survivors at k<=32, 1297 at k=101
    c.queue_cap = 8192;
  } else {
    c.surv_cap = nodes;                        // every node may survive (--low-cov 0 on noisy reads: fuzz case 10083, 17 k survivors of 17.4 k nodes)
    c.qv_cap = c.surv_cap * maxk;
    // Graph_t::bfs keeps whole partial paths in its FIFO until DFS_LIMIT dequeues (reference src/Graph.cc:1299-1425); every
    // dequeue enqueues at most the node's out-degree (a few after compaction).  The worst-case tier holds 4 entries per
    // permitted dequeue, capped at 4 Mi entries (96 MB per slot); beyond that the window reports an overflow.
    { uint64_t q = 4ull * (uint64_t)(p->dfs_limit > 0 ? p->dfs_limit : 1000000) + 4096; if (q < 65536) q = 65536; if (q > (4ull << 20)) q = 4ull << 20; c.queue_cap = (uint32_t)q; }
  }
  c.seq_cap = 3 * c.qv_cap + 65536;
  c.max_w = lc_max_w_for_sizes(bs);              // (a window above LC_MAXW is reported LANCET_W_OVERFLOW on its own)
  c.path_cap = c.max_w + (uint32_t)p->max_indel_len + 256;
  c.evt_cap = evt_cap;
  // trace level: 1 = -v; 2 = -V as well (the engine sets it from lancet_engine_set_trace_level; LANCET_TRACE_LEVEL=2 in the environment is how the
  // host emulation of the kernels is told, as it is told LANCET_NO_PREBUILD -- level 2 needs at least 16 words per window, see kernels.h evt_truncate)
  c.evt_level = evt_cap ? 1u : 0u;
  if (evt_cap >= 16u) { const char *lv = getenv("LANCET_TRACE_LEVEL"); if (lv && atoi(lv) == 2) c.evt_level = 2u; }
  // Records of the whole batch.  A scan emits ~0.7 per window; permissive settings (--low-cov 0 on noisy reads) reach several
  // hundred per window (fuzz case 7122: 355), and a small batch has no other windows to average that out: 64 per window and
  // a floor of 64 Ki records (lancet_variant is 64 bytes: 140 MB for a 32768-window batch).
  c.var_cap = (uint32_t)b->n_windows * 64u + 65536u;
  c.blob_cap = (uint32_t)b->n_windows * 4096u + (4u << 20);
  c.lr_mode = p->lr_mode ? 1u : 0u;
  c.bx_cap = c.lr_mode ? (uint32_t)b->n_windows * 8192u + (1u << 20) : 0u;
  c.pl = lc_pre_layout(PB_NCAP, PB_QVCAP, 1u, c.max_w);      // (the engine replaces it per upload: lc_pre_layout_for_batch)
#ifdef LANCET_WAVE_EMU
  c.hap_cap = lc_emu_hap_sink.cap;                            // (the engine sets it from lancet_engine_set_haplotypes)
  c.hap_aln = lc_emu_hap_sink.cap ? lc_emu_hap_sink.aln : 0u; // (... and from lancet_engine_set_haplotype_alignments)
  c.hap_cov = lc_emu_hap_sink.cap ? lc_emu_hap_sink.cov : 0u; // (... and from lancet_engine_set_haplotype_coverage)
  c.hap_sup = lc_emu_hap_sink.cap ? lc_emu_hap_sink.sup : 0u; // (... and from lancet_engine_set_haplotype_support)
  // settled windows: off unless the emulation is told otherwise, and then by the engine's rule (engine.hip lc_upload_caps: no trace, no capture, no linked reads)
  { const char *sv = getenv("LANCET_EMU_SETTLE"); const char *co = getenv("LANCET_SETTLE_CHAIN_ONLY");
    c.settle = (sv && atoi(sv) == 1 && !evt_cap && !c.hap_cap && !c.lr_mode) ? ((co && atoi(co) != 0) ? 2u : 1u) : 0u; }
#endif
  return c;
}

// ---- haplotype capture (layout.h HP_*): what the window kernels left in the windows' buffers, as lancet_engine_results_haplotypes returns it.
// Smallest buffer lancet_engine_set_haplotypes accepts: one header and one word of bases.
#define LC_HAP_MIN_WORDS (HP_HDR + 1u)
// Words of window w that hold closed entries, from its length word: none for a window that reports no result (status < 0).
static inline uint32_t lc_hap_used(uint32_t len_word, uint32_t cap, int32_t status) {
  const uint32_t u = len_word & ~HP_TRUNC;
  return status < 0 ? 0u : (u < cap ? u : cap);
}
// cigar_off / cigar: lancet_engine_results_haplotype_alignments -- haplotype i's CIGAR words are cigar[cigar_off[i] .. cigar_off[i + 1]) (none without EngineCaps::hap_aln)
// cov_off / cov: lancet_engine_results_haplotype_coverage -- haplotype i's 16-bit counts are cov[cov_off[i] .. cov_off[i + 1]): 4 per path base, then 4 per
// base of the stretch (none without EngineCaps::hap_cov)
struct LcHapResult { std::vector<lancet_haplotype> h; std::vector<uint32_t> words; std::vector<uint8_t> truncated; std::vector<uint32_t> cigar_off{0u}, cigar;
                     std::vector<uint32_t> cov_off{0u}; std::vector<uint16_t> cov;
                     std::vector<uint32_t> sup; /* lancet_engine_results_haplotype_support: 8 per haplotype (fit Tf Tr Nf Nr, alone Tf Tr Nf Nr), none without EngineCaps::hap_sup */ };
// len_word[w]: DevOut::hap_len as the run left it; dense: the used words of the windows one behind the other (window w's start at off[w],
// off[w + 1] - off[w] == lc_hap_used of it).
static inline void lc_hap_collect(int n_windows, const uint32_t *len_word, const uint32_t *off, const uint32_t *dense, const lancet_window_stats *stats, LcHapResult *r) {
  r->h.clear(); r->words.clear(); r->truncated.assign((size_t)(n_windows > 0 ? n_windows : 0), 0);
  r->cigar_off.assign(1, 0u); r->cigar.clear();
  r->cov_off.assign(1, 0u); r->cov.clear(); r->sup.clear();
  for (int w = 0; w < n_windows; ++w) {
    if (stats[w].status < 0) continue;
    r->truncated[(size_t)w] = (len_word[w] & HP_TRUNC) ? 1 : 0;
    const uint32_t *p = dense + off[w]; const uint32_t used = off[w + 1] - off[w];
    int32_t idx = 0;
    for (uint32_t at = 0; at + HP_HDR <= used;) {
      const uint32_t *e = p + at; const uint32_t nw = (e[HP_W_LEN] + 15u) / 16u;
      if (nw > used - at - HP_HDR) break;                     // (never: hap_close counts whole entries)
      const uint32_t nc = e[HP_W_NCIG];                       // the CIGAR words behind the path words: stepped over, kept apart from `words`
      if (nc > used - at - HP_HDR - nw) break;
      // ... and the coverage words behind those (LANCET_HAP_HAS_COVERAGE): two per base of path and stretch, each a pair of 16-bit counts, low half first
      const uint32_t nv = (e[HP_W_FLAGS] & LANCET_HAP_HAS_COVERAGE) ? 2u * (e[HP_W_LEN] + e[HP_W_REFLEN]) : 0u;
      if (nv > used - at - HP_HDR - nw - nc) break;
      // ... and the eight support words behind those (LANCET_HAP_HAS_SUPPORT)
      const uint32_t ns = (e[HP_W_FLAGS] & LANCET_HAP_HAS_SUPPORT) ? HP_SUP_WORDS : 0u;
      if (ns > used - at - HP_HDR - nw - nc - nv) break;
      lancet_haplotype x; memset(&x, 0, sizeof(x));
      x.window = w; x.index_in_window = idx++; x.kmer = (uint16_t)(e[HP_W_KC] & 0xFFFFu); x.component = (uint16_t)(e[HP_W_KC] >> 16);
      x.ref_off = e[HP_W_REFOFF]; x.ref_len = e[HP_W_REFLEN]; x.len = e[HP_W_LEN]; x.word_off = (uint32_t)r->words.size();
      x.first_variant = (int32_t)e[HP_W_FIRST]; x.n_variants = (int32_t)e[HP_W_NVAR]; x.flags = e[HP_W_FLAGS];
      r->words.insert(r->words.end(), e + HP_HDR, e + HP_HDR + nw);
      r->cigar.insert(r->cigar.end(), e + HP_HDR + nw, e + HP_HDR + nw + nc);
      r->cigar_off.push_back((uint32_t)r->cigar.size());
      if (nv) { const size_t o = r->cov.size(); r->cov.resize(o + 2u * (size_t)nv); memcpy(r->cov.data() + o, e + HP_HDR + nw + nc, sizeof(uint32_t) * (size_t)nv); }      // (little-endian host: a word is its two counts in order)
      r->cov_off.push_back((uint32_t)r->cov.size());
      r->sup.insert(r->sup.end(), e + HP_HDR + nw + nc + nv, e + HP_HDR + nw + nc + nv + ns);
      r->h.push_back(x);
      at += HP_HDR + nw + nc + nv + ns;
    }
  }
}
// ---- read placements (layout.h PL_*): the placement kernel's records as lancet_engine_results_haplotype_placements returns them.
// Limits lancet_engine_set_haplotype_placements checks: entries a window's buffer may hold against the index field, the longest path
// against the offset field.
static inline bool lc_place_words_ok(uint32_t words_per_window) { return words_per_window / LC_HAP_MIN_WORDS <= PL_IDX_MAX; }
static inline bool lc_place_params_ok(const lancet_params *p) { return p->max_indel_len >= 0 && (int64_t)LC_MAXW + p->max_indel_len + 256 < (int64_t)PL_OFF_BIAS; }
struct LcPlaceResult { std::vector<lancet_read_placement> p; std::vector<uint32_t> read_begin; std::vector<uint16_t> tlen; };
// read_begin: [n_windows + 1]; rinfo: [reads] DevBatch::rinfo; rec: [reads * PL_WORDS] as the kernel left them.  A window without a result
// (status < 0) has no placed read, whatever its buffer held.
static inline void lc_place_collect(int n_windows, const uint32_t *read_begin, const uint32_t *rinfo, const uint32_t *rec, const lancet_window_stats *stats, LcPlaceResult *r) {
  const int nw = n_windows > 0 ? n_windows : 0;
  const uint32_t R = nw ? read_begin[nw] : 0u;
  lancet_read_placement none; memset(&none, 0, sizeof(none)); none.haplotype = -1;
  r->p.assign((size_t)R, none); r->read_begin.assign(read_begin, read_begin + (nw ? nw + 1 : 0)); r->tlen.resize((size_t)R);
  if (!nw) r->read_begin.assign(1, 0u);
  for (uint32_t i = 0; i < R; ++i) r->tlen[i] = (uint16_t)RI_TLEN(rinfo[i]);
  for (int w = 0; w < nw; ++w) {
    if (stats[w].status < 0) continue;
    for (uint32_t i = read_begin[w]; i < read_begin[w + 1]; ++i) {
      const uint32_t w0 = rec[PL_WORDS * (size_t)i], w1 = rec[PL_WORDS * (size_t)i + 1];
      if (!(w0 & PL_IDX_MAX)) continue;
      lancet_read_placement &x = r->p[i];
      x.haplotype = (int32_t)(w0 & PL_IDX_MAX) - 1;
      x.mismatches = (uint16_t)(w0 >> PL_MM_SHIFT);
      x.offset = (int32_t)((w1 & PL_OFF_MASK) << (32 - PL_OFF_BITS)) >> (32 - PL_OFF_BITS);      // (two's complement in PL_OFF_BITS bits)
      x.n_offsets = (uint16_t)((w1 >> PL_NOFF_SHIFT) & PL_CNT_MAX);
      x.n_haplotypes = (uint16_t)((w1 >> PL_NHAP_SHIFT) & PL_CNT_MAX);
      x.cls = (uint16_t)((RI_NML(rinfo[i]) ? 2u : 0u) + (RI_REV(rinfo[i]) ? 1u : 0u));
    }
  }
}

// The alignment of a placed read on the window reference, through its haplotype's alignment: the one statement of the rule, for lancet_gpu
// and the tests (lancet_amd/abi.py read_cigar restates it in Python, written apart from this).
//   o, t: the placement's offset and the read's trimmed length; M, ref_off, cig[ncig]: the entry's length, stretch offset and CIGAR words
//   (length << 4 | HP_OP_*; none: the path lies on its stretch base for base).
// Read bases in front of path position 0 or behind M - 1 are S.  Over the path positions [max(0, o), min(M, o + t)) the entry's runs are
// walked: columns of = and X become M (the read may differ from the path), I stays I, D stays D unless no kept column lies in front of it or
// behind it.  *start: 0-based on the window reference, the stretch offset plus the reference columns in front of the first kept column.
// Neighbouring equal ops merge.  out: length << 4 | BAM op (LC_RC_*).  Returns false for a read without an M -- one that lies wholly inside
// an I run: *start is then the column behind the run.
enum { LC_RC_M = 0, LC_RC_I = 1, LC_RC_D = 2, LC_RC_S = 4 };
static inline bool lc_read_cigar(int32_t o, uint32_t t, uint32_t M, uint32_t ref_off, const uint32_t *cig, uint32_t ncig, uint32_t *start, std::vector<uint32_t> *out) {
  out->clear();
  const int64_t a = o > 0 ? o : 0, b = std::min<int64_t>((int64_t)M, (int64_t)o + (int64_t)t);
  auto push = [&](uint32_t n, uint32_t op) { if (!n) return; if (!out->empty() && (out->back() & 15u) == op) out->back() += n << 4; else out->push_back(n << 4 | op); };
  const uint32_t whole = M << 4 | (uint32_t)HP_OP_EQ;
  if (!ncig) { cig = &whole; ncig = 1; }
  *start = ref_off;
  if (b <= a) { push(t, LC_RC_S); return false; }       // (no placement: nothing of the read lies on the path)
  push((uint32_t)(a - (int64_t)o), LC_RC_S);
  int64_t pp = 0, rc = 0, pend_d = 0;          // path position and stretch column in front of the run at hand; a D run waiting for a kept column behind it
  bool kept = false, has_m = false;
  for (uint32_t q = 0; q < ncig && pp < b; ++q) {
    const int64_t L = (int64_t)(cig[q] >> 4); const uint32_t op = cig[q] & 15u;
    if (op == (uint32_t)HP_OP_D) { if (kept) pend_d += L; rc += L; continue; }
    const int64_t x0 = std::max(pp, a), x1 = std::min(pp + L, b);
    if (x1 > x0) {
      const bool m = op != (uint32_t)HP_OP_I;
      if (!kept) { *start = ref_off + (uint32_t)(rc + (m ? x0 - pp : 0)); kept = true; }
      if (pend_d) { push((uint32_t)pend_d, LC_RC_D); pend_d = 0; }
      push((uint32_t)(x1 - x0), m ? LC_RC_M : LC_RC_I);
      has_m = has_m || m;
    }
    pp += L; if (op != (uint32_t)HP_OP_I) rc += L;
  }
  if (!kept) *start = ref_off + (uint32_t)rc;
  push((uint32_t)((int64_t)o + (int64_t)t - b), LC_RC_S);
  return has_m;
}
// ---- variant evidence (layout.h EV_*): the evidence kernel's records as lancet_engine_results_haplotype_evidence returns them.
#define LC_EVID_CAP_MAX ((1u << 24) - 1u)      /* events_per_window lancet_engine_set_haplotype_evidence accepts */
struct LcEvidResult { std::vector<lancet_variant_evidence> ev; std::vector<uint32_t> event_off{0u}; std::vector<uint8_t> marked; };
// Records of window w that are kept, from its event count: none for a window that reports no result (status < 0).
static inline uint32_t lc_evid_used(uint32_t n_events, uint32_t cap, int32_t status) { return status < 0 ? 0u : (n_events < cap ? n_events : cap); }
// The record an event of haplotype h emitted: the one statement of the rule, for the engine, lancet_gpu and the tests (lancet_amd/abi.py
// evidence_variant restates it in Python, written apart from this).  The transcript walk (kernels.h walk_column) opens a transcript at the
// event's first column with t.pos = pos_in_ref + ref_start + trim5 -- pos_in_ref the stretch bases in front of the column, the event's rb;
// trim5 the stretch's offset, the haplotype's ref_off -- and the record's pos is t.pos - 1.  v[v0 .. v1): the window's records.
static inline int32_t lc_evid_join(const lancet_haplotype &h, uint32_t rb, int32_t ref_start, const lancet_variant *v, size_t v0, size_t v1) {
  for (size_t i = v0; i < v1; ++i) {
    if (v[i].seq_in_window < h.first_variant || v[i].seq_in_window >= h.first_variant + h.n_variants) continue;
    if ((int64_t)v[i].pos + 1 - (int64_t)ref_start - (int64_t)h.ref_off == (int64_t)rb) return (int32_t)i;
  }
  return -1;
}
// ev_len: [n_windows] the events every window has; dense: the kept records of the windows one behind the other (window w's start at record
// off[w], off[w + 1] - off[w] == lc_evid_used of it); haps: lc_hap_collect's, of the same run; v[nv]: the run's records, ordered by
// (window, seq_in_window); ref_start: [n_windows] DevBatch::ref_start.
static inline void lc_evid_collect(int n_windows, const uint32_t *ev_len, const uint32_t *off, const uint32_t *dense, uint32_t cap, const lancet_window_stats *stats,
                                   const int32_t *ref_start, const std::vector<lancet_haplotype> &haps, const lancet_variant *v, size_t nv, LcEvidResult *r) {
  r->ev.clear(); r->event_off.assign(1, 0u); r->marked.assign((size_t)(n_windows > 0 ? n_windows : 0), 0);
  for (int w = 0; w < n_windows; ++w) r->marked[(size_t)w] = (stats[w].status >= 0 && ev_len[w] > cap) ? 1 : 0;
  int cur_w = -1; uint32_t c = 0, c_end = 0; size_t v0 = 0, v1 = 0;
  for (size_t i = 0; i < haps.size(); ++i) {
    const lancet_haplotype &h = haps[i];
    if (h.window != cur_w) {
      cur_w = h.window; c = off[cur_w]; c_end = off[cur_w + 1];
      while (v0 < nv && v[v0].window < cur_w) ++v0;
      v1 = v0; while (v1 < nv && v[v1].window == cur_w) ++v1;
    }
    for (; c < c_end && dense[(size_t)c * EV_WORDS + EV_W_IDX] == (uint32_t)h.index_in_window; ++c) {
      const uint32_t *q = dense + (size_t)c * EV_WORDS;
      lancet_variant_evidence x; memset(&x, 0, sizeof(x));
      x.haplotype = (int32_t)i; x.rb = q[EV_W_RB]; x.rs = q[EV_W_RS]; x.pb = q[EV_W_PB]; x.ps = q[EV_W_PS]; x.flags = q[EV_W_FLAGS];
      for (int j = 0; j < 4; ++j) { x.alt[j] = q[EV_W_CNT + j]; x.ref[j] = q[EV_W_CNT + 4 + j]; x.other[j] = q[EV_W_CNT + 8 + j]; }
      x.variant = lc_evid_join(h, x.rb, ref_start[cur_w], v, v0, v1);
      r->ev.push_back(x);
    }
    r->event_off.push_back((uint32_t)r->ev.size());
  }
}
static inline EngineCaps lc_caps_for_batch(const lancet_window_batch *b, const lancet_params *p, uint32_t evt_cap,
                                           uint32_t max_nodes_limit, int tier = 2) {
  std::vector<uint32_t> wb; return lc_caps_for_sizes(lc_sizes_of_batch(b, &wb), p, evt_cap, max_nodes_limit, tier);
}

struct LcCarver {
  char *base; size_t off;
  template <class T> LC_GLOBAL T *take(size_t n) {
    off = (off + 63) & ~(size_t)63;
    LC_GLOBAL T *p = base ? (LC_GLOBAL T *)(base + off) : (LC_GLOBAL T *)nullptr;
    off += n * sizeof(T);
    return p;
  }
};

// Lays one Work slot out at `base` (may be null to just measure).  Returns bytes used.
static inline size_t lc_work_carve(Work *w, char *base, const EngineCaps &c) {
  LcCarver k{base, 0};
  const size_t nodes = (size_t)c.node_cap + c.special_cap;
  const size_t MW = c.max_w ? c.max_w : LC_MAXW_DEFAULT;
  Work t; memset(&t, 0, sizeof(t));
  t.occ_base = k.take<uint32_t>(c.reads_cap + 1);
  t.rd = k.take<uint32_t>(4 * (size_t)c.reads_cap);
  t.cand = k.take<uint8_t>(c.reads_cap);
  t.mate_of = k.take<uint32_t>(c.reads_cap);
  t.items = k.take<uint32_t>(2 * ((size_t)c.reads_cap + MW / LC_SEG + 2));
  t.chunk = k.take<uint32_t>(2 * (((size_t)c.reads_cap + MW / LC_SEG + 2) / 64 + 2));
  t.occ = k.take<uint32_t>(c.occ_cap);
  t.slots = k.take<uint32_t>(4 * (size_t)c.table_cap);
  t.todo = k.take<uint32_t>(c.todo_cap > c.table_cap ? c.todo_cap : c.table_cap);
  t.mv = k.take<uint32_t>((c.wide_ids ? 8 : 4) * (size_t)c.occ_cap);
  t.slot_key = k.take<unsigned long long>((size_t)c.table_cap * LC_NWMAX);
  t.bitmap = k.take<uint32_t>((c.occ_cap + c.special_cap) / 32 + 4);   /* also the visited set of the component search (node ids) */
  t.bitpre = k.take<uint32_t>(c.occ_cap / 32 + 2);
  t.csr = k.take<uint32_t>((c.wide_ids ? 2 : 1) * (size_t)c.occ_cap);
  t.nkey = k.take<unsigned long long>(nodes * LC_NWMAX);
  t.nhash = k.take<unsigned long long>(nodes);
  t.nfill = k.take<uint32_t>((c.wide_ids ? 2 : 1) * (nodes + 1));
  t.gr = k.take<NodeGr>(nodes + 1);          /* + the stand-in record of reference k-mers whose node is gone (prebuilt windows) */
  t.cmp = k.take<CmpRec>(nodes);
  t.nocc = k.take<uint32_t>(nodes + 1);
  t.qv = k.take<uint16_t>((size_t)c.qv_cap * (c.lr_mode ? 10 : 4));
  t.qv_own = t.qv;
  t.khp = k.take<uint16_t>(c.lr_mode ? nodes * 6 : 1);
  t.refhp = k.take<uint16_t>(c.lr_mode ? MW * 6 : 1);
  t.bxbuf = k.take<uint32_t>(c.lr_mode ? c.reads_cap : 1);
  t.lr_refnode = k.take<uint32_t>(c.lr_mode ? MW : 1);
  t.seq = k.take<uint32_t>(c.seq_cap);
  t.ht_next = k.take<uint32_t>(nodes);
  t.ht_bucket = k.take<uint32_t>(c.bucket_cap);
  t.ht_cnt = k.take<uint32_t>(c.bucket_cap);
  t.ht_start = k.take<uint32_t>(c.bucket_cap);
  t.order = k.take<uint32_t>(nodes + 1);
  t.scratch = k.take<uint32_t>(2 * nodes > c.occ_cap ? 2 * nodes : c.occ_cap);
  t.refcov = k.take<uint16_t>(MW * 4);
  t.queue = k.take<BfsEntry>(c.queue_cap);
  t.pnodes = k.take<uint32_t>(nodes); t.pedges = k.take<uint32_t>(nodes);
  t.pdesc = k.take<uint32_t>(c.path_cap);
  t.pseq = k.take<uint8_t>(c.path_cap);
  t.tb = k.take<uint8_t>((size_t)(MW + c.path_cap + 4) * (MW + 2));   /* anti-diagonal-major: (n+m+1) diagonals of n+1 cells */
  t.dp = k.take<int32_t>(7 * (MW + 2));
  t.aln = k.take<uint8_t>(2 * (size_t)(MW + c.path_cap + 2));
  t.evt = k.take<uint32_t>(c.evt_cap + 8);
  t.survb = k.take<uint8_t>(nodes + 1);
  if (w) *w = t;
  return (k.off + 255) & ~(size_t)255;
}
