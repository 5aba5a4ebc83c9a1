/* lancet_engine.h -- C-ABI of the MI355X micro-assembly engine (drop-in for Lancet's per-window hot path).
 *
 * The reference has no plugin / FFI interface.  The seam this library sits behind is the
 * C++ member call
 *      numreads = processGraph(g, graphref, minK, maxK);          reference src/Microassembler.cc:837
 *                                                        (declared reference src/Microassembler.hh:224)
 * whose inputs are, at that point, fully materialised:
 *      g.readid2info  -- reads filled by Graph_t::addAlignment     reference src/Graph.cc:487-501
 *                        (fields: reference src/ReadInfo.hh:44-67)
 *      Ref_t          -- window reference string + coordinates     reference src/Ref.hh:55-97
 *      knobs          -- Graph_t setters                           reference src/Microassembler.cc:726-753
 * and whose only output is the stream of
 *      vDB->addVar(Variant_t(...))                                 reference src/Graph.cc:1184-1188
 *                                                (ctor signature: reference src/Variant.hh:106-112)
 *
 * One `lancet_engine_run` == that call, for a whole batch of independent windows at once.
 * Plain pointers and sizes only; no C++ / torch types.  Return 0 on success, <0 on error (never aborts).
 * Outputs are owned by the engine and stay valid until the next upload/run/destroy on that engine.
 * One engine per (host thread, GPU); an engine is not thread-safe.
 */
#ifndef LANCET_ENGINE_H
#define LANCET_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* sample labels / strands as the reference encodes them */
#define LANCET_TMR 4 /* reference src/Ref.hh:36 */
#define LANCET_NML 5 /* reference src/Ref.hh:37 */
#define LANCET_FWD 1 /* reference src/ReadInfo.hh:30 */
#define LANCET_REV 2 /* reference src/ReadInfo.hh:31 */

/* Knobs copied into Graph_t before processGraph (reference src/Microassembler.cc:726-753, defaults
 * reference src/Lancet.hh:33-81).  lancet_params_default() fills the reference defaults. */
typedef struct lancet_params {
  int32_t min_k;             /* minK 11                      */
  int32_t max_k;             /* maxK 101                     */
  int32_t max_tip_len;       /* MAX_TIP_LEN 11               */
  int32_t cov_threshold;     /* COV_THRESHOLD 5              */
  int32_t low_cov_threshold; /* LOW_COV_THRESHOLD 1          */
  int32_t dfs_limit;         /* DFS_LIMIT 1000000            */
  int32_t max_indel_len;     /* MAX_INDEL_LEN 500            */
  int32_t max_mismatch;      /* MAX_MISMATCH 2               */
  int32_t min_qual_trim;     /* MIN_QV_TRIM 10 + '!'         */
  int32_t min_qual_call;     /* MIN_QV_CALL 17 + '!'         */
  int32_t max_unit_len;      /* MAX_UNIT_LEN 4   (STR)       */
  int32_t min_report_units;  /* MIN_REPORT_UNITS 3           */
  int32_t min_report_len;    /* MIN_REPORT_LEN 7             */
  int32_t dist_from_str;     /* DIST_FROM_STR 1              */
  int32_t lr_mode;           /* --linked-reads (LR_MODE false): barcode/haplotype aware coverage   */
  int32_t kmer_recovery;     /* -R / --kmer-recovery (KMER_RECOVERY false): 0 | 1.  After every buildgraph a tumour k-mer seen once lends its
                                occurrence to the well-supported k-mers one low-quality base away (reference src/ErrorCorrector.hh:38-134,
                                called at src/Microassembler.cc:137-140).  Not with lr_mode.  (Until this field the slot was `reserved`, 0.) */
  double  min_cov_ratio;     /* MIN_COV_RATIO 0.01           */
} lancet_params;

/* A batch of independent windows, SoA, caller-owned, read-only during the call.
 * Reads of window w are read_begin[w] .. read_begin[w+1]-1, in the order Graph_t::readid2info is filled:
 * tumor reads in BAM order, then normal reads in BAM order (reference src/Microassembler.cc:833-834).
 * Bases / qualities are ASCII exactly as BamAlignment::QueryBases / Qualities hold them (phred+33). */
typedef struct lancet_window_batch {
  int32_t         n_windows;
  const int32_t  *chr_id;      /* [n_windows] caller's chromosome id, echoed in lancet_variant        */
  const int32_t  *ref_start;   /* [n_windows] Ref_t::refstart (1-based)                               */
  const uint32_t *ref_off;     /* [n_windows+1] offsets into ref_bases                                 */
  const char     *ref_bases;   /* Ref_t::rawseq of every window, upper-case ACGTN, concatenated        */
  const uint32_t *read_begin;  /* [n_windows+1]                                                        */
  const uint32_t *seq_off;     /* [n_reads+1] offsets into seq / qual                                  */
  const char     *seq;         /* ReadInfo_t::seq_m                                                    */
  const char     *qual;        /* ReadInfo_t::qv_m                                                     */
  const uint8_t  *label;       /* [n_reads] LANCET_TMR | LANCET_NML   (ReadInfo_t::label_m); label / strand / mate with
                                   any other value are refused at upload (LANCET_E_ARG)                  */
  const uint8_t  *strand;      /* [n_reads] LANCET_FWD | LANCET_REV   (ReadInfo_t::strand)             */
  const uint8_t  *mate;        /* [n_reads] 0 | 1 | 2                 (ReadInfo_t::mate_order_m)       */
  const uint8_t  *mapped;      /* [n_reads] 1 = CODE_MAPPED, 0 = CODE_BASTARD (ReadInfo_t::code_m)     */
  const uint32_t *name_rank;   /* [n_reads] dense rank of ReadInfo_t::readname_m among the window's
                                  read names under std::string operator< (equal names = equal rank)   */
  /* --linked-reads only (lancet_params::lr_mode != 0); may be NULL otherwise.
   * reference: ReadInfo_t::BX / HP (src/ReadInfo.hh:60-61), filled by extractReads (src/Microassembler.cc:581-593) */
  const uint32_t *bx_rank;     /* [n_reads] dense rank of the BX:Z barcode among the batch's barcodes under
                                  std::string operator< ; LANCET_NO_BX for a read without barcode ("null")   */
  const uint8_t  *hp;          /* [n_reads] HP:i haplotype 0 (unassigned / absent) | 1 | 2                    */
} lancet_window_batch;
#define LANCET_NO_BX 0xFFFFFFFFu

/* One addVar(Variant_t(...)) call, arguments as passed at reference src/Graph.cc:1184-1188. */
typedef struct lancet_variant {
  int32_t  window;          /* index of the window in the batch                                      */
  int32_t  seq_in_window;   /* emission order within the window (0,1,2,...)                          */
  int32_t  chr_id;
  int32_t  pos;             /* transcript.pos - 1  (Variant_t ctor arg pos_)                          */
  uint8_t  code;            /* 'x' snv, '^' ins, 'v' del, 'c' complex                                 */
  uint8_t  prev_bp_ref;
  uint8_t  prev_bp_alt;
  uint8_t  reserved;
  uint16_t kmer;            /* K                                                                      */
  uint16_t cov[8];          /* RCN fwd,rev  RCT fwd,rev  ACN fwd,rev  ACT fwd,rev                     */
  uint16_t reserved2;
  uint32_t ref_off, ref_len;   /* transcript.ref  (may contain '-') in the blob                       */
  uint32_t alt_off, alt_len;   /* transcript.qry  (may contain '-') in the blob                       */
  uint32_t str_off, str_len;   /* STR annotation "<len><motif>" or empty                              */
} lancet_variant;

/* Per-window outcome. */
/* Linked-read annotations of variant i (same index as the lancet_variant array); all zero / empty unless lr_mode.
 * Replaces the HPRN/HPRT/HPAN/HPAT and bxset_* arguments of the Variant_t constructor (reference src/Graph.cc:1166-1188). */
typedef struct lancet_variant_lr {
  uint16_t hp[12];          /* HPRN, HPRT, HPAN, HPAT ; each {hp1, hp2, hp0}                                  */
  uint32_t bx_off[4];       /* bxset_ref_N, bxset_ref_T, bxset_alt_N, bxset_alt_T : offset (in u32) into bx_blob */
  uint32_t bx_len[4];       /* number of barcodes; they are bx_rank values in increasing order (== the ';'-joined
                               std::set<string> order of the reference); len 0 prints as "."                   */
  uint32_t reserved[2];
} lancet_variant_lr;

typedef struct lancet_window_stats {
  int32_t  status;        /* LANCET_W_* below                                                        */
  int32_t  final_k;       /* k of the last graph build (0 if none)                                   */
  int32_t  n_builds;      /* k-attempts that reached buildgraph                                       */
  int32_t  n_variants;
  uint64_t n_kmers;       /* sum over builds of the loadSequence trip count         */
  uint32_t max_nodes;     /* largest node table over the builds                                       */
  uint32_t sum_nodes;     /* sum over the builds of their node tables' sizes (40 B per node of every build) */
} lancet_window_stats;

#define LANCET_W_OK            0   /* processed (possibly with no variants)                          */
#define LANCET_W_NO_READS      1   /* countMappedReads()<=0 -> returned early (Microassembler.cc:83)  */
#define LANCET_W_K_EXHAUSTED   2   /* every k up to max_k was rejected                                */
#define LANCET_W_OVERFLOW     -1   /* a device work-space limit was hit; results for this window are
                                      NOT valid (reported loudly, never silently wrong).  Limits per window: a
                                      reference of at most 1024 bases, reads of at most 1023 + k bases (per-position
                                      counts wrap at 65 536 as the reference's unsigned short counters do), 2^21 reads
                                      (more than 65 535 reads: assembled by the re-run tier), 2^20 distinct k-mers
                                      unless LANCET_MAX_NODES says otherwise                            */

/* error codes */
#define LANCET_OK              0
#define LANCET_E_ARG          -1
#define LANCET_E_NO_DEVICE    -2
#define LANCET_E_HIP          -3
#define LANCET_E_UNSUPPORTED  -4
#define LANCET_E_OOM          -5
#define LANCET_E_STATE        -6

typedef struct lancet_engine lancet_engine;

void lancet_params_default(lancet_params *p);

/* device >= 0 : HIP device ordinal.  There is no CPU backend: creation fails with LANCET_E_NO_DEVICE
 * when no gfx950-compatible device is present.  LANCET_E_UNSUPPORTED: max_k > 127, min_k < 3 or max_unit_len > 8, or kmer_recovery together
 * with lr_mode (lancet_engine_last_error(NULL) then holds the reason).  LANCET_E_ARG: kmer_recovery other than 0 / 1.  Even k is
 * supported (k-mers that are their own reverse complement: CanonicalMer_t::set ties -> R, reference src/Mer.hh:57-71). */
int  lancet_engine_create(const lancet_params *p, int device, lancet_engine **out);
void lancet_engine_destroy(lancet_engine *e);
const char *lancet_engine_last_error(const lancet_engine *e);

/* Copies a batch to HBM (packs bases to 2 bit, sizes the per-window work space).  After this returns the
 * batch is device-resident and the caller's buffers are no longer referenced. */
int lancet_engine_upload(lancet_engine *e, const lancet_window_batch *b);

/* The same with the reads already trimmed and packed by the caller -- what lancet_engine_upload does itself, on host threads, from the
 * ASCII arrays (Graph_t::trim, reference src/Graph.cc:355-384, then 2 bit per base and one bit per base for `quality >= MIN_QUAL_CALL`):
 * 3 bits per base handed over instead of 16, and no second pass over the reads for a caller that assembles its batch from alignments anyway
 * (lancet_host_batch_packed does).  `b` as for lancet_engine_upload, but seq / qual / label / strand / mate / mapped are not looked at
 * (seq_off still gives the UNTRIMMED length of every read).  Read r owns (len + 15) / 16 words of `bases` from base_woff[r] and
 * (len + 31) / 32 words of `good` from good_woff[r], len its untrimmed length; both offset arrays have n_reads + 1 entries, `bases` has
 * 4 readable words past the last read's, `good` one.  Every read must have been packed by lancet_pack_read with the parameters this
 * engine was created with: the trim and the mask depend on min_qual_trim / min_qual_call, which the producer records in the struct
 * (lancet_host_batch_packed does; a caller of lancet_pack_read copies them from the lancet_params it packed with) -- an engine created
 * with other thresholds refuses the batch (LANCET_E_ARG) instead of building graphs from reads trimmed for another run. */
typedef struct lancet_packed_reads {
  uint32_t struct_size;        /* sizeof(lancet_packed_reads) as the CALLER's header has it: the first field, so that a caller built against
                                  another layout of this struct is refused (LANCET_E_ARG) instead of being read past its end.  The producers
                                  in this library (lancet_host_batch_packed) fill it in */
  uint32_t reserved;           /* 0 */
  const uint32_t *rinfo;       /* [n_reads] trimmed length and the read's flags, as lancet_pack_read leaves them */
  const uint32_t *base_woff;   /* [n_reads + 1] */
  const uint32_t *good_woff;   /* [n_reads + 1] */
  const uint32_t *bases;       /* 2 bit per base of the trimmed read, first base in the low bits */
  const uint32_t *good;        /* 1 bit per base of the trimmed read */
  int32_t min_qual_trim;       /* the thresholds the reads were trimmed / masked with (lancet_params of the packing side) */
  int32_t min_qual_call;
  /* Reads stored once (round 5).  Windows every 100 bases of 600 put an alignment into ~6 windows (reference src/Microassembler.cc:436-655
   * fetches it for each of them).  read_index != NULL: the five arrays above describe n_distinct DISTINCT reads (offsets: n_distinct + 1
   * entries) and read_index[r], r < read_begin[n_windows], says which of them read r of the batch is -- the words of an alignment are packed,
   * staged and copied to the device once per batch instead of once per window that holds it.  label / strand / mate / mapped are the
   * alignment's (in rinfo); only the name rank is per window (lancet_window_batch::name_rank).  NULL: one entry per read of the batch. */
  const uint32_t *read_index;
  uint32_t n_distinct;
  uint32_t reserved2;          /* 0 */
} lancet_packed_reads;
int lancet_engine_upload_packed(lancet_engine *e, const lancet_window_batch *b, const lancet_packed_reads *p);
/* One read, trimmed and packed: rinfo[0], (len + 15) / 16 words of bases and (len + 31) / 32 words of good are written (zero past the
 * trimmed length).  label / strand / mate / mapped as in lancet_window_batch. */
void lancet_pack_read(const lancet_params *P, const char *seq, const char *qual, int len, uint8_t label, uint8_t strand, uint8_t mate, uint8_t mapped,
                      uint32_t *rinfo, uint32_t *bases, uint32_t *good);

/* ---- device read selection (opt-in) -------------------------------------------------------------------------
 * The alignments of a scan are handed over ONCE (lancet_alignment_table -> lancet_device_reads); a batch is then a list of windows
 * (lancet_window_slice) and lancet_engine_upload_windows picks every window's reads on the device: the rules of extractReads /
 * isActiveRegion (reference src/Microassembler.cc:253-655) over per-alignment values that do not depend on the window.
 * lancet_host_alignment_table / lancet_host_windows (lancet_host.h) produce the two structs from BAMs; a caller that already holds decoded
 * alignments fills them itself.  All arrays are caller-owned and read-only during the calls. */
#define LANCET_NOT_TAKEN       1   /* lancet_engine_upload_windows: this batch has to go through lancet_host_batch[_packed] +
                                      lancet_engine_upload[_packed]; the reason is in lancet_engine_last_error.  Nothing was uploaded. */
#define LANCET_ALN_SEL_OK 1u       /* lancet_alignment_table::flags: passes every test of extractReads but containment and coverage */
#define LANCET_ALN_AR_OK  2u       /* ... passes isActiveRegion's filter (MAPQ, duplicate, l_seq != 0) */
#define LANCET_EVT_X  0            /* lancet_alignment_table::evt_kind: mismatch (MD or CIGAR X), insertion, deletion, soft clip */
#define LANCET_EVT_I  1
#define LANCET_EVT_D  2
#define LANCET_EVT_SC 3
typedef struct lancet_alignment_table {
  uint32_t struct_size;        /* sizeof(lancet_alignment_table) of the caller's header (another layout is refused) */
  uint32_t n_chroms;
  uint32_t n_aln[2];           /* alignments of the tumor [0] and of the normal [1]; every per-alignment array holds the tumor's, then the
                                  normal's, each in coordinate order per contig (the order extractReads walks) */
  const uint32_t *span;        /* [2][n_chroms][2]: per sample and contig (chr_id of the windows) its alignments [first, last) in the arrays */
  const int32_t  *pos0;        /* 0-based leftmost position */
  const int32_t  *ref_len;     /* reference bases covered */
  const uint32_t *l_seq;       /* untrimmed read length */
  const uint8_t  *flags;       /* LANCET_ALN_* */
  const uint32_t *rinfo;       /* trimmed length, sample, strand, mate, mapped: as lancet_pack_read leaves them (0 without LANCET_ALN_SEL_OK) */
  const uint32_t *evt_off;     /* [n + 1] CSR: the evidence events of isActiveRegion per alignment (none without LANCET_ALN_AR_OK) */
  const uint8_t  *evt_kind;    /* LANCET_EVT_* */
  const int32_t  *evt_pos;     /* the position isActiveRegion counts the event at (any int: it may lie past the alignment's end) */
  const uint32_t *name_off;    /* into names */
  const char     *names;       /* NUL-terminated read names; 8 readable bytes past the last name */
  uint64_t names_len;
  const uint32_t *base_woff;   /* (l_seq + 15) / 16 words of `bases` from here, (l_seq + 31) / 32 words of `good` from good_woff */
  const uint32_t *good_woff;
  const uint32_t *bases;       /* n_base_words + 4 words */
  const uint32_t *good;        /* n_good_words + 1 words */
  uint32_t n_base_words, n_good_words;
  int32_t min_qual_trim, min_qual_call;      /* the lancet_params thresholds the reads were trimmed / masked with */
  uint64_t load_id;            /* which load of the host object this is (0 for a caller's own table): windows of another load are not taken */
} lancet_alignment_table;

typedef struct lancet_window_slice {
  uint32_t struct_size;        /* sizeof(lancet_window_slice) */
  int32_t  n_windows;          /* windows of the range that pass the host-side window filters (empty sequence, isRepeat at max_k) */
  const int32_t  *widx;        /* [n] index in the tiling */
  const int32_t  *start, *end; /* [n] Ref_t coordinates (1-based start, the reference's `end`) */
  const int32_t  *chr_id;      /* [n] */
  const uint32_t *ref_off;     /* [n + 1] into ref_bases */
  const char     *ref_bases;
  uint32_t leak_reads;         /* reads the windows BEFORE the range left in the graph (reference src/Microassembler.cc:83); not 0: not taken */
  int32_t  host_reason;        /* LANCET_SLICE_* below: why the host side wants this range on the host route (0: no reason) */
  uint64_t load_id;            /* lancet_alignment_table::load_id the range's alignments belong to */
} lancet_window_slice;
#define LANCET_SLICE_RG_FILE    1  /* an --rg-file other than "keep all": isActiveRegion's read-group string is sequential state */
#define LANCET_SLICE_NOT_LOADED 2  /* batch-by-batch loading: the range's alignments are not the loaded ones (lancet_host_load_range) */

/* per-window result of the selection's first pass (debug / tests: lancet_engine_debug_select) */
typedef struct lancet_select_summary {
  uint32_t status;             /* bits 0-1: 0 filtered (no active region), 1 kept, 2 skipped for coverage; bit 2: a selected read is mapped;
                                  bit 3: the evidence table of the window overflowed (the batch is not taken) */
  uint32_t reads_t, reads_n;   /* selected reads per sample */
  uint32_t bases;              /* their untrimmed bases */
  uint32_t tw16, tw32;         /* sums of (trimmed length + 15) / 16 and (trimmed length + 31) / 32: the LDS build kernel's size test */
} lancet_select_summary;

typedef struct lancet_device_reads lancet_device_reads;
/* One device allocation that holds the table (the packed words of both samples in one array); shared by every engine on that device.
 * LANCET_E_NO_DEVICE without a gfx950 device: there is no CPU path. */
int  lancet_device_reads_create(int device, const lancet_alignment_table *tab, lancet_device_reads **out);
void lancet_device_reads_destroy(lancet_device_reads *r);
uint64_t lancet_device_reads_bytes(const lancet_device_reads *r);
struct lancet_host_opts;
/* Makes the engine's batch from the windows of `s` on the device -- the arrays lancet_engine_upload_packed stages, with the per-read
 * word offsets pointing into `reads` (no read word is copied).  kept[i] = tiled index of batch window i (room for s->n_windows).
 * LANCET_OK: uploaded, continue with lancet_engine_submit / run.  LANCET_NOT_TAKEN: see above; the cases are --linked-reads, a slice with a
 * host_reason or a non-empty leak or another load_id, a kept window with reads but no mapped read (the reference's read leak would start
 * there), a window with more selected reads or evidence positions than the selection kernel's LDS holds. */
int lancet_engine_upload_windows(lancet_engine *e, lancet_device_reads *reads, const lancet_window_slice *s, const struct lancet_host_opts *o,
                                 int32_t *kept, int32_t *n_kept);
/* Test hooks.  lancet_engine_debug_select: the summaries of the last lancet_engine_upload_windows (one per window of the slice, also after
 * LANCET_NOT_TAKEN).  lancet_engine_debug_batch: the uploaded batch read back from the device: which = 0 chr_id, 1 ref_start, 2 ref_off,
 * 3 ref_codes, 4 read_begin, 5 rinfo, 6 name_rank, 7 base_woff, 8 good_woff (bytes copied, < 0 on error); 9 / 10: the packed base / quality
 * words of read `arg` (its length is not known to the batch: `cap` bytes are copied); 11 / 12: the whole packed base / quality arrays the
 * offsets point into (out == NULL or cap == 0: only the size is returned). */
int lancet_engine_debug_select(lancet_engine *e, const lancet_select_summary **sum, int32_t *n);
long long lancet_engine_debug_batch(lancet_engine *e, int which, uint32_t arg, void *out, size_t cap);

/* Runs the whole hot path (self-tuning k loop included) for every uploaded window.  Blocking. */
int lancet_engine_run(lancet_engine *e);

/* upload + run in one call, the exact equivalent of the reference seam. */
int lancet_engine_process(lancet_engine *e, const lancet_window_batch *b);

/* lancet_engine_run in two halves: submit launches the kernels of the uploaded batch on the engine's stream and returns at once,
 * wait blocks until they are done (and re-runs what overflowed the small work space) and reads the results back.  One batch in
 * flight per engine; two engines on the same device, submitted in turn, overlap the tail of one batch with the bulk of the next. */
int lancet_engine_submit(lancet_engine *e);
int lancet_engine_wait(lancet_engine *e);
/* submit for the second of two engines that take turns on one device: e's kernels start when `prev`'s kernels are through (a batch's
 * kernels are sized for the whole device; side by side with another batch's they only slow each other down), while the host side of
 * the two batches -- upload, launch, read-back -- overlaps the other's kernels.  prev == NULL: lancet_engine_submit.
 * "Through" is, unless LANCET_GATE=0 is in the environment of the process that made the engines (and never in lr_mode): prev's window
 * kernel has taken the last quarter of its windows in hand -- e's build kernel is dispatched onto the CUs as that launch leaves them
 * (profiles/r6h_gate.txt).  Results do not depend on it. */
int lancet_engine_submit_after(lancet_engine *e, lancet_engine *prev);

/* Results of the last run: variants ordered by (window, seq_in_window) so that the caller can replay
 * addVar in reference order. */
int lancet_engine_results(lancet_engine *e, const lancet_variant **variants, uint32_t *n_variants,
                          const char **blob, uint32_t *blob_len, const lancet_window_stats **stats);

/* Timing of the last run as measured with HIP events on the engine's stream (milliseconds):
 * out[0] = all kernels of the run, out[1] = the assembly kernel only. */
/* Linked-read annotations of the last run (lr_mode engines; otherwise *lr = NULL): lr[i] belongs to variants[i]. */
int lancet_engine_results_lr(lancet_engine *e, const lancet_variant_lr **lr, const uint32_t **bx_blob, uint32_t *bx_blob_len);
int lancet_engine_last_timing(lancet_engine *e, float out[2]);

/* ---- assembled haplotypes ----
 * One lancet_haplotype per path the window kernel compared with the window reference (the reference's Graph_t::processPath, the calls for
 * which its -V prints "alignment" / "r:" / "p:"), in that order.  Off by default; on, it is a result like the records: every build route
 * (LDS build kernel, graphs built ahead, build service, general build), both tiers, lr_mode and kmer_recovery, with or without a trace.
 * lancet_engine_set_haplotypes: before an upload, reserve words_per_window 32-bit words per window (0 = off).  A haplotype of len bases
 * takes LANCET_HAP_HEADER_WORDS + (len + 15) / 16 of them; a value that does not hold one header and one word is LANCET_E_ARG.
 * LANCET_E_STATE between an upload and its run (the buffers are laid out by the upload) and while a batch is in flight.
 * A window whose haplotypes do not fit is marked truncated[w] = 1: it keeps, whole, the ones in front of the first that did not fit, and
 * nothing else about it changes -- the capture never overflows a window and never changes a record, a statistic or a trace word.  A
 * window with status < 0 has none; a window re-run by the second tier reports that tier's, once.
 * lancet_engine_results_haplotypes: after a run, ordered by (window, index_in_window); n = 0 and truncated all zero with the capture
 * off.  Base j of haplotype i: (words[h[i].word_off + j / 16] >> (2 * (j % 16))) & 3, A C G T = 0..3; the bits above len are 0. */
#define LANCET_HAP_HEADER_WORDS 8
#define LANCET_HAP_UNALIGNED 1u   /* flags: compared without alignment (same length, few mismatches: the Hamming short-cut, src/Graph.cc:818-826) */
#define LANCET_HAP_IS_REF 2u      /* flags: identical to the reference stretch                                                         */
#define LANCET_HAP_HAS_COVERAGE 4u   /* flags: the entry carries its per-base coverages (lancet_engine_set_haplotype_coverage)          */
#define LANCET_HAP_HAS_SUPPORT 8u    /* flags: the entry carries the counts of the reads that fit it (lancet_engine_set_haplotype_support) */
typedef struct lancet_haplotype {
  int32_t  window;            /* index in the batch */
  int32_t  index_in_window;   /* 0, 1, 2 ... in processPath order (across components and k, as -V prints them) */
  uint16_t kmer, component;
  uint32_t ref_off, ref_len;  /* the stretch of the window reference it was compared with (Ref_t::seq: trim5, length) = the r: line */
  uint32_t len;               /* bases of the path string = the p: line */
  uint32_t word_off;          /* (len + 15) / 16 words of `words` from here */
  int32_t  first_variant, n_variants;   /* seq_in_window of the lancet_variant records this path emitted */
  uint32_t flags;             /* LANCET_HAP_UNALIGNED | LANCET_HAP_IS_REF | LANCET_HAP_HAS_COVERAGE | LANCET_HAP_HAS_SUPPORT ; other bits 0 */
} lancet_haplotype;
int lancet_engine_set_haplotypes(lancet_engine *e, uint32_t words_per_window);
int lancet_engine_results_haplotypes(lancet_engine *e, const lancet_haplotype **h, uint32_t *n, const uint32_t **words,
                                     uint32_t *n_words, const uint8_t **truncated /* [n_windows] */);
/* Milliseconds on the host clock that the last run's read-back of the haplotypes took (the windows' lengths, the gather of the used words
 * on the device, one copy, the records); 0 with the capture off. */
float lancet_engine_haplotype_readback_ms(const lancet_engine *e);
/* ---- ... and how each lies on its reference stretch ----
 * lancet_engine_set_haplotype_alignments(e, 1): the uploads that follow also keep every path's alignment to its stretch, the one the
 * kernel walked for the records (global_align_aff's, or the two strings column by column for a path of the Hamming short-cut), as CIGAR
 * words: length << 4 | op, BAM's op codes (LANCET_HAP_OP_*), one word per maximal run of columns -- neighbouring words differ in op,
 * no length is 0, the I / = / X lengths sum to len and the D / = / X lengths to ref_len.  A haplotype identical to its stretch has one
 * '=' run; LANCET_HAP_UNALIGNED ones have '=' and 'X' only.  on is 0 or 1 (else LANCET_E_ARG); the state rules are those of
 * lancet_engine_set_haplotypes; without the capture itself the switch does nothing.  The words come out of the window's
 * words_per_window: an entry of the window's buffer is LANCET_HAP_HEADER_WORDS header words, the (len + 15) / 16 path words, and the
 * CIGAR words, whose number is header word LANCET_HAP_W_NCIGAR (0 with the switch off: the entry is then what it was before the switch
 * existed).  A haplotype whose CIGAR does not fit is one that does not fit: truncated[w] = 1, the ones in front of it stay whole.
 * lancet_engine_results_haplotype_alignments: after a run, the words of haplotype i of lancet_engine_results_haplotypes are
 * cigar[cigar_off[i] .. cigar_off[i + 1]); with the switch off every offset is 0 and n_cigar is 0.  words / word_off / n_words of
 * lancet_engine_results_haplotypes are path words only, whatever the switch says. */
#define LANCET_HAP_W_NCIGAR 7
#define LANCET_HAP_OP_I 1u        /* column with '-' in the reference string: bases of the path the stretch does not have */
#define LANCET_HAP_OP_D 2u        /* column with '-' in the path string                                                   */
#define LANCET_HAP_OP_EQ 7u       /* the same base in both                                                                */
#define LANCET_HAP_OP_X 8u        /* another base (an N of the reference included)                                        */
int lancet_engine_set_haplotype_alignments(lancet_engine *e, int on);
int lancet_engine_results_haplotype_alignments(lancet_engine *e, const uint32_t **cigar_off /* [n + 1] */, const uint32_t **cigar, uint32_t *n_cigar);
/* ---- ... and how well the reads support every base of it ----
 * lancet_engine_set_haplotype_coverage(e, 1): the uploads that follow also keep, for every path, the eight coverages the reference prints
 * per row of its vertical alignment (Graph_t::printVerticalAlignment under -v): for each base of the path the normal and the tumour
 * coverage, forward and reverse strand (an+ an- at+ at-: fwd / rev of Path_t::covDistr), and for each base of the stretch the reference's
 * (rn+ rn- rt+ rt-: Ref_t::getNormalCoverage / getTumorCoverage).  The values are the 16-bit counts the kernels hold -- they wrap where the
 * reference's unsigned short wraps; in lr_mode they are barcode counts, as the reference's are.  Which path base stands beside which
 * reference base is what the CIGAR says; the coverages themselves do not need the alignments switch.  on is 0 or 1 (else LANCET_E_ARG); the
 * state rules are those of lancet_engine_set_haplotypes; without the capture itself the switch does nothing.  The words come out of the
 * window's words_per_window: 2 * (len + ref_len) of them per entry, behind its CIGAR words, and the entry's flags say
 * LANCET_HAP_HAS_COVERAGE.  A haplotype whose coverages do not fit is one that does not fit: truncated[w] = 1, the ones in front stay whole.
 * lancet_engine_results_haplotype_coverage: after a run, cov[cov_off[i] .. cov_off[i + 1]) belongs to haplotype i of
 * lancet_engine_results_haplotypes: 4 * len values an+ an- at+ at- per path base, then 4 * ref_len values rn+ rn- rt+ rt- per base of the
 * stretch (offset ref_off + j of the window reference).  With the switch off every offset is 0 and n_cov is 0. */
int lancet_engine_set_haplotype_coverage(lancet_engine *e, int on);
int lancet_engine_results_haplotype_coverage(lancet_engine *e, const uint32_t **cov_off /* [n + 1] */, const uint16_t **cov, uint32_t *n_cov);
/* ---- ... and how many reads carry it rather than its rivals ----
 * lancet_engine_set_haplotype_support(e, 1, max_mismatches): after the windows of the runs that follow are through, a kernel of its own
 * compares every read of a window with every haplotype of it (XOR and popcount over the packed words, both still resident) and counts,
 * per haplotype and read class Tf Tr Nf Nr (tumour / normal, forward / reverse: the order of the coverages' counters), the reads that fit.
 * All of it is integer arithmetic, and this is its definition -- the reference has no such value:
 *   A read is taken as the kernels see it: trimmed (Graph_t::trim), t bases, in BAM orientation, as the path strings are.  The GROUP of a
 *   haplotype is its (kmer, component): haplotypes of one group share their stretch and compete, others do not.
 *   A placement of a read on a haplotype of M bases at k is an offset o, negative ones included, whose overlap
 *   v(o) = min(t, M - o) - max(0, -o) is at least k: the read may hang over either end of the path.  mm(o) counts the overlap positions i
 *   with read[i] != path[o + i]; d = min over o of mm(o).  A read with t < k has no d for that haplotype.
 *   The read FITS haplotype h iff d(h) is the smallest d over the haplotypes of h's group and d(h) <= max_mismatches; it fits h ALONE iff
 *   it fits no other haplotype of the group.
 * Limits: base qualities are not looked at; placements are ungapped; rivals are the haplotypes of the same (k, component) only; in a
 * truncated window the counts are those among its whole entries.
 * on is 0 or 1, max_mismatches 0..255 (else LANCET_E_ARG); the state rules are those of lancet_engine_set_haplotypes; without the
 * capture itself the switch does nothing.  The words come out of the window's words_per_window: 8 per entry, behind its coverage words,
 * and the entry's flags say LANCET_HAP_HAS_SUPPORT; a haplotype whose 8 words do not fit is one that does not fit.
 * lancet_engine_results_haplotype_support: after a run, support[8 * i .. 8 * i + 8) belongs to haplotype i of
 * lancet_engine_results_haplotypes: fit Tf Tr Nf Nr, then alone Tf Tr Nf Nr.  NULL with the switch off (or no haplotype).
 * lancet_engine_haplotype_support_ms: HIP-event milliseconds of the support kernel in the last run; 0 with the switch off.  (The kernel is
 * not one of lancet_engine_kernel_name's: it runs in lancet_engine_wait, behind the re-run tier.) */
int lancet_engine_set_haplotype_support(lancet_engine *e, int on, int max_mismatches);
int lancet_engine_results_haplotype_support(lancet_engine *e, const uint32_t **support /* [n][8]: fit Tf Tr Nf Nr, alone Tf Tr Nf Nr */);
float lancet_engine_haplotype_support_ms(const lancet_engine *e);
/* ---- ... and, per read, where it lies on the haplotype it fits best ----
 * lancet_engine_set_haplotype_placements(e, 1, max_mismatches): after the windows of the runs that follow are through, a second kernel of
 * that kind writes one record per read of the batch.  The reference has no such value; this is its definition, in the terms of the support
 * definition above (the read as the kernels see it: trimmed, t bases, in BAM orientation; a placement on a whole entry h of M bases at its k
 * is an offset o in [k - t, M - k], at least k bases of overlap; mm(o) the overlap positions that differ; d(r, h) the smallest mm(o) on h).
 * Over ALL whole entries of the read's window:
 *   mismatches   = the smallest d;
 *   haplotype    = the entry with that d that has the smallest index_in_window;
 *   offset       = the smallest o on that entry with mm(o) = d (negative: the read's first -o bases hang over the path's start);
 *   n_offsets    = how many offsets of that entry have mm(o) = d;
 *   n_haplotypes = how many entries of the window have that d -- across all (k, component) groups, so the same string reported at two k
 *                  counts twice, as it does in the support counts.
 * Both counts saturate at LANCET_PLACEMENT_COUNT_MAX.  A read is PLACED iff such an entry exists and mismatches <= max_mismatches; a read
 * that is not has haplotype = -1 and every other field 0: t < k for every entry, a junk read, a window without whole entries, a
 * window with status < 0.  In a truncated window the candidates are its whole entries; a window the second tier re-ran has that tier's.
 * The entry with the smallest d of the window has the smallest d of its own group: with equal limits a placed read FITS its haplotype in the
 * sense of lancet_engine_set_haplotype_support.
 * on is 0 or 1, max_mismatches 0..255 (else LANCET_E_ARG), independent of the support limit; the state rules are those of
 * lancet_engine_set_haplotype_support; without the capture itself the switch does nothing.  The records lie in a buffer of their own: no
 * entry changes, and neither switch changes the other's output.  A window's buffer that could hold more than 2^24 - 1 entries
 * (words_per_window above 9 * (2^24 - 1)) or parameters whose longest path (1024 + max_indel_len + 256 bases) is not below 2^17 bases are
 * refused with LANCET_E_ARG where the switch is set, and by lancet_engine_set_haplotypes while it is on.
 * lancet_engine_results_haplotype_placements: after a run, p[read_begin[w] .. read_begin[w + 1]) are the reads of window w in the
 * batch's read order, tlen[i] the trimmed length t the kernel used for read i (a caller tells soft clips from overlap by it).  p is NULL
 * and n_reads 0 with the switch off.  lancet_engine_haplotype_placement_ms: HIP-event milliseconds of the kernel in the last run. */
#define LANCET_PLACEMENT_COUNT_MAX 127u
typedef struct lancet_read_placement {
  int32_t haplotype;      /* index_in_window, -1: not placed */
  int32_t offset;
  uint16_t mismatches, n_offsets, n_haplotypes, cls;   /* cls 0..3 = Tf Tr Nf Nr */
} lancet_read_placement;
int   lancet_engine_set_haplotype_placements(lancet_engine *e, int on, int max_mismatches);   /* 0..255 */
int   lancet_engine_results_haplotype_placements(lancet_engine *e, const lancet_read_placement **p, uint32_t *n_reads,
                                                 const uint32_t **read_begin /* [n_windows + 1] */, const uint16_t **tlen);
float lancet_engine_haplotype_placement_ms(const lancet_engine *e);
/* ---- ... and, per allele, the reads that carry it, the reference allele or something else at its site ----
 * lancet_engine_set_haplotype_evidence(e, events_per_window, max_mismatches): after the windows of the runs that follow are through, a
 * third kernel of that kind writes one record per EVENT of every whole entry.  The reference has no such value; this is its definition, all
 * in integers, in the terms of the two definitions above (the read as the kernels see it: trimmed, t bases, in BAM orientation; offsets o
 * in [k - t, M - k]; mm(o); d(r, h); the GROUP of an entry: the run of whole entries with its (kmer, component), which share their stretch).
 * Events.  An event of an entry h is a maximal run of neighbouring CIGAR words whose op is not '=' -- what the kernels' transcript walk
 *   turns into one record.  It has four numbers: rb, the stretch bases in front of it; rs, the stretch bases it spans (its D and X
 *   lengths); pb, the path bases in front of it; ps, the path bases it spans (its I and X lengths).  A LANCET_HAP_IS_REF entry has none, a
 *   LANCET_HAP_UNALIGNED one has one per run of X.
 * Carriers.  An event e' of another entry h' of the group TOUCHES e = (rb, rs, ps, bases) iff rb' <= rb + rs and rb' + rs' >= rb (closed
 *   intervals: an insertion at either edge touches).  h' carries ALT iff exactly one of its events touches and that one has the same rb, rs
 *   and ps and the same ps path bases; REF iff none touches; OTHER otherwise.  h itself carries ALT.
 * Sites.  The site of e on h' is the path interval [left, right): lo = min(rb, the smallest rb' of a touching event), hi = max(rb + rs,
 *   the largest rb' + rs' of one), shift = the sum of ps" - rs" over the events of h' that lie wholly in front of lo, left = lo + shift,
 *   right = hi + shift + the sum of ps' - rs' over the touching events.  For an ALT carrier that is [pb', pb' + ps), for a REF carrier
 *   the image of [rb, rb + rs).
 * Reads.  Best(r) = the entries of the group whose d(r, h') is the group's smallest and <= max_mismatches: the entries r FITS in the
 *   sense of lancet_engine_set_haplotype_support.  On such an entry o* is the smallest offset with mm(o*) = d, the placement kernel's
 *   `offset`.  r is INFORMATIVE for e on h' iff left >= 1, right + 1 <= M, o* <= left - 1 and o* + t >= right + 1: one path base on
 *   either side of the site lies under the read.  r counts ALT for e iff it is informative on at least one ALT carrier of Best(r) and on
 *   no REF or OTHER carrier; REF iff on at least one REF carrier and on no ALT or OTHER carrier; OTHER iff it is informative anywhere
 *   and counts neither; a read that is informative nowhere counts nothing.  Per event: alt, ref and other, each by class Tf Tr Nf Nr.
 * Limits: base qualities are not looked at; placements are ungapped; rivals are the group's entries only (the same string at two k is
 * judged twice, each time among the entries of its k); a window whose reference path was not assembled has no REF carrier, so its ref
 * counts are 0; in a truncated window the candidates are its whole entries; an event at a path's first or last base has no flank and so
 * no informative read.  In lr_mode reads are reads here, not barcodes.
 * events_per_window: records kept per window, 0 = off; max_mismatches 0..255, independent of the other two limits (else LANCET_E_ARG, as
 * is an events_per_window of 2^24 or more); the state rules are those of lancet_engine_set_haplotypes.  The switch needs the capture and
 * lancet_engine_set_haplotype_alignments; without either it does nothing.  The records lie in a buffer of their own: no entry, record,
 * statistic or trace word changes.  A window with more events keeps the first events_per_window, whole, and is marked.  The kernel keeps a
 * group's entries and events in lists of LANCET_EVID_GROUP_ENTRIES and LANCET_EVID_GROUP_EVENTS; the events of a group beyond either come
 * with LANCET_EVID_UNEVALUATED and all counts 0, never with partial counts.
 * lancet_engine_results_haplotype_evidence: after a run, the events of haplotype i of lancet_engine_results_haplotypes are
 * ev[event_off[i] .. event_off[i + 1]), in CIGAR order; marked[w] = 1 where window w had more events than were kept.  `variant` is the
 * index in lancet_engine_results' records of the one the event emitted: the record of haplotype h with seq_in_window in [first_variant,
 * first_variant + n_variants) and pos + 1 - ref_start[window] - ref_off == rb; -1 where there is none (its alt coverage was 0, or the
 * walk ended in front of it).  ev is NULL and n_events 0 with the switch off.
 * lancet_engine_haplotype_evidence_ms: HIP-event milliseconds of the kernel in the last run; _readback_ms: host-clock milliseconds of the
 * read-back (the windows' counts, the gather of the kept records on the device, one copy, the join). */
#define LANCET_EVID_UNEVALUATED 1u
#define LANCET_EVID_GROUP_ENTRIES 32u
#define LANCET_EVID_GROUP_EVENTS 64u
typedef struct lancet_variant_evidence {
  int32_t  haplotype;       /* index in lancet_engine_results_haplotypes */
  int32_t  variant;         /* index in lancet_engine_results' records, -1: none */
  uint32_t rb, rs, pb, ps;
  uint32_t flags;           /* LANCET_EVID_UNEVALUATED ; other bits 0 */
  uint32_t alt[4], ref[4], other[4];   /* Tf Tr Nf Nr */
} lancet_variant_evidence;
int   lancet_engine_set_haplotype_evidence(lancet_engine *e, uint32_t events_per_window, int max_mismatches);   /* 0..255 */
int   lancet_engine_results_haplotype_evidence(lancet_engine *e, const lancet_variant_evidence **ev, uint32_t *n_events,
                                               const uint32_t **event_off /* [n_haplotypes + 1] */, const uint8_t **marked /* [n_windows] */);
float lancet_engine_haplotype_evidence_ms(const lancet_engine *e);
float lancet_engine_haplotype_evidence_readback_ms(const lancet_engine *e);

/* The kernels one run launches, back to back on the engine's stream: lancet_engine_kernel_name(i) for i = 0, 1, ... (NULL past
 * the last) and the HIP-event duration of each in the last run (milliseconds; returns how many were written, <= cap). */
const char *lancet_engine_kernel_name(int i);
int lancet_engine_kernel_times(lancet_engine *e, float *ms, int cap);
/* Windows of the last run whose first graph was assembled by the LDS build kernel (the others took the general build phases). */
int lancet_engine_prebuilt_count(lancet_engine *e);
/* Windows of the last run that the build kernel SETTLED: the graph after the first removeLowCov was the window reference's own k-mers in
 * one chain, beside components without a node for markRefEnds to start from at most, so the window ended at that k with no record and the
 * window kernel loaded nothing of it.  0 whenever the trace, the haplotype capture or --linked-reads is on, or LANCET_NO_SETTLE=1 is in the
 * environment; with LANCET_SETTLE_CHAIN_ONLY=1 only windows whose chain is the whole graph.  Results never depend on it. */
int lancet_engine_settled_count(lancet_engine *e);
/* Graphs the build kernel built AHEAD in the last run -- the next k of a window whose graph at the current k holds a k-mer twice
 * in one read and will be rejected (reference src/Microassembler.cc:198-206: cycle -> next k) -- and how many of them the window
 * kernel took instead of building that graph itself.  Scheduling only: results never depend on what was built ahead. */
int lancet_engine_ahead_counts(lancet_engine *e, int32_t *built, int32_t *used);
/* Build service of the last run.  A window whose k was rejected and whose next graph was not built ahead is suspended; a few
 * resident workgroups of the LDS build kernel build that graph while the window kernel goes on with other windows, then the window
 * resumes.  out = requests posted, served, not buildable in LDS, taken back by the window kernel (general build).  Scheduling
 * only: results never depend on who built a graph. */
int lancet_engine_svc_counts(lancet_engine *e, uint32_t out[4]);
/* Profiling aid: wall-clock ticks (10 ns) the LDS build kernel's workgroups spent per phase in the last run (16 values).
 * Accounted only in an engine made with LANCET_PHASE_TIMES set in the environment (zeros otherwise; the same holds for
 * lancet_engine_phase_times): the accounting costs both kernels a clock read per phase and the build kernel contended atomics per window. */
int lancet_engine_build_phase_times(lancet_engine *e, const unsigned long long **ticks);

/* ---- the reference's -v stage trace (reference src/Microassembler.cc:87-246, Graph.cc verbose blocks) ----
 * lancet_engine_set_trace: before an upload, reserve words_per_window 32-bit words of trace events per window (0 = off).
 * lancet_engine_trace: after a run, evt_len[w] words of window w's events start at evt[w * words_per_window].
 * lancet_trace_format: those events as the text the reference prints (malloc'd, free with lancet_free); idx1 = the running
 * number of the window ("== Processing N:"), hdr / chrom / start / end = the window's name and coordinates. */
int lancet_engine_set_trace(lancet_engine *e, uint32_t words_per_window);
/* The same with a trace level.  Level 1 is lancet_engine_set_trace.  Level 2 adds what the reference prints under -V / --more-verbose
 * (src/Graph.cc:328-332, :539, :2030-2034, :2168-2213, :800-802): reads that run through a k-mer twice, the reference pseudo-read's id, what
 * markRefEnds looked at and which nodes it cut off in front of the source and behind the sink, and per path the trimmed window reference and
 * the path's string.  A DIAGNOSTICS mode, not a throughput mode: those lines come from steps the LDS build kernel otherwise does, so while
 * level 2 is set every graph takes the general build (as under LANCET_NO_PREBUILD; no graphs built ahead, no build service).  Records, window
 * stats and the level-1 lines are those of a run without it.  Path strings are long: size words_per_window from the batch (lancet_gpu, per
 * batch: 512 words, 32 paths of (longest window reference + max_indel_len + 256) bases at a quarter word per base, 16 words per reference
 * base for the cycle lines).  At level 2 a window whose events
 * do not fit is not cut silently: evt_len[w] == words_per_window marks it, the last eight words of its buffer say how many words hold events
 * (lancet_trace_format2 prints them and a line "[trace truncated: ...]").  Level 2 needs words_per_window >= 16 (or 0 = off); LANCET_E_ARG
 * otherwise and for a level other than 1 or 2.  lancet_engine_trace_level: the level of the engine's next / last upload (0: tracing off). */
int lancet_engine_set_trace_level(lancet_engine *e, uint32_t words_per_window, int32_t level);
int lancet_engine_trace_level(const lancet_engine *e);
int lancet_engine_trace(lancet_engine *e, const uint32_t **evt_len, const uint32_t **evt, uint32_t *words_per_window);
char *lancet_trace_format(const uint32_t *words, uint32_t n_words, int32_t idx1, const char *hdr, const char *chrom,
                          int32_t start, int32_t end, int32_t dfs_limit);
/* lancet_trace_format for a level-2 trace: words_per_window as given to lancet_engine_set_trace_level (n_words == words_per_window is the
 * truncation mark), rawseq / rawseq_len = the window's Ref_t::rawseq (lancet_window_batch::ref_bases of the window), which the level-2
 * events refer to by offset.  With the events of a level-1 trace the text is lancet_trace_format's. */
char *lancet_trace_format2(const uint32_t *words, uint32_t n_words, uint32_t words_per_window, int32_t idx1, const char *hdr, const char *chrom,
                           int32_t start, int32_t end, int32_t dfs_limit, const char *rawseq, uint32_t rawseq_len);

/* ---- test hook: the device global_align_aff (reference src/align.cc:235-364) alone, on one pair of ACGT strings ----------
 * S has 1..1024 bases, T 1..16383 (the traceback keeps positions of T in 14 bits; longer: LANCET_E_ARG).  The aligned rows go to
 * S_aln / T_aln (cap bytes each, NUL-terminated).  mode:
 *   0  band of 128 diagonals first, the full matrix when the band cannot certify itself (what a window runs)
 *   1  the full matrix only
 *   2  the band only; LANCET_E_STATE when it did not certify itself
 *   4, 5, 6  modes 0, 1, 2 through the 512-lane build of the same source (the re-run tier's kernel)
 * LANCET_E_UNSUPPORTED: the reference's own traceback leaves its matrix on this pair (undefined behaviour there; a window
 * with such a path is reported LANCET_W_OVERFLOW), or the rows do not fit cap.  lancet_debug_align is mode 0.
 * lancet_engine_create refuses max_indel_len above 15103 (LANCET_E_ARG) for the same 14 bits: path strings have up to
 * 1024 + max_indel_len + 256 bases. */
int lancet_debug_align(lancet_engine *e, const char *S, const char *T, char *S_aln, char *T_aln, int cap);
int lancet_debug_align_mode(lancet_engine *e, const char *S, const char *T, char *S_aln, char *T_aln, int cap, int mode);

/* ---- host side of the seam: Variant_t normalisation + VariantDB + VCF ----------
 * reference src/Variant.hh:106-172 (ctor), src/VariantDB.cc:28-91 (addVar), :93-179 (VCF),
 * src/Variant.cc:39-223 (printVCF). */
typedef struct lancet_filters {     /* reference src/Variant.hh:42-56, defaults src/Lancet.cc:627-637 */
  double  min_phred_fisher_str, min_phred_fisher, max_vaf_normal, min_vaf_tumor;
  int32_t min_cov_normal, max_cov_normal, min_cov_tumor, max_cov_tumor;
  int32_t min_alt_cnt_tumor, max_alt_cnt_normal, min_strand_bias, reserved;
} lancet_filters;

typedef struct lancet_vdb lancet_vdb;

void lancet_filters_default(lancet_filters *f);
lancet_vdb *lancet_vdb_create(const lancet_filters *f);
void lancet_vdb_destroy(lancet_vdb *db);
/* addVar for records [0,n) in the given order; chr_names[chr_id] gives the chromosome string. */
int  lancet_vdb_add(lancet_vdb *db, const lancet_variant *v, uint32_t n, const char *blob,
                    const char *const *chr_names, int32_t n_chr);
/* --linked-reads flavour of lancet_vdb_add (VariantDB_t(LR_MODE=true)): lr / bx_blob from lancet_engine_results_lr,
 * bx_names[rank] = the barcode strings the batch's bx_rank values refer to.  A database is either fed with
 * lancet_vdb_add only or with lancet_vdb_add_lr only. */
int  lancet_vdb_add_lr(lancet_vdb *db, const lancet_variant *v, const lancet_variant_lr *lr, uint32_t n, const char *blob,
                       const uint32_t *bx_blob, const char *const *bx_names, uint32_t n_bx,
                       const char *const *chr_names, int32_t n_chr);
/* Keys where the records are made, inserts where the VariantDB lives (a multi-GPU run: every rank keys its own records, rank 0 merges):
 * lancet_vdb_keys writes the 32 raw sha256 bytes addVar keys its map with (reference src/VariantDB.cc:36-40, Variant_t::getSignature
 * src/Variant.cc:339-344) per record; lancet_vdb_add_keyed is lancet_vdb_add / lancet_vdb_add_lr (lr, bx_blob, bx_names may be null)
 * with those keys given.  Keys that do not belong to the records are the caller's error (not checked). */
int  lancet_vdb_keys(const lancet_variant *v, uint32_t n, const char *blob, const char *const *chr_names, int32_t n_chr, uint8_t *keys);
/* keep[i] = 1 for the records of a keyed stream that can change a VariantDB (per key: the first, and the first that reaches the key's
 * largest total coverage; reference src/VariantDB.cc:45-88); a rank drops the others before its records travel to the merging rank. */
int  lancet_vdb_reduce(const lancet_variant *v, const uint8_t *keys, uint32_t n, uint8_t *keep);
int  lancet_vdb_add_keyed(lancet_vdb *db, const lancet_variant *v, const lancet_variant_lr *lr, const uint8_t *keys, uint32_t n, const char *blob,
                          const uint32_t *bx_blob, const char *const *bx_names, uint32_t n_bx, const char *const *chr_names, int32_t n_chr);
uint32_t lancet_vdb_size(const lancet_vdb *db);
/* Writes the VCF (header + sorted body) into a malloc'd string the caller frees with lancet_free.
 * date_line: text after "##fileDate=" (ctime() format incl. trailing newline), may be NULL -> omitted. */
char *lancet_vdb_vcf(lancet_vdb *db, const char *version, const char *cmdline, const char *reference,
                     const char *date_line, const char *sample_normal, const char *sample_tumor);
void lancet_free(void *p);

#ifdef __cplusplus
}
#endif
#endif /* LANCET_ENGINE_H */
