// lancet_main.cc -- `lancet_gpu`: the reference's command line (reference src/Lancet.cc:655-800) on the native host side
// (include/lancet_host.h) and the MI355X engine (include/lancet_engine.h).
//
//     lancet_gpu --tumor T.bam --normal N.bam --ref ref.fa --reg chr22:1000-5000 > out.vcf
//
// There is no CPU path: without a gfx950 device engine creation fails and the program stops with an error.
// Beyond the reference's options: --device N | --devices a,b,... (one engine per entry; batches of --batch-windows windows
// go to the engines in turn while the host prepares the next one; records reach the VariantDB in window order whatever
// the number of engines), --strict (no VCF at all when a window exceeded the engine's work space; by default the run
// finishes, the windows are listed on stderr and the exit code is 3).
// --ranks N: N processes, one per GPU (rank r on --devices[r mod #devices], default device r): the batches of --batch-windows windows are
// dealt out to the ranks in contiguous runs, every rank keys and reduces its records (lancet_records_pack) and they are gathered to rank 0 over RCCL
// (lancet_comm_gather: sizes by one all-gather, payloads by send / recv to rank 0 only) and replayed into the VariantDB in window order
// (lancet_records_merge) -- what the reference does with its per-thread databases at the end of main() (reference src/Lancet.cc:940-959).
// Without --rank the program starts the N ranks itself (children of this process, --rank r --rendezvous <path> appended) and waits for
// them; a job launcher may start the ranks itself with --rank / --rendezvous.  The VCF (rank 0's stdout) does not depend on N.
// -R / --kmer-recovery: lancet_params::kmer_recovery (not together with --linked-reads: refused before any work is done).
// --device-select: the loaded alignments are exported once (lancet_host_alignment_table -> lancet_device_reads_create, one table per GPU) and a
// batch is lancet_host_windows -> lancet_engine_upload_windows -> lancet_host_windows_done; LANCET_NOT_TAKEN batches go through
// lancet_host_batch_packed -> lancet_engine_upload_packed as without the option.  One stderr line at the end counts both, by reason.
// Not offered: --print-graph; --num-threads is accepted and ignored (windows are
// batched on the GPU); -v prints the reference's per-window stage trace to stderr.
// -V / --more-verbose: -v plus the reference's -V lines (lancet_engine_set_trace_level, level 2): a diagnostics mode, every graph through the
// general build.  The trace buffer is sized per batch (trace_words_for); windows whose trace did not fit say so in the text and are counted
// on stderr.  The VCF is the one without the flag.
// --haplotypes FILE: every assembled path of every window (lancet_engine_set_haplotypes) as FASTA, one record per haplotype in window processing
// order: >chr:start-end|k=..|comp=..|path=..|ref=off+len|variants=first+n and the sequence on one line (ref: the stretch of the window reference
// the path was compared with; variants: the window's records, in emission order, that this path emitted).  The buffer is sized per batch
// (hap_words_for); windows whose haplotypes did not all fit are counted on stderr.  Not with --ranks above 1 (the gather carries records only);
// the option is left out of ##cmdline: the VCF is byte for byte the one without it.
// --haplotype-sam FILE: the same haplotypes as SAM records, each aligned to the contig as the window kernel aligned it to its reference stretch
// (lancet_engine_set_haplotype_alignments): @HD / @SQ per contig of the FASTA / @PG, then per haplotype QNAME = the FASTA record's name up to
// path=.., FLAG 0, POS = first base of the stretch, MAPQ 255, the CIGAR in = X I D (a D run at either end is dropped, POS moves past a leading
// one), SEQ, and the tags kk:i (k) cp:i (component) pi:i (index in window) wn:Z (window) vf:i / vn:i (first_variant, n_variants) fl:i (flags).
// Alone or with --haplotypes; the same rules (not with --ranks above 1, left out of ##cmdline); the buffer is 64 words per path larger.
// --haplotype-coverage FILE: per haplotype, in the same order, the --haplotypes header line up to ref=off+len and below it the table the
// reference prints for that path under -v (Graph_t::printVerticalAlignment, src/Graph.cc:749-783), byte for byte: the `Pos r p d an+ ...` line
// and one row per alignment column with the path's and the reference's normal / tumour coverage per strand
// (lancet_engine_set_haplotype_coverage; the alignments are turned on with it, the table needs the columns).  Alone or with the other two;
// the same rules; the buffer is 2 * (2 * longest + --max-indel-len + 256) words per path larger.  With --haplotype-sam every SAM record
// gains the tags nf nr tf tr (B:S): the path's an+ an- at+ at-, one value per SEQ base.
// --haplotype-support FILE: per haplotype, in the same order, one line: the --haplotypes header up to ref=off+len without the '>', a tab, and
// the eight counts of lancet_engine_set_haplotype_support tab-separated -- the reads that fit the path (fit_tf fit_tr fit_nf fit_nr) and
// that fit it alone among the paths of its (k, component) (alone_tf ... alone_nr), within --haplotype-support-mismatches N (default 5, the
// reference's HD_DISTANCE_CUTOFF) mismatches of an ungapped placement; the first line names the columns.  Alone or with the other three; the
// same rules; the buffer is 8 words per path larger.  With --haplotype-sam every SAM record gains the tags sf and sa (B:I, four values each).
// --haplotype-reads FILE: SAM again, the same header, one record per PLACED read of every window (lancet_engine_set_haplotype_placements, within
// --haplotype-read-mismatches N, default 5): the read realigned through the haplotype it fits best.  QNAME = chr:start-end|r=<the read's number
// in its window> (the batch carries name ranks, not names), FLAG 16 for a reverse-strand read, POS / CIGAR from lc_read_cigar (host_common.h)
// with the coordinate arithmetic of --haplotype-sam, MAPQ 255, SEQ the trimmed read, QUAL *, tags wn:Z hi:i (the pi of --haplotype-sam) kk:i
// cp:i ho:i hm:i on:i hn:i sm:A (T / N).  A read selected by several overlapping windows gets a record per window.  Alone or with the other
// four; the same rules; with --device-select the batches go the host route (SEQ comes from the host's packed words).
// --variant-evidence FILE: per record of the VCF's raw material, the reads for and against its allele by haplotype fit
// (lancet_engine_set_haplotype_evidence, within --variant-evidence-mismatches N, default 5).  The first line names the columns; then one line
// per event that has a record (lc_evid_join, host_common.h), in window processing order: window, chromosome, the record's position, code, ref
// and alt strings as the record holds them, k, component, path index, and the twelve counts alt / ref / other by class Tf Tr Nf Nr.  The
// capture and the alignments are turned on with it; EVID_EVENTS records are kept per window.  Alone or with the other five; the same rules:
// same VCF bytes, left out of ##cmdline, refused with --ranks above 1, windows with more events and unevaluated events counted on stderr.
// With --haplotype-sam every SAM record with events gains the tag ev:Z: its events as rb,rs,pb,ps,flags and the twelve counts, joined by ';'.
// With --device-select the device route works unchanged: the kernel reads the resident batch, whichever route made it.
#include "../../include/lancet_host.h"
#include "host_common.h"      // lc_read_cigar
#include "../../include/lancet_gather.h"

#include <signal.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <cctype>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <future>
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace {
struct Opt { const char *lng; char shrt; int has_arg; };
const Opt OPTS[] = {
  {"tumor", 't', 1}, {"normal", 'n', 1}, {"ref", 'r', 1}, {"reg", 'p', 1}, {"bed", 'B', 1}, {"rg-file", 'g', 1}, {"min-k", 'k', 1}, {"max-k", 'K', 1},
  {"trim-lowqual", 'q', 1}, {"min-base-qual", 'C', 1}, {"quality-range", 'Q', 1}, {"min-map-qual", 'b', 1},
  {"max-as-xs-diff", 'Z', 1}, {"tip-len", 'l', 1}, {"cov-thr", 'c', 1}, {"cov-ratio", 'x', 1}, {"low-cov", 'd', 1},
  {"max-avg-cov", 'u', 1}, {"window-size", 'w', 1}, {"padding", 'P', 1}, {"dfs-limit", 'F', 1}, {"max-indel-len", 'T', 1},
  {"max-mismatch", 'M', 1}, {"num-threads", 'X', 1}, {"min-alt-count-tumor", 'a', 1}, {"max-alt-count-normal", 'm', 1},
  {"min-vaf-tumor", 'e', 1}, {"max-vaf-normal", 'i', 1}, {"min-coverage-tumor", 'o', 1}, {"max-coverage-tumor", 'y', 1},
  {"min-coverage-normal", 'z', 1}, {"max-coverage-normal", 'j', 1}, {"min-phred-fisher", 's', 1},
  {"min-phred-fisher-str", 'E', 1}, {"min-strand-bias", 'f', 1}, {"max-unit-length", 'U', 1}, {"min-report-unit", 'N', 1},
  {"min-report-len", 'Y', 1}, {"dist-from-str", 'D', 1}, {"linked-reads", 'J', 0}, {"kmer-recovery", 'R', 0}, {"primary-alignment-only", 'I', 0},
  {"XA-tag-filter", 'O', 0}, {"active-region-off", 'W', 0}, {"verbose", 'v', 0}, {"more-verbose", 'V', 0}, {"device", 0, 1}, {"devices", 0, 1}, {"batch-windows", 0, 1}, {"date-line", 0, 1}, {"strict", 0, 0}, {"device-select", 0, 0}, {"haplotypes", 0, 1}, {"haplotype-sam", 0, 1}, {"haplotype-coverage", 0, 1}, {"haplotype-support", 0, 1}, {"haplotype-support-mismatches", 0, 1}, {"haplotype-reads", 0, 1}, {"haplotype-read-mismatches", 0, 1}, {"variant-evidence", 0, 1}, {"variant-evidence-mismatches", 0, 1}, {"ranks", 0, 1}, {"rank", 0, 1}, {"rendezvous", 0, 1}, {"help", 'h', 0},
};
// -V: trace words per window of a batch whose longest window reference has `longest` bases.  512 words for the stage lines; MV_PATHS paths of
// up to longest + --max-indel-len + 256 bases (EngineCaps::path_cap), a byte per base plus the event and the padding; 16 words per reference
// base for the reads that run through a k-mer twice (8 words per line, the read once).  A window that needs more says so in its trace.
const uint32_t MV_PATHS = 32;
uint32_t trace_words_for(uint32_t longest, int max_indel_len) {
  const uint32_t w = 512u + MV_PATHS * ((longest + (uint32_t)max_indel_len + 256u + 3u) / 4u + 16u) + 16u * longest;
  return (w + 7u) / 8u * 8u;
}
// --haplotypes: words per window of such a batch: MV_PATHS haplotypes of up to longest + --max-indel-len + 256 bases, 16 bases to a word behind a header
uint32_t hap_words_for(uint32_t longest, int max_indel_len) {
  return MV_PATHS * ((uint32_t)LANCET_HAP_HEADER_WORDS + (longest + (uint32_t)max_indel_len + 256u + 15u) / 16u);
}
// --haplotype-sam: 64 more words per path for the runs of its CIGAR
uint32_t hap_cigar_words() { return MV_PATHS * 64u; }
// --haplotype-coverage: two words per base of every path and of its stretch (four 16-bit counts each)
uint32_t hap_cov_words(uint32_t longest, int max_indel_len) { return MV_PATHS * 2u * (2u * longest + (uint32_t)max_indel_len + 256u); }
// --haplotype-support: eight words per path
uint32_t hap_sup_words() { return MV_PATHS * 8u; }
// --variant-evidence: records kept per window (MV_PATHS paths of four events each; a buffer of its own, 72 bytes per record)
const uint32_t EVID_EVENTS = 128;
// --haplotype-sam: (name, length) of the contigs of a FASTA file in its order -- from its .fai when there is one, else from the file itself
bool fasta_contigs(const std::string &path, std::vector<std::pair<std::string, long>> *out) {
  out->clear();
  if (FILE *f = fopen((path + ".fai").c_str(), "r")) {
    char line[4096];
    while (fgets(line, sizeof line, f)) {
      char *t1 = strchr(line, '\t');
      if (!t1) continue;
      out->emplace_back(std::string(line, (size_t)(t1 - line)), atol(t1 + 1));
    }
    fclose(f);
    if (!out->empty()) return true;
  }
  FILE *f = fopen(path.c_str(), "r");
  if (!f) return false;
  std::vector<char> buf(1 << 16);
  bool bol = true, in_name = false, in_head = false;
  size_t n;
  while ((n = fread(buf.data(), 1, buf.size(), f)) > 0) for (size_t i = 0; i < n; ++i) {
    const char ch = buf[i];
    if (ch == '\n') { bol = true; in_name = in_head = false; continue; }
    if (bol && ch == '>') { out->emplace_back(std::string(), 0L); in_name = in_head = true; bol = false; continue; }
    bol = false;
    if (in_head) { if (in_name && !isspace((unsigned char)ch)) out->back().first += ch; else in_name = false; }
    else if (!out->empty() && ch != '\r') ++out->back().second;
  }
  fclose(f);
  return true;
}
int die(const std::string &m) { fprintf(stderr, "lancet_gpu: %s\n", m.c_str()); return 1; }
void usage() {
  fputs("Usage: lancet_gpu --tumor T.bam --normal N.bam --ref ref.fa (--reg chr:start-end | --bed regions.bed) [options] > out.vcf\n"
        "The reference's options with the reference's defaults (lancet --help), except:\n"
        "   --window-size, -w  <int>   : at most 1024 bp (the engine's per-window tables; the reference default is 600)\n"
        "   --max-k, -K        <int>   : at most 127; --min-k at least 3; --max-unit-length at most 8\n"
        "   --num-threads, -X  <int>   : accepted and ignored (windows are batched on the GPU)\n"
        "   --kmer-recovery, -R        : as in the reference (tumour k-mers seen once lend their occurrence to well-supported k-mers one\n"
        "                                low-quality base away); not together with --linked-reads\n"
        "   --more-verbose, -V         : -v plus the reference's -V lines: reads that run through a k-mer twice, what markRefEnds looked at and\n"
        "                                cut off, the reference and the path string of every path.  DIAGNOSTICS, not a throughput mode: every graph\n"
        "                                takes the general build (no LDS build kernel, no graphs built ahead); same VCF as without it\n"
        "   --print-graph, --node-str-len, --print-config-file: not offered\n"
        "Additional options:\n"
        "   --device <n> | --devices a,b,...  : GPU(s) to use; an entry may repeat (two engines on one GPU overlap the upload of a\n"
        "                                       batch with the kernels of the previous one)\n"
        "   --batch-windows <n>               : windows per engine batch [8192: a scan waits for the host side, and smaller batches keep two engines\n"
        "                                       on the GPU busy while the next batch is assembled; 32768 is what the kernels alone like best]\n"
        "   --strict                          : write no VCF when a window exceeded the engine's work space (default: finish,\n"
        "                                       list those windows on stderr, exit code 3)\n"
        "   --device-select                   : the alignments go to the GPU once and every batch's reads are picked there (LANCET_DEVICE_SELECT=1 does\n"
        "                                       the same); batches the device route does not take -- --linked-reads, --rg-file, reads left in the\n"
        "                                       graph by a window without mapped reads, oversize windows -- go the usual way; same VCF either way\n"
        "   --haplotypes <file>               : every assembled path of every window as FASTA (>chr:start-end|k=|comp=|path=|ref=off+len|variants=first+n),\n"
        "                                       at full throughput; same VCF, the option is left out of ##cmdline; not with --ranks above 1\n"
        "   --haplotype-sam <file>            : the same haplotypes as SAM records on the contig, CIGAR in = X I D as the window kernel aligned them;\n"
        "                                       alone or with --haplotypes, same rules\n"
        "   --haplotype-coverage <file>       : per haplotype its header line and the reference's -v table of per-base coverages (Pos r p d an+ an- at+ at-\n"
        "                                       rn+ rn- rt+ rt-); alone or with the other two, same rules; adds the tags nf nr tf tr to --haplotype-sam\n"
        "   --haplotype-support <file>        : per haplotype one line: its header and the reads that fit it / fit it alone among the paths of its k and\n"
        "                                       component, by class (fit_tf fit_tr fit_nf fit_nr alone_tf ...); alone or with the other three, same rules;\n"
        "                                       adds the tags sf sa to --haplotype-sam\n"
        "   --haplotype-support-mismatches <n>: mismatches an ungapped placement of a read on a path may have, 0 .. 255 [default: 5]\n"
        "   --haplotype-reads <file>          : SAM, one record per read that fits a haplotype: the read realigned through the path it fits best (tags hi ho\n"
        "                                       hm on hn: path, offset, mismatches, offsets and paths that are as good); alone or with the other four\n"
        "   --haplotype-read-mismatches <n>   : mismatches such a read may have on its path, 0 .. 255 [default: 5]\n"
        "   --variant-evidence <file>         : per record the reads that carry its allele, the reference allele or something else at its site, judged by the\n"
        "                                       haplotypes they fit (alt / ref / other by class Tf Tr Nf Nr); alone or with the other five, same rules;\n"
        "                                       adds the tag ev to --haplotype-sam\n"
        "   --variant-evidence-mismatches <n> : mismatches a read may have on the haplotypes it is judged by, 0 .. 255 [default: 5]\n"
        "   --ranks <n>                       : n processes, one per GPU; records gathered to rank 0 over RCCL, same VCF for every n\n"
        "   --rank <r> --rendezvous <path>    : this process is rank r of --ranks (a launcher starts the ranks; without --rank the\n"
        "                                       program starts them itself)\n"
        "BAM input: <bam>.bai / <stem>.bai is used when present (one seek per tiled stretch); otherwise the BAM is streamed once.\n"
        "There is no CPU path: a gfx950 device is required.\n", stderr);
}
}  // namespace

int main(int argc, char **argv) {
  std::string tumor, normal, ref, reg, bed, qrange = "!", date_line, devices, rg_file;
  int min_k = 11, max_k = 101, trim_lowqual = 10, min_base_qual = 17, tip_len = 11, cov_thr = 5, low_cov = 1, dfs_limit = 1000000;
  int max_indel_len = 500, max_mismatch = 2, max_unit_length = 4, min_report_unit = 3, min_report_len = 7, dist_from_str = 1;
  int device = 0, batch_windows = 8192, verbose = 0, more_verbose = 0, strict = 0, ranks = 0, rank = -1, kmer_recovery = 0;
  int device_select = (getenv("LANCET_DEVICE_SELECT") && atoi(getenv("LANCET_DEVICE_SELECT")) != 0) ? 1 : 0;
  std::string rendezvous, hap_file, sam_file, cov_file, sup_file, reads_file;
  int sup_mm = 5, reads_mm = 5, evid_mm = 5;
  std::string evid_file;
  double cov_ratio = 0.01;
  lancet_host_opts ho; lancet_host_opts_default(&ho);
  lancet_filters flt; lancet_filters_default(&flt);
  for (int i = 1; i < argc; ++i) {
    const char *a = argv[i];
    const Opt *o = nullptr;
    if (a[0] == '-' && a[1] == '-') { for (const Opt &c : OPTS) if (strcmp(a + 2, c.lng) == 0) o = &c; }
    else if (a[0] == '-' && a[1] && !a[2]) { for (const Opt &c : OPTS) if (c.shrt && c.shrt == a[1]) o = &c; }
    if (!o) return die(std::string("unknown option ") + a);
    const char *v = "";
    if (o->has_arg) { if (i + 1 >= argc) return die(std::string("option ") + a + " needs a value"); v = argv[++i]; }
    const std::string L = o->lng;
    if (L == "tumor") tumor = v; else if (L == "normal") normal = v; else if (L == "ref") ref = v; else if (L == "reg") reg = v;
    else if (L == "min-k") min_k = atoi(v); else if (L == "max-k") max_k = atoi(v); else if (L == "trim-lowqual") trim_lowqual = atoi(v);
    else if (L == "min-base-qual") min_base_qual = atoi(v); else if (L == "quality-range") qrange = v; else if (L == "min-map-qual") ho.min_map_qual = atoi(v);
    else if (L == "max-as-xs-diff") { /* accepted and without effect, as in the reference: its main() parses -Z but never hands it to the
                                         assemblers (src/Lancet.cc:865-918 lacks the MAX_DELTA_AS_XS line of :496), so the filter always uses 5 */ } else if (L == "tip-len") tip_len = atoi(v); else if (L == "cov-thr") cov_thr = atoi(v);
    else if (L == "cov-ratio") cov_ratio = atof(v); else if (L == "low-cov") low_cov = atoi(v); else if (L == "max-avg-cov") ho.max_avg_cov = atoi(v);
    else if (L == "window-size") ho.window_size = atoi(v); else if (L == "padding") ho.padding = atoi(v); else if (L == "dfs-limit") dfs_limit = atoi(v);
    else if (L == "max-indel-len") max_indel_len = atoi(v); else if (L == "max-mismatch") max_mismatch = atoi(v); else if (L == "num-threads") {}
    else if (L == "min-alt-count-tumor") flt.min_alt_cnt_tumor = atoi(v); else if (L == "max-alt-count-normal") flt.max_alt_cnt_normal = atoi(v);
    else if (L == "min-vaf-tumor") flt.min_vaf_tumor = atof(v); else if (L == "max-vaf-normal") flt.max_vaf_normal = atof(v);
    else if (L == "min-coverage-tumor") flt.min_cov_tumor = atoi(v); else if (L == "max-coverage-tumor") flt.max_cov_tumor = atoi(v);
    else if (L == "min-coverage-normal") flt.min_cov_normal = atoi(v); else if (L == "max-coverage-normal") flt.max_cov_normal = atoi(v);
    else if (L == "min-phred-fisher") flt.min_phred_fisher = atof(v); else if (L == "min-phred-fisher-str") flt.min_phred_fisher_str = atof(v);
    else if (L == "min-strand-bias") flt.min_strand_bias = (int)atof(v); else if (L == "max-unit-length") max_unit_length = atoi(v);
    else if (L == "min-report-unit") min_report_unit = atoi(v); else if (L == "min-report-len") min_report_len = atoi(v); else if (L == "dist-from-str") dist_from_str = atoi(v);
    else if (L == "linked-reads") ho.linked = 1; else if (L == "kmer-recovery") kmer_recovery = 1; else if (L == "primary-alignment-only") ho.primary_alignment_only = 1; else if (L == "XA-tag-filter") ho.xa_filter = 1;
    else if (L == "active-region-off") ho.active_region = 0; else if (L == "verbose") verbose = 1; else if (L == "more-verbose") { verbose = 1; more_verbose = 1; } else if (L == "device") device = atoi(v); else if (L == "devices") devices = v; else if (L == "batch-windows") batch_windows = atoi(v);
    else if (L == "date-line") date_line = v; else if (L == "bed") bed = v; else if (L == "rg-file") rg_file = v; else if (L == "strict") strict = 1; else if (L == "device-select") device_select = 1; else if (L == "haplotypes") hap_file = v; else if (L == "haplotype-sam") sam_file = v; else if (L == "haplotype-coverage") cov_file = v;
    else if (L == "haplotype-support") sup_file = v; else if (L == "haplotype-support-mismatches") sup_mm = atoi(v);
    else if (L == "haplotype-reads") reads_file = v; else if (L == "haplotype-read-mismatches") reads_mm = atoi(v);
    else if (L == "variant-evidence") evid_file = v; else if (L == "variant-evidence-mismatches") evid_mm = atoi(v);
    else if (L == "ranks") ranks = atoi(v); else if (L == "rank") rank = atoi(v); else if (L == "rendezvous") rendezvous = v;
    else if (L == "help") { usage(); return 0; }
  }
  if (tumor.empty() || normal.empty() || ref.empty() || (reg.empty() && bed.empty())) { usage(); return die("--tumor, --normal, --ref and a region (--reg) or BED file (--bed) are required"); }
  if (kmer_recovery && ho.linked) return die("--kmer-recovery (-R) is not supported together with --linked-reads: the linked-read coverages come out of the barcode replay, where recovery is not built");
  if (ranks < 0 || (ranks == 0 && rank >= 0) || (ranks > 0 && rank >= ranks)) return die("--ranks must be >= 1 and --rank one of 0 .. ranks-1");
  if (!hap_file.empty() && ranks > 1) return die("--haplotypes is not offered together with --ranks above 1: the gather to rank 0 carries records only (--devices a,b works)");
  if (!sam_file.empty() && ranks > 1) return die("--haplotype-sam is not offered together with --ranks above 1: the gather to rank 0 carries records only (--devices a,b works)");
  if (!cov_file.empty() && ranks > 1) return die("--haplotype-coverage is not offered together with --ranks above 1: the gather to rank 0 carries records only (--devices a,b works)");
  if (!sup_file.empty() && ranks > 1) return die("--haplotype-support is not offered together with --ranks above 1: the gather to rank 0 carries records only (--devices a,b works)");
  if (sup_mm < 0 || sup_mm > 255) return die("--haplotype-support-mismatches must be 0 .. 255");
  if (!reads_file.empty() && ranks > 1) return die("--haplotype-reads is not offered together with --ranks above 1: the gather to rank 0 carries records only (--devices a,b works)");
  if (reads_mm < 0 || reads_mm > 255) return die("--haplotype-read-mismatches must be 0 .. 255");
  if (!evid_file.empty() && ranks > 1) return die("--variant-evidence is not offered together with --ranks above 1: the gather to rank 0 carries records only (--devices a,b works)");
  if (evid_mm < 0 || evid_mm > 255) return die("--variant-evidence-mismatches must be 0 .. 255");
  if (ranks > 0 && rank < 0) {
    // the launcher: rank r = this program again with --rank r --rendezvous <path>; rank 0 writes the VCF to the stdout they all inherit
    if (rendezvous.empty()) {
      const char *shm = access("/dev/shm", W_OK) == 0 ? "/dev/shm" : "/tmp";
      rendezvous = std::string(shm) + "/lancet_gpu_" + std::to_string((long)getpid()) + ".id";
    }
    unlink(rendezvous.c_str());
    std::vector<pid_t> kids;
    for (int r = 0; r < ranks; ++r) {
      const pid_t pid = fork();
      if (pid < 0) return die("fork failed");
      if (pid == 0) {
        std::vector<std::string> av(argv, argv + argc);
        av.push_back("--rank"); av.push_back(std::to_string(r)); av.push_back("--rendezvous"); av.push_back(rendezvous);
        std::vector<char *> cv; for (std::string &x : av) cv.push_back(&x[0]); cv.push_back(nullptr);
        execv("/proc/self/exe", cv.data());
        _exit(127);
      }
      kids.push_back(pid);
    }
    // a rank that fails (exit code other than 0 / 3: bad input, no device, a communicator that does not come up) takes the others with it --
    // they would wait for it at the rendezvous or in the gather
    int worst = 0; size_t left = kids.size();
    while (left > 0) {
      int st = 0;
      const pid_t k = waitpid(-1, &st, 0);
      if (k < 0) { worst = worst ? worst : 1; break; }
      if (std::find(kids.begin(), kids.end(), k) == kids.end()) continue;
      --left;
      const int c = WIFEXITED(st) ? WEXITSTATUS(st) : 1;
      if (c && (!worst || c == 1 || worst == 3)) worst = c;
      if (c != 0 && c != 3) for (pid_t o : kids) if (o != k) kill(o, SIGTERM);
    }
    unlink(rendezvous.c_str());
    return worst;
  }
  if (ranks > 0 && rendezvous.empty()) return die("--rank needs --rendezvous <path> (the same path for every rank)");
  const int qoff = qrange.empty() ? 33 : (unsigned char)qrange[0];
  lancet_params P; lancet_params_default(&P);
  P.min_k = min_k; P.max_k = max_k; P.max_tip_len = tip_len; P.cov_threshold = cov_thr; P.low_cov_threshold = low_cov; P.dfs_limit = dfs_limit;
  P.max_indel_len = max_indel_len; P.max_mismatch = max_mismatch; P.min_qual_trim = trim_lowqual + qoff; P.min_qual_call = min_base_qual + qoff;
  P.max_unit_len = max_unit_length; P.min_report_units = min_report_unit; P.min_report_len = min_report_len; P.dist_from_str = dist_from_str;
  P.lr_mode = ho.linked; P.kmer_recovery = kmer_recovery; P.min_cov_ratio = cov_ratio;
  ho.max_k = max_k; ho.min_evidence = flt.min_alt_cnt_tumor; ho.min_qual_call = min_base_qual + qoff;

  const bool timing = getenv("LANCET_HOST_TIMING") != nullptr;
  auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  double t_batch = 0, t_engine = 0, t_vdb = 0; float t_kernel = 0;
  const double t_start = now();
  // one engine per entry of --devices (default: --device); an entry may repeat a device (two engines on one GPU overlap the
  // upload of a batch with the kernels of the previous one).  Batches go to the engines in turn; there is no CPU path:
  // without a GPU engine creation fails.
  std::vector<int> devs;
  if (devices.empty()) devs.push_back(ranks > 0 ? rank : device);
  else { size_t p0 = 0; while (p0 <= devices.size()) { size_t q = devices.find(',', p0); if (q == std::string::npos) q = devices.size(); if (q > p0) devs.push_back(atoi(devices.substr(p0, q - p0).c_str())); p0 = q + 1; } }
  if (devs.empty()) return die("--devices is empty");
  if (ranks > 0) { const int d = devs[(size_t)rank % devs.size()]; devs.assign(1, d); }     // one GPU per rank
  // The communicator comes up on a thread of its own while this one decodes, tiles and assembles (loading librccl and ncclCommInitRank take
  // about a second and a half, and nothing needs the communicator before the gather at the end); a rank that cannot join reports it there --
  // the others then fail in ncclCommInitRank or time out at the rendezvous.
  const bool ranked = ranks > 0;
  lancet_comm *comm = nullptr;
  char cerr[512] = "";
  std::future<lancet_comm *> comm_fut;
  if (ranked) {
    if (ranks > 1 && !getenv("LANCET_HOST_LAZY")) setenv("LANCET_HOST_LAZY", "1", 0);     // a rank loads what ITS windows select, once (lancet_host_load_range; needs both .bai, else a notice and everything is loaded)
    const int cdev = devs[0];                                                                // (the environment is settled before the thread starts: it reads it)
    comm_fut = std::async(std::launch::async, [=, &cerr]() { return lancet_comm_create(rank, ranks, cdev, rendezvous.c_str(), 300.0, cerr, sizeof cerr); });
  }
  std::vector<lancet_engine *> engs;
  for (int d : devs) {
    lancet_engine *e = nullptr;
    const int rc = lancet_engine_create(&P, d, &e);
    if (rc == LANCET_E_UNSUPPORTED) return die("unsupported parameters: --max-k must be <= 127, --min-k >= 3, --max-unit-length <= 8");
    if (rc != LANCET_OK) return die(std::string("cannot create the MI355X engine on device ") + std::to_string(d) + " (code " + std::to_string(rc) + "): " + (e ? lancet_engine_last_error(e) : "no gfx950 device / HIP runtime"));
    if (verbose && !more_verbose) lancet_engine_set_trace(e, 1u << 17);            // -v: the reference's per-window stage trace, to stderr (-V: set per batch, below)
    engs.push_back(e);
  }
  char err[512] = "";
  lancet_host *H = lancet_host_open(tumor.c_str(), normal.c_str(), ref.c_str(), err, sizeof err);
  if (H && !rg_file.empty() && lancet_host_set_rg_file(H, rg_file.c_str()) != LANCET_OK) return die(lancet_host_last_error(H));
  if (!H) return die(err);
  const double t_tile0 = now();
  const char *regs[1] = {reg.c_str()};
  const int nwin = lancet_host_tile_regions(H, bed.empty() ? nullptr : bed.c_str(), regs, reg.empty() ? 0 : 1, &ho);
  const double t_tile = now() - t_tile0;
  if (nwin < 0) return die(lancet_host_last_error(H));
  if (ho.active_region && !lancet_host_first_has_md(H, 1) && !lancet_host_first_has_md(H, 0)) {      // reference src/Lancet.cc:817-825
    fputs("\n--------WARNING--------\nThe MD tag is required to select the active regions, but is missing from the alignments in the BAM(s) file(s).\n"
          "To avoid unpredictable behavior, the active region module has been automatically turned off (--active-region-off)\n-----------------------\n\n", stderr);
    ho.active_region = 0;
  }
  lancet_vdb *db = lancet_vdb_create(&flt);
  int n_chr = 0;
  const char *const *chr_names = lancet_host_chroms(H, &n_chr);
  const int step = batch_windows > 0 ? batch_windows : 1;
  const int nchunks = (nwin + step - 1) / step;
  // a scan of several batches on one GPU: a second engine on the same device, so that the upload / trim of batch i+1 and the tail
  // of its kernels overlap with batch i (what `--devices 0,0` asks for explicitly; bench.py --in-flight 2 measures it)
  if (devices.empty() && nchunks > 1 && engs.size() == 1) {
    lancet_engine *e2 = nullptr;
    if (lancet_engine_create(&P, devs[0], &e2) == LANCET_OK) { if (verbose && !more_verbose) lancet_engine_set_trace(e2, 1u << 17); engs.push_back(e2); }
  }
  FILE *hap_out = nullptr;
  if (!hap_file.empty() && !(hap_out = fopen(hap_file.c_str(), "w"))) return die("cannot write " + hap_file);
  FILE *sam_out = nullptr, *reads_out = nullptr;
  for (int q = 0; q < 2; ++q) {                          // --haplotype-sam and --haplotype-reads: one header
    const std::string &file = q == 0 ? sam_file : reads_file;
    if (file.empty()) continue;
    std::vector<std::pair<std::string, long>> contigs;
    if (!fasta_contigs(ref, &contigs)) return die("cannot read " + ref);
    FILE *f = fopen(file.c_str(), "w");
    if (!f) return die("cannot write " + file);
    fputs("@HD\tVN:1.6\tSO:unsorted\n", f);
    for (const auto &ct : contigs) fprintf(f, "@SQ\tSN:%s\tLN:%ld\n", ct.first.c_str(), ct.second);
    fputs("@PG\tID:lancet_gpu\tPN:lancet_gpu\n", f);
    (q == 0 ? sam_out : reads_out) = f;
  }
  FILE *cov_out = nullptr;
  if (!cov_file.empty() && !(cov_out = fopen(cov_file.c_str(), "w"))) return die("cannot write " + cov_file);
  FILE *sup_out = nullptr;
  if (!sup_file.empty() && !(sup_out = fopen(sup_file.c_str(), "w"))) return die("cannot write " + sup_file);
  if (sup_out) fputs("#haplotype\tfit_tf\tfit_tr\tfit_nf\tfit_nr\talone_tf\talone_tr\talone_nf\talone_nr\n", sup_out);
  FILE *evid_out = nullptr;
  if (!evid_file.empty() && !(evid_out = fopen(evid_file.c_str(), "w"))) return die("cannot write " + evid_file);
  if (evid_out) fputs("#window\tchrom\tpos\tcode\tref\talt\tk\tcomponent\tpath\talt_Tf\talt_Tr\talt_Nf\talt_Nr\tref_Tf\tref_Tr\tref_Nf\tref_Nr\tother_Tf\tother_Tr\tother_Nf\tother_Nr\n", evid_out);
  const bool sam_on = sam_out != nullptr, cov_on = cov_out != nullptr, sup_on = sup_out != nullptr, reads_on = reads_out != nullptr, evid_on = evid_out != nullptr;
  const bool aln_on = sam_on || cov_on || reads_on || evid_on;      // the table is laid out by the alignment's columns; a read's CIGAR goes through its path's; events are runs of CIGAR words
  long n_evid = 0, n_evid_marked = 0, n_evid_uneval = 0;          // --variant-evidence: lines written, windows with more events than EVID_EVENTS, events of groups beyond the kernel's lists
  const bool hap_on = hap_out != nullptr || aln_on || sup_on;      // any of the files turns the capture on; the SAM and the coverage one the alignments as well
  auto hap_extra_for = [&](uint32_t longest) -> uint32_t { return (aln_on ? hap_cigar_words() : 0u) + (cov_on ? hap_cov_words(longest, max_indel_len) : 0u) + (sup_on ? hap_sup_words() : 0u); };
  long n_hap_reads = 0;                            // --haplotype-reads: records written
  long n_hap = 0, n_hap_truncated = 0;             // --haplotypes: records written, windows whose haplotypes did not all fit hap_words_for
  struct Job { bool have = false; std::string trace; std::string hapfa; /* --haplotypes: the batch's FASTA records */ std::string hapsam; /* --haplotype-sam: its SAM records */ std::string hapcov; /* --haplotype-coverage: its tables */ std::string hapsup; /* --haplotype-support: its lines */ std::string hapreads; /* --haplotype-reads: its SAM records */ std::string evid; /* --variant-evidence: its lines */ std::vector<lancet_variant> v; std::string blob; std::vector<lancet_variant_lr> lr; std::vector<uint32_t> bx; std::vector<std::string> bxn;
               std::vector<int64_t> widx; /* --ranks: tiled (= global) number of the batch's window w */ };
  std::vector<std::vector<uint8_t>> parts;      // --ranks: this rank's batches, packed (lancet_records_pack), in batch order
  struct Slot { lancet_engine *e = nullptr; std::future<int> fut; int chunk = -1; int nk = 0; long base = 0; std::vector<int32_t> kept; std::vector<std::string> bxn;
                std::vector<std::string> raw; /* -V: Ref_t::rawseq of the batch's window w (the level-2 events refer to it by offset) */
                std::vector<uint32_t> rd_woff, rd_bases; /* --haplotype-reads: where read r of the batch starts in the packed words, and those words */ };
  std::vector<Job> jobs((size_t)nchunks);
  std::vector<Slot> slots(engs.size());
  for (size_t k = 0; k < engs.size(); ++k) { slots[k].e = engs[k]; slots[k].kept.resize((size_t)step); }
  long done = 0;
  std::map<int, lancet_engine *> last_on_dev;      // device -> the engine submitted last on it
  int next_add = 0;
  std::string fail;
  std::vector<std::string> overflowed;
  long n_truncated = 0;                            // -V: windows whose trace did not fit the batch's trace_words_for
  // results of a finished run are copied out (the engine's buffers live until its next upload) and added to the
  // VariantDB strictly in chunk order: addVar order is window order
  auto finish = [&](Slot &sl) -> bool {
    const double t0 = now();
    const int rc = sl.fut.get();
    t_engine += now() - t0;
    if (rc != LANCET_OK) { fail = std::string("engine: ") + lancet_engine_last_error(sl.e); return false; }
    { float tm[2] = {0, 0}; lancet_engine_last_timing(sl.e, tm); t_kernel += tm[0]; }
    const lancet_variant *v; uint32_t nv, blen; const char *blob; const lancet_window_stats *st;
    if (lancet_engine_results(sl.e, &v, &nv, &blob, &blen, &st) != LANCET_OK) { fail = std::string("engine: ") + lancet_engine_last_error(sl.e); return false; }
    for (int w = 0; w < sl.nk; ++w) if (st[w].status < 0) {
      if (strict) { fail = std::string("work-space overflow in window ") + lancet_host_window_hdr(H, sl.kept[(size_t)w]) + ": results withheld (--strict)"; return false; }
      overflowed.push_back(lancet_host_window_hdr(H, sl.kept[(size_t)w]));      // the window emitted nothing (the engine drops a window's records when it overflows)
    }
    Job &j = jobs[(size_t)sl.chunk];
    j.v.assign(v, v + nv); j.blob.assign(blob, blen);
    if (ranked) j.widx.assign(sl.kept.begin(), sl.kept.begin() + sl.nk);
    if (ho.linked) {
      const lancet_variant_lr *lr; const uint32_t *bxb; uint32_t bxl;
      if (lancet_engine_results_lr(sl.e, &lr, &bxb, &bxl) != LANCET_OK) { fail = std::string("engine: ") + lancet_engine_last_error(sl.e); return false; }
      j.lr.assign(lr, lr + nv); j.bx.assign(bxb, bxb + bxl); j.bxn.swap(sl.bxn);
    }
    if (verbose) {
      const uint32_t *elen, *evt; uint32_t wpw = 0;
      if (lancet_engine_trace(sl.e, &elen, &evt, &wpw) == LANCET_OK && wpw) for (int w = 0; w < sl.nk; ++w) {
        const int tw = sl.kept[(size_t)w];
        const char *hdr = lancet_host_window_hdr(H, tw);
        int32_t start = 0, end = 0; lancet_host_window_span(H, tw, &start, &end);
        const bool l2 = more_verbose && (size_t)w < sl.raw.size();
        if (l2 && elen[w] == wpw) ++n_truncated;
        char *t = l2 ? lancet_trace_format2(evt + (size_t)w * wpw, elen[w], wpw, (int32_t)(sl.base + w + 1), hdr, chr_names[lancet_host_window_chrom(H, tw)], start, end, dfs_limit,
                                            sl.raw[(size_t)w].data(), (uint32_t)sl.raw[(size_t)w].size())
                     : lancet_trace_format(evt + (size_t)w * wpw, elen[w], (int32_t)(sl.base + w + 1), hdr, chr_names[lancet_host_window_chrom(H, tw)], start, end, dfs_limit);
        if (t) { j.trace += t; lancet_free(t); }
      }
    }
    if (hap_on) {
      const lancet_haplotype *hp; uint32_t nh = 0, nwords = 0; const uint32_t *words; const uint8_t *trunc;
      if (lancet_engine_results_haplotypes(sl.e, &hp, &nh, &words, &nwords, &trunc) != LANCET_OK) { fail = std::string("engine: ") + lancet_engine_last_error(sl.e); return false; }
      const uint32_t *cig_off = nullptr, *cig = nullptr; uint32_t ncig = 0;
      if (aln_on && lancet_engine_results_haplotype_alignments(sl.e, &cig_off, &cig, &ncig) != LANCET_OK) { fail = std::string("engine: ") + lancet_engine_last_error(sl.e); return false; }
      const uint32_t *cov_off = nullptr; const uint16_t *cov = nullptr; uint32_t ncov = 0;
      if (cov_on && lancet_engine_results_haplotype_coverage(sl.e, &cov_off, &cov, &ncov) != LANCET_OK) { fail = std::string("engine: ") + lancet_engine_last_error(sl.e); return false; }
      const uint32_t *sup = nullptr;
      if (sup_on && lancet_engine_results_haplotype_support(sl.e, &sup) != LANCET_OK) { fail = std::string("engine: ") + lancet_engine_last_error(sl.e); return false; }
      for (int w = 0; w < sl.nk; ++w) if (trunc[w]) ++n_hap_truncated;
      const lancet_variant_evidence *evd = nullptr; uint32_t nevd = 0; const uint32_t *ev_off = nullptr; const uint8_t *ev_marked = nullptr;
      if (evid_on) {
        if (lancet_engine_results_haplotype_evidence(sl.e, &evd, &nevd, &ev_off, &ev_marked) != LANCET_OK) { fail = std::string("engine: ") + lancet_engine_last_error(sl.e); return false; }
        for (int w = 0; w < sl.nk; ++w) if (ev_marked[w]) ++n_evid_marked;
        for (uint32_t q = 0; q < nevd; ++q) if (evd[q].flags & LANCET_EVID_UNEVALUATED) ++n_evid_uneval;
      }
      if (reads_on) {
        // the reads' records: each placed read through its haplotype's CIGAR (lc_read_cigar), with --haplotype-sam's coordinates
        const lancet_read_placement *pl = nullptr; uint32_t npl = 0; const uint32_t *prb = nullptr; const uint16_t *ptl = nullptr;
        if (lancet_engine_results_haplotype_placements(sl.e, &pl, &npl, &prb, &ptl) != LANCET_OK) { fail = std::string("engine: ") + lancet_engine_last_error(sl.e); return false; }
        std::vector<uint32_t> first((size_t)sl.nk + 1, nh);       // haplotype i of window w is hp[first[w] + i]
        for (uint32_t i = nh; i-- > 0;) if (hp[i].window >= 0 && hp[i].window < sl.nk) first[(size_t)hp[i].window] = i;
        std::vector<uint32_t> ops; std::string seq; char head[320];
        for (int w = 0; pl && w < sl.nk; ++w) {
          const int tw = sl.kept[(size_t)w];
          const char *hdr = lancet_host_window_hdr(H, tw);
          int32_t start = 0, end = 0; lancet_host_window_span(H, tw, &start, &end);
          for (uint32_t r = prb[w]; r < prb[w + 1] && r < npl && r < sl.rd_woff.size(); ++r) {
            const lancet_read_placement &x = pl[r];
            if (x.haplotype < 0) continue;
            const uint32_t hi = first[(size_t)w] + (uint32_t)x.haplotype;
            if (hi >= nh || hp[hi].window != w || hp[hi].index_in_window != x.haplotype || cig_off[hi + 1] > ncig) continue;
            const lancet_haplotype &h = hp[hi];
            uint32_t start0 = 0;
            (void)lc_read_cigar(x.offset, ptl[r], h.len, h.ref_off, cig + cig_off[hi], cig_off[hi + 1] - cig_off[hi], &start0, &ops);
            const uint32_t *rw = sl.rd_bases.data() + sl.rd_woff[r];
            seq.assign((size_t)ptl[r], 'A');
            for (uint32_t b = 0; b < ptl[r]; ++b) seq[b] = "ACGT"[(rw[b / 16u] >> (2u * (b % 16u))) & 3u];
            snprintf(head, sizeof head, "%s|r=%u\t%d\t%s\t%ld\t255\t", hdr, r - prb[w], (x.cls & 1u) ? 16 : 0, chr_names[lancet_host_window_chrom(H, tw)], (long)start + (long)start0);
            j.hapreads += head;
            for (uint32_t op : ops) { j.hapreads += std::to_string(op >> 4); j.hapreads += (op & 15u) == LC_RC_M ? 'M' : (op & 15u) == LC_RC_I ? 'I' : (op & 15u) == LC_RC_D ? 'D' : 'S'; }
            j.hapreads += "\t*\t0\t0\t"; j.hapreads += seq;
            snprintf(head, sizeof head, "\t*\twn:Z:%s\thi:i:%d\tkk:i:%u\tcp:i:%u\tho:i:%d\thm:i:%u\ton:i:%u\thn:i:%u\tsm:A:%c\n", hdr, x.haplotype, (unsigned)h.kmer, (unsigned)h.component,
                     x.offset, (unsigned)x.mismatches, (unsigned)x.n_offsets, (unsigned)x.n_haplotypes, (x.cls & 2u) ? 'N' : 'T');
            j.hapreads += head;
            ++n_hap_reads;
          }
        }
      }
      for (uint32_t i = 0; i < nh; ++i) {
        const lancet_haplotype &x = hp[i];
        if (x.window < 0 || x.window >= sl.nk || (uint64_t)x.word_off + (x.len + 15u) / 16u > nwords) continue;
        const int tw = sl.kept[(size_t)x.window];
        const char *hdr = lancet_host_window_hdr(H, tw);
        char head[256];
        std::string seq((size_t)x.len, 'A');
        for (uint32_t b = 0; b < x.len; ++b) seq[b] = "ACGT"[(words[x.word_off + b / 16u] >> (2u * (b % 16u))) & 3u];
        // the haplotype's coverages: 4 per path base (an+ an- at+ at-), then 4 per base of the stretch (rn+ rn- rt+ rt-)
        const uint32_t e0 = (evd && ev_off[i + 1] <= nevd) ? ev_off[i] : 0u, e1 = (evd && ev_off[i + 1] <= nevd) ? ev_off[i + 1] : 0u;      // the haplotype's events
        for (uint32_t q = e0; q < e1; ++q) {
          const lancet_variant_evidence &ev = evd[q];
          if (ev.variant < 0 || (uint32_t)ev.variant >= nv) continue;
          const lancet_variant &r = v[ev.variant];
          j.evid += hdr; j.evid += '\t'; j.evid += chr_names[lancet_host_window_chrom(H, tw)]; j.evid += '\t'; j.evid += std::to_string(r.pos); j.evid += '\t'; j.evid += (char)r.code; j.evid += '\t';
          j.evid.append(blob + r.ref_off, r.ref_len); j.evid += '\t'; j.evid.append(blob + r.alt_off, r.alt_len);
          snprintf(head, sizeof head, "\t%u\t%u\t%d", (unsigned)x.kmer, (unsigned)x.component, x.index_in_window);
          j.evid += head;
          for (int c = 0; c < 4; ++c) { j.evid += '\t'; j.evid += std::to_string(ev.alt[c]); }
          for (int c = 0; c < 4; ++c) { j.evid += '\t'; j.evid += std::to_string(ev.ref[c]); }
          for (int c = 0; c < 4; ++c) { j.evid += '\t'; j.evid += std::to_string(ev.other[c]); }
          j.evid += '\n';
          ++n_evid;
        }
        const uint16_t *pcv = nullptr, *rcv = nullptr;
        if (cov_on && cov_off[i + 1] <= ncov && cov_off[i + 1] - cov_off[i] == 4u * (x.len + x.ref_len)) { pcv = cov + cov_off[i]; rcv = pcv + 4u * (size_t)x.len; }
        if (hap_out) {
          snprintf(head, sizeof head, ">%s|k=%u|comp=%u|path=%d|ref=%u+%u|variants=%d+%d\n", hdr, (unsigned)x.kmer, (unsigned)x.component,
                   x.index_in_window, x.ref_off, x.ref_len, x.first_variant, x.n_variants);
          j.hapfa += head; j.hapfa += seq; j.hapfa += '\n';
        }
        if (sam_on) {
          // the engine's runs; a D run at either end is no part of a read's alignment, and POS moves past a leading one
          uint32_t c0 = cig_off[i], c1 = cig_off[i + 1];
          if (c1 > ncig || c0 > c1) continue;
          int32_t start = 0, end = 0; lancet_host_window_span(H, tw, &start, &end);
          long pos = (long)start + (long)x.ref_off;      // 1-based: a record of the window sits at pos + 1 - this in the stretch (0-based pos)
          if (c0 < c1 && (cig[c0] & 15u) == LANCET_HAP_OP_D) { pos += (long)(cig[c0] >> 4); ++c0; }
          if (c0 < c1 && (cig[c1 - 1] & 15u) == LANCET_HAP_OP_D) --c1;
          snprintf(head, sizeof head, "%s|k=%u|comp=%u|path=%d\t0\t%s\t%ld\t255\t", hdr, (unsigned)x.kmer, (unsigned)x.component, x.index_in_window,
                   chr_names[lancet_host_window_chrom(H, tw)], pos);
          j.hapsam += head;
          if (c0 == c1) j.hapsam += '*';
          for (uint32_t q = c0; q < c1; ++q) {
            const uint32_t op = cig[q] & 15u;
            j.hapsam += std::to_string(cig[q] >> 4);
            j.hapsam += op == LANCET_HAP_OP_EQ ? '=' : op == LANCET_HAP_OP_X ? 'X' : op == LANCET_HAP_OP_I ? 'I' : 'D';
          }
          j.hapsam += "\t*\t0\t0\t"; j.hapsam += seq;
          snprintf(head, sizeof head, "\t*\tkk:i:%u\tcp:i:%u\tpi:i:%d\twn:Z:%s\tvf:i:%d\tvn:i:%d\tfl:i:%u", (unsigned)x.kmer, (unsigned)x.component, x.index_in_window, hdr,
                   x.first_variant, x.n_variants, x.flags);
          j.hapsam += head;
          if (pcv) for (int q = 0; q < 4; ++q) {          // --haplotype-coverage as well: the path's an+ an- at+ at-, one value per SEQ base
            j.hapsam += q == 0 ? "\tnf:B:S" : q == 1 ? "\tnr:B:S" : q == 2 ? "\ttf:B:S" : "\ttr:B:S";
            for (uint32_t b = 0; b < x.len; ++b) { j.hapsam += ','; j.hapsam += std::to_string((unsigned)pcv[4u * b + (uint32_t)q]); }
          }
          if (sup) for (int q = 0; q < 2; ++q) {           // --haplotype-support as well: fit and alone, Tf Tr Nf Nr
            j.hapsam += q == 0 ? "\tsf:B:I" : "\tsa:B:I";
            for (int c = 0; c < 4; ++c) { j.hapsam += ','; j.hapsam += std::to_string(sup[8u * (size_t)i + 4u * (uint32_t)q + (uint32_t)c]); }
          }
          for (uint32_t q = e0; q < e1; ++q) {               // --variant-evidence as well: the events, rb,rs,pb,ps,flags and alt ref other by Tf Tr Nf Nr
            const lancet_variant_evidence &ev = evd[q];
            j.hapsam += q == e0 ? "\tev:Z:" : ";";
            snprintf(head, sizeof head, "%u,%u,%u,%u,%u", ev.rb, ev.rs, ev.pb, ev.ps, ev.flags);
            j.hapsam += head;
            for (int c = 0; c < 12; ++c) { j.hapsam += ','; j.hapsam += std::to_string(c < 4 ? ev.alt[c] : c < 8 ? ev.ref[c - 4] : ev.other[c - 8]); }
          }
          j.hapsam += '\n';
        }
        if (sup_on) {
          snprintf(head, sizeof head, "%s|k=%u|comp=%u|path=%d|ref=%u+%u", hdr, (unsigned)x.kmer, (unsigned)x.component, x.index_in_window, x.ref_off, x.ref_len);
          j.hapsup += head;
          for (int c = 0; c < 8; ++c) { j.hapsup += '\t'; j.hapsup += std::to_string(sup ? sup[8u * (size_t)i + (uint32_t)c] : 0u); }
          j.hapsup += '\n';
        }
        if (cov_on) {
          // the reference's table (printVerticalAlignment): Pos is the path index and stays on a deletion column; the side with a gap has empty cells
          const uint32_t c0 = cig_off[i], c1 = cig_off[i + 1];
          const std::string *raw = (size_t)x.window < sl.raw.size() ? &sl.raw[(size_t)x.window] : nullptr;
          const bool ok = pcv && c1 <= ncig && c0 <= c1 && raw && (uint64_t)x.ref_off + x.ref_len <= raw->size();      // (else: no table, the haplotype still counts)
          snprintf(head, sizeof head, ">%s|k=%u|comp=%u|path=%d|ref=%u+%u\n", hdr, (unsigned)x.kmer, (unsigned)x.component, x.index_in_window, x.ref_off, x.ref_len);
          std::string &o = j.hapcov;
          if (ok) { o += head; o += "Pos\tr\tp\td\tan+\tan-\tat+\tat-\trn+\trn-\trt+\trt-\n"; }
          uint32_t pk = 0, rj = 0;
          auto four = [&](const uint16_t *v) { for (int q = 0; q < 4; ++q) { o += '\t'; if (v) o += std::to_string((unsigned)v[q]); } };
          for (uint32_t q = c0; ok && q < c1; ++q) {
            const uint32_t op = cig[q] & 15u;
            const bool ins = op == LANCET_HAP_OP_I, del = op == LANCET_HAP_OP_D;
            for (uint32_t n = cig[q] >> 4; n > 0 && (del || pk < x.len) && (ins || rj < x.ref_len); --n) {
              o += std::to_string(pk); o += '\t';
              o += ins ? '-' : (char)toupper((unsigned char)(*raw)[x.ref_off + rj]); o += '\t';
              o += del ? '-' : seq[pk]; o += '\t';
              o += ins ? '^' : del ? 'v' : op == LANCET_HAP_OP_EQ ? ' ' : 'x';
              four(del ? nullptr : pcv + 4u * pk); four(ins ? nullptr : rcv + 4u * rj);
              o += '\n';
              if (!del) ++pk;
              if (!ins) ++rj;
            }
          }
        }
        ++n_hap;
      }
    }
    j.have = true; sl.chunk = -1;
    return true;
  };
  auto flush = [&]() -> bool {
    const double t0 = now();
    while (next_add < nchunks && jobs[(size_t)next_add].have) {
      Job &j = jobs[(size_t)next_add];
      if (!j.trace.empty()) fputs(j.trace.c_str(), stderr);
      if (!j.hapfa.empty() && fwrite(j.hapfa.data(), 1, j.hapfa.size(), hap_out) != j.hapfa.size()) { fail = "cannot write " + hap_file; return false; }
      if (!j.hapsam.empty() && fwrite(j.hapsam.data(), 1, j.hapsam.size(), sam_out) != j.hapsam.size()) { fail = "cannot write " + sam_file; return false; }
      if (!j.hapreads.empty() && fwrite(j.hapreads.data(), 1, j.hapreads.size(), reads_out) != j.hapreads.size()) { fail = "cannot write " + reads_file; return false; }
      if (!j.hapsup.empty() && fwrite(j.hapsup.data(), 1, j.hapsup.size(), sup_out) != j.hapsup.size()) { fail = "cannot write " + sup_file; return false; }
      if (!j.evid.empty() && fwrite(j.evid.data(), 1, j.evid.size(), evid_out) != j.evid.size()) { fail = "cannot write " + evid_file; return false; }
      if (!j.hapcov.empty() && fwrite(j.hapcov.data(), 1, j.hapcov.size(), cov_out) != j.hapcov.size()) { fail = "cannot write " + cov_file; return false; }
      int arc = LANCET_OK;
      if (ranked) {                                  // the records travel: keyed, reduced, window numbers of the whole tiling
        if (!j.v.empty()) {
          std::vector<const char *> names; for (auto &n : j.bxn) names.push_back(n.c_str());
          uint8_t *pb = nullptr; size_t pl = 0;
          arc = lancet_records_pack(j.v.data(), (uint32_t)j.v.size(), j.blob.data(), (uint32_t)j.blob.size(), ho.linked ? j.lr.data() : nullptr, ho.linked ? j.bx.data() : nullptr,
                                    ho.linked ? names.data() : nullptr, (uint32_t)names.size(), chr_names, n_chr, j.widx.data(), (uint32_t)j.widx.size(), 1, &pb, &pl);
          if (arc == LANCET_OK) { parts.emplace_back(pb, pb + pl); lancet_free(pb); }
        }
      } else
      if (!j.v.empty()) {
        if (ho.linked) {
          std::vector<const char *> names; for (auto &n : j.bxn) names.push_back(n.c_str());
          arc = lancet_vdb_add_lr(db, j.v.data(), j.lr.data(), (uint32_t)j.v.size(), j.blob.c_str(), j.bx.data(), names.data(), (uint32_t)names.size(), chr_names, (uint32_t)n_chr);
        } else arc = lancet_vdb_add(db, j.v.data(), (uint32_t)j.v.size(), j.blob.c_str(), chr_names, (uint32_t)n_chr);
      }
      if (arc != LANCET_OK) { fail = "VariantDB rejected the records"; return false; }
      j = Job(); j.have = true;
      ++next_add;
    }
    t_vdb += now() - t0;
    return true;
  };
  // The host threads that assemble a batch also trim and pack its reads (lancet_host_batch_packed -> lancet_engine_upload_packed: 3 bits per
  // base handed over, one pass over the reads instead of two); LANCET_GPU_ASCII=1, or trim + pack on the device (LANCET_PREP=device), keep
  // the ASCII hand-over.
  const bool packed = getenv("LANCET_GPU_ASCII") == nullptr && !(getenv("LANCET_PREP") && strcmp(getenv("LANCET_PREP"), "device") == 0);
  // --ranks: rank r owns one contiguous run of batches -- in the table's order (header strings) that is a run of contigs, whose alignments
  // the rank loads once; the records then reach rank 0 in window order, rank by rank
  const int c_lo = ranked ? (int)((long)nchunks * rank / ranks) : 0, c_hi = ranked ? (int)((long)nchunks * (rank + 1) / ranks) : nchunks;
  if (ranked && c_hi > c_lo && lancet_host_load_range(H, c_lo * step, c_hi * step < nwin ? c_hi * step : nwin, &ho) != LANCET_OK) return die(lancet_host_last_error(H));
  // --device-select: what is loaded goes to every GPU in use once; a batch is then a list of windows
  std::map<int, lancet_device_reads *> dev_reads;
  std::map<std::string, long> not_taken;            // reason (up to its first ':') -> batches
  long n_taken = 0;
  if (device_select && packed && !ho.linked) {
    const double t0 = now();
    lancet_alignment_table tab;
    if (lancet_host_alignment_table(H, &ho, &P, &tab) != LANCET_OK) return die(lancet_host_last_error(H));
    const double t1 = now();
    for (int d : devs) if (!dev_reads.count(d)) {
      lancet_device_reads *dr = nullptr;
      const int rc = lancet_device_reads_create(d, &tab, &dr);
      if (rc != LANCET_OK) return die(std::string("cannot make the alignments resident on device ") + std::to_string(d) + " (code " + std::to_string(rc) + "): " + lancet_engine_last_error(nullptr));
      dev_reads[d] = dr;
    }
    if (timing) fprintf(stderr, "[lancet_gpu] device select: table of %u + %u alignments exported in %.3f s, %.1f MB resident per GPU after %.3f s\n", tab.n_aln[0], tab.n_aln[1], t1 - t0,
                        lancet_device_reads_bytes(dev_reads.begin()->second) / 1048576.0, now() - t1);
  }
  for (int c = 0; c < nchunks; ++c) {
    const int lo = c * step, hi = lo + step < nwin ? lo + step : nwin;
    if (ranked && (c < c_lo || c >= c_hi)) { jobs[(size_t)c].have = true; if (!flush()) return die(fail); continue; }      // another rank's batch
    Slot &sl = slots[(size_t)c % slots.size()];
    lancet_window_batch B; lancet_packed_reads PK; int32_t nk = 0;
    memset(&PK, 0, sizeof(PK));
    double t0 = now();
    if (sl.fut.valid() && !finish(sl)) return die(fail);          // its kept[] / engine must be free before they are reused
    const int dev = devs.size() > 1 ? devs[(size_t)c % slots.size() % devs.size()] : devs[0];
    bool taken = false;
    if (device_select) {
      std::string why;
      if (ho.linked) why = "linked reads";
      else if (reads_on) why = "haplotype reads";          // (--haplotype-reads decodes SEQ from the host's packed words: the batch is assembled on the host)
      else if (!packed) why = "ASCII hand-over";
      else {
        lancet_window_slice SL;
        if (lancet_host_windows(H, lo, hi, &ho, &SL) != LANCET_OK) return die(lancet_host_last_error(H));
        t_batch += now() - t0; t0 = now();
        if (more_verbose || hap_on) {      // (the slice's windows: the batch's are among them)
          uint32_t longest = 0;
          for (int32_t i = 0; i < SL.n_windows; ++i) longest = std::max(longest, SL.ref_off[i + 1] - SL.ref_off[i]);
          if (more_verbose && lancet_engine_set_trace_level(sl.e, trace_words_for(longest, max_indel_len), 2) != LANCET_OK) return die(std::string("engine: ") + lancet_engine_last_error(sl.e));
          if (hap_on && (lancet_engine_set_haplotypes(sl.e, hap_words_for(longest, max_indel_len) + hap_extra_for(longest)) != LANCET_OK || lancet_engine_set_haplotype_alignments(sl.e, aln_on ? 1 : 0) != LANCET_OK ||
                         lancet_engine_set_haplotype_coverage(sl.e, cov_on ? 1 : 0) != LANCET_OK ||
                         lancet_engine_set_haplotype_support(sl.e, sup_on ? 1 : 0, sup_mm) != LANCET_OK ||
                         lancet_engine_set_haplotype_evidence(sl.e, evid_on ? EVID_EVENTS : 0u, evid_mm) != LANCET_OK))
            return die(std::string("engine: ") + lancet_engine_last_error(sl.e));
        }
        const int rc = lancet_engine_upload_windows(sl.e, dev_reads[dev], &SL, &ho, sl.kept.data(), &nk);
        t_engine += now() - t0; t0 = now();
        if (rc == LANCET_OK && (more_verbose || cov_on)) {      // (--haplotype-coverage prints the stretch's bases)
          sl.raw.assign((size_t)nk, std::string());
          for (int32_t w = 0, i = 0; w < nk; ++w) {
            while (i < SL.n_windows && SL.widx[i] != sl.kept[(size_t)w]) ++i;
            if (i < SL.n_windows) sl.raw[(size_t)w].assign(SL.ref_bases + SL.ref_off[i], SL.ref_bases + SL.ref_off[i + 1]);
          }
        }
        if (rc == LANCET_OK) { taken = true; if (lancet_host_windows_done(H, lo, hi) != LANCET_OK) return die(lancet_host_last_error(H)); }
        else if (rc == LANCET_NOT_TAKEN) { why = lancet_engine_last_error(sl.e); if (why.compare(0, 11, "not taken: ") == 0) why.erase(0, 11); why = why.substr(0, why.find(':')); }
        else return die(std::string("engine: ") + lancet_engine_last_error(sl.e));
      }
      if (taken) ++n_taken; else ++not_taken[why];
    }
    if (!taken && (packed ? lancet_host_batch_packed(H, lo, hi, &ho, &P, &B, &PK, sl.kept.data(), &nk) : lancet_host_batch(H, lo, hi, &ho, &B, sl.kept.data(), &nk)) != LANCET_OK)
      return die(lancet_host_last_error(H));                      // (overlaps the other engines' kernels)
    t_batch += now() - t0;
    if (nk == 0) { jobs[(size_t)c].have = true; if (!flush()) return die(fail); continue; }
    t0 = now();
    if (!taken && more_verbose) {
      uint32_t longest = 0;
      sl.raw.assign((size_t)nk, std::string());
      for (int32_t w = 0; w < nk; ++w) { longest = std::max(longest, B.ref_off[w + 1] - B.ref_off[w]); sl.raw[(size_t)w].assign(B.ref_bases + B.ref_off[w], B.ref_bases + B.ref_off[w + 1]); }
      if (lancet_engine_set_trace_level(sl.e, trace_words_for(longest, max_indel_len), 2) != LANCET_OK) return die(std::string("engine: ") + lancet_engine_last_error(sl.e));
    }
    if (!taken && hap_on) {
      uint32_t longest = 0;
      for (int32_t w = 0; w < nk; ++w) longest = std::max(longest, B.ref_off[w + 1] - B.ref_off[w]);
      if (cov_on && !more_verbose) { sl.raw.assign((size_t)nk, std::string()); for (int32_t w = 0; w < nk; ++w) sl.raw[(size_t)w].assign(B.ref_bases + B.ref_off[w], B.ref_bases + B.ref_off[w + 1]); }
      if (lancet_engine_set_haplotypes(sl.e, hap_words_for(longest, max_indel_len) + hap_extra_for(longest)) != LANCET_OK || lancet_engine_set_haplotype_alignments(sl.e, aln_on ? 1 : 0) != LANCET_OK ||
          lancet_engine_set_haplotype_coverage(sl.e, cov_on ? 1 : 0) != LANCET_OK || lancet_engine_set_haplotype_support(sl.e, sup_on ? 1 : 0, sup_mm) != LANCET_OK ||
          lancet_engine_set_haplotype_placements(sl.e, reads_on ? 1 : 0, reads_mm) != LANCET_OK ||
          lancet_engine_set_haplotype_evidence(sl.e, evid_on ? EVID_EVENTS : 0u, evid_mm) != LANCET_OK)
        return die(std::string("engine: ") + lancet_engine_last_error(sl.e));
    }
    if (!taken && reads_on) {                                    // the batch's packed reads stay with the slot until its records are written
      const uint32_t R = B.read_begin[nk];
      sl.rd_woff.assign((size_t)R, 0u); sl.rd_bases.clear();
      if (packed) {
        const uint32_t n = PK.read_index ? PK.n_distinct : R;
        sl.rd_bases.assign(PK.bases, PK.bases + PK.base_woff[n]);
        for (uint32_t r = 0; r < R; ++r) sl.rd_woff[r] = PK.base_woff[PK.read_index ? PK.read_index[r] : r];
      } else {
        std::vector<uint32_t> good;
        for (uint32_t r = 0; r < R; ++r) {
          const uint32_t o = B.seq_off[r], len = B.seq_off[r + 1] - o; uint32_t ri = 0;
          sl.rd_woff[r] = (uint32_t)sl.rd_bases.size();
          sl.rd_bases.resize(sl.rd_bases.size() + (len + 15u) / 16u + 1u, 0u); good.assign((size_t)(len + 31u) / 32u + 1u, 0u);
          lancet_pack_read(&P, B.seq + o, B.qual + o, (int)len, B.label[r], B.strand[r], B.mate[r], B.mapped[r], &ri, sl.rd_bases.data() + sl.rd_woff[r], good.data());
        }
      }
      sl.rd_bases.push_back(0u);
    }
    if (!taken && (packed ? lancet_engine_upload_packed(sl.e, &B, &PK) : lancet_engine_upload(sl.e, &B)) != LANCET_OK) return die(std::string("engine: ") + lancet_engine_last_error(sl.e));
    t_engine += now() - t0;
    sl.chunk = c; sl.nk = nk; sl.base = done; done += nk; sl.bxn.clear();
    if (ho.linked) { uint32_t nbx = 0; const char *const *bxn = lancet_host_bx_names(H, &nbx); for (uint32_t i = 0; i < nbx; ++i) sl.bxn.emplace_back(bxn[i]); }
    lancet_engine *e = sl.e;
    // The launch happens HERE, on the one thread that submits (a few hundred microseconds: everything is asynchronous), behind the kernels
    // of the last engine submitted on the same GPU -- the two batches' kernels run back to back, not side by side; its done-event is
    // recorded by then because its own submit has returned.  Only the wait (re-run tier, read-back) goes to another thread.
    lancet_engine *prev = last_on_dev.count(dev) ? last_on_dev[dev] : nullptr;
    t0 = now();
    if (lancet_engine_submit_after(e, prev) != LANCET_OK) return die(std::string("engine: ") + lancet_engine_last_error(e));
    t_engine += now() - t0;
    last_on_dev[dev] = e;
    sl.fut = std::async(std::launch::async, [e]() { return lancet_engine_wait(e); });
    if (!flush()) return die(fail);
  }
  for (Slot &sl : slots) if (sl.fut.valid() && !finish(sl)) return die(fail);
  if (!flush()) return die(fail);
  if (device_select) {
    std::string line = "[lancet_gpu] device select: " + std::to_string(n_taken) + " batches taken, ";
    long nn = 0; std::string by;
    for (auto &kv : not_taken) { nn += kv.second; by += (by.empty() ? "" : ", ") + kv.first + " " + std::to_string(kv.second); }
    line += std::to_string(nn) + " not taken" + (by.empty() ? "" : " (" + by + ")");
    if (ranked) line += " [rank " + std::to_string(rank) + "]";
    fprintf(stderr, "%s\n", line.c_str());
  }
  if (more_verbose && n_truncated) fprintf(stderr, "lancet_gpu: %ld window(s) whose -V trace did not fit its buffer (%u paths of the longest window reference + --max-indel-len bases): their text ends with a [trace truncated] line%s\n",
                                           n_truncated, MV_PATHS, ranked ? (" [rank " + std::to_string(rank) + "]").c_str() : "");
  if (hap_on) {
    if (hap_out) {
      if (fclose(hap_out) != 0) return die("cannot write " + hap_file);
      fprintf(stderr, "[lancet_gpu] %ld haplotypes written to %s\n", n_hap, hap_file.c_str());
    }
    if (sam_on) {
      if (fclose(sam_out) != 0) return die("cannot write " + sam_file);
      fprintf(stderr, "[lancet_gpu] %ld haplotypes written to %s\n", n_hap, sam_file.c_str());
    }
    if (cov_on) {
      if (fclose(cov_out) != 0) return die("cannot write " + cov_file);
      fprintf(stderr, "[lancet_gpu] %ld haplotypes written to %s\n", n_hap, cov_file.c_str());
    }
    if (sup_on) {
      if (fclose(sup_out) != 0) return die("cannot write " + sup_file);
      fprintf(stderr, "[lancet_gpu] %ld haplotypes written to %s\n", n_hap, sup_file.c_str());
    }
    if (reads_on) {
      if (fclose(reads_out) != 0) return die("cannot write " + reads_file);
      fprintf(stderr, "[lancet_gpu] %ld reads written to %s\n", n_hap_reads, reads_file.c_str());
    }
    if (evid_on) {
      if (fclose(evid_out) != 0) return die("cannot write " + evid_file);
      fprintf(stderr, "[lancet_gpu] %ld events written to %s\n", n_evid, evid_file.c_str());
      if (n_evid_marked || n_evid_uneval) fprintf(stderr, "lancet_gpu: %ld window(s) with more than %u events (the first ones are kept), %ld unevaluated event(s) of groups beyond %u paths or %u events: all their counts are 0\n",
                                                  n_evid_marked, EVID_EVENTS, n_evid_uneval, (unsigned)LANCET_EVID_GROUP_ENTRIES, (unsigned)LANCET_EVID_GROUP_EVENTS);
    }
    if (n_hap_truncated) fprintf(stderr, "lancet_gpu: %ld window(s) whose haplotypes did not all fit their buffer (%u paths of the longest window reference + --max-indel-len bases): the first ones are in %s\n",
                                 n_hap_truncated, MV_PATHS, hap_out ? hap_file.c_str() : sam_on ? sam_file.c_str() : cov_on ? cov_file.c_str() : sup_on ? sup_file.c_str() : reads_on ? reads_file.c_str() : evid_file.c_str());
  }
  for (auto &kv : dev_reads) lancet_device_reads_destroy(kv.second);
  double t_gather = 0;
  if (ranked) {
    comm = comm_fut.get();
    if (!comm) return die(std::string("rank ") + std::to_string(rank) + ": cannot join the communicator: " + cerr);
    // one payload per rank: u64 number of parts, their lengths, the parts; rank 0 replays every rank's parts into the database
    const double tg0 = now();
    std::vector<uint8_t> payload(8 * (1 + parts.size()));
    { uint64_t x = parts.size(); memcpy(payload.data(), &x, 8); for (size_t i = 0; i < parts.size(); ++i) { x = parts[i].size(); memcpy(payload.data() + 8 * (1 + i), &x, 8); } }
    for (auto &pt : parts) payload.insert(payload.end(), pt.begin(), pt.end());
    uint8_t *all = nullptr; std::vector<size_t> lens((size_t)ranks, 0);
    if (lancet_comm_gather(comm, payload.data(), payload.size(), &all, lens.data()) != LANCET_OK) return die(std::string("rank ") + std::to_string(rank) + ": gather: " + lancet_comm_last_error(comm));
    uint32_t added = 0;
    if (rank == 0) {
      std::vector<const uint8_t *> pp; std::vector<size_t> pl;
      size_t o = 0;
      for (int r = 0; r < ranks; ++r) {
        const uint8_t *b = all + o; const size_t len = lens[(size_t)r]; o += len;
        if (len < 8) return die("gather: a rank sent a damaged payload");
        uint64_t np = 0; memcpy(&np, b, 8);
        if (8 * (1 + np) > len) return die("gather: a rank sent a damaged payload");
        size_t q = 8 * (1 + (size_t)np);
        for (uint64_t i = 0; i < np; ++i) { uint64_t x; memcpy(&x, b + 8 * (1 + i), 8); if (q + x > len) return die("gather: a rank sent a damaged payload"); pp.push_back(b + q); pl.push_back((size_t)x); q += (size_t)x; }
      }
      if (lancet_records_merge(db, pp.data(), pl.data(), (int)pp.size(), &added) != LANCET_OK) return die("VariantDB rejected the gathered records");
    }
    t_gather = now() - tg0;
    fprintf(stderr, "[lancet_gpu] rank %d of %d on GPU %d (%s): %ld windows assembled, %zu batches, %zu bytes to rank 0%s\n", rank, ranks, devs[0], lancet_comm_transport(comm), done, parts.size(),
            payload.size(), rank == 0 ? (std::string("; ") + std::to_string(added) + " records replayed").c_str() : "");
    if (all) lancet_free(all);
    lancet_comm_destroy(comm);
  }
  if (ranks > 0 && rank != 0) {
    lancet_vdb_destroy(db); lancet_host_close(H); for (lancet_engine *e : engs) lancet_engine_destroy(e);
    if (!overflowed.empty()) {
      fprintf(stderr, "lancet_gpu: rank %d: %zu window(s) exceeded the engine's work space and contributed NO variants:\n", rank, overflowed.size());
      for (const std::string &w : overflowed) fprintf(stderr, "lancet_gpu:   %s\n", w.c_str());
      return 3;
    }
    return 0;
  }
  std::string cmdline = "lancet";
  for (int i = 1; i < argc; ++i) {
    if (strcmp(argv[i], "--date-line") == 0 || strcmp(argv[i], "--rank") == 0 || strcmp(argv[i], "--rendezvous") == 0) { ++i; continue; }     // (what names the run / the process, not the job)
    if (strcmp(argv[i], "--device-select") == 0) continue;       // (which route assembles the batches: the same VCF either way)
    if (strcmp(argv[i], "--haplotypes") == 0 || strcmp(argv[i], "--haplotype-sam") == 0 || strcmp(argv[i], "--haplotype-coverage") == 0 ||
        strcmp(argv[i], "--haplotype-support") == 0 || strcmp(argv[i], "--haplotype-support-mismatches") == 0 ||
        strcmp(argv[i], "--haplotype-reads") == 0 || strcmp(argv[i], "--haplotype-read-mismatches") == 0 ||
        strcmp(argv[i], "--variant-evidence") == 0 || strcmp(argv[i], "--variant-evidence-mismatches") == 0) { ++i; continue; }  // (a second output of the same run)
    cmdline += " "; cmdline += argv[i];
  }
  if (date_line.empty()) { time_t t = time(nullptr); date_line = ctime(&t); }
  else if (date_line.back() != '\n') date_line += "\n";
  char *vcf = lancet_vdb_vcf(db, nullptr, cmdline.c_str(), ref.c_str(), date_line.c_str(), lancet_host_sample(H, 0), lancet_host_sample(H, 1));
  if (!vcf) return die("VCF rendering failed");
  fputs(vcf, stdout);
  fprintf(stderr, "[lancet_gpu] %d windows tiled, %ld assembled on %zu engine(s), first GPU %d, %u variants\n", nwin, done, engs.size(), devs[0], lancet_vdb_size(db));
  if (timing) fprintf(stderr, "[lancet_gpu] wall %.3f s: input decode + tiling %.3f, window filters + batches %.3f, engine (upload + kernels + results) %.3f (kernels %.3f), VariantDB %.3f\n",
                      now() - t_start, t_tile, t_batch, t_engine, t_kernel / 1000.0, t_vdb + t_gather);
  lancet_free(vcf);
  lancet_vdb_destroy(db); lancet_host_close(H); for (lancet_engine *e : engs) lancet_engine_destroy(e);
  if (!overflowed.empty()) {
    fprintf(stderr, "lancet_gpu: %zu window(s) exceeded the engine's work space (tier-2 limits, DESIGN.md section 9) and contributed NO variants:\n", overflowed.size());
    for (const std::string &w : overflowed) fprintf(stderr, "lancet_gpu:   %s\n", w.c_str());
    return 3;
  }
  return 0;
}
