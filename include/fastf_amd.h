/*
 * fastf_amd.h — C ABI of the MI355X-native bam2db UMI-counting engine.
 *
 * Three layers, all plain C (pointers + sizes, no C++/torch types):
 *
 *   1. OUTER drop-in symbols — what the reference's own main.c binds
 *        int bam2db(...)            replaces  src/bam2db_ds.c:106-573 (decl. bam2db_ds.h:62-70)
 *        int _umi_copies_flag       replaces  src/bam2db_ds.c:3       (decl. bam2db_ds.h:23)
 *        int cmd_bam2db(argc,argv)  replaces  src/main.c:288-362
 *      and, for the tag-histogram commands,
 *        extract_bam / read_bam / print_CB_node / free_CB_node   replace  src/extract.c (decl. extract.h:15-26)
 *        cmd_crb / cmd_extract                                   replace  src/main.c:231-286, 364-402
 *      and, for the FASTQ histogram,
 *        cell_counts / cmd_freq                                  replace  src/count.c:3-21, src/main.c:30-92
 *        fastF / cmd_filter                                      replace  src/filter.c:286-350, src/main.c:94-228
 *
 *   2. INNER seam (host buffers in, COO out) — what replaces the reference's
 *      per-record loop + SQLite aggregate (bam2db_ds.c:360-438, 480-483):
 *        fastf_engine_create / _push / _finish / _umi_rows / _reset / _destroy
 *      plus the host-side exact string→key packer that replaces
 *      hash()+hash_table_lookup() key handling (bam2db_ds.c:96-104, hashtable.c:98-115).
 *
 *   3. DEVICE-level entry points (device pointers + a hipStream_t passed as void*)
 *      for callers that already own HBM buffers (bench.py, the multi-GPU host in
 *      fastf_amd/dist.py, kernel parity tests).
 *
 * Every function returns 0 on success and non-zero on failure unless stated;
 * the message is available from fastf_last_error() — the last error of the process, whichever
 * thread raised it (reader workers fail on their own threads); the returned pointer is a
 * per-thread snapshot.
 * The reference convention "0 ok / 1 fail + message on stderr" (bam2db_ds.h:60)
 * is kept by the outer layer.
 */
#ifndef FASTF_AMD_H
#define FASTF_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ===================================================================== */
/* 1. outer drop-in symbols                                              */
/* ===================================================================== */

/* bam2db_ds.h:23 / bam2db_ds.c:3 — set by `-u/--umicopies` (main.c:309) */
extern int _umi_copies_flag;

/* bam2db_ds.h:62-70.  db_file is accepted and ignored (no SQLite). */
int bam2db(char *bam_file, char *db_file, char *path_out, char *barcodes_file,
           char *features_file, float rate_cell, float rate_depth, unsigned int seed);

/* main.c:288-362; argv[0] == "bam2db". */
int cmd_bam2db(int argc, const char **argv);
/* which device(s) bam2db() uses, from the values of FASTF_DEVICES ("a,b,.." or a count) and FASTF_DEVICE (either may be NULL):
 * *dev0 = the engine's and the reader's device, *dev_second = the second listed device or -1 */
void fastf_pick_devices(const char *devices, const char *device, int *dev0, int *dev_second);

/* --- crb / extract: src/extract.c.  The tree types are the reference's (filter.h:28-34, extract.h:8-13); they are
 * declared here under guards so that this header can be included next to the reference's own. --- */
#ifndef FASTF_NO_TREE_TYPES
#if !defined(FASTQ_FILTER_H)
typedef struct node { char *data; long int count; struct node *left; struct node *right; } node;
#endif
#if !defined(EXTRACT_H)
typedef struct CB_node { node *CR; char *CB; struct CB_node *left; struct CB_node *right; } CB_node;
#endif
/* extract.c:135-216 — histogram of one tag (type 0: string, 1: integer) → ./tag_summary.csv, counters on stdout */
void extract_bam(char *bam_file, const char *tag, int type);
/* extract.c:64-133 — the CB → CR tree of the reference, node for node (malloc'ed; release with free_CB_node) */
CB_node *read_bam(char *bam_file);
/* extract.c:33-45.  print_CB_node(CB_node *, gzFile) (extract.c:47-62) is exported too; it is declared in
 * host_io.h / the reference's extract.h because its second parameter is zlib's gzFile. */
void free_CB_node(CB_node *root);
#endif
int cmd_crb(int argc, const char **argv);       /* main.c:231-286; argv[0] == "crb"     */
int cmd_extract(int argc, const char **argv);   /* main.c:364-402; argv[0] == "extract" */
/* the same results as bytes: the decompressed content of `crb`'s output file / of tag_summary.csv (malloc'ed) */
int fastf_crb_text(const char *bam_file, char **txt, size_t *txt_len, uint64_t *n_records);
int fastf_extract_text(const char *bam_file, const char *tag, int type, char **csv, size_t *csv_len,
                       uint64_t *n_records, uint64_t *n_valid);

/* --- freq: src/main.c:30-92, count.c.  cell_counts(gzFile, ...) (count.c:3-21) is exported too; it is declared in host_io.h
 * because its first parameter is zlib's gzFile. --- */
int cmd_freq(int argc, const char **argv);      /* main.c:30-92; argv[0] == "freq" */
/* the bytes of whitelist.txt for an R1 FASTQ (plain, gzip or BGZF): "<first len_cb + len_umi bytes of the read>,<count>\n" in the
 * pre-order of the reference's insertion-order tree (malloc'ed); *n_reads = reads in the file */
int fastf_freq_text(const char *fastq_file, size_t len_cellbarcode, size_t len_umi, char **txt, size_t *txt_len,
                    uint64_t *n_reads);

/* --- filter: src/main.c:94-228, filter.c:286-350.  fastF(gzFile in[3], gzFile out[3], ...) (filter.c:286) is exported too; it
 * is declared in host_io.h because of zlib's gzFile. --- */
int cmd_filter(int argc, const char **argv);    /* main.c:94-228; argv[0] == "filter" */
/* I1 / R2 may be NULL; out_dir NULL = "."; whitelist NULL needs all_cells.  Writes <out_dir>/R1.fastq.gz (and I1 / R2): the reads
 * whose draw (float) rand() / RAND_MAX after srand(seed) is below rate and (all_cells, or whose first len_cellbarcode bytes of the
 * R1 sequence line equal those of a whitelist line), as gzip members.  *n_reads = R1 reads, *n_kept = reads kept. */
int fastf_filter(const char *r1, const char *i1, const char *r2, const char *out_dir, const char *whitelist, uint32_t len_cellbarcode,
                 uint32_t seed, float rate, int all_cells, uint64_t *n_reads, uint64_t *n_kept);
/* rand() outputs first .. first + n - 1 after srand(seed), computed by the device kernel of filter (out: n words) */
int fastf_filter_draws(uint32_t seed, uint64_t first, uint64_t n, uint32_t *out);
/* the same by the host: the jump-ahead to `first`, then the recurrence word by word; one output by the jump-ahead alone; the
 * reference's keep rule for one draw */
int fastf_filter_draws_host(uint32_t seed, uint64_t first, uint64_t n, uint32_t *out);
uint32_t fastf_filter_rand_at(uint32_t seed, uint64_t index);
int fastf_filter_draw_passes(uint32_t r, float rate);

/* --- fqcap: the FASTQ triple with every cell capped at N reads (fqcap_cmds.c, fqcap_kernels.hpp; not a command of the reference).
 * filter with a rate per cell in place of the one global rate.  The definition:
 *   cell of a read   the first len_cellbarcode bytes of its R1 sequence line exactly as filter's whitelist test sees them: strncmp
 *                    semantics, a shorter line taken with its '\n', cut at a NUL.  A read is MATCHED iff `filter -w` would match
 *                    it; two matched reads are of the same cell iff those bytes are equal.  Duplicate whitelist lines and lines
 *                    that share their first len_cellbarcode bytes are one cell.
 *   h[k]             the matched R1 reads of cell k, counted over the whole file before any draw (the order of cap, which counts
 *                    before xf).
 *   draw of read i   output i of rand() after srand(seed), consumed by every R1 read, matched or not: filter's stream, so that
 *                    the two commands are coupled by the seed.
 *   rate of cell k   t = the rate given, 2.0f when none is (every draw passes: no global thinning).  rate_k = t where h[k] <= N,
 *                    min(t, (float)((double)N / (double)h[k])) otherwise: fastf_fqcap_rate(N, h[k], t).  Read i of cell k is kept
 *                    iff fastf_filter_draw_passes(draw_i, rate_k), the draw that rounds to 1.0 included.  Bernoulli per read, as
 *                    cap: "at most N" holds in expectation.
 *   mates            I1 and R2 follow R1's keep bitmap exactly as in filter (shorter or longer mates, a last line without '\n').
 *   outputs          <out_dir>/R1.fastq.gz (and I1 / R2 when given) as filter writes them, and <out_dir>/fqcap_cells.tsv.gz: the
 *                    line "barcode\treads\tkept", then one row per cell with h > 0 — its bytes, h, reads kept — ascending by the
 *                    bytes of the barcode (memcmp, the shorter first), DNA-form and other cells in one order.  A byte of a barcode
 *                    outside 0x21 .. 0x7e, and the backslash, is written \xHH (upper-case hex).  sum(kept) = *n_kept.
 * Consequences: with N >= max h the three FASTQ outputs hold the bytes of `filter -w ... -t t` with the same seed; for any N the
 * kept reads are a subset of that filter's.
 * Refused with a message (1 returned, the output directory untouched): no R1, no whitelist, cap 0, a negative length, a directory
 * that cannot be written, filter's declared divergences in R1 (a line longer than 1023 bytes, a file that ends partway through a
 * read, corrupt input) and an R1 of 2^32 reads or more (the per-cell counters are 32-bit).  A refusal that only a mate file
 * shows comes after R1 was written: the outputs made so far are removed. --- */
int cmd_fqcap(int argc, const char **argv);     /* argv[0] == "fqcap"; filter's option dialect, -n N required, no -a */
int fastf_fqcap(const char *r1, const char *i1, const char *r2, const char *out_dir, const char *whitelist, uint32_t len_cellbarcode,
                uint32_t seed, float rate, uint64_t cap, uint64_t *n_reads, uint64_t *n_matched, uint64_t *n_kept);
float fastf_fqcap_rate(uint64_t cap, uint64_t hits, float t);
/* The device seam of fqcap on filter's window handle (host_io.h: fastf_fltdev_create / set_whitelist / reset / parse / emit / end),
 * one caller-supplied window at a time.  hits[], kept[] and rate[] hold one word per whitelist key and 16 guard words behind
 * (0xa5a5a5a5), which no kernel touches.
 *   begin      after set_whitelist: hits[] and kept[] cleared, rate[] and the guards filled with the guard word
 *   count      pass 0 of the parsed window: hits[k] += its matched reads of key k; *esc / *n_esc: every read of the window whose
 *              barcode is not DNA-form (pinned, valid until the next call); the window is done (no emit follows)
 *   set_rates  n = the key count; kept[] cleared
 *   decide     pass 1 of the parsed window: fastf_fltdev_decide's R1 mode with the draw tested against t, then against rate[k];
 *              kept[k] += the reads kept; *esc: the reads that passed t and are not DNA-form; fastf_fltdev_emit follows
 *   draws      the rand() outputs of the window decided last
 *   read       which = 0 hits[], 1 kept[], 2 the bits of rate[]; n_words <= keys + 16 */
typedef struct fastf_fltdev fastf_fltdev_t;
typedef struct { uint32_t i, s1; } fastf_flt_esc_t;     /* read i of the window, its sequence line at buffer offset s1 */
int fastf_fcpdev_begin(fastf_fltdev_t *p);
int fastf_fcpdev_count(fastf_fltdev_t *p, uint32_t len_cellbarcode, const fastf_flt_esc_t **esc, uint32_t *n_esc);
int fastf_fcpdev_set_rates(fastf_fltdev_t *p, const float *rate, size_t n);
int fastf_fcpdev_decide(fastf_fltdev_t *p, uint32_t len_cellbarcode, float t, const uint32_t *chunk_states,
                        const fastf_flt_esc_t **esc, uint32_t *n_esc);
int fastf_fcpdev_draws(fastf_fltdev_t *p, uint32_t *out, uint64_t n);
int fastf_fcpdev_read(fastf_fltdev_t *p, int which, uint32_t *out, size_t n_words);

/* --- fqcells: the cells of an R1 FASTQ, called by UMIs per barcode (fqcells_cmds.c, fqcells_kernels.hpp; not a command of the
 * reference).  Its whitelist.txt is what `filter -w` and `fqcap -w` read with the same -l.  The definition:
 *   counted reads    a read is COUNTED iff the first l + u bytes of its R1 sequence line are exactly l + u bytes of ACGT (freq's DNA
 *                    form; l = len_cellbarcode >= 1, u = len_umi >= 0, l + u <= 31).  Its barcode is the first l of those bytes, its
 *                    UMI the next u.  Every other read (a shorter line, N, lower case, '\r') is counted in `other` and belongs to no
 *                    barcode.
 *   per barcode b    reads[b] = its counted reads, umis[b] = the distinct UMIs among them (u = 0: 1 for every barcode).
 *   order            by umis descending, then reads descending, then the barcode's bytes ascending; rank = the 1-based position in
 *                    that order; B = the number of barcodes.
 *   calling rule     exactly one of (none given: 'e' with 3000):
 *                      'k' K   called iff rank <= K
 *                      'm' M   called iff umis >= M
 *                      'e' E   m = umis of the barcode at rank min(B, E / 100 + 1) (integer division), T = max(1, (m + 5) / 10),
 *                              called iff umis >= T: Cell Ranger's order-of-magnitude rule in integers
 *                    threshold = T, M, or for 'k' the umis of the last barcode called (0 when B = 0; 'e' with B = 0 has m = 0, T = 1).
 *   outputs          <out_dir>/fqcells.tsv.gz: the line "barcode\treads\tumis\trank\tcalled", then one row per barcode ascending by
 *                    its bytes, called written 0 or 1 (gzip members);
 *                    <out_dir>/whitelist.txt: the called barcodes, one a line, ascending (plain text);
 *                    <out_dir>/fqcells_summary.tsv: the line "reads\tcounted\tother\tbarcodes\tumis\trule\targ\tthreshold\tcalled\t
 *                    called_reads\tcalled_umis" and one row: R1 reads, counted reads, other reads, B, distinct barcode+UMI pairs, the
 *                    rule's letter, its argument, the threshold, barcodes called, their reads, their umis.
 * Refused with a message (1 returned, the output directory untouched): no R1, l < 1, l or u negative, l + u > 31, a rule other than
 * 'e', 'k', 'm', an argument of 0, a directory that cannot be written, freq's declared divergences (a line longer than 1023 bytes, a
 * file that ends after a header line, corrupt input) and 2^32 - 1 reads or more (the histogram's limit).  An R1 with no counted
 * read is no error: header-only tables and an empty whitelist. --- */
typedef struct {
    uint64_t reads, counted, other, barcodes, umis;
    uint64_t rule;                              /* 'e', 'k' or 'm' */
    uint64_t arg, threshold, called, called_reads, called_umis;
} fastf_fqcells_summary_t;
int cmd_fqcells(int argc, const char **argv);   /* argv[0] == "fqcells"; freq's option dialect: -R -o -l -u and one of -e -k -m */
int fastf_fqcells(const char *r1, const char *out_dir, uint32_t len_cellbarcode, uint32_t len_umi, int rule, uint64_t arg,
                  fastf_fqcells_summary_t *summary);
/* The order and the rule on a table of n barcodes, on the host threads (no device).  bc[] need not be sorted; it holds distinct
 * barcodes packed 2 bits a base (A < C < G < T, first base highest), so that its order is the order of the bytes.  rank[i]
 * (1-based), called[i] (0 / 1) and *threshold as defined above; rank and called may be NULL.  1 for a rule or argument refused. */
int fastf_fqcells_call(const uint64_t *bc, const uint64_t *reads, const uint32_t *umis, size_t n, int rule, uint64_t arg,
                       uint32_t *rank, uint8_t *called, uint64_t *threshold);
/* The device seam: m1 ascending DNA-form keys of l + u bases (bit 63 set or not: it is masked) with their counts, host arrays of
 * the caller's, through the kernels of the per-barcode reduce.  Out: rows [0, *n_rows) of bc (the key without bit 63, >> 2 * len_umi),
 * reads and umis, ascending, and 16 guard entries behind them as the device arrays carry them (every byte 0xa5), which no kernel
 * touches: the three arrays hold m1 + 16 entries.  fastf_fqcells_tile: the keys one workgroup of the reduce takes. */
int fastf_fqcells_reduce(const uint64_t *keys, const uint32_t *counts, size_t m1, uint32_t len_umi, uint64_t *bc, uint64_t *reads,
                         uint32_t *umis, size_t *n_rows);
size_t fastf_fqcells_tile(void);

/* --- sweep: bam2db over a grid of (cell rate, depth rate) points from ONE decode of the BAM (sweep_cmds.c; not a command of the
 * reference).  Per point <out_dir>/c<rate_cell>_r<rate_depth>/ (rates printed %.3f) holds matrix.mtx.gz, barcodes.tsv.gz and
 * features.tsv.gz with the bytes bam2db() writes for that point; <out_dir>/sweep.tsv holds a header and one row per point, cell
 * rates major, depth rates minor:
 *   rate_cell rate_depth seed n_cells total_reads sampled_reads sampled_valid_reads nnz umis saturation
 *   median_umis_per_cell median_genes_per_cell
 * umis = sum of the matrix counts; saturation = 1 - umis / sampled_valid_reads (0 when that is 0); genes of a cell = its rows with
 * count >= 1; the medians run over all n_cells sampled cells.  Two values of one list that print the same at %.3f are refused.
 * Keys wider than 64 bits, UMIs beyond what a 64-bit key holds and FASTF_DEVICES naming several devices run point by point through
 * bam2db() (one line on stderr says so); the results are the same bytes.  On failure no sweep.tsv is left. --- */
int cmd_sweep(int argc, const char **argv);     /* argv[0] == "sweep"; -b -a -f -o -c <list> -r <list> [-s] [--summary-only] [--genes] [--cells] [--fidelity] [--gene-fidelity] [--neighbors] [--coexpression] [--labels FILE] [--markers N] [--mapping] [--pseudotime FILE] */
#define FASTF_SWEEP_SUMMARY_ONLY 1u             /* sweep.tsv alone: no rows leave the device, no point directories */
#define FASTF_SWEEP_GENES        2u             /* --genes: the per-gene files below, beside everything else */
#define FASTF_SWEEP_CELLS        8u             /* --cells: the per-cell files below, beside everything else (resident form only); bit 4 is not assigned */
int fastf_sweep(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                const float *rates_depth, uint32_t n_r, uint32_t seed, uint32_t flags);
/* the host pieces of it: a comma-separated list of rates (strtof per element; empty elements, trailing characters, NaN and negative
 * values are refused, cell rates above 1 too); the grid check; a point's directory name; the header line of sweep.tsv; per cell
 * (index c -> slot c - 1) the sum of the counts and the rows with count >= 1 of a COO; one row of sweep.tsv from those */
int fastf_sweep_parse_rates(const char *text, int cell_rates, float *out, uint32_t cap, uint32_t *n_out);
int fastf_sweep_check_grid(const float *rates_cell, uint32_t n_c, const float *rates_depth, uint32_t n_r);
int fastf_sweep_point_dir(float rate_cell, float rate_depth, char *buf, size_t cap);
const char *fastf_sweep_header(void);
/* --genes (FASTF_SWEEP_GENES, FASTF_CAP_GENES): per-gene detection across the grid.  For a point, cells[g - 1] = matrix rows of
 * feature g with count >= 1 (the cells that detect the gene: the rule of genes per cell) and umis[g - 1] = the sum of their counts.
 *   <out_dir>/sweep_genes.tsv (cap_genes.tsv): a header and one row per point in sweep.tsv's order, all integers but the rates:
 *     rate_cell rate_depth|reads_per_cell seed genes_detected genes_min_cells_3 genes_min_cells_10 max_gene_umis
 *     (genes with cells >= 1, >= 3, >= 10; the largest umis[]); written as .partial and renamed, as sweep.tsv is
 *   <out_dir>/sweep_gene_cells.tsv.gz (cap_gene_cells.tsv.gz): header `feature` and the point directory names, then one row per
 *     feature in list order — its id, the first field of its line in features.tsv.gz — with cells[] of every point; written with
 *     --summary-only too, and left only when every point is done
 *   <point dir>/genes.tsv.gz (not with --summary-only): `feature id \t cells \t umis` for every feature in list order
 * Every other output is the bytes it is without the flag.  sweep's point-by-point path fills the same files from each point's matrix. */
const char *fastf_sweep_genes_header(void);
const char *fastf_cap_genes_header(void);
/* one row of either table (with its newline): reads_per_cell == 0 prints rate_depth (%.3f) in the second column — a sweep row —
 * and reads_per_cell >= 1 prints that integer — a cap row */
int fastf_genes_summary_row(float rate_cell, float rate_depth, uint64_t reads_per_cell, uint32_t seed, const uint32_t *cells_per_gene,
                            const uint64_t *umis_per_gene, uint32_t n_features, char *buf, size_t cap);
/* --cells (FASTF_SWEEP_CELLS, FASTF_CAP_CELLS): how deeply every cell was sequenced at a point, and the copy-number histogram of its
 * UMIs.  A point's keys — one per sampled_valid read — sorted fully and run-length encoded (fastf_dev_umi_rows) give one row per
 * distinct (cell, feature, blob) with its run length n_copy; a row whose blob is NULL is a NULL row.  For a point, reads[c - 1] =
 * the sum of n_copy over all rows of cell c (its sampled_valid reads), null_reads[c - 1] = that sum over its NULL rows, single[c - 1]
 * = its non-NULL rows with n_copy == 1, and hist[] (FASTF_COPY_BINS + 1 entries, below) counts the non-NULL rows by n_copy.
 *   <out_dir>/sweep_cells.tsv (cap_cells.tsv): a header and one row per point in sweep.tsv's order, all integers but the rates:
 *     rate_cell rate_depth|reads_per_cell seed valid_reads null_umi_reads umis singleton_umis median_reads_per_cell
 *     copies_1 .. copies_31 copies_32_plus reads_copies_32_plus
 *     (valid_reads = the sum of reads[], umis = the non-NULL rows = the sum of copies_*, the median over all sampled cells by the
 *     rule of sweep.tsv's medians, printed %.1f; sum of k * copies_k (k < 32) + reads_copies_32_plus + null_umi_reads = valid_reads);
 *     written as .partial and renamed, with --summary-only too
 *   <point dir>/cells.tsv.gz (not with --summary-only): a header and one row per sampled cell in barcodes.tsv.gz's order:
 *     barcode reads null_umi_reads umis genes singleton_umis saturation
 *     (barcode = that file's line; umis, genes = the per-cell numbers behind sweep.tsv's medians; saturation = 1 - umis / reads
 *     printed %.6f, 0.000000 when reads == 0)
 * Every other output is the bytes it is without the flag.  A job outside the resident form (keys wider than 64 bits, UMIs beyond
 * what a 64-bit key holds, several devices) is refused with the flag: sweep's point-by-point path has no such rows. */
#define FASTF_COPY_BINS 32u
const char *fastf_sweep_cells_header(void);
const char *fastf_cap_cells_header(void);
/* one row of either table (with its newline): the second column as fastf_genes_summary_row prints it; hist: FASTF_COPY_BINS + 1 */
int fastf_cells_summary_row(float rate_cell, float rate_depth, uint64_t reads_per_cell, uint32_t seed, const uint32_t *reads,
                            const uint32_t *null_reads, const uint32_t *single, uint32_t n_cells, const uint64_t *hist, char *buf, size_t cap);

/* --- cap: every cell downsampled to at most N reads (cap_cmds.c; not a command of the reference).  For one point (cell rate c,
 * cap N >= 1, seed s): the cells are sampled as `bam2db -c c -s s` samples them; h[k] = records whose CB is sampled cell k (counted
 * before xf, as the reference's depth draw is), H = sum h; the i-th CB hit in file order consumes draw i of init_genrand(s)
 * advanced by the draws SampleInt consumed — bam2db's own coupling; hit i of cell k is kept iff draw[i] < T[k], T[k] = 2^32 where
 * h[k] <= N (the cell loses no read) and fastf_draw_threshold((float)((double)N / (double)h[k])) otherwise; everything behind the depth
 * draw runs as in bam2db.  Per point <out_dir>/c<rate_cell>_n<N>/ holds the three files of bam2db, the matrix header's rate_depth
 * carrying the realised fraction (float)((double)sampled / (double)H) (1.0 when H == 0); <out_dir>/cap.tsv holds a header and one row per
 * point, cell rates major, caps minor: sweep.tsv's columns with rate_depth replaced by reads_per_cell, and hits, cells_capped
 * (cells with h > N) and realised_depth (%.6f) appended.  Refused: N < 1, an empty list, a value twice, and jobs outside the
 * resident form (keys wider than 64 bits, UMIs beyond what a 64-bit key holds, FASTF_DEVICES naming several devices) — bam2db cannot
 * express a cap, so there is no point-by-point fallback.  On failure no cap.tsv is left. --- */
int cmd_cap(int argc, const char **argv);       /* argv[0] == "cap"; -b -a -f -o -c <list> -n <list> [-s] [--summary-only] [--genes] [--cells] [--fidelity] [--gene-fidelity] [--neighbors] [--coexpression] [--labels FILE] [--markers N] [--mapping] [--pseudotime FILE] */
#define FASTF_CAP_SUMMARY_ONLY 1u               /* cap.tsv alone */
#define FASTF_CAP_GENES        2u               /* --genes: cap_genes.tsv, cap_gene_cells.tsv.gz and genes.tsv.gz per point, as sweep writes them */
#define FASTF_CAP_CELLS        8u               /* --cells: cap_cells.tsv and cells.tsv.gz per point, as sweep writes them; bit 4 is not assigned */
int fastf_cap(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
              const uint64_t *caps, uint32_t n_n, uint32_t seed, uint32_t flags);
/* the host pieces of it: a comma-separated list of caps (decimal integers >= 1; empty elements, signs, trailing characters and
 * values twice are refused); the grid check; a point's directory name; the header line of cap.tsv; one row of it (with its
 * newline; counters = {total, sampled, sampled_valid}); the per-cell thresholds T[] above from h[] */
int fastf_cap_parse_caps(const char *text, uint64_t *out, uint32_t cap, uint32_t *n_out);
int fastf_cap_check_grid(const float *rates_cell, uint32_t n_c, const uint64_t *caps, uint32_t n_n);
int fastf_cap_point_dir(float rate_cell, uint64_t reads_per_cell, char *buf, size_t cap);
const char *fastf_cap_header(void);
int fastf_cap_summary_row(float rate_cell, uint64_t reads_per_cell, uint32_t seed, const uint64_t counters[3], uint64_t nnz, uint64_t umis,
                          const uint64_t *umis_per_cell, const uint32_t *genes_per_cell, uint32_t n_cells, uint64_t hits,
                          uint32_t cells_capped, char *buf, size_t cap);
int fastf_cap_thresholds(const uint32_t *hits, uint32_t n_cells, uint64_t cap, uint64_t *thresholds_out);
/* the realised fraction of a point as the matrix header carries it */
float fastf_cap_realised(uint64_t sampled, uint64_t hits);

/* --- level: every cell downsampled to at most M UMIs, exactly (level_cmds.c; not a command of the reference).  One point is a cell
 * rate c, a UMI cap M >= 1 and a seed s.  Cells are sampled as `bam2db -c c -s s` samples them; H and the coupling "hit i consumes
 * draw i, advanced by SampleInt's draws" are cap's (above).
 *   - For cell k and an integer T in [0, 2^32], U_k(T) is the sum of the counts of cell k's matrix column when hit i of cell k is kept
 *     iff draw[i] < T.  Everything behind the depth draw runs as in bam2db.  It depends on cell k's hits alone.
 *   - T[k] = max { T in [0, 2^32] : U_k(T) <= M }.  U_k(0) = 0, so it exists.  T[k] = 2^32 means the cell loses no read.
 *   - cells_capped is the number of cells with U_k(2^32) > M.
 *   - The point is cap's pipeline run with these T[k].  The matrix header's rate_depth carries fastf_cap_realised(sampled, H).
 *   - Every column sum of the point's matrix is <= M.  It is exactly M for a capped cell, unless two of its hits that each start a new
 *     UMI share one 32-bit draw.  The definition covers that case as it stands.
 * The kept sets of a cell are nested in T, so U_k is a non-decreasing step function of T and T[k] is found by bisection, for all cells
 * at once on the device (fastf_dev_level_init / fastf_dev_level_step below; at most 32 probing passes per point).
 * Per point <out_dir>/c<rate_cell>_m<M>/ (replicate runs: .._s<seed>) holds the three files of bam2db and thresholds.tsv.gz: header
 * `barcode threshold umis_full umis`, one row per sampled cell in barcodes.tsv.gz's order: T[k] as a decimal, U_k(2^32), U_k(T[k]).
 * <out_dir>/level.tsv is cap.tsv with reads_per_cell named umi_cap (hits, cells_capped and realised_depth are kept); --genes, --cells
 * and replicate runs write level_genes.tsv, level_gene_cells.tsv.gz, level_cells.tsv, level_reps.tsv, level_genes_reps.tsv,
 * level_gene_reps.tsv.gz and the per-point files as cap writes its own, the one column renamed.  Refused: what cap refuses (M < 1, an
 * empty list, a value twice, more than 64 values, -u, and jobs outside the resident form: several devices, keys wider than 64 bits,
 * UMIs beyond what a 64-bit key holds — there is no point-by-point form).  Every table goes through .partial; on failure none is left. --- */
int cmd_level(int argc, const char **argv);     /* argv[0] == "level"; -b -a -f -o -c <list> -m|--umis <list> [-s | --seeds | --reps] [--summary-only] [--genes] [--cells] [--fidelity] [--gene-fidelity] [--neighbors] [--coexpression] [--labels FILE] [--markers N] [--mapping] [--pseudotime FILE] */
#define FASTF_LEVEL_SUMMARY_ONLY 1u             /* level.tsv (and the other tables) alone: no point directories */
#define FASTF_LEVEL_GENES        2u             /* --genes, as cap's */
#define FASTF_LEVEL_CELLS        8u             /* --cells, as cap's; bit 4 is not assigned */
int fastf_level(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                const uint64_t *umi_caps, uint32_t n_m, uint32_t seed, uint32_t flags);
int fastf_level_reps(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                     const uint64_t *umi_caps, uint32_t n_m, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags);
/* the host pieces of it: the list of UMI caps and the grid check (fastf_cap_parse_caps's and fastf_cap_check_grid's rules, the
 * messages naming this verb); a point's directory name; the header lines (cap's, with reads_per_cell named umi_cap); one row of
 * level.tsv (with its newline; the arguments of fastf_cap_summary_row) */
int fastf_level_parse_caps(const char *text, uint64_t *out, uint32_t cap, uint32_t *n_out);
int fastf_level_check_grid(const float *rates_cell, uint32_t n_c, const uint64_t *umi_caps, uint32_t n_m);
int fastf_level_point_dir(float rate_cell, uint64_t umi_cap, char *buf, size_t cap);
const char *fastf_level_header(void);
const char *fastf_level_genes_header(void);
const char *fastf_level_cells_header(void);
const char *fastf_level_reps_header(void);
const char *fastf_level_genes_reps_header(void);
int fastf_level_summary_row(float rate_cell, uint64_t umi_cap, uint32_t seed, const uint64_t counters[3], uint64_t nnz, uint64_t umis,
                            const uint64_t *umis_per_cell, const uint32_t *genes_per_cell, uint32_t n_cells, uint64_t hits,
                            uint32_t cells_capped, char *buf, size_t cap);

/* --- --fidelity on sweep, cap and level (FASTF_*_FIDELITY, flag 32; `fidelity=True` in Python): how well every grid point still
 * reproduces the full-depth data of the same cells.
 * For a (cell rate, seed) pair, the FULL MATRIX X is what a point gives when every CB hit of the pair's sampled cells is kept: the
 * all-ones decision plane — cap's T = 2^32, level's pass 0.  It is not `-r 1.0`, which drops a draw of 0xFFFFFFFF.
 * For a grid point with matrix Y, and every sampled cell k, in the order of barcodes.tsv.gz:
 *   umis_full  = sum over g of x             umis  = sum over g of y
 *   genes_full = rows of X with count >= 1   genes = rows of Y with count >= 1
 *   sum_xx = sum of x^2      sum_yy = sum of y^2
 *   sum_xy = sum of x * y, over the rows of Y, each joined with the row of X of the same (cell, feature)
 * All seven are u64 and exact: every sum is at most (sum of x)^2 < 2^64, because the sum of all counts is below 2^32.  Every point of
 * a pair keeps a subset of the pair's hits, so every row of Y has its partner in X; a row without one is an error
 * (FASTF_ERR_NO_PARTNER).
 * With G = the number of features, in exact 128-bit integers:
 *   num = G * sum_xy - umis_full * umis      dx = G * sum_xx - umis_full^2      dy = G * sum_yy - umis^2
 *   pearson = (double)num / (sqrt((double)dx) * sqrt((double)dy)), or NA when dx == 0 or dy == 0
 *   cosine  = (double)sum_xy / (sqrt((double)sum_xx) * sqrt((double)sum_yy)), or NA when either sum is 0
 * Both are printed %.6f.  They are correlations of the RAW counts over ALL G genes (the zeros included), not of log-normalised values.
 *   <point dir>/fidelity.tsv.gz (not with --summary-only): a header and one row per sampled cell:
 *     barcode umis_full umis genes_full genes sum_xx sum_yy sum_xy pearson cosine
 *   <out_dir>/<verb>_fidelity.tsv: a header and one row per point — in replicate runs per (cell rate, seed, list value), as <verb>.tsv —
 *     through .partial, with --summary-only too: the verb's two leading columns, then
 *     seed n_cells cells_defined median_pearson p10_pearson mean_pearson median_cosine umis_kept genes_kept
 *     cells_defined = the cells whose pearson is not NA (their cosine is defined too); the four statistics run over those cells:
 *     the median by the rule of <verb>.tsv's medians (the mean of the two middle values for an even number), p10 = the value at index
 *     floor(0.1 * (n - 1)) of the ascending values, the mean summed in ascending order; all four NA when cells_defined == 0.
 *     umis_kept = sum of umis / sum of umis_full, genes_kept likewise (NA when the denominator is 0).  All %.6f.
 * Every other output is the bytes it is without the flag.  A job outside the resident form (keys wider than 64 bits, UMIs beyond what a
 * 64-bit key holds, several devices) is refused with the flag, as with --cells. --- */
#define FASTF_SWEEP_FIDELITY 32u             /* bits 4 and 16 are not assigned: tests/test_genes_host.py and tests/test_cells_host.py pin them as the unknown bits that are refused */
#define FASTF_CAP_FIDELITY   32u
#define FASTF_LEVEL_FIDELITY 32u
const char *fastf_fidelity_header(void);          /* the header of fidelity.tsv.gz */
const char *fastf_sweep_fidelity_header(void);    /* the headers of <verb>_fidelity.tsv */
const char *fastf_cap_fidelity_header(void);
const char *fastf_level_fidelity_header(void);
/* one row of fidelity.tsv.gz (with its newline) from the seven integers of a cell */
int fastf_fidelity_row(const char *barcode, uint64_t umis_full, uint64_t umis, uint64_t genes_full, uint64_t genes, uint64_t sum_xx,
                       uint64_t sum_yy, uint64_t sum_xy, uint64_t n_features, char *buf, size_t cap);
/* the two metrics of a cell; returns bit 0: pearson is defined, bit 1: cosine is defined (an undefined one is left untouched) */
int fastf_fidelity_metrics(uint64_t umis_full, uint64_t umis, uint64_t sum_xx, uint64_t sum_yy, uint64_t sum_xy, uint64_t n_features,
                           double *pearson, double *cosine);
/* one row of <verb>_fidelity.tsv (with its newline); the second column as fastf_genes_summary_row prints it (list_value == 0: rate_depth) */
int fastf_fidelity_summary_row(float rate_cell, float rate_depth, uint64_t list_value, uint32_t seed, const uint64_t *umis_full,
                               const uint64_t *umis, const uint32_t *genes_full, const uint32_t *genes, const uint64_t *sum_xx,
                               const uint64_t *sum_yy, const uint64_t *sum_xy, uint32_t n_cells, uint64_t n_features, char *buf, size_t cap);

/* --- --gene-fidelity on sweep, cap and level (FASTF_*_GENE_FIDELITY, flag 128; `gene_fidelity=True` in Python; the long option
 * alone): the comparison of --fidelity along the other axis — does a gene's expression pattern across the cells survive the
 * downsampling, and are the genes that full depth ranks as highly variable still ranked so at a point.
 * For a (cell rate, seed) pair X is the full matrix exactly as --fidelity defines it (the all-ones decision plane, not `-r 1.0`), Y the
 * matrix of a grid point, n the number of sampled cells (the lines of the point's barcodes.tsv.gz).  For every feature g, over ALL n
 * sampled cells, zeros included:
 *   sum_x  = sum of x      cells_full = rows of X of gene g with count >= 1      sum_xx = sum of x^2
 *   sum_y  = sum of y      cells      = rows of Y of gene g with count >= 1      sum_yy = sum of y^2
 *   sum_xy = sum of x * y over the rows of Y, each joined with the row of X of the same (cell, feature)
 * All seven are u64 and exact: every sum is at most (sum of x)^2 < 2^64, because the sum of all counts is below 2^32.  A row of Y
 * without a partner is an error (FASTF_ERR_NO_PARTNER).
 * In exact 128-bit integers up to one conversion to double each:
 *   num = n * sum_xy - sum_x * sum_y      dx = n * sum_xx - sum_x^2      dy = n * sum_yy - sum_y^2
 *   pearson   = (double)num / (sqrt((double)dx) * sqrt((double)dy)), NA when dx == 0 or dy == 0
 *   disp_full = (double)dx / ((double)(n - 1) * (double)sum_x), NA when n < 2 or sum_x == 0      (variance / mean of the raw counts)
 *   disp      = (double)dy / ((double)(n - 1) * (double)sum_y), NA when n < 2 or sum_y == 0
 * Highly variable genes: K = min(FASTF_HVG_TOP, genes whose disp_full is defined); A = the first K genes by descending disp_full, ties
 * by ascending feature index; B = the first min(K, genes with disp defined) genes by descending disp, the same tie rule;
 * hvg_overlap = |A and B| / K, NA when K == 0.  Both ranking values are IEEE doubles computed in the operation order above.
 *   <point dir>/gene_fidelity.tsv.gz (not with --summary-only): a header and one row per feature in the order of features.tsv.gz, the
 *     feature named by its id as genes.tsv.gz names it:
 *     feature sum_x sum_y cells_full cells sum_xx sum_yy sum_xy pearson disp_full disp          (floats %.6f or NA)
 *   <out_dir>/<verb>_gene_fidelity.tsv: a header and one row per point — in replicate runs per (cell rate, seed, list value), in the
 *     row order of <verb>_fidelity.tsv — through .partial, with --summary-only too: the verb's two leading columns, then
 *     seed n_cells genes_full genes_defined median_pearson p10_pearson mean_pearson hvg_k hvg_overlap
 *     genes_full = genes with sum_x > 0; genes_defined = genes whose pearson is not NA; median, p10 and mean by the rules of
 *     <verb>_fidelity.tsv over those genes, NA when genes_defined == 0; hvg_k = K.
 * The flag works without --fidelity and --genes and keeps the pair's full rows by itself.  Every other output is the bytes it is
 * without the flag.  Jobs outside the resident form are refused as --fidelity refuses them.  No _reps aggregate is written. --- */
#define FASTF_SWEEP_GENE_FIDELITY 128u       /* bits 4, 16 and 64 are not assigned: tests pin them as the unknown bits that are refused */
#define FASTF_CAP_GENE_FIDELITY   128u
#define FASTF_LEVEL_GENE_FIDELITY 128u
#define FASTF_HVG_TOP 2000u
const char *fastf_gene_fidelity_header(void);          /* the header of gene_fidelity.tsv.gz */
const char *fastf_sweep_gene_fidelity_header(void);    /* the headers of <verb>_gene_fidelity.tsv */
const char *fastf_cap_gene_fidelity_header(void);
const char *fastf_level_gene_fidelity_header(void);
/* the three metrics of a gene over n_cells sampled cells; returns bit 0: pearson is defined, bit 1: disp_full, bit 2: disp (an
 * undefined one is left untouched) */
int fastf_gene_fidelity_metrics(uint64_t n_cells, uint64_t sum_x, uint64_t sum_y, uint64_t sum_xx, uint64_t sum_yy, uint64_t sum_xy,
                                double *pearson, double *disp_full, double *disp);
/* one row of gene_fidelity.tsv.gz (with its newline) from the seven integers of a gene */
int fastf_gene_fidelity_row(const char *feature, uint64_t n_cells, uint64_t sum_x, uint64_t sum_y, uint64_t cells_full, uint64_t cells, uint64_t sum_xx,
                            uint64_t sum_yy, uint64_t sum_xy, char *buf, size_t cap);
/* one row of <verb>_gene_fidelity.tsv (with its newline), the ranking of the highly variable genes included; the second column as
 * fastf_genes_summary_row prints it (list_value == 0: rate_depth) */
int fastf_gene_fidelity_summary_row(float rate_cell, float rate_depth, uint64_t list_value, uint32_t seed, uint32_t n_cells, const uint64_t *sum_x,
                                    const uint64_t *sum_y, const uint64_t *sum_xx, const uint64_t *sum_yy, const uint64_t *sum_xy, uint32_t n_features,
                                    char *buf, size_t cap);

/* --- --neighbors on sweep, cap and level (FASTF_*_NEIGHBORS, flag 512; `neighbors=True` in Python; the long option alone): the third
 * comparison with full depth, BETWEEN the cells — does a cell keep the nearest neighbours it has at full depth, on the genes a
 * clustering would use.  For a (cell rate, seed) pair X is the full matrix exactly as --fidelity defines it, Y the matrix of a grid
 * point, n the number of sampled cells.  A is the highly variable gene set of --gene-fidelity: the first
 * K = min(FASTF_HVG_TOP, genes with disp_full defined) genes by descending disp_full, ties by ascending feature index (fastf_hvg_rank:
 * the same doubles in the same operation order).  A is fixed per pair: it is used for X and for every Y of the pair.
 * For a matrix M (X or Y) restricted to the genes of A, with v_i the count vector of cell i:
 *   d_ij = v_i . v_j        n_i = d_ii
 *   N_M(i) = the first min(k, #{j != i : d_ij > 0}) cells j != i with d_ij > 0 by descending cosine d_ij / sqrt(n_i n_j), ties by
 *            ascending cell index.  Decided exactly: j precedes l iff d_ij^2 n_l > d_il^2 n_j, or the two products are equal and
 *            j < l — in 128-bit unsigned integers; no floating point takes part in the selection.
 * k = FASTF_NEIGHBORS_K = 15 in the three verbs; the device entry point and the host twin take k from 1 to 64.
 * Range: the largest n_i is read back (one reduction) and a pair whose value is 2^42 or more is refused (FASTF_ERR_NEIGHBOR_NORM in
 * the message: fastf_neighbors_check_norm).  Below it d_ij <= sqrt(n_i n_j) < 2^42, so every product stays below 2^126.  The counts go
 * to the device's matrix cores as digits of 7 bits; a count of 2^21 or more among the genes of A is refused likewise
 * (FASTF_ERR_NEIGHBOR_COUNT).
 * Per cell at a point:  k_full = |N_X(i)|   k_point = |N_Y(i)|   shared = |N_X(i) and N_Y(i)|   overlap = shared / k_full (%.6f; NA when
 * k_full == 0).
 *   <point dir>/neighbors.tsv.gz (not with --summary-only): a header and one row per barcode in the order of barcodes.tsv.gz:
 *     barcode k_full k_point shared overlap
 *   <out_dir>/<verb>_neighbors.tsv: a header and one row per point — in replicate runs per (cell rate, seed, list value), in the row
 *     order of <verb>_fidelity.tsv — through .partial, with --summary-only too: the verb's two leading columns, then
 *     seed n_cells hvg_k k cells_defined median_overlap p10_overlap mean_overlap mean_k_point
 *     cells_defined = cells with k_full > 0; median, p10 and mean of the overlap by the rules of <verb>_fidelity.tsv over those cells, NA
 *     when there is none; mean_k_point = the mean of k_point over all n cells (%.6f; NA when n == 0); hvg_k = K.
 * The flag works without --fidelity, --gene-fidelity and --genes: it keeps the pair's full rows and ranks A by itself.  Every other
 * output is the bytes it is without the flag.  Jobs outside the resident form are refused as --fidelity refuses them.  No _reps
 * aggregate is written. --- */
#define FASTF_SWEEP_NEIGHBORS 512u           /* bits 4, 16, 64 and 256 are not assigned: tests pin them as the unknown bits that are refused */
#define FASTF_CAP_NEIGHBORS   512u
#define FASTF_LEVEL_NEIGHBORS 512u
#define FASTF_NEIGHBORS_K 15u
#define FASTF_NEIGHBORS_MAX_K 64u
#define FASTF_NEIGHBORS_NONE 0xFFFFu         /* the slot of a feature that is not in A */
const char *fastf_neighbors_header(void);          /* the header of neighbors.tsv.gz */
const char *fastf_sweep_neighbors_header(void);    /* the headers of <verb>_neighbors.tsv */
const char *fastf_cap_neighbors_header(void);
const char *fastf_level_neighbors_header(void);
/* the ranking both --gene-fidelity and --neighbors use: genes[0 .. K) = the first K = min(FASTF_HVG_TOP, genes whose dispersion is
 * defined) genes (0-based) by descending dispersion of (sum, sum_sq) over n_cells cells, ties by ascending index; genes holds
 * FASTF_HVG_TOP entries (NULL: K alone); *n_defined (may be NULL) the genes whose dispersion is defined.  Returns K */
uint32_t fastf_hvg_rank(uint32_t n_cells, const uint64_t *sum, const uint64_t *sum_sq, uint32_t n_features, uint32_t *genes, uint32_t *n_defined);
/* slot_map[f] (u16, n_features + 1 entries, f the 1-based feature) = the rank of feature f in genes[0 .. K), FASTF_NEIGHBORS_NONE for
 * every other feature and for f == 0; fails when K exceeds FASTF_HVG_TOP or a gene is outside the list or named twice */
int fastf_neighbors_slot_map(const uint32_t *genes, uint32_t K, uint32_t n_features, uint16_t *slot_map);
/* the padded shape of the device's byte planes for n_cells cells and K genes: n_pad rows (a multiple of 128) of K_pad bytes (a multiple
 * of 32, at least 32) */
void fastf_neighbors_pad(uint32_t n_cells, uint32_t K, uint32_t *n_pad, uint32_t *K_pad);
/* the range rule: fails, naming FASTF_ERR_NEIGHBOR_NORM, when max_norm >= 2^42 */
int fastf_neighbors_check_norm(uint64_t max_norm);
/* one row of neighbors.tsv.gz (with its newline) */
int fastf_neighbors_row(const char *barcode, uint32_t k_full, uint32_t k_point, uint32_t shared, char *buf, size_t cap);
/* one row of <verb>_neighbors.tsv (with its newline); the second column as fastf_genes_summary_row prints it (list_value == 0:
 * rate_depth) */
int fastf_neighbors_summary_row(float rate_cell, float rate_depth, uint64_t list_value, uint32_t seed, uint32_t n_cells, uint32_t hvg_k, uint32_t k,
                                const uint32_t *k_full, const uint32_t *k_point, const uint32_t *shared, char *buf, size_t cap);

/* --- co-expression partners against full depth: the fourth comparison, BETWEEN THE GENES — does a gene keep the partners
 * it is co-expressed with at full depth.  X is the full-depth rows of a (cell rate, seed) pair, Y the rows of a grid point, A the K
 * highly variable genes --neighbors uses (slot g of A is the gene of rank g of fastf_hvg_rank), n the sampled cells of the pair; cells
 * without a count are included.  For M in {X, Y} and slots g, h of A, with m_ig the raw count of cell i (0 without a row):
 *   S_g = sum_i m_ig      Q_g = sum_i m_ig^2      D_gh = sum_i m_ig m_ih      (Q_g = D_gg)
 *   c_gh = n D_gh - S_g S_h (signed)              V_g = n Q_g - S_g^2 (>= 0)
 *   P_M(g) = the first min(k, #{h != g : c_gh > 0}) slots h != g with c_gh > 0 by descending Pearson c_gh / sqrt(V_g V_h).  Decided
 *            exactly: for fixed g, h precedes l iff c_gh^2 V_l > c_gl^2 V_h, or the two products are equal and h < l — in unsigned
 *            integers of 256 bits (coexpr_order.h); no floating point takes part in the selection.  A gene with V = 0 is nobody's
 *            partner and has none: c > 0 implies both V > 0.
 * k = FASTF_COEXPR_K = 15; the host calls take k from 1 to 64.
 * Range: a pair with n * max_g Q_g >= 2^63 is refused by name (FASTF_ERR_COEXPR_RANGE in the message: fastf_coexpr_check_range).  Below
 * it |c| <= n sqrt(Q_g Q_h) < 2^63 and V < 2^63, so every product stays below 2^189.  A count of 2^21 or more among the genes of A is
 * refused as --neighbors refuses it (FASTF_ERR_NEIGHBOR_COUNT): the three 7-bit digit planes of that option are the range of this one.
 * --coexpression on sweep, cap and level (FASTF_*_COEXPRESSION, flag 4096; `coexpression=True` in Python; the long option alone) computes
 * it on the device (fastf_dev_coexpr_sums, fastf_dev_coexpr_select below) for the full rows of every pair and for every point, and writes
 * <out_dir>/<verb>_coexpr.tsv (one row per point, through .partial, with --summary-only too; in replicate runs one row per (cell rate,
 * seed, list value) and no _reps table) and <point dir>/coexpr.tsv.gz (not with --summary-only).  Alone it keeps the full rows, the
 * pair's per-gene sums and the slot map of A, and nothing of the neighbour sets; every other output is the bytes it is without the
 * option.  Jobs outside the resident form are refused as --neighbors refuses them, naming --coexpression.
 * Per gene at a point:  k_full = |P_X(g)|   k_point = |P_Y(g)|   shared = |P_X(g) and P_Y(g)|.
 *   one row per gene of A in rank order (fastf_coexpr_header, fastf_coexpr_row):   gene k_full k_point shared      (gene: the feature id)
 *   one row per point (fastf_<verb>_coexpr_header, fastf_coexpr_summary_row): the verb's two leading columns, then
 *     seed n_cells hvg_k k genes_defined sum_k_full sum_k_point sum_shared mean_kept genes_half_kept
 *     genes_defined = genes with k_full > 0; mean_kept = the mean of shared / k_full over those genes (%.6f; NA when there is none);
 *     genes_half_kept = those of them with 2 shared >= k_full.  Ratios are formed only where they are printed. --- */
#define FASTF_SWEEP_COEXPRESSION 4096u       /* bits 1024 and 2048 are not assigned: tests pin them as the unknown bits that are refused */
#define FASTF_CAP_COEXPRESSION   4096u
#define FASTF_LEVEL_COEXPRESSION 4096u
#define FASTF_COEXPR_K 15u
#define FASTF_COEXPR_CHUNK 8192u             /* the cells a wave of the Gram kernel reduces before it adds into D; FASTF_COEXPR_CHUNK lowers it */
#define FASTF_COEXPR_MAX_K 64u
#define FASTF_COEXPR_MAX_PLANES 3u
#define FASTF_COEXPR_MAX_GENES 4096u
const char *fastf_coexpr_header(void);             /* the header of the per-gene rows */
const char *fastf_sweep_coexpr_header(void);       /* the headers of the per-point rows */
const char *fastf_cap_coexpr_header(void);
const char *fastf_level_coexpr_header(void);
/* the range rule of the selection: fails, naming FASTF_ERR_COEXPR_RANGE, when n_cells * max_q >= 2^63 */
int fastf_coexpr_check_range(uint32_t n_cells, uint64_t max_q);
/* the bound of the sums of products alone: fails, naming FASTF_ERR_COEXPR_CELLS, when n_cells * (2^(7 planes) - 1)^2 >= 2^64 — D_gh would leave
 * u64 — and for planes outside 1 .. 3 */
int fastf_coexpr_check_gram(uint32_t n_cells, uint32_t planes);
/* one per-gene row (with its newline) */
int fastf_coexpr_row(const char *gene, uint32_t k_full, uint32_t k_point, uint32_t shared, char *buf, size_t cap);
/* one per-point row (with its newline) over the hvg_k genes of A; the second column as fastf_genes_summary_row prints it (list_value == 0:
 * rate_depth) */
int fastf_coexpr_summary_row(float rate_cell, float rate_depth, uint64_t list_value, uint32_t seed, uint32_t n_cells, uint32_t hvg_k, uint32_t k,
                             const uint32_t *k_full, const uint32_t *k_point, const uint32_t *shared, char *buf, size_t cap);

/* --- --labels FILE on sweep, cap and level (fastf_sweep_labels, fastf_cap_labels, fastf_level_labels; `labels=` in Python; the long
 * option alone): do the cell types survive at this depth.  The user brings one label per barcode from the full-depth analysis; the
 * neighbour sets of --neighbors turn them into votes.
 * The file: plain text, one `barcode<TAB>label` per line, lines end in LF, one trailing CR is dropped, empty lines are skipped.  The
 * first line is a header, and skipped, iff its first field is exactly `barcode`.  A barcode is matched as the exact string
 * barcodes.tsv.gz prints for a cell; a label is 1 to 63 bytes without a tab; the label `NA` means unlabelled.  Refused by name, with the
 * line number, before the output directory is made: a file that does not exist or starts with the gzip magic, a line without exactly
 * two fields, a label that is empty or 64 bytes or longer, a barcode named twice, more than FASTF_LABELS_MAX distinct labels, and a
 * file of which no line names a barcode of the barcode list.  A barcode that is not in the barcode list is counted (labels_unknown in
 * the stage line) and ignored; a listed barcode without a line is unlabelled.
 * Label ids: 1 .. L in ascending bytewise order of the label strings (on a common prefix the shorter first), whatever the order of the
 * file; 0 is unlabelled.  Per (cell rate, seed) pair lab[i] (u8) for the n sampled cells in the order of barcodes.tsv.gz.
 * X, Y, A, N_M(i) and k = FASTF_NEIGHBORS_K are exactly those of --neighbors.  For M in {X, Y}:
 *   votes_M(i, l) = #{ j in N_M(i) : lab[j] == l } for l in 1 .. L (unlabelled neighbours do not vote)
 *   labelled_M(i) = sum_l votes_M(i, l)
 *   same_M(i)     = votes_M(i, lab[i]), 0 when lab[i] == 0
 *   pred_M(i)     = the l with the most votes, ties to the smallest l; 0 when labelled_M(i) == 0 (cells with lab[i] == 0 are predicted too)
 *   conf_M[a][b]  = #{ i : lab[i] == a, pred_M(i) == b } for a in 1 .. L, b in 0 .. L (u32)
 * Everything is integers; no floating point is used before the printing.
 *   <point dir>/labels.tsv.gz (not with --summary-only): a header and one row per barcode in the order of barcodes.tsv.gz:
 *     barcode label pred_full pred_point same_full labelled_full same_point labelled_point     (labels as their strings, NA for 0)
 *   <point dir>/label_confusion.tsv.gz (not with --summary-only): the header `label cells NA <label 1> ... <label L>` and one row per
 *     label a: cells = #{i : lab[i] == a}, then conf_Y[a][0 .. L]
 *   <out_dir>/<verb>_labels.tsv: a header and one row per point — in replicate runs per (cell rate, seed, list value), in the row
 *     order of <verb>_neighbors.tsv — through .partial, with --summary-only too: the verb's two leading columns, then
 *     seed n_cells k n_labels cells_labelled agree_full agree_point accuracy_full accuracy_point kept purity_full purity_point
 *     agree_M = sum_a conf_M[a][a]; accuracy_M = agree_M / cells_labelled; kept = #{i : lab[i] >= 1, pred_X(i) == lab[i],
 *     pred_Y(i) == lab[i]} / agree_full; purity_M = sum same_M / sum labelled_M over the cells with lab[i] >= 1; the ratios %.6f, NA on a
 *     zero denominator
 *   <out_dir>/<verb>_label_classes.tsv likewise, one row per (point, label): the leading columns and seed, then
 *     label cells correct_full correct_point predicted_full predicted_point
 *     correct_M = conf_M[a][a], predicted_M = the column sum of conf_M over a
 * No _reps aggregate is written.  The option switches on, by itself, the full-depth rows, the per-gene sums that rank A and the
 * neighbour sets of --neighbors, and writes none of that option's files unless it is given too; every other output is the bytes it is
 * without the option.  Jobs outside the resident form are refused as --neighbors refuses them, naming --labels. --- */
#define FASTF_LABELS_MAX 255u
#define FASTF_LABEL_BYTES 64u                /* a label with its terminator */
typedef struct fastf_labels fastf_labels_t;
/* the labels file against the barcode list file (every line of it, cut as the list loader cuts it); on failure *out is NULL and
 * fastf_last_error() names the file and the line */
int fastf_labels_load(const char *labels_file, const char *barcodes_file, fastf_labels_t **out);
void fastf_labels_free(fastf_labels_t *t);
uint32_t fastf_labels_count(const fastf_labels_t *t);                        /* L */
const char *fastf_labels_name(const fastf_labels_t *t, uint32_t id);         /* id 0: "NA"; beyond L: NULL */
uint64_t fastf_labels_unknown(const fastf_labels_t *t);                      /* lines whose barcode is not in the barcode list */
uint64_t fastf_labels_known(const fastf_labels_t *t);                        /* lines whose barcode is */
uint32_t fastf_labels_id(const fastf_labels_t *t, const char *barcode);      /* 0: no line, or NA */
/* lab[i] = fastf_labels_id(t, barcodes[i]) for n barcodes */
int fastf_labels_assign(const fastf_labels_t *t, char *const *barcodes, uint32_t n, uint8_t *lab);
/* the host twin of fastf_dev_label_votes: the same arguments on host arrays.  idx: k slots a cell, cnt[i] of them valid (more than k
 * counts as k); no slot from cnt[i] on is read as an index, an index of n_cells and beyond and a label above n_labels count as
 * unlabelled.  conf (n_labels * (n_labels + 1) u32) is zeroed by the call */
int fastf_label_votes(const uint32_t *idx, const uint32_t *cnt, const uint8_t *lab, uint32_t n_cells, uint32_t k, uint32_t n_labels,
                      uint8_t *pred, uint8_t *same, uint8_t *labelled, uint32_t *conf);
const char *fastf_labels_header(void);             /* the header of labels.tsv.gz */
const char *fastf_sweep_labels_header(void);       /* the headers of <verb>_labels.tsv */
const char *fastf_cap_labels_header(void);
const char *fastf_level_labels_header(void);
const char *fastf_sweep_label_classes_header(void);    /* the headers of <verb>_label_classes.tsv */
const char *fastf_cap_label_classes_header(void);
const char *fastf_level_label_classes_header(void);
/* one row of labels.tsv.gz (with its newline); the three labels as their strings */
int fastf_labels_row(const char *barcode, const char *label, const char *pred_full, const char *pred_point, uint32_t same_full, uint32_t labelled_full,
                     uint32_t same_point, uint32_t labelled_point, char *buf, size_t cap);
/* the header of label_confusion.tsv.gz for names[1 .. n_labels] (names[0] is not read), and the row of one label: conf_row[0 .. n_labels] */
int fastf_label_confusion_header(const char *const *names, uint32_t n_labels, char *buf, size_t cap);
int fastf_label_confusion_row(const char *label, uint32_t cells, const uint32_t *conf_row, uint32_t n_labels, char *buf, size_t cap);
/* one row of <verb>_labels.tsv (with its newline); the second column as fastf_genes_summary_row prints it (list_value == 0: rate_depth) */
int fastf_labels_summary_row(float rate_cell, float rate_depth, uint64_t list_value, uint32_t seed, uint32_t n_cells, uint32_t k, uint32_t n_labels,
                             const uint8_t *lab, const uint8_t *pred_full, const uint8_t *pred_point, const uint8_t *same_full, const uint8_t *labelled_full,
                             const uint8_t *same_point, const uint8_t *labelled_point, const uint32_t *conf_full, const uint32_t *conf_point,
                             char *buf, size_t cap);
/* one row of <verb>_label_classes.tsv (with its newline) for label a (1 .. n_labels) */
int fastf_label_classes_row(float rate_cell, float rate_depth, uint64_t list_value, uint32_t seed, const char *label, uint32_t a, uint32_t n_cells,
                            uint32_t n_labels, const uint8_t *lab, const uint32_t *conf_full, const uint32_t *conf_point, char *buf, size_t cap);
/* sweep, cap and level with --labels: the arguments of the verb's _reps call, then seed and labels_path.  n_seeds == 0: the plain run at
 * `seed` (the directories and tables fastf_sweep() writes; seeds is not read); n_seeds >= 1: the replicate run.  labels_path == NULL:
 * exactly the existing call.  flags: the existing word, no new bit */
int fastf_sweep_labels(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                       const float *rates_depth, uint32_t n_r, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path);
int fastf_cap_labels(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                     const uint64_t *caps, uint32_t n_n, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path);
int fastf_level_labels(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                       const uint64_t *umi_caps, uint32_t n_m, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path);

/* --- --markers N on sweep, cap and level, with --labels (fastf_sweep_markers, fastf_cap_markers, fastf_level_markers; `markers=N` in
 * Python; the long option alone; no new flag bit): do the marker genes of the cell types survive at this depth.  X, Y, A (K genes, slot
 * g of A is the gene of rank g of fastf_hvg_rank) and lab[] are those of --neighbors and --labels.  Only labelled sampled cells take
 * part (lab[i] in 1 .. L): n_lab of them, n_a with label a, n_out = n_lab - n_a.  For a matrix M (X or Y) and a gene g of A, x_i is the
 * raw count of cell i (0 without a row).  The statistic is the Mann-Whitney U of label a against all other labelled cells, doubled:
 *   2U_M[a][g] = sum over i in a, j labelled and not in a, of 2 * (x_i > x_j) + (x_i == x_j)
 * computed per gene from E(v) = #{labelled cells with x == v} and C(v) = #{labelled cells with x < v} as
 *   2U_M[a][g] = sum over i in a of (2 C(x_i) + E(x_i)) - n_a^2        (the same sum over the pairs inside a is exactly n_a^2)
 * in integers alone; AUC = 2U / (2 n_a n_out) is formed only where it is printed.  Beside it, per (label, gene):
 *   det_M[a][g] = #{i in a : x_i > 0} (u32)        sum_M[a][g] = sum over i in a of x_i (u64)
 * Ranking: for a label with n_a >= 1 and n_out >= 1 the genes of A by descending 2U, ties by ascending feature number; rank 1 is the
 * best.  Its markers are the first N_eff = min(N, K).  A label with n_a == 0 or n_out == 0 has no ranking (rank 0) and prints NA.
 * Range: counts of the genes of A below 2^14 (one or two byte planes).  A (cell rate, seed) pair whose full rows need three planes is
 * refused for this option by name (FASTF_ERR_MARKER_COUNT in the message), as --neighbors refuses 2^21: the rank table of a gene — E,
 * then 2C + E, one u32 per possible count — lives in the LDS of the device, 64 KB a gene at 2^14 counts.
 *   <point dir>/markers.tsv.gz (not with --summary-only): a header and, per label in id order, one row per gene in the union of the
 *     label's markers at full depth and at the point, by ascending rank_full:
 *     label gene rank_full rank_point auc_full auc_point det_in_full det_out_full det_in_point det_out_point mean_in_point
 *     gene: the feature id; auc_M = 2U_M / (2 n_a n_out) (%.6f); det_in_M = det_M[a][g], det_out_M = sum over b != a of det_M[b][g];
 *     mean_in_point = sum_Y[a][g] / n_a (%.6f).  A label without a ranking has one row, NA in every column behind the label.
 *   <out_dir>/<verb>_markers.tsv: a header and per point — in replicate runs per (cell rate, seed, list value), in the row order of
 *     <verb>_labels.tsv — one row per label in id order and one row `all`, through .partial, with --summary-only too: the verb's two
 *     leading columns, then   seed label n_in n_out top kept auc_full_mean auc_point_mean
 *     n_in = n_a, n_out as above, top = N_eff, kept = the genes in the label's markers at full depth AND at the point,
 *     auc_M_mean = the mean of auc_M over the label's markers AT FULL DEPTH: (sum of 2U_M over them) / (2 n_a n_out) / N_eff (%.6f);
 *     a label without a ranking prints NA in the last three.  The `all` row: n_in, n_out, top and kept summed over the labels (top and
 *     kept over those with a ranking), the two means pooled over every (label, marker) pair of those labels, NA when there is none.
 * The option needs --labels (refused without it, and for N outside 1 .. FASTF_MARKERS_MAX, before the output directory is made) and
 * switches on what --labels switches on; every other output is the bytes it is without the option.  No _reps aggregate is written. --- */
#define FASTF_MARKERS_MAX 2000u              /* N of --markers: 1 .. FASTF_HVG_TOP */
#define FASTF_MARKER_MAX_PLANES 2u
/* the host twin of fastf_dev_marker_auc: the same arguments on host arrays.  planes: n_planes byte planes of n_pad x K_pad
 * (fastf_neighbors_pad), plane p holds bits 7p .. 7p+6 of the count of (cell, slot); rows from n_cells on, slots from K on and bit 7 of
 * a byte are never used.  s2u, sum (u64) and det (u32): n_labels x K, [a - 1][slot]; n_per_label (u32, n_labels): the cells per label.
 * The call clears all four.  Refused: n_planes outside 1 .. 2 (FASTF_ERR_MARKER_COUNT), n_labels outside 1 .. FASTF_LABELS_MAX */
int fastf_marker_auc(const void *planes, uint32_t n_planes, uint32_t n_cells, uint32_t K, const uint8_t *lab, uint32_t n_labels,
                     uint64_t *s2u, uint32_t *det, uint64_t *sum, uint32_t *n_per_label);
/* which accumulator form one device call takes: 1 — in LDS beside the bins, 0 — global atomics (n_labels that do not fit: 226 and
 * more at one plane, none at two; and every call under FASTF_MARKERS_LDS=0), -1 — a call with these arguments is refused */
int fastf_marker_auc_form(uint32_t n_planes, uint32_t n_labels);
/* rank[(a - 1) * K + slot] (u32) = the rank, from 1, of the slot among the K slots of label a by descending s2u, ties by ascending
 * genes[slot] (genes == NULL: by ascending slot); 0 in every slot of a label with n_a == 0 or n_out == 0 */
int fastf_marker_rank(const uint64_t *s2u, const uint32_t *n_per_label, const uint32_t *genes, uint32_t K, uint32_t n_labels, uint32_t *rank);
const char *fastf_markers_header(void);            /* the header of markers.tsv.gz */
const char *fastf_sweep_markers_header(void);      /* the headers of <verb>_markers.tsv */
const char *fastf_cap_markers_header(void);
const char *fastf_level_markers_header(void);
/* one row of markers.tsv.gz (with its newline); gene == NULL, n_in == 0 or n_out == 0: the NA row of a label without a ranking */
int fastf_markers_row(const char *label, const char *gene, uint32_t n_in, uint32_t n_out, uint32_t rank_full, uint32_t rank_point, uint64_t s2u_full,
                      uint64_t s2u_point, uint32_t det_in_full, uint32_t det_out_full, uint32_t det_in_point, uint32_t det_out_point, uint64_t sum_in_point,
                      char *buf, size_t cap);
/* the n_labels + 1 rows of one point of <verb>_markers.tsv (with their newlines) into buf; names[1 .. n_labels] the labels (names[0] is
 * not read); top_n: N; the tables [a - 1][slot] over K slots; the second column as fastf_genes_summary_row prints it */
int fastf_markers_summary_rows(float rate_cell, float rate_depth, uint64_t list_value, uint32_t seed, const char *const *names, uint32_t n_labels, uint32_t K,
                               uint32_t top_n, const uint32_t *n_per_label, const uint32_t *rank_full, const uint32_t *rank_point, const uint64_t *s2u_full,
                               const uint64_t *s2u_point, char *buf, size_t cap);
/* sweep, cap and level with --labels and --markers: the arguments of the verb's _labels call, then N.  labels_path == NULL and N outside
 * 1 .. FASTF_MARKERS_MAX are refused */
int fastf_sweep_markers(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                        const float *rates_depth, uint32_t n_r, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path,
                        uint32_t markers);
int fastf_cap_markers(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                      const uint64_t *caps, uint32_t n_n, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path,
                      uint32_t markers);
int fastf_level_markers(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                        const uint64_t *umi_caps, uint32_t n_m, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path,
                        uint32_t markers);

/* --- --mapping on sweep, cap and level (fastf_sweep_mapping, fastf_cap_mapping, fastf_level_mapping; `mapping=True` in Python; the long
 * option alone; no flag bit): the cells of a point looked up in the full-depth data — the comparison that CROSSES the two depths.  Is a
 * point cell's own full-depth profile still its nearest full-depth cell; if not, how many got in front of it; does it land in the
 * neighbourhood its full-depth self has; do the labels around it still give its own label.  Per (cell rate, seed) pair:
 * X = the full-depth rows, Y = the point's rows, A and its slot map as --neighbors has them, n = the pair's cells; x_j, y_i the count
 * vectors over A;  e_ij = <y_i, x_j>  and  m_j = <x_j, x_j> (the full norms), both u64.
 * The query is y_i.  The candidates are ALL full-depth cells j with e_ij > 0.  Order: j precedes l iff e_ij^2 m_l > e_il^2 m_j, or these are
 * equal and j < l (|y_i| cancels) — in 128-bit unsigned integers, the compare of --neighbors; no floating point takes part until a ratio
 * is printed.
 *   M(i)         = the first k candidates j != i in that order; k = FASTF_MAPPING_K = 15 in the verbs, the device call and the host twin
 *                  take k from 1 to 64.  Written ascending by index, unused slots 0xFFFFFFFF, cnt[i] valid: the layout fastf_dev_neighbors
 *                  writes, so fastf_dev_neighbors_shared and fastf_dev_label_votes take it unchanged.
 *   self_dot(i)  = e_ii
 *   self_rank(i) = the number of candidates j != i that precede i, when e_ii > 0; FASTF_MAPPING_NO_RANK (printed NA) otherwise.  Rank 0:
 *                  the cell's own full-depth profile is its nearest.
 *   hood(i)      = |M(i) and N_X(i)|, N_X the full-depth neighbour set of --neighbors at the same k.
 *   with --labels: pred_map(i), same_map(i), labelled_map(i) are the vote of fastf_label_votes over M(i) with the pair's lab[], as that
 *                  call defines them.  Self is never in M, so the vote does not leak.
 * Range: the largest m_j AND the largest <y_i, y_i> are read back and a pair with either at 2^42 or beyond is refused
 * (FASTF_ERR_NEIGHBOR_NORM, through fastf_neighbors_check_norm); below that e_ij < 2^42 and every product stays under 2^126.  Counts of
 * 2^21 and beyond among A are refused as --neighbors refuses them.
 *   <point dir>/mapping.tsv.gz (not with --summary-only): a header and one row per barcode in the order of barcodes.tsv.gz:
 *     barcode self_dot self_rank k_map k_full hood pred_map      (k_map = |M(i)|, k_full = |N_X(i)|; pred_map the label string, NA without
 *     --labels or without a labelled neighbour)
 *   <out_dir>/<verb>_mapping.tsv: a header and one row per point — in replicate runs per (cell rate, seed, list value), as
 *     <verb>_neighbors.tsv — through .partial, with --summary-only too: the verb's two leading columns, then
 *     seed n_cells hvg_k k cells_defined self_top1 self_topk median_self_rank p90_self_rank mean_hood cells_labelled accuracy_map
 *     cells_defined = cells with self_dot > 0; self_top1, self_topk = the share of them with rank 0, rank < k (%.6f); median (%.6f, the mean
 *     of the two middle values) and p90 (the value at floor(0.9 (cells_defined - 1)) of the ascending ranks: the quantile rule of
 *     <verb>_fidelity.tsv) of the rank over them; mean_hood = the mean of hood / k_full over the cells with k_full > 0 (%.6f);
 *     cells_labelled = the cells with lab[i] >= 1; accuracy_map = sum same_map / sum labelled_map over those cells (%.6f): the share of the
 *     labelled full-depth cells a labelled cell maps among that carry its own label.  The last two are NA without --labels; NA wherever
 *     a denominator is 0.
 * The option switches on what --labels alone switches on — the full rows, the sums that rank A, both neighbour sets — and writes none of
 * the files of --neighbors unless that option is given too; every other output is the bytes it is without it.  Jobs outside the resident
 * form (several devices, the wide-UMI layout) are refused as --neighbors refuses them, naming --mapping.  No _reps aggregate. --- */
#define FASTF_MAPPING_K 15u
#define FASTF_MAPPING_NO_RANK 0xFFFFFFFFu
const char *fastf_mapping_header(void);            /* the header of mapping.tsv.gz */
const char *fastf_sweep_mapping_header(void);      /* the headers of <verb>_mapping.tsv */
const char *fastf_cap_mapping_header(void);
const char *fastf_level_mapping_header(void);
/* one row of mapping.tsv.gz (with its newline); self_rank == FASTF_MAPPING_NO_RANK and pred_map == NULL print NA */
int fastf_mapping_row(const char *barcode, uint64_t self_dot, uint32_t self_rank, uint32_t k_map, uint32_t k_full, uint32_t hood, const char *pred_map,
                      char *buf, size_t cap);
/* one row of <verb>_mapping.tsv (with its newline); the second column as fastf_genes_summary_row prints it (list_value == 0: rate_depth);
 * lab == NULL: a run without --labels (same_map and labelled_map are not read) */
int fastf_mapping_summary_row(float rate_cell, float rate_depth, uint64_t list_value, uint32_t seed, uint32_t n_cells, uint32_t hvg_k, uint32_t k,
                              const uint64_t *self_dot, const uint32_t *self_rank, const uint32_t *k_full, const uint32_t *hood, const uint8_t *lab,
                              const uint8_t *same_map, const uint8_t *labelled_map, char *buf, size_t cap);
/* sweep, cap and level with --mapping: the arguments of the verb's _markers call, then mapping (0 / 1).  labels_path may be NULL and
 * markers 0 here (markers != 0 still needs labels_path); mapping == 0: what the _markers, _labels or _reps call of the same arguments does */
int fastf_sweep_mapping(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                        const float *rates_depth, uint32_t n_r, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path,
                        uint32_t markers, uint32_t mapping);
int fastf_cap_mapping(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                      const uint64_t *caps, uint32_t n_n, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path,
                      uint32_t markers, uint32_t mapping);
int fastf_level_mapping(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                        const uint64_t *umi_caps, uint32_t n_m, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path,
                        uint32_t markers, uint32_t mapping);

/* --- --pseudotime FILE on sweep, cap and level (fastf_sweep_pseudotime, fastf_cap_pseudotime, fastf_level_pseudotime; `pseudotime=` in
 * Python; the long option alone; no flag bit): does a trajectory survive at this depth.  The user brings one number per barcode from the
 * full-depth analysis (a pseudotime, or any per-cell score); the neighbour sets of --neighbors estimate it back, at full depth and at
 * the point, and the order of the cells along the estimate is compared with the order along the value: the continuous counterpart of
 * --labels.  Everything is integer until a ratio is printed.
 * The file: plain text, one `barcode<TAB>value` per line, read under the rules of the labels file (one loader cuts the lines of both):
 * lines end in LF, one trailing CR is dropped, empty lines are skipped, the first line is skipped iff its first field is exactly
 * `barcode`, a barcode is the string barcodes.tsv.gz prints.  A value is 1 to 63 bytes: `NA` (no value), or a number that strtod in the C
 * locale consumes whole and that is finite.  Refused by name, with the line number, before the output directory is made: a file that
 * does not exist or is gzip-compressed, a line without exactly two fields, a value that is empty or 64 bytes or longer, a value strtod
 * does not consume whole, nan and inf (an overflow to inf too), a barcode named twice, and a file of which no line names a barcode of the
 * barcode list.  A barcode that is not in the barcode list is counted (pseudotime_unknown in the stage line) and ignored; a listed
 * barcode without a line has no value.
 * Per (cell rate, seed) pair, with its n sampled cells in the order of barcodes.tsv.gz; X, Y, A, N_M(i) and k = FASTF_NEIGHBORS_K are
 * those of --neighbors; m = the cells of the pair that have a value (cells_valued).
 *   t[i] (u32)  = the doubled midrank of cell i among those m cells:
 *                 2 * #{j valued : v_j < v_i} + #{j valued : v_j == v_i} + 1   (i counts itself in the second term): 2 .. 2m, ties share a
 *                 value; 0 without a value.  Doubles are compared as doubles: -0 equals 0.  Made on the host (fastf_ptime_assign), once a pair.
 * For M in {X, Y}, and Z with --mapping (M(i) of that option: a list over the full-depth cells of the same pair):
 *   V_M(i)      = the multiset { t[j] : j in N_M(i), t[j] > 0 };  c_M(i) = |V_M(i)|
 *   e_M(i)      = the LOWER median of V_M(i), its ceil(c / 2)-th smallest element; 0 when c_M(i) == 0.  Cells without a value of their own
 *                 are estimated too.  Slots from cnt[i] on and indices of n and beyond are never used, as in fastf_label_votes.
 * Census: S_M = { i : t[i] > 0, e_M(i) > 0 }.  Every pair i < j of S_M falls in exactly one of five u64 counts:
 *   conc      (e_i - e_j)(t_i - t_j) > 0          disc      (e_i - e_j)(t_i - t_j) < 0
 *   tie_e     e_i == e_j, t_i != t_j              tie_t     t_i == t_j, e_i != e_j              tie_both  both equal
 * and cells_M = |S_M|, shift_sum_M = sum over S_M of |e_M(i) - t[i]| (u64).
 * Printed, %.6f, NA on a zero denominator:
 *   tau_M   = (double)(int64)(conc - disc) / sqrt((double)(conc + disc + tie_e) * (double)(conc + disc + tie_t))    (Kendall's tau-b)
 *   shift_M = (double)shift_sum_M / ((double)(2 m) * (double)cells_M)                 (the mean displacement as a share of the rank range)
 *   <point dir>/pseudotime.tsv.gz (not with --summary-only): a header and one row per barcode in the order of barcodes.tsv.gz:
 *     barcode rank est_full valued_full est_point valued_point est_map valued_map      (rank = t; rank and est_* print NA for 0; the two
 *     map columns are NA without --mapping)
 *   <out_dir>/<verb>_pseudotime.tsv: a header and one row per point — in replicate runs per (cell rate, seed, list value), in the row
 *     order of <verb>_labels.tsv — through .partial, with --summary-only too: the verb's two leading columns, then
 *     seed n_cells k cells_valued   and per M in full, point, map:   cells_M conc_M disc_M tau_M shift_M      (the map columns NA without
 *     --mapping)
 * The option switches on what --labels alone switches on and writes none of the files of --neighbors unless that option is given too;
 * every other output is the bytes it is without it.  Jobs outside the resident form (several devices, the wide-UMI layout) are refused
 * as --neighbors refuses them, naming --pseudotime.  No _reps aggregate. --- */
#define FASTF_PTIME_TILE 1024u               /* the tile edge of the device census: cells per tile (PT_TILE) */
#define FASTF_PTIME_OUT_WORDS 7u             /* conc disc tie_e tie_t tie_both cells shift_sum */
#define FASTF_PTIME_MAX_CELLS (65535u * FASTF_PTIME_TILE)      /* the device census: the pairs of tiles stay below 2^31 workgroups */
typedef struct fastf_ptime fastf_ptime_t;
/* the pseudotime file against the barcode list file; on failure *out is NULL and fastf_last_error() names the file and the line */
int fastf_ptime_load(const char *ptime_file, const char *barcodes_file, fastf_ptime_t **out);
void fastf_ptime_free(fastf_ptime_t *t);
uint64_t fastf_ptime_known(const fastf_ptime_t *t);                          /* lines whose barcode is in the barcode list */
uint64_t fastf_ptime_unknown(const fastf_ptime_t *t);                        /* lines whose barcode is not */
uint64_t fastf_ptime_valued(const fastf_ptime_t *t);                         /* lines of a listed barcode that carry a value (not NA) */
/* rank[i] = t[i] of barcodes[i] among the n barcodes given, *m (may be NULL) = those of them with a value */
int fastf_ptime_assign(const fastf_ptime_t *t, char *const *barcodes, uint32_t n, uint32_t *rank, uint32_t *m);
/* the host twins of fastf_dev_ptime_medians and fastf_dev_ptime_census: the same arguments on host arrays.  idx: k slots a cell (k from 1
 * to 64), cnt[i] of them valid (more than k counts as k); est, valued: u32[n_cells].  The census is the definition, O(n_cells^2);
 * out: FASTF_PTIME_OUT_WORDS u64 */
int fastf_ptime_medians(const uint32_t *idx, const uint32_t *cnt, const uint32_t *t, uint32_t n_cells, uint32_t k, uint32_t *est, uint32_t *valued);
int fastf_ptime_census(const uint32_t *est, const uint32_t *t, uint32_t n_cells, uint64_t *out);
const char *fastf_ptime_header(void);              /* the header of pseudotime.tsv.gz */
const char *fastf_sweep_pseudotime_header(void);   /* the headers of <verb>_pseudotime.tsv */
const char *fastf_cap_pseudotime_header(void);
const char *fastf_level_pseudotime_header(void);
/* one row of pseudotime.tsv.gz (with its newline); mapping == 0: est_map and valued_map are not read and print NA */
int fastf_ptime_row(const char *barcode, uint32_t rank, uint32_t est_full, uint32_t valued_full, uint32_t est_point, uint32_t valued_point,
                    uint32_t est_map, uint32_t valued_map, int mapping, char *buf, size_t cap);
/* one row of <verb>_pseudotime.tsv (with its newline); the second column as fastf_genes_summary_row prints it (list_value == 0:
 * rate_depth); census_*: FASTF_PTIME_OUT_WORDS u64 each; census_map == NULL: a run without --mapping */
int fastf_ptime_summary_row(float rate_cell, float rate_depth, uint64_t list_value, uint32_t seed, uint32_t n_cells, uint32_t k, uint32_t cells_valued,
                            const uint64_t *census_full, const uint64_t *census_point, const uint64_t *census_map, char *buf, size_t cap);
/* sweep, cap and level with --pseudotime: the arguments of the verb's _mapping call, then pseudotime_path.  pseudotime_path == NULL:
 * exactly the _mapping call of the same arguments */
int fastf_sweep_pseudotime(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                           const float *rates_depth, uint32_t n_r, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path,
                           uint32_t markers, uint32_t mapping, const char *pseudotime_path);
int fastf_cap_pseudotime(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                         const uint64_t *caps, uint32_t n_n, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path,
                         uint32_t markers, uint32_t mapping, const char *pseudotime_path);
int fastf_level_pseudotime(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                           const uint64_t *umi_caps, uint32_t n_m, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path,
                           uint32_t markers, uint32_t mapping, const char *pseudotime_path);

/* --- replicate seeds of sweep and cap (--seeds a,b,c | --reps N; fastf_sweep_reps, fastf_cap_reps): the grid at several seeds from
 * ONE decode.  A replicate run is any run through these, one seed included; fastf_sweep() and fastf_cap() are what they were.
 *   point directories   <point name>_s<seed> (c0.500_r0.100_s927): the bytes `bam2db -s <seed>` (cap: `cap -s <seed>`) writes
 *   <verb>.tsv          today's header and rows, one per (cell rate, seed, depth | cap): cell rates outer, then the seeds as listed,
 *                       then the verb's list
 *   <verb>_reps.tsv     one row per grid point in grid order: rate_cell, rate_depth | reads_per_cell, n_reps, n_cells (the same at
 *                       every seed — the sample size depends on the rate alone; a run whose replicates disagree fails), then
 *                       <m>_mean <m>_sd <m>_min <m>_max for m = sampled_reads, sampled_valid_reads, nnz, umis, saturation,
 *                       median_umis_per_cell, median_genes_per_cell.  Mean and sd in double, two passes over the seeds in list
 *                       order, sd the sample sd (divisor n - 1), both %.6f, sd `NA` at one replicate; min and max in the
 *                       metric's own format of <verb>.tsv
 *   --genes             <verb>_genes.tsv one row per (point, seed), genes.tsv.gz per point directory; NO <verb>_gene_cells.tsv.gz;
 *                       <verb>_gene_reps.tsv.gz: header `feature` and per grid point p `<p>:reps_detected <p>:cells_sum
 *                       <p>:cells_sumsq`, one row per feature — the seeds at which at least one cell detects the gene, the sum and
 *                       the sum of squares over the seeds of the cells that detect it (exact u64; summed on the device:
 *                       fastf_dev_gene_reps_add); <verb>_genes_reps.tsv one row per grid point: rate_cell, rate_depth |
 *                       reads_per_cell, n_reps, genes_detected_mean _sd _min _max (the rule above), genes_in_all_reps,
 *                       genes_in_any_rep
 *   --cells             <verb>_cells.tsv one row per (point, seed), the seed in its third column as ever; cells.tsv.gz per point directory
 * Every table goes through .partial; on failure none is left.  sweep runs jobs outside the resident form point by point and seed by
 * seed through bam2db() into the same names; --cells and cap refuse them as without replicates. --- */
#define FASTF_MAX_SEEDS 64u
/* a comma-separated list of 1 .. FASTF_MAX_SEEDS seeds, each by the rule of -s (strtol(.., 0): decimal, 0x.., 0..; the value taken
 * modulo 2^32).  Refused, the message naming --seeds: an empty list or element, trailing characters, out of range, a value twice,
 * more than `cap` (at most FASTF_MAX_SEEDS) values */
int fastf_parse_seeds(const char *text, uint32_t *out, uint32_t cap, uint32_t *n_out);
/* --reps N from -s first: first, first + 1, .. first + N - 1; refused: N outside 1 .. FASTF_MAX_SEEDS, a run that wraps past 2^32 - 1 */
int fastf_reps_seeds(uint32_t first, uint64_t n_reps, uint32_t *out, uint32_t cap, uint32_t *n_out);
/* the arguments of fastf_sweep / fastf_cap with a list of 1 .. FASTF_MAX_SEEDS distinct seeds in place of `seed` */
int fastf_sweep_reps(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                     const float *rates_depth, uint32_t n_r, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags);
int fastf_cap_reps(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                   const uint64_t *caps, uint32_t n_n, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags);
/* the host pieces: `<point>_s<seed>`; the header lines; one row of <verb>_reps.tsv (with its newline) from the metrics of the
 * replicates — metrics[k * FASTF_REPS_METRICS + m], m in the order above, the integers as doubles (exact below 2^53);
 * reads_per_cell == 0: a sweep row, >= 1: a cap row; one row of <verb>_genes_reps.tsv; the host form of fastf_dev_gene_reps_add */
#define FASTF_REPS_METRICS 7u
int fastf_reps_point_dir(const char *point_name, uint32_t seed, char *buf, size_t cap);
const char *fastf_sweep_reps_header(void);
const char *fastf_cap_reps_header(void);
const char *fastf_sweep_genes_reps_header(void);
const char *fastf_cap_genes_reps_header(void);
int fastf_reps_summary_row(float rate_cell, float rate_depth, uint64_t reads_per_cell, uint32_t n_cells, const double *metrics,
                           uint32_t n_reps, char *buf, size_t cap);
int fastf_genes_reps_row(float rate_cell, float rate_depth, uint64_t reads_per_cell, const uint32_t *genes_detected, uint32_t n_reps,
                         const uint64_t *reps_detected, uint32_t n_features, char *buf, size_t cap);
int fastf_gene_reps_add_host(const uint32_t *cells_per_gene, uint32_t n_features, uint64_t *detected, uint64_t *sum, uint64_t *sumsq);

const char *fastf_last_error(void);
const char *fastf_version(void);

/* ===================================================================== */
/* 2a. host-side primitives of the path                                   */
/* ===================================================================== */

/* MT19937 stream — replaces the global-state generator of mt19937ar.c:56-140
 * with an explicit state object; bit-identical output. */
typedef struct fastf_mt { uint32_t s[624]; int idx; } fastf_mt_t;
void     fastf_mt_seed(fastf_mt_t *mt, uint32_t seed);           /* mt19937ar.c:60-73   */
uint32_t fastf_mt_next(fastf_mt_t *mt);                          /* mt19937ar.c:105-140 */
void     fastf_mt_fill(fastf_mt_t *mt, uint32_t *out, size_t n); /* n consecutive draws */
void     fastf_mt_skip(fastf_mt_t *mt, uint64_t n);

/* Integer form of `genrand_real1() >= rate_depth → drop` (bam2db_ds.c:385-390):
 * a record is kept iff draw < fastf_draw_threshold(rate). */
uint64_t fastf_draw_threshold(float rate_depth);   /* 0 .. 2^32 */

/* Cell sub-sampling — bam2db_ds.c:240-244 + utils.c:29-75.
 * n_sampled = (size_t)(n_cells * rate_cell); writes the sorted 0-based line numbers.
 * *draws_used = MT draws consumed (0 when n_sampled == n_cells). Returns non-zero if
 * the reference would exit (n_sampled > n_cells) or the rate is negative/NaN. */
int fastf_sample_cells(size_t n_cells, float rate_cell, unsigned int seed,
                       uint64_t *lines_out, size_t *n_sampled, uint64_t *draws_used);

/* 2-bit UMI codec — bam2db_ds.c:5-51 (+ size rule :419).  Packs up to 16 bases
 * MSB-first into a left-aligned u32.  Returns meta bits (FASTF_META_*). */
uint32_t fastf_pack_umi(const char *ub, size_t len, uint32_t *umi_out);
/* The same for UMIs of up to 32 bases: bases 1..16 into *umi_out, bases 17..32 left-aligned into *ext_out (the reference
 * encodes a UMI of any length, bam2db_ds.c:417-419; an engine created with umi_max_bases 17..32 takes these) */
uint32_t fastf_pack_umi_long(const char *ub, size_t len, uint32_t *umi_out, uint32_t *ext_out);

#define FASTF_META_XF_OK      0x01u   /* xf present and in {25,17}   (bam2db_ds.c:397)  */
#define FASTF_META_HAS_UB     0x02u   /* UB tag present              (bam2db_ds.c:412)  */
#define FASTF_META_UMI_NONNULL 0x04u  /* every base in ACGT          (bam2db_ds.c:36-41)*/
#define FASTF_META_UMI_TOOLONG 0x08u  /* > 16 bases (fastf_pack_umi) / > 32 (_long): not representable, the engine errors */
#define FASTF_META_LEN_SHIFT  4       /* bits 4..7: blob byte length (len+3)/4, 0..8     */
#define FASTF_META_LEN_MASK   0xF0u

/* Exact string → 64-bit key packer.  Two strings get the same key iff they are
 * equal (for every string registered with _add and every string later passed to
 * _pack), which is what the reference's strcmp-verified table guarantees
 * (hashtable.c:98-115).  Key 0 means "cannot match any registered string". */
typedef struct fastf_keydict fastf_keydict_t;
fastf_keydict_t *fastf_keydict_create(void);
void     fastf_keydict_destroy(fastf_keydict_t *d);
uint64_t fastf_keydict_add(fastf_keydict_t *d, const char *s, size_t len);
uint64_t fastf_keydict_pack(const fastf_keydict_t *d, const char *s, size_t len);
/* pack, registering the string when it is new (thread-safe; the tag-histogram paths have no list up front) */
uint64_t fastf_keydict_intern(fastf_keydict_t *d, const char *s, size_t len);
/* key → string; returns the length or -1 (unknown key / buffer too small; cap counts the NUL) */
long     fastf_keydict_decode(const fastf_keydict_t *d, uint64_t key, char *buf, size_t cap);
/* fixed-stride NUL-terminated strings; present may be NULL (all present) */
void     fastf_keydict_pack_many(const fastf_keydict_t *d, const char *strs, size_t stride,
                                 size_t n, const uint8_t *present, uint64_t *out);

/* ===================================================================== */
/* 2b. inner seam: the engine                                             */
/* ===================================================================== */

typedef struct fastf_engine fastf_engine_t;

typedef struct fastf_engine_config {
    const uint64_t *cell_keys;     /* key of cell_index i+1 (sampled barcodes, file order) */
    uint32_t        n_cells;
    const uint64_t *feature_keys;  /* key of feature_index i+1                             */
    uint32_t        n_features;
    uint64_t        draw_threshold;/* fastf_draw_threshold(rate_depth), 0..2^32            */
    uint32_t        umi_max_bases; /* 1..32; widths of the packed sort key follow from it.  A key of more than 64 bits (many
                                      barcodes x many features x long UMIs; always from 17 bases on, which also need
                                      fastf_batch_t.umi_ext) runs on the single-device engine: it sorts the (cell, feature)
                                      word and carries the rest of the key beside it.  From 25 bases on the rest of the key
                                      is itself more than the 52 bits the reduce holds exactly: its top 17 bits (the UMI's
                                      first bases) join the sorted word, the matrix rows of one (cell, feature) are summed
                                      on the host */
    uint32_t        mt_seed;       /* engine-owned draw stream: init_genrand(seed) …       */
    uint64_t        mt_skip;       /* … advanced by the draws SampleInt consumed           */
    uint32_t        n_shards;      /* cell-hash shards (1 = single GPU)                    */
    uint32_t        shard_rank;    /* which shard this engine sorts/reduces                */
    int32_t         device;        /* HIP device ordinal                                   */
    uint64_t        batch_records; /* staging capacity (records per push), 0 = default     */
    uint64_t        key_capacity;  /* initial key-store capacity, 0 = default; grows       */
    /* One host process, several devices (SURVEY 8b inner seam / 8e): n_devices >= 2 makes this ONE engine drive that
     * many GPUs behind the same push / finish / umi_rows calls — chunks of the record stream are dealt to the devices,
     * keys travel to the device that owns their cell in a single exchange (RCCL send/recv group over xGMI; peer
     * copies when devices repeat), every device sorts and reduces its cells, the rows are merged by cell on the
     * host.  n_shards / shard_rank / device are then ignored.  0 or 1: the single-device engine.
     * devices: n_devices HIP ordinals, NULL = 0 .. n_devices-1; ordinals may repeat (all shards on one GPU: the
     * rehearsal the one-GPU tests run). */
    uint32_t        n_devices;
    const int32_t  *devices;
} fastf_engine_config_t;

/* One SoA batch of packed records (host memory; pinned is faster, any works). */
typedef struct fastf_batch {
    const uint64_t *cb_key;   /* 0 = CB absent / cannot match                 */
    const uint64_t *gx_key;   /* 0 = GX absent / cannot match                 */
    const uint32_t *umi;      /* fastf_pack_umi()                             */
    const uint32_t *meta;     /* FASTF_META_*                                 */
    size_t          n;
    const uint32_t *umi_ext;  /* NULL, or bases 17..32 of every UMI (fastf_pack_umi_long) for an engine with umi_max_bases > 16 */
} fastf_batch_t;

typedef struct fastf_coo {
    const uint32_t *feature;  /* 1-based feature_index */
    const uint32_t *cell;     /* 1-based cell_index    */
    const uint32_t *count;    /* COUNT(DISTINCT non-NULL umi) — may be 0 */
    size_t          nnz;      /* rows, ascending (cell, feature) */
} fastf_coo_t;

typedef struct fastf_umi_rows {     /* -u output, ascending (cell, feature, blob) */
    const uint32_t *feature, *cell, *n_copy;
    const uint32_t *umi;            /* left-aligned 2-bit bases; valid iff nonnull[i] */
    const uint8_t  *nonnull;
    size_t          n;
} fastf_umi_rows_t;

/* sweep (section 1): per cell the sum of the counts and the rows with count >= 1 of a COO ascending by (cell, feature) — the host
 * form of fastf_dev_cell_summary — and one row of sweep.tsv (with its newline) from them */
int fastf_sweep_cells_from_coo(const fastf_coo_t *coo, uint32_t n_cells, uint64_t *umis_per_cell, uint32_t *genes_per_cell, uint64_t *umis);
int fastf_sweep_summary_row(float rate_cell, float rate_depth, uint32_t seed, const uint64_t counters[3], uint64_t nnz, uint64_t umis,
                            const uint64_t *umis_per_cell, const uint32_t *genes_per_cell, uint32_t n_cells, char *buf, size_t cap);

/* --genes (section 1): per gene (1-based feature g -> slot g - 1) the rows with count >= 1 and the sum of the counts of a COO in any
 * order — the host form of fastf_dev_gene_summary; a row whose feature is outside 1 .. n_features adds nothing, as there */
int fastf_sweep_genes_from_coo(const fastf_coo_t *coo, uint32_t n_features, uint32_t *cells_per_gene, uint64_t *umis_per_gene);

/* --cells (section 1): reads[], null_reads[], single[] (n_cells entries each) and hist[FASTF_COPY_BINS + 1] of -u rows — the host
 * form of fastf_dev_copy_summary, by the same rules: a row with nonnull[i] == 0 is a NULL row, a row whose cell is outside
 * 1 .. n_cells adds nothing to the per-cell arrays, a row with n_copy == 0 is in no bin */
int fastf_copies_from_umi_rows(const fastf_umi_rows_t *rows, uint32_t n_cells, uint32_t *reads, uint32_t *null_reads, uint32_t *single, uint64_t *hist);

/* --fidelity (section 1): sum_xy[c - 1] and sum_yy[c - 1] (n_cells entries each, cleared first) of a point COO joined with the full
 * COO, both ascending by (cell, feature) — the host form of fastf_dev_fidelity; fails on a point row without a partner among the
 * full rows (nothing is read outside the arrays).  A row whose cell is outside 1 .. n_cells adds nothing */
int fastf_fidelity_from_coo(const fastf_coo_t *full, const fastf_coo_t *point, uint32_t n_cells, uint64_t *sum_xy, uint64_t *sum_yy);

/* --gene-fidelity (section 1): the seven per-gene arrays (n_features u64 entries each, cleared first) of a point COO and the full COO,
 * both ascending by (cell, feature) — the host form of fastf_dev_partner_counts, fastf_dev_gene_moments and fastf_dev_gene_summary
 * together; fails on a point row without a partner.  A row whose feature is outside 1 .. n_features adds nothing */
int fastf_gene_fidelity_from_coo(const fastf_coo_t *full, const fastf_coo_t *point, uint32_t n_features, uint64_t *sum_x, uint64_t *sum_y,
                                 uint64_t *cells_full, uint64_t *cells, uint64_t *sum_xx, uint64_t *sum_yy, uint64_t *sum_xy);

/* --neighbors (section 1): the neighbour sets of a COO matrix restricted to the features with a slot in slot_map
 * (fastf_neighbors_slot_map) — the host form of fastf_dev_neighbor_planes and fastf_dev_neighbors together, in plain C with 128-bit
 * compares.  idx[i * k + s], s < cnt[i]: the neighbours of cell i (0-based, ascending; the other slots 0xFFFFFFFF); norms[i] = n_i
 * (may be NULL).  The rows may come in any order; one whose cell is outside 1 .. n_cells or whose feature is outside 1 .. n_features
 * adds nothing.  Fails as the device does on a norm of 2^42 or more and on k outside 1 .. 64 */
int fastf_neighbors_from_coo(const fastf_coo_t *m, uint32_t n_cells, const uint16_t *slot_map, uint32_t n_features, uint32_t k,
                             uint32_t *idx, uint32_t *cnt, uint64_t *norms);
/* the number of values in both of two ascending lists */
uint32_t fastf_neighbors_shared(const uint32_t *a, uint32_t na, const uint32_t *b, uint32_t nb);
/* --mapping (its section above): M(i), self_dot and self_rank of the point's rows against the full rows, both restricted to the features
 * with a slot in slot_map — the host form of fastf_dev_neighbor_planes on both row sets and fastf_dev_mapping together, in plain C with
 * 128-bit compares; rows in any order; idx (n_cells * k), cnt, self_dot, self_rank (n_cells) as the device call writes them.  Refused: k
 * outside 1 .. 64, and a squared norm of 2^42 or more on either side (FASTF_ERR_NEIGHBOR_NORM) */
int fastf_mapping_from_coo(const fastf_coo_t *full, const fastf_coo_t *point, uint32_t n_cells, const uint16_t *slot_map, uint32_t n_features, uint32_t k,
                           uint32_t *idx, uint32_t *cnt, uint64_t *self_dot, uint32_t *self_rank);

/* co-expression partners (section above) in plain C.  m: a COO matrix, rows in any order, restricted to the features with a slot below K in slot_map
 * (fastf_neighbors_slot_map); a row whose cell is outside 1 .. n_cells or whose feature is outside 1 .. n_features adds nothing.
 * idx[g * k + s], s < cnt[g]: the partners of slot g (slots, ascending; the other slots 0xFFFFFFFF).  D (u64[K * K]) and S (u64[K])
 * may be NULL.  Fails on a count of 2^21 or more, on the range rule and on k outside 1 .. 64 */
int fastf_coexpr_from_coo(const fastf_coo_t *m, uint32_t n_cells, const uint16_t *slot_map, uint32_t n_features, uint32_t K, uint32_t k,
                          uint32_t *idx, uint32_t *cnt, uint64_t *D, uint64_t *S);
/* the selection alone: D, S over n_cells cells -> the partner sets */
int fastf_coexpr_select(const uint64_t *D, const uint64_t *S, uint32_t n_cells, uint32_t K, uint32_t k, uint32_t *idx, uint32_t *cnt);

int  fastf_engine_create(const fastf_engine_config_t *cfg, fastf_engine_t **out);
void fastf_engine_destroy(fastf_engine_t *e);
/* H2D on the engine's copy stream, probe/filter/pack on its compute stream.  The
 * batch may be reused by the caller as soon as the call returns. */
int  fastf_engine_push(fastf_engine_t *e, const fastf_batch_t *batch);
/* Same, with caller-supplied draws (draws[i] belongs to the i-th CB hit of this batch). */
int  fastf_engine_push_draws(fastf_engine_t *e, const fastf_batch_t *batch,
                             const uint32_t *draws, size_t n_draws);
/* Zero-copy variant: the four arrays of the batch are PINNED host memory (fastf_pinned_alloc, or any memory passed
 * through fastf_pinned_register) and go to the device straight from where they are — no staging copy.  The call
 * returns once the copies are queued; the arrays must stay untouched until fastf_engine_wait_input() or
 * fastf_engine_finish() has returned.  This is the path SURVEY 8d calls "device-path": pinned SoA batches ->
 * hipMemcpyAsync on the copy stream -> kernels.  No push waits for the result of an earlier one: the hit-rank base
 * of a chunk (bam2db_ds.c:385 consumes one draw per CB hit) is carried on the device.
 * The arrays may also be DEVICE memory of the engine's device (single-device engines): records packed on the device by
 * the BAM front end (fastf_bam_read_batch_dev) are pushed this way. */
int  fastf_engine_push_pinned(fastf_engine_t *e, const fastf_batch_t *batch);
int  fastf_engine_wait_input(fastf_engine_t *e);   /* every host-to-device copy queued so far has completed */
void *fastf_pinned_alloc(size_t bytes);            /* hipHostMalloc; NULL on failure */
void  fastf_pinned_free(void *p);
/* pin memory the caller allocated (hipHostRegister).  The caller MUST unregister before the memory is freed, unmapped or its pages
 * dropped: the runtime keeps its entry for the addresses otherwise, and the next owner of those addresses inherits it (a later copy
 * into them faults on the GPU).  Prefer memory that is a mapping of its own over malloc heap memory.  The library keeps a ledger of
 * its registrations; FASTF_DEBUG_PINS=1 makes a violation abort and checks the pointers of the *_pinned / lend / gather entries. */
int   fastf_pinned_register(void *p, size_t bytes);
void  fastf_pinned_unregister(void *p);
int   fastf_debug_live_registrations(void);        /* registrations made through this library that are still live (tests) */
/* Sort + segmented unique/reduce over everything pushed; results stay valid until
 * reset/destroy.  counters = {total, sampled, sampled_valid} (bam2db_ds.c:342-344). */
int  fastf_engine_finish(fastf_engine_t *e, fastf_coo_t *coo, uint64_t counters[3]);
/* Optional, before fastf_engine_finish: PINNED host memory of the caller's (fastf_pinned_alloc / fastf_pinned_register)
 * for the matrix rows — three arrays of bytes / 12 entries.  When the matrix fits, finish() writes the rows there from
 * the device (no row buffer of its own to allocate and fault in) and the coo pointers point into it; the caller keeps
 * the memory alive and untouched until it is done with the rows.  NULL withdraws the loan; fastf_engine_reset ends it.
 * bam2db() lends one half of its decoder slab, idle once the last record is on the device. */
int  fastf_engine_lend_rows(fastf_engine_t *e, void *pinned, size_t bytes);
int  fastf_engine_umi_rows(fastf_engine_t *e, fastf_umi_rows_t *rows);
/* records each device of a multi-device engine (n_devices > 1) has been given since the last reset, records[n_devices];
 * a single-device engine reports its total in records[0] */
int  fastf_engine_device_records(const fastf_engine_t *e, uint64_t *records, uint32_t n);
int  fastf_engine_reset(fastf_engine_t *e);
/* key layout chosen at create time */
int  fastf_engine_key_bits(const fastf_engine_t *e, uint32_t *cell_bits, uint32_t *feature_bits,
                           uint32_t *umi_bits, uint32_t *total_bits);

/* ===================================================================== */
/* 2c. inner seam of crb / extract: the tag histogram                     */
/* ===================================================================== */
/* Replaces the per-record insert_tree / insert_CB_node loops (extract.c:88-108, 161-197; filter.c:105-124):
 * host buffers of exact 64-bit tag keys in (0 = tag absent), per distinct value its count and the index of the
 * record it first occurred on out — the three things the shape of the reference's insertion-order tree depends on. */
typedef struct fastf_taghist fastf_taghist_t;
typedef struct fastf_taghist_result {
    uint64_t n_records;              /* records pushed                                                     */
    uint64_t n_valid;                /* records with key1 != 0 (pair mode: and key2 != 0)                   */
    uint64_t n_key1_present;         /* records with key1 != 0                                              */
    /* level 1: distinct key1, ascending key value.  Pair mode: count1/first1 cover valid records only, and an
     * entry whose key1 never met a key2 has count1 == 0 and first1 == UINT64_MAX (it has no first valid record). */
    const uint64_t *key1, *count1, *first1; size_t n1;
    /* pair mode: distinct (key1, key2) of valid records, grouped by key1 in level-1 order */
    const uint32_t *pair_k1;         /* index into key1[]                                                   */
    const uint64_t *pair_key2, *pair_count, *pair_first; size_t n_pairs;
} fastf_taghist_result_t;
int  fastf_taghist_create(int device, fastf_taghist_t **out);
void fastf_taghist_destroy(fastf_taghist_t *h);
/* key2 == NULL: single-tag histogram; otherwise the two-level (key1 → key2) histogram.  One mode per object. */
int  fastf_taghist_push(fastf_taghist_t *h, const uint64_t *key1, const uint64_t *key2, size_t n);
/* single-tag keys already in DEVICE memory (freq packs them on the device): reserve_device returns where n more keys go in the
 * object's own key array (valid until the next reserve / push; keys written into an earlier reservation are kept when the array
 * grows), to be written by work queued on fastf_taghist_stream (a hipStream_t); push_device appends n keys from device memory —
 * from that reservation without a copy — with the summary of the present keys reduced on the device */
uint64_t *fastf_taghist_reserve_device(fastf_taghist_t *h, size_t n);
void *fastf_taghist_stream(fastf_taghist_t *h);
int  fastf_taghist_push_device(fastf_taghist_t *h, const uint64_t *d_key1, size_t n);
/* result arrays are owned by the object and stay valid until the next finish / destroy */
int  fastf_taghist_finish(fastf_taghist_t *h, fastf_taghist_result_t *result);

/* ===================================================================== */
/* 3. device-level entry points (all pointers are device pointers)        */
/* ===================================================================== */

/* number of CB hits in a record range (multi-GPU: draw-rank base of each shard).  Runs K1a and leaves the cell
 * index of every record in the engine's scratch: a fastf_dev_probe_pack over the very same records, next on the same
 * stream, may pass FASTF_PROBE_REUSE_HITS to skip its own K1a.  The caller vouches for "same records": nothing is
 * cached by pointer. */
int fastf_dev_count_hits(fastf_engine_t *e, const uint64_t *d_cb_key, uint64_t n,
                         uint64_t *d_hits_out, void *stream);

/* K1: probe + filter + pack.  d_keys_out holds n_shards buffers of `shard_stride`
 * keys each; d_key_counts[n_shards] (u64) are appended to (not reset);
 * d_counters[4] = {hits, sampled, sampled_valid, error bits} are added to.
 * The i-th CB hit of this range uses d_draws[*d_draw_base + i] (d_draw_base may be NULL = 0):
 * a sharded run keeps the whole draw stream resident and passes its hit-rank base here. */
int fastf_dev_probe_pack(fastf_engine_t *e,
                         const uint64_t *d_cb_key, const uint64_t *d_gx_key,
                         const uint32_t *d_umi, const uint32_t *d_meta, uint64_t n,
                         const uint32_t *d_draws, uint64_t n_draws, const uint64_t *d_draw_base,
                         uint64_t *d_keys_out, uint64_t shard_stride,
                         uint64_t *d_key_counts, uint64_t *d_counters, uint32_t flags, void *stream);
#define FASTF_PROBE_REUSE_HITS 1u  /* fastf_dev_count_hits(e, d_cb_key, n, …) was the previous call on this stream */
/* Streaming form of K1b (single shard, gene list in LDS): every wave filters and packs on its own and writes into
 * private regions of d_keys_out (two per workgroup, filled by turns) — no barrier and no global atomic in the loop.  The
 * key buffer is then SEGMENTED (regions with gaps): d_key_counts[0] is SET to the number of keys, the buffer must hold
 * fastf_dev_probe_capacity() slots, and the next fastf_dev_sort over it must carry FASTF_SORT_SEGMENTED.  The kernel also
 * leaves, per region, the histogram of the first digit of the FASTF_SORT_SKIP_LOW sort: such a sort's first pass walks the
 * regions and counts nothing (scatter_regions_kernel); a sort on another digit grid counts per tile through the region map
 * the engine keeps.  The sorted result is contiguous as always.  One sort per probe_pack: the histograms are used up. */
#define FASTF_PROBE_SEGMENTED 2u
/* key slots a FASTF_PROBE_SEGMENTED call over n records needs in d_keys_out (a little more than n);
 * 0 = this engine cannot run the streaming form (several shards, or a gene list that does not fit LDS) */
int fastf_dev_probe_capacity(const fastf_engine_t *e, uint64_t n, uint64_t *key_slots);

/* BLOCKED record layout — the engine's own device staging.  Per 256-record unit one contiguous run
 *     gx u64[256] | umi u32[256] | meta u32[256] | cell scratch (u16[256], or u32[256] when n_cells > 65535)
 * of 4608 (5120) bytes; the cb keys stay an array of their own.  K1a writes a unit's scratch slice, the streaming K1b reads a
 * unit as ONE stream instead of four distant ones (the same 18 bytes per record move 18 % faster that way:
 * tools/hbm_probe_streams.hip).  fastf_batch_t is untouched: fastf_engine_push / _push_pinned land every chunk of a batch in
 * this layout themselves — three hipMemcpy2DAsync per chunk (a row = one unit's slice of gx / umi / meta, destination pitch =
 * the run) plus three plain copies for a last partial unit, umi_engine.hip push_chunk — and run the same K1a + streaming K1b
 * on it as the device-level calls below; engines whose gene list stays in L2, keys wider than 64 bits and sharded engines
 * stage SoA and run the tile form of K1b.  Device-resident SoA gets here through fastf_dev_block_records.
 * NARROW runs: an engine in stream mode whose listed features all belong to the one LDS gene family, with numbers below
 * 2^32 - 1, and whose UMIs have at most 12 bases uses per unit
 *     gx32 u32[256] | um32 u32[256] | cell scratch (u16[256] or u32[256])
 * of 2560 (3072) bytes: gx32 = the family key's number + 1 (0: key 0, another family, a number of 2^32 - 1 or more),
 * um32 = (umi & ~0xFF) | the FASTF_META_* byte (FASTF_META_UMI_TOOLONG also where the UMI has bits a 12-base key cannot hold).
 * The runs are written by fastf_dev_block_records, and by the push path with a kernel on the copy stream after plain copies
 * (host batches) or straight from device-resident batches.  The layout is fixed at fastf_engine_create; FASTF_BLOCK_WIDE=1
 * keeps the wide runs.
 * fastf_dev_block_bytes: size of the buffer for n records (a multiple of 2560, 3072, 4608 or 5120: the layout in use);
 * 0 = this engine cannot run the streaming K1b (gene list not in LDS, FASTF_NO_STREAM_K1B): use the SoA form. */
int fastf_dev_block_bytes(const fastf_engine_t *e, uint64_t n, uint64_t *bytes);
int fastf_dev_block_records(fastf_engine_t *e, const uint64_t *d_gx_key, const uint32_t *d_umi, const uint32_t *d_meta,
                            uint64_t n, void *d_blocked, void *stream);
/* fastf_dev_probe_pack: d_gx_key points at a blocked buffer of the n records (d_umi, d_meta are ignored).  The cell
 * scratch lives in that buffer, so with FASTF_PROBE_REUSE_HITS the preceding count must have been
 * fastf_dev_count_hits_blocked on the same buffer. */
#define FASTF_PROBE_BLOCKED 8u
int fastf_dev_count_hits_blocked(fastf_engine_t *e, const uint64_t *d_cb_key, uint64_t n, void *d_blocked,
                                 uint64_t *d_hits_out, void *stream);
/* The decision stream.  All K1b wants from the draw of a CB hit is one bit — the read is kept iff
 * genrand_real1() < rate (the reference drops on `>=`, bam2db_ds.c:385-390), i.e. draw < the engine's integer threshold
 * (fastf_draw_threshold) — so that is what it reads:
 * bit (i & 31) of word i >> 5 = draws[i] < threshold.  fastf_dev_probe_pack takes 32-bit draws and converts them on
 * every call (one extra pass over them); a caller that runs the same stream more than once converts it once with
 * fastf_dev_draw_bits (d_bits_out: 8-byte aligned, (n_draws + 63) / 64 * 8 bytes, the tail of the last 64 bits zero) and passes the result
 * as d_draws together with FASTF_PROBE_DRAW_BITS — n_draws and *d_draw_base keep counting draws. */
#define FASTF_PROBE_DRAW_BITS 16u
int fastf_dev_draw_bits(fastf_engine_t *e, const uint32_t *d_draws, uint64_t n_draws, uint32_t *d_bits_out, void *stream);
/* The decision stream from the DEVICE's generator: bit i of d_bits_out = draw i of init_genrand(seed) advanced by `skip` draws is
 * below the engine's threshold (mt19937ar.c:105-140 + bam2db_ds.c:385-390) — same layout and size rule as fastf_dev_draw_bits.
 * Large counts run on many workgroups at once: the stream's state is linear, sub-streams 624 x 256 draws apart are seated by
 * jump-ahead (mt_jump.c) and generated side by side.  Synchronises the stream. */
int fastf_dev_mt_decisions(fastf_engine_t *e, uint32_t seed, uint64_t skip, uint64_t n_draws, uint32_t *d_bits_out, void *stream);

/* The decision PLANES of a sweep over depth rates: the same stream generated ONCE and compared against n_thresholds thresholds
 * (each 0 .. 2^32, fastf_draw_threshold) in the same pass — plane j starts at d_planes_out + j * plane_stride_words and has the
 * layout of fastf_dev_draw_bits: bit i = draw i < thresholds[j], 8-byte aligned (plane_stride_words even, at least
 * (n_draws + 63) / 64 * 2), the tail of the last 64 bits zero.  The engine's own threshold plays no part.  thresholds: host
 * memory.  Synchronises the stream. */
int fastf_dev_mt_decisions_multi(fastf_engine_t *e, uint32_t seed, uint64_t skip, uint64_t n_draws, const uint64_t *thresholds,
                                 uint32_t n_thresholds, uint32_t *d_planes_out, uint64_t plane_stride_words, void *stream);
/* Per-cell summary of matrix rows ascending by (cell, feature) — what fastf_dev_reduce / fastf_dev_rows_gather leave: *d_nnz rows
 * of d_cell (1-based) and d_count.  d_umis_per_cell[c - 1] = sum of the counts of cell c, d_genes_per_cell[c - 1] = its rows with
 * count >= 1, and d_umis_per_cell[n_cells] = the sum of all counts: n_cells + 1 (u64) and n_cells (u32) entries, cleared by the
 * call.  d_cell / d_count may be NULL when there are no rows. */
int fastf_dev_cell_summary(fastf_engine_t *e, const uint32_t *d_cell, const uint32_t *d_count, const uint64_t *d_nnz, uint32_t n_cells,
                           uint64_t *d_umis_per_cell, uint32_t *d_genes_per_cell, void *stream);
/* Per-gene summary of the same rows, in any order: *d_nnz rows of d_feature (1-based, the matrix's row number: what
 * fastf_dev_reduce / fastf_dev_rows_gather leave) and d_count.  d_cells_per_gene[g - 1] = rows of feature g with count >= 1 (u32),
 * d_umis_per_gene[g - 1] = the sum of their counts (u64): n_features entries each, cleared by the call, nothing behind them written.
 * A row whose feature is outside 1 .. n_features adds nothing.  Precondition: the sum of ALL counts is below 2^32 (it is a number of
 * records, and the device-level calls stop at 2^32 - 2 records) — up to 131 072 features both numbers of a gene share one 64-bit
 * counter in LDS (FASTF_GENE_LDS_RANGES=0: global atomics always).  d_feature / d_count may be NULL when there are no rows. */
int fastf_dev_gene_summary(fastf_engine_t *e, const uint32_t *d_feature, const uint32_t *d_count, const uint64_t *d_nnz,
                           uint32_t n_features, uint32_t *d_cells_per_gene, uint64_t *d_umis_per_gene, void *stream);
/* Replicate runs: d_cells_per_gene — what fastf_dev_gene_summary left, n_features entries on the device — added into the three
 * u64[n_features] accumulators of a grid point on `stream`: d_detected[g] += (cells[g] >= 1), d_sum[g] += cells[g], d_sumsq[g] +=
 * cells[g]^2.  Nothing is cleared: the caller zeroes the accumulators before the first seed.  Nothing behind the arrays is written. */
int fastf_dev_gene_reps_add(fastf_engine_t *e, const uint32_t *d_cells_per_gene, uint32_t n_features, uint64_t *d_detected,
                            uint64_t *d_sum, uint64_t *d_sumsq, void *stream);
/* the layout fastf_dev_block_records writes for this engine over n records, as one word (0: no blocked form): engines with the same
 * word write the same bytes for the same records — narrow or wide runs, the width of the cell scratch, and for narrow runs the
 * constants folded into their words — so a blocked copy made for one serves the other, K1a's scratch slices aside */
int fastf_dev_block_layout(const fastf_engine_t *e, uint64_t n, uint64_t *layout);
/* Per-cell reads and the copy-number histogram of -u rows: the output of fastf_dev_umi_rows on this engine — *d_nrows rows of
 * d_ukeys (ascending, so the rows of one cell are neighbours) and d_ncopy.  The cell of a row and whether its blob is NULL are read
 * from the engine's own key layout.  d_reads_per_cell[c - 1] = the sum of n_copy over all rows of cell c (NULL rows included),
 * d_null_reads_per_cell[c - 1] = that sum over its NULL rows, d_single_per_cell[c - 1] = its non-NULL rows with n_copy == 1: n_cells
 * entries each (u32).  d_hist[k - 1], k = 1 .. FASTF_COPY_BINS - 1, = the non-NULL rows with n_copy == k, d_hist[FASTF_COPY_BINS - 1] =
 * those with n_copy >= FASTF_COPY_BINS, d_hist[FASTF_COPY_BINS] = the sum of n_copy over those tail rows: with it the histogram accounts
 * for every read.  All four arrays are cleared by the call, nothing behind them is written.  A row whose cell is outside 1 .. n_cells
 * adds nothing to the per-cell arrays (it is counted in d_hist).  Every per-cell number is below 2^32: it is a number of records,
 * and the device-level calls stop at 2^32 - 2 records.  Refused: NULL arguments, an engine whose keys are wider than 64 bits. */
int fastf_dev_copy_summary(fastf_engine_t *e, const uint64_t *d_ukeys, const uint32_t *d_ncopy, const uint64_t *d_nrows,
                           uint32_t n_cells, uint32_t *d_reads_per_cell, uint32_t *d_null_reads_per_cell, uint32_t *d_single_per_cell,
                           uint64_t *d_hist, void *stream);

/* cap (section 1) on the device.  fastf_dev_cell_hits: d_hits_per_cell[c - 1] (u32, the engine's n_cells entries, cleared by the call)
 * = records whose cell index in K1a's scratch is c.  Valid right after fastf_dev_count_hits (d_blocked NULL: the SoA scratch) or
 * fastf_dev_count_hits_blocked (d_blocked: that call's buffer) over the same n records on the same stream — the
 * FASTF_PROBE_REUSE_HITS contract.
 * fastf_dev_cell_decisions: the decision plane of per-cell thresholds, in the layout and with the size rule of fastf_dev_draw_bits
 * (8-byte aligned, (n_draws + 63) / 64 * 8 bytes, the tail of the last 64 bits zero, nothing behind it written): bit i = draw i of
 * init_genrand(seed) advanced by `skip` draws < d_thresholds[c - 1], c = the cell of the i-th CB hit of the n records; d_thresholds:
 * u64[n_cells] in DEVICE memory, each 0 .. 2^32 — the caller guarantees the range, the call does not read the values.  The engine keeps
 * the raw draws of the last (seed, skip): further calls over the same stream (the other caps of a cell rate) skip the generator.
 * n_draws is the hit count fastf_dev_count_hits reported; hits beyond it get no bit.
 * Valid where fastf_dev_cell_hits is, and a fastf_dev_probe_pack(FASTF_PROBE_REUSE_HITS | FASTF_PROBE_DRAW_BITS [| _BLOCKED |
 * _SEGMENTED]) over the plane may follow.  Synchronises the stream, on every path. */
int fastf_dev_cell_hits(fastf_engine_t *e, uint64_t n, const void *d_blocked, uint32_t *d_hits_per_cell, void *stream);
int fastf_dev_cell_decisions(fastf_engine_t *e, uint64_t n, const void *d_blocked, uint32_t seed, uint64_t skip, uint64_t n_draws,
                             const uint64_t *d_thresholds, uint32_t *d_bits_out, void *stream);

/* level (section 1) on the device: the search for the per-cell thresholds, one step per pass.  State of cell k, all u64[n_cells] in
 * DEVICE memory with values 0 .. 2^32: d_lo, d_hi, and d_probe — the thresholds of the next pass, in the form
 * fastf_dev_cell_decisions takes.
 *   - An uncapped cell (U_k(2^32) <= umi_cap) is settled at lo = hi = 2^32.  A capped cell starts at lo = 0, hi = 2^32.
 *   - The invariant is U_k(lo) <= umi_cap < U_k(hi).  A cell is open while hi - lo > 1.
 *   - d_probe[k] = (lo + hi) / 2 for an open cell and 0 for every other cell: their U is not needed, so their reads drop out of
 *     K1b's output and the pass sorts the open cells' keys alone.
 *   - fastf_dev_level_init: d_umis_full[k] = U_k(2^32); writes the state, the first probes, d_out[0] = the cells open (= capped) and
 *     d_out[1] = cells_capped.
 *   - fastf_dev_level_step: d_umis_per_cell[k] = U_k(d_probe[k]) as fastf_dev_cell_summary left it after a pass on the probes this
 *     state gave; an open cell sets lo = probe if U <= umi_cap, else hi = probe; writes the state, the next probes and d_out[0] = the
 *     cells still open.  hi - lo halves per step from 2^32: no cell is open after 32 steps, and then d_lo holds T[k].
 *   - d_out: FASTF_LEVEL_OUT_WORDS u64 in device memory.  d_out[2] = the error bits the step found: the engine's own error word
 *     OR *d_err_in (a device word, e.g. the error word of the counters fastf_dev_probe_pack filled; NULL: none), read in stream
 *     order.  If any is set the pass's U is not to be trusted: the step writes NO state and no probe, d_out[0] (and [1]) stay 0 and
 *     d_out[3] = 1; else d_out[3] = 0.  So a pass needs one device-to-host copy, of d_out (and whatever lies next to it).
 * Nothing behind the arrays is written.  Stream-ordered; no synchronisation.  Refused: NULL arguments, umi_cap < 1. */
#define FASTF_LEVEL_OUT_WORDS 4u
int fastf_dev_level_init(fastf_engine_t *e, const uint64_t *d_umis_full, uint32_t n_cells, uint64_t umi_cap, uint64_t *d_lo, uint64_t *d_hi,
                         uint64_t *d_probe, uint64_t *d_out, const uint64_t *d_err_in, void *stream);
int fastf_dev_level_step(fastf_engine_t *e, const uint64_t *d_umis_per_cell, uint32_t n_cells, uint64_t umi_cap, uint64_t *d_lo, uint64_t *d_hi,
                         uint64_t *d_probe, uint64_t *d_out, const uint64_t *d_err_in, void *stream);

/* --fidelity (section 1): the join of a point's rows with the full rows of its pair (fidelity_kernel).  Both row sets lie on the
 * device, ascending by (cell, feature): what fastf_dev_rows_gather leaves; *d_nnz_full and *d_nnz (device, u64) rows are read.
 * d_sum_xy[c - 1] = the sum of x * y over the point rows of cell c, d_sum_yy[c - 1] = the sum of y * y (u64, n_cells entries each,
 * cleared by the call).  The same call on (X, X) gives sum_xx.  A point row without a partner raises FASTF_ERR_NO_PARTNER in *d_err
 * (device, u64; NULL: the engine's own error word) and counts with x = 0; nothing outside the arrays is read.  The call synchronises
 * the stream and fails while that bit is set in the word.  A cell index outside 1 .. n_cells writes nothing. */
#define FASTF_ERR_NO_PARTNER 32u
int fastf_dev_fidelity(fastf_engine_t *e, const uint32_t *d_feature_full, const uint32_t *d_cell_full, const uint32_t *d_count_full,
                       const uint64_t *d_nnz_full, const uint32_t *d_feature, const uint32_t *d_cell, const uint32_t *d_count,
                       const uint64_t *d_nnz, uint32_t n_cells, uint64_t *d_sum_xy, uint64_t *d_sum_yy, uint64_t *d_err, void *stream);

/* --gene-fidelity (section 1).  fastf_dev_partner_counts (partner_counts_kernel): the join of fastf_dev_fidelity, kept per row —
 * d_x[i] = the count of the full row with the (cell, feature) of point row i, *d_nnz entries (u32); the row sets, the error word, the
 * synchronisation and the failure on FASTF_ERR_NO_PARTNER are fastf_dev_fidelity's, and a row without a partner gets x = 0.
 * fastf_dev_gene_moments (gene_moments_kernel): rows (d_feature 1-based, d_a, d_b) in any order, *d_nnz of them -> d_sum_ab[g - 1] =
 * the sum of a * b, d_sum_bb[g - 1] = the sum of b * b (u64, n_features entries each, cleared by the call; every sum below 2^64).  A
 * feature outside 1 .. n_features adds nothing, a row with b == 0 issues no atomic.  d_sum_ab == NULL: d_sum_bb alone, at half the
 * atomics.  On (X, x, x) it gives sum_xx, on (Y, x of y, y)
 * sum_xy and sum_yy.  Stream-ordered.  Lists of up to 131 072 features are counted in LDS, range by range; longer ones, and every
 * list under FASTF_GENE_MOMENTS_LDS_RANGES=0, with global atomics. */
int fastf_dev_partner_counts(fastf_engine_t *e, const uint32_t *d_feature_full, const uint32_t *d_cell_full, const uint32_t *d_count_full,
                             const uint64_t *d_nnz_full, const uint32_t *d_feature, const uint32_t *d_cell, const uint64_t *d_nnz,
                             uint32_t *d_x, uint64_t *d_err, void *stream);
int fastf_dev_gene_moments(fastf_engine_t *e, const uint32_t *d_feature, const uint32_t *d_a, const uint32_t *d_b, const uint64_t *d_nnz,
                           uint32_t n_features, uint64_t *d_sum_ab, uint64_t *d_sum_bb, void *stream);

/* --neighbors (section 1), three calls on device pointers.
 * fastf_dev_neighbor_planes (nbr_max_count_kernel, nbr_planes_kernel): rows (d_feature 1-based, d_cell 1-based, d_count), *d_nnz of
 * them, each (cell, feature) at most once, and d_slot_map (u16[n_features + 1], fastf_neighbors_slot_map) -> *planes_out = P, the planes
 * the largest count among the rows with a slot needs (1 below 2^7, 2 below 2^14, 3 below 2^21; beyond that the call fails, naming
 * FASTF_ERR_NEIGHBOR_COUNT), and — d_planes != NULL — P byte planes of n_pad x K_pad (fastf_neighbors_pad), zeroed first: plane p holds
 * bits 7p .. 7p+6 of the count of (cell, slot).  planes_bytes: the room behind d_planes.  Synchronises the stream once (the maximum).
 * fastf_dev_neighbors (nbr_norms_kernel, nbr_gram_kernel): the planes -> d_norms[i] = n_i (u64), *max_norm_out their maximum (read
 * back; 2^42 and beyond fails before anything else is launched), d_idx[i * k + s], s < d_cnt[i]: the neighbours of cell i (0-based,
 * ascending; the other slots 0xFFFFFFFF), k from 1 to 64.  A workgroup owns 128 query rows, a wave 32 of them, and streams the column
 * tiles; n x n is never stored.  The dot products come from the i8 MFMA (32x32x32), under FASTF_NEIGHBORS_MFMA=0 from ordinary integer
 * instructions: the same numbers either way.
 * fastf_dev_neighbors_shared (nbr_shared_kernel): two index / count sets of the same k -> d_shared[i] = the cells in both sets of i. */
int fastf_dev_neighbor_planes(fastf_engine_t *e, const uint32_t *d_feature, const uint32_t *d_cell, const uint32_t *d_count, const uint64_t *d_nnz,
                              const uint16_t *d_slot_map, uint32_t n_features, uint32_t n_cells, uint32_t K, void *d_planes, size_t planes_bytes,
                              uint32_t *planes_out, void *stream);
int fastf_dev_neighbors(fastf_engine_t *e, const void *d_planes, uint32_t planes, uint32_t n_cells, uint32_t K, uint32_t k, uint32_t *d_idx,
                        uint32_t *d_cnt, uint64_t *d_norms, uint64_t *max_norm_out, void *stream);
int fastf_dev_neighbors_shared(fastf_engine_t *e, const uint32_t *d_idx_a, const uint32_t *d_cnt_a, const uint32_t *d_idx_b, const uint32_t *d_cnt_b,
                               uint32_t n_cells, uint32_t k, uint32_t *d_shared, void *stream);

/* --mapping (its section above), one call on device pointers (map_diag_kernel, map_gram_kernel; mapping_kernels.hpp).  d_planes_point
 * (planes_point planes) and d_planes_full (planes_full planes; planes_point <= planes_full, what a subsample gives — another pair is
 * refused) are what fastf_dev_neighbor_planes filled for (n_cells, K) from the point's and from the full rows; d_norms_full (u64[n_cells])
 * is what fastf_dev_neighbors left for the full rows.  The largest point norm (*max_norm_point_out, may be NULL) and the largest full norm
 * are reduced and read back first; either at 2^42 or beyond fails the call (FASTF_ERR_NEIGHBOR_NORM) before anything else is launched.
 * Then d_self_dot (u64[n_cells]), d_idx (u32[n_cells * k]) and d_cnt (u32[n_cells]) in the layout of fastf_dev_neighbors, and d_self_rank
 * (u32[n_cells], FASTF_MAPPING_NO_RANK where self_dot is 0); k from 1 to 64.  The dot products come from the i8 MFMA (32x32x32), under
 * FASTF_MAPPING_MFMA=0 from ordinary integer instructions: the same numbers.  hood is fastf_dev_neighbors_shared on (d_idx, d_cnt) and the
 * full sets, the vote fastf_dev_label_votes on (d_idx, d_cnt).  Synchronises the stream once.  Not re-entrant per engine: the two maxima
 * share one engine buffer. */
int fastf_dev_mapping(fastf_engine_t *e, const void *d_planes_point, uint32_t planes_point, const void *d_planes_full, uint32_t planes_full, uint32_t n_cells,
                      uint32_t K, uint32_t k, const uint64_t *d_norms_full, uint32_t *d_idx, uint32_t *d_cnt, uint64_t *d_self_dot, uint32_t *d_self_rank,
                      uint64_t *max_norm_point_out, void *stream);

/* --coexpression (section above), on device pointers (coexpr_kernels.hpp).
 * fastf_coexpr_pad: the shape of the GENE-MAJOR byte planes of (n_cells, K): K_pad rows (K rounded up to 32) of n_pad bytes — n_cells rounded
 * up to 32, then to a multiple of *chunk, the cells a wave reduces at a time: FASTF_COEXPR_CHUNK cells (the environment variable of that
 * name lowers it: a value from 32 to below the default is rounded down to a multiple of 32, any other value is ignored and the default
 * holds; read at each call, it changes no result) or the rounded cells where they are fewer.
 * Plane p holds bits 7p .. 7p+6 of the count of (slot, cell) at [(p * K_pad + slot) * n_pad + cell].  fastf_coexpr_work_bytes: the bytes of
 * `planes` such planes.
 * fastf_dev_coexpr_sums (coex_planes_kernel, coex_gram_kernel, coex_sums_kernel): rows and d_slot_map as fastf_dev_neighbor_planes takes them,
 * `planes` what that call returned for them (its FASTF_ERR_NEIGHBOR_COUNT is this option's too) -> the planes in d_work (work_bytes of
 * room, 16-byte aligned; too little fails by name), d_D[g * K + h] = D_gh (u64, dense, both halves) and d_S[g] = S_g; D and S are zeroed
 * by the call.  fastf_coexpr_check_gram refuses (n_cells, planes) before anything is launched.  A wave owns one 32 x 32 tile of D for one
 * chunk of cells, one i32 accumulator tile per digit sum (3 * chunk * 127^2 < 2^31), and adds sum_t 2^(7t) acc_t into D with 64-bit
 * integer atomics.  The dot products come from the i8 MFMA (32x32x32), under FASTF_COEXPR_MFMA=0 from ordinary integer instructions: the
 * same numbers either way.  Asynchronous on `stream`.
 * fastf_dev_coexpr_select (coex_var_kernel, coex_select_kernel): D, S over n_cells cells -> d_idx[g * k + s], s < d_cnt[g]: the partners
 * of gene g (slots, ascending; the other slots 0xFFFFFFFF), k from 1 to 64, K at most 4096.  The largest D_gg is read back and
 * fastf_coexpr_check_range refuses the call (FASTF_ERR_COEXPR_RANGE) before the selection is launched.  One thread per gene walks the
 * slots in ascending order and keeps its best k by the rule of fastf_coexpr_select: the same sets.  Synchronises the stream once.  V and the
 * word of the maximum live in ONE buffer of the engine: the call is not re-entrant per engine — two selections on one engine run one
 * after the other, whatever their streams (the buffer is freed by fastf_engine_destroy).
 * The shared counts of two sets: fastf_dev_neighbors_shared with n_cells := K (the layout of the sets is the same). */
void fastf_coexpr_pad(uint32_t n_cells, uint32_t K, uint32_t *K_pad, uint32_t *n_pad, uint32_t *chunk);
size_t fastf_coexpr_work_bytes(uint32_t n_cells, uint32_t K, uint32_t planes);
int fastf_dev_coexpr_sums(fastf_engine_t *e, const uint32_t *d_feature, const uint32_t *d_cell, const uint32_t *d_count, const uint64_t *d_nnz,
                          const uint16_t *d_slot_map, uint32_t n_features, uint32_t n_cells, uint32_t K, uint32_t planes, void *d_work,
                          size_t work_bytes, uint64_t *d_D, uint64_t *d_S, void *stream);
int fastf_dev_coexpr_select(fastf_engine_t *e, const uint64_t *d_D, const uint64_t *d_S, uint32_t n_cells, uint32_t K, uint32_t k,
                            uint32_t *d_idx, uint32_t *d_cnt, void *stream);

/* --labels (section above), one call on device pointers (label_votes_kernel).  d_idx and d_cnt are what fastf_dev_neighbors writes: k
 * slots a cell, d_cnt[i] of them valid; the other slots hold 0xFFFFFFFF and are never used as an index.  k from 1 to 64, n_labels up to
 * FASTF_LABELS_MAX.  d_lab: u8[n_cells].  d_pred, d_same, d_labelled: u8[n_cells]; d_conf: n_labels x (n_labels + 1) u32, zeroed by the
 * call.  A cell owns a lane group of 16, 32 or 64 lanes, the smallest that holds k; the confusion counts of a workgroup are added up
 * in LDS where n_labels * (n_labels + 1) * 4 bytes fit it (201 labels and fewer) and flushed with one global atomic per non-zero
 * entry, else every labelled cell adds with a global atomic; FASTF_LABELS_LDS=0 takes that general form always.  Asynchronous on
 * `stream` */
int fastf_dev_label_votes(fastf_engine_t *e, const uint32_t *d_idx, const uint32_t *d_cnt, const uint8_t *d_lab, uint32_t n_cells, uint32_t k,
                          uint32_t n_labels, uint8_t *d_pred, uint8_t *d_same, uint8_t *d_labelled, uint32_t *d_conf, void *stream);

/* --pseudotime (section above), on device pointers (ptime_kernels.hpp).
 * fastf_dev_ptime_medians (pt_median_kernel): d_idx and d_cnt as fastf_dev_neighbors or fastf_dev_mapping writes them, k from 1 to 64;
 * d_t: u32[n_cells]; d_est, d_valued: u32[n_cells].  A cell owns a lane group of 16, 32 or 64 lanes, the smallest that holds k; every
 * valid lane finds its position under the order (value, slot) by shuffles inside the group, and the lane at ceil(c / 2) - 1 writes.
 * fastf_dev_ptime_census (pt_pairs_kernel): d_est, d_t -> d_out, FASTF_PTIME_OUT_WORDS u64, zeroed by the call.  One workgroup per pair
 * of tiles (a <= b) of FASTF_PTIME_TILE cells, n_cells^2 / 2 comparisons, nothing of size n x n is stored; n_cells beyond
 * FASTF_PTIME_MAX_CELLS is refused.  Both asynchronous on `stream` */
int fastf_dev_ptime_medians(fastf_engine_t *e, const uint32_t *d_idx, const uint32_t *d_cnt, const uint32_t *d_t, uint32_t n_cells, uint32_t k,
                            uint32_t *d_est, uint32_t *d_valued, void *stream);
int fastf_dev_ptime_census(fastf_engine_t *e, const uint32_t *d_est, const uint32_t *d_t, uint32_t n_cells, uint64_t *d_out, void *stream);

/* --markers (section above), one call on device pointers (marker_labels_kernel, marker_auc_kernel).  d_planes: what
 * fastf_dev_neighbor_planes filled for (n_cells, K) with `planes` planes; d_lab: u8[n_cells].  d_s2u, d_sum: u64[n_labels * K]; d_det:
 * u32[n_labels * K]; d_n_per_label: u32[n_labels]; the call clears all four.  A workgroup owns a tile of adjacent slots (32 at one plane,
 * 2 at two) and walks the rows twice: E per slot in LDS, a scan in place to 2C + E, then each non-zero entry's term, detection and count;
 * the zero counts enter in closed form.  The accumulators of a tile sit in LDS where they fit beside the bins
 * (fastf_marker_auc_form), else, and always under FASTF_MARKERS_LDS=0, they go by global atomics: the same numbers.  planes == 3
 * (FASTF_ERR_MARKER_COUNT) and n_labels outside 1 .. FASTF_LABELS_MAX are refused before anything is launched.  Asynchronous on `stream` */
int fastf_dev_marker_auc(fastf_engine_t *e, const void *d_planes, uint32_t planes, uint32_t n_cells, uint32_t K, const uint8_t *d_lab,
                         uint32_t n_labels, uint64_t *d_s2u, uint32_t *d_det, uint64_t *d_sum, uint32_t *d_n_per_label, void *stream);

/* Keys wider than 64 bits on a SHARDED engine (n_shards > 1; one process per GPU: fastf_amd/dist.py).  The calls above take
 * 64-bit keys; an engine whose keys are wider (fastf_engine_is_wide: many barcodes x many features x long UMIs, or
 * umi_max_bases > 16) runs the same E1-E12 chain (bam2db_ds.c:360-438) with the key in two words:
 *   fastf_dev_probe_pack_wide   as fastf_dev_probe_pack (tile form; flags FASTF_PROBE_REUSE_HITS / _DRAW_BITS), the group word of
 *                               every surviving record into d_keys_out[shard][..], the rest of its key into d_vals_out[shard][..]
 *                               (same slot), d_umi_ext = bases 17.. of the UMIs or NULL;
 *   [the caller exchanges both arrays: keys and values of shard s to rank s]
 *   fastf_dev_adopt_wide        the n pairs this shard owns into the engine's own key store (synchronises the stream);
 *                               fastf_engine_finish / fastf_engine_umi_rows then give this shard's rows (hashtable.c:70-115 and
 *                               bam2db_ds.c:417-419 take any list size and UMI length; the GROUP BY of :480-483 never joins cells). */
int fastf_engine_is_wide(const fastf_engine_t *e);
int fastf_dev_probe_pack_wide(fastf_engine_t *e, const uint64_t *d_cb_key, const uint64_t *d_gx_key, const uint32_t *d_umi,
                              const uint32_t *d_meta, const uint32_t *d_umi_ext, uint64_t n,
                              const uint32_t *d_draws, uint64_t n_draws, const uint64_t *d_draw_base,
                              uint64_t *d_keys_out, uint64_t *d_vals_out, uint64_t shard_stride, uint64_t *d_key_counts,
                              uint64_t *d_counters, uint32_t flags, void *stream);
int fastf_dev_adopt_wide(fastf_engine_t *e, const uint64_t *d_keys, const uint64_t *d_vals, uint64_t n, void *stream);

/* K2: LSD radix sort of the low `key_bits` bits of n keys (n read from *d_n on the
 * device, at most max_n).  d_keys and d_tmp are ping-pong buffers of max_n keys;
 * *sorted_in_tmp tells where the result landed. */
#define FASTF_SORT_SKIP_LOW   2u   /* leave the low fastf_engine_skip_bits() bits unsorted: enough for the matrix
                                      (equal keys stay neighbours of their (cell, feature, top-UMI-bits) run);
                                      pass the same flag to fastf_dev_reduce.  Not for fastf_dev_umi_rows.        */
#define FASTF_SORT_SEGMENTED  4u   /* d_keys is the output of the last FASTF_PROBE_SEGMENTED fastf_dev_probe_pack */
/* The keys of the next FASTF_SORT_SEGMENTED fastf_dev_sort lie in n_regions rows of `stride` slots of its d_keys, row r
 * holding d_counts[r] keys at its front (device array, u64): the receive buffer of a fixed-capacity key exchange is sorted
 * where it landed, no compaction pass.  Writes the total to *d_n_out on the device. */
int fastf_dev_set_regions(fastf_engine_t *e, const uint64_t *d_counts, uint32_t n_regions, uint64_t stride,
                          uint64_t *d_n_out, void *stream);
int fastf_engine_skip_bits(const fastf_engine_t *e, uint32_t *bits);
/* number of 8-bit LSD passes fastf_dev_sort runs for this engine's keys with the given flags: the digit grid starts at
 * the skip bit (not necessarily a byte boundary) when FASTF_SORT_SKIP_LOW is set, at bit 0 otherwise */
int fastf_engine_sort_passes(const fastf_engine_t *e, uint32_t flags, uint32_t *passes);
/* The grids of the step as this engine launches them for n_records records and n_keys keys: out[2 f] = workgroups and
 * out[2 f + 1] = the turns' worth of work they share ("tiles": a workgroup goes round ceil(tiles / workgroups) times), for
 * the kernel families f below.  K1A, K1B_TILES, K1B_STREAM and SCATTER_REGIONS are the forms this engine's tables select (0, 0
 * for the streaming form where the engine has none); every other family is reported as the engine WOULD launch it, whether or
 * not its paths reach that kernel (PAIRS: wide keys only; K3_HASHED: engines that leave low bits unsorted, and wide keys).  A
 * count of 0 reports 0, 0.  The widths come from
 * FASTF_GRID_CUS (the CU count every capped grid is cut from, 1 .. the device's), FASTF_TILE_GRID_CAP and FASTF_K3_PER_CU
 * as they stood when the engine was created: test and diagnostic switches.
 *   K1A             probe_cells_lds_kernel (tiles: pairs of K1 tiles), probe_cells_filtered_kernel or probe_cells_kernel
 *   BLOCK_RECORDS   block_records_kernel (tiles: four 256-record units)
 *   DRAW_BITS       draw_bits_kernel over n_records draws (tiles: sixteen 64-draw words)
 *   K1B_TILES       filter_pack_kernel (K1 tiles)
 *   K1B_STREAM      filter_pack_stream_kernel (tiles: one 256-record unit per wave)
 *   SCATTER_REGIONS scatter_regions_kernel over the regions K1B_STREAM leaves (tiles: regions)
 *   SORT_TILES      tile_count_kernel and scatter_kernel (sort tiles)
 *   RGN_HIST        rgn_hist_kernel over adopted keys (tiles: regions of 65 536 keys)
 *   K3_WINDOWS      reduce_windows_kernel<false / true> (tiles: 2048-key windows; a workgroup owns one chunk of them)
 *   K3_HASHED       reduce_hashed_kernel, the form this engine's keys take (the same)
 *   GIANT           giant_groups_kernel (tiles 0: its work items are as the keys have them)
 *   PAIRS           pair_heads_kernel, pair_rows_kernel, pair_copies_kernel (2048-key tiles)
 *   ROWS_GATHER     rows_gather_kernel after the matrix rows' K3 (tiles: chunks) */
enum { FASTF_GRID_K1A = 0, FASTF_GRID_BLOCK_RECORDS, FASTF_GRID_DRAW_BITS, FASTF_GRID_K1B_TILES, FASTF_GRID_K1B_STREAM,
       FASTF_GRID_SCATTER_REGIONS, FASTF_GRID_SORT_TILES, FASTF_GRID_RGN_HIST, FASTF_GRID_K3_WINDOWS, FASTF_GRID_K3_HASHED,
       FASTF_GRID_GIANT, FASTF_GRID_PAIRS, FASTF_GRID_ROWS_GATHER, FASTF_GRID_FAMILIES };
int fastf_engine_grids(const fastf_engine_t *e, uint64_t n_records, uint64_t n_keys, uint32_t *out /* [2 * FASTF_GRID_FAMILIES] */);
/* The engine's tile scan on the caller's device arrays (16-byte aligned): d_out[i] = d_in[0] + .. + d_in[i - 1] in 64 bits,
 * d_in[0 .. T) is left all zero, *d_total = the sum, *d_base = *d_running and then *d_running += the sum.  d_total,
 * d_running and d_base may each be null.  Entries are at most 4096 (the hits of a K1 tile): the sums inside a round of
 * 16 384 entries are 32-bit.  slot 0 or 1: scans of more than 16 384 entries keep chunk totals per slot, so that two scans
 * may run side by side on two streams. */
int fastf_dev_scan_tiles(fastf_engine_t *e, uint32_t *d_in, uint32_t T, uint64_t *d_out, uint64_t *d_total,
                         uint64_t *d_running, uint64_t *d_base, uint32_t slot, void *stream);
/* which lookup structure the lists qualified for: 1 = LDS-resident (barcodes: perfect hash of 32-bit codes; genes:
 * bitmap + rank + permutation over one id family; genes: 2 = direct index table over a dense id range),
 * 0 = open-addressed table in L2 */
int fastf_engine_table_modes(const fastf_engine_t *e, int *cells_in_lds, int *genes_in_lds);
/* width of one entry of the cell-index scratch K1a leaves for K1b: 2 bytes when every cell index fits 16 bits, else 4 */
int fastf_engine_cell_scratch_bytes(const fastf_engine_t *e, uint32_t *bytes);
int fastf_dev_sort(fastf_engine_t *e, uint64_t *d_keys, uint64_t *d_tmp,
                   const uint64_t *d_n, uint64_t max_n, uint32_t key_bits, uint32_t flags,
                   int *sorted_in_tmp, void *stream);

/* K3: segmented unique/reduce of sorted keys → COO (SoA, capacity max_n rows);
 * *d_nnz (u64) receives the row count. */
#define FASTF_REDUCE_SEGMENTED 8u   /* leave the rows in the engine's row regions (one per workgroup chunk, each in
                                       order, the regions in order) and only report *d_nnz: d_feature/d_cell/d_count are
                                       not touched; fastf_dev_rows_gather concatenates the regions later */
int fastf_dev_reduce(fastf_engine_t *e, const uint64_t *d_sorted, const uint64_t *d_n,
                     uint64_t max_n, uint32_t *d_feature, uint32_t *d_cell,
                     uint32_t *d_count, uint64_t *d_nnz, uint32_t flags, void *stream);
/* Concatenates the row regions of the last fastf_dev_reduce on this engine (same d_n) into feature/cell/count: device
 * arrays, or PINNED HOST memory (hipHostMalloc / fastf_pinned_alloc) — then this kernel is the device-to-host copy of
 * the matrix rows.  A fastf_dev_reduce without FASTF_REDUCE_SEGMENTED runs it itself. */
int fastf_dev_rows_gather(fastf_engine_t *e, const uint64_t *d_n, uint32_t *feature, uint32_t *cell,
                          uint32_t *count, void *stream);

/* K3u: run-length rows for -u (capacity max_n rows). */
int fastf_dev_umi_rows(fastf_engine_t *e, const uint64_t *d_sorted, const uint64_t *d_n,
                       uint64_t max_n, uint64_t *d_ukeys, uint32_t *d_ncopy,
                       uint64_t *d_nrows, void *stream);

/* bytes of device workspace the engine holds for sorts of up to max_n keys
 * (grown on demand by the calls above; call once up front to avoid growth in a
 * timed region) */
int fastf_dev_reserve(fastf_engine_t *e, uint64_t max_records, uint64_t max_keys);

/* Error bits raised by device kernels since the last clear (synchronises).  Bit 16 (FASTF_ERR_RUN_TOO_LONG) after
 * a FASTF_SORT_SKIP_LOW reduce means the result of that reduce is not valid: sort fully and reduce again
 * (fastf_engine_finish does this by itself). */
#define FASTF_ERR_RUN_TOO_LONG 16u
int fastf_dev_error_bits(fastf_engine_t *e, uint64_t *bits);
/* stream-ordered (an atomicAnd on the device; no synchronisation) */
int fastf_dev_clear_error_bits(fastf_engine_t *e, uint64_t mask, void *stream);

/* name of the dominant kernel symbols, for profile post-processing */
const char *fastf_kernel_names(void);

#ifdef __cplusplus
}
#endif
#endif /* FASTF_AMD_H */
