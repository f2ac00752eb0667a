/* resident.h — the resident pipeline `fastF sweep`, `fastF cap` and `fastF level` share (resident.c): the packed records of a BAM stay
 * in device memory after ONE decode; per cell rate one engine, the records in its layout and K1a once; per point K1b on that point's
 * decision plane, sort, reduce, the per-cell summary and — when the matrices are wanted — the rows gathered into pinned memory
 * for the writers of bam2db.  What differs between the verbs is how a point's decision plane is made: each verb describes itself in
 * ONE res_verb_t (its name, index, summary header, wording and the hooks that make the planes), and ONE driver (grid_run.c:
 * fastf_res_grid_run) runs the checks, the tables, the (cell rate, seed) pairs and the body of every point for all three.  The way
 * into it is ONE too: every exported entry point forwards to fastf_res_grid_entry, and the three commands are fastf_res_cmd.
 * The files: resident.c has the device side, the lists, the replicate accumulators and the command; res_tables.c every table and
 * point file of a run — the comparisons against full depth below are ONE descriptor each there (res_cmp_t); grid_rows.c the host
 * analysis, the rows and the headers of the per-verb tables, defined once (fastf_res_table_header).  The last two touch no device.
 * --cells adds a stage of its own behind a point (fastf_res_point_cells): the point's keys sorted fully, K3u's rows, their per-cell
 * and copy-number summary.  It runs AFTER the point's matrix rows have left the device — K3u writes the engine's row regions
 * (their count array and the span tables are the ones the matrix rows lie in) and fastf_res_point_write gathers from those.
 * --fidelity adds the full-depth rows of the pair, kept on the device behind every open (fastf_res_full_run / fastf_res_full_keep), and
 * behind every point the join of its rows with them (fastf_res_point_fidelity) — BEFORE fastf_res_point_cells, whose K3u output
 * overwrites the point's rows in S->buf.rows.
 * --gene-fidelity reduces the same pair of row sets along the gene axis (fastf_res_point_gene_fidelity, behind fastf_res_point_fidelity
 * and before fastf_res_point_cells too); alone it switches the full-depth rows on by itself.
 * --neighbors compares the k-nearest-neighbour sets of the cells over the pair's highly variable genes (fastf_res_point_neighbors, behind
 * the two above and before fastf_res_point_cells); alone it switches on the full-depth rows and the pair's per-gene sums that rank the genes.
 * --labels turns those neighbour sets into label votes (fastf_res_point_labels, directly behind fastf_res_point_neighbors); alone it
 * switches on everything --neighbors needs on the device and writes none of its files.
 * --markers N (with --labels) ranks the genes of A per label by the exact AUC of the label against the other labelled cells, from the
 * byte planes the neighbour sets were made of (fastf_res_point_markers, directly behind fastf_res_point_labels).
 * --mapping looks every cell of the point up among ALL full-depth cells of the pair (fastf_res_point_mapping, directly behind
 * fastf_res_point_labels, while the point's byte planes are in the plane buffer); alone it switches on what --labels alone switches on, and
 * keeps a copy of the full rows' planes for the life of the pair.
 * --pseudotime FILE estimates every cell's rank along the user's value back from its neighbour sets and counts the order of all pairs
 * (fastf_res_point_ptime, directly behind fastf_res_point_labels; the mapping list's side inside fastf_res_point_mapping); alone it switches
 * on what --labels alone switches on.
 * --coexpression compares the co-expression partners of the genes of A, at full depth and at the point (fastf_res_point_coexpr, behind
 * fastf_res_point_markers and before fastf_res_point_cells); alone it switches on the full-depth rows, the pair's per-gene sums and the
 * slot map, and nothing of the neighbour sets. */
#ifndef FASTF_RESIDENT_H
#define FASTF_RESIDENT_H

#include "host_io.h"
#include "res_layout.h"

#include <stdio.h>

#define FASTF_HIDDEN __attribute__((visibility("hidden")))

/* device memory for the C side of the library (umi_engine.hip) */
void *fastf_devmem_alloc(int device, size_t bytes);
void  fastf_devmem_free(void *p);
int   fastf_devmem_copy(void *dst, const void *src, size_t bytes);
int   fastf_devmem_zero(void *dst, size_t bytes);
int   fastf_devmem_sync(void);

enum { RES_OK = 0, RES_FAIL = 1, RES_NOT_COVERED = 2 };   /* NOT_COVERED: keys wider than 64 bits or UMIs beyond what a 64-bit key holds */
/* layout of the small device block of one point (u64 words; atomics and plain loads on different 256-byte segments) */
enum { SM_KEYS = 0, SM_CNT = 32, SM_NNZ = 64, SM_BASE = 96, SM_HITS = 128, SM_UROWS = 160, SM_LEVEL = 192, SM_FULL = 224, SM_WORDS_ = 256 };   /* SM_UROWS: --cells, K3u's row count; SM_LEVEL: level, the result block of a step (FASTF_LEVEL_OUT_WORDS); SM_FULL: --fidelity, the row count of the pair's full rows (no point clears it) */

typedef struct { double lists, decode, engine, block_k1a, planes, device, d2h, summary, write, genes, cells_dev, cells, reps, search, fidelity, gene_fid, neighbors, labels, markers, coexpr, mapping, ptime; uint32_t opens, relays, passes; } res_times_t;   /* ptime: --pseudotime alone — the ranks of every pair, the median and census calls, their D2H, rows and files (the neighbour sets it switches on are booked under neighbors); mapping: --mapping alone — the copy of the full planes, the mapping calls, the shared counts and votes, their D2H, rows and files (the neighbour sets it switches on are booked under neighbors); coexpr: --coexpression alone — the planes, the Gram products and selections, the shared counts, their D2H, rows and files, and the full point and per-gene sums of every pair when none of the three flags below is set; markers: --markers alone — the kernel calls on the planes, their D2H, the ranks, rows and files; labels: --labels alone — the label arrays of every pair, the vote calls, their D2H, rows and files (the neighbour sets it switches on are booked under neighbors); neighbors: --neighbors alone — the planes, the Gram products and selections, the shared counts, their D2H, rows and files, and the full point and per-gene sums of every pair when neither flag above is set; gene_fid: --gene-fidelity alone — what fidelity books, and the full point of every pair when --fidelity is not set; fidelity: --fidelity alone — the full point of every pair, the joins, their D2H, rows and files; search, passes: level alone — the seconds and the number of its search passes; genes: --genes alone (D2H, rows, files); cells_dev, cells: --cells alone (full sort + K3u + summary + D2H; rows and files); reps: the replicate tables and the per-gene accumulators; opens, relays: fastf_res_rate_open calls, and those that laid the blocked copy out */

/* the error message of the grid files, set as printf formats it; returns 1 (grid_rows.c) */
int    fastf_res_err(const char *fmt, ...) __attribute__((format(printf, 1, 2))) FASTF_HIDDEN;
double fastf_res_now(void) FASTF_HIDDEN;
int    fastf_res_make_dir(const char *path) FASTF_HIDDEN;

/* the lists of every (cell rate, seed) pair, and ONE dictionary for the records: the first pair's, with the barcodes of the others
 * registered in it — a key then means the same string whichever pair's table it is looked up in.  keys[i][k]: key of cell k + 1 of
 * pair i.  L[i].mt_skip: the draws that pair's own SampleInt consumed of init_genrand(seeds[i]) */
typedef struct { uint32_t n; fastf_lists_t *L; uint64_t **keys; } res_lists_t;
int  fastf_res_lists_load(const char *barcodes, const char *features, const float *rates_cell, const uint32_t *seeds, uint32_t n_pairs, res_lists_t *out) FASTF_HIDDEN;
void fastf_res_lists_free(res_lists_t *l) FASTF_HIDDEN;

/* the packed records (24 bytes each) in device memory */
typedef struct {
    int device; const char *verb;
    uint64_t n, cap;                     /* records held, room */
    uint64_t *cb, *gx; uint32_t *umi, *meta;   /* device arrays of cap entries */
} resident_t;
int  fastf_res_decode(const char *verb, const char *bam_file, const fastf_lists_t *L0, int device, resident_t *R) FASTF_HIDDEN;
void fastf_res_free(resident_t *R) FASTF_HIDDEN;

/* one (cell rate, seed) pair: the engine, the records in its layout, K1a (the cell scratch and the hit count H serve every point),
 * the buffers of a point.  DESIGN.md section 10q describes this state once; in short:
 * cfg   what the caller sets before the first open and no open or close touches: the comparisons that are on (fastf_res_cmp_cfg, from
 *       the mask of the run's res_cmp_t: neighbors is set with labels, with mapping and with ptime too; markers = N needs labels), max_cells, the most cells any pair of the run samples (0: unknown), which the lists tell,
 *       and no_reuse (the verbs read FASTF_RES_NO_REUSE=1 once per run): fresh buffers and a fresh blocked copy for every pair.
 * buf   the buffer table: every device, pinned or host buffer of the state.  The buffers outlive the pair: a run keeps ONE res_rate_t,
 *       zeroed before its first open, and every later fastf_res_rate_open on it ends the pair before (its engine) and takes its buffers
 *       over — each is allocated again only where the new pair needs more (have: the bytes held; n: the entries per array a carved
 *       block was allocated for, by which it is carved while it lives).  fastf_res_rate_close frees the table in a loop.
 * the views (res_layout.h)   the typed arrays inside the carved blocks, set by the open that made room for them.
 * blk_layout: the layout word (fastf_dev_block_layout) the blocked copy in buf.blk was written for, 0: none — a pair whose engine has
 * the same word runs K1a alone */
typedef struct { union { void *p; uint8_t *u8; uint32_t *u32; uint64_t *u64; }; size_t have, n; int kind; } res_buf_t;
enum { RES_DEV = 1, RES_PIN, RES_HOST };             /* the kinds of a buffer: device, pinned, plain host memory */
typedef struct { int fidelity, gene_fid, neighbors, labels, coexpr, mapping, ptime; const fastf_labels_t *lab_t; const fastf_ptime_t *pt_t; uint32_t markers, max_cells; int no_reuse; } res_cfg_t;
typedef struct {
    res_cfg_t cfg;
    const char *verb; const resident_t *R; const fastf_lists_t *L; int device; float rate_cell; uint32_t seed;
    fastf_engine_t *e;
    uint32_t n_cells, key_bits, kflags; int blocked, segmented;
    uint64_t key_slots, H, blk_layout;
    int genes; uint32_t n_features;      /* --genes: the per-gene arrays of a point (buf.cpg, buf.upg and their pinned copies, n_features entries each) */
    /* --cells: where fastf_res_point_run left the point's sorted keys (sorted_full: by every bit, the FASTF_ERR_RUN_TOO_LONG branch
     * ran) and the other buffer of the pair */
    int cells, sorted_full; uint64_t *sorted, *sorted_other;
    uint64_t full_nnz;                   /* the pair's full rows in buf.full (their number in buf.small[SM_FULL] too) */
    size_t nbr_map_bytes, mk_set;        /* the bytes of the slot map; of one set of marker tables in buf.h_mk */
    uint32_t pt_m;                       /* --pseudotime: the cells of the pair with a value */
    uint32_t hvg_k, nbr_planes, full_planes, n_labels;   /* the genes of A and the byte planes of the row set at hand (fastf_res_full_keep); full_planes: --mapping, those of the full rows in buf.fplanes */
    struct {
        res_buf_t blk, keys, tmp, small, rows, upc, gpc, h_small, h_upc, h_gpc, h_rows;   /* h_rows.n: the rows there is room for */
        res_buf_t cpg, upg, h_cpg, h_upg, cellsum, h_cellsum, level;
        res_buf_t full, fid, h_fid, gx, gfid, h_gfid;   /* gx: the partner column, x of every point row (u32, R->n entries) */
        res_buf_t nbr, h_nbr, nplanes, lab, h_lab, mk, h_mk, mk_rank;   /* mk_rank: the ranks of the full rows and of the point (host) */
        res_buf_t map, h_map, fplanes;       /* --mapping: the device and the pinned block, the byte planes of the full rows for the life of the pair */
        res_buf_t pt, h_pt;                  /* --pseudotime: the device and the pinned block */
        res_buf_t cx, h_cx, cxwork;          /* --coexpression: the device and the pinned block, the gene-major planes of the row set at hand */
    } buf;
    res_cellsum_v h_cs; res_level_v lv; res_fid_v d_fid, h_fid; res_gfid_v d_gfid, h_gfid;   /* with --genes h_gfid.sy and h_gfid.c are buf.h_upg and buf.h_cpg */
    res_nbr_v d_nbr; res_nbr_pin_v h_nbr; res_lab_v d_lab, h_lab; res_map_v d_map, h_map; res_pt_v d_pt, h_pt; res_cx_v d_cx; res_cx_pin_v h_cx;
} res_rate_t;
static inline res_rows_t res_rows_point(const res_rate_t *S) { return res_rows(S->buf.rows.p, S->R->n); }   /* the rows of the last point */
static inline res_rows_t res_rows_full(const res_rate_t *S) { return res_rows(S->buf.full.p, S->R->n); }     /* the full rows of the pair */
int  fastf_res_rate_open(res_rate_t *S, const char *verb, const resident_t *R, const fastf_lists_t *L, const uint64_t *cell_keys, float rate_cell,
                         uint32_t seed, int device, int genes, int cells, res_times_t *T) FASTF_HIDDEN;
void fastf_res_rate_close(res_rate_t *S) FASTF_HIDDEN;
/* one point: K1b on the decision plane (H decisions), sort, reduce, rows gathered on the device, per-cell summary to the host
 * (S->buf.h_upc[0 .. n_cells]: UMIs per cell and their sum, S->buf.h_gpc: genes per cell) and, with S->genes, the per-gene summary on the
 * same stream (S->buf.h_cpg: cells per gene, S->buf.h_upg: UMIs per gene); counters = {total, sampled, sampled_valid} */
int  fastf_res_point_run(res_rate_t *S, const uint32_t *d_plane, const char *point_name, uint64_t counters[3], uint64_t *nnz, res_times_t *T) FASTF_HIDDEN;
/* the rows of the last point into pinned memory, and the three files of bam2db into dir (created) */
int  fastf_res_point_write(res_rate_t *S, const char *dir, const char *bam_label, float rate_depth, const uint64_t counters[3], uint64_t nnz,
                           res_times_t *T) FASTF_HIDDEN;

/* level (level_cmds.c): the search for the per-cell thresholds.  fastf_res_level_room: the state arrays of S, after every open.
 * fastf_res_search_pass: the device half of fastf_res_point_run up to fastf_dev_cell_summary on the plane d_plane, then one step of the
 * search on the device and ONE device-to-host copy, of the small block (counters, error bits, the step's result): no per-cell or
 * per-gene array and no row leaves the device.  first != 0: the pass whose plane keeps every hit — its U_k(2^32) is kept in
 * S->lv.ufull for every cap of the pair and the state is initialised for umi_cap from it (*capped_out: the cells with
 * U_k(2^32) > umi_cap); else S->buf.upc is U_k(S->lv.probe) and the state moves by the rules of fastf_dev_level_step.  Either way
 * S->lv.probe then holds the thresholds of the next pass and *open_out the cells still open.  The error bits of the pass are
 * handled as fastf_res_point_run handles them (RES_NOT_COVERED; a run too long for the group-only sort is sorted fully and the
 * step taken again, which costs that pass a second small copy).  fastf_res_level_init: the state for another cap of the same
 * pair, from S->lv.ufull. */
int  fastf_res_level_room(res_rate_t *S) FASTF_HIDDEN;
int  fastf_res_search_pass(res_rate_t *S, const uint32_t *d_plane, const char *point_name, uint64_t umi_cap, int first, uint64_t *open_out,
                           uint64_t *capped_out, res_times_t *T) FASTF_HIDDEN;
int  fastf_res_level_init(res_rate_t *S, uint64_t umi_cap, uint64_t *open_out, uint64_t *capped_out, res_times_t *T) FASTF_HIDDEN;

/* --fidelity (S->cfg.fidelity).  fastf_res_full_keep: behind a pass on the all-ones plane that left its gathered rows in S->buf.rows, their
 * count in S->buf.h_small[SM_NNZ] and their per-cell summary in S->buf.upc / S->buf.gpc (fastf_res_point_run, or level's first
 * fastf_res_search_pass) — the rows copied into S->buf.full, sum_xx by the join of the full rows with themselves, umis_full and
 * genes_full to the host: once per pair.  fastf_res_full_run: fastf_res_point_run on d_plane (every hit kept) and that.
 * fastf_res_point_fidelity: behind fastf_res_point_run, the join of the point's rows (still in S->buf.rows) with the full rows, S->h_fid.sxy
 * and S->h_fid.syy to the host; a row without a partner fails the point.  fastf_res_full_keep and fastf_res_full_run do nothing without
 * S->cfg.fidelity or S->cfg.gene_fid, fastf_res_point_fidelity nothing without S->cfg.fidelity.
 * --gene-fidelity (S->cfg.gene_fid).  fastf_res_full_keep also leaves the pair's sum_x, cells_full and sum_xx per gene in S->h_gfid.sx, S->h_gfid.cf
 * and S->h_gfid.sxx.  fastf_res_point_gene_fidelity: behind fastf_res_point_run (and fastf_res_point_fidelity), before fastf_res_point_cells —
 * every point row's partner count into S->buf.gx, then sum_y, cells, sum_yy and sum_xy per gene to the host (S->h_gfid.sy, S->h_gfid.c,
 * S->h_gfid.syy, S->h_gfid.sxy); a row without a partner fails the point.  Nothing without S->cfg.gene_fid */
int  fastf_res_full_keep(res_rate_t *S, res_times_t *T) FASTF_HIDDEN;
/* a pair needs its full rows: any of the three is on (labels and markers come with neighbors).  fastf_res_full_timer: where the
 * full-depth work of a pair is booked (per_gene: its per-gene sums, which --fidelity has no part in) */
static inline int res_cfg_full(const res_cfg_t *cfg) { return cfg->fidelity || cfg->gene_fid || cfg->neighbors || cfg->coexpr; }
static inline int res_cfg_per_gene(const res_cfg_t *cfg) { return cfg->gene_fid || cfg->neighbors || cfg->coexpr; }   /* the pair's per-gene sums: --gene-fidelity's own, and what ranks A */
double *fastf_res_full_timer(const res_rate_t *S, res_times_t *T, int per_gene) FASTF_HIDDEN;
int  fastf_res_full_run(res_rate_t *S, const uint32_t *d_plane, res_times_t *T) FASTF_HIDDEN;
int  fastf_res_point_fidelity(res_rate_t *S, const char *point_name, res_times_t *T) FASTF_HIDDEN;
int  fastf_res_point_gene_fidelity(res_rate_t *S, const char *point_name, res_times_t *T) FASTF_HIDDEN;
/* --neighbors (S->cfg.neighbors).  fastf_res_full_keep also ranks A of the pair from S->h_gfid.sx and S->h_gfid.sxx (S->hvg_k genes), lays the slot
 * map down, and leaves the neighbour sets of the full rows on the device and k_full in S->h_nbr.kf.  fastf_res_point_neighbors: behind
 * fastf_res_point_run, before fastf_res_point_cells — the planes and neighbour sets of the point's rows, the shared counts, k_point and
 * shared to the host (S->h_nbr.kp, S->h_nbr.sh).  A count beyond three planes or a norm of 2^42 and beyond fails the pair by name.  Nothing
 * without S->cfg.neighbors */
int  fastf_res_point_neighbors(res_rate_t *S, const char *point_name, res_times_t *T) FASTF_HIDDEN;
/* --labels (S->cfg.labels).  fastf_res_rate_open lays lab[] of the pair's cells down and uploads it, once per pair; fastf_res_full_keep votes
 * on the full sets and brings pred, same, labelled and conf_X to the host, once per pair.  fastf_res_point_labels: directly behind
 * fastf_res_point_neighbors, before fastf_res_point_cells — one vote call on the point's sets, then pred_point, same_point,
 * labelled_point and conf_Y to the host in one copy.  Nothing without S->cfg.labels */
int  fastf_res_point_labels(res_rate_t *S, const char *point_name, res_times_t *T) FASTF_HIDDEN;
/* --markers (S->cfg.markers).  fastf_res_full_keep runs fastf_dev_marker_auc once per pair on the planes of the full rows, before the first
 * point overwrites the plane buffer, brings the four tables to the host and ranks them (the full ranks stay for every point of the
 * pair).  fastf_res_point_markers: directly behind fastf_res_point_labels — the same on the point's planes (with the point's own P).
 * A row set with three planes fails the pair by name (FASTF_ERR_MARKER_COUNT).  Nothing without S->cfg.markers.  The pinned tables and the ranks of the full rows (0) and of the point (1): */
int  fastf_res_point_markers(res_rate_t *S, const char *point_name, res_times_t *T) FASTF_HIDDEN;
static inline res_mk_v res_mk_host(const res_rate_t *S, int point) { return res_mk_layout(S->buf.h_mk.u8 + (size_t)point * S->mk_set, S->n_labels, S->hvg_k); }
static inline const uint32_t *res_mk_rank(const res_rate_t *S, int point) { return S->buf.mk_rank.u32 + (size_t)point * S->n_labels * FASTF_HVG_TOP; }
/* --mapping (S->cfg.mapping; S->cfg.neighbors is on with it).  fastf_res_full_keep copies the byte planes of the full rows out of the plane
 * buffer (S->buf.fplanes, S->full_planes of them) and their norms into the block, before the first point overwrites either.
 * fastf_res_point_mapping: directly behind fastf_res_point_labels, while the point's planes are in S->buf.nplanes — fastf_dev_mapping, the
 * shared counts with the full sets, with --labels the votes over M, then self_dot, self_rank, k_map, hood and the vote bytes to the host
 * in ONE copy (S->h_map).  A norm of 2^42 and beyond on either side fails the point by name.  Nothing without S->cfg.mapping */
int  fastf_res_point_mapping(res_rate_t *S, const char *point_name, res_times_t *T) FASTF_HIDDEN;
/* --pseudotime (S->cfg.ptime; S->cfg.neighbors is on with it).  fastf_res_rate_open ranks the pair's cells (fastf_ptime_assign) and uploads
 * t[] beside lab[].  One side is a median call and a census call on a list of neighbours, then its half of the block — the census, est,
 * valued — to the host in ONE copy: the full sets in fastf_res_full_keep (half 0, which stays for every point of the pair), the point's
 * sets in fastf_res_point_ptime (half 1), directly behind fastf_res_point_labels, and with --mapping the list M inside
 * fastf_res_point_mapping (half 2), while that list is live.  Nothing without S->cfg.ptime */
int  fastf_res_point_ptime(res_rate_t *S, const char *point_name, res_times_t *T) FASTF_HIDDEN;
/* --coexpression (S->cfg.coexpr).  fastf_res_full_keep ranks A exactly as for --neighbors (alone it switches on the full rows, the pair's
 * per-gene sums and the slot map, and nothing of the neighbour sets), and leaves the partner sets of the full rows on the device and
 * k_full in S->h_cx.kf.  fastf_res_point_coexpr: directly behind fastf_res_point_markers — the gene-major planes, D, S and the partner sets
 * of the point's rows, the shared counts, k_point and shared to the host (S->h_cx.kp, S->h_cx.sh).  A count beyond three planes, sums
 * beyond 64 bits or n * max Q of 2^63 and beyond fail the pair or the point by name.  Nothing without S->cfg.coexpr */
int  fastf_res_point_coexpr(res_rate_t *S, const char *point_name, res_times_t *T) FASTF_HIDDEN;
/* the eight above in their order (fidelity, gene fidelity, neighbors, labels, pseudotime, mapping, markers, co-expression), behind fastf_res_point_run and before
 * fastf_res_point_write and fastf_res_point_cells: the one place a further comparison of a point is called from */
int  fastf_res_point_compare(res_rate_t *S, const char *point_name, res_times_t *T) FASTF_HIDDEN;

/* --cells, behind a point (S->cells): the keys fastf_res_point_run left sorted fully (skipped where that call already did), K3u
 * into S->buf.rows — 12 bytes a record, free once the summaries of fastf_res_point_run have run: fastf_res_point_write gathers into
 * pinned memory and nothing else reads it before the next point's gather overwrites it — then fastf_dev_copy_summary and the four
 * arrays to the host (S->h_cs.hist, S->h_cs.rpc, S->h_cs.npc, S->h_cs.spc).  Call it after fastf_res_point_write, or directly after
 * fastf_res_point_run when no rows are written: K3u overwrites the row regions that call gathers from. */
int  fastf_res_point_cells(res_rate_t *S, const char *point_name, res_times_t *T) FASTF_HIDDEN;

/* ---- the tables and point files of a run (res_tables.c) ----
 * the per-verb tables <out_dir>/<verb>_<stem>.tsv: their stems and headers are defined once (grid_rows.c: GRID_TABLES, from which the
 * exported fastf_<verb>_<stem>_header getters come too) and looked up by (verb index, table id) */
typedef struct res_verb res_verb_t;
enum { VERB_SWEEP, VERB_CAP, VERB_LEVEL };
enum { TB_GENES, TB_CELLS, TB_FIDELITY, TB_GENE_FIDELITY, TB_NEIGHBORS, TB_LABELS, TB_LABEL_CLASSES, TB_MARKERS, TB_COEXPR, TB_MAPPING, TB_PTIME, TB_REPS, TB_GENES_REPS, TB_N_ };
const char *fastf_res_table_stem(int table) FASTF_HIDDEN;
const char *fastf_res_table_header(int verb, int table) FASTF_HIDDEN;

/* a table: written as <out_dir>/<name>.partial, renamed to <out_dir>/<name> by a close with ok != 0; otherwise nothing of it is left.
 * fastf_res_table_open: the per-verb table `table` of V, under its name and header */
typedef struct { FILE *f; char tmp[4096], final[4096]; } res_tsv_t;
int fastf_res_tsv_open(res_tsv_t *t, const char *out_dir, const char *name, const char *header) FASTF_HIDDEN;
int fastf_res_table_open(res_tsv_t *t, const res_verb_t *V, const char *out_dir, int table) FASTF_HIDDEN;
int fastf_res_tsv_close(res_tsv_t *t, int ok) FASTF_HIDDEN;

/* a text that grows, and its file: fastf_res_text_file writes the finished text t, gzipped, as dir/name through dir/name.partial (dir is
 * created) unless bad != 0 — the text was not finished — and frees it either way; returns bad, or 1 after its own error */
typedef struct { char *p; size_t len, cap; } gtext;
int fastf_gt_str(gtext *t, const char *s) FASTF_HIDDEN;
int fastf_gt_u64(gtext *t, char lead, uint64_t v) FASTF_HIDDEN;       /* `lead`, then v in decimal */
int fastf_res_text_file(const char *dir, const char *name, gtext *t, int bad) FASTF_HIDDEN;

/* --genes of a verb: <out_dir>/<verb>_genes.tsv (one row per point, through .partial), <out_dir>/<verb>_gene_cells.tsv.gz (the cells
 * per gene of every point, written by a close with ok != 0) and <point dir>/genes.tsv.gz.  on == 0: every call does nothing */
typedef struct {
    int on, no_grid; const char *verb; char out_dir[4096];   /* no_grid: a replicate run — no <verb>_gene_cells.tsv.gz, no cells[] kept */
    res_tsv_t tsv;
    uint32_t n_features, n_points, max_points;
    char **feat_id;                      /* copies: the lists of the first point */
    uint32_t *cells;                     /* [max_points][n_features] */
    char (*names)[64];                   /* the point directory names */
} res_genes_t;
int fastf_res_genes_open(res_genes_t *G, int on, const res_verb_t *V, const char *out_dir, uint32_t max_points, int no_grid) FASTF_HIDDEN;
/* one point: `row` (fastf_genes_summary_row) into the table, cells[] kept for the grid file, and — dir != NULL — dir/genes.tsv.gz */
int fastf_res_genes_point(res_genes_t *G, const fastf_lists_t *L, const char *point_name, const char *dir, const char *row,
                          const uint32_t *cells, const uint64_t *umis) FASTF_HIDDEN;
int fastf_res_genes_close(res_genes_t *G, int ok) FASTF_HIDDEN;

/* --cells of a verb: <out_dir>/<verb>_cells.tsv (one row per point, through .partial) and <point dir>/cells.tsv.gz.  on == 0: every
 * call does nothing */
typedef struct { int on; const char *verb; res_tsv_t tsv; } res_cells_t;
int fastf_res_cells_open(res_cells_t *C, int on, const res_verb_t *V, const char *out_dir) FASTF_HIDDEN;
/* one point, after fastf_res_point_cells: `row` (fastf_cells_summary_row) into the table and — dir != NULL — dir/cells.tsv.gz from the
 * arrays of S (h_rpc, h_npc, h_upc, h_gpc, h_spc) and the barcodes of its lists */
int fastf_res_cells_point(res_cells_t *C, const res_rate_t *S, const char *dir, const char *row) FASTF_HIDDEN;
int fastf_res_cells_close(res_cells_t *C, int ok) FASTF_HIDDEN;

/* the comparisons of a point against full depth: --neighbors, --labels FILE, --markers N, --coexpression, --mapping, --pseudotime FILE, --gene-fidelity, --fidelity, in the order a
 * point writes them.  Each is ONE descriptor in res_tables.c — its tables (labels has two: labels and label_classes), its timer in
 * res_times_t, its point writer, which puts the point's row(s) into the table(s) and, with a directory, <point dir>/<name>.tsv.gz
 * (labels: labels.tsv.gz and label_confusion.tsv.gz) from the host views of S.  on: bit c set — comparison c is on; tsv: the tables
 * TB_FIDELITY .. TB_PTIME at [table - TB_FIDELITY], which is the order they are opened and renamed in.
 * fastf_res_cmp_open clears C and opens the tables of the comparisons the flag word (FASTF_SWEEP_*), labels != NULL, markers != 0,
 * mapping != 0 and ptime != NULL switch on; on failure nothing of them is left.  fastf_res_cmp_cfg: what the device side is to compute for them (S->cfg).
 * fastf_res_cmp_point: one point, behind fastf_res_point_compare — every writer that is on, timed into its timer (list_value == 0:
 * rate_depth in the second column).  fastf_res_cmp_close closes every table before it renames any, and where a rename fails no
 * table is left and the message names the file.  A C that is all zero is closed: every call on it does nothing */
enum { CMP_NEIGHBORS, CMP_LABELS, CMP_MARKERS, CMP_COEXPR, CMP_MAPPING, CMP_PTIME, CMP_GENE_FID, CMP_FIDELITY, CMP_N_ };
#define RES_CMP_TABLES (TB_PTIME - TB_FIDELITY + 1)
typedef struct { uint32_t on; res_tsv_t tsv[RES_CMP_TABLES]; const fastf_labels_t *labels; uint32_t markers; const fastf_ptime_t *ptime; } res_cmp_t;
static inline int res_cmp_on(const res_cmp_t *C, int c) { return (int)(C->on >> c & 1); }
int  fastf_res_cmp_open(res_cmp_t *C, const res_verb_t *V, const char *out_dir, uint32_t flags, const fastf_labels_t *labels, uint32_t markers, uint32_t mapping,
                        const fastf_ptime_t *ptime) FASTF_HIDDEN;
void fastf_res_cmp_cfg(const res_cmp_t *C, res_cfg_t *cfg) FASTF_HIDDEN;
int  fastf_res_cmp_point(res_cmp_t *C, const res_rate_t *S, const char *dir, float rate_depth, uint64_t list_value, res_times_t *T) FASTF_HIDDEN;
int  fastf_res_cmp_close(res_cmp_t *C, int ok) FASTF_HIDDEN;

/* replicate runs (--seeds, --reps; fastf_sweep_reps, fastf_cap_reps): <verb>_reps.tsv, and with --genes <verb>_genes_reps.tsv and
 * <verb>_gene_reps.tsv.gz.  The metrics of the cell rate in work are kept per (list value j, seed k) until its last seed is done;
 * the per-gene accumulators of that cell rate live on the device (d_acc: [n_list][3][n_features] u64, fastf_dev_gene_reps_add behind
 * every point) and come to the host once per grid point, in fastf_res_reps_rate_end; on the point-by-point path (no device arrays)
 * the host twin adds into h_acc directly.  on == 0: every call does nothing */
typedef struct {
    int on, genes, device; const char *verb; char out_dir[4096];
    uint32_t n_seeds, n_list, n_rates, rate_at; const uint32_t *seeds;
    res_tsv_t tsv, gtsv;
    double *m;                           /* [n_list][n_seeds][FASTF_REPS_METRICS] */
    uint32_t *n_cells, *gdet;            /* [n_list][n_seeds]: the sampled cells, the genes detected */
    uint8_t *seen;                       /* [n_list][n_seeds] */
    uint32_t n_features; char **feat_id;
    void *d_acc; uint64_t *h_acc;        /* h_acc: [n_rates * n_list][3][n_features] */
} res_reps_t;
int fastf_res_reps_open(res_reps_t *P, int on, const res_verb_t *V, const char *out_dir, const uint32_t *seeds, uint32_t n_seeds, uint32_t n_rates,
                        uint32_t n_list, int genes, int device) FASTF_HIDDEN;
/* a cell rate begins: the names of the features (first call), the accumulators cleared; on_device: d_acc is used */
int fastf_res_reps_rate_begin(res_reps_t *P, const fastf_lists_t *L, int on_device) FASTF_HIDDEN;
/* point (list value j, seed k) of the cell rate in work: its metrics; with --genes its per-gene array — S != NULL: S->buf.cpg on the
 * device, right behind the point's fastf_res_point_run; else cells_per_gene on the host */
int fastf_res_reps_point(res_reps_t *P, uint32_t j, uint32_t k, uint32_t n_cells, const double *metrics) FASTF_HIDDEN;
int fastf_res_reps_genes(res_reps_t *P, res_rate_t *S, uint32_t j, uint32_t k, const uint32_t *cells_per_gene, uint32_t n_features) FASTF_HIDDEN;
/* the last seed of the cell rate is done: its rows; rates_depth or caps names the verb's list (the other NULL) */
int fastf_res_reps_rate_end(res_reps_t *P, float rate_cell, const float *rates_depth, const uint64_t *caps, res_times_t *T) FASTF_HIDDEN;
/* ok != 0: <verb>_gene_reps.tsv.gz (its columns named from the grid: rates_cell and ONE of rates_depth / caps), then the tables
 * renamed; otherwise nothing of them is left */
int fastf_res_reps_close_grid(res_reps_t *P, int ok, const float *rates_cell, const float *rates_depth, const uint64_t *caps) FASTF_HIDDEN;
int fastf_res_reps_close(res_reps_t *P, int ok) FASTF_HIDDEN;   /* ok == 0 only */
/* a replicate run failed after tables were renamed into place: none of <verb>_{genes,cells,reps,genes_reps}.tsv, of the tables of
 * res_cmp_t and <verb>_gene_reps.tsv.gz is left (res_tables.c) */
void fastf_res_reps_unlink_tables(const char *out_dir, const char *verb) FASTF_HIDDEN;
/* the most cells any pair of the lists samples */
uint32_t fastf_res_lists_max_cells(const res_lists_t *l) FASTF_HIDDEN;

/* ---- the command (resident.c) ----
 * ONE command line, ONE body and ONE help text for the three verbs: -h -b -f -a -d -c -o -s -u --summary-only --genes --cells --fidelity
 * --gene-fidelity --neighbors --coexpression --mapping --labels --markers --pseudotime --seeds --reps and ONE list option of the verb's own.
 * What a verb does not share is its res_cmd_t, ONE static const instance in its file:
 *   list_short, list_long   its list option: -r/--depth, -n/--reads, -m/--umis
 *   parse_caps              the parser of a caps list; NULL: the list holds depth rates (fastf_sweep_parse_rates)
 *   u_message               what -u is refused with
 *   needs_list              what a command line without the list is refused with; NULL: list_default stands in for it
 *   help_*                  the help text's intro, the line of the list option, the list's part of a point directory's name, and what
 *                           follows an option that a verb with a point-by-point form has in its resident form only ("" without one)
 * fastf_res_cmd: the options, the missing list, the cell rates, the list and the grid (the verb's check_caps, or fastf_sweep_check_grid),
 * the three input files, the run through fastf_res_grid_entry ("<verb> failed: ..."), the "... is generated." lines.  An option is
 * added in the table and the switch of fastf_res_parse_args, in res_args_t, in the help template (fastf_res_usage) and, where it is
 * no flag bit, in the call of fastf_res_cmd; fastf_res_print_generated names its table.
 * res_args_t: n_seeds >= 1: a replicate run over seeds[] (--seeds as listed; --reps N: seed, seed + 1, ..); 0: neither option was given */
typedef struct {
    char list_short; const char *list_long, *list_default;
    int (*parse_caps)(const char *text, uint64_t *out, uint32_t cap, uint32_t *n_out);
    const char *u_message, *needs_list;
    const char *help_intro, *help_list, *help_point, *help_resident;
} res_cmd_t;
typedef struct { const char *bam, *feat, *bar, *out, *cells, *list; unsigned int seed; int summary_only, genes, per_cell, fidelity, gene_fidelity, neighbors, coexpression, mapping; const char *labels, *pseudotime; uint32_t markers;   /* markers: N of --markers, 0 without */
                 uint32_t seeds[FASTF_MAX_SEEDS], n_seeds; } res_args_t;   /* cells: the -c list; per_cell: --cells */
int fastf_res_cmd(const res_verb_t *V, const res_cmd_t *D, int argc, const char **argv) FASTF_HIDDEN;

/* ---- the grid driver (grid_run.c) ----
 * res_job_t: what an entry point of a verb was asked for.  The verb's list is rates_depth (sweep) or caps (cap, level), the other NULL —
 * the convention of fastf_res_reps_rate_end and of the *_summary_row(rate_depth, list_value) functions.  reps != 0: a replicate run
 * (the suffixed directories and the replicate tables, with one seed too), its seeds checked by the driver */
typedef struct {
    const char *bam, *out_dir, *barcodes, *features;
    const float *rates_cell; uint32_t n_c;
    const float *rates_depth; const uint64_t *caps; uint32_t n_list;
    const uint32_t *seeds; uint32_t n_s; int reps;
    uint32_t flags; const char *labels_path; uint32_t markers, mapping; const char *ptime_path;
} res_job_t;
/* the tables of a run, zeroed before the first open: every close is safe on a table that was never opened */
typedef struct { res_tsv_t tsv; res_genes_t G; res_cells_t C; res_cmp_t Fd; res_reps_t P; } res_tables_t;
/* one (cell rate, seed) pair as the hooks see it: S is open (fastf_res_rate_open) */
typedef struct {
    const res_job_t *job; res_rate_t *S; const resident_t *R; const fastf_lists_t *L; res_times_t *T;
    float rate_cell; uint32_t seed; int device, summary_only, prof;   /* prof: FASTF_PROFILE is set */
} res_pair_t;
/* a verb: ONE static const instance in its file.  The hooks (ctx: what pair_begin made, handed to the others; a hook that is NULL is
 * not called):
 *   pair_begin   what a pair needs before its first point — sweep: every plane of the pair in one fastf_dev_mt_decisions_multi call and
 *                the full rows from the extra plane; cap: the hits per cell, and the full rows from an all-ones plane; level: the
 *                search state, pass 0 with every hit kept, the full rows kept from it.  RES_*
 *   point_plane  the decision plane of list value j — sweep: an offset into the planes; cap: the thresholds of the cap and their plane;
 *                level: the probing passes, then the plane of the thresholds found.  RES_*
 *   point_done   level: its profile line of the point, directly behind fastf_res_point_run
 *   point_row    the row of the verb's summary table and the metrics of fastf_summary_tail_
 *   point_files  level: thresholds.tsv.gz into the point's directory, behind fastf_res_point_write
 *   pair_end     frees what pair_begin made (ctx may be NULL or half built)
 *   run_profile  level: its search line under FASTF_PROFILE, behind the stage line
 *   point_by_point  sweep: the grid through bam2db() for a job outside the resident form; the tables were opened afresh */
struct res_verb {
    const char *name; int index;         /* index: VERB_*, which picks the verb's headers of the per-verb tables */
    const char *(*header)(void);         /* of <verb>.tsv */
    /* cap, level: the grid check and the directory name of a point of a caps list; NULL: sweep's, of a depth-rate list */
    int (*check_caps)(const float *rates_cell, uint32_t n_c, const uint64_t *caps, uint32_t n);
    int (*caps_point_dir)(float rate_cell, uint64_t cap_value, char *buf, size_t cap);
    const char *refusal_tail;            /* behind the refusal of a job outside the resident form; NULL with point_by_point */
    const char *planes_words;            /* the stage line: what T->planes holds */
    const char *fid_before, *fid_after;  /* the --fidelity line: around the number of pairs */
    int unlink_reps_always;              /* a failed run removes the replicate tables even when it is no replicate run */
    int  (*pair_begin)(const res_pair_t *p, void **ctx);
    int  (*point_plane)(void *ctx, const res_pair_t *p, uint32_t j, const char *point_name, const uint32_t **d_plane);
    void (*point_done)(void *ctx, const res_pair_t *p, const char *point_name);
    int  (*point_row)(void *ctx, const res_pair_t *p, uint32_t j, const uint64_t counters[3], uint64_t nnz, char *row, size_t cap, double *metrics);
    int  (*point_files)(void *ctx, const res_pair_t *p, const char *dir);
    void (*pair_end)(void *ctx);
    void (*run_profile)(const res_job_t *job, const res_times_t *T);
    int  (*point_by_point)(const res_job_t *job, int summary_only, res_tables_t *tb);
};
/* the run of an entry point: the seeds of a replicate run, null arguments, with labels_path the bam file and the labels (before anything
 * is written), the grid, the flags, the bam file, the devices, the output directory, the tables, the pairs, the close */
int fastf_res_grid_run(const res_verb_t *V, const res_job_t *job) FASTF_HIDDEN;
/* the ONE way into it: each of the six exported calls of a verb (fastf_<verb>, _reps, _labels, _markers, _mapping, _pseudotime) and its
 * command forward here with the union of their arguments — what a call does not take is NULL or 0, the verb's list is ONE of
 * rates_depth / caps.  It fills the res_job_t — the ONE place a new option of a run is carried from an argument into the job — and
 * checks what the entry points check before the driver: mapping beyond 1 first, then N of --markers and its labels path where N != 0.
 * how: ENTRY_REPS — fastf_<verb>_reps: a replicate run whatever n_seeds is (0 is then refused by the driver's seed check); otherwise
 * n_seeds == 0 is the plain run at `seed`.  ENTRY_MARKERS — fastf_<verb>_markers: N and the labels path are checked with N == 0 too */
enum { ENTRY_REPS = 1, ENTRY_MARKERS = 2 };
int fastf_res_grid_entry(const res_verb_t *V, unsigned how, const char *bam, const char *out_dir, const char *barcodes, const char *features,
                         const float *rates_cell, uint32_t n_c, const float *rates_depth, const uint64_t *caps, uint32_t n_list,
                         const uint32_t *seeds, uint32_t n_seeds, uint32_t seed, uint32_t flags,
                         const char *labels_path, uint32_t markers, uint32_t mapping, const char *ptime_path) FASTF_HIDDEN;

/* grid_rows.c: the columns of a summary row from `seed` on (no newline); metrics != NULL: the FASTF_REPS_METRICS numbers a replicate
 * table takes from the row (sampled_reads, sampled_valid_reads, nnz, umis, saturation, the two medians) as the row printed them */
int fastf_summary_tail_(uint32_t seed, const uint64_t counters[3], uint64_t nnz, uint64_t umis, const uint64_t *umis_per_cell,
                        const uint32_t *genes_per_cell, uint32_t n_cells, char *buf, size_t cap, double *metrics) FASTF_HIDDEN;

/* grid_rows.c: one row of sweep.tsv (with its newline); metrics: fastf_summary_tail_ */
int fastf_sweep_row_(float rate_cell, float rate_depth, uint32_t seed, const uint64_t counters[3], uint64_t nnz, uint64_t umis,
                     const uint64_t *umis_per_cell, const uint32_t *genes_per_cell, uint32_t n_cells, char *buf, size_t cap, double *metrics) FASTF_HIDDEN;

/* cap_cmds.c: one row of cap.tsv or level.tsv (with its newline); metrics: fastf_summary_tail_ */
int fastf_cap_row_(float rate_cell, uint64_t list_value, uint32_t seed, const uint64_t counters[3], uint64_t nnz, uint64_t umis,
                   const uint64_t *umis_per_cell, const uint32_t *genes_per_cell, uint32_t n_cells, uint64_t hits, uint32_t cells_capped,
                   char *buf, size_t cap, double *metrics) FASTF_HIDDEN;

#endif
