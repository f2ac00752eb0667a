/*
 * cap_cmds.c — `fastF cap`: every cell downsampled to at most N reads, over a grid of (cell rate, cap) points from ONE decode of
 * the BAM.
 *
 *   cmd_cap()    the command the three verbs share (resident.c: fastf_res_cmd) with this verb's res_cmd_t: its list option -n <list>,
 *                which has no default, its -u message and its words of the help text
 *   fastf_cap()  the same in process, and _reps, _labels, _markers, _mapping, _pseudotime: each ONE forwarding statement to
 *                fastf_res_grid_entry (grid_run.c), as sweep's (sweep_cmds.c)
 * Per point <out>/c<rate_cell>_n<N>/{matrix.mtx.gz, barcodes.tsv.gz, features.tsv.gz} and one row of <out>/cap.tsv.
 *
 * The resident pipeline of sweep (resident.c).  Per cell rate K1a once, the hits per cell counted on the device
 * (fastf_dev_cell_hits) and copied to the host once; per cap the per-cell thresholds computed on the host (n_cells is small, the
 * device does no floating point) and sent to the device, the decision plane made from the draw stream and the thresholds
 * (fastf_dev_cell_decisions), then K1b on that plane and everything behind it as in bam2db.  A global depth rate cannot express a
 * cap, so a job outside the resident form is refused: there is no point-by-point fallback.
 * --genes: as in sweep (cap_genes.tsv, cap_gene_cells.tsv.gz, genes.tsv.gz per point; resident.c).
 * --cells: as in sweep (cap_cells.tsv, cells.tsv.gz per point; fastf_res_point_cells behind every point): the reads each cell kept.
 */
#define _GNU_SOURCE
#include "resident.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* ------------------------------------------------------------------ */
/* the grid                                                            */
/* ------------------------------------------------------------------ */
/* "10,100,1000" -> integers >= 1: digits only (no sign, no blanks); refused: an empty list or element, 0, a value twice */
int fastf_cap_parse_caps(const char *text, uint64_t *out, uint32_t cap, uint32_t *n_out)
{
    uint32_t n = 0;
    if (n_out) *n_out = 0;
    if (!text || !out || !n_out) return fastf_res_err("null argument");
    for (const char *p = text;;) {
        const char *q = p;
        uint64_t v = 0;
        if (*q == ',' || !*q) return fastf_res_err("reads per cell `%s`: empty element", text);
        for (; *q && *q != ','; q++) {
            if (*q < '0' || *q > '9') return fastf_res_err("reads per cell `%s`: expects positive integers", text);
            if (v > (UINT64_MAX - (uint64_t)(*q - '0')) / 10) return fastf_res_err("reads per cell `%s`: numerical result out of range", text);
            v = v * 10 + (uint64_t)(*q - '0');
        }
        if (v < 1) return fastf_res_err("reads per cell `%s`: a cap is at least 1", text);
        for (uint32_t j = 0; j < n; j++) if (out[j] == v) return fastf_res_err("reads per cell `%s`: %llu is listed twice", text, (unsigned long long)v);
        if (n == cap) return fastf_res_err("reads per cell `%s`: more than %u values", text, cap);
        out[n++] = v;
        if (!*q) break;
        p = q + 1;
    }
    *n_out = n;
    return 0;
}

int fastf_cap_point_dir(float rate_cell, uint64_t reads_per_cell, char *buf, size_t cap)
{
    const int n = snprintf(buf, cap, "c%.3f_n%llu", (double)rate_cell, (unsigned long long)reads_per_cell);
    return (n < 0 || (size_t)n >= cap) ? fastf_res_err("directory name too long") : 0;
}

int fastf_cap_check_grid(const float *rates_cell, uint32_t n_c, const uint64_t *caps, uint32_t n_n)
{
    if (!n_c || !n_n || !rates_cell || !caps) return fastf_res_err("cap: the grid needs at least one cell rate and one cap");
    const float one = 1.0f;
    if (fastf_sweep_check_grid(rates_cell, n_c, &one, 1)) {       /* the cell rates are sweep's */
        char keep[400]; snprintf(keep, sizeof keep, "%s", fastf_last_error());
        return fastf_res_err("cap: %s", !strncmp(keep, "sweep: ", 7) ? keep + 7 : keep);
    }
    for (uint32_t i = 0; i < n_n; i++) {
        if (caps[i] < 1) return fastf_res_err("cap: reads per cell %llu: a cap is at least 1", (unsigned long long)caps[i]);
        for (uint32_t j = 0; j < i; j++) if (caps[j] == caps[i]) return fastf_res_err("cap: reads per cell %llu is listed twice", (unsigned long long)caps[i]);
    }
    return 0;
}

/* ------------------------------------------------------------------ */
/* thresholds, the summary row (level.tsv has cap.tsv's columns)       */
/* ------------------------------------------------------------------ */
int fastf_cap_thresholds(const uint32_t *hits, uint32_t n_cells, uint64_t cap, uint64_t *thresholds_out)
{
    if (n_cells && (!hits || !thresholds_out)) return fastf_res_err("null argument");
    if (cap < 1) return fastf_res_err("cap: a cap is at least 1");
    for (uint32_t k = 0; k < n_cells; k++)
        thresholds_out[k] = hits[k] <= cap ? (uint64_t)1 << 32 : fastf_draw_threshold((float)((double)cap / (double)hits[k]));
    return 0;
}

float fastf_cap_realised(uint64_t sampled, uint64_t hits) { return hits ? (float)((double)sampled / (double)hits) : 1.0f; }

#define CAP_COLUMNS_TAIL "seed\tn_cells\ttotal_reads\tsampled_reads\tsampled_valid_reads\tnnz\tumis\tsaturation\t" \
    "median_umis_per_cell\tmedian_genes_per_cell\thits\tcells_capped\trealised_depth\n"
const char *fastf_cap_header(void) { return "rate_cell\treads_per_cell\t" CAP_COLUMNS_TAIL; }
const char *fastf_level_header(void) { return "rate_cell\tumi_cap\t" CAP_COLUMNS_TAIL; }

/* metrics: fastf_summary_tail_ */
int fastf_cap_row_(float rate_cell, uint64_t list_value, uint32_t seed, const uint64_t counters[3], uint64_t nnz, uint64_t umis,
                   const uint64_t *umis_per_cell, const uint32_t *genes_per_cell, uint32_t n_cells, uint64_t hits, uint32_t cells_capped,
                   char *buf, size_t cap, double *metrics)
{
    char tail[400];
    if (fastf_summary_tail_(seed, counters, nnz, umis, umis_per_cell, genes_per_cell, n_cells, tail, sizeof tail, metrics)) return 1;
    const int n = snprintf(buf, cap, "%.3f\t%llu\t%s\t%llu\t%u\t%.6f\n", (double)rate_cell, (unsigned long long)list_value, tail,
                           (unsigned long long)hits, cells_capped, (double)fastf_cap_realised(counters[1], hits));
    return (n < 0 || (size_t)n >= cap) ? fastf_res_err("summary row too long") : 0;
}
int fastf_cap_summary_row(float rate_cell, uint64_t reads_per_cell, uint32_t seed, const uint64_t counters[3], uint64_t nnz, uint64_t umis,
                          const uint64_t *umis_per_cell, const uint32_t *genes_per_cell, uint32_t n_cells, uint64_t hits, uint32_t cells_capped,
                          char *buf, size_t cap)
{
    return fastf_cap_row_(rate_cell, reads_per_cell, seed, counters, nnz, umis, umis_per_cell, genes_per_cell, n_cells, hits, cells_capped, buf, cap, NULL);
}

/* ------------------------------------------------------------------ */
/* the verb (resident.h: res_verb_t; the driver: grid_run.c)           */
/* ------------------------------------------------------------------ */
/* what a (cell rate, seed) pair keeps: ONE plane, made again for every cap; the hits per cell on the host; the thresholds on both sides */
typedef struct { void *d_plane, *d_hits, *d_thr; uint32_t *h_hits; uint64_t *h_thr; uint32_t capped; } cap_pair_t;

static void cap_pair_end(void *ctx)
{
    cap_pair_t *c = (cap_pair_t *)ctx;
    if (!c) return;
    fastf_devmem_free(c->d_plane); fastf_devmem_free(c->d_hits); fastf_devmem_free(c->d_thr);
    if (c->h_hits) fastf_pinned_free(c->h_hits);
    if (c->h_thr) fastf_pinned_free(c->h_thr);
    free(c);
}

/* the plane of the thresholds in c->h_thr */
static int cap_plane(cap_pair_t *c, const res_pair_t *p)
{
    const res_rate_t *S = p->S;
    return fastf_devmem_copy(c->d_thr, c->h_thr, (size_t)S->n_cells * 8) ||
           fastf_dev_cell_decisions(S->e, p->R->n, S->blocked ? S->buf.blk.p : NULL, p->seed, p->L->mt_skip, S->H, (const uint64_t *)c->d_thr, (uint32_t *)c->d_plane, NULL);
}

static int cap_pair_begin(const res_pair_t *p, void **ctx)
{
    res_rate_t *S = p->S;
    res_times_t *T = p->T;
    const uint64_t H = S->H;
    const uint32_t n_cells = S->n_cells;
    cap_pair_t *c = (cap_pair_t *)calloc(1, sizeof *c);
    if (!(*ctx = c)) return fastf_res_err("out of memory");
    double tt = fastf_res_now();

    /* the hits per cell, counted where K1a left the cell indices; to the host once, through pinned memory */
    const size_t nc1 = (size_t)n_cells + 1;
    const uint64_t plane_words = ((H + 63) / 64) * 2 + 64;      /* (zeroed slack behind the plane: K1b reads a unit's words unconditionally) */
    if (!(c->d_hits = fastf_devmem_alloc(p->device, nc1 * 4)) || !(c->d_thr = fastf_devmem_alloc(p->device, nc1 * 8)) ||
        !(c->h_hits = (uint32_t *)fastf_pinned_alloc(nc1 * 4)) || !(c->h_thr = (uint64_t *)fastf_pinned_alloc(nc1 * 8)) ||
        !(c->d_plane = fastf_devmem_alloc(p->device, (size_t)plane_words * 4)) || fastf_devmem_zero(c->d_plane, (size_t)plane_words * 4)) return RES_FAIL;
    if (fastf_dev_cell_hits(S->e, p->R->n, S->blocked ? S->buf.blk.p : NULL, (uint32_t *)c->d_hits, NULL) || fastf_devmem_sync() ||
        fastf_devmem_copy(c->h_hits, c->d_hits, (size_t)n_cells * 4)) return RES_FAIL;
    uint64_t sum = 0;
    for (uint32_t k = 0; k < n_cells; k++) sum += c->h_hits[k];
    if (sum != H) return fastf_res_err("internal error: %llu hits per cell in total, K1a counted %llu", (unsigned long long)sum, (unsigned long long)H);
    T->planes += fastf_res_now() - tt;
    if (!res_cfg_full(&S->cfg)) return RES_OK;
    tt = fastf_res_now();                                   /* the full rows of the pair, once: T = 2^32 for every cell */
    for (uint32_t k = 0; k < n_cells; k++) c->h_thr[k] = (uint64_t)1 << 32;
    if (cap_plane(c, p)) return RES_FAIL;
    *fastf_res_full_timer(S, T, 0) += fastf_res_now() - tt;
    return fastf_res_full_run(S, (const uint32_t *)c->d_plane, T);
}

static int cap_point_plane(void *ctx, const res_pair_t *p, uint32_t j, const char *point_name, const uint32_t **d_plane)
{
    cap_pair_t *c = (cap_pair_t *)ctx;
    const uint64_t cap = p->job->caps[j];
    const uint32_t n_cells = p->S->n_cells;
    (void)point_name;
    const double tt = fastf_res_now();
    if (fastf_cap_thresholds(c->h_hits, n_cells, cap, c->h_thr)) return RES_FAIL;
    c->capped = 0;
    for (uint32_t k = 0; k < n_cells; k++) c->capped += c->h_hits[k] > cap;
    if (cap_plane(c, p)) return RES_FAIL;
    p->T->planes += fastf_res_now() - tt;
    *d_plane = (const uint32_t *)c->d_plane;
    return RES_OK;
}

static int cap_point_row(void *ctx, const res_pair_t *p, uint32_t j, const uint64_t counters[3], uint64_t nnz, char *row, size_t cap, double *metrics)
{
    const res_rate_t *S = p->S;
    return fastf_cap_row_(p->rate_cell, p->job->caps[j], p->seed, counters, nnz, S->buf.h_upc.u64[S->n_cells], S->buf.h_upc.u64, S->buf.h_gpc.u32, S->n_cells, S->H,
                          ((const cap_pair_t *)ctx)->capped, row, cap, metrics);
}

static const res_verb_t cap_verb = {
    .name = "cap", .index = VERB_CAP, .header = fastf_cap_header,
    .check_caps = fastf_cap_check_grid, .caps_point_dir = fastf_cap_point_dir,
    .refusal_tail = ", and a cap has no point-by-point form",     /* (a global depth rate cannot express a cap) */
    .planes_words = "hits per cell + thresholds + planes", .fid_before = "", .fid_after = " full-depth points",
    .pair_begin = cap_pair_begin, .point_plane = cap_point_plane, .point_row = cap_point_row, .pair_end = cap_pair_end,
};

/* ------------------------------------------------------------------ */
/* the entry points, the command                                       */
/* ------------------------------------------------------------------ */
int fastf_cap(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
              const uint64_t *caps, uint32_t n_n, uint32_t seed, uint32_t flags)
{
    return fastf_res_grid_entry(&cap_verb, 0, bam, out_dir, barcodes, features, rates_cell, n_c, NULL, caps, n_n, NULL, 0, seed, flags, NULL, 0, 0, NULL);
}

/* seeds[]: 1 .. FASTF_MAX_SEEDS distinct values */
int fastf_cap_reps(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                   const uint64_t *caps, uint32_t n_n, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags)
{
    return fastf_res_grid_entry(&cap_verb, ENTRY_REPS, bam, out_dir, barcodes, features, rates_cell, n_c, NULL, caps, n_n, seeds, n_seeds, 0, flags, NULL, 0, 0, NULL);
}

/* n_seeds == 0: the one seed `seed`, no replicate run */
int fastf_cap_labels(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                     const uint64_t *caps, uint32_t n_n, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path)
{
    return fastf_res_grid_entry(&cap_verb, 0, bam, out_dir, barcodes, features, rates_cell, n_c, NULL, caps, n_n, seeds, n_seeds, seed, flags, labels_path, 0, 0, NULL);
}

/* --markers N: the labels run with the marker tables beside it; N and the labels path are checked always */
int fastf_cap_markers(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                      const uint64_t *caps, uint32_t n_n, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path,
                      uint32_t markers)
{
    return fastf_res_grid_entry(&cap_verb, ENTRY_MARKERS, bam, out_dir, barcodes, features, rates_cell, n_c, NULL, caps, n_n, seeds, n_seeds, seed, flags, labels_path, markers, 0, NULL);
}

/* --mapping: labels_path may be NULL and markers 0 */
int fastf_cap_mapping(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                      const uint64_t *caps, uint32_t n_n, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path,
                      uint32_t markers, uint32_t mapping)
{
    return fastf_res_grid_entry(&cap_verb, 0, bam, out_dir, barcodes, features, rates_cell, n_c, NULL, caps, n_n, seeds, n_seeds, seed, flags, labels_path, markers, mapping, NULL);
}

/* --pseudotime FILE, the most general call: labels_path and pseudotime_path may be NULL, markers and mapping 0 */
int fastf_cap_pseudotime(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                         const uint64_t *caps, uint32_t n_n, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path,
                         uint32_t markers, uint32_t mapping, const char *pseudotime_path)
{
    return fastf_res_grid_entry(&cap_verb, 0, bam, out_dir, barcodes, features, rates_cell, n_c, NULL, caps, n_n, seeds, n_seeds, seed, flags, labels_path, markers, mapping, pseudotime_path);
}

/* the command: what it does not share with the other two (resident.h: res_cmd_t) */
static const res_cmd_t cap_cmd = {
    .list_short = 'n', .list_long = "reads", .parse_caps = fastf_cap_parse_caps,
    .u_message = "cap does not write umi.tsv.gz (-u).", .needs_list = "cap needs -n <list>: the reads per cell at most",
    .help_intro = "every cell downsampled to at most N reads, over a grid of cell rates and caps from one decode of the bam file: per point\n"
                  "<out>/c<cell>_n<N>/ with the three files of bam2db, and <out>/cap.tsv with one summary row per point.",
    .help_list = "-n, --reads=<list>    reads per cell at most, comma separated integers >= 1",
    .help_point = "n<N>", .help_resident = "",
};
int cmd_cap(int argc, const char **argv) { return fastf_res_cmd(&cap_verb, &cap_cmd, argc, argv); }
