/*
 * sweep_cmds.c — `fastF sweep`: bam2db over a grid of (cell rate, depth rate) points from ONE decode of the BAM.
 *
 *   cmd_sweep()    the command the three verbs share (resident.c: fastf_res_cmd) with this verb's res_cmd_t: its list option -r <list>,
 *                  default 1, its -u message and its words of the help text
 *   fastf_sweep()  the same in process, and _reps, _labels, _markers, _mapping, _pseudotime: each ONE forwarding statement to
 *                  fastf_res_grid_entry (grid_run.c), which fills the job and runs the driver on this verb's res_verb_t
 * Per point <out>/c<rate_cell>_r<rate_depth>/{matrix.mtx.gz, barcodes.tsv.gz, features.tsv.gz} — the bytes `fastF bam2db`
 * writes for that point — and one row of <out>/sweep.tsv.
 *
 * Resident form (resident.c and the driver grid_run.c, shared with `fastF cap` and `fastF level`): the packed records (24 bytes each) stay in device memory.  Per cell rate one engine, the records in its
 * layout, K1a once; the draw stream generated once and compared against every depth threshold in the same pass
 * (fastf_dev_mt_decisions_multi); per depth rate K1b on that point's decision plane, sort, reduce, the per-cell summary
 * (fastf_dev_cell_summary), and — unless --summary-only — the rows gathered into pinned memory for the writers of bam2db.
 * Jobs this form does not cover (keys wider than 64 bits, UMIs beyond 16 bases, several devices) run point by point
 * through bam2db() itself, the summary then read back from each point's matrix.
 * --genes: per point the rows reduced along the gene axis too (fastf_dev_gene_summary; point by point fastf_sweep_genes_from_coo)
 * into sweep_genes.tsv, sweep_gene_cells.tsv.gz and the point's genes.tsv.gz (res_tables.c).
 * --cells: behind every point its keys sorted fully, K3u's rows and their reduction along the cell axis and into the copy-number
 * histogram (fastf_res_point_cells: fastf_dev_umi_rows, fastf_dev_copy_summary) into sweep_cells.tsv and the point's cells.tsv.gz;
 * resident form only — a job outside it is refused with the flag.
 * --fidelity: behind every open the pair's full-depth rows — one more decision plane, every hit kept — stay on the device
 * (fastf_res_full_run); behind every point its rows are joined with them (fastf_res_point_fidelity: fastf_dev_fidelity) into
 * sweep_fidelity.tsv and the point's fidelity.tsv.gz; resident form only, as --cells.
 * --gene-fidelity: the same pair of row sets per gene (fastf_res_point_gene_fidelity: fastf_dev_partner_counts, fastf_dev_gene_moments)
 * into sweep_gene_fidelity.tsv and the point's gene_fidelity.tsv.gz; it keeps the full rows by itself.
 * --neighbors: the k-nearest-neighbour sets of the cells over the pair's highly variable genes, at full depth and at the point
 * (fastf_res_point_neighbors: fastf_dev_neighbor_planes, fastf_dev_neighbors, fastf_dev_neighbors_shared) into sweep_neighbors.tsv and
 * the point's neighbors.tsv.gz; it keeps the full rows and ranks the genes by itself.
 * --labels FILE: the votes of those neighbour sets for the labels of the file (fastf_res_point_labels: fastf_dev_label_votes)
 * into sweep_labels.tsv, sweep_label_classes.tsv and the point's labels.tsv.gz and label_confusion.tsv.gz; it switches the neighbour sets
 * on by itself and writes no --neighbors file.
 * --coexpression: the co-expression partners of the genes of A, at full depth and at the point (fastf_res_point_coexpr:
 * fastf_dev_coexpr_sums, fastf_dev_coexpr_select, fastf_dev_neighbors_shared) into sweep_coexpr.tsv and the point's coexpr.tsv.gz; it
 * keeps the full rows and ranks the genes by itself, and computes nothing of the neighbour sets.
 * --seeds / --reps: the same records at several seeds — per cell rate every seed opens its own (cell rate, seed) pair on
 * the run's one res_rate_t (its buffers are handed on, the blocked copy laid out again only where the layout changes), the points
 * go to <point>_s<seed>/, and per grid point the metrics of the seeds are reduced into sweep_reps.tsv; with --genes the per-gene
 * arrays are summed across the seeds on the device (fastf_dev_gene_reps_add).
 */
#define _GNU_SOURCE
#include "resident.h"

#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

/* ------------------------------------------------------------------ */
/* the grid                                                            */
/* ------------------------------------------------------------------ */
/* "0.25,0.5,1" -> floats, each element parsed with strtof as bam2db parses its one value.  Refused: an empty list or element
 * (a trailing comma is one), trailing characters, out of range, NaN, negative; cell rates above 1 (fastf_sample_cells refuses them) */
int fastf_sweep_parse_rates(const char *text, int cell_rates, float *out, uint32_t cap, uint32_t *n_out)
{
    const char *what = cell_rates ? "cell" : "depth";
    uint32_t n = 0;
    if (n_out) *n_out = 0;
    if (!text || !out || !n_out) return fastf_res_err("null argument");
    for (const char *p = text;;) {
        const char *q = p;
        while (*q && *q != ',') q++;
        char el[64];
        const size_t len = (size_t)(q - p);
        if (len == 0) return fastf_res_err("%s rates `%s`: empty element", what, text);
        if (len >= sizeof el) return fastf_res_err("%s rates `%s`: element too long", what, text);
        memcpy(el, p, len); el[len] = '\0';
        char *end = NULL;
        errno = 0;
        const float v = strtof(el, &end);
        if (errno == ERANGE) return fastf_res_err("%s rate `%s`: numerical result out of range", what, el);
        if (end == el || *end) return fastf_res_err("%s rate `%s`: expects a numerical value", what, el);
        if (isnan(v)) return fastf_res_err("%s rate `%s`: not a number", what, el);
        if (v < 0 || signbit(v)) return fastf_res_err("%s rate `%s`: negative", what, el);
        if (cell_rates && v > 1.0f) return fastf_res_err("cell rate `%s`: sample size must lie in [0, number of barcodes]", el);
        if (n == cap) return fastf_res_err("%s rates `%s`: more than %u values", what, text, cap);
        out[n++] = v;
        if (!*q) break;
        p = q + 1;
    }
    *n_out = n;
    return 0;
}

int fastf_sweep_point_dir(float rate_cell, float rate_depth, char *buf, size_t cap)
{
    const int n = snprintf(buf, cap, "c%.3f_r%.3f", (double)rate_cell, (double)rate_depth);
    return (n < 0 || (size_t)n >= cap) ? fastf_res_err("directory name too long") : 0;
}

/* two values of one list that print the same at %.3f would share their directories and header lines */
int fastf_sweep_check_grid(const float *rates_cell, uint32_t n_c, const float *rates_depth, uint32_t n_r)
{
    if (!n_c || !n_r || !rates_cell || !rates_depth) return fastf_res_err("sweep: the grid needs at least one cell rate and one depth rate");
    for (int pass = 0; pass < 2; pass++) {
        const float *v = pass ? rates_depth : rates_cell;
        const uint32_t n = pass ? n_r : n_c;
        for (uint32_t i = 0; i < n; i++) {
            if (isnan(v[i]) || v[i] < 0) return fastf_res_err("sweep: %s rate %g is negative or not a number", pass ? "depth" : "cell", (double)v[i]);
            if (!pass && v[i] > 1.0f) return fastf_res_err("sweep: cell rate %g: sample size must lie in [0, number of barcodes]", (double)v[i]);
            char a[32], b[32];
            snprintf(a, sizeof a, "%.3f", (double)v[i]);
            for (uint32_t j = 0; j < i; j++) {
                snprintf(b, sizeof b, "%.3f", (double)v[j]);
                if (!strcmp(a, b)) return fastf_res_err("sweep: %s rates %g and %g both print as %s", pass ? "depth" : "cell", (double)v[j], (double)v[i], a);
            }
        }
    }
    return 0;
}

/* ------------------------------------------------------------------ */
/* point by point through bam2db()                                     */
/* ------------------------------------------------------------------ */
/* counters, dimensions and rows of a matrix.mtx.gz bam2db() wrote */
static int read_matrix(const char *path, uint64_t counters[3], uint32_t *n_features, uint32_t *n_cells, fastf_coo_t *coo, uint32_t **rows_out)
{
    gzFile g = gzopen(path, "rb");
    if (!g) return fastf_res_err("cannot read %s back", path);
    char line[8192];
    int rc = 1, have_dims = 0;
    size_t nnz = 0, at = 0;
    uint32_t *rows = NULL;
    memset(counters, 0, 3 * sizeof counters[0]);
    while (gzgets(g, line, sizeof line)) {
        if (line[0] == '%') {
            unsigned long long v;
            if (sscanf(line, "%%\t\"total_n_FastQ\": %llu", &v) == 1) counters[0] = v;
            else if (sscanf(line, "%%\t\"sampled_n_FastQ\": %llu", &v) == 1) counters[1] = v;
            else if (sscanf(line, "%%\t\"sampled_valid_n_FastQ\": %llu", &v) == 1) counters[2] = v;
            continue;
        }
        if (!have_dims) {
            size_t nf, nb;
            if (sscanf(line, "%zu %zu %zu", &nf, &nb, &nnz) != 3) { fastf_res_err("%s: no dimension line", path); goto done; }
            *n_features = (uint32_t)nf; *n_cells = (uint32_t)nb;
            rows = (uint32_t *)malloc((nnz ? nnz : 1) * 12);
            if (!rows) { fastf_res_err("out of memory"); goto done; }
            have_dims = 1;
            continue;
        }
        unsigned f, c, k;
        if (at >= nnz || sscanf(line, "%u %u %u", &f, &c, &k) != 3) { fastf_res_err("%s: malformed row", path); goto done; }
        rows[at] = f; rows[nnz + at] = c; rows[2 * nnz + at] = k; at++;
    }
    if (!have_dims || at != nnz) { fastf_res_err("%s: %zu rows of %zu", path, at, nnz); goto done; }
    coo->feature = rows; coo->cell = rows + nnz; coo->count = rows + 2 * nnz; coo->nnz = nnz;
    *rows_out = rows; rows = NULL;
    rc = 0;
done:
    free(rows);
    gzclose(g);
    return rc;
}

/* the hook of a job outside the resident form (res_verb_t.point_by_point) */
static int sweep_point_by_point(const res_job_t *job, int summary_only, res_tables_t *tb)
{
    const char *bam = job->bam, *out_dir = job->out_dir, *barcodes = job->barcodes, *features = job->features;
    const float *rc_list = job->rates_cell, *rd_list = job->rates_depth;
    const uint32_t n_c = job->n_c, n_r = job->n_list, n_s = job->n_s, *seeds = job->seeds;
    res_tsv_t *tsv = &tb->tsv; res_genes_t *G = &tb->G; res_reps_t *P = &tb->P;
    const int saved_u = _umi_copies_flag;
    _umi_copies_flag = 0;
    int rc = 1;
    fastf_lists_t GL; memset(&GL, 0, sizeof GL);           /* --genes: the feature names (bam2db() loads its own lists) */
    if (G->on && fastf_lists_load(barcodes, features, 1.0f, seeds[0], &GL)) goto done;
    for (uint32_t i = 0; i < n_c; i++) {
      if (fastf_res_reps_rate_begin(P, &GL, 0)) goto done;
      for (uint32_t k = 0; k < n_s; k++)
        for (uint32_t j = 0; j < n_r; j++) {
            char base[64], name[96], dir[4096], path[4200];
            const uint32_t seed = seeds[k];
            double metrics[FASTF_REPS_METRICS];
            if (fastf_sweep_point_dir(rc_list[i], rd_list[j], base, sizeof base)) goto done;
            if (P->on ? fastf_reps_point_dir(base, seed, name, sizeof name) : (snprintf(name, sizeof name, "%s", base), 0)) goto done;
            if (summary_only) snprintf(dir, sizeof dir, "%s/.%s.partial", out_dir, name);      /* (removed again below) */
            else snprintf(dir, sizeof dir, "%s/%s", out_dir, name);
            if (fastf_res_make_dir(dir)) goto done;
            const int brc = bam2db((char *)bam, NULL, dir, (char *)barcodes, (char *)features, rc_list[i], rd_list[j], seed);
            uint64_t counters[3]; uint32_t n_features = 0, n_cells = 0; fastf_coo_t coo; uint32_t *rows = NULL;
            snprintf(path, sizeof path, "%s/matrix.mtx.gz", dir);
            int prc = brc ? 1 : read_matrix(path, counters, &n_features, &n_cells, &coo, &rows);
            if (summary_only) {
                static const char *const files[] = {"matrix.mtx.gz", "barcodes.tsv.gz", "features.tsv.gz"};
                for (int k = 0; k < 3; k++) { snprintf(path, sizeof path, "%s/%s", dir, files[k]); unlink(path); }
                rmdir(dir);
            }
            if (brc) { if (!strstr(fastf_last_error(), "bam2db")) fastf_res_err("bam2db failed at point %s: %s", name, fastf_last_error()); goto done; }
            if (prc) goto done;
            uint64_t *upc = (uint64_t *)calloc((size_t)n_cells + 1, sizeof *upc);
            uint32_t *gpc = (uint32_t *)calloc((size_t)n_cells + 1, sizeof *gpc);
            uint64_t umis = 0;
            char row[512];
            prc = !upc || !gpc || fastf_sweep_cells_from_coo(&coo, n_cells, upc, gpc, &umis) ||
                  fastf_sweep_row_(rc_list[i], rd_list[j], seed, counters, coo.nnz, umis, upc, gpc, n_cells, row, sizeof row, metrics) ||
                  fastf_res_reps_point(P, j, k, n_cells, metrics);
            free(upc); free(gpc);
            if (!prc && G->on) {
                char grow[256];
                uint32_t *cpg = (uint32_t *)calloc((size_t)n_features + 1, sizeof *cpg);
                uint64_t *upg = (uint64_t *)calloc((size_t)n_features + 1, sizeof *upg);
                prc = !cpg || !upg || (n_features != GL.n_features && fastf_res_err("%s names %u features, the list has %zu", name, n_features, GL.n_features)) ||
                      fastf_sweep_genes_from_coo(&coo, n_features, cpg, upg) ||
                      fastf_genes_summary_row(rc_list[i], rd_list[j], 0, seed, cpg, upg, n_features, grow, sizeof grow) ||
                      fastf_res_genes_point(G, &GL, name, summary_only ? NULL : dir, grow, cpg, upg) ||
                      fastf_res_reps_genes(P, NULL, j, k, cpg, n_features);
                free(cpg); free(upg);
            }
            free(rows);
            if (prc) goto done;
            fputs(row, tsv->f);
        }
      if (fastf_res_reps_rate_end(P, rc_list[i], rd_list, NULL, NULL)) goto done;
    }
    rc = 0;
done:
    if (G->on) fastf_lists_free(&GL);
    _umi_copies_flag = saved_u;
    return rc;
}

/* ------------------------------------------------------------------ */
/* the verb (resident.h: res_verb_t; the driver: grid_run.c)           */
/* ------------------------------------------------------------------ */
/* what a (cell rate, seed) pair keeps: every plane of the pair, plane_words apart, and the thresholds they were made from */
typedef struct { void *d_planes; uint64_t *thr; uint64_t plane_words; } sweep_pair_t;

static void sweep_pair_end(void *ctx)
{
    sweep_pair_t *c = (sweep_pair_t *)ctx;
    if (!c) return;
    fastf_devmem_free(c->d_planes);
    free(c->thr); free(c);
}

/* the decision planes: the draw stream once, every threshold in the same pass */
static int sweep_pair_begin(const res_pair_t *p, void **ctx)
{
    res_rate_t *S = p->S;
    const uint32_t n_r = p->job->n_list;
    const uint32_t n_planes = n_r + (res_cfg_full(&S->cfg) ? 1u : 0u);   /* --fidelity, --gene-fidelity: one more plane behind the grid's, every hit kept */
    sweep_pair_t *c = (sweep_pair_t *)calloc(1, sizeof *c);
    if (!(*ctx = c) || !(c->thr = (uint64_t *)malloc(n_planes * sizeof *c->thr))) return fastf_res_err("out of memory");
    const double tt = fastf_res_now();
    c->plane_words = ((S->H + 63) / 64) * 2 + 64;           /* (zeroed slack behind each plane: K1b reads a unit's words unconditionally) */
    if (!(c->d_planes = fastf_devmem_alloc(p->device, (size_t)n_planes * c->plane_words * 4)) || fastf_devmem_zero(c->d_planes, (size_t)n_planes * c->plane_words * 4)) return RES_FAIL;
    for (uint32_t j = 0; j < n_r; j++) c->thr[j] = fastf_draw_threshold(p->job->rates_depth[j]);
    if (res_cfg_full(&S->cfg)) c->thr[n_r] = (uint64_t)1 << 32;
    if (fastf_dev_mt_decisions_multi(S->e, p->seed, p->L->mt_skip, S->H, c->thr, n_planes, (uint32_t *)c->d_planes, c->plane_words, NULL)) return RES_FAIL;
    p->T->planes += fastf_res_now() - tt;
    /* the full rows of the pair, once */
    return res_cfg_full(&S->cfg) ? fastf_res_full_run(S, (const uint32_t *)c->d_planes + (size_t)n_r * c->plane_words, p->T) : RES_OK;
}

static int sweep_point_plane(void *ctx, const res_pair_t *p, uint32_t j, const char *point_name, const uint32_t **d_plane)
{
    const sweep_pair_t *c = (const sweep_pair_t *)ctx;
    (void)p; (void)point_name;
    *d_plane = (const uint32_t *)c->d_planes + (size_t)j * c->plane_words;
    return RES_OK;
}

static int sweep_point_row(void *ctx, const res_pair_t *p, uint32_t j, const uint64_t counters[3], uint64_t nnz, char *row, size_t cap, double *metrics)
{
    const res_rate_t *S = p->S;
    (void)ctx;
    return fastf_sweep_row_(p->rate_cell, p->job->rates_depth[j], p->seed, counters, nnz, S->buf.h_upc.u64[S->n_cells], S->buf.h_upc.u64, S->buf.h_gpc.u32, S->n_cells, row, cap, metrics);
}

static const res_verb_t sweep_verb = {
    .name = "sweep", .index = VERB_SWEEP, .header = fastf_sweep_header,
    .planes_words = "planes", .fid_before = "", .fid_after = " full-depth points",
    .pair_begin = sweep_pair_begin, .point_plane = sweep_point_plane, .point_row = sweep_point_row, .pair_end = sweep_pair_end,
    .point_by_point = sweep_point_by_point,
};

/* ------------------------------------------------------------------ */
/* the entry points, the command                                       */
/* ------------------------------------------------------------------ */
int fastf_sweep(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                const float *rates_depth, uint32_t n_r, uint32_t seed, uint32_t flags)
{
    return fastf_res_grid_entry(&sweep_verb, 0, bam, out_dir, barcodes, features, rates_cell, n_c, rates_depth, NULL, n_r, NULL, 0, seed, flags, NULL, 0, 0, NULL);
}

/* seeds[]: 1 .. FASTF_MAX_SEEDS distinct values */
int fastf_sweep_reps(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                     const float *rates_depth, uint32_t n_r, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags)
{
    return fastf_res_grid_entry(&sweep_verb, ENTRY_REPS, bam, out_dir, barcodes, features, rates_cell, n_c, rates_depth, NULL, n_r, seeds, n_seeds, 0, flags, NULL, 0, 0, NULL);
}

/* n_seeds == 0: the one seed `seed`, no replicate run */
int fastf_sweep_labels(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                       const float *rates_depth, uint32_t n_r, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path)
{
    return fastf_res_grid_entry(&sweep_verb, 0, bam, out_dir, barcodes, features, rates_cell, n_c, rates_depth, NULL, n_r, seeds, n_seeds, seed, flags, labels_path, 0, 0, NULL);
}

/* --markers N: the labels run with the marker tables beside it; N and the labels path are checked always */
int fastf_sweep_markers(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                        const float *rates_depth, uint32_t n_r, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path,
                        uint32_t markers)
{
    return fastf_res_grid_entry(&sweep_verb, ENTRY_MARKERS, bam, out_dir, barcodes, features, rates_cell, n_c, rates_depth, NULL, n_r, seeds, n_seeds, seed, flags, labels_path, markers, 0, NULL);
}

/* --mapping: labels_path may be NULL and markers 0 */
int fastf_sweep_mapping(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                        const float *rates_depth, uint32_t n_r, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path,
                        uint32_t markers, uint32_t mapping)
{
    return fastf_res_grid_entry(&sweep_verb, 0, bam, out_dir, barcodes, features, rates_cell, n_c, rates_depth, NULL, n_r, seeds, n_seeds, seed, flags, labels_path, markers, mapping, NULL);
}

/* --pseudotime FILE, the most general call: labels_path and pseudotime_path may be NULL, markers and mapping 0 */
int fastf_sweep_pseudotime(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                           const float *rates_depth, uint32_t n_r, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path,
                           uint32_t markers, uint32_t mapping, const char *pseudotime_path)
{
    return fastf_res_grid_entry(&sweep_verb, 0, bam, out_dir, barcodes, features, rates_cell, n_c, rates_depth, NULL, n_r, seeds, n_seeds, seed, flags, labels_path, markers, mapping, pseudotime_path);
}

/* the command: what it does not share with the other two (resident.h: res_cmd_t) */
static const res_cmd_t sweep_cmd = {
    .list_short = 'r', .list_long = "depth", .list_default = "1",
    .u_message = "sweep does not write umi.tsv.gz (-u): run bam2db -u for the points that need it.",
    .help_intro = "bam2db over a grid of cell and depth rates from one decode of the bam file: per point <out>/c<cell>_r<depth>/ with the\n"
                  "three files of bam2db, and <out>/sweep.tsv with one summary row per point.",
    .help_list = "-r, --depth=<list>    rates of depth, comma separated (default 1.0)",
    .help_point = "r<depth>", .help_resident = "; resident form only",
};
int cmd_sweep(int argc, const char **argv) { return fastf_res_cmd(&sweep_verb, &sweep_cmd, argc, argv); }
