/*
 * level_cmds.c — `fastF level`: every cell downsampled to at most M UMIs, exactly, over a grid of (cell rate, UMI cap) points from
 * ONE decode of the BAM.
 *
 *   cmd_level()    the command the three verbs share (resident.c: fastf_res_cmd) with this verb's res_cmd_t: its list option -m <list>,
 *                  which has no default, its -u message and its words of the help text
 *   fastf_level()  the same in process, and _reps, _labels, _markers, _mapping, _pseudotime: each ONE forwarding statement to
 *                  fastf_res_grid_entry (grid_run.c), as sweep's (sweep_cmds.c)
 * Per point <out>/c<rate_cell>_m<M>/{matrix.mtx.gz, barcodes.tsv.gz, features.tsv.gz, thresholds.tsv.gz} and one row of <out>/level.tsv.
 *
 * The resident pipeline of sweep and cap (resident.c), and cap's coupling: hit i owns draw i and is kept iff draw[i] < T[cell].  The
 * kept sets of a cell are nested in T, so its UMI count U_k(T) is a non-decreasing step function and T[k] = max { T : U_k(T) <= M } is
 * found by bisection — for all cells at once, one pass of the point's device half per step (fastf_res_search_pass): pass 0 keeps
 * every hit and gives U_k(2^32), once per (cell rate, seed); per cap up to 32 probing passes, in which a cell that is settled is
 * probed at 0 and drops out of K1b's output; then the point itself with T = lo through the unchanged fastf_res_point_run.  The state
 * lives on the device (level_kernels.hpp); a pass ends in one small copy to the host.  Jobs outside the resident form are refused
 * as cap refuses them.  --genes, --cells and the replicate tables: as in cap, under the names level_*.
 */
#define _GNU_SOURCE
#include "resident.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

/* a message of cap's list rules, speaking of this verb's list */
static int lv_from_cap(void)
{
    char keep[400], out[480]; snprintf(keep, sizeof keep, "%s", fastf_last_error());
    const char *p = keep;
    if (!strncmp(p, "cap: ", 5)) p += 5;
    if (!strncmp(p, "reads per cell", 14)) snprintf(out, sizeof out, "level: UMIs per cell%s", p + 14);
    else snprintf(out, sizeof out, "level: %s", p);
    fastf_set_error_(out);
    return 1;
}

/* ------------------------------------------------------------------ */
/* the grid, the names, the headers, the summary row                   */
/* ------------------------------------------------------------------ */
int fastf_level_parse_caps(const char *text, uint64_t *out, uint32_t cap, uint32_t *n_out)
{
    return fastf_cap_parse_caps(text, out, cap, n_out) ? lv_from_cap() : 0;      /* the list rules are cap's */
}

int fastf_level_check_grid(const float *rates_cell, uint32_t n_c, const uint64_t *caps, uint32_t n_m)
{
    return fastf_cap_check_grid(rates_cell, n_c, caps, n_m) ? lv_from_cap() : 0;
}

int fastf_level_point_dir(float rate_cell, uint64_t umi_cap, char *buf, size_t cap)
{
    const int n = snprintf(buf, cap, "c%.3f_m%llu", (double)rate_cell, (unsigned long long)umi_cap);
    return (n < 0 || (size_t)n >= cap) ? fastf_res_err("directory name too long") : 0;
}

/* level.tsv has cap.tsv's columns, its second named umi_cap (the headers: beside cap's) */
int fastf_level_summary_row(float rate_cell, uint64_t umi_cap, uint32_t seed, const uint64_t counters[3], uint64_t nnz, uint64_t umis,
                            const uint64_t *umis_per_cell, const uint32_t *genes_per_cell, uint32_t n_cells, uint64_t hits, uint32_t cells_capped,
                            char *buf, size_t cap)
{
    return fastf_cap_row_(rate_cell, umi_cap, seed, counters, nnz, umis, umis_per_cell, genes_per_cell, n_cells, hits, cells_capped, buf, cap, NULL);
}

/* ------------------------------------------------------------------ */
/* <point dir>/thresholds.tsv.gz                                       */
/* ------------------------------------------------------------------ */
static int write_thresholds(const char *dir, const fastf_lists_t *L, uint32_t n_cells, const uint64_t *thr, const uint64_t *umis_full, const uint64_t *umis)
{
    gtext t = { NULL, 0, 0 };
    int bad = fastf_gt_str(&t, "barcode\tthreshold\tumis_full\tumis\n");
    for (uint32_t k = 0; k < n_cells && !bad; k++)
        bad = fastf_gt_str(&t, L->barcode[k]) || fastf_gt_u64(&t, '\t', thr[k]) || fastf_gt_u64(&t, '\t', umis_full[k]) || fastf_gt_u64(&t, '\t', umis[k]) || fastf_gt_str(&t, "\n");
    return fastf_res_text_file(dir, "thresholds.tsv.gz", &t, bad);
}

/* ------------------------------------------------------------------ */
/* the verb (resident.h: res_verb_t; the driver: grid_run.c)           */
/* ------------------------------------------------------------------ */
#define LEVEL_MAX_PASSES 32u                             /* hi - lo halves per probing pass, from 2^32 */
/* what a (cell rate, seed) pair keeps: ONE plane, made again for every pass; the state of the search (on the device: S->lv.lo ..);
 * of the point in work its probing passes and where the clocks stood before them */
typedef struct { void *d_plane; uint64_t *h_thr, *h_ufull; uint64_t open, capped; uint32_t passes; double search0, device0; } level_pair_t;

static void level_pair_end(void *ctx)
{
    level_pair_t *c = (level_pair_t *)ctx;
    if (!c) return;
    fastf_devmem_free(c->d_plane);
    if (c->h_thr) fastf_pinned_free(c->h_thr);
    if (c->h_ufull) fastf_pinned_free(c->h_ufull);
    free(c);
}

/* the plane of the thresholds thr (on the device) */
static int level_plane(level_pair_t *c, const res_pair_t *p, const uint64_t *thr)
{
    const res_rate_t *S = p->S;
    return fastf_dev_cell_decisions(S->e, p->R->n, S->blocked ? S->buf.blk.p : NULL, p->seed, p->L->mt_skip, S->H, thr, (uint32_t *)c->d_plane, NULL);
}

static int level_pair_begin(const res_pair_t *p, void **ctx)
{
    res_rate_t *S = p->S;
    res_times_t *T = p->T;
    const uint32_t n_cells = S->n_cells;
    level_pair_t *c = (level_pair_t *)calloc(1, sizeof *c);
    if (!(*ctx = c)) return fastf_res_err("out of memory");
    double tt = fastf_res_now();
    const size_t nc1 = (size_t)n_cells + 1;
    const uint64_t plane_words = ((S->H + 63) / 64) * 2 + 64;   /* (zeroed slack behind the plane: K1b reads a unit's words unconditionally) */
    if (fastf_res_level_room(S)) return RES_FAIL;
    if (!(c->h_thr = (uint64_t *)fastf_pinned_alloc(nc1 * 8)) || (!p->summary_only && !(c->h_ufull = (uint64_t *)fastf_pinned_alloc(nc1 * 8))) ||
        !(c->d_plane = fastf_devmem_alloc(p->device, (size_t)plane_words * 4)) || fastf_devmem_zero(c->d_plane, (size_t)plane_words * 4)) return RES_FAIL;
    T->planes += fastf_res_now() - tt;

    /* pass 0: every hit kept.  U_k(2^32) stays on the device for every cap of the list; the state of the first cap comes with it */
    tt = fastf_res_now();
    for (uint32_t k = 0; k < n_cells; k++) c->h_thr[k] = (uint64_t)1 << 32;
    if (fastf_devmem_copy(S->lv.probe, c->h_thr, (size_t)n_cells * 8) || level_plane(c, p, S->lv.probe)) return RES_FAIL;
    T->search += fastf_res_now() - tt;
    char name0[64]; snprintf(name0, sizeof name0, "c%.3f (every hit)", (double)p->rate_cell);
    const int prc = fastf_res_search_pass(S, (const uint32_t *)c->d_plane, name0, p->job->caps[0], 1, &c->open, &c->capped, T);
    if (prc != RES_OK) return prc;
    if (fastf_res_full_keep(S, T)) return RES_FAIL;         /* --fidelity: pass 0's rows are the full rows of the pair */
    if (c->h_ufull && fastf_devmem_copy(c->h_ufull, S->lv.ufull, (size_t)n_cells * 8)) return RES_FAIL;
    return RES_OK;
}

static int level_point_plane(void *ctx, const res_pair_t *p, uint32_t j, const char *point_name, const uint32_t **d_plane)
{
    level_pair_t *c = (level_pair_t *)ctx;
    res_rate_t *S = p->S;
    res_times_t *T = p->T;
    const uint64_t umi_cap = p->job->caps[j];
    c->search0 = T->search; c->device0 = T->device; c->passes = 0;
    if (j) { const int irc = fastf_res_level_init(S, umi_cap, &c->open, &c->capped, T); if (irc != RES_OK) return irc; }
    while (c->open) {                                       /* open cells are probed at (lo + hi) / 2, every other cell at 0 */
        if (c->passes == LEVEL_MAX_PASSES)
            return fastf_res_err("internal error: %llu cells still open after %u passes at point %s", (unsigned long long)c->open, c->passes, point_name);
        const double tt = fastf_res_now();
        if (level_plane(c, p, S->lv.probe)) return RES_FAIL;
        T->search += fastf_res_now() - tt;
        const int prc = fastf_res_search_pass(S, (const uint32_t *)c->d_plane, point_name, umi_cap, 0, &c->open, NULL, T);
        if (prc != RES_OK) return prc;
        c->passes++;
    }
    /* the point: T = lo */
    const double tt = fastf_res_now();
    if (level_plane(c, p, S->lv.lo)) return RES_FAIL;
    T->planes += fastf_res_now() - tt;
    *d_plane = (const uint32_t *)c->d_plane;
    return RES_OK;
}

static void level_point_done(void *ctx, const res_pair_t *p, const char *point_name)
{
    const level_pair_t *c = (const level_pair_t *)ctx;
    if (p->prof) fprintf(stderr, "[level] point %s: %u probing passes, search %.4f s, the point's own pass %.4f s\n", point_name, c->passes, p->T->search - c->search0, p->T->device - c->device0);
}

static int level_point_row(void *ctx, const res_pair_t *p, uint32_t j, const uint64_t counters[3], uint64_t nnz, char *row, size_t cap, double *metrics)
{
    const res_rate_t *S = p->S;
    return fastf_cap_row_(p->rate_cell, p->job->caps[j], p->seed, counters, nnz, S->buf.h_upc.u64[S->n_cells], S->buf.h_upc.u64, S->buf.h_gpc.u32, S->n_cells, S->H,
                          (uint32_t)((const level_pair_t *)ctx)->capped, row, cap, metrics);
}

static int level_point_files(void *ctx, const res_pair_t *p, const char *dir)
{
    level_pair_t *c = (level_pair_t *)ctx;
    const res_rate_t *S = p->S;
    const double tt = fastf_res_now();
    if (fastf_devmem_copy(c->h_thr, S->lv.lo, (size_t)S->n_cells * 8) || write_thresholds(dir, p->L, S->n_cells, c->h_thr, c->h_ufull, S->buf.h_upc.u64)) return 1;
    p->T->write += fastf_res_now() - tt;
    return 0;
}

static void level_run_profile(const res_job_t *job, const res_times_t *T)
{
    const uint32_t pairs = job->n_c * job->n_s, points = pairs * job->n_list;
    fprintf(stderr, "[level] search: %u passes in all (%u with every hit kept, one per cell rate and seed; %.1f probing passes a point), %.3f s "
                    "(%.4f s a point, %.4f s a pass with its plane and step)\n",
            T->passes, pairs, (double)(T->passes - pairs) / points, T->search, T->search / points, T->passes ? T->search / T->passes : 0.0);
}

static const res_verb_t level_verb = {
    .name = "level", .index = VERB_LEVEL, .header = fastf_level_header,
    .check_caps = fastf_level_check_grid, .caps_point_dir = fastf_level_point_dir,
    .refusal_tail = ", and a UMI cap has no point-by-point form",
    .planes_words = "planes of the points", .fid_before = "the full rows kept from ", .fid_after = " first passes",
    .unlink_reps_always = 1,
    .pair_begin = level_pair_begin, .point_plane = level_point_plane, .point_done = level_point_done, .point_row = level_point_row,
    .point_files = level_point_files, .pair_end = level_pair_end, .run_profile = level_run_profile,
};

/* ------------------------------------------------------------------ */
/* the entry points, the command                                       */
/* ------------------------------------------------------------------ */
int fastf_level(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                const uint64_t *umi_caps, uint32_t n_m, uint32_t seed, uint32_t flags)
{
    return fastf_res_grid_entry(&level_verb, 0, bam, out_dir, barcodes, features, rates_cell, n_c, NULL, umi_caps, n_m, NULL, 0, seed, flags, NULL, 0, 0, NULL);
}

/* seeds[]: 1 .. FASTF_MAX_SEEDS distinct values */
int fastf_level_reps(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                     const uint64_t *umi_caps, uint32_t n_m, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags)
{
    return fastf_res_grid_entry(&level_verb, ENTRY_REPS, bam, out_dir, barcodes, features, rates_cell, n_c, NULL, umi_caps, n_m, seeds, n_seeds, 0, flags, NULL, 0, 0, NULL);
}

/* n_seeds == 0: the one seed `seed`, no replicate run */
int fastf_level_labels(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                       const uint64_t *umi_caps, uint32_t n_m, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path)
{
    return fastf_res_grid_entry(&level_verb, 0, bam, out_dir, barcodes, features, rates_cell, n_c, NULL, umi_caps, n_m, seeds, n_seeds, seed, flags, labels_path, 0, 0, NULL);
}

/* --markers N: the labels run with the marker tables beside it; N and the labels path are checked always */
int fastf_level_markers(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                        const uint64_t *umi_caps, uint32_t n_m, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path,
                        uint32_t markers)
{
    return fastf_res_grid_entry(&level_verb, ENTRY_MARKERS, bam, out_dir, barcodes, features, rates_cell, n_c, NULL, umi_caps, n_m, seeds, n_seeds, seed, flags, labels_path, markers, 0, NULL);
}

/* --mapping: labels_path may be NULL and markers 0 */
int fastf_level_mapping(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                        const uint64_t *umi_caps, uint32_t n_m, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path,
                        uint32_t markers, uint32_t mapping)
{
    return fastf_res_grid_entry(&level_verb, 0, bam, out_dir, barcodes, features, rates_cell, n_c, NULL, umi_caps, n_m, seeds, n_seeds, seed, flags, labels_path, markers, mapping, NULL);
}

/* --pseudotime FILE, the most general call: labels_path and pseudotime_path may be NULL, markers and mapping 0 */
int fastf_level_pseudotime(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                           const uint64_t *umi_caps, uint32_t n_m, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path,
                           uint32_t markers, uint32_t mapping, const char *pseudotime_path)
{
    return fastf_res_grid_entry(&level_verb, 0, bam, out_dir, barcodes, features, rates_cell, n_c, NULL, umi_caps, n_m, seeds, n_seeds, seed, flags, labels_path, markers, mapping, pseudotime_path);
}

/* the command: what it does not share with the other two (resident.h: res_cmd_t) */
static const res_cmd_t level_cmd = {
    .list_short = 'm', .list_long = "umis", .parse_caps = fastf_level_parse_caps,
    .u_message = "level does not write umi.tsv.gz (-u).", .needs_list = "level needs -m <list>: the UMIs per cell at most",
    .help_intro = "every cell downsampled to at most M UMIs, exactly: the deepest read-level subsample of each cell whose UMI count does not\n"
                  "exceed M, over a grid of cell rates and UMI caps from one decode of the bam file: per point <out>/c<cell>_m<M>/ with the three\n"
                  "files of bam2db and thresholds.tsv.gz, and <out>/level.tsv with one summary row per point.",
    .help_list = "-m, --umis=<list>     UMIs per cell at most, comma separated integers >= 1",
    .help_point = "m<M>", .help_resident = "",
};
int cmd_level(int argc, const char **argv) { return fastf_res_cmd(&level_verb, &level_cmd, argc, argv); }
