/*
 * res_tables.c — every table and point file of a run of `fastF sweep`, `fastF cap` and `fastF level` (resident.h): the summary table
 * through .partial, the --genes and --cells tables, and the comparisons against full depth (res_cmp_t) behind ONE descriptor array —
 * one open, one point function and one close loop over it.  The point files go through one file helper (fastf_res_text_file) and,
 * where they are a header and n lines, one line loop (flat_file).  Host code alone: the arrays come from the host views of a
 * res_rate_t, so the file links into a CPU program with grid_rows.c and the writers of host_io.c.
 */
#define _GNU_SOURCE
#include "resident.h"

#include <errno.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

double fastf_res_now(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + t.tv_nsec * 1e-9; }
int fastf_res_make_dir(const char *path)
{
    if (mkdir(path, 0777) == 0 || errno == EEXIST) return 0;
    return fastf_res_err("cannot create directory %s: %s", path, strerror(errno));
}

/* ------------------------------------------------------------------ */
/* a table through .partial                                            */
/* ------------------------------------------------------------------ */
int fastf_res_tsv_open(res_tsv_t *t, const char *out_dir, const char *name, const char *header)
{
    snprintf(t->final, sizeof t->final, "%s/%s", out_dir, name);
    snprintf(t->tmp, sizeof t->tmp, "%s/%s.partial", out_dir, name);
    if (!(t->f = fopen(t->tmp, "w"))) return fastf_res_err("cannot open %s: %s", t->tmp, strerror(errno));
    fputs(header, t->f);
    return 0;
}
int fastf_res_table_open(res_tsv_t *t, const res_verb_t *V, const char *out_dir, int table)
{
    char name[64];
    snprintf(name, sizeof name, "%s_%s.tsv", V->name, fastf_res_table_stem(table));
    return fastf_res_tsv_open(t, out_dir, name, fastf_res_table_header(V->index, table));
}
int fastf_res_tsv_close(res_tsv_t *t, int ok)
{
    if (!t->f) return 0;
    const int bad = ferror(t->f) | (fclose(t->f) != 0);
    t->f = NULL;
    if (ok && !bad && rename(t->tmp, t->final) == 0) return 0;
    unlink(t->tmp);
    return ok ? fastf_res_err("cannot write %s", t->final) : 0;
}

/* ------------------------------------------------------------------ */
/* the text of a point file, the file                                  */
/* ------------------------------------------------------------------ */
static int gt_room(gtext *t, size_t more)
{
    if (t->len + more <= t->cap) return 0;
    size_t cap = t->cap ? t->cap : ((size_t)1 << 16);
    while (cap < t->len + more) cap *= 2;
    char *np = (char *)realloc(t->p, cap);
    if (!np) return fastf_res_err("out of memory");
    t->p = np; t->cap = cap;
    return 0;
}
int fastf_gt_str(gtext *t, const char *s) { const size_t n = strlen(s); if (!n) return 0; if (gt_room(t, n)) return 1; memcpy(t->p + t->len, s, n); t->len += n; return 0; }
int fastf_gt_u64(gtext *t, char lead, uint64_t v)
{
    if (gt_room(t, 24)) return 1;
    t->len += (size_t)snprintf(t->p + t->len, 24, "%c%llu", lead, (unsigned long long)v);
    return 0;
}

int fastf_res_text_file(const char *dir, const char *name, gtext *t, int bad)
{
    if (!bad) {
        char path[4200], tmp[4300];
        snprintf(path, sizeof path, "%s/%s", dir, name);
        snprintf(tmp, sizeof tmp, "%s.partial", path);
        bad = fastf_res_make_dir(dir);
        if (!bad && (fastf_write_gz_text(tmp, t->p ? t->p : "", t->len) || rename(tmp, path) != 0)) { unlink(tmp); bad = fastf_res_err("cannot write %s", path); }
    }
    free(t->p);
    memset(t, 0, sizeof *t);
    return bad;
}

/* dir/name: `header`, then n lines, line i appended by line(t, ctx, i) */
typedef int (*res_line_fn)(gtext *t, const void *ctx, uint32_t i);
static int flat_file(const char *dir, const char *name, const char *header, uint32_t n, res_line_fn line, const void *ctx)
{
    gtext t = { NULL, 0, 0 };
    int bad = fastf_gt_str(&t, header);
    for (uint32_t i = 0; i < n && !bad; i++) bad = line(&t, ctx, i);
    return fastf_res_text_file(dir, name, &t, bad);
}

/* ------------------------------------------------------------------ */
/* --genes: the table, the grid file, a point's file                   */
/* ------------------------------------------------------------------ */
static void genes_release(res_genes_t *G)
{
    if (G->feat_id) for (uint32_t i = 0; i < G->n_features; i++) free(G->feat_id[i]);
    free(G->feat_id); free(G->cells); free(G->names);
    G->feat_id = NULL; G->cells = NULL; G->names = NULL; G->n_features = G->n_points = 0;
}

int fastf_res_genes_open(res_genes_t *G, int on, const res_verb_t *V, const char *out_dir, uint32_t max_points, int no_grid)
{
    memset(G, 0, sizeof *G);
    if (!on) return 0;
    G->verb = V->name; G->max_points = no_grid ? 0 : max_points; G->no_grid = no_grid;
    snprintf(G->out_dir, sizeof G->out_dir, "%s", out_dir);
    if (!(G->names = calloc(G->max_points ? G->max_points : 1, sizeof *G->names))) return fastf_res_err("out of memory");
    if (fastf_res_table_open(&G->tsv, V, out_dir, TB_GENES)) { genes_release(G); return 1; }
    G->on = 1;
    return 0;
}

typedef struct { char *const *feat_id; const uint32_t *cells; const uint64_t *umis; } genes_lines_t;
static int genes_line(gtext *t, const void *ctx, uint32_t i)
{
    const genes_lines_t *g = (const genes_lines_t *)ctx;
    return fastf_gt_str(t, g->feat_id[i]) || fastf_gt_u64(t, '\t', g->cells[i]) || fastf_gt_u64(t, '\t', g->umis[i]) || fastf_gt_str(t, "\n");
}

int fastf_res_genes_point(res_genes_t *G, const fastf_lists_t *L, const char *point_name, const char *dir, const char *row,
                          const uint32_t *cells, const uint64_t *umis)
{
    if (!G->on) return 0;
    if (!G->feat_id) {                                      /* the first point: the names and the room of the grid file */
        const uint32_t nf = (uint32_t)L->n_features;
        if (!(G->feat_id = (char **)calloc(nf ? nf : 1, sizeof *G->feat_id)) ||
            !(G->cells = (uint32_t *)malloc(((size_t)G->max_points * nf + 1) * sizeof *G->cells))) return fastf_res_err("out of memory");
        for (uint32_t i = 0; i < nf; i++) { if (!(G->feat_id[i] = strdup(L->feat_id[i]))) return fastf_res_err("out of memory"); G->n_features = i + 1; }
    }
    if ((uint32_t)L->n_features != G->n_features) return fastf_res_err("internal error: the feature list changed between points");
    const uint32_t nf = G->n_features;
    if (!G->no_grid) {
        if (G->n_points >= G->max_points) return fastf_res_err("internal error: more points than the grid has");
        snprintf(G->names[G->n_points], sizeof G->names[0], "%s", point_name);
        if (nf) memcpy(G->cells + (size_t)G->n_points * nf, cells, (size_t)nf * sizeof *cells);
        G->n_points++;
    }
    const genes_lines_t lines = { G->feat_id, cells, umis };
    if (dir && flat_file(dir, "genes.tsv.gz", "", nf, genes_line, &lines)) return 1;
    fputs(row, G->tsv.f);
    return 0;
}

/* ok: the grid file, then the table; otherwise nothing of either is left */
int fastf_res_genes_close(res_genes_t *G, int ok)
{
    if (!G->on) return 0;
    int rc = 0;
    if (ok && !G->no_grid) {
        char name[64];
        gtext t = { NULL, 0, 0 };
        int bad = fastf_gt_str(&t, "feature");
        for (uint32_t p = 0; p < G->n_points && !bad; p++) bad = fastf_gt_str(&t, "\t") || fastf_gt_str(&t, G->names[p]);
        if (!bad) bad = fastf_gt_str(&t, "\n");
        for (uint32_t i = 0; i < G->n_features && !bad; i++) {
            bad = fastf_gt_str(&t, G->feat_id[i]);
            for (uint32_t p = 0; p < G->n_points && !bad; p++) bad = fastf_gt_u64(&t, '\t', G->cells[(size_t)p * G->n_features + i]);
            if (!bad) bad = fastf_gt_str(&t, "\n");
        }
        snprintf(name, sizeof name, "%s_gene_cells.tsv.gz", G->verb);
        rc = fastf_res_text_file(G->out_dir, name, &t, bad);
    }
    char keep[512]; snprintf(keep, sizeof keep, "%s", fastf_last_error());
    if (fastf_res_tsv_close(&G->tsv, ok && !rc)) rc = 1; else if (rc) fastf_set_error_(keep);
    genes_release(G);
    G->on = 0;
    return rc;
}

/* ------------------------------------------------------------------ */
/* --cells: the table, a point's file                                  */
/* ------------------------------------------------------------------ */
int fastf_res_cells_open(res_cells_t *C, int on, const res_verb_t *V, const char *out_dir)
{
    memset(C, 0, sizeof *C);
    if (!on) return 0;
    C->verb = V->name;
    if (fastf_res_table_open(&C->tsv, V, out_dir, TB_CELLS)) return 1;
    C->on = 1;
    return 0;
}

static int cells_line(gtext *t, const void *ctx, uint32_t k)
{
    const res_rate_t *S = (const res_rate_t *)ctx;
    const uint64_t reads = S->h_cs.rpc[k], umis = S->buf.h_upc.u64[k];
    char sat[32];
    snprintf(sat, sizeof sat, "\t%.6f\n", reads ? 1.0 - (double)umis / (double)reads : 0.0);
    return fastf_gt_str(t, S->L->barcode[k]) || fastf_gt_u64(t, '\t', reads) || fastf_gt_u64(t, '\t', S->h_cs.npc[k]) || fastf_gt_u64(t, '\t', umis) ||
           fastf_gt_u64(t, '\t', S->buf.h_gpc.u32[k]) || fastf_gt_u64(t, '\t', S->h_cs.spc[k]) || fastf_gt_str(t, sat);
}

int fastf_res_cells_point(res_cells_t *C, const res_rate_t *S, const char *dir, const char *row)
{
    if (!C->on) return 0;
    if (dir && flat_file(dir, "cells.tsv.gz", "barcode\treads\tnull_umi_reads\tumis\tgenes\tsingleton_umis\tsaturation\n", S->n_cells, cells_line, S)) return 1;
    fputs(row, C->tsv.f);
    return 0;
}

int fastf_res_cells_close(res_cells_t *C, int ok)
{
    if (!C->on) return 0;
    C->on = 0;
    return fastf_res_tsv_close(&C->tsv, ok);
}

/* ------------------------------------------------------------------ */
/* the comparisons against full depth: the point writers               */
/* ------------------------------------------------------------------ */
/* each: the row(s) of the point into its table(s) and — dir != NULL — its file(s) into dir, from the host views of S */
static FILE *cmp_tsv(res_cmp_t *C, int table) { return C->tsv[table - TB_FIDELITY].f; }

static int fid_line(gtext *t, const void *ctx, uint32_t k)
{
    const res_rate_t *S = (const res_rate_t *)ctx;
    char line[512];
    return fastf_fidelity_row(S->L->barcode[k], S->h_fid.ufull[k], S->buf.h_upc.u64[k], S->h_fid.gfull[k], S->buf.h_gpc.u32[k], S->h_fid.sxx[k], S->h_fid.syy[k], S->h_fid.sxy[k],
                              S->n_features, line, sizeof line) || fastf_gt_str(t, line);
}
static int fid_point(res_cmp_t *C, const res_rate_t *S, const char *dir, float rate_depth, uint64_t list_value)
{
    char row[640];
    if (fastf_fidelity_summary_row(S->rate_cell, rate_depth, list_value, S->seed, S->h_fid.ufull, S->buf.h_upc.u64, S->h_fid.gfull, S->buf.h_gpc.u32, S->h_fid.sxx, S->h_fid.syy, S->h_fid.sxy,
                                   S->n_cells, S->n_features, row, sizeof row)) return 1;
    if (dir && flat_file(dir, "fidelity.tsv.gz", fastf_fidelity_header(), S->n_cells, fid_line, S)) return 1;
    fputs(row, cmp_tsv(C, TB_FIDELITY));
    return 0;
}

static int gene_fid_line(gtext *t, const void *ctx, uint32_t g)
{
    const res_rate_t *S = (const res_rate_t *)ctx;
    char line[640];
    return fastf_gene_fidelity_row(S->L->feat_id[g], S->n_cells, S->h_gfid.sx[g], S->h_gfid.sy[g], S->h_gfid.cf[g], S->h_gfid.c[g], S->h_gfid.sxx[g], S->h_gfid.syy[g],
                                   S->h_gfid.sxy[g], line, sizeof line) || fastf_gt_str(t, line);
}
static int gene_fid_point(res_cmp_t *C, const res_rate_t *S, const char *dir, float rate_depth, uint64_t list_value)
{
    char row[640];
    if (fastf_gene_fidelity_summary_row(S->rate_cell, rate_depth, list_value, S->seed, S->n_cells, S->h_gfid.sx, S->h_gfid.sy, S->h_gfid.sxx, S->h_gfid.syy, S->h_gfid.sxy,
                                        S->n_features, row, sizeof row)) return 1;
    if (dir && flat_file(dir, "gene_fidelity.tsv.gz", fastf_gene_fidelity_header(), S->n_features, gene_fid_line, S)) return 1;
    fputs(row, cmp_tsv(C, TB_GENE_FIDELITY));
    return 0;
}

static int nbr_line(gtext *t, const void *ctx, uint32_t c)
{
    const res_rate_t *S = (const res_rate_t *)ctx;
    char line[512];
    return fastf_neighbors_row(S->L->barcode[c], S->h_nbr.kf[c], S->h_nbr.kp[c], S->h_nbr.sh[c], line, sizeof line) || fastf_gt_str(t, line);
}
static int nbr_point(res_cmp_t *C, const res_rate_t *S, const char *dir, float rate_depth, uint64_t list_value)
{
    char row[640];
    if (fastf_neighbors_summary_row(S->rate_cell, rate_depth, list_value, S->seed, S->n_cells, S->hvg_k, FASTF_NEIGHBORS_K, S->h_nbr.kf, S->h_nbr.kp, S->h_nbr.sh, row, sizeof row)) return 1;
    if (dir && flat_file(dir, "neighbors.tsv.gz", fastf_neighbors_header(), S->n_cells, nbr_line, S)) return 1;
    fputs(row, cmp_tsv(C, TB_NEIGHBORS));
    return 0;
}

/* --labels: labels.tsv.gz is flat; label_confusion.tsv.gz has a header and rows as wide as the labels are many */
typedef struct { const res_rate_t *S; const char **names; } lab_lines_t;
static int lab_line(gtext *t, const void *ctx, uint32_t c)
{
    const lab_lines_t *x = (const lab_lines_t *)ctx;
    const res_rate_t *S = x->S;
    char line[512];
    return fastf_labels_row(S->L->barcode[c], x->names[S->h_lab.lab[c]], x->names[S->h_lab.half[0].pred[c]], x->names[S->h_lab.half[1].pred[c]], S->h_lab.half[0].same[c],
                            S->h_lab.half[0].labelled[c], S->h_lab.half[1].same[c], S->h_lab.half[1].labelled[c], line, sizeof line) || fastf_gt_str(t, line);
}
static int lab_point(res_cmp_t *C, const res_rate_t *S, const char *dir, float rate_depth, uint64_t list_value)
{
    const uint32_t L = S->n_labels;
    const uint8_t *const lab = S->h_lab.lab;
    const uint32_t *const cx = S->h_lab.half[0].conf, *const cy = S->h_lab.half[1].conf;
    char row[640];
    if (fastf_labels_summary_row(S->rate_cell, rate_depth, list_value, S->seed, S->n_cells, FASTF_NEIGHBORS_K, L, lab, S->h_lab.half[0].pred, S->h_lab.half[1].pred, S->h_lab.half[0].same,
                                 S->h_lab.half[0].labelled, S->h_lab.half[1].same, S->h_lab.half[1].labelled, cx, cy, row, sizeof row)) return 1;
    if (dir) {
        const size_t wide = 64 + (size_t)(L + 1) * FASTF_LABEL_BYTES;
        char *const wl = (char *)malloc(wide);
        const char **const names = (const char **)malloc(((size_t)L + 1) * sizeof *names);
        uint32_t *const cells = (uint32_t *)calloc((size_t)L + 1, sizeof *cells);
        const lab_lines_t lines = { S, names };
        gtext u = { NULL, 0, 0 };
        int bad = !wl || !names || !cells;
        if (bad) fastf_res_err("out of memory");
        for (uint32_t l = 0; l <= L && !bad; l++) names[l] = fastf_labels_name(C->labels, l);
        if (!bad) bad = flat_file(dir, "labels.tsv.gz", fastf_labels_header(), S->n_cells, lab_line, &lines);
        for (uint32_t c = 0; c < S->n_cells && !bad; c++) cells[lab[c]]++;
        if (!bad) bad = fastf_label_confusion_header(names, L, wl, wide) || fastf_gt_str(&u, wl);
        for (uint32_t a = 1; a <= L && !bad; a++)
            bad = fastf_label_confusion_row(names[a], cells[a], cy + (size_t)(a - 1) * (L + 1), L, wl, wide) || fastf_gt_str(&u, wl);
        bad = fastf_res_text_file(dir, "label_confusion.tsv.gz", &u, bad);
        free(wl); free(names); free(cells);
        if (bad) return 1;
    }
    fputs(row, cmp_tsv(C, TB_LABELS));
    for (uint32_t a = 1; a <= L; a++) {
        if (fastf_label_classes_row(S->rate_cell, rate_depth, list_value, S->seed, fastf_labels_name(C->labels, a), a, S->n_cells, L, lab, cx, cy, row, sizeof row)) return 1;
        fputs(row, cmp_tsv(C, TB_LABEL_CLASSES));
    }
    return 0;
}

/* --markers: markers.tsv.gz lists per label the genes in the top N_eff of the full rows or of the point, in the order of their full ranks */
static int mk_point(res_cmp_t *C, const res_rate_t *S, const char *dir, float rate_depth, uint64_t list_value)
{
    const uint32_t L = S->n_labels, K = S->hvg_k, top = C->markers < K ? C->markers : K;
    const res_mk_v mf = res_mk_host(S, 0), mp = res_mk_host(S, 1);
    const uint32_t *const npl = mf.npl, *const rf = res_mk_rank(S, 0), *const rp = res_mk_rank(S, 1);
    const uint32_t *const df = mf.det, *const dp = mp.det;
    const size_t rows_cap = ((size_t)L + 1) * (FASTF_LABEL_BYTES + 160);
    char *const rows = (char *)malloc(rows_cap);
    const char **const names = (const char **)malloc(((size_t)L + 1) * sizeof *names);
    uint32_t *const by_rank = (uint32_t *)malloc(((size_t)K + 1) * sizeof *by_rank), *const det_all = (uint32_t *)calloc(2 * (size_t)K + 1, sizeof *det_all);
    int bad = !rows || !names || !by_rank || !det_all;
    if (bad) fastf_res_err("out of memory");
    for (uint32_t l = 0; l <= L && !bad; l++) names[l] = fastf_labels_name(C->labels, l);
    if (!bad) bad = fastf_markers_summary_rows(S->rate_cell, rate_depth, list_value, S->seed, names, L, K, C->markers, npl, rf, rp, mf.s2u, mp.s2u, rows, rows_cap);
    if (dir && !bad) {
        char line[512];
        gtext t = { NULL, 0, 0 };
        uint64_t n_lab = 0;
        for (uint32_t a = 0; a < L; a++) { n_lab += npl[a]; for (uint32_t g = 0; g < K; g++) { det_all[g] += df[(size_t)a * K + g]; det_all[K + g] += dp[(size_t)a * K + g]; } }
        bad = fastf_gt_str(&t, fastf_markers_header());
        for (uint32_t a = 0; a < L && !bad; a++) {
            const size_t at = (size_t)a * K;
            const uint32_t n_in = npl[a], n_out = (uint32_t)(n_lab - n_in);
            if (!n_in || !n_out) { bad = fastf_markers_row(names[a + 1], NULL, n_in, n_out, 0, 0, 0, 0, 0, 0, 0, 0, 0, line, sizeof line) || fastf_gt_str(&t, line); continue; }
            for (uint32_t g = 0; g < K; g++) by_rank[rf[at + g] - 1] = g;
            for (uint32_t r = 0; r < K && !bad; r++) {
                const uint32_t g = by_rank[r];
                if (r >= top && rp[at + g] > top) continue;
                bad = fastf_markers_row(names[a + 1], S->L->feat_id[S->h_nbr.genes[g]], n_in, n_out, rf[at + g], rp[at + g], mf.s2u[at + g], mp.s2u[at + g],
                                        df[at + g], det_all[g] - df[at + g], dp[at + g], det_all[K + g] - dp[at + g], mp.sum[at + g], line, sizeof line) || fastf_gt_str(&t, line);
            }
        }
        bad = fastf_res_text_file(dir, "markers.tsv.gz", &t, bad);
    }
    if (!bad) fputs(rows, cmp_tsv(C, TB_MARKERS));
    free(rows); free(names); free(by_rank); free(det_all);
    return bad;
}

/* --coexpression: one row per gene of A in rank order, the gene named by its feature id */
static int cx_line(gtext *t, const void *ctx, uint32_t g)
{
    const res_rate_t *S = (const res_rate_t *)ctx;
    char line[512];
    return fastf_coexpr_row(S->L->feat_id[S->h_cx.genes[g]], S->h_cx.kf[g], S->h_cx.kp[g], S->h_cx.sh[g], line, sizeof line) || fastf_gt_str(t, line);
}
static int cx_point(res_cmp_t *C, const res_rate_t *S, const char *dir, float rate_depth, uint64_t list_value)
{
    char row[640];
    if (fastf_coexpr_summary_row(S->rate_cell, rate_depth, list_value, S->seed, S->n_cells, S->hvg_k, FASTF_COEXPR_K, S->h_cx.kf, S->h_cx.kp, S->h_cx.sh, row, sizeof row)) return 1;
    if (dir && flat_file(dir, "coexpr.tsv.gz", fastf_coexpr_header(), S->hvg_k, cx_line, S)) return 1;
    fputs(row, cmp_tsv(C, TB_COEXPR));
    return 0;
}

/* --mapping: one row per barcode; pred_map as the label string with --labels */
typedef struct { const res_rate_t *S; const fastf_labels_t *labels; } map_lines_t;
static int map_line(gtext *t, const void *ctx, uint32_t c)
{
    const map_lines_t *x = (const map_lines_t *)ctx;
    const res_rate_t *S = x->S;
    const uint8_t pred = x->labels ? S->h_map.pred[c] : 0;
    char line[512];
    return fastf_mapping_row(S->L->barcode[c], S->h_map.sd[c], S->h_map.rank[c], S->h_map.km[c], S->h_nbr.kf[c], S->h_map.hood[c], pred ? fastf_labels_name(x->labels, pred) : NULL,
                             line, sizeof line) || fastf_gt_str(t, line);
}
static int map_point(res_cmp_t *C, const res_rate_t *S, const char *dir, float rate_depth, uint64_t list_value)
{
    const map_lines_t lines = { S, C->labels };
    char row[640];
    if (fastf_mapping_summary_row(S->rate_cell, rate_depth, list_value, S->seed, S->n_cells, S->hvg_k, FASTF_MAPPING_K, S->h_map.sd, S->h_map.rank, S->h_nbr.kf, S->h_map.hood,
                                  C->labels ? S->h_lab.lab : NULL, S->h_map.same, S->h_map.labelled, row, sizeof row)) return 1;
    if (dir && flat_file(dir, "mapping.tsv.gz", fastf_mapping_header(), S->n_cells, map_line, &lines)) return 1;
    fputs(row, cmp_tsv(C, TB_MAPPING));
    return 0;
}

/* --pseudotime: one row per barcode; the map columns from the third half with --mapping (C->on says so) */
typedef struct { const res_rate_t *S; int mapping; } pt_lines_t;
static int pt_line(gtext *t, const void *ctx, uint32_t c)
{
    const pt_lines_t *x = (const pt_lines_t *)ctx;
    const res_rate_t *S = x->S;
    char line[512];
    return fastf_ptime_row(S->L->barcode[c], S->h_pt.t[c], S->h_pt.half[0].est[c], S->h_pt.half[0].valued[c], S->h_pt.half[1].est[c], S->h_pt.half[1].valued[c],
                           x->mapping ? S->h_pt.half[2].est[c] : 0, x->mapping ? S->h_pt.half[2].valued[c] : 0, x->mapping, line, sizeof line) || fastf_gt_str(t, line);
}
static int pt_point(res_cmp_t *C, const res_rate_t *S, const char *dir, float rate_depth, uint64_t list_value)
{
    const pt_lines_t lines = { S, res_cmp_on(C, CMP_MAPPING) };
    char row[640];
    if (fastf_ptime_summary_row(S->rate_cell, rate_depth, list_value, S->seed, S->n_cells, FASTF_NEIGHBORS_K, S->pt_m, S->h_pt.half[0].census, S->h_pt.half[1].census,
                                lines.mapping ? S->h_pt.half[2].census : NULL, row, sizeof row)) return 1;
    if (dir && flat_file(dir, "pseudotime.tsv.gz", fastf_ptime_header(), S->n_cells, pt_line, &lines)) return 1;
    fputs(row, cmp_tsv(C, TB_PTIME));
    return 0;
}

/* ------------------------------------------------------------------ */
/* the comparisons against full depth: the descriptors, open, point, close */
/* ------------------------------------------------------------------ */
/* ONE descriptor per comparison, in the order a point writes them: the flag bit of the verbs' flag word that switches it on (0: --labels,
 * --markers, --mapping and --pseudotime come with an argument of their own), its tables (-1: none), its timer in res_times_t, its point writer.  A further comparison
 * is an entry here, its writer above and its table in GRID_TABLES (grid_rows.c) */
static const struct {
    uint32_t flag; int table[2]; size_t timer;
    int (*point)(res_cmp_t *C, const res_rate_t *S, const char *dir, float rate_depth, uint64_t list_value);
} cmp_desc[CMP_N_] = {
    [CMP_NEIGHBORS] = { FASTF_SWEEP_NEIGHBORS,     { TB_NEIGHBORS, -1 },            offsetof(res_times_t, neighbors), nbr_point },
    [CMP_LABELS]    = { 0,                         { TB_LABELS, TB_LABEL_CLASSES }, offsetof(res_times_t, labels),    lab_point },
    [CMP_MARKERS]   = { 0,                         { TB_MARKERS, -1 },              offsetof(res_times_t, markers),   mk_point },
    [CMP_COEXPR]    = { FASTF_SWEEP_COEXPRESSION,  { TB_COEXPR, -1 },               offsetof(res_times_t, coexpr),    cx_point },
    [CMP_MAPPING]   = { 0,                         { TB_MAPPING, -1 },              offsetof(res_times_t, mapping),   map_point },
    [CMP_PTIME]     = { 0,                         { TB_PTIME, -1 },                offsetof(res_times_t, ptime),     pt_point },
    [CMP_GENE_FID]  = { FASTF_SWEEP_GENE_FIDELITY, { TB_GENE_FIDELITY, -1 },        offsetof(res_times_t, gene_fid),  gene_fid_point },
    [CMP_FIDELITY]  = { FASTF_SWEEP_FIDELITY,      { TB_FIDELITY, -1 },             offsetof(res_times_t, fidelity),  fid_point },
};

/* the tables are opened in the order of their ids, which is the order of the renames */
int fastf_res_cmp_open(res_cmp_t *C, const res_verb_t *V, const char *out_dir, uint32_t flags, const fastf_labels_t *labels, uint32_t markers, uint32_t mapping,
                       const fastf_ptime_t *ptime)
{
    uint32_t want = 0;
    memset(C, 0, sizeof *C);
    C->labels = labels; C->markers = markers; C->ptime = ptime;
    for (int c = 0; c < CMP_N_; c++) {
        if (!(c == CMP_LABELS ? labels != NULL : c == CMP_MARKERS ? markers != 0 : c == CMP_MAPPING ? mapping != 0 : c == CMP_PTIME ? ptime != NULL : (flags & cmp_desc[c].flag) != 0)) continue;
        C->on |= 1u << c;
        for (int k = 0; k < 2; k++) if (cmp_desc[c].table[k] >= 0) want |= 1u << (cmp_desc[c].table[k] - TB_FIDELITY);
    }
    for (int k = 0; k < RES_CMP_TABLES; k++)
        if ((want >> k & 1) && fastf_res_table_open(&C->tsv[k], V, out_dir, TB_FIDELITY + k)) { fastf_res_cmp_close(C, 0); return 1; }
    return 0;
}

/* what the device side computes for the comparisons that are on: the neighbour sets for --labels, --mapping and --pseudotime too */
void fastf_res_cmp_cfg(const res_cmp_t *C, res_cfg_t *cfg)
{
    cfg->fidelity = res_cmp_on(C, CMP_FIDELITY); cfg->gene_fid = res_cmp_on(C, CMP_GENE_FID); cfg->labels = res_cmp_on(C, CMP_LABELS);
    cfg->mapping = res_cmp_on(C, CMP_MAPPING); cfg->ptime = res_cmp_on(C, CMP_PTIME);
    cfg->neighbors = res_cmp_on(C, CMP_NEIGHBORS) || cfg->labels || cfg->mapping || cfg->ptime;
    cfg->coexpr = res_cmp_on(C, CMP_COEXPR);
    cfg->lab_t = C->labels; cfg->markers = C->markers; cfg->pt_t = C->ptime;
}

int fastf_res_cmp_point(res_cmp_t *C, const res_rate_t *S, const char *dir, float rate_depth, uint64_t list_value, res_times_t *T)
{
    for (int c = 0; c < CMP_N_; c++) {
        if (!res_cmp_on(C, c)) continue;
        const double tt = fastf_res_now();
        if (cmp_desc[c].point(C, S, dir, rate_depth, list_value)) return 1;
        *(double *)((char *)T + cmp_desc[c].timer) += fastf_res_now() - tt;
    }
    return 0;
}

/* every table is closed before any is renamed, and a rename that fails takes the others back: none is left alone */
int fastf_res_cmp_close(res_cmp_t *C, int ok)
{
    int bad = 0, rc = 0;
    uint32_t renamed = 0;
    const char *failed = NULL;
    for (int k = 0; k < RES_CMP_TABLES; k++) {
        res_tsv_t *const t = &C->tsv[k];
        if (t->f) { if (ferror(t->f) | (fclose(t->f) != 0)) { bad = 1; failed = t->final; } t->f = NULL; }
    }
    for (int k = 0; k < RES_CMP_TABLES && ok && !bad; k++) {
        res_tsv_t *const t = &C->tsv[k];
        if (!t->tmp[0]) continue;
        if (rename(t->tmp, t->final) == 0) renamed |= 1u << k; else { bad = 1; failed = t->final; }
    }
    if (!ok || bad) for (int k = 0; k < RES_CMP_TABLES; k++) if (C->tsv[k].tmp[0]) { unlink(C->tsv[k].tmp); if (renamed >> k & 1) unlink(C->tsv[k].final); }
    if (ok && bad) rc = fastf_res_err("cannot write %s", failed);
    memset(C, 0, sizeof *C);
    return rc;
}

/* a run failed after tables were renamed into place: none of the per-verb tables a run can have written is left */
void fastf_res_reps_unlink_tables(const char *out_dir, const char *verb)
{
    static const int others[] = { TB_GENES, TB_CELLS, TB_REPS, TB_GENES_REPS };
    char path[4200];
    for (int k = 0; k < 4 + RES_CMP_TABLES; k++) {
        snprintf(path, sizeof path, "%s/%s_%s.tsv", out_dir, verb, fastf_res_table_stem(k < 4 ? others[k] : TB_FIDELITY + k - 4));
        unlink(path);
    }
    snprintf(path, sizeof path, "%s/%s_gene_reps.tsv.gz", out_dir, verb);
    unlink(path);
}
