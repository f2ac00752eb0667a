/*
 * grid_rows.c — the host analysis and the rows `fastF sweep`, `fastF cap` and `fastF level` share: the host twins of the device
 * summaries (*_from_coo and their kin), the metrics, the rows of every table and point file (*_row, *_summary_row) and the headers of
 * the per-verb tables, defined once (GRID_TABLES).  Nothing here touches the device: the file links into a CPU program as it is.
 */
#define _GNU_SOURCE
#include "resident.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int fastf_res_err(const char *fmt, ...)
{
    char buf[480];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    fastf_set_error_(buf);
    return 1;
}

/* ------------------------------------------------------------------ */
/* the headers of the per-verb tables                                  */
/* ------------------------------------------------------------------ */
/* every table the three verbs write beside their summary, once: (table id of resident.h, stem of <verb>_<stem>.tsv and of the getters,
 * the columns behind the verb's two).  The three getters of a table and the lookup of the grid come from this list */
#define REPS_STAT4(m) "\t" m "_mean\t" m "_sd\t" m "_min\t" m "_max"
#define GRID_TABLES(X) \
    X(TB_GENES, genes, "seed\tgenes_detected\tgenes_min_cells_3\tgenes_min_cells_10\tmax_gene_umis\n") \
    X(TB_CELLS, cells, "seed\tvalid_reads\tnull_umi_reads\tumis\tsingleton_umis\tmedian_reads_per_cell\t" \
        "copies_1\tcopies_2\tcopies_3\tcopies_4\tcopies_5\tcopies_6\tcopies_7\tcopies_8\tcopies_9\tcopies_10\tcopies_11\tcopies_12\tcopies_13\t" \
        "copies_14\tcopies_15\tcopies_16\tcopies_17\tcopies_18\tcopies_19\tcopies_20\tcopies_21\tcopies_22\tcopies_23\tcopies_24\tcopies_25\t" \
        "copies_26\tcopies_27\tcopies_28\tcopies_29\tcopies_30\tcopies_31\tcopies_32_plus\treads_copies_32_plus\n") \
    X(TB_FIDELITY, fidelity, "seed\tn_cells\tcells_defined\tmedian_pearson\tp10_pearson\tmean_pearson\tmedian_cosine\tumis_kept\tgenes_kept\n") \
    X(TB_GENE_FIDELITY, gene_fidelity, "seed\tn_cells\tgenes_full\tgenes_defined\tmedian_pearson\tp10_pearson\tmean_pearson\thvg_k\thvg_overlap\n") \
    X(TB_NEIGHBORS, neighbors, "seed\tn_cells\thvg_k\tk\tcells_defined\tmedian_overlap\tp10_overlap\tmean_overlap\tmean_k_point\n") \
    X(TB_LABELS, labels, "seed\tn_cells\tk\tn_labels\tcells_labelled\tagree_full\tagree_point\taccuracy_full\taccuracy_point\tkept\tpurity_full\tpurity_point\n") \
    X(TB_LABEL_CLASSES, label_classes, "seed\tlabel\tcells\tcorrect_full\tcorrect_point\tpredicted_full\tpredicted_point\n") \
    X(TB_MARKERS, markers, "seed\tlabel\tn_in\tn_out\ttop\tkept\tauc_full_mean\tauc_point_mean\n") \
    X(TB_COEXPR, coexpr, "seed\tn_cells\thvg_k\tk\tgenes_defined\tsum_k_full\tsum_k_point\tsum_shared\tmean_kept\tgenes_half_kept\n") \
    X(TB_MAPPING, mapping, "seed\tn_cells\thvg_k\tk\tcells_defined\tself_top1\tself_topk\tmedian_self_rank\tp90_self_rank\tmean_hood\tcells_labelled\taccuracy_map\n") \
    X(TB_PTIME, pseudotime, "seed\tn_cells\tk\tcells_valued\tcells_full\tconc_full\tdisc_full\ttau_full\tshift_full\tcells_point\tconc_point\tdisc_point\ttau_point\tshift_point\t" \
        "cells_map\tconc_map\tdisc_map\ttau_map\tshift_map\n") \
    X(TB_REPS, reps, "n_reps\tn_cells" REPS_STAT4("sampled_reads") REPS_STAT4("sampled_valid_reads") REPS_STAT4("nnz") REPS_STAT4("umis") \
        REPS_STAT4("saturation") REPS_STAT4("median_umis_per_cell") REPS_STAT4("median_genes_per_cell") "\n") \
    X(TB_GENES_REPS, genes_reps, "n_reps" REPS_STAT4("genes_detected") "\tgenes_in_all_reps\tgenes_in_any_rep\n")

#define X(id, stem, tail) \
    const char *fastf_sweep_##stem##_header(void) { return "rate_cell\trate_depth\t" tail; } \
    const char *fastf_cap_##stem##_header(void) { return "rate_cell\treads_per_cell\t" tail; } \
    const char *fastf_level_##stem##_header(void) { return "rate_cell\tumi_cap\t" tail; }
GRID_TABLES(X)
#undef X

static const struct { const char *stem; const char *(*header[3])(void); } grid_table[TB_N_] = {
#define X(id, stem, tail) [id] = { #stem, { [VERB_SWEEP] = fastf_sweep_##stem##_header, [VERB_CAP] = fastf_cap_##stem##_header, [VERB_LEVEL] = fastf_level_##stem##_header } },
    GRID_TABLES(X)
#undef X
};
const char *fastf_res_table_stem(int table) { return grid_table[table].stem; }
const char *fastf_res_table_header(int verb, int table) { return grid_table[table].header[verb](); }

/* ------------------------------------------------------------------ */
/* the summary row                                                     */
/* ------------------------------------------------------------------ */
const char *fastf_sweep_header(void)
{
    return "rate_cell\trate_depth\tseed\tn_cells\ttotal_reads\tsampled_reads\tsampled_valid_reads\tnnz\tumis\tsaturation\t"
           "median_umis_per_cell\tmedian_genes_per_cell\n";
}

static int cmp_u64(const void *a, const void *b) { const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b; return x < y ? -1 : x > y; }

/* median over all n values (a cell without rows is a 0 among them); the mean of the two middle values when n is even */
static double median_u64(uint64_t *v, size_t n)
{
    if (!n) return 0.0;
    qsort(v, n, sizeof *v, cmp_u64);
    return (n & 1) ? (double)v[n / 2] : ((double)v[n / 2 - 1] + (double)v[n / 2]) / 2.0;
}

/* per cell (1-based index c -> slot c - 1) the sum of the counts and the rows with count >= 1, and the sum of all counts: the host
 * form of the device call cell_summary (the point-by-point path, tests) */
int fastf_sweep_cells_from_coo(const fastf_coo_t *coo, uint32_t n_cells, uint64_t *umis_per_cell, uint32_t *genes_per_cell, uint64_t *umis)
{
    if (!coo || !umis || (n_cells && (!umis_per_cell || !genes_per_cell))) return fastf_res_err("null argument");
    memset(umis_per_cell, 0, (size_t)n_cells * sizeof *umis_per_cell);
    memset(genes_per_cell, 0, (size_t)n_cells * sizeof *genes_per_cell);
    uint64_t total = 0;
    for (size_t i = 0; i < coo->nnz; i++) {
        const uint32_t c = coo->cell[i];
        if (c == 0 || c > n_cells) return fastf_res_err("matrix row %zu names cell %u of %u", i, c, n_cells);
        umis_per_cell[c - 1] += coo->count[i];
        genes_per_cell[c - 1] += coo->count[i] >= 1;
        total += coo->count[i];
    }
    *umis = total;
    return 0;
}

/* the columns from `seed` on (no newline): shared with cap.tsv */
int fastf_summary_tail_(uint32_t seed, const uint64_t counters[3], uint64_t nnz, uint64_t umis, const uint64_t *umis_per_cell,
                        const uint32_t *genes_per_cell, uint32_t n_cells, char *buf, size_t cap, double *metrics)
{
    if (!counters || !buf || (n_cells && (!umis_per_cell || !genes_per_cell))) return fastf_res_err("null argument");
    uint64_t *tmp = (uint64_t *)malloc(((size_t)n_cells + 1) * sizeof *tmp);
    if (!tmp) return fastf_res_err("out of memory");
    memcpy(tmp, umis_per_cell, (size_t)n_cells * sizeof *tmp);
    const double med_u = median_u64(tmp, n_cells);
    for (uint32_t i = 0; i < n_cells; i++) tmp[i] = genes_per_cell[i];
    const double med_g = median_u64(tmp, n_cells);
    free(tmp);
    const double sat = counters[2] ? 1.0 - (double)umis / (double)counters[2] : 0.0;
    if (metrics) {
        metrics[0] = (double)counters[1]; metrics[1] = (double)counters[2]; metrics[2] = (double)nnz; metrics[3] = (double)umis;
        metrics[4] = sat; metrics[5] = med_u; metrics[6] = med_g;
    }
    const int n = snprintf(buf, cap, "%u\t%u\t%llu\t%llu\t%llu\t%llu\t%llu\t%.6f\t%.1f\t%.1f", seed, n_cells, (unsigned long long)counters[0],
                           (unsigned long long)counters[1], (unsigned long long)counters[2], (unsigned long long)nnz, (unsigned long long)umis, sat, med_u, med_g);
    return (n < 0 || (size_t)n >= cap) ? fastf_res_err("summary row too long") : 0;
}

/* one row of sweep.tsv (with its newline); metrics: fastf_summary_tail_ */
int fastf_sweep_row_(float rate_cell, float rate_depth, uint32_t seed, const uint64_t counters[3], uint64_t nnz, uint64_t umis,
                        const uint64_t *umis_per_cell, const uint32_t *genes_per_cell, uint32_t n_cells, char *buf, size_t cap, double *metrics)
{
    char tail[400];
    if (fastf_summary_tail_(seed, counters, nnz, umis, umis_per_cell, genes_per_cell, n_cells, tail, sizeof tail, metrics)) return 1;
    const int n = snprintf(buf, cap, "%.3f\t%.3f\t%s\n", (double)rate_cell, (double)rate_depth, tail);
    return (n < 0 || (size_t)n >= cap) ? fastf_res_err("summary row too long") : 0;
}
int fastf_sweep_summary_row(float rate_cell, float rate_depth, uint32_t seed, const uint64_t counters[3], uint64_t nnz, uint64_t umis,
                            const uint64_t *umis_per_cell, const uint32_t *genes_per_cell, uint32_t n_cells, char *buf, size_t cap)
{
    return fastf_sweep_row_(rate_cell, rate_depth, seed, counters, nnz, umis, umis_per_cell, genes_per_cell, n_cells, buf, cap, NULL);
}

/* ------------------------------------------------------------------ */
/* --genes: the host twin, the row                                     */
/* ------------------------------------------------------------------ */
/* per gene (1-based feature g -> slot g - 1) the rows with count >= 1 and the sum of the counts: the host form of
 * the device call gene_summary (the point-by-point path, tests); a feature outside 1 .. n_features adds nothing, as there */
int fastf_sweep_genes_from_coo(const fastf_coo_t *coo, uint32_t n_features, uint32_t *cells_per_gene, uint64_t *umis_per_gene)
{
    if (!coo || (n_features && (!cells_per_gene || !umis_per_gene)) || (coo->nnz && (!coo->feature || !coo->count))) return fastf_res_err("null argument");
    memset(cells_per_gene, 0, (size_t)n_features * sizeof *cells_per_gene);
    memset(umis_per_gene, 0, (size_t)n_features * sizeof *umis_per_gene);
    for (size_t i = 0; i < coo->nnz; i++) {
        const uint32_t g = coo->feature[i] - 1u;
        if (g >= n_features) continue;
        cells_per_gene[g] += coo->count[i] >= 1;
        umis_per_gene[g] += coo->count[i];
    }
    return 0;
}

/* one row of sweep_genes.tsv (reads_per_cell == 0) or cap_genes.tsv (reads_per_cell >= 1: a cap is at least 1), with its newline */
int fastf_genes_summary_row(float rate_cell, float rate_depth, uint64_t reads_per_cell, uint32_t seed, const uint32_t *cells_per_gene,
                            const uint64_t *umis_per_gene, uint32_t n_features, char *buf, size_t cap)
{
    if (!buf || (n_features && (!cells_per_gene || !umis_per_gene))) return fastf_res_err("null argument");
    uint32_t d1 = 0, d3 = 0, d10 = 0;
    uint64_t top = 0;
    for (uint32_t g = 0; g < n_features; g++) {
        d1 += cells_per_gene[g] >= 1; d3 += cells_per_gene[g] >= 3; d10 += cells_per_gene[g] >= 10;
        if (umis_per_gene[g] > top) top = umis_per_gene[g];
    }
    char second[32];
    if (reads_per_cell) snprintf(second, sizeof second, "%llu", (unsigned long long)reads_per_cell);
    else snprintf(second, sizeof second, "%.3f", (double)rate_depth);
    const int n = snprintf(buf, cap, "%.3f\t%s\t%u\t%u\t%u\t%u\t%llu\n", (double)rate_cell, second, seed, d1, d3, d10, (unsigned long long)top);
    return (n < 0 || (size_t)n >= cap) ? fastf_res_err("summary row too long") : 0;
}

/* ------------------------------------------------------------------ */
/* --cells: the host twin, the row                                     */
/* ------------------------------------------------------------------ */
/* the host form of the device call copy_summary, by its rules (tests; a reader of umi.tsv.gz) */
int fastf_copies_from_umi_rows(const fastf_umi_rows_t *rows, uint32_t n_cells, uint32_t *reads, uint32_t *null_reads, uint32_t *single, uint64_t *hist)
{
    if (!rows || !reads || !null_reads || !single || !hist || (rows->n && (!rows->cell || !rows->n_copy || !rows->nonnull))) return fastf_res_err("null argument");
    memset(reads, 0, (size_t)n_cells * sizeof *reads);
    memset(null_reads, 0, (size_t)n_cells * sizeof *null_reads);
    memset(single, 0, (size_t)n_cells * sizeof *single);
    memset(hist, 0, (FASTF_COPY_BINS + 1) * sizeof *hist);
    for (size_t i = 0; i < rows->n; i++) {
        const uint32_t c = rows->cell[i] - 1u, k = rows->n_copy[i];
        const int nn = rows->nonnull[i] != 0;
        if (nn && k) {
            hist[(k < FASTF_COPY_BINS ? k : FASTF_COPY_BINS) - 1u]++;
            if (k >= FASTF_COPY_BINS) hist[FASTF_COPY_BINS] += k;
        }
        if (c >= n_cells) continue;
        reads[c] += k;
        if (!nn) null_reads[c] += k;
        else single[c] += k == 1;
    }
    return 0;
}


/* one row of sweep_cells.tsv (reads_per_cell == 0) or cap_cells.tsv (reads_per_cell >= 1), with its newline */
int fastf_cells_summary_row(float rate_cell, float rate_depth, uint64_t reads_per_cell, uint32_t seed, const uint32_t *reads,
                            const uint32_t *null_reads, const uint32_t *single, uint32_t n_cells, const uint64_t *hist, char *buf, size_t cap)
{
    if (!buf || !hist || (n_cells && (!reads || !null_reads || !single))) return fastf_res_err("null argument");
    uint64_t *tmp = (uint64_t *)malloc(((size_t)n_cells + 1) * sizeof *tmp);
    if (!tmp) return fastf_res_err("out of memory");
    uint64_t valid = 0, nulls = 0, singles = 0, umis = 0;
    for (uint32_t k = 0; k < n_cells; k++) { tmp[k] = reads[k]; valid += reads[k]; nulls += null_reads[k]; singles += single[k]; }
    const double med = median_u64(tmp, n_cells);
    free(tmp);
    for (uint32_t k = 0; k < FASTF_COPY_BINS; k++) umis += hist[k];
    char second[32];
    if (reads_per_cell) snprintf(second, sizeof second, "%llu", (unsigned long long)reads_per_cell);
    else snprintf(second, sizeof second, "%.3f", (double)rate_depth);
    int n = snprintf(buf, cap, "%.3f\t%s\t%u\t%llu\t%llu\t%llu\t%llu\t%.1f", (double)rate_cell, second, seed, (unsigned long long)valid,
                     (unsigned long long)nulls, (unsigned long long)umis, (unsigned long long)singles, med);
    for (uint32_t k = 0; k <= FASTF_COPY_BINS && n >= 0 && (size_t)n < cap; k++) {
        const int m = snprintf(buf + n, cap - (size_t)n, "\t%llu", (unsigned long long)hist[k]);
        n = m < 0 ? -1 : n + m;
    }
    if (n < 0 || (size_t)n + 1 >= cap) return fastf_res_err("summary row too long");
    buf[n] = '\n'; buf[n + 1] = '\0';
    return 0;
}

/* ------------------------------------------------------------------ */
/* --fidelity: the host twin, the metrics, the rows                    */
/* ------------------------------------------------------------------ */
/* the host form of the device call fidelity: both COOs ascend by (cell, feature), so the partner of a point row lies behind the partner of
 * the row before it — one forward walk of the full rows */
int fastf_fidelity_from_coo(const fastf_coo_t *full, const fastf_coo_t *point, uint32_t n_cells, uint64_t *sum_xy, uint64_t *sum_yy)
{
    if (!full || !point || (n_cells && (!sum_xy || !sum_yy)) || (point->nnz && (!point->feature || !point->cell || !point->count)) ||
        (full->nnz && (!full->feature || !full->cell || !full->count))) return fastf_res_err("null argument");
    memset(sum_xy, 0, (size_t)n_cells * sizeof *sum_xy);
    memset(sum_yy, 0, (size_t)n_cells * sizeof *sum_yy);
    size_t j = 0;
    for (size_t i = 0; i < point->nnz; i++) {
        const uint64_t key = ((uint64_t)point->cell[i] << 32) | point->feature[i];
        while (j < full->nnz && (((uint64_t)full->cell[j] << 32) | full->feature[j]) < key) j++;
        if (j == full->nnz || full->cell[j] != point->cell[i] || full->feature[j] != point->feature[i])
            return fastf_res_err("fidelity: point row %zu (cell %u, feature %u) has no partner among the full rows (device error bits 0x%x)", i, point->cell[i],
                          point->feature[i], FASTF_ERR_NO_PARTNER);
        const uint32_t c = point->cell[i] - 1u;
        if (c >= n_cells) continue;
        sum_xy[c] += (uint64_t)full->count[j] * point->count[i];
        sum_yy[c] += (uint64_t)point->count[i] * point->count[i];
    }
    return 0;
}

int fastf_fidelity_metrics(uint64_t umis_full, uint64_t umis, uint64_t sum_xx, uint64_t sum_yy, uint64_t sum_xy, uint64_t n_features,
                           double *pearson, double *cosine)
{
    typedef __int128 i128;
    const i128 G = (i128)n_features;
    const i128 num = G * (i128)sum_xy - (i128)umis_full * (i128)umis;
    const i128 dx = G * (i128)sum_xx - (i128)umis_full * (i128)umis_full, dy = G * (i128)sum_yy - (i128)umis * (i128)umis;
    int defined = 0;
    if (dx > 0 && dy > 0) {                                 /* (never negative for counts over G genes: Cauchy-Schwarz) */
        if (pearson) *pearson = (double)num / (sqrt((double)dx) * sqrt((double)dy));
        defined |= 1;
    }
    if (sum_xx && sum_yy) {
        if (cosine) *cosine = (double)sum_xy / (sqrt((double)sum_xx) * sqrt((double)sum_yy));
        defined |= 2;
    }
    return defined;
}

const char *fastf_fidelity_header(void) { return "barcode\tumis_full\tumis\tgenes_full\tgenes\tsum_xx\tsum_yy\tsum_xy\tpearson\tcosine\n"; }

int fastf_fidelity_row(const char *barcode, uint64_t umis_full, uint64_t umis, uint64_t genes_full, uint64_t genes, uint64_t sum_xx,
                       uint64_t sum_yy, uint64_t sum_xy, uint64_t n_features, char *buf, size_t cap)
{
    if (!barcode || !buf) return fastf_res_err("null argument");
    double p = 0.0, c = 0.0;
    const int defined = fastf_fidelity_metrics(umis_full, umis, sum_xx, sum_yy, sum_xy, n_features, &p, &c);
    char ps[40], cs[40];
    if (defined & 1) snprintf(ps, sizeof ps, "%.6f", p); else snprintf(ps, sizeof ps, "NA");
    if (defined & 2) snprintf(cs, sizeof cs, "%.6f", c); else snprintf(cs, sizeof cs, "NA");
    const int n = snprintf(buf, cap, "%s\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%s\t%s\n", barcode, (unsigned long long)umis_full, (unsigned long long)umis,
                           (unsigned long long)genes_full, (unsigned long long)genes, (unsigned long long)sum_xx, (unsigned long long)sum_yy,
                           (unsigned long long)sum_xy, ps, cs);
    return (n < 0 || (size_t)n >= cap) ? fastf_res_err("fidelity row too long") : 0;
}

static int cmp_dbl(const void *a, const void *b) { const double x = *(const double *)a, y = *(const double *)b; return x < y ? -1 : x > y; }
/* the rule of median_u64 on ascending values */
static double median_sorted(const double *v, size_t n) { return (n & 1) ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2.0; }

int fastf_fidelity_summary_row(float rate_cell, float rate_depth, uint64_t list_value, uint32_t seed, const uint64_t *umis_full,
                               const uint64_t *umis, const uint32_t *genes_full, const uint32_t *genes, const uint64_t *sum_xx,
                               const uint64_t *sum_yy, const uint64_t *sum_xy, uint32_t n_cells, uint64_t n_features, char *buf, size_t cap)
{
    if (!buf || (n_cells && (!umis_full || !umis || !genes_full || !genes || !sum_xx || !sum_yy || !sum_xy))) return fastf_res_err("null argument");
    double *pe = (double *)malloc(((size_t)n_cells + 1) * 2 * sizeof *pe), *co = pe ? pe + n_cells + 1 : NULL;
    if (!pe) return fastf_res_err("out of memory");
    size_t nd = 0;
    uint64_t su = 0, suf = 0, sg = 0, sgf = 0;
    for (uint32_t k = 0; k < n_cells; k++) {
        double p = 0.0, c = 0.0;
        su += umis[k]; suf += umis_full[k]; sg += genes[k]; sgf += genes_full[k];
        if (fastf_fidelity_metrics(umis_full[k], umis[k], sum_xx[k], sum_yy[k], sum_xy[k], n_features, &p, &c) & 1) { pe[nd] = p; co[nd] = c; nd++; }
    }
    char f[6][40];
    if (nd) {
        qsort(pe, nd, sizeof *pe, cmp_dbl);
        qsort(co, nd, sizeof *co, cmp_dbl);
        double sum = 0.0;
        for (size_t k = 0; k < nd; k++) sum += pe[k];
        snprintf(f[0], sizeof f[0], "%.6f", median_sorted(pe, nd));
        snprintf(f[1], sizeof f[1], "%.6f", pe[(size_t)floor(0.1 * (double)(nd - 1))]);
        snprintf(f[2], sizeof f[2], "%.6f", sum / (double)nd);
        snprintf(f[3], sizeof f[3], "%.6f", median_sorted(co, nd));
    } else for (int k = 0; k < 4; k++) snprintf(f[k], sizeof f[k], "NA");
    free(pe);
    if (suf) snprintf(f[4], sizeof f[4], "%.6f", (double)su / (double)suf); else snprintf(f[4], sizeof f[4], "NA");
    if (sgf) snprintf(f[5], sizeof f[5], "%.6f", (double)sg / (double)sgf); else snprintf(f[5], sizeof f[5], "NA");
    char second[32];
    if (list_value) snprintf(second, sizeof second, "%llu", (unsigned long long)list_value);
    else snprintf(second, sizeof second, "%.3f", (double)rate_depth);
    const int n = snprintf(buf, cap, "%.3f\t%s\t%u\t%u\t%zu\t%s\t%s\t%s\t%s\t%s\t%s\n", (double)rate_cell, second, seed, n_cells, nd, f[0], f[1], f[2], f[3], f[4], f[5]);
    return (n < 0 || (size_t)n >= cap) ? fastf_res_err("summary row too long") : 0;
}

/* ------------------------------------------------------------------ */
/* --gene-fidelity: the host twin, the metrics, the rows, the ranking   */
/* ------------------------------------------------------------------ */
/* the host form of the device calls partner_counts + gene_moments + gene_summary on both row sets: the walk of
 * fastf_fidelity_from_coo, every sum kept per gene */
int fastf_gene_fidelity_from_coo(const fastf_coo_t *full, const fastf_coo_t *point, uint32_t n_features, uint64_t *sum_x, uint64_t *sum_y,
                                 uint64_t *cells_full, uint64_t *cells, uint64_t *sum_xx, uint64_t *sum_yy, uint64_t *sum_xy)
{
    if (!full || !point || (n_features && (!sum_x || !sum_y || !cells_full || !cells || !sum_xx || !sum_yy || !sum_xy)) ||
        (point->nnz && (!point->feature || !point->cell || !point->count)) || (full->nnz && (!full->feature || !full->cell || !full->count)))
        return fastf_res_err("null argument");
    uint64_t *const all[7] = {sum_x, sum_y, cells_full, cells, sum_xx, sum_yy, sum_xy};
    for (int k = 0; k < 7; k++) memset(all[k], 0, (size_t)n_features * sizeof(uint64_t));
    for (size_t j = 0; j < full->nnz; j++) {
        const uint32_t g = full->feature[j] - 1u;
        if (g >= n_features) continue;
        const uint64_t x = full->count[j];
        sum_x[g] += x; cells_full[g] += x >= 1; sum_xx[g] += x * x;
    }
    size_t j = 0;
    for (size_t i = 0; i < point->nnz; i++) {
        const uint64_t key = ((uint64_t)point->cell[i] << 32) | point->feature[i];
        while (j < full->nnz && (((uint64_t)full->cell[j] << 32) | full->feature[j]) < key) j++;
        if (j == full->nnz || full->cell[j] != point->cell[i] || full->feature[j] != point->feature[i])
            return fastf_res_err("gene fidelity: point row %zu (cell %u, feature %u) has no partner among the full rows (device error bits 0x%x)", i, point->cell[i],
                          point->feature[i], FASTF_ERR_NO_PARTNER);
        const uint32_t g = point->feature[i] - 1u;
        if (g >= n_features) continue;
        const uint64_t y = point->count[i];
        sum_y[g] += y; cells[g] += y >= 1; sum_yy[g] += y * y; sum_xy[g] += (uint64_t)full->count[j] * y;
    }
    return 0;
}

int fastf_gene_fidelity_metrics(uint64_t n_cells, uint64_t sum_x, uint64_t sum_y, uint64_t sum_xx, uint64_t sum_yy, uint64_t sum_xy,
                                double *pearson, double *disp_full, double *disp)
{
    typedef __int128 i128;
    const i128 n = (i128)n_cells;
    const i128 num = n * (i128)sum_xy - (i128)sum_x * (i128)sum_y;
    const i128 dx = n * (i128)sum_xx - (i128)sum_x * (i128)sum_x, dy = n * (i128)sum_yy - (i128)sum_y * (i128)sum_y;
    int defined = 0;
    if (dx > 0 && dy > 0) {                                 /* (never negative for counts over n cells: Cauchy-Schwarz) */
        if (pearson) *pearson = (double)num / (sqrt((double)dx) * sqrt((double)dy));
        defined |= 1;
    }
    if (n_cells >= 2 && sum_x) {
        if (disp_full) *disp_full = (double)dx / ((double)(n_cells - 1) * (double)sum_x);
        defined |= 2;
    }
    if (n_cells >= 2 && sum_y) {
        if (disp) *disp = (double)dy / ((double)(n_cells - 1) * (double)sum_y);
        defined |= 4;
    }
    return defined;
}

const char *fastf_gene_fidelity_header(void) { return "feature\tsum_x\tsum_y\tcells_full\tcells\tsum_xx\tsum_yy\tsum_xy\tpearson\tdisp_full\tdisp\n"; }

int fastf_gene_fidelity_row(const char *feature, uint64_t n_cells, uint64_t sum_x, uint64_t sum_y, uint64_t cells_full, uint64_t cells, uint64_t sum_xx,
                            uint64_t sum_yy, uint64_t sum_xy, char *buf, size_t cap)
{
    if (!feature || !buf) return fastf_res_err("null argument");
    double v[3] = {0.0, 0.0, 0.0};
    const int defined = fastf_gene_fidelity_metrics(n_cells, sum_x, sum_y, sum_xx, sum_yy, sum_xy, &v[0], &v[1], &v[2]);
    char f[3][48];
    for (int k = 0; k < 3; k++) if (defined & (1 << k)) snprintf(f[k], sizeof f[k], "%.6f", v[k]); else snprintf(f[k], sizeof f[k], "NA");
    const int n = snprintf(buf, cap, "%s\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%s\t%s\t%s\n", feature, (unsigned long long)sum_x, (unsigned long long)sum_y,
                           (unsigned long long)cells_full, (unsigned long long)cells, (unsigned long long)sum_xx, (unsigned long long)sum_yy,
                           (unsigned long long)sum_xy, f[0], f[1], f[2]);
    return (n < 0 || (size_t)n >= cap) ? fastf_res_err("gene fidelity row too long") : 0;
}

/* the ranking of the highly variable genes: descending value, ties by ascending feature index */
typedef struct { double v; uint32_t g; } hvg_item;
static int cmp_hvg(const void *a, const void *b)
{
    const hvg_item *x = (const hvg_item *)a, *y = (const hvg_item *)b;
    if (x->v != y->v) return x->v > y->v ? -1 : 1;
    return x->g < y->g ? -1 : x->g > y->g;
}

/* the dispersion of (sum, sum_sq) is disp_full of fastf_gene_fidelity_metrics — and its disp, which is the same expression on the other
 * pair of sums.  Out of memory: UINT32_MAX, and *n_defined likewise */
uint32_t fastf_hvg_rank(uint32_t n_cells, const uint64_t *sum, const uint64_t *sum_sq, uint32_t n_features, uint32_t *genes, uint32_t *n_defined)
{
    hvg_item *A = (hvg_item *)malloc(((size_t)n_features + 1) * sizeof *A);
    if (!A) { if (n_defined) *n_defined = UINT32_MAX; return UINT32_MAX; }
    size_t na = 0;
    for (uint32_t g = 0; g < n_features; g++) {
        double d = 0.0;
        if (fastf_gene_fidelity_metrics(n_cells, sum[g], 0, sum_sq[g], 0, 0, NULL, &d, NULL) & 2) { A[na].v = d; A[na].g = g; na++; }
    }
    qsort(A, na, sizeof *A, cmp_hvg);
    const uint32_t K = (uint32_t)(na < FASTF_HVG_TOP ? na : FASTF_HVG_TOP);
    if (genes) for (uint32_t k = 0; k < K; k++) genes[k] = A[k].g;
    if (n_defined) *n_defined = (uint32_t)na;
    free(A);
    return K;
}

int fastf_gene_fidelity_summary_row(float rate_cell, float rate_depth, uint64_t list_value, uint32_t seed, uint32_t n_cells, const uint64_t *sum_x,
                                    const uint64_t *sum_y, const uint64_t *sum_xx, const uint64_t *sum_yy, const uint64_t *sum_xy, uint32_t n_features,
                                    char *buf, size_t cap)
{
    if (!buf || (n_features && (!sum_x || !sum_y || !sum_xx || !sum_yy || !sum_xy))) return fastf_res_err("null argument");
    double *pe = (double *)malloc(((size_t)n_features + 1) * sizeof *pe);
    uint32_t *A = (uint32_t *)malloc(2 * FASTF_HVG_TOP * sizeof *A), *B = A ? A + FASTF_HVG_TOP : NULL;
    uint8_t *inA = (uint8_t *)calloc((size_t)n_features + 1, 1);
    if (!pe || !A || !inA) { free(pe); free(A); free(inA); return fastf_res_err("out of memory"); }
    size_t nd = 0;
    uint32_t genes_full = 0, nb = 0;
    for (uint32_t g = 0; g < n_features; g++) {
        double p = 0.0;
        const int defined = fastf_gene_fidelity_metrics(n_cells, sum_x[g], sum_y[g], sum_xx[g], sum_yy[g], sum_xy[g], &p, NULL, NULL);
        genes_full += sum_x[g] > 0;
        if (defined & 1) pe[nd++] = p;
    }
    const size_t K = fastf_hvg_rank(n_cells, sum_x, sum_xx, n_features, A, NULL);
    (void)fastf_hvg_rank(n_cells, sum_y, sum_yy, n_features, B, &nb);
    const size_t KB = nb < K ? nb : K;
    size_t both = 0;
    if (K == UINT32_MAX || nb == UINT32_MAX) { free(pe); free(A); free(inA); return fastf_res_err("out of memory"); }
    for (size_t k = 0; k < K; k++) inA[A[k]] = 1;
    for (size_t k = 0; k < KB; k++) both += inA[B[k]];
    char f[4][40];
    if (nd) {
        qsort(pe, nd, sizeof *pe, cmp_dbl);
        double sum = 0.0;
        for (size_t k = 0; k < nd; k++) sum += pe[k];
        snprintf(f[0], sizeof f[0], "%.6f", median_sorted(pe, nd));
        snprintf(f[1], sizeof f[1], "%.6f", pe[(size_t)floor(0.1 * (double)(nd - 1))]);
        snprintf(f[2], sizeof f[2], "%.6f", sum / (double)nd);
    } else for (int k = 0; k < 3; k++) snprintf(f[k], sizeof f[k], "NA");
    if (K) snprintf(f[3], sizeof f[3], "%.6f", (double)both / (double)K); else snprintf(f[3], sizeof f[3], "NA");
    free(pe); free(A); free(inA);
    char second[32];
    if (list_value) snprintf(second, sizeof second, "%llu", (unsigned long long)list_value);
    else snprintf(second, sizeof second, "%.3f", (double)rate_depth);
    const int n = snprintf(buf, cap, "%.3f\t%s\t%u\t%u\t%u\t%zu\t%s\t%s\t%s\t%zu\t%s\n", (double)rate_cell, second, seed, n_cells, genes_full, nd, f[0], f[1], f[2], K, f[3]);
    return (n < 0 || (size_t)n >= cap) ? fastf_res_err("summary row too long") : 0;
}

/* ------------------------------------------------------------------ */
/* --neighbors: the host twin, the rows                                 */
/* ------------------------------------------------------------------ */
void fastf_neighbors_pad(uint32_t n_cells, uint32_t K, uint32_t *n_pad, uint32_t *K_pad)
{
    if (n_pad) *n_pad = n_cells ? (n_cells + 127u) & ~127u : 128u;
    if (K_pad) *K_pad = K ? (K + 31u) & ~31u : 32u;
}

int fastf_neighbors_check_norm(uint64_t max_norm)
{
    if (max_norm >> 42)
        return fastf_res_err("FASTF_ERR_NEIGHBOR_NORM: a cell's squared norm over the highly variable genes is %llu, 2^42 or more: the 128-bit order of --neighbors does not hold it",
                      (unsigned long long)max_norm);
    return 0;
}

int fastf_neighbors_slot_map(const uint32_t *genes, uint32_t K, uint32_t n_features, uint16_t *slot_map)
{
    if (!slot_map || (K && !genes)) return fastf_res_err("null argument");
    if (K > FASTF_HVG_TOP) return fastf_res_err("neighbors: %u genes, at most %u", K, FASTF_HVG_TOP);
    for (size_t f = 0; f <= n_features; f++) slot_map[f] = FASTF_NEIGHBORS_NONE;
    for (uint32_t k = 0; k < K; k++) {
        if (genes[k] >= n_features || slot_map[genes[k] + 1] != FASTF_NEIGHBORS_NONE) return fastf_res_err("neighbors: gene %u of the set is outside the list or named twice", genes[k]);
        slot_map[genes[k] + 1] = (uint16_t)k;
    }
    return 0;
}

uint32_t fastf_neighbors_shared(const uint32_t *a, uint32_t na, const uint32_t *b, uint32_t nb)
{
    uint32_t x = 0, y = 0, both = 0;
    while (x < na && y < nb) {
        const uint32_t va = a[x], vb = b[y];
        both += va == vb; x += va <= vb; y += vb <= va;
    }
    return both;
}

typedef unsigned __int128 u128;
/* j precedes l among the candidates of one query cell */
static int nbr_precedes(uint64_t dj, uint64_t nj, uint32_t j, uint64_t dl, uint64_t nl, uint32_t l)
{
    const u128 a = (u128)dj * dj * nl, b = (u128)dl * dl * nj;
    return a > b || (a == b && j < l);
}
static int cmp_u32(const void *a, const void *b) { const uint32_t x = *(const uint32_t *)a, y = *(const uint32_t *)b; return x < y ? -1 : x > y; }

/* the rows of a COO matrix with a slot in slot_map, cell by cell (a counting sort by cell): rs, rv = slot and count of the rows
 * start[c] .. start[c + 1] of cell c (0-based), nn[c] the squared norm (saturating), max_norm their maximum.  Rows in any order */
typedef struct { size_t *start; uint32_t *rs, *rv; uint64_t *nn, max_norm; } nbr_rows_t;
static void nbr_rows_free(nbr_rows_t *o) { free(o->start); free(o->rs); free(o->rv); free(o->nn); memset(o, 0, sizeof *o); }
static int nbr_rows_build(const fastf_coo_t *m, uint32_t n_cells, const uint16_t *slot_map, uint32_t n_features, nbr_rows_t *o)
{
    memset(o, 0, sizeof *o);
    o->start = (size_t *)calloc((size_t)n_cells + 2, sizeof *o->start);
    o->nn = (uint64_t *)calloc((size_t)n_cells + 1, sizeof *o->nn);
    if (!o->start || !o->nn) return fastf_res_err("out of memory");
    size_t *const start = o->start;
    size_t kept = 0;
    for (size_t r = 0; r < m->nnz; r++) {
        const uint32_t c = m->cell[r] - 1u, f = m->feature[r];
        if (c >= n_cells || f - 1u >= n_features || slot_map[f] >= FASTF_HVG_TOP) continue;
        start[c + 2]++; kept++;
    }
    for (uint32_t c = 0; c < n_cells; c++) start[c + 2] += start[c + 1];
    o->rs = (uint32_t *)malloc((kept + 1) * sizeof *o->rs); o->rv = (uint32_t *)malloc((kept + 1) * sizeof *o->rv);
    if (!o->rs || !o->rv) return fastf_res_err("out of memory");
    for (size_t r = 0; r < m->nnz; r++) {
        const uint32_t c = m->cell[r] - 1u, f = m->feature[r];
        if (c >= n_cells || f - 1u >= n_features || slot_map[f] >= FASTF_HVG_TOP) continue;
        const size_t at = start[c + 1]++;
        o->rs[at] = slot_map[f]; o->rv[at] = m->count[r];
        const u128 sq = (u128)o->nn[c] + (u128)m->count[r] * m->count[r];
        o->nn[c] = sq >> 64 ? UINT64_MAX : (uint64_t)sq;
    }
    for (uint32_t c = 0; c < n_cells; c++) if (o->nn[c] > o->max_norm) o->max_norm = o->nn[c];      /* (start[c] .. start[c + 1]: the rows of cell c) */
    return 0;
}

/* candidate (d, j) into out[0 .. *have) — kept in the order of the definition, best first, bd[] their d, nn[] the candidates' norms; a
 * later cell never precedes an equal earlier one */
static void nbr_list_insert(uint32_t *out, uint64_t *bd, uint32_t *have, uint32_t k, const uint64_t *nn, uint64_t d, uint32_t j)
{
    uint32_t at = *have;
    while (at > 0 && nbr_precedes(d, nn[j], j, bd[at - 1], nn[out[at - 1]], out[at - 1])) at--;
    if (at >= k) return;
    const uint32_t last = *have < k ? *have : k - 1;
    for (uint32_t s = last; s > at; s--) { out[s] = out[s - 1]; bd[s] = bd[s - 1]; }
    out[at] = j; bd[at] = d;
    if (*have < k) ++*have;
}

int fastf_neighbors_from_coo(const fastf_coo_t *m, uint32_t n_cells, const uint16_t *slot_map, uint32_t n_features, uint32_t k,
                             uint32_t *idx, uint32_t *cnt, uint64_t *norms)
{
    if (!m || !slot_map || (n_cells && (!idx || !cnt)) || (m->nnz && (!m->feature || !m->cell || !m->count))) return fastf_res_err("null argument");
    if (k < 1 || k > FASTF_NEIGHBORS_MAX_K) return fastf_res_err("neighbors: k = %u, from 1 to %u", k, FASTF_NEIGHBORS_MAX_K);
    int rc = 1;
    nbr_rows_t R;
    uint64_t *vec = (uint64_t *)calloc(FASTF_HVG_TOP, sizeof *vec), *bd = (uint64_t *)malloc(FASTF_NEIGHBORS_MAX_K * sizeof *bd);
    if (nbr_rows_build(m, n_cells, slot_map, n_features, &R)) goto done;
    if (!vec || !bd) { fastf_res_err("out of memory"); goto done; }
    if (fastf_neighbors_check_norm(R.max_norm)) goto done;
    for (uint32_t i = 0; i < n_cells; i++) {
        uint32_t *const out = idx + (size_t)i * k;
        uint32_t have = 0;
        for (size_t r = R.start[i]; r < R.start[i + 1]; r++) vec[R.rs[r]] += R.rv[r];
        for (uint32_t j = 0; j < n_cells; j++) {
            if (j == i) continue;
            uint64_t d = 0;
            for (size_t r = R.start[j]; r < R.start[j + 1]; r++) d += vec[R.rs[r]] * R.rv[r];
            if (d) nbr_list_insert(out, bd, &have, k, R.nn, d, j);
        }
        for (size_t r = R.start[i]; r < R.start[i + 1]; r++) vec[R.rs[r]] = 0;
        qsort(out, have, sizeof *out, cmp_u32);
        for (uint32_t s = have; s < k; s++) out[s] = UINT32_MAX;
        cnt[i] = have;
        if (norms) norms[i] = R.nn[i];
    }
    rc = 0;
done:
    nbr_rows_free(&R); free(vec); free(bd);
    return rc;
}

const char *fastf_neighbors_header(void) { return "barcode\tk_full\tk_point\tshared\toverlap\n"; }

int fastf_neighbors_row(const char *barcode, uint32_t k_full, uint32_t k_point, uint32_t shared, char *buf, size_t cap)
{
    if (!barcode || !buf) return fastf_res_err("null argument");
    char f[48];
    if (k_full) snprintf(f, sizeof f, "%.6f", (double)shared / (double)k_full); else snprintf(f, sizeof f, "NA");
    const int n = snprintf(buf, cap, "%s\t%u\t%u\t%u\t%s\n", barcode, k_full, k_point, shared, f);
    return (n < 0 || (size_t)n >= cap) ? fastf_res_err("neighbors row too long") : 0;
}

int fastf_neighbors_summary_row(float rate_cell, float rate_depth, uint64_t list_value, uint32_t seed, uint32_t n_cells, uint32_t hvg_k, uint32_t k,
                                const uint32_t *k_full, const uint32_t *k_point, const uint32_t *shared, char *buf, size_t cap)
{
    if (!buf || (n_cells && (!k_full || !k_point || !shared))) return fastf_res_err("null argument");
    double *ov = (double *)malloc(((size_t)n_cells + 1) * sizeof *ov);
    if (!ov) return fastf_res_err("out of memory");
    size_t nd = 0;
    uint64_t kp = 0;
    for (uint32_t c = 0; c < n_cells; c++) {
        kp += k_point[c];
        if (k_full[c]) ov[nd++] = (double)shared[c] / (double)k_full[c];
    }
    char f[4][40];
    if (nd) {
        qsort(ov, nd, sizeof *ov, cmp_dbl);
        double sum = 0.0;
        for (size_t c = 0; c < nd; c++) sum += ov[c];
        snprintf(f[0], sizeof f[0], "%.6f", median_sorted(ov, nd));
        snprintf(f[1], sizeof f[1], "%.6f", ov[(size_t)floor(0.1 * (double)(nd - 1))]);
        snprintf(f[2], sizeof f[2], "%.6f", sum / (double)nd);
    } else for (int c = 0; c < 3; c++) snprintf(f[c], sizeof f[c], "NA");
    if (n_cells) snprintf(f[3], sizeof f[3], "%.6f", (double)kp / (double)n_cells); else snprintf(f[3], sizeof f[3], "NA");
    free(ov);
    char second[32];
    if (list_value) snprintf(second, sizeof second, "%llu", (unsigned long long)list_value);
    else snprintf(second, sizeof second, "%.3f", (double)rate_depth);
    const int n = snprintf(buf, cap, "%.3f\t%s\t%u\t%u\t%u\t%u\t%zu\t%s\t%s\t%s\t%s\n", (double)rate_cell, second, seed, n_cells, hvg_k, k, nd, f[0], f[1], f[2], f[3]);
    return (n < 0 || (size_t)n >= cap) ? fastf_res_err("summary row too long") : 0;
}

/* ------------------------------------------------------------------ */
/* --mapping: the host twin, the rows                                   */
/* ------------------------------------------------------------------ */
int fastf_mapping_from_coo(const fastf_coo_t *full, const fastf_coo_t *point, uint32_t n_cells, const uint16_t *slot_map, uint32_t n_features, uint32_t k,
                           uint32_t *idx, uint32_t *cnt, uint64_t *self_dot, uint32_t *self_rank)
{
    if (!full || !point || !slot_map || (n_cells && (!idx || !cnt || !self_dot || !self_rank)) || (full->nnz && (!full->feature || !full->cell || !full->count)) ||
        (point->nnz && (!point->feature || !point->cell || !point->count))) return fastf_res_err("null argument");
    if (k < 1 || k > FASTF_NEIGHBORS_MAX_K) return fastf_res_err("mapping: k = %u, from 1 to %u", k, FASTF_NEIGHBORS_MAX_K);
    int rc = 1;
    nbr_rows_t X, Y;
    uint64_t *vec = (uint64_t *)calloc(FASTF_HVG_TOP, sizeof *vec), *bd = (uint64_t *)malloc(FASTF_NEIGHBORS_MAX_K * sizeof *bd);
    uint64_t *e = (uint64_t *)malloc(((size_t)n_cells + 1) * sizeof *e);
    memset(&Y, 0, sizeof Y);
    if (nbr_rows_build(full, n_cells, slot_map, n_features, &X) || nbr_rows_build(point, n_cells, slot_map, n_features, &Y)) goto done;
    if (!vec || !bd || !e) { fastf_res_err("out of memory"); goto done; }
    if (fastf_neighbors_check_norm(X.max_norm) || fastf_neighbors_check_norm(Y.max_norm)) goto done;
    for (uint32_t i = 0; i < n_cells; i++) {
        uint32_t *const out = idx + (size_t)i * k;
        uint32_t have = 0, rank = 0;
        for (size_t r = Y.start[i]; r < Y.start[i + 1]; r++) vec[Y.rs[r]] += Y.rv[r];
        for (uint32_t j = 0; j < n_cells; j++) {
            uint64_t d = 0;
            for (size_t r = X.start[j]; r < X.start[j + 1]; r++) d += vec[X.rs[r]] * X.rv[r];
            e[j] = d;
        }
        for (size_t r = Y.start[i]; r < Y.start[i + 1]; r++) vec[Y.rs[r]] = 0;
        const uint64_t sd = e[i];
        for (uint32_t j = 0; j < n_cells; j++) {
            if (j == i || !e[j]) continue;
            if (sd) rank += (uint32_t)nbr_precedes(e[j], X.nn[j], j, sd, X.nn[i], i);
            nbr_list_insert(out, bd, &have, k, X.nn, e[j], j);
        }
        qsort(out, have, sizeof *out, cmp_u32);
        for (uint32_t s = have; s < k; s++) out[s] = UINT32_MAX;
        cnt[i] = have; self_dot[i] = sd; self_rank[i] = sd ? rank : FASTF_MAPPING_NO_RANK;
    }
    rc = 0;
done:
    nbr_rows_free(&X); nbr_rows_free(&Y); free(vec); free(bd); free(e);
    return rc;
}

const char *fastf_mapping_header(void) { return "barcode\tself_dot\tself_rank\tk_map\tk_full\thood\tpred_map\n"; }

int fastf_mapping_row(const char *barcode, uint64_t self_dot, uint32_t self_rank, uint32_t k_map, uint32_t k_full, uint32_t hood, const char *pred_map,
                      char *buf, size_t cap)
{
    if (!barcode || !buf) return fastf_res_err("null argument");
    char f[24];
    if (self_rank != FASTF_MAPPING_NO_RANK) snprintf(f, sizeof f, "%u", self_rank); else snprintf(f, sizeof f, "NA");
    const int n = snprintf(buf, cap, "%s\t%llu\t%s\t%u\t%u\t%u\t%s\n", barcode, (unsigned long long)self_dot, f, k_map, k_full, hood, pred_map ? pred_map : "NA");
    return (n < 0 || (size_t)n >= cap) ? fastf_res_err("mapping row too long") : 0;
}

int fastf_mapping_summary_row(float rate_cell, float rate_depth, uint64_t list_value, uint32_t seed, uint32_t n_cells, uint32_t hvg_k, uint32_t k,
                              const uint64_t *self_dot, const uint32_t *self_rank, const uint32_t *k_full, const uint32_t *hood, const uint8_t *lab,
                              const uint8_t *same_map, const uint8_t *labelled_map, char *buf, size_t cap)
{
    if (!buf || (n_cells && (!self_dot || !self_rank || !k_full || !hood)) || (lab && n_cells && (!same_map || !labelled_map))) return fastf_res_err("null argument");
    double *rk = (double *)malloc(((size_t)n_cells + 1) * sizeof *rk);
    if (!rk) return fastf_res_err("out of memory");
    size_t nd = 0, top1 = 0, topk = 0, n_hood = 0;
    uint64_t cells_labelled = 0, same = 0, labelled = 0;
    double hood_sum = 0.0;
    for (uint32_t c = 0; c < n_cells; c++) {
        if (self_dot[c] > 0) { rk[nd++] = (double)self_rank[c]; top1 += self_rank[c] == 0; topk += self_rank[c] < k; }
        if (k_full[c]) { hood_sum += (double)hood[c] / (double)k_full[c]; n_hood++; }
        if (lab && lab[c]) { cells_labelled++; same += same_map[c]; labelled += labelled_map[c]; }
    }
    char f[7][40];
    if (nd) {
        qsort(rk, nd, sizeof *rk, cmp_dbl);
        snprintf(f[0], sizeof f[0], "%.6f", (double)top1 / (double)nd);
        snprintf(f[1], sizeof f[1], "%.6f", (double)topk / (double)nd);
        snprintf(f[2], sizeof f[2], "%.6f", median_sorted(rk, nd));
        snprintf(f[3], sizeof f[3], "%.0f", rk[(size_t)floor(0.9 * (double)(nd - 1))]);
    } else for (int c = 0; c < 4; c++) snprintf(f[c], sizeof f[c], "NA");
    if (n_hood) snprintf(f[4], sizeof f[4], "%.6f", hood_sum / (double)n_hood); else snprintf(f[4], sizeof f[4], "NA");
    if (lab) snprintf(f[5], sizeof f[5], "%llu", (unsigned long long)cells_labelled); else snprintf(f[5], sizeof f[5], "NA");
    if (lab && labelled) snprintf(f[6], sizeof f[6], "%.6f", (double)same / (double)labelled); else snprintf(f[6], sizeof f[6], "NA");
    free(rk);
    char second[32];
    if (list_value) snprintf(second, sizeof second, "%llu", (unsigned long long)list_value);
    else snprintf(second, sizeof second, "%.3f", (double)rate_depth);
    const int n = snprintf(buf, cap, "%.3f\t%s\t%u\t%u\t%u\t%u\t%zu\t%s\t%s\t%s\t%s\t%s\t%s\t%s\n", (double)rate_cell, second, seed, n_cells, hvg_k, k, nd, f[0], f[1], f[2], f[3],
                           f[4], f[5], f[6]);
    return (n < 0 || (size_t)n >= cap) ? fastf_res_err("summary row too long") : 0;
}

/* ------------------------------------------------------------------ */
/* --labels: the host twin, the rows                                    */
/* ------------------------------------------------------------------ */
int fastf_label_votes(const uint32_t *idx, const uint32_t *cnt, const uint8_t *lab, uint32_t n_cells, uint32_t k, uint32_t n_labels,
                      uint8_t *pred, uint8_t *same, uint8_t *labelled, uint32_t *conf)
{
    if (k < 1 || k > FASTF_NEIGHBORS_MAX_K) return fastf_res_err("label votes: k = %u, from 1 to %u", k, FASTF_NEIGHBORS_MAX_K);
    if (n_labels > FASTF_LABELS_MAX) return fastf_res_err("label votes: %u labels, at most %u", n_labels, FASTF_LABELS_MAX);
    if ((n_labels && !conf) || (n_cells && (!idx || !cnt || !lab || !pred || !same || !labelled))) return fastf_res_err("null argument");
    if (n_labels) memset(conf, 0, (size_t)n_labels * (n_labels + 1) * sizeof *conf);
    for (uint32_t i = 0; i < n_cells; i++) {
        uint32_t votes[FASTF_LABELS_MAX + 1] = {0}, all = 0, best = 0;
        const uint32_t c = cnt[i] < k ? cnt[i] : k, own = lab[i] <= n_labels ? lab[i] : 0;
        for (uint32_t s = 0; s < c; s++) {
            const uint32_t j = idx[(size_t)i * k + s];
            const uint32_t l = j < n_cells && lab[j] <= n_labels ? lab[j] : 0;
            if (l) { votes[l]++; all++; }
        }
        for (uint32_t l = 1; l <= n_labels; l++) if (votes[l] > votes[best]) best = l;     /* (votes[0] == 0: a first l needs one vote; ties keep the smaller l) */
        pred[i] = (uint8_t)best; same[i] = (uint8_t)(own ? votes[own] : 0); labelled[i] = (uint8_t)all;
        if (own) conf[(size_t)(own - 1) * (n_labels + 1) + best]++;
    }
    return 0;
}

const char *fastf_labels_header(void) { return "barcode\tlabel\tpred_full\tpred_point\tsame_full\tlabelled_full\tsame_point\tlabelled_point\n"; }

int fastf_labels_row(const char *barcode, const char *label, const char *pred_full, const char *pred_point, uint32_t same_full, uint32_t labelled_full,
                     uint32_t same_point, uint32_t labelled_point, char *buf, size_t cap)
{
    if (!barcode || !label || !pred_full || !pred_point || !buf) return fastf_res_err("null argument");
    const int n = snprintf(buf, cap, "%s\t%s\t%s\t%s\t%u\t%u\t%u\t%u\n", barcode, label, pred_full, pred_point, same_full, labelled_full, same_point, labelled_point);
    return (n < 0 || (size_t)n >= cap) ? fastf_res_err("labels row too long") : 0;
}

int fastf_label_confusion_header(const char *const *names, uint32_t n_labels, char *buf, size_t cap)
{
    if (!buf || (n_labels && !names)) return fastf_res_err("null argument");
    int n = snprintf(buf, cap, "label\tcells\tNA");
    for (uint32_t l = 1; l <= n_labels && n >= 0 && (size_t)n < cap; l++) {
        const int m = snprintf(buf + n, cap - (size_t)n, "\t%s", names[l]);
        n = m < 0 ? m : n + m;
    }
    if (n >= 0 && (size_t)n < cap) { const int m = snprintf(buf + n, cap - (size_t)n, "\n"); n = m < 0 ? m : n + m; }
    return (n < 0 || (size_t)n >= cap) ? fastf_res_err("confusion header too long") : 0;
}

int fastf_label_confusion_row(const char *label, uint32_t cells, const uint32_t *conf_row, uint32_t n_labels, char *buf, size_t cap)
{
    if (!label || !conf_row || !buf) return fastf_res_err("null argument");
    int n = snprintf(buf, cap, "%s\t%u", label, cells);
    for (uint32_t b = 0; b <= n_labels && n >= 0 && (size_t)n < cap; b++) {
        const int m = snprintf(buf + n, cap - (size_t)n, "\t%u", conf_row[b]);
        n = m < 0 ? m : n + m;
    }
    if (n >= 0 && (size_t)n < cap) { const int m = snprintf(buf + n, cap - (size_t)n, "\n"); n = m < 0 ? m : n + m; }
    return (n < 0 || (size_t)n >= cap) ? fastf_res_err("confusion row too long") : 0;
}

static void lab_ratio(char *f, size_t cap, uint64_t num, uint64_t den)
{
    if (den) snprintf(f, cap, "%.6f", (double)num / (double)den); else snprintf(f, cap, "NA");
}
static void lab_second(char *f, size_t cap, float rate_depth, uint64_t list_value)
{
    if (list_value) snprintf(f, cap, "%llu", (unsigned long long)list_value); else snprintf(f, cap, "%.3f", (double)rate_depth);
}

int fastf_labels_summary_row(float rate_cell, float rate_depth, uint64_t list_value, uint32_t seed, uint32_t n_cells, uint32_t k, uint32_t n_labels,
                             const uint8_t *lab, const uint8_t *pred_full, const uint8_t *pred_point, const uint8_t *same_full, const uint8_t *labelled_full,
                             const uint8_t *same_point, const uint8_t *labelled_point, const uint32_t *conf_full, const uint32_t *conf_point,
                             char *buf, size_t cap)
{
    if (!buf || (n_cells && (!lab || !pred_full || !pred_point || !same_full || !labelled_full || !same_point || !labelled_point)) ||
        (n_labels && (!conf_full || !conf_point))) return fastf_res_err("null argument");
    uint64_t cells_labelled = 0, kept = 0, sf = 0, lf = 0, sp = 0, lp = 0, agree_full = 0, agree_point = 0;
    for (uint32_t i = 0; i < n_cells; i++) {
        if (!lab[i] || lab[i] > n_labels) continue;
        cells_labelled++;
        kept += pred_full[i] == lab[i] && pred_point[i] == lab[i];
        sf += same_full[i]; lf += labelled_full[i]; sp += same_point[i]; lp += labelled_point[i];
    }
    for (uint32_t a = 1; a <= n_labels; a++) { agree_full += conf_full[(size_t)(a - 1) * (n_labels + 1) + a]; agree_point += conf_point[(size_t)(a - 1) * (n_labels + 1) + a]; }
    char f[5][40], second[32];
    lab_ratio(f[0], sizeof f[0], agree_full, cells_labelled); lab_ratio(f[1], sizeof f[1], agree_point, cells_labelled);
    lab_ratio(f[2], sizeof f[2], kept, agree_full); lab_ratio(f[3], sizeof f[3], sf, lf); lab_ratio(f[4], sizeof f[4], sp, lp);
    lab_second(second, sizeof second, rate_depth, list_value);
    const int n = snprintf(buf, cap, "%.3f\t%s\t%u\t%u\t%u\t%u\t%llu\t%llu\t%llu\t%s\t%s\t%s\t%s\t%s\n", (double)rate_cell, second, seed, n_cells, k, n_labels,
                           (unsigned long long)cells_labelled, (unsigned long long)agree_full, (unsigned long long)agree_point, f[0], f[1], f[2], f[3], f[4]);
    return (n < 0 || (size_t)n >= cap) ? fastf_res_err("summary row too long") : 0;
}

int fastf_label_classes_row(float rate_cell, float rate_depth, uint64_t list_value, uint32_t seed, const char *label, uint32_t a, uint32_t n_cells,
                            uint32_t n_labels, const uint8_t *lab, const uint32_t *conf_full, const uint32_t *conf_point, char *buf, size_t cap)
{
    if (!buf || !label || !conf_full || !conf_point || (n_cells && !lab)) return fastf_res_err("null argument");
    if (a < 1 || a > n_labels) return fastf_res_err("label classes: label %u, from 1 to %u", a, n_labels);
    uint64_t cells = 0, pf = 0, pp = 0;
    for (uint32_t i = 0; i < n_cells; i++) cells += lab[i] == a;
    for (uint32_t r = 0; r < n_labels; r++) { pf += conf_full[(size_t)r * (n_labels + 1) + a]; pp += conf_point[(size_t)r * (n_labels + 1) + a]; }
    char second[32];
    lab_second(second, sizeof second, rate_depth, list_value);
    const int n = snprintf(buf, cap, "%.3f\t%s\t%u\t%s\t%llu\t%u\t%u\t%llu\t%llu\n", (double)rate_cell, second, seed, label, (unsigned long long)cells,
                           conf_full[(size_t)(a - 1) * (n_labels + 1) + a], conf_point[(size_t)(a - 1) * (n_labels + 1) + a], (unsigned long long)pf, (unsigned long long)pp);
    return (n < 0 || (size_t)n >= cap) ? fastf_res_err("classes row too long") : 0;
}

/* ------------------------------------------------------------------ */
/* --pseudotime: the host twins, the rows                               */
/* ------------------------------------------------------------------ */
/* the lower median by insertion into a sorted run of at most k values */
int fastf_ptime_medians(const uint32_t *idx, const uint32_t *cnt, const uint32_t *t, uint32_t n_cells, uint32_t k, uint32_t *est, uint32_t *valued)
{
    if (k < 1 || k > FASTF_NEIGHBORS_MAX_K) return fastf_res_err("ptime medians: k = %u, from 1 to %u", k, FASTF_NEIGHBORS_MAX_K);
    if (n_cells && (!idx || !cnt || !t || !est || !valued)) return fastf_res_err("null argument");
    for (uint32_t i = 0; i < n_cells; i++) {
        uint32_t v[FASTF_NEIGHBORS_MAX_K], c = 0;
        const uint32_t slots = cnt[i] < k ? cnt[i] : k;
        for (uint32_t s = 0; s < slots; s++) {
            const uint32_t j = idx[(size_t)i * k + s];
            const uint32_t x = j < n_cells ? t[j] : 0;
            if (!x) continue;
            uint32_t at = c++;
            while (at && v[at - 1] > x) { v[at] = v[at - 1]; at--; }
            v[at] = x;
        }
        est[i] = c ? v[(c + 1) / 2 - 1] : 0; valued[i] = c;
    }
    return 0;
}

/* the definition, pair by pair */
int fastf_ptime_census(const uint32_t *est, const uint32_t *t, uint32_t n_cells, uint64_t *out)
{
    if (!out || (n_cells && (!est || !t))) return fastf_res_err("null argument");
    uint64_t conc = 0, disc = 0, tie_e = 0, tie_t = 0, tie_both = 0, cells = 0, shift = 0;
    for (uint32_t i = 0; i < n_cells; i++) {
        if (!t[i] || !est[i]) continue;
        cells++; shift += est[i] > t[i] ? est[i] - t[i] : t[i] - est[i];
        for (uint32_t j = i + 1; j < n_cells; j++) {
            if (!t[j] || !est[j]) continue;
            const int se = (est[i] > est[j]) - (est[i] < est[j]), st = (t[i] > t[j]) - (t[i] < t[j]);
            if (se * st > 0) conc++; else if (se * st < 0) disc++; else if (!se && st) tie_e++; else if (se && !st) tie_t++; else tie_both++;
        }
    }
    out[0] = conc; out[1] = disc; out[2] = tie_e; out[3] = tie_t; out[4] = tie_both; out[5] = cells; out[6] = shift;
    return 0;
}

const char *fastf_ptime_header(void) { return "barcode\trank\test_full\tvalued_full\test_point\tvalued_point\test_map\tvalued_map\n"; }

static void pt_rank(char *f, size_t cap, uint32_t v) { if (v) snprintf(f, cap, "%u", v); else snprintf(f, cap, "NA"); }

int fastf_ptime_row(const char *barcode, uint32_t rank, uint32_t est_full, uint32_t valued_full, uint32_t est_point, uint32_t valued_point,
                    uint32_t est_map, uint32_t valued_map, int mapping, char *buf, size_t cap)
{
    if (!barcode || !buf) return fastf_res_err("null argument");
    char f[5][16];
    pt_rank(f[0], sizeof f[0], rank); pt_rank(f[1], sizeof f[1], est_full); pt_rank(f[2], sizeof f[2], est_point);
    pt_rank(f[3], sizeof f[3], mapping ? est_map : 0);
    if (mapping) snprintf(f[4], sizeof f[4], "%u", valued_map); else snprintf(f[4], sizeof f[4], "NA");
    const int n = snprintf(buf, cap, "%s\t%s\t%s\t%u\t%s\t%u\t%s\t%s\n", barcode, f[0], f[1], valued_full, f[2], valued_point, f[3], f[4]);
    return (n < 0 || (size_t)n >= cap) ? fastf_res_err("pseudotime row too long") : 0;
}

/* cells conc disc tau shift of one census (no leading tab); NULL: five NA */
static int pt_census_text(char *f, size_t cap, const uint64_t *c, uint32_t cells_valued)
{
    if (!c) { const int n = snprintf(f, cap, "NA\tNA\tNA\tNA\tNA"); return n < 0 || (size_t)n >= cap; }
    const uint64_t conc = c[0], disc = c[1], tie_e = c[2], tie_t = c[3], cells = c[5], shift = c[6];
    char tau[40], sh[40];
    if (conc + disc + tie_e == 0 || conc + disc + tie_t == 0) snprintf(tau, sizeof tau, "NA");
    else snprintf(tau, sizeof tau, "%.6f", (double)(int64_t)(conc - disc) / sqrt((double)(conc + disc + tie_e) * (double)(conc + disc + tie_t)));
    if (!cells_valued || !cells) snprintf(sh, sizeof sh, "NA");
    else snprintf(sh, sizeof sh, "%.6f", (double)shift / ((double)(2 * (uint64_t)cells_valued) * (double)cells));
    const int n = snprintf(f, cap, "%llu\t%llu\t%llu\t%s\t%s", (unsigned long long)cells, (unsigned long long)conc, (unsigned long long)disc, tau, sh);
    return n < 0 || (size_t)n >= cap;
}

int fastf_ptime_summary_row(float rate_cell, float rate_depth, uint64_t list_value, uint32_t seed, uint32_t n_cells, uint32_t k, uint32_t cells_valued,
                            const uint64_t *census_full, const uint64_t *census_point, const uint64_t *census_map, char *buf, size_t cap)
{
    if (!buf || !census_full || !census_point) return fastf_res_err("null argument");
    char f[3][160], second[32];
    if (pt_census_text(f[0], sizeof f[0], census_full, cells_valued) || pt_census_text(f[1], sizeof f[1], census_point, cells_valued) ||
        pt_census_text(f[2], sizeof f[2], census_map, cells_valued)) return fastf_res_err("summary row too long");
    lab_second(second, sizeof second, rate_depth, list_value);
    const int n = snprintf(buf, cap, "%.3f\t%s\t%u\t%u\t%u\t%u\t%s\t%s\t%s\n", (double)rate_cell, second, seed, n_cells, k, cells_valued, f[0], f[1], f[2]);
    return (n < 0 || (size_t)n >= cap) ? fastf_res_err("summary row too long") : 0;
}

/* ------------------------------------------------------------------ */
/* --markers: the host twin, the ranks, the rows                        */
/* ------------------------------------------------------------------ */
int fastf_marker_auc(const void *planes, uint32_t n_planes, uint32_t n_cells, uint32_t K, const uint8_t *lab, uint32_t n_labels,
                     uint64_t *s2u, uint32_t *det, uint64_t *sum, uint32_t *n_per_label)
{
    if (n_planes < 1 || n_planes > FASTF_MARKER_MAX_PLANES)
        return fastf_res_err("fastf_marker_auc: FASTF_ERR_MARKER_COUNT: %u planes — a count of 2^14 or more among the highly variable genes: the rank table of a gene does not fit the LDS", n_planes);
    if (n_labels < 1 || n_labels > FASTF_LABELS_MAX) return fastf_res_err("fastf_marker_auc: %u labels, from 1 to %u", n_labels, FASTF_LABELS_MAX);
    if (K > 4096) return fastf_res_err("fastf_marker_auc: %u genes, at most 4096", K);
    if (!n_per_label || (K && (!s2u || !det || !sum)) || (n_cells && (!lab || (K && !planes)))) return fastf_res_err("null argument");
    const size_t words = (size_t)n_labels * K;
    memset(n_per_label, 0, (size_t)n_labels * sizeof *n_per_label);
    if (words) { memset(s2u, 0, words * sizeof *s2u); memset(det, 0, words * sizeof *det); memset(sum, 0, words * sizeof *sum); }
    uint32_t n_pad = 0, K_pad = 0, n_lab = 0;
    fastf_neighbors_pad(n_cells, K, &n_pad, &K_pad);
    for (uint32_t i = 0; i < n_cells; i++) if (lab[i] - 1u < n_labels) { n_per_label[lab[i] - 1u]++; n_lab++; }
    if (!n_cells || !K) return 0;
    const uint32_t bins = n_planes == 1 ? 128u : 16384u;
    const size_t plane_bytes = (size_t)n_pad * K_pad;
    const uint8_t *const pl = (const uint8_t *)planes;
    uint32_t *const E = (uint32_t *)malloc(((size_t)bins + n_cells) * sizeof *E), *const x = E ? E + bins : NULL;
    if (!E) return fastf_res_err("out of memory");
    for (uint32_t g = 0; g < K; g++) {
        memset(E, 0, bins * sizeof *E);
        for (uint32_t i = 0; i < n_cells; i++) {
            uint32_t v = pl[(size_t)i * K_pad + g] & 127u;
            if (n_planes == 2) v |= (uint32_t)(pl[plane_bytes + (size_t)i * K_pad + g] & 127u) << 7;
            x[i] = v;
            if (lab[i] - 1u < n_labels) E[v]++;
        }
        uint32_t c = 0;
        for (uint32_t v = 0; v < bins; v++) { const uint32_t e = E[v]; E[v] = 2u * c + e; c += e; }     /* 2 C(v) + E(v) */
        for (uint32_t i = 0; i < n_cells; i++) {
            const uint32_t a = lab[i] - 1u;
            if (a >= n_labels) continue;
            const size_t at = (size_t)a * K + g;
            s2u[at] += E[x[i]];
            if (x[i]) { det[at]++; sum[at] += x[i]; }
        }
        for (uint32_t a = 0; a < n_labels; a++) s2u[(size_t)a * K + g] -= (uint64_t)n_per_label[a] * n_per_label[a];
    }
    (void)n_lab;
    free(E);
    return 0;
}

typedef struct { uint64_t s2u; uint32_t gene, slot; } mk_key;
static int cmp_mk_key(const void *a, const void *b)
{
    const mk_key *x = (const mk_key *)a, *y = (const mk_key *)b;
    if (x->s2u != y->s2u) return x->s2u > y->s2u ? -1 : 1;
    return x->gene < y->gene ? -1 : x->gene > y->gene;
}

int fastf_marker_rank(const uint64_t *s2u, const uint32_t *n_per_label, const uint32_t *genes, uint32_t K, uint32_t n_labels, uint32_t *rank)
{
    if (n_labels > FASTF_LABELS_MAX) return fastf_res_err("fastf_marker_rank: %u labels, at most %u", n_labels, FASTF_LABELS_MAX);
    if ((n_labels && !n_per_label) || (n_labels && K && (!s2u || !rank))) return fastf_res_err("null argument");
    if (!n_labels || !K) return 0;
    uint64_t n_lab = 0;
    for (uint32_t a = 0; a < n_labels; a++) n_lab += n_per_label[a];
    mk_key *const key = (mk_key *)malloc((size_t)K * sizeof *key);
    if (!key) return fastf_res_err("out of memory");
    for (uint32_t a = 0; a < n_labels; a++) {
        uint32_t *const r = rank + (size_t)a * K;
        if (!n_per_label[a] || n_lab == n_per_label[a]) { memset(r, 0, (size_t)K * sizeof *r); continue; }     /* no ranking */
        for (uint32_t g = 0; g < K; g++) { key[g].s2u = s2u[(size_t)a * K + g]; key[g].gene = genes ? genes[g] : g; key[g].slot = g; }
        qsort(key, K, sizeof *key, cmp_mk_key);
        for (uint32_t k = 0; k < K; k++) r[key[k].slot] = k + 1;
    }
    free(key);
    return 0;
}

const char *fastf_markers_header(void) { return "label\tgene\trank_full\trank_point\tauc_full\tauc_point\tdet_in_full\tdet_out_full\tdet_in_point\tdet_out_point\tmean_in_point\n"; }

int fastf_markers_row(const char *label, const char *gene, uint32_t n_in, uint32_t n_out, uint32_t rank_full, uint32_t rank_point, uint64_t s2u_full,
                      uint64_t s2u_point, uint32_t det_in_full, uint32_t det_out_full, uint32_t det_in_point, uint32_t det_out_point, uint64_t sum_in_point,
                      char *buf, size_t cap)
{
    if (!label || !buf) return fastf_res_err("null argument");
    int n;
    if (!gene || !n_in || !n_out) n = snprintf(buf, cap, "%s\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n", label);
    else {
        const double den = 2.0 * (double)n_in * (double)n_out;
        n = snprintf(buf, cap, "%s\t%s\t%u\t%u\t%.6f\t%.6f\t%u\t%u\t%u\t%u\t%.6f\n", label, gene, rank_full, rank_point, (double)s2u_full / den, (double)s2u_point / den,
                     det_in_full, det_out_full, det_in_point, det_out_point, (double)sum_in_point / (double)n_in);
    }
    return (n < 0 || (size_t)n >= cap) ? fastf_res_err("markers row too long") : 0;
}

int fastf_markers_summary_rows(float rate_cell, float rate_depth, uint64_t list_value, uint32_t seed, const char *const *names, uint32_t n_labels, uint32_t K,
                               uint32_t top_n, const uint32_t *n_per_label, const uint32_t *rank_full, const uint32_t *rank_point, const uint64_t *s2u_full,
                               const uint64_t *s2u_point, char *buf, size_t cap)
{
    if (!buf || (n_labels && (!names || !n_per_label)) || (n_labels && K && (!rank_full || !rank_point || !s2u_full || !s2u_point))) return fastf_res_err("null argument");
    const uint32_t top = top_n < K ? top_n : K;
    uint64_t n_lab = 0, all_out = 0, all_top = 0, all_kept = 0;
    double all_full = 0.0, all_point = 0.0;
    char second[32], f[2][40];
    size_t at = 0;
    lab_second(second, sizeof second, rate_depth, list_value);
    for (uint32_t a = 0; a < n_labels; a++) n_lab += n_per_label[a];
    for (uint32_t a = 0; a <= n_labels; a++) {
        int n;
        if (a == n_labels) {
            if (all_top) { snprintf(f[0], sizeof f[0], "%.6f", all_full / (double)all_top); snprintf(f[1], sizeof f[1], "%.6f", all_point / (double)all_top); }
            else { snprintf(f[0], sizeof f[0], "NA"); snprintf(f[1], sizeof f[1], "NA"); }
            n = snprintf(buf + at, cap - at, "%.3f\t%s\t%u\tall\t%llu\t%llu\t%llu\t%llu\t%s\t%s\n", (double)rate_cell, second, seed, (unsigned long long)n_lab,
                         (unsigned long long)all_out, (unsigned long long)all_top, (unsigned long long)all_kept, f[0], f[1]);
        } else {
            const uint64_t n_in = n_per_label[a], n_out = n_lab - n_in;
            all_out += n_out;
            if (!n_in || !n_out || !top)
                n = snprintf(buf + at, cap - at, "%.3f\t%s\t%u\t%s\t%llu\t%llu\t%u\tNA\tNA\tNA\n", (double)rate_cell, second, seed, names[a + 1], (unsigned long long)n_in,
                             (unsigned long long)n_out, top);
            else {
                uint64_t kept = 0, sf = 0, sp = 0;
                for (uint32_t g = 0; g < K; g++) {
                    const size_t w = (size_t)a * K + g;
                    if (rank_full[w] < 1 || rank_full[w] > top) continue;
                    kept += rank_point[w] >= 1 && rank_point[w] <= top;
                    sf += s2u_full[w]; sp += s2u_point[w];
                }
                const double den = 2.0 * (double)n_in * (double)n_out, mf = (double)sf / den, mp = (double)sp / den;
                all_top += top; all_kept += kept; all_full += mf; all_point += mp;
                n = snprintf(buf + at, cap - at, "%.3f\t%s\t%u\t%s\t%llu\t%llu\t%u\t%llu\t%.6f\t%.6f\n", (double)rate_cell, second, seed, names[a + 1], (unsigned long long)n_in,
                             (unsigned long long)n_out, top, (unsigned long long)kept, mf / (double)top, mp / (double)top);
            }
        }
        if (n < 0 || (size_t)n >= cap - at) return fastf_res_err("markers summary rows too long");
        at += (size_t)n;
    }
    return 0;
}
