/*
 * cap_cmds.c — `fastF cap`: every cell downsampled to at most N reads, over a grid of (cell rate, cap) points from ONE decode of
 * the BAM.
 *
 *   cmd_cap()    -b -a -f -o -c <list> -n <list> [-s seed | --seeds <list> | --reps N] [--summary-only] [--genes] [--cells]; -d accepted and
 *                ignored, -u refused
 *   fastf_cap()  the same in process; fastf_cap_reps(): with a list of seeds, as sweep takes them (sweep_cmds.c)
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

#include <errno.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

static int cp_err(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static int cp_err(const char *fmt, ...)
{
    char buf[480];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    fastf_set_error_(buf);
    return 1;
}

/* ------------------------------------------------------------------ */
/* the grid                                                            */
/* ------------------------------------------------------------------ */
/* "10,100,1000" -> integers >= 1: digits only (no sign, no blanks); refused: an empty list or element, 0, a value twice */
int fastf_cap_parse_caps(const char *text, uint64_t *out, uint32_t cap, uint32_t *n_out)
{
    uint32_t n = 0;
    if (n_out) *n_out = 0;
    if (!text || !out || !n_out) return cp_err("null argument");
    for (const char *p = text;;) {
        const char *q = p;
        uint64_t v = 0;
        if (*q == ',' || !*q) return cp_err("reads per cell `%s`: empty element", text);
        for (; *q && *q != ','; q++) {
            if (*q < '0' || *q > '9') return cp_err("reads per cell `%s`: expects positive integers", text);
            if (v > (UINT64_MAX - (uint64_t)(*q - '0')) / 10) return cp_err("reads per cell `%s`: numerical result out of range", text);
            v = v * 10 + (uint64_t)(*q - '0');
        }
        if (v < 1) return cp_err("reads per cell `%s`: a cap is at least 1", text);
        for (uint32_t j = 0; j < n; j++) if (out[j] == v) return cp_err("reads per cell `%s`: %llu is listed twice", text, (unsigned long long)v);
        if (n == cap) return cp_err("reads per cell `%s`: more than %u values", text, cap);
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
    return (n < 0 || (size_t)n >= cap) ? cp_err("directory name too long") : 0;
}

int fastf_cap_check_grid(const float *rates_cell, uint32_t n_c, const uint64_t *caps, uint32_t n_n)
{
    if (!n_c || !n_n || !rates_cell || !caps) return cp_err("cap: the grid needs at least one cell rate and one cap");
    const float one = 1.0f;
    if (fastf_sweep_check_grid(rates_cell, n_c, &one, 1)) {       /* the cell rates are sweep's */
        char keep[400]; snprintf(keep, sizeof keep, "%s", fastf_last_error());
        return cp_err("cap: %s", !strncmp(keep, "sweep: ", 7) ? keep + 7 : keep);
    }
    for (uint32_t i = 0; i < n_n; i++) {
        if (caps[i] < 1) return cp_err("cap: reads per cell %llu: a cap is at least 1", (unsigned long long)caps[i]);
        for (uint32_t j = 0; j < i; j++) if (caps[j] == caps[i]) return cp_err("cap: reads per cell %llu is listed twice", (unsigned long long)caps[i]);
    }
    return 0;
}

/* ------------------------------------------------------------------ */
/* thresholds, the summary row                                         */
/* ------------------------------------------------------------------ */
int fastf_cap_thresholds(const uint32_t *hits, uint32_t n_cells, uint64_t cap, uint64_t *thresholds_out)
{
    if (n_cells && (!hits || !thresholds_out)) return cp_err("null argument");
    if (cap < 1) return cp_err("cap: a cap is at least 1");
    for (uint32_t k = 0; k < n_cells; k++)
        thresholds_out[k] = hits[k] <= cap ? (uint64_t)1 << 32 : fastf_draw_threshold((float)((double)cap / (double)hits[k]));
    return 0;
}

float fastf_cap_realised(uint64_t sampled, uint64_t hits) { return hits ? (float)((double)sampled / (double)hits) : 1.0f; }

const char *fastf_cap_header(void)
{
    return "rate_cell\treads_per_cell\tseed\tn_cells\ttotal_reads\tsampled_reads\tsampled_valid_reads\tnnz\tumis\tsaturation\t"
           "median_umis_per_cell\tmedian_genes_per_cell\thits\tcells_capped\trealised_depth\n";
}

static int cap_row_(float rate_cell, uint64_t reads_per_cell, uint32_t seed, const uint64_t counters[3], uint64_t nnz, uint64_t umis,
                    const uint64_t *umis_per_cell, const uint32_t *genes_per_cell, uint32_t n_cells, uint64_t hits, uint32_t cells_capped,
                    char *buf, size_t cap, double *metrics);
int fastf_cap_summary_row(float rate_cell, uint64_t reads_per_cell, uint32_t seed, const uint64_t counters[3], uint64_t nnz, uint64_t umis,
                          const uint64_t *umis_per_cell, const uint32_t *genes_per_cell, uint32_t n_cells, uint64_t hits, uint32_t cells_capped,
                          char *buf, size_t cap)
{
    return cap_row_(rate_cell, reads_per_cell, seed, counters, nnz, umis, umis_per_cell, genes_per_cell, n_cells, hits, cells_capped, buf, cap, NULL);
}
/* metrics: fastf_summary_tail_ */
static int cap_row_(float rate_cell, uint64_t reads_per_cell, uint32_t seed, const uint64_t counters[3], uint64_t nnz, uint64_t umis,
                    const uint64_t *umis_per_cell, const uint32_t *genes_per_cell, uint32_t n_cells, uint64_t hits, uint32_t cells_capped,
                    char *buf, size_t cap, double *metrics)
{
    char tail[400];
    if (fastf_summary_tail_(seed, counters, nnz, umis, umis_per_cell, genes_per_cell, n_cells, tail, sizeof tail, metrics)) return 1;
    const int n = snprintf(buf, cap, "%.3f\t%llu\t%s\t%llu\t%u\t%.6f\n", (double)rate_cell, (unsigned long long)reads_per_cell, tail,
                           (unsigned long long)hits, cells_capped, (double)fastf_cap_realised(counters[1], hits));
    return (n < 0 || (size_t)n >= cap) ? cp_err("summary row too long") : 0;
}

/* ------------------------------------------------------------------ */
/* cap.tsv                                                             */
/* ------------------------------------------------------------------ */
static int tsv_open(res_tsv_t *t, const char *out_dir) { return fastf_res_tsv_open(t, out_dir, "cap.tsv", fastf_cap_header()); }

/* ------------------------------------------------------------------ */
/* one (cell rate, seed) pair, on the run's res_rate_t               */
/* ------------------------------------------------------------------ */
static int cap_cell_rate(res_rate_t *S, const resident_t *R, const fastf_lists_t *L, const uint64_t *cell_keys, const char *bam_label, const char *out_dir,
                         float rate_cell, const uint64_t *caps, uint32_t n_n, uint32_t seed, int summary_only, int device, FILE *tsv, res_genes_t *G,
                         res_cells_t *C, res_fid_t *Fd, res_reps_t *P, uint32_t k_seed, res_times_t *T)
{
    int rc = RES_FAIL;
    void *d_plane = NULL, *d_hits = NULL, *d_thr = NULL;
    uint32_t *h_hits = NULL; uint64_t *h_thr = NULL;
    if ((rc = fastf_res_rate_open(S, "cap", R, L, cell_keys, rate_cell, seed, device, G->on, C->on, T)) != RES_OK) goto done;
    rc = RES_FAIL;
    const uint64_t H = S->H, N = R->n;
    const uint32_t n_cells = S->n_cells;
    double tt = fastf_res_now();

    /* the hits per cell, counted where K1a left the cell indices; to the host once, through pinned memory */
    const size_t nc1 = (size_t)n_cells + 1;
    const uint64_t plane_words = ((H + 63) / 64) * 2 + 64;      /* (zeroed slack behind the plane: K1b reads a unit's words unconditionally) */
    if (!(d_hits = fastf_devmem_alloc(device, nc1 * 4)) || !(d_thr = fastf_devmem_alloc(device, nc1 * 8)) ||
        !(h_hits = (uint32_t *)fastf_pinned_alloc(nc1 * 4)) || !(h_thr = (uint64_t *)fastf_pinned_alloc(nc1 * 8)) ||
        !(d_plane = fastf_devmem_alloc(device, (size_t)plane_words * 4)) || fastf_devmem_zero(d_plane, (size_t)plane_words * 4)) goto done;
    if (fastf_dev_cell_hits(S->e, N, S->blocked ? S->d_blk : NULL, (uint32_t *)d_hits, NULL) || fastf_devmem_sync() ||
        fastf_devmem_copy(h_hits, d_hits, (size_t)n_cells * 4)) goto done;
    {   uint64_t sum = 0;
        for (uint32_t k = 0; k < n_cells; k++) sum += h_hits[k];
        if (sum != H) { cp_err("internal error: %llu hits per cell in total, K1a counted %llu", (unsigned long long)sum, (unsigned long long)H); goto done; } }
    T->planes += fastf_res_now() - tt;
    if (Fd->full) {                                         /* the full rows of the pair, once: T = 2^32 for every cell */
        tt = fastf_res_now();
        for (uint32_t k = 0; k < n_cells; k++) h_thr[k] = (uint64_t)1 << 32;
        if (fastf_devmem_copy(d_thr, h_thr, (size_t)n_cells * 8) ||
            fastf_dev_cell_decisions(S->e, N, S->blocked ? S->d_blk : NULL, seed, L->mt_skip, H, (const uint64_t *)d_thr, (uint32_t *)d_plane, NULL)) goto done;
        *(Fd->on ? &T->fidelity : Fd->gene_on ? &T->gene_fid : &T->neighbors) += fastf_res_now() - tt;
        const int frc = fastf_res_full_run(S, (const uint32_t *)d_plane, T);
        if (frc != RES_OK) { rc = frc; goto done; }
    }

    for (uint32_t j = 0; j < n_n; j++) {
        char base[64], name[96], dir[4096], row[640];
        uint64_t counters[3], nnz = 0;
        uint32_t capped = 0;
        double metrics[FASTF_REPS_METRICS];
        if (fastf_cap_point_dir(rate_cell, caps[j], base, sizeof base)) goto done;
        if (P->on ? fastf_reps_point_dir(base, seed, name, sizeof name) : (snprintf(name, sizeof name, "%s", base), 0)) goto done;
        tt = fastf_res_now();
        if (fastf_cap_thresholds(h_hits, n_cells, caps[j], h_thr)) goto done;
        for (uint32_t k = 0; k < n_cells; k++) capped += h_hits[k] > caps[j];
        if (fastf_devmem_copy(d_thr, h_thr, (size_t)n_cells * 8) ||
            fastf_dev_cell_decisions(S->e, N, S->blocked ? S->d_blk : NULL, seed, L->mt_skip, H, (const uint64_t *)d_thr, (uint32_t *)d_plane, NULL)) goto done;
        T->planes += fastf_res_now() - tt;
        const int prc = fastf_res_point_run(S, (const uint32_t *)d_plane, name, counters, &nnz, T);
        if (prc != RES_OK) { rc = prc; goto done; }
        tt = fastf_res_now();
        if (cap_row_(rate_cell, caps[j], seed, counters, nnz, S->h_upc[n_cells], S->h_upc, S->h_gpc, n_cells, H, capped, row, sizeof row, metrics) ||
            fastf_res_reps_point(P, j, k_seed, n_cells, metrics)) goto done;
        T->summary += fastf_res_now() - tt;
        if (fastf_res_point_fidelity(S, name, T)) goto done;     /* (the point's rows are still in the row buffer) */
        if (fastf_res_point_gene_fidelity(S, name, T)) goto done;
        if (fastf_res_point_neighbors(S, name, T)) goto done;
        if (fastf_res_point_labels(S, name, T)) goto done;
        if (fastf_res_point_markers(S, name, T)) goto done;
        if (G->on && P->on) {                               /* (the point's per-gene array is still on the device) */
            tt = fastf_res_now();
            if (fastf_res_reps_genes(P, S, j, k_seed, S->h_cpg, S->n_features)) goto done;
            T->reps += fastf_res_now() - tt;
        }
        if (!summary_only) {
            snprintf(dir, sizeof dir, "%s/%s", out_dir, name);
            if (fastf_res_point_write(S, dir, bam_label, fastf_cap_realised(counters[1], H), counters, nnz, T)) goto done;
        }
        if (fastf_res_fid_point(Fd, S, summary_only ? NULL : dir, 0.0f, caps[j], T)) goto done;
        if (G->on) {
            char grow[256];
            tt = fastf_res_now();
            if (fastf_genes_summary_row(rate_cell, 0.0f, caps[j], seed, S->h_cpg, S->h_upg, S->n_features, grow, sizeof grow) ||
                fastf_res_genes_point(G, L, name, summary_only ? NULL : dir, grow, S->h_cpg, S->h_upg)) goto done;
            T->genes += fastf_res_now() - tt;
        }
        if (C->on) {                                        /* (behind the point's rows: K3u overwrites the regions they were gathered from) */
            char crow[1024];
            if (fastf_res_point_cells(S, name, T)) goto done;
            tt = fastf_res_now();
            if (fastf_cells_summary_row(rate_cell, 0.0f, caps[j], seed, S->h_rpc, S->h_npc, S->h_spc, n_cells, S->h_hist, crow, sizeof crow) ||
                fastf_res_cells_point(C, S, summary_only ? NULL : dir, crow)) goto done;
            T->cells += fastf_res_now() - tt;
        }
        fputs(row, tsv);
    }
    rc = RES_OK;
done:
    fastf_devmem_free(d_plane); fastf_devmem_free(d_hits); fastf_devmem_free(d_thr);
    if (h_hits) fastf_pinned_free(h_hits);
    if (h_thr) fastf_pinned_free(h_thr);
    return rc;
}

static int cap_resident(const char *bam_file, const char *out_dir, const char *barcodes, const char *features, const float *rc_list, uint32_t n_c,
                        const uint64_t *caps, uint32_t n_n, const uint32_t *seeds, uint32_t n_s, int summary_only, int device, FILE *tsv, res_genes_t *G,
                        res_cells_t *C, res_fid_t *Fd, res_reps_t *P)
{
    int rc = RES_FAIL;
    const int prof = getenv("FASTF_PROFILE") != NULL;
    res_times_t T; memset(&T, 0, sizeof T);
    const double t0 = fastf_res_now();
    double tt = t0;
    res_lists_t LL; memset(&LL, 0, sizeof LL);
    resident_t R; memset(&R, 0, sizeof R);
    res_rate_t S; memset(&S, 0, sizeof S);
    /* the (cell rate, seed) pairs: cell rates outer, the seeds as listed */
    const uint32_t n_pairs = n_c * n_s;
    float *pair_rate = (float *)malloc(n_pairs * sizeof *pair_rate);
    uint32_t *pair_seed = (uint32_t *)malloc(n_pairs * sizeof *pair_seed);
    if (!pair_rate || !pair_seed) { cp_err("out of memory"); goto done; }
    for (uint32_t i = 0; i < n_c; i++) for (uint32_t k = 0; k < n_s; k++) { pair_rate[i * n_s + k] = rc_list[i]; pair_seed[i * n_s + k] = seeds[k]; }
    if ((rc = fastf_res_lists_load(barcodes, features, pair_rate, pair_seed, n_pairs, &LL)) != RES_OK) goto done;
    rc = RES_FAIL;
    S.max_cells = fastf_res_lists_max_cells(&LL);
    S.fidelity = Fd->on; S.gene_fid = Fd->gene_on; S.neighbors = Fd->nbr_on || Fd->lab_on; S.labels = Fd->lab_on; S.lab_t = Fd->labels; S.markers = Fd->markers;
    {   const char *nr = getenv("FASTF_RES_NO_REUSE"); S.no_reuse = nr && nr[0] == '1'; }
    T.lists = fastf_res_now() - tt; tt = fastf_res_now();
    if (fastf_res_decode("cap", bam_file, &LL.L[0], device, &R)) goto done;
    T.decode = fastf_res_now() - tt;
    if (P->on) printf("cap: %llu records resident on the device (%llu bytes), %u x %u points x %u seeds\n", (unsigned long long)R.n, (unsigned long long)(R.n * 24), n_c, n_n, n_s);
    else printf("cap: %llu records resident on the device (%llu bytes), %u x %u points\n", (unsigned long long)R.n, (unsigned long long)(R.n * 24), n_c, n_n);
    for (uint32_t i = 0; i < n_c; i++) {
        if (fastf_res_reps_rate_begin(P, &LL.L[i * n_s], 1)) { rc = RES_FAIL; goto done; }
        for (uint32_t k = 0; k < n_s; k++) {
            const uint32_t at = i * n_s + k;
            rc = cap_cell_rate(&S, &R, &LL.L[at], LL.keys[at], bam_file, out_dir, rc_list[i], caps, n_n, seeds[k], summary_only, device, tsv, G, C, Fd, P, k, &T);
            if (rc != RES_OK) goto done;
        }
        if (fastf_res_reps_rate_end(P, rc_list[i], NULL, caps, &T)) { rc = RES_FAIL; goto done; }
    }
    rc = RES_OK;
    if (prof)
        fprintf(stderr, "[cap] lists %.3f s, decode to resident records %.3f s, engines %.3f s, layout+K1a %.3f s, hits per cell + thresholds + planes %.3f s, "
                        "per-point device work %.3f s (%.4f s a point), summary D2H+medians %.3f s, rows D2H %.3f s, writers %.3f s, total %.3f s\n",
                T.lists, T.decode, T.engine, T.block_k1a, T.planes, T.device, T.device / (n_c * n_n * n_s), T.summary, T.d2h, T.write, fastf_res_now() - t0);
    if (prof && P->on) fprintf(stderr, "[cap] replicates: %u (cell rate, seed) pairs opened in %.3f s (engines %.3f s, buffers + layout + K1a %.3f s), the blocked copy "
                                       "laid out %u times; replicate tables and per-gene accumulation %.3f s\n", T.opens, T.engine + T.block_k1a, T.engine, T.block_k1a, T.relays, T.reps);
    if (prof && G->on) fprintf(stderr, "[cap] --genes: per-gene D2H, rows and files %.3f s (the kernel is part of the per-point device work)\n", T.genes);
    if (prof && C->on) fprintf(stderr, "[cap] --cells: full sort + K3u + copy summary + D2H %.3f s (%.4f s a point), rows and files %.3f s\n",
                               T.cells_dev, T.cells_dev / (n_c * n_n * n_s), T.cells);
    if (prof && Fd->on) fprintf(stderr, "[cap] --fidelity: %u full-depth points, the joins, their D2H, rows and files %.3f s\n", n_c * n_s, T.fidelity);
    if (prof && Fd->gene_on) fprintf(stderr, "[cap] --gene-fidelity: %sthe partner counts, the per-gene sums, their D2H, rows and files %.3f s\n", Fd->on ? "" : "the full-depth rows of every pair, ", T.gene_fid);
    if (prof && Fd->mk_on) fprintf(stderr, "[cap] --markers: top %u of the genes per label; the kernel calls on the planes, their D2H, the ranks, rows and files %.3f s\n", Fd->markers, T.markers);
    if (prof && Fd->lab_on) fprintf(stderr, "[cap] --labels: %u labels, labels_unknown %llu; %sthe label arrays of every pair, the vote calls, their D2H, rows and files %.3f s\n", fastf_labels_count(Fd->labels),
                                    (unsigned long long)fastf_labels_unknown(Fd->labels), Fd->nbr_on ? "" : "the neighbour sets of --neighbors and what they need, ", T.labels + (Fd->nbr_on ? 0.0 : T.neighbors));
    if (prof && Fd->nbr_on) fprintf(stderr, "[cap] --neighbors: %sthe planes, the Gram products and selections, the shared counts, their D2H, rows and files %.3f s\n", Fd->on || Fd->gene_on ? "" : "the full-depth rows and per-gene sums of every pair, ", T.neighbors);
done:
    fastf_res_rate_close(&S);
    fastf_res_free(&R);
    fastf_res_lists_free(&LL);
    free(pair_rate); free(pair_seed);
    return rc;
}

/* ------------------------------------------------------------------ */
/* the command                                                         */
/* ------------------------------------------------------------------ */
/* reps != 0: a replicate run (fastf_cap_reps) — the suffixed directories and the replicate tables, with one seed too */
static int cap_run_(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                   const uint64_t *caps, uint32_t n_n, const uint32_t *seeds, uint32_t n_s, int reps, uint32_t flags, const fastf_labels_t *labels, uint32_t markers)
{
    if (!bam || !barcodes || !features) return cp_err("cap: null argument");
    if (!out_dir) out_dir = ".";
    if (fastf_cap_check_grid(rates_cell, n_c, caps, n_n)) return 1;
    if (flags & ~(uint32_t)(FASTF_CAP_SUMMARY_ONLY | FASTF_CAP_GENES | FASTF_CAP_CELLS | FASTF_CAP_FIDELITY | FASTF_CAP_GENE_FIDELITY | FASTF_CAP_NEIGHBORS)) return cp_err("cap: unknown flags 0x%x", flags);
    const int summary_only = (flags & FASTF_CAP_SUMMARY_ONLY) != 0, genes = (flags & FASTF_CAP_GENES) != 0, cells = (flags & FASTF_CAP_CELLS) != 0;
    const int fidelity = (flags & FASTF_CAP_FIDELITY) != 0, gene_fidelity = (flags & FASTF_CAP_GENE_FIDELITY) != 0, neighbors = (flags & FASTF_CAP_NEIGHBORS) != 0;
    if (access(bam, R_OK) == -1) return cp_err("bam file: %s does not exist.", bam);
    int dev0 = 0, dev_second = -1;
    {   const char *dvs = getenv("FASTF_DEVICES");
        fastf_pick_devices(dvs, getenv("FASTF_DEVICE"), &dev0, &dev_second);
        if (dvs && *dvs && (strchr(dvs, ',') || atoi(dvs) >= 2))
            return labels ? cp_err("cap: --labels needs the resident form, and this job is outside it (several devices), and a cap has no point-by-point form") :
                   neighbors ? cp_err("cap: --neighbors needs the resident form, and this job is outside it (several devices), and a cap has no point-by-point form") :
                   gene_fidelity ? cp_err("cap: --gene-fidelity needs the resident form, and this job is outside it (several devices), and a cap has no point-by-point form")
                                 : cp_err("cap: this job is outside the resident form (several devices), and a cap has no point-by-point form"); }
    if (fastf_res_make_dir(out_dir)) return 1;
    res_tsv_t tsv; memset(&tsv, 0, sizeof tsv);
    if (tsv_open(&tsv, out_dir)) return 1;
    res_genes_t G;
    if (fastf_res_genes_open(&G, genes, "cap", out_dir, fastf_cap_genes_header(), n_c * n_n, reps)) { fastf_res_tsv_close(&tsv, 0); return 1; }
    res_cells_t C;
    if (fastf_res_cells_open(&C, cells, "cap", out_dir, fastf_cap_cells_header())) { fastf_res_tsv_close(&tsv, 0); fastf_res_genes_close(&G, 0); return 1; }
    res_fid_t Fd;
    if (fastf_res_fid_open(&Fd, fidelity, gene_fidelity, "cap", out_dir, fastf_cap_fidelity_header(), fastf_cap_gene_fidelity_header())) { fastf_res_tsv_close(&tsv, 0); fastf_res_genes_close(&G, 0); fastf_res_cells_close(&C, 0); return 1; }
    if (fastf_res_fid_open_neighbors(&Fd, neighbors, "cap", out_dir, fastf_cap_neighbors_header())) { fastf_res_tsv_close(&tsv, 0); fastf_res_genes_close(&G, 0); fastf_res_cells_close(&C, 0); fastf_res_fid_close(&Fd, 0); return 1; }
    if (fastf_res_fid_open_labels(&Fd, labels, "cap", out_dir, fastf_cap_labels_header(), fastf_cap_label_classes_header())) { fastf_res_tsv_close(&tsv, 0); fastf_res_genes_close(&G, 0); fastf_res_cells_close(&C, 0); fastf_res_fid_close(&Fd, 0); return 1; }
    if (fastf_res_fid_open_markers(&Fd, markers, "cap", out_dir, fastf_cap_markers_header())) { fastf_res_tsv_close(&tsv, 0); fastf_res_genes_close(&G, 0); fastf_res_cells_close(&C, 0); fastf_res_fid_close(&Fd, 0); return 1; }
    res_reps_t P;
    if (fastf_res_reps_open(&P, reps, "cap", out_dir, seeds, n_s, n_c, n_n, genes, dev0, fastf_cap_reps_header(), fastf_cap_genes_reps_header())) {
        fastf_res_tsv_close(&tsv, 0); fastf_res_genes_close(&G, 0); fastf_res_cells_close(&C, 0); fastf_res_fid_close(&Fd, 0); return 1;
    }
    int rc = cap_resident(bam, out_dir, barcodes, features, rates_cell, n_c, caps, n_n, seeds, n_s, summary_only, dev0, tsv.f, &G, &C, &Fd, &P);
    if (rc == RES_NOT_COVERED && labels)
        cp_err("cap: --labels needs the resident form, and this job is outside it (keys wider than 64 bits or UMIs beyond what a 64-bit key holds), and a cap has no point-by-point form");
    else if (rc == RES_NOT_COVERED && neighbors)
        cp_err("cap: --neighbors needs the resident form, and this job is outside it (keys wider than 64 bits or UMIs beyond what a 64-bit key holds), and a cap has no point-by-point form");
    else if (rc == RES_NOT_COVERED && gene_fidelity)
        cp_err("cap: --gene-fidelity needs the resident form, and this job is outside it (keys wider than 64 bits or UMIs beyond what a 64-bit key holds), and a cap has no point-by-point form");
    else if (rc == RES_NOT_COVERED)
        cp_err("cap: this job is outside the resident form (keys wider than 64 bits or UMIs beyond what a 64-bit key holds), and a cap has no point-by-point form");
    if (!rc && fastf_res_genes_close(&G, 1)) rc = 1;
    if (!rc && fastf_res_cells_close(&C, 1)) rc = 1;
    if (!rc && fastf_res_fid_close(&Fd, 1)) rc = 1;
    if (!rc && fastf_res_reps_close_grid(&P, 1, rates_cell, NULL, caps)) rc = 1;
    if (rc) {
        char keep[512]; snprintf(keep, sizeof keep, "%s", fastf_last_error());
        fastf_res_tsv_close(&tsv, 0); fastf_res_genes_close(&G, 0); fastf_res_cells_close(&C, 0); fastf_res_fid_close(&Fd, 0); fastf_res_reps_close(&P, 0);
        if (reps) fastf_res_reps_unlink_tables(out_dir, "cap");      /* (the tables that were already renamed go too: none is left) */
        fastf_set_error_(keep);
        return 1;
    }
    if (fastf_res_tsv_close(&tsv, 1)) { if (reps) fastf_res_reps_unlink_tables(out_dir, "cap"); return 1; }
    return 0;
}

/* labels_path != NULL: the labels file is read and checked before anything is written */
static int cap_run(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                   const uint64_t *caps, uint32_t n_l, const uint32_t *seeds, uint32_t n_s, int reps, uint32_t flags, const char *labels_path, uint32_t markers)
{
    if (!labels_path) return cap_run_(bam, out_dir, barcodes, features, rates_cell, n_c, caps, n_l, seeds, n_s, reps, flags, NULL, 0);
    if (!bam || !barcodes || !features) return cp_err("cap: null argument");
    if (access(bam, R_OK) == -1) return cp_err("bam file: %s does not exist.", bam);
    fastf_labels_t *labels = NULL;
    if (fastf_labels_load(labels_path, barcodes, &labels)) return 1;
    const int rc = cap_run_(bam, out_dir, barcodes, features, rates_cell, n_c, caps, n_l, seeds, n_s, reps, flags, labels, markers);
    fastf_labels_free(labels);
    return rc;
}

int fastf_cap_labels(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                     const uint64_t *caps, uint32_t n_n, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path)
{
    if (!n_seeds) return cap_run(bam, out_dir, barcodes, features, rates_cell, n_c, caps, n_n, &seed, 1, 0, flags, labels_path, 0);
    if (fastf_check_seeds_("cap", seeds, n_seeds)) return 1;
    return cap_run(bam, out_dir, barcodes, features, rates_cell, n_c, caps, n_n, seeds, n_seeds, 1, flags, labels_path, 0);
}

/* --markers N: the labels run with the marker tables beside it */
int fastf_cap_markers(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                       const uint64_t *caps, uint32_t n_n, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path,
                       uint32_t markers)
{
    if (markers < 1 || markers > FASTF_MARKERS_MAX) return cp_err("cap: --markers: N = %u, from 1 to %u", markers, FASTF_MARKERS_MAX);
    if (!labels_path) return cp_err("cap: --markers needs --labels");
    if (!n_seeds) return cap_run(bam, out_dir, barcodes, features, rates_cell, n_c, caps, n_n, &seed, 1, 0, flags, labels_path, markers);
    if (fastf_check_seeds_("cap", seeds, n_seeds)) return 1;
    return cap_run(bam, out_dir, barcodes, features, rates_cell, n_c, caps, n_n, seeds, n_seeds, 1, flags, labels_path, markers);
}

int fastf_cap(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
              const uint64_t *caps, uint32_t n_n, uint32_t seed, uint32_t flags)
{
    return cap_run(bam, out_dir, barcodes, features, rates_cell, n_c, caps, n_n, &seed, 1, 0, flags, NULL, 0);
}

int fastf_cap_reps(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                   const uint64_t *caps, uint32_t n_n, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags)
{
    if (fastf_check_seeds_("cap", seeds, n_seeds)) return 1;
    return cap_run(bam, out_dir, barcodes, features, rates_cell, n_c, caps, n_n, seeds, n_seeds, 1, flags, NULL, 0);
}

static void usage_cap(FILE *f)
{
    fprintf(f,
            "Usage: fastF cap [options]\n\n"
            "every cell downsampled to at most N reads, over a grid of cell rates and caps from one decode of the bam file: per point\n"
            "<out>/c<cell>_n<N>/ with the three files of bam2db, and <out>/cap.tsv with one summary row per point.\n\n"
            "    -h, --help            show this help message and exit\n"
            "    -b, --bam=<str>       path to bam file\n"
            "    -f, --feature=<str>   path to feature list file\n"
            "    -a, --barcode=<str>   path to barcode list file\n"
            "    -d, --dbname=<str>    name of database (accepted for compatibility, ignored)\n"
            "    -c, --cell=<list>     rates of cell barcode, comma separated (default 1.0)\n"
            "    -n, --reads=<list>    reads per cell at most, comma separated integers >= 1\n"
            "    -o, --out=<str>       path to output directory (default .)\n"
            "    -s, --seed=<int>      seed for random number generator (default 926)\n"
            "        --summary-only    write cap.tsv alone\n"
            "        --genes           per-gene detection too: cap_genes.tsv, cap_gene_cells.tsv.gz and genes.tsv.gz per point\n"
            "        --cells           per-cell reads, saturation and UMI copy numbers too: cap_cells.tsv and cells.tsv.gz per point\n"
            "        --fidelity        every point against the full-depth data of the same cells (every read of the sampled cells kept):\n"
            "                          cap_fidelity.tsv and fidelity.tsv.gz per point, with the Pearson and the cosine of the RAW counts\n"
            "                          over ALL genes per cell (not log-normalised)\n"
            "        --gene-fidelity   every point against the full-depth data of the same cells, per GENE: cap_gene_fidelity.tsv and\n"
            "                          gene_fidelity.tsv.gz per point, with the Pearson of the RAW counts over ALL sampled cells per gene,\n"
            "                          the dispersion (variance / mean) at full depth and at the point, and the overlap of the 2000\n"
            "                          most variable genes\n"
            "        --neighbors       every point against the full-depth data of the same cells, BETWEEN the cells: cap_neighbors.tsv and\n"
            "                          neighbors.tsv.gz per point, with the share of a cell's 15 nearest neighbours at full depth (cosine of\n"
            "                          the RAW counts over the 2000 most variable genes, decided in exact integers) that it keeps\n"
            "        --labels=<file>   one `barcode<TAB>label` per line (cell types of the full-depth analysis): cap_labels.tsv,\n"
            "                          cap_label_classes.tsv and labels.tsv.gz, label_confusion.tsv.gz per point, with the share of labelled\n"
            "                          cells whose 15 nearest neighbours still vote for their own label, at full depth and at the point\n"
            "        --markers=<N>     with --labels: per label the N (1 to 2000) best marker genes among the 2000 most variable, ranked by the\n"
            "                          exact AUC of the label's cells against the other labelled cells, at full depth and at the point:\n"
            "                          cap_markers.tsv and markers.tsv.gz per point\n"
            "        --seeds=<list>    replicates: the grid at each of 1 to 64 seeds, comma separated, from the one decode; per point and\n"
            "                          seed <out>/c<cell>_n<N>_s<seed>/, one cap.tsv row each, and cap_reps.tsv with mean, sd, min and max\n"
            "                          of every metric per grid point (with --genes cap_genes_reps.tsv and cap_gene_reps.tsv.gz in\n"
            "                          place of cap_gene_cells.tsv.gz); not with -s or --reps\n"
            "        --reps=<int>      the same at the seeds s, s + 1, .. s + N - 1 (s: -s; N from 1 to 64)\n");
}

#define CAP_MAX_POINTS 64
int cmd_cap(int argc, const char **argv)
{
    res_args_t A;
    const int prc = fastf_res_parse_args(argc, argv, 'n', "reads", usage_cap, "cap does not write umi.tsv.gz (-u).", &A);
    if (prc) return prc == 2 ? 0 : 1;
    const char *cells = A.cells, *reads = A.list;
    float rc[CAP_MAX_POINTS]; uint64_t caps[CAP_MAX_POINTS];
    uint32_t n_c = 0, n_n = 0;
    if (!reads) { fprintf(stderr, "\x1b[31mError:\x1b[0m cap needs -n <list>: the reads per cell at most\n"); return 1; }
    if (fastf_sweep_parse_rates(cells, 1, rc, CAP_MAX_POINTS, &n_c) || fastf_cap_parse_caps(reads, caps, CAP_MAX_POINTS, &n_n) ||
        fastf_cap_check_grid(rc, n_c, caps, n_n)) {
        fprintf(stderr, "\x1b[31mError:\x1b[0m %s\n", fastf_last_error());
        return 1;
    }
    if (fastf_res_check_inputs(&A)) return 1;
    const uint32_t flags = (A.summary_only ? FASTF_CAP_SUMMARY_ONLY : 0) | (A.genes ? FASTF_CAP_GENES : 0) | (A.per_cell ? FASTF_CAP_CELLS : 0) | (A.fidelity ? FASTF_CAP_FIDELITY : 0) |
                           (A.gene_fidelity ? FASTF_CAP_GENE_FIDELITY : 0) | (A.neighbors ? FASTF_CAP_NEIGHBORS : 0);
    if (A.markers ? fastf_cap_markers(A.bam, A.out, A.bar, A.feat, rc, n_c, caps, n_n, A.seeds, A.n_seeds, flags, A.seed, A.labels, A.markers) :
        A.labels ? fastf_cap_labels(A.bam, A.out, A.bar, A.feat, rc, n_c, caps, n_n, A.seeds, A.n_seeds, flags, A.seed, A.labels) :
        A.n_seeds ? fastf_cap_reps(A.bam, A.out, A.bar, A.feat, rc, n_c, caps, n_n, A.seeds, A.n_seeds, flags)
                  : fastf_cap(A.bam, A.out, A.bar, A.feat, rc, n_c, caps, n_n, A.seed, flags)) {
        fprintf(stderr, "\x1b[31mError:\x1b[0m cap failed: %s\n", fastf_last_error());
        return 1;
    }
    if (A.genes && A.n_seeds) printf("cap_genes.tsv, cap_genes_reps.tsv and cap_gene_reps.tsv.gz are generated.\n");
    else if (A.genes) printf("cap_genes.tsv and cap_gene_cells.tsv.gz are generated.\n");
    if (A.per_cell) printf("cap_cells.tsv is generated.\n");
    if (A.fidelity) printf("cap_fidelity.tsv is generated.\n");
    if (A.gene_fidelity) printf("cap_gene_fidelity.tsv is generated.\n");
    if (A.neighbors) printf("cap_neighbors.tsv is generated.\n");
    if (A.labels) printf("cap_labels.tsv and cap_label_classes.tsv are generated.\n");
    if (A.markers) printf("cap_markers.tsv is generated.\n");
    if (A.n_seeds) printf("cap_reps.tsv is generated.\n");
    printf("cap.tsv is generated.\n");
    return 0;
}
