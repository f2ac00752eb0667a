/*
 * level_cmds.c — `fastF level`: every cell downsampled to at most M UMIs, exactly, over a grid of (cell rate, UMI cap) points from
 * ONE decode of the BAM.
 *
 *   cmd_level()    -b -a -f -o -c <list> -m <list> [-s seed | --seeds <list> | --reps N] [--summary-only] [--genes] [--cells]; -d accepted
 *                  and ignored, -u refused
 *   fastf_level()  the same in process; fastf_level_reps(): with a list of seeds, as cap takes them
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

#include <errno.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

static int lv_err(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static int lv_err(const char *fmt, ...)
{
    char buf[480];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    fastf_set_error_(buf);
    return 1;
}
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
    return (n < 0 || (size_t)n >= cap) ? lv_err("directory name too long") : 0;
}

/* cap's header with its second column named umi_cap (every call writes the same bytes) */
static const char *renamed_(char *buf, size_t cap, const char *cap_header)
{
    static const char from[] = "rate_cell\treads_per_cell\t", to[] = "rate_cell\tumi_cap\t";
    if (strncmp(cap_header, from, sizeof from - 1)) return cap_header;
    snprintf(buf, cap, "%s%s", to, cap_header + sizeof from - 1);
    return buf;
}
const char *fastf_level_header(void) { static char b[512]; return renamed_(b, sizeof b, fastf_cap_header()); }
const char *fastf_level_genes_header(void) { static char b[512]; return renamed_(b, sizeof b, fastf_cap_genes_header()); }
const char *fastf_level_cells_header(void) { static char b[1024]; return renamed_(b, sizeof b, fastf_cap_cells_header()); }
const char *fastf_level_reps_header(void) { static char b[2048]; return renamed_(b, sizeof b, fastf_cap_reps_header()); }
const char *fastf_level_genes_reps_header(void) { static char b[512]; return renamed_(b, sizeof b, fastf_cap_genes_reps_header()); }

/* metrics: fastf_summary_tail_ */
static int level_row_(float rate_cell, uint64_t umi_cap, uint32_t seed, const uint64_t counters[3], uint64_t nnz, uint64_t umis,
                      const uint64_t *umis_per_cell, const uint32_t *genes_per_cell, uint32_t n_cells, uint64_t hits, uint32_t cells_capped,
                      char *buf, size_t cap, double *metrics)
{
    char tail[400];
    if (fastf_summary_tail_(seed, counters, nnz, umis, umis_per_cell, genes_per_cell, n_cells, tail, sizeof tail, metrics)) return 1;
    const int n = snprintf(buf, cap, "%.3f\t%llu\t%s\t%llu\t%u\t%.6f\n", (double)rate_cell, (unsigned long long)umi_cap, tail,
                           (unsigned long long)hits, cells_capped, (double)fastf_cap_realised(counters[1], hits));
    return (n < 0 || (size_t)n >= cap) ? lv_err("summary row too long") : 0;
}
int fastf_level_summary_row(float rate_cell, uint64_t umi_cap, uint32_t seed, const uint64_t counters[3], uint64_t nnz, uint64_t umis,
                            const uint64_t *umis_per_cell, const uint32_t *genes_per_cell, uint32_t n_cells, uint64_t hits, uint32_t cells_capped,
                            char *buf, size_t cap)
{
    return level_row_(rate_cell, umi_cap, seed, counters, nnz, umis, umis_per_cell, genes_per_cell, n_cells, hits, cells_capped, buf, cap, NULL);
}

/* ------------------------------------------------------------------ */
/* <point dir>/thresholds.tsv.gz                                       */
/* ------------------------------------------------------------------ */
static int write_thresholds(const char *dir, const fastf_lists_t *L, uint32_t n_cells, const uint64_t *thr, const uint64_t *umis_full, const uint64_t *umis)
{
    static const char head[] = "barcode\tthreshold\tumis_full\tumis\n";
    size_t room = sizeof head;
    for (uint32_t k = 0; k < n_cells; k++) room += strlen(L->barcode[k]) + 3 * 21 + 2;
    char *text = (char *)malloc(room), path[4200], tmp[4300];
    if (!text) return lv_err("out of memory");
    size_t len = (size_t)snprintf(text, room, "%s", head);
    for (uint32_t k = 0; k < n_cells; k++)
        len += (size_t)snprintf(text + len, room - len, "%s\t%llu\t%llu\t%llu\n", L->barcode[k], (unsigned long long)thr[k],
                                (unsigned long long)umis_full[k], (unsigned long long)umis[k]);
    snprintf(path, sizeof path, "%s/thresholds.tsv.gz", dir);
    snprintf(tmp, sizeof tmp, "%s.partial", path);
    int bad = fastf_res_make_dir(dir);
    if (!bad && (fastf_write_gz_text(tmp, text, len) || rename(tmp, path) != 0)) { unlink(tmp); bad = lv_err("cannot write %s", path); }
    free(text);
    return bad;
}

/* ------------------------------------------------------------------ */
/* one (cell rate, seed) pair, on the run's res_rate_t               */
/* ------------------------------------------------------------------ */
#define LEVEL_MAX_PASSES 32u                             /* hi - lo halves per probing pass, from 2^32 */
static int level_cell_rate(res_rate_t *S, const resident_t *R, const fastf_lists_t *L, const uint64_t *cell_keys, const char *bam_label, const char *out_dir,
                           float rate_cell, const uint64_t *caps, uint32_t n_m, uint32_t seed, int summary_only, int device, FILE *tsv, res_genes_t *G,
                           res_cells_t *C, res_fid_t *Fd, res_reps_t *P, uint32_t k_seed, res_times_t *T, int prof)
{
    int rc = RES_FAIL;
    void *d_plane = NULL;
    uint64_t *h_thr = NULL, *h_ufull = NULL;
    if ((rc = fastf_res_rate_open(S, "level", R, L, cell_keys, rate_cell, seed, device, G->on, C->on, T)) != RES_OK) goto done;
    rc = RES_FAIL;
    const uint64_t H = S->H, N = R->n;
    const uint32_t n_cells = S->n_cells;
    const void *const blk = S->blocked ? S->d_blk : NULL;
    double tt = fastf_res_now();
    const size_t nc1 = (size_t)n_cells + 1;
    const uint64_t plane_words = ((H + 63) / 64) * 2 + 64;      /* (zeroed slack behind the plane: K1b reads a unit's words unconditionally) */
    if (fastf_res_level_room(S)) goto done;
    if (!(h_thr = (uint64_t *)fastf_pinned_alloc(nc1 * 8)) || (!summary_only && !(h_ufull = (uint64_t *)fastf_pinned_alloc(nc1 * 8))) ||
        !(d_plane = fastf_devmem_alloc(device, (size_t)plane_words * 4)) || fastf_devmem_zero(d_plane, (size_t)plane_words * 4)) goto done;
    T->planes += fastf_res_now() - tt;

    /* pass 0: every hit kept.  U_k(2^32) stays on the device for every cap of the list; the state of the first cap comes with it */
    uint64_t open = 0, capped = 0;
    tt = fastf_res_now();
    for (uint32_t k = 0; k < n_cells; k++) h_thr[k] = (uint64_t)1 << 32;
    if (fastf_devmem_copy(S->d_probe, h_thr, (size_t)n_cells * 8) ||
        fastf_dev_cell_decisions(S->e, N, blk, seed, L->mt_skip, H, S->d_probe, (uint32_t *)d_plane, NULL)) goto done;
    T->search += fastf_res_now() - tt;
    {   char name0[64]; snprintf(name0, sizeof name0, "c%.3f (every hit)", (double)rate_cell);
        const int prc = fastf_res_search_pass(S, (const uint32_t *)d_plane, name0, caps[0], 1, &open, &capped, T);
        if (prc != RES_OK) { rc = prc; goto done; } }
    if (fastf_res_full_keep(S, T)) goto done;               /* --fidelity: pass 0's rows are the full rows of the pair */
    if (h_ufull && fastf_devmem_copy(h_ufull, S->d_ufull, (size_t)n_cells * 8)) goto done;

    for (uint32_t j = 0; j < n_m; j++) {
        char base[64], name[96], dir[4096], row[640];
        uint64_t counters[3], nnz = 0;
        double metrics[FASTF_REPS_METRICS];
        if (fastf_level_point_dir(rate_cell, caps[j], base, sizeof base)) goto done;
        if (P->on ? fastf_reps_point_dir(base, seed, name, sizeof name) : (snprintf(name, sizeof name, "%s", base), 0)) goto done;
        const double search0 = T->search, device0 = T->device;
        uint32_t passes = 0;
        if (j) { const int irc = fastf_res_level_init(S, caps[j], &open, &capped, T); if (irc != RES_OK) { rc = irc; goto done; } }
        while (open) {                                      /* open cells are probed at (lo + hi) / 2, every other cell at 0 */
            if (passes == LEVEL_MAX_PASSES) { lv_err("internal error: %llu cells still open after %u passes at point %s", (unsigned long long)open, passes, name); goto done; }
            tt = fastf_res_now();
            if (fastf_dev_cell_decisions(S->e, N, blk, seed, L->mt_skip, H, S->d_probe, (uint32_t *)d_plane, NULL)) goto done;
            T->search += fastf_res_now() - tt;
            const int prc = fastf_res_search_pass(S, (const uint32_t *)d_plane, name, caps[j], 0, &open, NULL, T);
            if (prc != RES_OK) { rc = prc; goto done; }
            passes++;
        }
        /* the point: T = lo */
        tt = fastf_res_now();
        if (fastf_dev_cell_decisions(S->e, N, blk, seed, L->mt_skip, H, S->d_lo, (uint32_t *)d_plane, NULL)) goto done;
        T->planes += fastf_res_now() - tt;
        const int prc = fastf_res_point_run(S, (const uint32_t *)d_plane, name, counters, &nnz, T);
        if (prc != RES_OK) { rc = prc; goto done; }
        if (prof) fprintf(stderr, "[level] point %s: %u probing passes, search %.4f s, the point's own pass %.4f s\n", name, passes, T->search - search0, T->device - device0);
        tt = fastf_res_now();
        if (level_row_(rate_cell, caps[j], seed, counters, nnz, S->h_upc[n_cells], S->h_upc, S->h_gpc, n_cells, H, (uint32_t)capped, row, sizeof row, metrics) ||
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
            tt = fastf_res_now();
            if (fastf_devmem_copy(h_thr, S->d_lo, (size_t)n_cells * 8) || write_thresholds(dir, L, n_cells, h_thr, h_ufull, S->h_upc)) goto done;
            T->write += fastf_res_now() - tt;
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
    fastf_devmem_free(d_plane);
    if (h_thr) fastf_pinned_free(h_thr);
    if (h_ufull) fastf_pinned_free(h_ufull);
    return rc;
}

static int level_resident(const char *bam_file, const char *out_dir, const char *barcodes, const char *features, const float *rc_list, uint32_t n_c,
                          const uint64_t *caps, uint32_t n_m, const uint32_t *seeds, uint32_t n_s, int summary_only, int device, FILE *tsv, res_genes_t *G,
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
    if (!pair_rate || !pair_seed) { lv_err("out of memory"); goto done; }
    for (uint32_t i = 0; i < n_c; i++) for (uint32_t k = 0; k < n_s; k++) { pair_rate[i * n_s + k] = rc_list[i]; pair_seed[i * n_s + k] = seeds[k]; }
    if ((rc = fastf_res_lists_load(barcodes, features, pair_rate, pair_seed, n_pairs, &LL)) != RES_OK) goto done;
    rc = RES_FAIL;
    S.max_cells = fastf_res_lists_max_cells(&LL);
    S.fidelity = Fd->on; S.gene_fid = Fd->gene_on; S.neighbors = Fd->nbr_on || Fd->lab_on; S.labels = Fd->lab_on; S.lab_t = Fd->labels; S.markers = Fd->markers;
    {   const char *nr = getenv("FASTF_RES_NO_REUSE"); S.no_reuse = nr && nr[0] == '1'; }
    T.lists = fastf_res_now() - tt; tt = fastf_res_now();
    if (fastf_res_decode("level", bam_file, &LL.L[0], device, &R)) goto done;
    T.decode = fastf_res_now() - tt;
    if (P->on) printf("level: %llu records resident on the device (%llu bytes), %u x %u points x %u seeds\n", (unsigned long long)R.n, (unsigned long long)(R.n * 24), n_c, n_m, n_s);
    else printf("level: %llu records resident on the device (%llu bytes), %u x %u points\n", (unsigned long long)R.n, (unsigned long long)(R.n * 24), n_c, n_m);
    for (uint32_t i = 0; i < n_c; i++) {
        if (fastf_res_reps_rate_begin(P, &LL.L[i * n_s], 1)) { rc = RES_FAIL; goto done; }
        for (uint32_t k = 0; k < n_s; k++) {
            const uint32_t at = i * n_s + k;
            rc = level_cell_rate(&S, &R, &LL.L[at], LL.keys[at], bam_file, out_dir, rc_list[i], caps, n_m, seeds[k], summary_only, device, tsv, G, C, Fd, P, k, &T, prof);
            if (rc != RES_OK) goto done;
        }
        if (fastf_res_reps_rate_end(P, rc_list[i], NULL, caps, &T)) { rc = RES_FAIL; goto done; }
    }
    rc = RES_OK;
    if (prof) {
        const uint32_t points = n_c * n_m * n_s;
        fprintf(stderr, "[level] lists %.3f s, decode to resident records %.3f s, engines %.3f s, layout+K1a %.3f s, planes of the points %.3f s, "
                        "per-point device work %.3f s (%.4f s a point), summary D2H+medians %.3f s, rows D2H %.3f s, writers %.3f s, total %.3f s\n",
                T.lists, T.decode, T.engine, T.block_k1a, T.planes, T.device, T.device / points, T.summary, T.d2h, T.write, fastf_res_now() - t0);
        fprintf(stderr, "[level] search: %u passes in all (%u with every hit kept, one per cell rate and seed; %.1f probing passes a point), %.3f s "
                        "(%.4f s a point, %.4f s a pass with its plane and step)\n",
                T.passes, n_c * n_s, (double)(T.passes - n_c * n_s) / points, T.search, T.search / points, T.passes ? T.search / T.passes : 0.0);
    }
    if (prof && P->on) fprintf(stderr, "[level] replicates: %u (cell rate, seed) pairs opened in %.3f s (engines %.3f s, buffers + layout + K1a %.3f s), the blocked copy "
                                       "laid out %u times; replicate tables and per-gene accumulation %.3f s\n", T.opens, T.engine + T.block_k1a, T.engine, T.block_k1a, T.relays, T.reps);
    if (prof && G->on) fprintf(stderr, "[level] --genes: per-gene D2H, rows and files %.3f s (the kernel is part of the per-point device work)\n", T.genes);
    if (prof && C->on) fprintf(stderr, "[level] --cells: full sort + K3u + copy summary + D2H %.3f s (%.4f s a point), rows and files %.3f s\n",
                               T.cells_dev, T.cells_dev / (n_c * n_m * n_s), T.cells);
    if (prof && Fd->on) fprintf(stderr, "[level] --fidelity: the full rows kept from %u first passes, the joins, their D2H, rows and files %.3f s\n", n_c * n_s, T.fidelity);
    if (prof && Fd->gene_on) fprintf(stderr, "[level] --gene-fidelity: %sthe partner counts, the per-gene sums, their D2H, rows and files %.3f s\n", Fd->on ? "" : "the full-depth rows of every pair, ", T.gene_fid);
    if (prof && Fd->mk_on) fprintf(stderr, "[level] --markers: top %u of the genes per label; the kernel calls on the planes, their D2H, the ranks, rows and files %.3f s\n", Fd->markers, T.markers);
    if (prof && Fd->lab_on) fprintf(stderr, "[level] --labels: %u labels, labels_unknown %llu; %sthe label arrays of every pair, the vote calls, their D2H, rows and files %.3f s\n", fastf_labels_count(Fd->labels),
                                    (unsigned long long)fastf_labels_unknown(Fd->labels), Fd->nbr_on ? "" : "the neighbour sets of --neighbors and what they need, ", T.labels + (Fd->nbr_on ? 0.0 : T.neighbors));
    if (prof && Fd->nbr_on) fprintf(stderr, "[level] --neighbors: %sthe planes, the Gram products and selections, the shared counts, their D2H, rows and files %.3f s\n", Fd->on || Fd->gene_on ? "" : "the full-depth rows and per-gene sums of every pair, ", T.neighbors);
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
/* reps != 0: a replicate run (fastf_level_reps) — the suffixed directories and the replicate tables, with one seed too */
static int level_run_(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                     const uint64_t *caps, uint32_t n_m, const uint32_t *seeds, uint32_t n_s, int reps, uint32_t flags, const fastf_labels_t *labels, uint32_t markers)
{
    if (!bam || !barcodes || !features) return lv_err("level: null argument");
    if (!out_dir) out_dir = ".";
    if (fastf_level_check_grid(rates_cell, n_c, caps, n_m)) return 1;
    if (flags & ~(uint32_t)(FASTF_LEVEL_SUMMARY_ONLY | FASTF_LEVEL_GENES | FASTF_LEVEL_CELLS | FASTF_LEVEL_FIDELITY | FASTF_LEVEL_GENE_FIDELITY | FASTF_LEVEL_NEIGHBORS)) return lv_err("level: unknown flags 0x%x", flags);
    const int summary_only = (flags & FASTF_LEVEL_SUMMARY_ONLY) != 0, genes = (flags & FASTF_LEVEL_GENES) != 0, cells = (flags & FASTF_LEVEL_CELLS) != 0;
    const int fidelity = (flags & FASTF_LEVEL_FIDELITY) != 0, gene_fidelity = (flags & FASTF_LEVEL_GENE_FIDELITY) != 0, neighbors = (flags & FASTF_LEVEL_NEIGHBORS) != 0;
    if (access(bam, R_OK) == -1) return lv_err("bam file: %s does not exist.", bam);
    int dev0 = 0, dev_second = -1;
    {   const char *dvs = getenv("FASTF_DEVICES");
        fastf_pick_devices(dvs, getenv("FASTF_DEVICE"), &dev0, &dev_second);
        if (dvs && *dvs && (strchr(dvs, ',') || atoi(dvs) >= 2))
            return labels ? lv_err("level: --labels needs the resident form, and this job is outside it (several devices), and a UMI cap has no point-by-point form") :
                   neighbors ? lv_err("level: --neighbors needs the resident form, and this job is outside it (several devices), and a UMI cap has no point-by-point form") :
                   gene_fidelity ? lv_err("level: --gene-fidelity needs the resident form, and this job is outside it (several devices), and a UMI cap has no point-by-point form")
                                 : lv_err("level: this job is outside the resident form (several devices), and a UMI cap has no point-by-point form"); }
    if (fastf_res_make_dir(out_dir)) return 1;
    res_tsv_t tsv; memset(&tsv, 0, sizeof tsv);
    if (fastf_res_tsv_open(&tsv, out_dir, "level.tsv", fastf_level_header())) return 1;
    res_genes_t G;
    if (fastf_res_genes_open(&G, genes, "level", out_dir, fastf_level_genes_header(), n_c * n_m, reps)) { fastf_res_tsv_close(&tsv, 0); return 1; }
    res_cells_t C;
    if (fastf_res_cells_open(&C, cells, "level", out_dir, fastf_level_cells_header())) { fastf_res_tsv_close(&tsv, 0); fastf_res_genes_close(&G, 0); return 1; }
    res_fid_t Fd;
    if (fastf_res_fid_open(&Fd, fidelity, gene_fidelity, "level", out_dir, fastf_level_fidelity_header(), fastf_level_gene_fidelity_header())) { fastf_res_tsv_close(&tsv, 0); fastf_res_genes_close(&G, 0); fastf_res_cells_close(&C, 0); return 1; }
    if (fastf_res_fid_open_neighbors(&Fd, neighbors, "level", out_dir, fastf_level_neighbors_header())) { fastf_res_tsv_close(&tsv, 0); fastf_res_genes_close(&G, 0); fastf_res_cells_close(&C, 0); fastf_res_fid_close(&Fd, 0); return 1; }
    if (fastf_res_fid_open_labels(&Fd, labels, "level", out_dir, fastf_level_labels_header(), fastf_level_label_classes_header())) { fastf_res_tsv_close(&tsv, 0); fastf_res_genes_close(&G, 0); fastf_res_cells_close(&C, 0); fastf_res_fid_close(&Fd, 0); return 1; }
    if (fastf_res_fid_open_markers(&Fd, markers, "level", out_dir, fastf_level_markers_header())) { fastf_res_tsv_close(&tsv, 0); fastf_res_genes_close(&G, 0); fastf_res_cells_close(&C, 0); fastf_res_fid_close(&Fd, 0); return 1; }
    res_reps_t P;
    if (fastf_res_reps_open(&P, reps, "level", out_dir, seeds, n_s, n_c, n_m, genes, dev0, fastf_level_reps_header(), fastf_level_genes_reps_header())) {
        fastf_res_tsv_close(&tsv, 0); fastf_res_genes_close(&G, 0); fastf_res_cells_close(&C, 0); fastf_res_fid_close(&Fd, 0); return 1;
    }
    int rc = level_resident(bam, out_dir, barcodes, features, rates_cell, n_c, caps, n_m, seeds, n_s, summary_only, dev0, tsv.f, &G, &C, &Fd, &P);
    if (rc == RES_NOT_COVERED && labels)
        lv_err("level: --labels needs the resident form, and this job is outside it (keys wider than 64 bits or UMIs beyond what a 64-bit key holds), and a UMI cap has no point-by-point form");
    else if (rc == RES_NOT_COVERED && neighbors)
        lv_err("level: --neighbors needs the resident form, and this job is outside it (keys wider than 64 bits or UMIs beyond what a 64-bit key holds), and a UMI cap has no point-by-point form");
    else if (rc == RES_NOT_COVERED && gene_fidelity)
        lv_err("level: --gene-fidelity needs the resident form, and this job is outside it (keys wider than 64 bits or UMIs beyond what a 64-bit key holds), and a UMI cap has no point-by-point form");
    else if (rc == RES_NOT_COVERED)
        lv_err("level: this job is outside the resident form (keys wider than 64 bits or UMIs beyond what a 64-bit key holds), and a UMI cap has no point-by-point form");
    if (!rc && fastf_res_genes_close(&G, 1)) rc = 1;
    if (!rc && fastf_res_cells_close(&C, 1)) rc = 1;
    if (!rc && fastf_res_fid_close(&Fd, 1)) rc = 1;
    if (!rc && fastf_res_reps_close_grid(&P, 1, rates_cell, NULL, caps)) rc = 1;
    if (rc) {
        char keep[512]; snprintf(keep, sizeof keep, "%s", fastf_last_error());
        fastf_res_tsv_close(&tsv, 0); fastf_res_genes_close(&G, 0); fastf_res_cells_close(&C, 0); fastf_res_fid_close(&Fd, 0); fastf_res_reps_close(&P, 0);
        fastf_res_reps_unlink_tables(out_dir, "level");     /* (the tables that were already renamed go too: none is left) */
        fastf_set_error_(keep);
        return 1;
    }
    if (fastf_res_tsv_close(&tsv, 1)) { fastf_res_reps_unlink_tables(out_dir, "level"); return 1; }
    return 0;
}

/* labels_path != NULL: the labels file is read and checked before anything is written */
static int level_run(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                   const uint64_t *caps, uint32_t n_l, const uint32_t *seeds, uint32_t n_s, int reps, uint32_t flags, const char *labels_path, uint32_t markers)
{
    if (!labels_path) return level_run_(bam, out_dir, barcodes, features, rates_cell, n_c, caps, n_l, seeds, n_s, reps, flags, NULL, 0);
    if (!bam || !barcodes || !features) return lv_err("level: null argument");
    if (access(bam, R_OK) == -1) return lv_err("bam file: %s does not exist.", bam);
    fastf_labels_t *labels = NULL;
    if (fastf_labels_load(labels_path, barcodes, &labels)) return 1;
    const int rc = level_run_(bam, out_dir, barcodes, features, rates_cell, n_c, caps, n_l, seeds, n_s, reps, flags, labels, markers);
    fastf_labels_free(labels);
    return rc;
}

int fastf_level_labels(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                     const uint64_t *umi_caps, uint32_t n_m, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path)
{
    if (!n_seeds) return level_run(bam, out_dir, barcodes, features, rates_cell, n_c, umi_caps, n_m, &seed, 1, 0, flags, labels_path, 0);
    if (fastf_check_seeds_("level", seeds, n_seeds)) return 1;
    return level_run(bam, out_dir, barcodes, features, rates_cell, n_c, umi_caps, n_m, seeds, n_seeds, 1, flags, labels_path, 0);
}

/* --markers N: the labels run with the marker tables beside it */
int fastf_level_markers(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                       const uint64_t *umi_caps, uint32_t n_m, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags, uint32_t seed, const char *labels_path,
                       uint32_t markers)
{
    if (markers < 1 || markers > FASTF_MARKERS_MAX) return lv_err("level: --markers: N = %u, from 1 to %u", markers, FASTF_MARKERS_MAX);
    if (!labels_path) return lv_err("level: --markers needs --labels");
    if (!n_seeds) return level_run(bam, out_dir, barcodes, features, rates_cell, n_c, umi_caps, n_m, &seed, 1, 0, flags, labels_path, markers);
    if (fastf_check_seeds_("level", seeds, n_seeds)) return 1;
    return level_run(bam, out_dir, barcodes, features, rates_cell, n_c, umi_caps, n_m, seeds, n_seeds, 1, flags, labels_path, markers);
}

int fastf_level(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                const uint64_t *umi_caps, uint32_t n_m, uint32_t seed, uint32_t flags)
{
    return level_run(bam, out_dir, barcodes, features, rates_cell, n_c, umi_caps, n_m, &seed, 1, 0, flags, NULL, 0);
}

int fastf_level_reps(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                     const uint64_t *umi_caps, uint32_t n_m, const uint32_t *seeds, uint32_t n_seeds, uint32_t flags)
{
    if (fastf_check_seeds_("level", seeds, n_seeds)) return 1;
    return level_run(bam, out_dir, barcodes, features, rates_cell, n_c, umi_caps, n_m, seeds, n_seeds, 1, flags, NULL, 0);
}

static void usage_level(FILE *f)
{
    fprintf(f,
            "Usage: fastF level [options]\n\n"
            "every cell downsampled to at most M UMIs, exactly: the deepest read-level subsample of each cell whose UMI count does not\n"
            "exceed M, over a grid of cell rates and UMI caps from one decode of the bam file: per point <out>/c<cell>_m<M>/ with the three\n"
            "files of bam2db and thresholds.tsv.gz, and <out>/level.tsv with one summary row per point.\n\n"
            "    -h, --help            show this help message and exit\n"
            "    -b, --bam=<str>       path to bam file\n"
            "    -f, --feature=<str>   path to feature list file\n"
            "    -a, --barcode=<str>   path to barcode list file\n"
            "    -d, --dbname=<str>    name of database (accepted for compatibility, ignored)\n"
            "    -c, --cell=<list>     rates of cell barcode, comma separated (default 1.0)\n"
            "    -m, --umis=<list>     UMIs per cell at most, comma separated integers >= 1\n"
            "    -o, --out=<str>       path to output directory (default .)\n"
            "    -s, --seed=<int>      seed for random number generator (default 926)\n"
            "        --summary-only    write level.tsv alone\n"
            "        --genes           per-gene detection too: level_genes.tsv, level_gene_cells.tsv.gz and genes.tsv.gz per point\n"
            "        --cells           per-cell reads, saturation and UMI copy numbers too: level_cells.tsv and cells.tsv.gz per point\n"
            "        --fidelity        every point against the full-depth data of the same cells (every read of the sampled cells kept):\n"
            "                          level_fidelity.tsv and fidelity.tsv.gz per point, with the Pearson and the cosine of the RAW counts\n"
            "                          over ALL genes per cell (not log-normalised)\n"
            "        --gene-fidelity   every point against the full-depth data of the same cells, per GENE: level_gene_fidelity.tsv and\n"
            "                          gene_fidelity.tsv.gz per point, with the Pearson of the RAW counts over ALL sampled cells per gene,\n"
            "                          the dispersion (variance / mean) at full depth and at the point, and the overlap of the 2000\n"
            "                          most variable genes\n"
            "        --neighbors       every point against the full-depth data of the same cells, BETWEEN the cells: level_neighbors.tsv and\n"
            "                          neighbors.tsv.gz per point, with the share of a cell's 15 nearest neighbours at full depth (cosine of\n"
            "                          the RAW counts over the 2000 most variable genes, decided in exact integers) that it keeps\n"
            "        --labels=<file>   one `barcode<TAB>label` per line (cell types of the full-depth analysis): level_labels.tsv,\n"
            "                          level_label_classes.tsv and labels.tsv.gz, label_confusion.tsv.gz per point, with the share of labelled\n"
            "                          cells whose 15 nearest neighbours still vote for their own label, at full depth and at the point\n"
            "        --markers=<N>     with --labels: per label the N (1 to 2000) best marker genes among the 2000 most variable, ranked by the\n"
            "                          exact AUC of the label's cells against the other labelled cells, at full depth and at the point:\n"
            "                          level_markers.tsv and markers.tsv.gz per point\n"
            "        --seeds=<list>    replicates: the grid at each of 1 to 64 seeds, comma separated, from the one decode; per point and\n"
            "                          seed <out>/c<cell>_m<M>_s<seed>/, one level.tsv row each, and level_reps.tsv with mean, sd, min and\n"
            "                          max of every metric per grid point (with --genes level_genes_reps.tsv and level_gene_reps.tsv.gz\n"
            "                          in place of level_gene_cells.tsv.gz); not with -s or --reps\n"
            "        --reps=<int>      the same at the seeds s, s + 1, .. s + N - 1 (s: -s; N from 1 to 64)\n");
}

#define LEVEL_MAX_POINTS 64
int cmd_level(int argc, const char **argv)
{
    res_args_t A;
    const int prc = fastf_res_parse_args(argc, argv, 'm', "umis", usage_level, "level does not write umi.tsv.gz (-u).", &A);
    if (prc) return prc == 2 ? 0 : 1;
    float rc[LEVEL_MAX_POINTS]; uint64_t caps[LEVEL_MAX_POINTS];
    uint32_t n_c = 0, n_m = 0;
    if (!A.list) { fprintf(stderr, "\x1b[31mError:\x1b[0m level needs -m <list>: the UMIs per cell at most\n"); return 1; }
    if (fastf_sweep_parse_rates(A.cells, 1, rc, LEVEL_MAX_POINTS, &n_c) || fastf_level_parse_caps(A.list, caps, LEVEL_MAX_POINTS, &n_m) ||
        fastf_level_check_grid(rc, n_c, caps, n_m)) {
        fprintf(stderr, "\x1b[31mError:\x1b[0m %s\n", fastf_last_error());
        return 1;
    }
    if (fastf_res_check_inputs(&A)) return 1;
    const uint32_t flags = (A.summary_only ? FASTF_LEVEL_SUMMARY_ONLY : 0) | (A.genes ? FASTF_LEVEL_GENES : 0) | (A.per_cell ? FASTF_LEVEL_CELLS : 0) | (A.fidelity ? FASTF_LEVEL_FIDELITY : 0) |
                           (A.gene_fidelity ? FASTF_LEVEL_GENE_FIDELITY : 0) | (A.neighbors ? FASTF_LEVEL_NEIGHBORS : 0);
    if (A.markers ? fastf_level_markers(A.bam, A.out, A.bar, A.feat, rc, n_c, caps, n_m, A.seeds, A.n_seeds, flags, A.seed, A.labels, A.markers) :
        A.labels ? fastf_level_labels(A.bam, A.out, A.bar, A.feat, rc, n_c, caps, n_m, A.seeds, A.n_seeds, flags, A.seed, A.labels) :
        A.n_seeds ? fastf_level_reps(A.bam, A.out, A.bar, A.feat, rc, n_c, caps, n_m, A.seeds, A.n_seeds, flags)
                  : fastf_level(A.bam, A.out, A.bar, A.feat, rc, n_c, caps, n_m, A.seed, flags)) {
        fprintf(stderr, "\x1b[31mError:\x1b[0m level failed: %s\n", fastf_last_error());
        return 1;
    }
    if (A.genes && A.n_seeds) printf("level_genes.tsv, level_genes_reps.tsv and level_gene_reps.tsv.gz are generated.\n");
    else if (A.genes) printf("level_genes.tsv and level_gene_cells.tsv.gz are generated.\n");
    if (A.per_cell) printf("level_cells.tsv is generated.\n");
    if (A.fidelity) printf("level_fidelity.tsv is generated.\n");
    if (A.gene_fidelity) printf("level_gene_fidelity.tsv is generated.\n");
    if (A.neighbors) printf("level_neighbors.tsv is generated.\n");
    if (A.labels) printf("level_labels.tsv and level_label_classes.tsv are generated.\n");
    if (A.markers) printf("level_markers.tsv is generated.\n");
    if (A.n_seeds) printf("level_reps.tsv is generated.\n");
    printf("level.tsv is generated.\n");
    return 0;
}
