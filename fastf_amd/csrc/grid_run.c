/*
 * grid_run.c — the driver of `fastF sweep`, `fastF cap` and `fastF level` (resident.h: res_job_t, res_verb_t): the one way in of the
 * entry points (fastf_res_grid_entry, at the end), their checks, the tables of the run, the (cell rate, seed) pairs on ONE res_rate_t, the
 * body of every point, the close.  A verb hands in
 * its descriptor; what it does by itself — making the decision plane of a point — it does in the hooks.  A further comparison of a
 * point against full depth is a descriptor and a writer in res_tables.c and a device stage in fastf_res_point_compare (resident.c);
 * here it has only its option and its profile line.
 */
#define _GNU_SOURCE
#include "resident.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#define GRID_FLAGS (FASTF_SWEEP_SUMMARY_ONLY | FASTF_SWEEP_GENES | FASTF_SWEEP_CELLS | FASTF_SWEEP_FIDELITY | FASTF_SWEEP_GENE_FIDELITY | FASTF_SWEEP_NEIGHBORS | FASTF_SWEEP_COEXPRESSION)

/* the first two checks of --markers N */
static int check_markers(const char *verb, uint32_t markers, const char *labels_path)
{
    if (markers < 1 || markers > FASTF_MARKERS_MAX) return fastf_res_err("%s: --markers: N = %u, from 1 to %u", verb, markers, FASTF_MARKERS_MAX);
    return labels_path ? 0 : fastf_res_err("%s: --markers needs --labels", verb);
}

/* seeds[] of a replicate run: 1 .. FASTF_MAX_SEEDS distinct values */
static int check_seeds(const char *verb, const uint32_t *seeds, uint32_t n_seeds)
{
    if (!seeds || n_seeds < 1 || n_seeds > FASTF_MAX_SEEDS) return fastf_res_err("%s: a replicate run takes 1 to %u seeds", verb, FASTF_MAX_SEEDS);
    for (uint32_t k = 0; k < n_seeds; k++)
        for (uint32_t j = 0; j < k; j++) if (seeds[j] == seeds[k]) return fastf_res_err("%s: seed %u is listed twice", verb, seeds[k]);
    return 0;
}

/* ------------------------------------------------------------------ */
/* a job outside the resident form                                     */
/* ------------------------------------------------------------------ */
/* The option that needs the resident form is named, the first of the order below that is set.  A verb with a point-by-point form
 * (sweep) refuses --cells and --fidelity by name too — --cells first where the job is known to be outside before the run
 * (cells_first), last behind a resident attempt — and returns 0 with no option set: the job falls back.  A verb without one refuses
 * every such job, with its tail.  1: refused, the message set */
static int grid_refuse(const res_verb_t *V, const res_job_t *job, int labels, int cells_first, const char *why)
{
    const int fallback = V->point_by_point != NULL;
    const uint32_t f = job->flags;
    const char *const tail = V->refusal_tail ? V->refusal_tail : "";
    const char *opt = NULL, *needs = "needs";
    if (fallback && cells_first && (f & FASTF_SWEEP_CELLS)) opt = "--cells";
    else if (labels) opt = "--labels";
    else if (f & FASTF_SWEEP_NEIGHBORS) opt = "--neighbors";
    else if (job->mapping) opt = "--mapping";
    else if (job->ptime_path) opt = "--pseudotime";
    else if (f & FASTF_SWEEP_COEXPRESSION) opt = "--coexpression";
    else if (fallback && (f & FASTF_SWEEP_FIDELITY) && (f & FASTF_SWEEP_GENE_FIDELITY)) { opt = "--fidelity and --gene-fidelity"; needs = "need"; }
    else if (fallback && (f & FASTF_SWEEP_FIDELITY)) opt = "--fidelity";      /* (the full rows live on the device alone: bam2db() point by point has none) */
    else if (f & FASTF_SWEEP_GENE_FIDELITY) opt = "--gene-fidelity";
    else if (fallback && (f & FASTF_SWEEP_CELLS)) opt = "--cells";            /* (the per-cell rows come from the device's keys alone) */
    if (opt) return fastf_res_err("%s: %s %s the resident form, and this job is outside it (%s)%s", V->name, opt, needs, why, tail);
    return fallback ? 0 : fastf_res_err("%s: this job is outside the resident form (%s)%s", V->name, why, tail);
}

/* ------------------------------------------------------------------ */
/* the tables of a run                                                 */
/* ------------------------------------------------------------------ */
static void grid_close(res_tables_t *tb)
{
    fastf_res_tsv_close(&tb->tsv, 0); fastf_res_genes_close(&tb->G, 0); fastf_res_cells_close(&tb->C, 0); fastf_res_cmp_close(&tb->Fd, 0); fastf_res_reps_close(&tb->P, 0);
}

/* on failure the caller closes what was opened (grid_close) */
static int grid_open(const res_verb_t *V, const res_job_t *job, const fastf_labels_t *labels, const fastf_ptime_t *ptime, int device, res_tables_t *tb)
{
    const uint32_t f = job->flags;
    const int genes = (f & FASTF_SWEEP_GENES) != 0;
    const char *const out = job->out_dir;
    char name[64];
    memset(tb, 0, sizeof *tb);
    snprintf(name, sizeof name, "%s.tsv", V->name);
    return fastf_res_tsv_open(&tb->tsv, out, name, V->header()) ||
           fastf_res_genes_open(&tb->G, genes, V, out, job->n_c * job->n_list, job->reps) ||
           fastf_res_cells_open(&tb->C, (f & FASTF_SWEEP_CELLS) != 0, V, out) ||
           fastf_res_cmp_open(&tb->Fd, V, out, f, labels, job->markers, job->mapping, ptime) ||
           fastf_res_reps_open(&tb->P, job->reps, V, out, job->seeds, job->n_s, job->n_c, job->n_list, genes, device);
}

/* ------------------------------------------------------------------ */
/* one (cell rate, seed) pair — seed k_seed of a replicate run — on the run's res_rate_t */
/* ------------------------------------------------------------------ */
static int grid_pair(const res_verb_t *V, const res_pair_t *p, const uint64_t *cell_keys, res_tables_t *tb, uint32_t k_seed)
{
    const res_job_t *const job = p->job;
    res_rate_t *const S = p->S;
    res_times_t *const T = p->T;
    res_genes_t *const G = &tb->G; res_cells_t *const C = &tb->C; res_reps_t *const P = &tb->P;
    void *ctx = NULL;
    int rc = fastf_res_rate_open(S, V->name, p->R, p->L, cell_keys, p->rate_cell, p->seed, p->device, G->on, C->on, T);
    if (rc != RES_OK) return rc;
    if ((rc = V->pair_begin(p, &ctx)) != RES_OK) goto done;
    rc = RES_FAIL;

    for (uint32_t j = 0; j < job->n_list; j++) {
        char base[64], name[96], dir[4096], row[640];
        uint64_t counters[3], nnz = 0;
        double metrics[FASTF_REPS_METRICS];
        const uint32_t *d_plane = NULL;
        const float rd = job->rates_depth ? job->rates_depth[j] : 0.0f;      /* the list value: ONE of the two */
        const uint64_t lv = job->caps ? job->caps[j] : 0;
        if (job->caps ? V->caps_point_dir(p->rate_cell, lv, base, sizeof base) : fastf_sweep_point_dir(p->rate_cell, rd, base, sizeof base)) goto done;
        if (P->on ? fastf_reps_point_dir(base, p->seed, name, sizeof name) : (snprintf(name, sizeof name, "%s", base), 0)) goto done;
        int prc = V->point_plane(ctx, p, j, name, &d_plane);
        if (prc == RES_OK) prc = fastf_res_point_run(S, d_plane, name, counters, &nnz, T);
        if (prc != RES_OK) { rc = prc; goto done; }
        if (V->point_done) V->point_done(ctx, p, name);
        double tt = fastf_res_now();
        if (V->point_row(ctx, p, j, counters, nnz, row, sizeof row, metrics) || fastf_res_reps_point(P, j, k_seed, S->n_cells, metrics)) goto done;
        T->summary += fastf_res_now() - tt;
        if (fastf_res_point_compare(S, name, T)) goto done;
        if (G->on && P->on) {                               /* (the point's per-gene array is still on the device) */
            tt = fastf_res_now();
            if (fastf_res_reps_genes(P, S, j, k_seed, S->buf.h_cpg.u32, S->n_features)) goto done;
            T->reps += fastf_res_now() - tt;
        }
        if (!p->summary_only) {
            snprintf(dir, sizeof dir, "%s/%s", job->out_dir, name);
            if (fastf_res_point_write(S, dir, job->bam, job->caps ? fastf_cap_realised(counters[1], S->H) : rd, counters, nnz, T)) goto done;
            if (V->point_files && V->point_files(ctx, p, dir)) goto done;
        }
        if (fastf_res_cmp_point(&tb->Fd, S, p->summary_only ? NULL : dir, rd, lv, T)) goto done;
        if (G->on) {
            char grow[256];
            tt = fastf_res_now();
            if (fastf_genes_summary_row(p->rate_cell, rd, lv, p->seed, S->buf.h_cpg.u32, S->buf.h_upg.u64, S->n_features, grow, sizeof grow) ||
                fastf_res_genes_point(G, p->L, name, p->summary_only ? NULL : dir, grow, S->buf.h_cpg.u32, S->buf.h_upg.u64)) goto done;
            T->genes += fastf_res_now() - tt;
        }
        if (C->on) {                                        /* (behind the point's rows: K3u overwrites the regions they were gathered from) */
            char crow[1024];
            if (fastf_res_point_cells(S, name, T)) goto done;
            tt = fastf_res_now();
            if (fastf_cells_summary_row(p->rate_cell, rd, lv, p->seed, S->h_cs.rpc, S->h_cs.npc, S->h_cs.spc, S->n_cells, S->h_cs.hist, crow, sizeof crow) ||
                fastf_res_cells_point(C, S, p->summary_only ? NULL : dir, crow)) goto done;
            T->cells += fastf_res_now() - tt;
        }
        fputs(row, tb->tsv.f);
    }
    rc = RES_OK;
done:
    V->pair_end(ctx);
    return rc;
}

/* ------------------------------------------------------------------ */
/* the resident form: one decode, then the pairs                       */
/* ------------------------------------------------------------------ */
static int grid_resident(const res_verb_t *V, const res_job_t *job, int device, res_tables_t *tb)
{
    int rc = RES_FAIL;
    const res_cmp_t *const Fd = &tb->Fd;
    const uint32_t n_c = job->n_c, n_s = job->n_s, points = n_c * job->n_list * n_s;
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
    if (!pair_rate || !pair_seed) { fastf_res_err("out of memory"); goto done; }
    for (uint32_t i = 0; i < n_c; i++) for (uint32_t k = 0; k < n_s; k++) { pair_rate[i * n_s + k] = job->rates_cell[i]; pair_seed[i * n_s + k] = job->seeds[k]; }
    if ((rc = fastf_res_lists_load(job->barcodes, job->features, pair_rate, pair_seed, n_pairs, &LL)) != RES_OK) goto done;
    rc = RES_FAIL;
    S.cfg.max_cells = fastf_res_lists_max_cells(&LL);
    fastf_res_cmp_cfg(Fd, &S.cfg);
    {   const char *nr = getenv("FASTF_RES_NO_REUSE"); S.cfg.no_reuse = nr && nr[0] == '1'; }
    T.lists = fastf_res_now() - tt; tt = fastf_res_now();
    if (fastf_res_decode(V->name, job->bam, &LL.L[0], device, &R)) goto done;
    T.decode = fastf_res_now() - tt;
    printf("%s: %llu records resident on the device (%llu bytes), %u x %u points", V->name, (unsigned long long)R.n, (unsigned long long)(R.n * 24), n_c, job->n_list);
    if (tb->P.on) printf(" x %u seeds", n_s);
    printf("\n");

    for (uint32_t i = 0; i < n_c; i++) {
        if (fastf_res_reps_rate_begin(&tb->P, &LL.L[i * n_s], 1)) { rc = RES_FAIL; goto done; }
        for (uint32_t k = 0; k < n_s; k++) {
            const uint32_t at = i * n_s + k;
            const res_pair_t pair = { job, &S, &R, &LL.L[at], &T, job->rates_cell[i], job->seeds[k], device, (job->flags & FASTF_SWEEP_SUMMARY_ONLY) != 0, prof };
            if ((rc = grid_pair(V, &pair, LL.keys[at], tb, k)) != RES_OK) goto done;
        }
        if (fastf_res_reps_rate_end(&tb->P, job->rates_cell[i], job->rates_depth, job->caps, &T)) { rc = RES_FAIL; goto done; }
    }
    rc = RES_OK;
    if (prof) {
        const char *const v = V->name;
        fprintf(stderr, "[%s] lists %.3f s, decode to resident records %.3f s, engines %.3f s, layout+K1a %.3f s, %s %.3f s, "
                        "per-point device work %.3f s (%.4f s a point), summary D2H+medians %.3f s, rows D2H %.3f s, writers %.3f s, total %.3f s\n",
                v, T.lists, T.decode, T.engine, T.block_k1a, V->planes_words, T.planes, T.device, T.device / points, T.summary, T.d2h, T.write, fastf_res_now() - t0);
        if (V->run_profile) V->run_profile(job, &T);
        if (tb->P.on) fprintf(stderr, "[%s] replicates: %u (cell rate, seed) pairs opened in %.3f s (engines %.3f s, buffers + layout + K1a %.3f s), the blocked copy "
                                      "laid out %u times; replicate tables and per-gene accumulation %.3f s\n", v, T.opens, T.engine + T.block_k1a, T.engine, T.block_k1a, T.relays, T.reps);
        if (tb->G.on) fprintf(stderr, "[%s] --genes: per-gene D2H, rows and files %.3f s (the kernel is part of the per-point device work)\n", v, T.genes);
        if (tb->C.on) fprintf(stderr, "[%s] --cells: full sort + K3u + copy summary + D2H %.3f s (%.4f s a point), rows and files %.3f s\n", v, T.cells_dev, T.cells_dev / points, T.cells);
        const int fid = res_cmp_on(Fd, CMP_FIDELITY), gene_fid = res_cmp_on(Fd, CMP_GENE_FID), nbr = res_cmp_on(Fd, CMP_NEIGHBORS);
        if (fid) fprintf(stderr, "[%s] --fidelity: %s%u%s, the joins, their D2H, rows and files %.3f s\n", v, V->fid_before, n_pairs, V->fid_after, T.fidelity);
        if (gene_fid) fprintf(stderr, "[%s] --gene-fidelity: %sthe partner counts, the per-gene sums, their D2H, rows and files %.3f s\n", v, fid ? "" : "the full-depth rows of every pair, ", T.gene_fid);
        if (res_cmp_on(Fd, CMP_MARKERS)) fprintf(stderr, "[%s] --markers: top %u of the genes per label; the kernel calls on the planes, their D2H, the ranks, rows and files %.3f s\n", v, Fd->markers, T.markers);
        if (res_cmp_on(Fd, CMP_LABELS)) fprintf(stderr, "[%s] --labels: %u labels, labels_unknown %llu; %sthe label arrays of every pair, the vote calls, their D2H, rows and files %.3f s\n", v, fastf_labels_count(Fd->labels),
                                (unsigned long long)fastf_labels_unknown(Fd->labels), nbr ? "" : "the neighbour sets of --neighbors and what they need, ", T.labels + (nbr ? 0.0 : T.neighbors));
        if (nbr) fprintf(stderr, "[%s] --neighbors: %sthe planes, the Gram products and selections, the shared counts, their D2H, rows and files %.3f s\n", v, fid || gene_fid ? "" : "the full-depth rows and per-gene sums of every pair, ", T.neighbors);
        if (res_cmp_on(Fd, CMP_MAPPING)) fprintf(stderr, "[%s] --mapping: %sthe copy of the full planes, the mapping calls, the shared counts%s, their D2H, rows and files %.3f s\n", v,
                                                 nbr || res_cmp_on(Fd, CMP_LABELS) ? "" : "the neighbour sets of --neighbors and what they need, ", res_cmp_on(Fd, CMP_LABELS) ? " and votes" : "",
                                                 T.mapping + (nbr || res_cmp_on(Fd, CMP_LABELS) ? 0.0 : T.neighbors));
        if (res_cmp_on(Fd, CMP_PTIME)) fprintf(stderr, "[%s] --pseudotime: %llu values, pseudotime_unknown %llu; %sthe ranks of every pair, the median and census calls, their D2H, rows and files %.3f s\n", v,
                                               (unsigned long long)fastf_ptime_valued(Fd->ptime), (unsigned long long)fastf_ptime_unknown(Fd->ptime),
                                               nbr || res_cmp_on(Fd, CMP_LABELS) || res_cmp_on(Fd, CMP_MAPPING) ? "" : "the neighbour sets of --neighbors and what they need, ",
                                               T.ptime + (nbr || res_cmp_on(Fd, CMP_LABELS) || res_cmp_on(Fd, CMP_MAPPING) ? 0.0 : T.neighbors));
        if (res_cmp_on(Fd, CMP_COEXPR)) fprintf(stderr, "[%s] --coexpression: %sthe gene-major planes, the Gram sums and selections, the shared counts, their D2H, rows and files %.3f s\n", v,
                                                fid || gene_fid || nbr || res_cmp_on(Fd, CMP_LABELS) ? "" : "the full-depth rows and per-gene sums of every pair, ", T.coexpr);
    }
done:
    fastf_res_rate_close(&S);
    fastf_res_free(&R);
    fastf_res_lists_free(&LL);
    free(pair_rate); free(pair_seed);
    return rc;
}

/* ------------------------------------------------------------------ */
/* the run of an entry point                                           */
/* ------------------------------------------------------------------ */
#define NOT_COVERED_WHY "keys wider than 64 bits or UMIs beyond what a 64-bit key holds"
static int grid_run_(const res_verb_t *V, const res_job_t *job, const fastf_labels_t *labels, const fastf_ptime_t *ptime)
{
    if (V->check_caps ? V->check_caps(job->rates_cell, job->n_c, job->caps, job->n_list) : fastf_sweep_check_grid(job->rates_cell, job->n_c, job->rates_depth, job->n_list)) return 1;
    if (job->flags & ~(uint32_t)GRID_FLAGS) return fastf_res_err("%s: unknown flags 0x%x", V->name, job->flags);
    if (access(job->bam, R_OK) == -1) return fastf_res_err("bam file: %s does not exist.", job->bam);
    int dev0 = 0, dev_second = -1, several = 0;
    {   const char *dvs = getenv("FASTF_DEVICES");
        fastf_pick_devices(dvs, getenv("FASTF_DEVICE"), &dev0, &dev_second);
        several = dvs && *dvs && (strchr(dvs, ',') || atoi(dvs) >= 2); }
    if (several && grid_refuse(V, job, labels != NULL, 1, "several devices")) return 1;
    if (fastf_res_make_dir(job->out_dir)) return 1;
    res_tables_t tb;
    char keep[512];
    int rc = RES_FAIL, ran = 0;                             /* ran: a failure of the run, not of an open — the replicate tables may have to go */
    if (grid_open(V, job, labels, ptime, dev0, &tb)) goto fail;
    ran = 1;
    rc = several ? RES_NOT_COVERED : grid_resident(V, job, dev0, &tb);
    if (rc == RES_NOT_COVERED && !grid_refuse(V, job, labels != NULL, 0, NOT_COVERED_WHY)) {
        /* (wide keys and a UMI length set beyond the key are known before the first point; a UMI found too long among the records stops
         * the point that meets it.  Rows a resident attempt had written are of no use: the tables start again) */
        fprintf(stderr, "%s: this job is outside the resident form (%s): running bam2db point by point\n", V->name, several ? "several devices" : NOT_COVERED_WHY);
        grid_close(&tb);
        ran = 0;
        if (grid_open(V, job, labels, ptime, dev0, &tb)) goto fail;
        ran = 1;
        rc = V->point_by_point(job, (job->flags & FASTF_SWEEP_SUMMARY_ONLY) != 0, &tb);
    }
    if (rc || fastf_res_genes_close(&tb.G, 1) || fastf_res_cells_close(&tb.C, 1) || fastf_res_cmp_close(&tb.Fd, 1) ||
        fastf_res_reps_close_grid(&tb.P, 1, job->rates_cell, job->rates_depth, job->caps) || fastf_res_tsv_close(&tb.tsv, 1)) goto fail;
    return 0;
fail:
    snprintf(keep, sizeof keep, "%s", fastf_last_error());
    grid_close(&tb);
    if (ran && (job->reps || V->unlink_reps_always)) fastf_res_reps_unlink_tables(job->out_dir, V->name);      /* (the tables that were already renamed go too: none is left) */
    fastf_set_error_(keep);
    return 1;
}

int fastf_res_grid_run(const res_verb_t *V, const res_job_t *asked)
{
    res_job_t job = *asked;
    if (job.reps && check_seeds(V->name, job.seeds, job.n_s)) return 1;
    if (!job.bam || !job.barcodes || !job.features) return fastf_res_err("%s: null argument", V->name);
    if (!job.out_dir) job.out_dir = ".";
    fastf_labels_t *labels = NULL;                          /* the labels file is read and checked before anything is written */
    if (job.labels_path) {
        if (access(job.bam, R_OK) == -1) return fastf_res_err("bam file: %s does not exist.", job.bam);
        if (fastf_labels_load(job.labels_path, job.barcodes, &labels)) return 1;
    }
    fastf_ptime_t *ptime = NULL;                            /* the pseudotime file likewise */
    if (job.ptime_path) {
        if (access(job.bam, R_OK) == -1) { fastf_labels_free(labels); return fastf_res_err("bam file: %s does not exist.", job.bam); }
        if (fastf_ptime_load(job.ptime_path, job.barcodes, &ptime)) { fastf_labels_free(labels); return 1; }
    }
    const int rc = grid_run_(V, &job, labels, ptime);
    fastf_labels_free(labels); fastf_ptime_free(ptime);
    return rc;
}

/* ------------------------------------------------------------------ */
/* the one way in of the eighteen entry points                         */
/* ------------------------------------------------------------------ */
/* The union of their arguments, `seed` by value.  A replicate run: n_seeds != 0, or ENTRY_REPS (fastf_<verb>_reps, whose n_seeds == 0 the
 * driver's seed check then refuses); otherwise the plain run at `seed`.  mapping beyond 1 is refused first; N of --markers and its labels
 * path are checked where N != 0, and with ENTRY_MARKERS (fastf_<verb>_markers) always */
int fastf_res_grid_entry(const res_verb_t *V, unsigned how, const char *bam, const char *out_dir, const char *barcodes, const char *features,
                         const float *rates_cell, uint32_t n_c, const float *rates_depth, const uint64_t *caps, uint32_t n_list,
                         const uint32_t *seeds, uint32_t n_seeds, uint32_t seed, uint32_t flags,
                         const char *labels_path, uint32_t markers, uint32_t mapping, const char *ptime_path)
{
    const int reps = (how & ENTRY_REPS) || n_seeds != 0;
    const res_job_t job = { .bam = bam, .out_dir = out_dir, .barcodes = barcodes, .features = features, .rates_cell = rates_cell, .n_c = n_c,
                            .rates_depth = rates_depth, .caps = caps, .n_list = n_list, .seeds = reps ? seeds : &seed, .n_s = reps ? n_seeds : 1, .reps = reps,
                            .flags = flags, .labels_path = labels_path, .markers = markers, .mapping = mapping, .ptime_path = ptime_path };
    if (mapping > 1) return fastf_res_err("%s: --mapping: %u, 0 or 1", V->name, mapping);
    if (((how & ENTRY_MARKERS) || markers) && check_markers(V->name, markers, labels_path)) return 1;
    return fastf_res_grid_run(V, &job);
}
