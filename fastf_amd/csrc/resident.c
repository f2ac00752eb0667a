/*
 * resident.c — the resident pipeline of `fastF sweep` and `fastF cap` (resident.h): list loading with one dictionary, the decode
 * of the BAM into device-resident records, per cell rate the engine + the records in its layout + K1a, per point K1b / sort /
 * reduce / gather / summary and the writers.
 */
#define _GNU_SOURCE
#include "resident.h"

#include <errno.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

double fastf_res_now(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + t.tv_nsec * 1e-9; }
static int rs_err(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static int rs_err(const char *fmt, ...)
{
    char buf[480];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    fastf_set_error_(buf);
    return 1;
}

int fastf_res_make_dir(const char *path)
{
    if (mkdir(path, 0777) == 0 || errno == EEXIST) return 0;
    return rs_err("cannot create directory %s: %s", path, strerror(errno));
}

static uint32_t bits_for(uint64_t v) { uint32_t b = 0; while (b < 64 && (v >> b)) b++; return b ? b : 1; }

/* ------------------------------------------------------------------ */
/* lists                                                               */
/* ------------------------------------------------------------------ */
void fastf_res_lists_free(res_lists_t *l)
{
    if (l->keys) for (uint32_t i = 0; i < l->n; i++) free(l->keys[i]);
    free(l->keys);
    if (l->L) for (uint32_t i = 0; i < l->n; i++) fastf_lists_free(&l->L[i]);
    free(l->L);
    memset(l, 0, sizeof *l);
}

int fastf_res_lists_load(const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c, uint32_t seed, res_lists_t *out)
{
    memset(out, 0, sizeof *out);
    fastf_lists_t *L = out->L = (fastf_lists_t *)calloc(n_c, sizeof *L);
    uint64_t **keys = out->keys = (uint64_t **)calloc(n_c, sizeof *keys);
    if (!L || !keys) { rs_err("out of memory"); return RES_FAIL; }
    for (uint32_t i = 0; i < n_c; i++) {
        if (fastf_lists_load(barcodes, features, rates_cell[i], seed, &L[i])) return RES_FAIL;
        out->n = i + 1;
    }
    for (uint32_t i = 0; i < n_c; i++) {
        if (L[i].n_features != L[0].n_features) { rs_err("internal error: the feature list changed between loads"); return RES_FAIL; }
        if (!(keys[i] = (uint64_t *)malloc((L[i].n_cells ? L[i].n_cells : 1) * sizeof **keys))) { rs_err("out of memory"); return RES_FAIL; }
        for (size_t k = 0; k < L[i].n_cells; k++) keys[i][k] = fastf_keydict_add(L[0].cell_dict, L[i].barcode[k], strlen(L[i].barcode[k]));
        /* keys wider than 64 bits with the shortest UMI field: that cell rate would need the wide engine */
        if (bits_for(L[i].n_cells) + bits_for(L[i].n_features) + 27 > 64) return RES_NOT_COVERED;
    }
    return RES_OK;
}

/* ------------------------------------------------------------------ */
/* the records                                                         */
/* ------------------------------------------------------------------ */
void fastf_res_free(resident_t *r)
{
    fastf_devmem_free(r->cb); fastf_devmem_free(r->gx); fastf_devmem_free(r->umi); fastf_devmem_free(r->meta);
    r->cb = r->gx = NULL; r->umi = r->meta = NULL; r->cap = 0;
}
static int resident_reserve(resident_t *r, uint64_t need)
{
    if (need <= r->cap) return 0;
    uint64_t cap = r->cap ? r->cap : ((uint64_t)8 << 20);
    while (cap < need) cap *= 2;
    resident_t nr = *r;
    nr.cap = cap;
    nr.cb = (uint64_t *)fastf_devmem_alloc(r->device, cap * 8); nr.gx = (uint64_t *)fastf_devmem_alloc(r->device, cap * 8);
    nr.umi = (uint32_t *)fastf_devmem_alloc(r->device, cap * 4); nr.meta = (uint32_t *)fastf_devmem_alloc(r->device, cap * 4);
    if (!nr.cb || !nr.gx || !nr.umi || !nr.meta) {
        fastf_res_free(&nr);
        return rs_err("%s: the records do not fit the device: %llu bytes were needed for %llu records", r->verb, (unsigned long long)(cap * 24), (unsigned long long)need);
    }
    if (r->n && (fastf_devmem_copy(nr.cb, r->cb, r->n * 8) || fastf_devmem_copy(nr.gx, r->gx, r->n * 8) ||
                 fastf_devmem_copy(nr.umi, r->umi, r->n * 4) || fastf_devmem_copy(nr.meta, r->meta, r->n * 4))) { fastf_res_free(&nr); return 1; }
    fastf_res_free(r);
    *r = nr;
    return 0;
}

/* R->device is set by the caller through `device`; on failure the caller releases R */
int fastf_res_decode(const char *verb, const char *bam_file, const fastf_lists_t *L0, int device, resident_t *R)
{
    int rc = 1;
    fastf_bam_t *bam = NULL;
    void *stage = NULL;
    memset(R, 0, sizeof *R); R->device = device; R->verb = verb;
    {   const char *gp = getenv("FASTF_GPU_PARSE");
        bam = fastf_bam_open2(bam_file, 0, 1 | ((gp && gp[0] == '0') ? 0 : 4) | ((device + 1) << 8)); }
    if (!bam) { rs_err("Fail to open BAM file %s (%s)", bam_file, fastf_last_error()); goto done; }
    (void)fastf_bam_enable_device_parse(bam, L0->cell_dict, L0->feat_dict);
    const size_t cap = (size_t)4 << 20;
    if (!(stage = fastf_pinned_alloc(cap * 24))) { rs_err("%s: no pinned staging memory (%s)", verb, fastf_last_error()); goto done; }
    uint64_t *s_cb = (uint64_t *)stage, *s_gx = s_cb + cap; uint32_t *s_umi = (uint32_t *)(s_gx + cap), *s_meta = s_umi + cap;
    for (;;) {
        int on_dev = 0; fastf_batch_t dev; memset(&dev, 0, sizeof dev);
        const long n = fastf_bam_read_batch_dev(bam, L0->cell_dict, L0->feat_dict, s_cb, s_gx, s_umi, s_meta, cap, &on_dev, &dev);
        if (n < 0) { rs_err("%s: %s", bam_file, fastf_last_error()); goto done; }
        if (n == 0) break;
        if (R->n + (uint64_t)n >= ((uint64_t)1 << 32) - 1) { rs_err("%s: more than 2^32 - 2 records: %llu bytes of records are beyond what the device-level calls take", verb, (unsigned long long)((R->n + (uint64_t)n) * 24)); goto done; }
        if (resident_reserve(R, R->n + (uint64_t)n)) goto done;
        const uint64_t *f_cb = on_dev ? dev.cb_key : s_cb, *f_gx = on_dev ? dev.gx_key : s_gx;
        const uint32_t *f_umi = on_dev ? dev.umi : s_umi, *f_meta = on_dev ? dev.meta : s_meta;
        if (fastf_devmem_copy(R->cb + R->n, f_cb, (size_t)n * 8) || fastf_devmem_copy(R->gx + R->n, f_gx, (size_t)n * 8) ||
            fastf_devmem_copy(R->umi + R->n, f_umi, (size_t)n * 4) || fastf_devmem_copy(R->meta + R->n, f_meta, (size_t)n * 4)) goto done;
        R->n += (uint64_t)n;
    }
    {   uint64_t no_xf = 0, no_gx = 0;
        fastf_bam_stats(bam, NULL, &no_xf, &no_gx);
        if (no_xf || no_gx)
            fprintf(stderr, "Note: %llu records with a CB but no xf tag and %llu with a valid xf but no GX tag were skipped "
                            "(the reference dereferences NULL on them).\n", (unsigned long long)no_xf, (unsigned long long)no_gx); }
    fastf_bam_close(bam); bam = NULL;
    fastf_pinned_free(stage); stage = NULL;
    if (resident_reserve(R, 1)) goto done;               /* (an empty BAM: the arrays exist) */
    rc = 0;
done:
    if (bam) fastf_bam_close(bam);
    if (stage) fastf_pinned_free(stage);
    return rc;
}

/* ------------------------------------------------------------------ */
/* one cell rate                                                       */
/* ------------------------------------------------------------------ */
void fastf_res_rate_close(res_rate_t *S)
{
    if (S->e) fastf_engine_destroy(S->e);
    fastf_devmem_free(S->d_blk); fastf_devmem_free(S->d_keys); fastf_devmem_free(S->d_tmp); fastf_devmem_free(S->d_small);
    fastf_devmem_free(S->d_rows); fastf_devmem_free(S->d_upc); fastf_devmem_free(S->d_gpc);
    if (S->h_small) fastf_pinned_free(S->h_small);
    if (S->h_upc) fastf_pinned_free(S->h_upc);
    if (S->h_gpc) fastf_pinned_free(S->h_gpc);
    if (S->h_rows) fastf_pinned_free(S->h_rows);
    fastf_devmem_free(S->d_cpg); fastf_devmem_free(S->d_upg);
    if (S->h_cpg) fastf_pinned_free(S->h_cpg);
    if (S->h_upg) fastf_pinned_free(S->h_upg);
    fastf_devmem_free(S->d_cellsum);
    if (S->h_hist) fastf_pinned_free(S->h_hist);
    memset(S, 0, sizeof *S);
}

/* on anything but RES_OK the caller still calls fastf_res_rate_close */
int fastf_res_rate_open(res_rate_t *S, const char *verb, const resident_t *R, const fastf_lists_t *L, const uint64_t *cell_keys, float rate_cell,
                        uint32_t seed, int device, int genes, int cells, res_times_t *T)
{
    memset(S, 0, sizeof *S);
    S->genes = genes; S->n_features = (uint32_t)L->n_features; S->cells = cells;
    S->verb = verb; S->R = R; S->L = L; S->device = device; S->rate_cell = rate_cell; S->seed = seed;
    const uint64_t N = R->n;
    const uint32_t n_cells = S->n_cells = (uint32_t)L->n_cells;
    double tt = fastf_res_now();

    fastf_engine_config_t cfg; memset(&cfg, 0, sizeof cfg);
    cfg.cell_keys = cell_keys; cfg.n_cells = n_cells;
    cfg.feature_keys = L->feature_key; cfg.n_features = (uint32_t)L->n_features;
    cfg.draw_threshold = fastf_draw_threshold(1.0f);        /* (no part in the planes: every point brings its own threshold) */
    cfg.mt_seed = seed; cfg.mt_skip = L->mt_skip;
    cfg.n_shards = 1; cfg.device = device;
    cfg.batch_records = (uint64_t)1 << 16;                  /* (the push path is not used) */
    {   /* the UMI field as bam2db chooses it */
        const char *ul = getenv("FASTF_UMI_MAX_BASES");
        const uint32_t group_bits = bits_for(cfg.n_cells) + bits_for(cfg.n_features);
        cfg.umi_max_bases = ul ? (uint32_t)atoi(ul) : ((group_bits + 36 <= 64 || group_bits + 27 > 64) ? 16 : 12);
    }
    if (cfg.umi_max_bases > 16) return RES_NOT_COVERED;
    if (fastf_engine_create(&cfg, &S->e)) return RES_FAIL;
    if (fastf_engine_is_wide(S->e)) return RES_NOT_COVERED;
    T->engine += fastf_res_now() - tt; tt = fastf_res_now();

    {   uint32_t cb, fb, ub; if (fastf_engine_key_bits(S->e, &cb, &fb, &ub, &S->key_bits)) return RES_FAIL; }
    uint64_t blk_bytes = 0, seg_slots = 0;
    if (fastf_dev_block_bytes(S->e, N, &blk_bytes) || fastf_dev_probe_capacity(S->e, N, &seg_slots)) return RES_FAIL;
    S->blocked = blk_bytes != 0 && seg_slots != 0; S->segmented = seg_slots != 0;
    S->key_slots = (seg_slots > N ? seg_slots : N) + 64;
    S->kflags = FASTF_PROBE_REUSE_HITS | FASTF_PROBE_DRAW_BITS | (S->blocked ? FASTF_PROBE_BLOCKED : 0) | (S->segmented ? FASTF_PROBE_SEGMENTED : 0);
    const size_t need = (S->blocked ? blk_bytes : 0) + 2 * S->key_slots * 8 + N * 12 + ((size_t)n_cells + 1) * 12;
    if (!(S->d_small = fastf_devmem_alloc(device, SM_WORDS_ * 8)) || !(S->h_small = (uint64_t *)fastf_pinned_alloc(SM_WORDS_ * 8)) ||
        (S->blocked && !(S->d_blk = fastf_devmem_alloc(device, blk_bytes))) ||
        !(S->d_keys = fastf_devmem_alloc(device, S->key_slots * 8)) || !(S->d_tmp = fastf_devmem_alloc(device, S->key_slots * 8)) ||
        !(S->d_rows = fastf_devmem_alloc(device, (N ? N : 1) * 12)) ||
        !(S->d_upc = fastf_devmem_alloc(device, ((size_t)n_cells + 1) * 8)) || !(S->d_gpc = fastf_devmem_alloc(device, ((size_t)n_cells + 1) * 4)) ||
        !(S->h_upc = (uint64_t *)fastf_pinned_alloc(((size_t)n_cells + 1) * 8)) || !(S->h_gpc = (uint32_t *)fastf_pinned_alloc(((size_t)n_cells + 1) * 4))) {
        rs_err("%s: the working set of cell rate %.3f does not fit: %zu bytes were needed beside the records (%s)", verb, (double)rate_cell, need, fastf_last_error());
        return RES_FAIL;
    }
    if (genes) {                                            /* the per-gene arrays of a point and their pinned host copies, once */
        const size_t nf1 = (size_t)S->n_features + 1;
        if (!(S->d_cpg = fastf_devmem_alloc(device, nf1 * 4)) || !(S->d_upg = fastf_devmem_alloc(device, nf1 * 8)) ||
            !(S->h_cpg = (uint32_t *)fastf_pinned_alloc(nf1 * 4)) || !(S->h_upg = (uint64_t *)fastf_pinned_alloc(nf1 * 8))) {
            rs_err("%s: the per-gene arrays of cell rate %.3f do not fit: %zu bytes (%s)", verb, (double)rate_cell, nf1 * 12, fastf_last_error());
            return RES_FAIL;
        }
    }
    if (cells) {                                            /* the histogram and the three per-cell arrays of a point and their pinned host copy, once */
        const size_t bytes = RES_CELLS_HIST_BYTES + (size_t)n_cells * 12;
        if (!(S->d_cellsum = fastf_devmem_alloc(device, bytes)) || !(S->h_hist = (uint64_t *)fastf_pinned_alloc(bytes))) {
            rs_err("%s: the per-cell arrays of cell rate %.3f do not fit: %zu bytes (%s)", verb, (double)rate_cell, bytes, fastf_last_error());
            return RES_FAIL;
        }
        S->h_rpc = (uint32_t *)((char *)S->h_hist + RES_CELLS_HIST_BYTES); S->h_npc = S->h_rpc + n_cells; S->h_spc = S->h_npc + n_cells;
    }
    uint64_t *const sm = (uint64_t *)S->d_small;
    if (fastf_devmem_zero(S->d_small, SM_WORDS_ * 8) || fastf_dev_reserve(S->e, S->blocked ? 0 : N, N)) return RES_FAIL;

    /* the records into the engine's layout, K1a once: the cell scratch and the hit count serve every point */
    if (S->blocked) {
        if (fastf_dev_block_records(S->e, R->gx, R->umi, R->meta, N, S->d_blk, NULL) ||
            fastf_dev_count_hits_blocked(S->e, R->cb, N, S->d_blk, sm + SM_HITS, NULL)) return RES_FAIL;
    } else if (fastf_dev_count_hits(S->e, R->cb, N, sm + SM_HITS, NULL)) return RES_FAIL;
    if (fastf_devmem_sync() || fastf_devmem_copy(S->h_small, S->d_small, SM_WORDS_ * 8)) return RES_FAIL;
    S->H = S->h_small[SM_HITS];
    T->block_k1a += fastf_res_now() - tt;
    return RES_OK;
}

/* ------------------------------------------------------------------ */
/* one point                                                           */
/* ------------------------------------------------------------------ */
int fastf_res_point_run(res_rate_t *S, const uint32_t *d_plane, const char *point_name, uint64_t counters[3], uint64_t *nnz_out, res_times_t *T)
{
    const resident_t *R = S->R;
    const uint64_t N = R->n;
    fastf_engine_t *e = S->e;
    uint64_t *const sm = (uint64_t *)S->d_small;
    uint32_t *const d_f = (uint32_t *)S->d_rows, *const d_c = d_f + N, *const d_k = d_c + N;
    double tt = fastf_res_now();
    if (fastf_devmem_zero(S->d_small, SM_HITS * 8)) return RES_FAIL;
    if (fastf_dev_probe_pack(e, R->cb, S->blocked ? (const uint64_t *)S->d_blk : R->gx, R->umi, R->meta, N, d_plane, S->H, sm + SM_BASE,
                             (uint64_t *)S->d_keys, S->key_slots, sm + SM_KEYS, sm + SM_CNT, S->kflags, NULL)) return RES_FAIL;
    int in_tmp = 0;
    if (fastf_dev_sort(e, (uint64_t *)S->d_keys, (uint64_t *)S->d_tmp, sm + SM_KEYS, N, S->key_bits, FASTF_SORT_SKIP_LOW | (S->segmented ? FASTF_SORT_SEGMENTED : 0), &in_tmp, NULL)) return RES_FAIL;
    uint64_t *src = in_tmp ? (uint64_t *)S->d_tmp : (uint64_t *)S->d_keys, *other = in_tmp ? (uint64_t *)S->d_keys : (uint64_t *)S->d_tmp;
    if (fastf_dev_reduce(e, src, sm + SM_KEYS, N, NULL, NULL, NULL, sm + SM_NNZ, FASTF_SORT_SKIP_LOW | FASTF_REDUCE_SEGMENTED, NULL)) return RES_FAIL;
    uint64_t bits = 0;
    if (fastf_dev_error_bits(e, &bits)) return RES_FAIL;
    S->sorted_full = 0;
    if (bits & FASTF_ERR_RUN_TOO_LONG) {
        /* deep (cell, feature) groups: sort fully and reduce again, as fastf_engine_finish does (every key is still there, permuted) */
        int in_other = 0;
        if (fastf_dev_clear_error_bits(e, FASTF_ERR_RUN_TOO_LONG, NULL) ||
            fastf_dev_sort(e, src, other, sm + SM_KEYS, N, S->key_bits, 0, &in_other, NULL)) return RES_FAIL;
        if (in_other) { uint64_t *t = src; src = other; other = t; }
        if (fastf_dev_reduce(e, src, sm + SM_KEYS, N, NULL, NULL, NULL, sm + SM_NNZ, FASTF_REDUCE_SEGMENTED, NULL) || fastf_dev_error_bits(e, &bits)) return RES_FAIL;
        S->sorted_full = 1;
    }
    S->sorted = src; S->sorted_other = other;
    if (fastf_devmem_copy(S->h_small, S->d_small, SM_HITS * 8)) return RES_FAIL;
    bits |= S->h_small[SM_CNT + 3];
    if (bits & 4) return RES_NOT_COVERED;                   /* UMIs longer than the key holds: bam2db() runs such a file again with wider keys */
    if (bits) { rs_err("%s: device error bits 0x%llx at point %s", S->verb, (unsigned long long)bits, point_name); return RES_FAIL; }
    counters[0] = N; counters[1] = S->h_small[SM_CNT + 1]; counters[2] = S->h_small[SM_CNT + 2];
    const uint64_t nnz = *nnz_out = S->h_small[SM_NNZ];
    if (nnz > N) { rs_err("internal error: %llu matrix rows out of %llu records", (unsigned long long)nnz, (unsigned long long)N); return RES_FAIL; }
    /* the rows, concatenated on the device, and their per-cell summary */
    if (fastf_dev_rows_gather(e, sm + SM_KEYS, d_f, d_c, d_k, NULL) ||
        fastf_dev_cell_summary(e, nnz ? d_c : NULL, nnz ? d_k : NULL, sm + SM_NNZ, S->n_cells, (uint64_t *)S->d_upc, (uint32_t *)S->d_gpc, NULL) ||
        (S->genes && fastf_dev_gene_summary(e, nnz ? d_f : NULL, nnz ? d_k : NULL, sm + SM_NNZ, S->n_features, (uint32_t *)S->d_cpg, (uint64_t *)S->d_upg, NULL)) ||
        fastf_devmem_sync()) return RES_FAIL;
    T->device += fastf_res_now() - tt; tt = fastf_res_now();
    if (fastf_devmem_copy(S->h_upc, S->d_upc, ((size_t)S->n_cells + 1) * 8) || fastf_devmem_copy(S->h_gpc, S->d_gpc, (size_t)S->n_cells * 4)) return RES_FAIL;
    T->summary += fastf_res_now() - tt;
    if (S->genes) {
        tt = fastf_res_now();
        if (S->n_features && (fastf_devmem_copy(S->h_cpg, S->d_cpg, (size_t)S->n_features * 4) || fastf_devmem_copy(S->h_upg, S->d_upg, (size_t)S->n_features * 8))) return RES_FAIL;
        T->genes += fastf_res_now() - tt;
    }
    return RES_OK;
}

int fastf_res_point_write(res_rate_t *S, const char *dir, const char *bam_label, float rate_depth, const uint64_t counters[3], uint64_t nnz, res_times_t *T)
{
    uint64_t *const sm = (uint64_t *)S->d_small;
    double tt = fastf_res_now();
    if (nnz > S->h_rows_cap) {
        if (S->h_rows) fastf_pinned_free(S->h_rows);
        S->h_rows_cap = nnz + nnz / 8 + 1024;
        if (!(S->h_rows = (uint32_t *)fastf_pinned_alloc(S->h_rows_cap * 12))) { S->h_rows_cap = 0; return rs_err("%s: no pinned memory for %llu matrix rows", S->verb, (unsigned long long)nnz); }
    }
    uint32_t *const h_rows = S->h_rows; const uint64_t cap = S->h_rows_cap;
    fastf_coo_t coo = { h_rows, h_rows + cap, h_rows + 2 * cap, (size_t)nnz };
    /* (the gather kernel writes pinned host memory directly: it is the device-to-host copy of the rows) */
    if (nnz && (fastf_dev_rows_gather(S->e, sm + SM_KEYS, h_rows, h_rows + cap, h_rows + 2 * cap, NULL) || fastf_devmem_sync())) return 1;
    T->d2h += fastf_res_now() - tt; tt = fastf_res_now();
    if (fastf_res_make_dir(dir) || fastf_write_outputs(dir, bam_label, S->rate_cell, rate_depth, counters, S->L, &coo, NULL)) return 1;
    T->write += fastf_res_now() - tt;
    return 0;
}

/* --cells: behind the point.  The full sort and K3u use the engine's workspace, and K3u writes the engine's row regions — the count
 * array and the span tables of the matrix rows — so this runs once fastf_res_point_write has gathered them (resident.h) */
int fastf_res_point_cells(res_rate_t *S, const char *point_name, res_times_t *T)
{
    if (!S->cells) return 0;
    const uint64_t N = S->R->n;
    fastf_engine_t *e = S->e;
    uint64_t *const sm = (uint64_t *)S->d_small;
    double tt = fastf_res_now();
    if (!S->sorted) return rs_err("internal error: no sorted keys at point %s", point_name);
    uint64_t *src = S->sorted;
    if (!S->sorted_full) {                                  /* (every key is still there, sorted but for its low bits) */
        int in_other = 0;
        if (fastf_dev_sort(e, src, S->sorted_other, sm + SM_KEYS, N, S->key_bits, 0, &in_other, NULL)) return 1;
        if (in_other) src = S->sorted_other;
    }
    S->sorted = NULL;                                       /* (one use: the next point brings its own) */
    uint64_t *const d_uk = (uint64_t *)S->d_rows; uint32_t *const d_nc = (uint32_t *)(d_uk + N);
    uint64_t *const d_hist = (uint64_t *)S->d_cellsum;
    uint32_t *const d_rpc = (uint32_t *)((char *)S->d_cellsum + RES_CELLS_HIST_BYTES), *const d_npc = d_rpc + S->n_cells, *const d_spc = d_npc + S->n_cells;
    uint64_t bits = 0;
    if (fastf_dev_umi_rows(e, src, sm + SM_KEYS, N, d_uk, d_nc, sm + SM_UROWS, NULL) ||
        fastf_dev_copy_summary(e, d_uk, d_nc, sm + SM_UROWS, S->n_cells, d_rpc, d_npc, d_spc, d_hist, NULL) ||
        fastf_dev_error_bits(e, &bits)) return 1;
    if (bits) return rs_err("%s: device error bits 0x%llx in the per-cell stage of point %s", S->verb, (unsigned long long)bits, point_name);
    if (fastf_devmem_copy(S->h_hist, S->d_cellsum, RES_CELLS_HIST_BYTES + (size_t)S->n_cells * 12)) return 1;
    T->cells_dev += fastf_res_now() - tt;
    return 0;
}

/* ------------------------------------------------------------------ */
/* the summary table, the command line                                 */
/* ------------------------------------------------------------------ */
int fastf_res_tsv_open(res_tsv_t *t, const char *out_dir, const char *name, const char *header)
{
    snprintf(t->final, sizeof t->final, "%s/%s", out_dir, name);
    snprintf(t->tmp, sizeof t->tmp, "%s/%s.partial", out_dir, name);
    if (!(t->f = fopen(t->tmp, "w"))) return rs_err("cannot open %s: %s", t->tmp, strerror(errno));
    fputs(header, t->f);
    return 0;
}
int fastf_res_tsv_close(res_tsv_t *t, int ok)
{
    if (!t->f) return 0;
    const int bad = ferror(t->f) | (fclose(t->f) != 0);
    t->f = NULL;
    if (ok && !bad && rename(t->tmp, t->final) == 0) return 0;
    unlink(t->tmp);
    return ok ? rs_err("cannot write %s", t->final) : 0;
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

int fastf_res_genes_open(res_genes_t *G, int on, const char *verb, const char *out_dir, const char *header, uint32_t max_points)
{
    memset(G, 0, sizeof *G);
    if (!on) return 0;
    G->verb = verb; G->max_points = max_points;
    snprintf(G->out_dir, sizeof G->out_dir, "%s", out_dir);
    char name[64];
    snprintf(name, sizeof name, "%s_genes.tsv", verb);
    if (!(G->names = calloc(max_points ? max_points : 1, sizeof *G->names))) return rs_err("out of memory");
    if (fastf_res_tsv_open(&G->tsv, out_dir, name, header)) { genes_release(G); return 1; }
    G->on = 1;
    return 0;
}

/* text of n lines `id \t a[i] [\t b[i]]` */
typedef struct { char *p; size_t len, cap; } gtext;
static int gt_room(gtext *t, size_t more)
{
    if (t->len + more <= t->cap) return 0;
    size_t cap = t->cap ? t->cap : ((size_t)1 << 16);
    while (cap < t->len + more) cap *= 2;
    char *np = (char *)realloc(t->p, cap);
    if (!np) return rs_err("out of memory");
    t->p = np; t->cap = cap;
    return 0;
}
static int gt_str(gtext *t, const char *s) { const size_t n = strlen(s); if (gt_room(t, n)) return 1; memcpy(t->p + t->len, s, n); t->len += n; return 0; }
static int gt_u64(gtext *t, char lead, uint64_t v)
{
    if (gt_room(t, 24)) return 1;
    t->len += (size_t)snprintf(t->p + t->len, 24, "%c%llu", lead, (unsigned long long)v);
    return 0;
}
/* a finished text through <path>.partial */
static int gz_text_renamed(const char *path, const gtext *t)
{
    char tmp[4200];
    snprintf(tmp, sizeof tmp, "%s.partial", path);
    if (fastf_write_gz_text(tmp, t->p ? t->p : "", t->len) || rename(tmp, path) != 0) { unlink(tmp); return rs_err("cannot write %s", path); }
    return 0;
}

int fastf_res_genes_point(res_genes_t *G, const fastf_lists_t *L, const char *point_name, const char *dir, const char *row,
                          const uint32_t *cells, const uint64_t *umis)
{
    if (!G->on) return 0;
    if (!G->feat_id) {                                      /* the first point: the names and the room of the grid file */
        const uint32_t nf = (uint32_t)L->n_features;
        if (!(G->feat_id = (char **)calloc(nf ? nf : 1, sizeof *G->feat_id)) ||
            !(G->cells = (uint32_t *)malloc(((size_t)G->max_points * nf + 1) * sizeof *G->cells))) return rs_err("out of memory");
        for (uint32_t i = 0; i < nf; i++) { if (!(G->feat_id[i] = strdup(L->feat_id[i]))) return rs_err("out of memory"); G->n_features = i + 1; }
    }
    if ((uint32_t)L->n_features != G->n_features) return rs_err("internal error: the feature list changed between points");
    if (G->n_points >= G->max_points) return rs_err("internal error: more points than the grid has");
    const uint32_t nf = G->n_features;
    snprintf(G->names[G->n_points], sizeof G->names[0], "%s", point_name);
    if (nf) memcpy(G->cells + (size_t)G->n_points * nf, cells, (size_t)nf * sizeof *cells);
    G->n_points++;
    if (dir) {
        char path[4200];
        gtext t = { NULL, 0, 0 };
        int bad = 0;
        for (uint32_t i = 0; i < nf && !bad; i++)
            bad = gt_str(&t, G->feat_id[i]) || gt_u64(&t, '\t', cells[i]) || gt_u64(&t, '\t', umis[i]) || gt_str(&t, "\n");
        snprintf(path, sizeof path, "%s/genes.tsv.gz", dir);
        if (!bad) bad = fastf_res_make_dir(dir) || gz_text_renamed(path, &t);
        free(t.p);
        if (bad) return 1;
    }
    fputs(row, G->tsv.f);
    return 0;
}

/* ok: the grid file, then the table; otherwise nothing of either is left */
int fastf_res_genes_close(res_genes_t *G, int ok)
{
    if (!G->on) return 0;
    int rc = 0;
    if (ok) {
        char path[4200];
        gtext t = { NULL, 0, 0 };
        int bad = gt_str(&t, "feature");
        for (uint32_t p = 0; p < G->n_points && !bad; p++) bad = gt_str(&t, "\t") || gt_str(&t, G->names[p]);
        if (!bad) bad = gt_str(&t, "\n");
        for (uint32_t i = 0; i < G->n_features && !bad; i++) {
            bad = gt_str(&t, G->feat_id[i]);
            for (uint32_t p = 0; p < G->n_points && !bad; p++) bad = gt_u64(&t, '\t', G->cells[(size_t)p * G->n_features + i]);
            if (!bad) bad = gt_str(&t, "\n");
        }
        snprintf(path, sizeof path, "%s/%s_gene_cells.tsv.gz", G->out_dir, G->verb);
        if (!bad) bad = gz_text_renamed(path, &t);
        free(t.p);
        rc = bad;
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
int fastf_res_cells_open(res_cells_t *C, int on, const char *verb, const char *out_dir, const char *header)
{
    memset(C, 0, sizeof *C);
    if (!on) return 0;
    char name[64];
    snprintf(name, sizeof name, "%s_cells.tsv", verb);
    C->verb = verb;
    if (fastf_res_tsv_open(&C->tsv, out_dir, name, header)) return 1;
    C->on = 1;
    return 0;
}

int fastf_res_cells_point(res_cells_t *C, const res_rate_t *S, const char *dir, const char *row)
{
    if (!C->on) return 0;
    if (dir) {
        char path[4200];
        gtext t = { NULL, 0, 0 };
        int bad = gt_str(&t, "barcode\treads\tnull_umi_reads\tumis\tgenes\tsingleton_umis\tsaturation\n");
        for (uint32_t k = 0; k < S->n_cells && !bad; k++) {
            const uint64_t reads = S->h_rpc[k], umis = S->h_upc[k];
            char sat[32];
            snprintf(sat, sizeof sat, "\t%.6f\n", reads ? 1.0 - (double)umis / (double)reads : 0.0);
            bad = gt_str(&t, S->L->barcode[k]) || gt_u64(&t, '\t', reads) || gt_u64(&t, '\t', S->h_npc[k]) || gt_u64(&t, '\t', umis) ||
                  gt_u64(&t, '\t', S->h_gpc[k]) || gt_u64(&t, '\t', S->h_spc[k]) || gt_str(&t, sat);
        }
        snprintf(path, sizeof path, "%s/cells.tsv.gz", dir);
        if (!bad) bad = fastf_res_make_dir(dir) || gz_text_renamed(path, &t);
        free(t.p);
        if (bad) return 1;
    }
    fputs(row, C->tsv.f);
    return 0;
}

int fastf_res_cells_close(res_cells_t *C, int ok)
{
    if (!C->on) return 0;
    C->on = 0;
    return fastf_res_tsv_close(&C->tsv, ok);
}

struct ropt { char s; const char *l; int has_arg; };
int fastf_res_parse_args(int argc, const char **argv, char list_short, const char *list_long, void (*usage)(FILE *), const char *u_message,
                         res_args_t *out)
{
    const struct ropt opts[] = {
        {'h', "help", 0}, {'b', "bam", 1}, {'f', "feature", 1}, {'a', "barcode", 1}, {'d', "dbname", 1}, {'c', "cell", 1}, {list_short, list_long, 1},
        {'o', "out", 1}, {'s', "seed", 1}, {'u', "umicopies", 0}, {'S', "summary-only", 0}, {'G', "genes", 0}, {'C', "cells", 0}, {0, NULL, 0}};
    out->bam = out->feat = out->bar = out->list = NULL; out->out = "."; out->cells = "1"; out->seed = 926; out->summary_only = 0; out->genes = 0; out->per_cell = 0;
    for (int i = 1; i < argc; i++) {
        const char *a = argv[i];
        const struct ropt *o = NULL;
        const char *val = NULL;
        if (a[0] != '-' || !a[1]) break;
        if (a[1] == '-') {
            if (!a[2]) break;
            const char *eq = strchr(a + 2, '=');
            const size_t nl = eq ? (size_t)(eq - a - 2) : strlen(a + 2);
            for (const struct ropt *k = opts; k->l; k++)
                if (strlen(k->l) == nl && strncmp(k->l, a + 2, nl) == 0) { o = k; break; }
            if (o && eq) val = eq + 1;
        } else {
            for (const struct ropt *k = opts; k->l; k++) if (k->s == a[1] && k->s != 'S' && k->s != 'G' && k->s != 'C') { o = k; break; }
            if (o && o->has_arg && a[2]) val = a + 2;
        }
        if (!o) { fprintf(stderr, "error: unknown option `%s`\n", a); usage(stderr); return 1; }
        char oname[32];
        if (a[1] == '-') snprintf(oname, sizeof oname, "--%s", o->l); else snprintf(oname, sizeof oname, "-%c", o->s);
        if (o->has_arg && !val) {
            if (i + 1 >= argc) { fprintf(stderr, "error: option `%s` requires a value\n", oname); return 1; }
            val = argv[++i];
        }
        char *end = NULL;
        if (o->s == list_short) { out->list = val; continue; }
        switch (o->s) {
        case 'h': usage(stdout); return 2;
        case 'b': out->bam = val; break;
        case 'f': out->feat = val; break;
        case 'a': out->bar = val; break;
        case 'd': break;
        case 'o': out->out = val; break;
        case 'c': out->cells = val; break;
        case 's': errno = 0; out->seed = (unsigned int)strtol(val, &end, 0);
                  if (errno == ERANGE) { fprintf(stderr, "error: option `%s` numerical result out of range\n", oname); return 1; }
                  if (*end) { fprintf(stderr, "error: option `%s` expects an integer value\n", oname); return 1; }
                  break;
        case 'u': fprintf(stderr, "\x1b[31mError:\x1b[0m %s\n", u_message); return 1;
        case 'S': out->summary_only = 1; break;
        case 'G': out->genes = 1; break;
        case 'C': out->per_cell = 1; break;
        }
    }
    return 0;
}
/* (after the verb has parsed its lists: the order of the messages of cmd_sweep) */
int fastf_res_check_inputs(const res_args_t *a)
{
    if (!a->bam || access(a->bam, F_OK) == -1) { fprintf(stderr, "\x1b[31mError:\x1b[0m bam file: %s does not exist.\n", a->bam ? a->bam : "(null)"); return 1; }
    if (!a->feat || access(a->feat, F_OK) == -1) { fprintf(stderr, "\x1b[31mError:\x1b[0m feature file: %s does not exist.\n", a->feat ? a->feat : "(null)"); return 1; }
    if (!a->bar || access(a->bar, F_OK) == -1) { fprintf(stderr, "\x1b[31mError:\x1b[0m barcode file: %s does not exist.\n", a->bar ? a->bar : "(null)"); return 1; }
    return 0;
}
