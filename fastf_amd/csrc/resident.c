/*
 * resident.c — the resident pipeline of `fastF sweep`, `fastF cap` and `fastF level` (resident.h): list loading with one dictionary,
 * the decode of the BAM into device-resident records, per cell rate the engine + the records in its layout + K1a, per point K1b /
 * sort / reduce / gather / summary and the matrix writers, the replicate accumulators and the command line of the three verbs.  The
 * tables and point files of a run: res_tables.c; the driver that runs a verb's grid: grid_run.c.
 */
#define _GNU_SOURCE
#include "resident.h"
#include "cli_opts.h"

#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

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

int fastf_res_lists_load(const char *barcodes, const char *features, const float *rates_cell, const uint32_t *seeds, uint32_t n_c, res_lists_t *out)
{
    memset(out, 0, sizeof *out);
    fastf_lists_t *L = out->L = (fastf_lists_t *)calloc(n_c, sizeof *L);
    uint64_t **keys = out->keys = (uint64_t **)calloc(n_c, sizeof *keys);
    if (!L || !keys) { fastf_res_err("out of memory"); return RES_FAIL; }
    for (uint32_t i = 0; i < n_c; i++) {
        if (fastf_lists_load(barcodes, features, rates_cell[i], seeds[i], &L[i])) return RES_FAIL;
        out->n = i + 1;
    }
    for (uint32_t i = 0; i < n_c; i++) {
        if (L[i].n_features != L[0].n_features) { fastf_res_err("internal error: the feature list changed between loads"); return RES_FAIL; }
        if (!(keys[i] = (uint64_t *)malloc((L[i].n_cells ? L[i].n_cells : 1) * sizeof **keys))) { fastf_res_err("out of memory"); return RES_FAIL; }
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
        return fastf_res_err("%s: the records do not fit the device: %llu bytes were needed for %llu records", r->verb, (unsigned long long)(cap * 24), (unsigned long long)need);
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
    if (!bam) { fastf_res_err("Fail to open BAM file %s (%s)", bam_file, fastf_last_error()); goto done; }
    (void)fastf_bam_enable_device_parse(bam, L0->cell_dict, L0->feat_dict);
    const size_t cap = (size_t)4 << 20;
    if (!(stage = fastf_pinned_alloc(cap * 24))) { fastf_res_err("%s: no pinned staging memory (%s)", verb, fastf_last_error()); goto done; }
    uint64_t *s_cb = (uint64_t *)stage, *s_gx = s_cb + cap; uint32_t *s_umi = (uint32_t *)(s_gx + cap), *s_meta = s_umi + cap;
    for (;;) {
        int on_dev = 0; fastf_batch_t dev; memset(&dev, 0, sizeof dev);
        const long n = fastf_bam_read_batch_dev(bam, L0->cell_dict, L0->feat_dict, s_cb, s_gx, s_umi, s_meta, cap, &on_dev, &dev);
        if (n < 0) { fastf_res_err("%s: %s", bam_file, fastf_last_error()); goto done; }
        if (n == 0) break;
        if (R->n + (uint64_t)n >= ((uint64_t)1 << 32) - 1) { fastf_res_err("%s: more than 2^32 - 2 records: %llu bytes of records are beyond what the device-level calls take", verb, (unsigned long long)((R->n + (uint64_t)n) * 24)); goto done; }
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
static void res_buf_free(res_buf_t *b)
{
    if (b->kind == RES_DEV) fastf_devmem_free(b->p);
    else if (b->kind == RES_PIN) { if (b->p) fastf_pinned_free(b->p); }
    else free(b->p);
    memset(b, 0, sizeof *b);
}
void fastf_res_rate_close(res_rate_t *S)
{
    const res_cfg_t cfg = S->cfg;                           /* (the caller's: it outlives the pairs) */
    if (S->e) fastf_engine_destroy(S->e);
    for (res_buf_t *b = (res_buf_t *)&S->buf, *const end = b + sizeof S->buf / sizeof *b; b < end; b++) res_buf_free(b);
    memset(S, 0, sizeof *S);
    S->cfg = cfg;
}

/* room of at least `need` bytes in a buffer that outlives the pair: what is there is kept when it is large enough */
static int res_room(res_buf_t *b, int kind, size_t need, int device)
{
    if (b->p && b->have >= need) return 0;
    res_buf_free(b);
    b->p = kind == RES_DEV ? fastf_devmem_alloc(device, need) : kind == RES_PIN ? fastf_pinned_alloc(need) : malloc(need ? need : 1);
    if (!b->p) return 1;
    b->kind = kind; b->have = need;
    return 0;
}
/* the same for a carved block of `bytes` for n entries per array: a block that stays is carved by the n it was allocated for */
static int res_block_room(res_buf_t *b, int kind, size_t bytes, size_t n, int device)
{
    if (res_room(b, kind, bytes, device)) return 1;
    if (!b->n) b->n = n;                                    /* (allocated just now: res_buf_free cleared it) */
    return 0;
}
static int no_room(const res_rate_t *S, const char *what, size_t bytes)
{
    fastf_res_err("%s: %s of cell rate %.3f do not fit: %zu bytes (%s)", S->verb, what, (double)S->rate_cell, bytes, fastf_last_error());
    return RES_FAIL;
}

/* S: zeroed before the first open of a run but for S->cfg, or as the open of the pair before left it (resident.h).  On anything but
 * RES_OK the caller still calls fastf_res_rate_close */
int fastf_res_rate_open(res_rate_t *S, const char *verb, const resident_t *R, const fastf_lists_t *L, const uint64_t *cell_keys, float rate_cell,
                        uint32_t seed, int device, int genes, int cells, res_times_t *T)
{
    if (S->e) { fastf_engine_destroy(S->e); S->e = NULL; }     /* (the pair before: its buffers stay) */
    if (S->cfg.no_reuse) fastf_res_rate_close(S);
    S->sorted = S->sorted_other = NULL; S->sorted_full = 0; S->H = 0;
    T->opens++;
    S->genes = genes; S->n_features = (uint32_t)L->n_features; S->cells = cells;
    S->verb = verb; S->R = R; S->L = L; S->device = device; S->rate_cell = rate_cell; S->seed = seed;
    const uint64_t N = R->n;
    const uint32_t n_cells = S->n_cells = (uint32_t)L->n_cells;
    double tt = fastf_res_now();

    fastf_engine_config_t ec; memset(&ec, 0, sizeof ec);
    ec.cell_keys = cell_keys; ec.n_cells = n_cells;
    ec.feature_keys = L->feature_key; ec.n_features = (uint32_t)L->n_features;
    ec.draw_threshold = fastf_draw_threshold(1.0f);        /* (no part in the planes: every point brings its own threshold) */
    ec.mt_seed = seed; ec.mt_skip = L->mt_skip;
    ec.n_shards = 1; ec.device = device;
    ec.batch_records = (uint64_t)1 << 16;                  /* (the push path is not used) */
    {   /* the UMI field as bam2db chooses it */
        const char *ul = getenv("FASTF_UMI_MAX_BASES");
        const uint32_t group_bits = bits_for(ec.n_cells) + bits_for(ec.n_features);
        ec.umi_max_bases = ul ? (uint32_t)atoi(ul) : ((group_bits + 36 <= 64 || group_bits + 27 > 64) ? 16 : 12);
    }
    if (ec.umi_max_bases > 16) return RES_NOT_COVERED;
    if (fastf_engine_create(&ec, &S->e)) return RES_FAIL;
    if (fastf_engine_is_wide(S->e)) return RES_NOT_COVERED;
    T->engine += fastf_res_now() - tt; tt = fastf_res_now();

    {   uint32_t cb, fb, ub; if (fastf_engine_key_bits(S->e, &cb, &fb, &ub, &S->key_bits)) return RES_FAIL; }
    uint64_t blk_bytes = 0, seg_slots = 0;
    if (fastf_dev_block_bytes(S->e, N, &blk_bytes) || fastf_dev_probe_capacity(S->e, N, &seg_slots)) return RES_FAIL;
    S->blocked = blk_bytes != 0 && seg_slots != 0; S->segmented = seg_slots != 0;
    S->key_slots = (seg_slots > N ? seg_slots : N) + 64;
    S->kflags = FASTF_PROBE_REUSE_HITS | FASTF_PROBE_DRAW_BITS | (S->blocked ? FASTF_PROBE_BLOCKED : 0) | (S->segmented ? FASTF_PROBE_SEGMENTED : 0);
    const size_t need = (S->blocked ? blk_bytes : 0) + 2 * S->key_slots * 8 + N * 12 + ((size_t)n_cells + 1) * 12;
    uint64_t layout = 0;
    if (fastf_dev_block_layout(S->e, N, &layout)) return RES_FAIL;
    /* room for the run's widest pair: its cells in the per-cell arrays, and a 32-bit cell scratch in the blocked runs where a later
     * pair samples more than 65535 cells while this one has the 16-bit scratch (2 bytes more for each of a unit's 256 records) */
    const size_t room_cells = (S->cfg.max_cells > n_cells ? S->cfg.max_cells : n_cells) + (size_t)1;
    const size_t blk_room = blk_bytes + ((S->cfg.max_cells > 65535u && n_cells <= 65535u) ? ((N + 255) / 256) * 512 : 0);
    const int blk_fits = S->buf.blk.p && S->buf.blk.have >= blk_bytes;
    if (S->blocked && !blk_fits) S->blk_layout = 0;         /* (a new buffer holds no copy) */
    if (res_room(&S->buf.small, RES_DEV, SM_WORDS_ * 8, device) || res_room(&S->buf.h_small, RES_PIN, SM_WORDS_ * 8, device) ||
        (S->blocked && res_room(&S->buf.blk, RES_DEV, blk_fits ? blk_bytes : blk_room, device)) ||
        res_room(&S->buf.keys, RES_DEV, S->key_slots * 8, device) || res_room(&S->buf.tmp, RES_DEV, S->key_slots * 8, device) ||
        res_room(&S->buf.rows, RES_DEV, (N ? N : 1) * 12, device) ||
        res_room(&S->buf.upc, RES_DEV, room_cells * 8, device) || res_room(&S->buf.gpc, RES_DEV, room_cells * 4, device) ||
        res_room(&S->buf.h_upc, RES_PIN, room_cells * 8, device) || res_room(&S->buf.h_gpc, RES_PIN, room_cells * 4, device)) {
        fastf_res_err("%s: the working set of cell rate %.3f does not fit: %zu bytes were needed beside the records (%s)", verb, (double)rate_cell, need, fastf_last_error());
        return RES_FAIL;
    }
    if (genes) {                                            /* the per-gene arrays of a point and their pinned host copies, once */
        const size_t nf1 = (size_t)S->n_features + 1;
        if (res_room(&S->buf.cpg, RES_DEV, nf1 * 4, device) || res_room(&S->buf.upg, RES_DEV, nf1 * 8, device) ||
            res_room(&S->buf.h_cpg, RES_PIN, nf1 * 4, device) || res_room(&S->buf.h_upg, RES_PIN, nf1 * 8, device)) return no_room(S, "the per-gene arrays", nf1 * 12);
    }
    if (cells) {                                            /* the histogram and the three per-cell arrays of a point and their pinned host copy, once */
        const size_t room = res_cellsum_layout(NULL, room_cells - 1).bytes;
        if (res_room(&S->buf.cellsum, RES_DEV, room, device) || res_room(&S->buf.h_cellsum, RES_PIN, room, device))
            return no_room(S, "the per-cell arrays", res_cellsum_layout(NULL, n_cells).bytes);
        S->h_cs = res_cellsum_layout(S->buf.h_cellsum.p, n_cells);
    }
    if (res_cfg_per_gene(&S->cfg) && !S->cfg.fidelity) {    /* the full rows of the pair, for --gene-fidelity, --neighbors or --coexpression alone */
        if (res_room(&S->buf.full, RES_DEV, (N ? N : 1) * 12, device)) return no_room(S, "the full-depth rows", (size_t)(N * 12));
        S->full_nnz = 0;
    }
    if (res_cfg_per_gene(&S->cfg)) {                        /* the partner column, the per-gene sums of the pair and of a point and their pinned copies, once (--neighbors or --coexpression alone: the pair's sums, which rank A) */
        const size_t nf1 = (size_t)S->n_features + 1, bytes = res_gfid_layout(NULL, nf1).bytes;
        if ((S->cfg.gene_fid && res_room(&S->buf.gx, RES_DEV, (N ? N : 1) * 4, device)) || res_block_room(&S->buf.gfid, RES_DEV, bytes, nf1, device) ||
            res_block_room(&S->buf.h_gfid, RES_PIN, bytes, nf1, device)) return no_room(S, "the partner column and the per-gene sums", (size_t)(N * 4 + bytes));
        S->d_gfid = res_gfid_layout(S->buf.gfid.p, S->buf.gfid.n); S->h_gfid = res_gfid_layout(S->buf.h_gfid.p, S->buf.h_gfid.n);
        if (genes) { S->h_gfid.sy = S->buf.h_upg.u64; S->h_gfid.c = S->buf.h_cpg.u32; }      /* (the point's own two are --genes') */
    }
    if (S->cfg.neighbors) {                                 /* the device and the pinned block of the neighbour sets.  The planes wait for P (fastf_res_full_keep) */
        const size_t nc = room_cells, map_bytes = S->nbr_map_bytes = res_nbr_map_bytes(S->n_features);
        const size_t dev_bytes = res_nbr_layout(NULL, map_bytes, FASTF_NEIGHBORS_K, nc).bytes;
        if (res_room(&S->buf.nbr, RES_DEV, dev_bytes, device) || res_room(&S->buf.h_nbr, RES_PIN, res_nbr_pin_layout(NULL, map_bytes, nc, FASTF_HVG_TOP).bytes, device))
            return no_room(S, "the neighbour sets", dev_bytes);
        S->d_nbr = res_nbr_layout(S->buf.nbr.p, map_bytes, FASTF_NEIGHBORS_K, nc); S->h_nbr = res_nbr_pin_layout(S->buf.h_nbr.p, map_bytes, nc, FASTF_HVG_TOP);
        S->hvg_k = 0; S->nbr_planes = 0;
    }
    if (S->cfg.coexpr) {                                    /* the device and the pinned block of the partner sets.  The planes wait for P (fastf_res_full_keep) */
        const size_t map_bytes = S->nbr_map_bytes = res_nbr_map_bytes(S->n_features);
        const size_t dev_bytes = res_cx_layout(NULL, map_bytes, FASTF_COEXPR_K, FASTF_HVG_TOP).bytes;
        if (res_room(&S->buf.cx, RES_DEV, dev_bytes, device) || res_room(&S->buf.h_cx, RES_PIN, res_cx_pin_layout(NULL, map_bytes, FASTF_HVG_TOP).bytes, device))
            return no_room(S, "the co-expression sums and partner sets", dev_bytes);
        S->d_cx = res_cx_layout(S->buf.cx.p, map_bytes, FASTF_COEXPR_K, FASTF_HVG_TOP); S->h_cx = res_cx_pin_layout(S->buf.h_cx.p, map_bytes, FASTF_HVG_TOP);
        S->hvg_k = 0;
    }
    if (S->cfg.labels) {                                    /* the label block and its pinned copy; lab[] goes up once per pair */
        S->n_labels = fastf_labels_count(S->cfg.lab_t);
        const size_t lab_cells = res_lab_cells(room_cells), bytes = res_lab_layout(NULL, lab_cells, S->n_labels).bytes;
        if (res_room(&S->buf.lab, RES_DEV, bytes, device) || res_room(&S->buf.h_lab, RES_PIN, bytes, device)) return no_room(S, "the label arrays", bytes);
        S->d_lab = res_lab_layout(S->buf.lab.p, lab_cells, S->n_labels); S->h_lab = res_lab_layout(S->buf.h_lab.p, lab_cells, S->n_labels);
        const double tl = fastf_res_now();
        if (fastf_labels_assign(S->cfg.lab_t, L->barcode, n_cells, S->h_lab.lab) || (n_cells && fastf_devmem_copy(S->d_lab.lab, S->h_lab.lab, n_cells))) return RES_FAIL;
        T->labels += fastf_res_now() - tl;
    }
    if (S->cfg.ptime) {                                     /* the pseudotime block and its pinned copy; t[] is ranked among the pair's cells and goes up once per pair */
        const size_t pt_cells = res_pt_cells(room_cells), bytes = res_pt_layout(NULL, pt_cells).bytes;
        if (res_room(&S->buf.pt, RES_DEV, bytes, device) || res_room(&S->buf.h_pt, RES_PIN, bytes, device)) return no_room(S, "the pseudotime arrays", bytes);
        S->d_pt = res_pt_layout(S->buf.pt.p, pt_cells); S->h_pt = res_pt_layout(S->buf.h_pt.p, pt_cells);
        const double tp = fastf_res_now();
        if (fastf_ptime_assign(S->cfg.pt_t, L->barcode, n_cells, S->h_pt.t, &S->pt_m) || (n_cells && fastf_devmem_copy(S->d_pt.t, S->h_pt.t, (size_t)n_cells * 4))) return RES_FAIL;
        T->ptime += fastf_res_now() - tp;
    }
    if (S->cfg.mapping) {                                   /* the device and the pinned block of the mapping.  The copy of the full planes waits for P (fastf_res_full_keep) */
        const size_t lab_cells = S->cfg.labels ? res_lab_cells(room_cells) : 0, n_labels = S->cfg.labels ? S->n_labels : 0;
        const size_t dev_bytes = res_map_layout(NULL, FASTF_MAPPING_K, room_cells, lab_cells, n_labels, 0).bytes;
        if (res_room(&S->buf.map, RES_DEV, dev_bytes, device) || res_room(&S->buf.h_map, RES_PIN, res_map_layout(NULL, FASTF_MAPPING_K, room_cells, lab_cells, n_labels, 1).bytes, device))
            return no_room(S, "the mapping arrays", dev_bytes);
        S->d_map = res_map_layout(S->buf.map.p, FASTF_MAPPING_K, room_cells, lab_cells, n_labels, 0); S->h_map = res_map_layout(S->buf.h_map.p, FASTF_MAPPING_K, room_cells, lab_cells, n_labels, 1);
        S->full_planes = 0;
    }
    if (S->cfg.markers) {                                   /* the four tables of one row set on the device, of both row sets pinned, and the two rank tables */
        S->mk_set = res_mk_set_bytes(S->n_labels, FASTF_HVG_TOP);
        if (res_room(&S->buf.mk, RES_DEV, S->mk_set, device) || res_room(&S->buf.h_mk, RES_PIN, 2 * S->mk_set, device)) return no_room(S, "the marker tables", S->mk_set);
        if (res_room(&S->buf.mk_rank, RES_HOST, 2 * (size_t)S->n_labels * FASTF_HVG_TOP * sizeof(uint32_t), device)) { fastf_res_err("%s: out of memory", verb); return RES_FAIL; }
    }
    if (S->cfg.fidelity) {                                  /* the full rows of the pair, the three sums and their pinned copies with umis_full and genes_full, once */
        const size_t dev_bytes = res_fid_layout(NULL, room_cells, 0).bytes;
        if (res_room(&S->buf.full, RES_DEV, (N ? N : 1) * 12, device) || res_block_room(&S->buf.fid, RES_DEV, dev_bytes, room_cells, device) ||
            res_block_room(&S->buf.h_fid, RES_PIN, res_fid_layout(NULL, room_cells, 1).bytes, room_cells, device)) return no_room(S, "the full-depth rows", (size_t)(N * 12 + dev_bytes));
        S->d_fid = res_fid_layout(S->buf.fid.p, S->buf.fid.n, 0); S->h_fid = res_fid_layout(S->buf.h_fid.p, S->buf.h_fid.n, 1);
        S->full_nnz = 0;
    }
    uint64_t *const sm = S->buf.small.u64;
    if (fastf_devmem_zero(S->buf.small.p, SM_WORDS_ * 8) || fastf_dev_reserve(S->e, S->blocked ? 0 : N, N)) return RES_FAIL;

    /* the records into the engine's layout, K1a once: the cell scratch and the hit count serve every point */
    if (S->blocked) {
        /* the blocked copy is laid out again only where this engine's layout is not the one the copy is in (a new buffer holds none):
         * otherwise K1a alone, which fills the cell scratch slices of every unit */
        if (layout != S->blk_layout || !layout) {
            S->blk_layout = 0;
            if (fastf_dev_block_records(S->e, R->gx, R->umi, R->meta, N, S->buf.blk.p, NULL)) return RES_FAIL;
            S->blk_layout = layout;
            T->relays++;
        }
        if (fastf_dev_count_hits_blocked(S->e, R->cb, N, S->buf.blk.p, sm + SM_HITS, NULL)) return RES_FAIL;
    } else if (fastf_dev_count_hits(S->e, R->cb, N, sm + SM_HITS, NULL)) return RES_FAIL;
    if (fastf_devmem_sync() || fastf_devmem_copy(S->buf.h_small.u64, S->buf.small.p, SM_WORDS_ * 8)) return RES_FAIL;
    S->H = S->buf.h_small.u64[SM_HITS];
    T->block_k1a += fastf_res_now() - tt;
    return RES_OK;
}

/* ------------------------------------------------------------------ */
/* one point                                                           */
/* ------------------------------------------------------------------ */
/* K1b on the plane, the group-only sort and the reduce: what a point and a search pass begin with */
static int point_sort_reduce_(res_rate_t *S, const uint32_t *d_plane, uint64_t **src_out, uint64_t **other_out)
{
    const resident_t *R = S->R;
    const uint64_t N = R->n;
    fastf_engine_t *e = S->e;
    uint64_t *const sm = S->buf.small.u64;
    if (fastf_devmem_zero(S->buf.small.p, SM_HITS * 8)) return RES_FAIL;
    if (fastf_dev_probe_pack(e, R->cb, S->blocked ? S->buf.blk.u64 : R->gx, R->umi, R->meta, N, d_plane, S->H, sm + SM_BASE,
                             S->buf.keys.u64, S->key_slots, sm + SM_KEYS, sm + SM_CNT, S->kflags, NULL)) return RES_FAIL;
    int in_tmp = 0;
    if (fastf_dev_sort(e, S->buf.keys.u64, S->buf.tmp.u64, sm + SM_KEYS, N, S->key_bits, FASTF_SORT_SKIP_LOW | (S->segmented ? FASTF_SORT_SEGMENTED : 0), &in_tmp, NULL)) return RES_FAIL;
    uint64_t *src = in_tmp ? S->buf.tmp.u64 : S->buf.keys.u64, *other = in_tmp ? S->buf.keys.u64 : S->buf.tmp.u64;
    if (fastf_dev_reduce(e, src, sm + SM_KEYS, N, NULL, NULL, NULL, sm + SM_NNZ, FASTF_SORT_SKIP_LOW | FASTF_REDUCE_SEGMENTED, NULL)) return RES_FAIL;
    *src_out = src; *other_out = other;
    return RES_OK;
}
/* deep (cell, feature) groups (FASTF_ERR_RUN_TOO_LONG): sort fully and reduce again, as fastf_engine_finish does (every key is still
 * there, permuted) */
static int point_full_again_(res_rate_t *S, uint64_t **src_io, uint64_t **other_io)
{
    const uint64_t N = S->R->n;
    fastf_engine_t *e = S->e;
    uint64_t *const sm = S->buf.small.u64;
    uint64_t *src = *src_io, *other = *other_io;
    int in_other = 0;
    if (fastf_dev_clear_error_bits(e, FASTF_ERR_RUN_TOO_LONG, NULL) ||
        fastf_dev_sort(e, src, other, sm + SM_KEYS, N, S->key_bits, 0, &in_other, NULL)) return RES_FAIL;
    if (in_other) { uint64_t *t = src; src = other; other = t; }
    if (fastf_dev_reduce(e, src, sm + SM_KEYS, N, NULL, NULL, NULL, sm + SM_NNZ, FASTF_REDUCE_SEGMENTED, NULL)) return RES_FAIL;
    *src_io = src; *other_io = other;
    return RES_OK;
}

int fastf_res_point_run(res_rate_t *S, const uint32_t *d_plane, const char *point_name, uint64_t counters[3], uint64_t *nnz_out, res_times_t *T)
{
    const resident_t *R = S->R;
    const uint64_t N = R->n;
    fastf_engine_t *e = S->e;
    uint64_t *const sm = S->buf.small.u64;
    const res_rows_t d = res_rows_point(S);
    double tt = fastf_res_now();
    uint64_t *src = NULL, *other = NULL;
    if (point_sort_reduce_(S, d_plane, &src, &other)) return RES_FAIL;
    uint64_t bits = 0;
    if (fastf_dev_error_bits(e, &bits)) return RES_FAIL;
    S->sorted_full = 0;
    if (bits & FASTF_ERR_RUN_TOO_LONG) {
        if (point_full_again_(S, &src, &other) || fastf_dev_error_bits(e, &bits)) return RES_FAIL;
        S->sorted_full = 1;
    }
    S->sorted = src; S->sorted_other = other;
    if (fastf_devmem_copy(S->buf.h_small.u64, S->buf.small.p, SM_HITS * 8)) return RES_FAIL;
    bits |= S->buf.h_small.u64[SM_CNT + 3];
    if (bits & 4) return RES_NOT_COVERED;                   /* UMIs longer than the key holds: bam2db() runs such a file again with wider keys */
    if (bits) { fastf_res_err("%s: device error bits 0x%llx at point %s", S->verb, (unsigned long long)bits, point_name); return RES_FAIL; }
    counters[0] = N; counters[1] = S->buf.h_small.u64[SM_CNT + 1]; counters[2] = S->buf.h_small.u64[SM_CNT + 2];
    const uint64_t nnz = *nnz_out = S->buf.h_small.u64[SM_NNZ];
    if (nnz > N) { fastf_res_err("internal error: %llu matrix rows out of %llu records", (unsigned long long)nnz, (unsigned long long)N); return RES_FAIL; }
    /* the rows, concatenated on the device, and their per-cell summary */
    if (fastf_dev_rows_gather(e, sm + SM_KEYS, d.f, d.c, d.k, NULL) ||
        fastf_dev_cell_summary(e, nnz ? d.c : NULL, nnz ? d.k : NULL, sm + SM_NNZ, S->n_cells, S->buf.upc.u64, S->buf.gpc.u32, NULL) ||
        (S->genes && fastf_dev_gene_summary(e, nnz ? d.f : NULL, nnz ? d.k : NULL, sm + SM_NNZ, S->n_features, S->buf.cpg.u32, S->buf.upg.u64, NULL)) ||
        fastf_devmem_sync()) return RES_FAIL;
    T->device += fastf_res_now() - tt; tt = fastf_res_now();
    if (fastf_devmem_copy(S->buf.h_upc.u64, S->buf.upc.p, ((size_t)S->n_cells + 1) * 8) || fastf_devmem_copy(S->buf.h_gpc.u32, S->buf.gpc.p, (size_t)S->n_cells * 4)) return RES_FAIL;
    T->summary += fastf_res_now() - tt;
    if (S->genes) {
        tt = fastf_res_now();
        if (S->n_features && (fastf_devmem_copy(S->buf.h_cpg.u32, S->buf.cpg.p, (size_t)S->n_features * 4) || fastf_devmem_copy(S->buf.h_upg.u64, S->buf.upg.p, (size_t)S->n_features * 8))) return RES_FAIL;
        T->genes += fastf_res_now() - tt;
    }
    return RES_OK;
}

/* ------------------------------------------------------------------ */
/* level: the state arrays, a search pass                              */
/* ------------------------------------------------------------------ */
int fastf_res_level_room(res_rate_t *S)
{
    const size_t room_cells = (S->cfg.max_cells > S->n_cells ? S->cfg.max_cells : S->n_cells) + (size_t)1;
    const size_t bytes = res_level_layout(NULL, room_cells).bytes;
    if (res_block_room(&S->buf.level, RES_DEV, bytes, room_cells, S->device))
        return fastf_res_err("%s: the search state of cell rate %.3f does not fit: %zu bytes (%s)", S->verb, (double)S->rate_cell, bytes, fastf_last_error());
    S->lv = res_level_layout(S->buf.level.p, S->buf.level.n);
    return 0;
}

/* the small block to the host — the one copy of a pass — and what it says: RES_OK with *held = 0 (the state moved), *held = 1 (a
 * run was too long for the group-only sort and nothing else is wrong: the caller sorts fully and steps again), or the end of the run */
static int level_result_(res_rate_t *S, const char *point_name, int *held, uint64_t *open_out, uint64_t *capped_out)
{
    if (fastf_devmem_copy(S->buf.h_small.u64, S->buf.small.p, SM_WORDS_ * 8)) return RES_FAIL;
    const uint64_t *const r = S->buf.h_small.u64 + SM_LEVEL;
    const uint64_t bits = r[2] | S->buf.h_small.u64[SM_CNT + 3];
    *held = 0;
    if (bits & 4) return RES_NOT_COVERED;                   /* UMIs longer than the key holds: as in fastf_res_point_run */
    if (bits == FASTF_ERR_RUN_TOO_LONG && r[3]) { *held = 1; return RES_OK; }
    if (bits || r[3]) { fastf_res_err("%s: device error bits 0x%llx in the search of point %s", S->verb, (unsigned long long)bits, point_name); return RES_FAIL; }
    if (S->buf.h_small.u64[SM_NNZ] > S->R->n) { fastf_res_err("internal error: %llu matrix rows out of %llu records", (unsigned long long)S->buf.h_small.u64[SM_NNZ], (unsigned long long)S->R->n); return RES_FAIL; }
    *open_out = r[0];
    if (capped_out) *capped_out = r[1];
    return RES_OK;
}

int fastf_res_search_pass(res_rate_t *S, const uint32_t *d_plane, const char *point_name, uint64_t umi_cap, int first, uint64_t *open_out,
                          uint64_t *capped_out, res_times_t *T)
{
    fastf_engine_t *e = S->e;
    uint64_t *const sm = S->buf.small.u64;
    const res_rows_t d = res_rows_point(S);
    const double t0 = fastf_res_now();
    if (!S->buf.level.p) { fastf_res_err("internal error: no search state at point %s", point_name); return RES_FAIL; }
    uint64_t *src = NULL, *other = NULL;
    if (point_sort_reduce_(S, d_plane, &src, &other)) return RES_FAIL;
    S->sorted = NULL; S->sorted_full = 0;                   /* (a search pass leaves no keys for --cells: the point's own run does) */
    for (int again = 0;; again++) {
        /* the rows concatenated on the device, their per-cell summary, the step: the row count is read on the device (a reduce that
         * raised an error bit leaves rows the step does not consume) */
        if (fastf_dev_rows_gather(e, sm + SM_KEYS, d.f, d.c, d.k, NULL) ||
            fastf_dev_cell_summary(e, d.c, d.k, sm + SM_NNZ, S->n_cells, S->buf.upc.u64, S->buf.gpc.u32, NULL) ||
            (first ? fastf_dev_level_init(e, S->buf.upc.u64, S->n_cells, umi_cap, S->lv.lo, S->lv.hi, S->lv.probe, sm + SM_LEVEL, sm + SM_CNT + 3, NULL)
                   : fastf_dev_level_step(e, S->buf.upc.u64, S->n_cells, umi_cap, S->lv.lo, S->lv.hi, S->lv.probe, sm + SM_LEVEL, sm + SM_CNT + 3, NULL)))
            return RES_FAIL;
        int held = 0;
        const int rc = level_result_(S, point_name, &held, open_out, first ? capped_out : NULL);
        if (rc != RES_OK) return rc;
        if (!held) break;
        if (again) { fastf_res_err("%s: device error bits 0x%llx after the full sort in the search of point %s", S->verb, (unsigned long long)FASTF_ERR_RUN_TOO_LONG, point_name); return RES_FAIL; }
        if (point_full_again_(S, &src, &other)) return RES_FAIL;
    }
    if (first && fastf_devmem_copy(S->lv.ufull, S->buf.upc.p, ((size_t)S->n_cells + 1) * 8)) return RES_FAIL;
    T->search += fastf_res_now() - t0; T->passes++;
    return RES_OK;
}

int fastf_res_level_init(res_rate_t *S, uint64_t umi_cap, uint64_t *open_out, uint64_t *capped_out, res_times_t *T)
{
    uint64_t *const sm = S->buf.small.u64;
    const double t0 = fastf_res_now();
    int held = 0;
    if (!S->buf.level.p) { fastf_res_err("internal error: no search state"); return RES_FAIL; }
    if (fastf_devmem_zero(S->buf.small.p, SM_HITS * 8) ||       /* (the counters of the point before: their error word is read again) */
        fastf_dev_level_init(S->e, S->lv.ufull, S->n_cells, umi_cap, S->lv.lo, S->lv.hi, S->lv.probe, sm + SM_LEVEL, NULL, NULL)) return RES_FAIL;
    const int rc = level_result_(S, "(the state of a cap)", &held, open_out, capped_out);
    if (rc != RES_OK) return rc;
    if (held) { fastf_res_err("%s: device error bits 0x%llx before a search", S->verb, (unsigned long long)FASTF_ERR_RUN_TOO_LONG); return RES_FAIL; }
    T->search += fastf_res_now() - t0;
    return RES_OK;
}

int fastf_res_point_write(res_rate_t *S, const char *dir, const char *bam_label, float rate_depth, const uint64_t counters[3], uint64_t nnz, res_times_t *T)
{
    uint64_t *const sm = S->buf.small.u64;
    double tt = fastf_res_now();
    if (nnz > S->buf.h_rows.n) {                            /* (more than there is room for: the need below is beyond what is held) */
        const size_t room = nnz + nnz / 8 + 1024;
        if (res_block_room(&S->buf.h_rows, RES_PIN, room * 12, room, S->device)) return fastf_res_err("%s: no pinned memory for %llu matrix rows", S->verb, (unsigned long long)nnz);
    }
    uint32_t *const h_rows = S->buf.h_rows.u32; const uint64_t cap = S->buf.h_rows.n;
    fastf_coo_t coo = { h_rows, h_rows + cap, h_rows + 2 * cap, (size_t)nnz };
    /* (the gather kernel writes pinned host memory directly: it is the device-to-host copy of the rows) */
    if (nnz && (fastf_dev_rows_gather(S->e, sm + SM_KEYS, h_rows, h_rows + cap, h_rows + 2 * cap, NULL) || fastf_devmem_sync())) return 1;
    T->d2h += fastf_res_now() - tt; tt = fastf_res_now();
    if (fastf_res_make_dir(dir) || fastf_write_outputs(dir, bam_label, S->rate_cell, rate_depth, counters, S->L, &coo, NULL)) return 1;
    T->write += fastf_res_now() - tt;
    return 0;
}

/* ------------------------------------------------------------------ */
/* --fidelity: the full rows of a pair, the join behind a point        */
/* ------------------------------------------------------------------ */
static const char *fastf_last_error_copy(void) { static __thread char keep[400]; snprintf(keep, sizeof keep, "%s", fastf_last_error()); return keep; }

/* the planes of one row set (P planes: what the largest count of the set needs) and its neighbour sets into the full (point == 0) or
 * the point's half of the block */
static int nbr_sets(res_rate_t *S, const uint32_t *r_f, const uint32_t *r_c, const uint32_t *r_k, const uint64_t *d_nnz, uint32_t P, int point)
{
    uint32_t n_pad = 0, K_pad = 0;
    uint64_t max_norm = 0;
    fastf_neighbors_pad(S->n_cells, S->hvg_k, &n_pad, &K_pad);
    const size_t need = (size_t)P * n_pad * K_pad;
    if (res_room(&S->buf.nplanes, RES_DEV, need ? need : 1, S->device))
        return fastf_res_err("%s: --neighbors: %u planes of %u cells x %u genes do not fit: %zu bytes (%s)", S->verb, P, n_pad, K_pad, need, fastf_last_error_copy());
    if (fastf_dev_neighbor_planes(S->e, r_f, r_c, r_k, d_nnz, S->d_nbr.map, S->n_features, S->n_cells, S->hvg_k, S->buf.nplanes.p, S->buf.nplanes.have, &P, NULL) ||
        fastf_dev_neighbors(S->e, S->buf.nplanes.p, P, S->n_cells, S->hvg_k, FASTF_NEIGHBORS_K, S->d_nbr.idx[point], S->d_nbr.cnt[point],
                            S->d_nbr.norms, &max_norm, NULL) || fastf_devmem_sync())
        return fastf_res_err("%s: --neighbors at cell rate %.3f, seed %u: %s", S->verb, (double)S->rate_cell, S->seed, fastf_last_error_copy());
    S->nbr_planes = P;
    return 0;
}

int fastf_res_point_neighbors(res_rate_t *S, const char *point_name, res_times_t *T)
{
    if (!S->cfg.neighbors) return 0;
    const uint64_t nnz = S->buf.h_small.u64[SM_NNZ];
    uint64_t *const sm = S->buf.small.u64;
    const res_rows_t d = res_rows_point(S);
    uint32_t P = 0;
    const double tt = fastf_res_now();
    /* (a point's counts are at most the full ones: P of the point never exceeds P of the pair) */
    if (fastf_dev_neighbor_planes(S->e, nnz ? d.f : NULL, d.c, d.k, sm + SM_NNZ, S->d_nbr.map, S->n_features, S->n_cells, S->hvg_k, NULL, 0, &P, NULL))
        return fastf_res_err("%s: --neighbors at point %s: %s", S->verb, point_name, fastf_last_error_copy());
    if (nbr_sets(S, nnz ? d.f : NULL, d.c, d.k, sm + SM_NNZ, P, 1)) return 1;
    if (fastf_dev_neighbors_shared(S->e, S->d_nbr.idx[0], S->d_nbr.cnt[0], S->d_nbr.idx[1], S->d_nbr.cnt[1], S->n_cells, FASTF_NEIGHBORS_K, S->d_nbr.shared, NULL) || fastf_devmem_sync()) return 1;
    if (S->n_cells && (fastf_devmem_copy(S->h_nbr.kp, S->d_nbr.cnt[1], (size_t)S->n_cells * 4) || fastf_devmem_copy(S->h_nbr.sh, S->d_nbr.shared, (size_t)S->n_cells * 4))) return 1;
    T->neighbors += fastf_res_now() - tt;
    return 0;
}

/* --labels: one vote call on the full (point == 0) or the point's neighbour sets, then that half of the block to the host in one copy */
static int lab_votes(res_rate_t *S, int point)
{
    if (fastf_dev_label_votes(S->e, S->d_nbr.idx[point], S->d_nbr.cnt[point], S->d_lab.lab, S->n_cells, FASTF_NEIGHBORS_K, S->n_labels,
                              S->d_lab.half[point].pred, S->d_lab.half[point].same, S->d_lab.half[point].labelled, S->d_lab.half[point].conf, NULL) || fastf_devmem_sync())
        return fastf_res_err("%s: --labels at cell rate %.3f, seed %u: %s", S->verb, (double)S->rate_cell, S->seed, fastf_last_error_copy());
    return fastf_devmem_copy(S->h_lab.half[point].pred, S->d_lab.half[point].pred, S->d_lab.half_bytes);
}

int fastf_res_point_labels(res_rate_t *S, const char *point_name, res_times_t *T)
{
    if (!S->cfg.labels) return 0;
    (void)point_name;
    const double tt = fastf_res_now();
    if (lab_votes(S, 1)) return 1;
    T->labels += fastf_res_now() - tt;
    return 0;
}

/* --pseudotime: the medians over one list of neighbours (the full sets: side 0, the point's: 1, the mapping list: 2) and their census,
 * then that half of the block to the host in one copy */
static int pt_side(res_rate_t *S, int side, const uint32_t *d_idx, const uint32_t *d_cnt, const char *where)
{
    if (fastf_dev_ptime_medians(S->e, d_idx, d_cnt, S->d_pt.t, S->n_cells, FASTF_NEIGHBORS_K, S->d_pt.half[side].est, S->d_pt.half[side].valued, NULL) ||
        fastf_dev_ptime_census(S->e, S->d_pt.half[side].est, S->d_pt.t, S->n_cells, S->d_pt.half[side].census, NULL) || fastf_devmem_sync())
        return fastf_res_err("%s: --pseudotime at %s: %s", S->verb, where, fastf_last_error_copy());
    return fastf_devmem_copy(S->h_pt.half[side].census, S->d_pt.half[side].census, S->d_pt.half_bytes);
}

int fastf_res_point_ptime(res_rate_t *S, const char *point_name, res_times_t *T)
{
    if (!S->cfg.ptime) return 0;
    char where[128];
    const double tt = fastf_res_now();
    snprintf(where, sizeof where, "point %s", point_name);
    if (pt_side(S, 1, S->d_nbr.idx[1], S->d_nbr.cnt[1], where)) return 1;
    T->ptime += fastf_res_now() - tt;
    return 0;
}

_Static_assert(FASTF_MAPPING_K == FASTF_NEIGHBORS_K, "hood compares M(i) with the full neighbour set of the same k");
int fastf_res_point_mapping(res_rate_t *S, const char *point_name, res_times_t *T)
{
    if (!S->cfg.mapping) return 0;
    const res_map_v d = S->d_map;
    uint64_t max_norm = 0;
    const double tt = fastf_res_now();
    /* (the point's planes are still in the plane buffer, S->nbr_planes of them: fastf_res_point_neighbors ran directly before) */
    if (fastf_dev_mapping(S->e, S->buf.nplanes.p, S->nbr_planes, S->buf.fplanes.p, S->full_planes, S->n_cells, S->hvg_k, FASTF_MAPPING_K, d.norms, d.idx, d.km, d.sd, d.rank,
                          &max_norm, NULL) ||
        fastf_dev_neighbors_shared(S->e, d.idx, d.km, S->d_nbr.idx[0], S->d_nbr.cnt[0], S->n_cells, FASTF_MAPPING_K, d.hood, NULL) ||
        (S->cfg.labels && fastf_dev_label_votes(S->e, d.idx, d.km, S->d_lab.lab, S->n_cells, FASTF_MAPPING_K, S->n_labels, d.pred, d.same, d.labelled, d.conf, NULL)) ||
        fastf_devmem_sync())
        return fastf_res_err("%s: --mapping at point %s: %s", S->verb, point_name, fastf_last_error_copy());
    if (S->n_cells && fastf_devmem_copy(S->h_map.sd, d.sd, d.out_bytes)) return 1;
    T->mapping += fastf_res_now() - tt;
    if (S->cfg.ptime) {                                     /* the ranks M(i) carries, while the list is live: its cells are full-depth cells of the same pair */
        char where[128];
        const double tp = fastf_res_now();
        snprintf(where, sizeof where, "point %s (the mapping list)", point_name);
        if (pt_side(S, 2, d.idx, d.km, where)) return 1;
        T->ptime += fastf_res_now() - tp;
    }
    return 0;
}

/* --markers: one kernel call on the planes at hand (S->nbr_planes of them: the full rows', point == 0, or the point's), the four tables
 * to the host in one copy, then the ranks */
static int mk_tables(res_rate_t *S, int point)
{
    const res_mk_v dm = res_mk_layout(S->buf.mk.p, S->n_labels, S->hvg_k), hm = res_mk_host(S, point);
    if (fastf_dev_marker_auc(S->e, S->buf.nplanes.p, S->nbr_planes, S->n_cells, S->hvg_k, S->d_lab.lab, S->n_labels, dm.s2u, dm.det, dm.sum, dm.npl, NULL) ||
        fastf_devmem_sync())
        return fastf_res_err("%s: --markers at cell rate %.3f, seed %u: %s", S->verb, (double)S->rate_cell, S->seed, fastf_last_error_copy());
    if (fastf_devmem_copy(hm.s2u, dm.s2u, dm.bytes)) return 1;
    return fastf_marker_rank(hm.s2u, hm.npl, S->h_nbr.genes, S->hvg_k, S->n_labels, S->buf.mk_rank.u32 + (size_t)point * S->n_labels * FASTF_HVG_TOP);
}

int fastf_res_point_markers(res_rate_t *S, const char *point_name, res_times_t *T)
{
    if (!S->cfg.markers) return 0;
    (void)point_name;
    const double tt = fastf_res_now();
    if (mk_tables(S, 1)) return 1;
    T->markers += fastf_res_now() - tt;
    return 0;
}

/* --coexpression: the gene-major planes of one row set (P planes: what the largest count of the set needs), its D and S and its partner
 * sets into the full (point == 0) or the point's half of the block; `where` names the pair or the point in a failure */
static int cx_sets(res_rate_t *S, const uint32_t *r_f, const uint32_t *r_c, const uint32_t *r_k, const uint64_t *d_nnz, int point, const char *where)
{
    uint32_t P = 0;
    if (fastf_dev_neighbor_planes(S->e, r_f, r_c, r_k, d_nnz, S->d_cx.map, S->n_features, S->n_cells, S->hvg_k, NULL, 0, &P, NULL))
        return fastf_res_err("%s: --coexpression at %s: %s", S->verb, where, fastf_last_error_copy());
    const size_t need = fastf_coexpr_work_bytes(S->n_cells, S->hvg_k, P);
    if (res_room(&S->buf.cxwork, RES_DEV, need ? need : 1, S->device))
        return fastf_res_err("%s: --coexpression at %s: %u planes of %u genes x %u cells do not fit: %zu bytes (%s)", S->verb, where, P, S->hvg_k, S->n_cells, need, fastf_last_error_copy());
    if (fastf_dev_coexpr_sums(S->e, r_f, r_c, r_k, d_nnz, S->d_cx.map, S->n_features, S->n_cells, S->hvg_k, P, S->buf.cxwork.p, S->buf.cxwork.have, S->d_cx.D, S->d_cx.S, NULL) ||
        fastf_dev_coexpr_select(S->e, S->d_cx.D, S->d_cx.S, S->n_cells, S->hvg_k, FASTF_COEXPR_K, S->d_cx.idx[point], S->d_cx.cnt[point], NULL) || fastf_devmem_sync())
        return fastf_res_err("%s: --coexpression at %s: %s", S->verb, where, fastf_last_error_copy());
    return 0;
}

int fastf_res_point_coexpr(res_rate_t *S, const char *point_name, res_times_t *T)
{
    if (!S->cfg.coexpr) return 0;
    const uint64_t nnz = S->buf.h_small.u64[SM_NNZ];
    const res_rows_t d = res_rows_point(S);
    char where[128];
    const double tt = fastf_res_now();
    snprintf(where, sizeof where, "point %s", point_name);
    if (cx_sets(S, nnz ? d.f : NULL, d.c, d.k, S->buf.small.u64 + SM_NNZ, 1, where)) return 1;
    if (fastf_dev_neighbors_shared(S->e, S->d_cx.idx[0], S->d_cx.cnt[0], S->d_cx.idx[1], S->d_cx.cnt[1], S->hvg_k, FASTF_COEXPR_K, S->d_cx.shared, NULL) || fastf_devmem_sync())
        return fastf_res_err("%s: --coexpression at %s: %s", S->verb, where, fastf_last_error_copy());
    if (S->hvg_k && (fastf_devmem_copy(S->h_cx.kp, S->d_cx.cnt[1], (size_t)S->hvg_k * 4) || fastf_devmem_copy(S->h_cx.sh, S->d_cx.shared, (size_t)S->hvg_k * 4)))
        return fastf_res_err("%s: --coexpression at %s: %s", S->verb, where, fastf_last_error_copy());
    T->coexpr += fastf_res_now() - tt;
    return 0;
}

/* where the full-depth work of a pair is booked: under the first flag that is on, in the order fidelity, gene fidelity, neighbours;
 * then co-expression; per_gene: the per-gene sums of the pair, which --fidelity has no part in */
double *fastf_res_full_timer(const res_rate_t *S, res_times_t *T, int per_gene)
{
    return S->cfg.fidelity && !per_gene ? &T->fidelity : S->cfg.gene_fid ? &T->gene_fid : S->cfg.neighbors ? &T->neighbors : &T->coexpr;
}

int fastf_res_full_keep(res_rate_t *S, res_times_t *T)
{
    if (!res_cfg_full(&S->cfg)) return 0;
    const uint64_t N = S->R->n, nnz = S->buf.h_small.u64[SM_NNZ];
    uint64_t *const sm = S->buf.small.u64;
    const res_rows_t d = res_rows_point(S), x = res_rows_full(S);
    double tt = fastf_res_now();
    if (nnz > N) return fastf_res_err("internal error: %llu full-depth rows out of %llu records", (unsigned long long)nnz, (unsigned long long)N);
    if (fastf_devmem_copy(x.f, d.f, (size_t)nnz * 4) || fastf_devmem_copy(x.c, d.c, (size_t)nnz * 4) || fastf_devmem_copy(x.k, d.k, (size_t)nnz * 4) ||
        fastf_devmem_copy(sm + SM_FULL, sm + SM_NNZ, 8)) return 1;
    S->full_nnz = nnz;
    if (res_cfg_per_gene(&S->cfg)) {                                /* per gene sum_x and cells_full (the per-gene summary of the full rows), sum_xx (their moments with themselves) */
        uint64_t *const g_sx = S->d_gfid.sx, *const g_sxx = S->d_gfid.sxx;
        uint32_t *const g_cf = S->d_gfid.cf;
        if (fastf_dev_gene_summary(S->e, nnz ? x.f : NULL, nnz ? x.k : NULL, sm + SM_FULL, S->n_features, g_cf, g_sx, NULL) ||
            fastf_dev_gene_moments(S->e, nnz ? x.f : NULL, nnz ? x.k : NULL, nnz ? x.k : NULL, sm + SM_FULL, S->n_features, NULL, g_sxx, NULL) ||
            fastf_devmem_sync()) return 1;
        if (S->n_features && (fastf_devmem_copy(S->h_gfid.sx, g_sx, (size_t)S->n_features * 8) || fastf_devmem_copy(S->h_gfid.sxx, g_sxx, (size_t)S->n_features * 8) ||
                              fastf_devmem_copy(S->h_gfid.cf, g_cf, (size_t)S->n_features * 4))) return 1;
        *fastf_res_full_timer(S, T, 1) += fastf_res_now() - tt; tt = fastf_res_now();
    }
    if (S->cfg.neighbors) {                                     /* A of the pair, its slot map, the planes of the full rows and their neighbour sets, which stay */
        uint32_t P = 0;
        S->hvg_k = fastf_hvg_rank(S->n_cells, S->h_gfid.sx, S->h_gfid.sxx, S->n_features, S->h_nbr.genes, NULL);
        if (fastf_neighbors_slot_map(S->h_nbr.genes, S->hvg_k, S->n_features, S->h_nbr.map) || fastf_devmem_copy(S->d_nbr.map, S->h_nbr.map, S->nbr_map_bytes)) return 1;
        if (fastf_dev_neighbor_planes(S->e, nnz ? x.f : NULL, x.c, x.k, sm + SM_FULL, S->d_nbr.map, S->n_features, S->n_cells, S->hvg_k, NULL, 0, &P, NULL))
            return fastf_res_err("%s: --neighbors at cell rate %.3f, seed %u: %s", S->verb, (double)S->rate_cell, S->seed, fastf_last_error_copy());
        if (nbr_sets(S, nnz ? x.f : NULL, x.c, x.k, sm + SM_FULL, P, 0)) return 1;
        if (S->n_cells && fastf_devmem_copy(S->h_nbr.kf, S->d_nbr.cnt[0], (size_t)S->n_cells * 4)) return 1;
        T->neighbors += fastf_res_now() - tt; tt = fastf_res_now();
    }
    if (S->cfg.labels) {                                        /* the votes of the full sets, which stay for every point of the pair */
        if (lab_votes(S, 0)) return 1;
        T->labels += fastf_res_now() - tt; tt = fastf_res_now();
    }
    if (S->cfg.ptime) {                                         /* the estimates and the census of the full sets, which stay for every point of the pair */
        char where[96];
        snprintf(where, sizeof where, "cell rate %.3f, seed %u", (double)S->rate_cell, S->seed);
        if (pt_side(S, 0, S->d_nbr.idx[0], S->d_nbr.cnt[0], where)) return 1;
        T->ptime += fastf_res_now() - tt; tt = fastf_res_now();
    }
    if (S->cfg.markers) {                                       /* the tables and ranks of the full rows, while their planes are still in the plane buffer */
        if (mk_tables(S, 0)) return 1;
        T->markers += fastf_res_now() - tt; tt = fastf_res_now();
    }
    if (S->cfg.mapping) {                                       /* the planes and the norms of the full rows, before the first point overwrites the plane buffer and the norms */
        uint32_t n_pad = 0, K_pad = 0;
        fastf_neighbors_pad(S->n_cells, S->hvg_k, &n_pad, &K_pad);
        const size_t bytes = (size_t)S->nbr_planes * n_pad * K_pad;
        if (res_room(&S->buf.fplanes, RES_DEV, bytes, S->device))
            return fastf_res_err("%s: --mapping: the %u planes of the full-depth rows, %u cells x %u genes, do not fit: %zu bytes (%s)", S->verb, S->nbr_planes, n_pad, K_pad, bytes, fastf_last_error_copy());
        if (fastf_devmem_copy(S->buf.fplanes.p, S->buf.nplanes.p, bytes) || (S->n_cells && fastf_devmem_copy(S->d_map.norms, S->d_nbr.norms, (size_t)S->n_cells * 8))) return 1;
        S->full_planes = S->nbr_planes;
        T->mapping += fastf_res_now() - tt; tt = fastf_res_now();
    }
    if (S->cfg.coexpr) {                                        /* A of the pair as --neighbors ranks it (its own ranking and slot map without that option), the partner sets of the full rows, which stay */
        char where[96];
        snprintf(where, sizeof where, "cell rate %.3f, seed %u", (double)S->rate_cell, S->seed);
        if (S->cfg.neighbors) { memcpy(S->h_cx.genes, S->h_nbr.genes, (size_t)S->hvg_k * 4); memcpy(S->h_cx.map, S->h_nbr.map, S->nbr_map_bytes); }
        else {
            S->hvg_k = fastf_hvg_rank(S->n_cells, S->h_gfid.sx, S->h_gfid.sxx, S->n_features, S->h_cx.genes, NULL);
            if (fastf_neighbors_slot_map(S->h_cx.genes, S->hvg_k, S->n_features, S->h_cx.map)) return fastf_res_err("%s: --coexpression at %s: %s", S->verb, where, fastf_last_error_copy());
        }
        if (fastf_devmem_copy(S->d_cx.map, S->h_cx.map, S->nbr_map_bytes)) return fastf_res_err("%s: --coexpression at %s: %s", S->verb, where, fastf_last_error_copy());
        if (cx_sets(S, nnz ? x.f : NULL, x.c, x.k, sm + SM_FULL, 0, where)) return 1;
        if (S->hvg_k && fastf_devmem_copy(S->h_cx.kf, S->d_cx.cnt[0], (size_t)S->hvg_k * 4)) return fastf_res_err("%s: --coexpression at %s: %s", S->verb, where, fastf_last_error_copy());
        T->coexpr += fastf_res_now() - tt; tt = fastf_res_now();
    }
    if (!S->cfg.fidelity) return 0;
    /* sum_xx: the full rows joined with themselves (sum_xy == sum_yy; the first of the two lands in the point's own slot, which the
     * first point overwrites) */
    if (fastf_dev_fidelity(S->e, x.f, x.c, x.k, sm + SM_FULL, nnz ? x.f : NULL, nnz ? x.c : NULL, nnz ? x.k : NULL, sm + SM_FULL, S->n_cells, S->d_fid.sxy, S->d_fid.sxx, NULL, NULL)) return 1;
    if (fastf_devmem_copy(S->h_fid.sxx, S->d_fid.sxx, (size_t)S->n_cells * 8) || fastf_devmem_copy(S->h_fid.ufull, S->buf.upc.p, ((size_t)S->n_cells + 1) * 8) ||
        fastf_devmem_copy(S->h_fid.gfull, S->buf.gpc.p, (size_t)S->n_cells * 4)) return 1;
    T->fidelity += fastf_res_now() - tt;
    return 0;
}

int fastf_res_full_run(res_rate_t *S, const uint32_t *d_plane, res_times_t *T)
{
    if (!res_cfg_full(&S->cfg)) return RES_OK;
    char name[64];
    uint64_t counters[3], nnz = 0;
    const res_times_t before = *T;
    const double tt = fastf_res_now();
    snprintf(name, sizeof name, "c%.3f (every hit)", (double)S->rate_cell);
    const int prc = fastf_res_point_run(S, d_plane, name, counters, &nnz, T);
    if (prc != RES_OK) return prc;
    *T = before;                                            /* (the stages of this point are the flag's own) */
    *fastf_res_full_timer(S, T, 0) += fastf_res_now() - tt;
    return fastf_res_full_keep(S, T) ? RES_FAIL : RES_OK;
}

int fastf_res_point_fidelity(res_rate_t *S, const char *point_name, res_times_t *T)
{
    if (!S->cfg.fidelity) return 0;
    const uint64_t nnz = S->buf.h_small.u64[SM_NNZ];
    uint64_t *const sm = S->buf.small.u64;
    const res_rows_t d = res_rows_point(S), x = res_rows_full(S);
    const double tt = fastf_res_now();
    if (fastf_dev_fidelity(S->e, x.f, x.c, x.k, sm + SM_FULL, nnz ? d.f : NULL, nnz ? d.c : NULL, nnz ? d.k : NULL, sm + SM_NNZ, S->n_cells, S->d_fid.sxy, S->d_fid.syy, NULL, NULL))
        return fastf_res_err("%s: point %s against the full-depth rows of its cell rate and seed: %s", S->verb, point_name, fastf_last_error_copy());
    if (fastf_devmem_copy(S->h_fid.sxy, S->d_fid.sxy, (size_t)S->n_cells * 8) || fastf_devmem_copy(S->h_fid.syy, S->d_fid.syy, (size_t)S->n_cells * 8)) return 1;
    T->fidelity += fastf_res_now() - tt;
    return 0;
}

int fastf_res_point_gene_fidelity(res_rate_t *S, const char *point_name, res_times_t *T)
{
    if (!S->cfg.gene_fid) return 0;
    const uint64_t nnz = S->buf.h_small.u64[SM_NNZ];
    uint64_t *const sm = S->buf.small.u64;
    const res_rows_t d = res_rows_point(S), x = res_rows_full(S);
    uint64_t *const g_sy = S->d_gfid.sy, *const g_syy = S->d_gfid.syy, *const g_sxy = S->d_gfid.sxy;
    uint32_t *const g_c = S->d_gfid.c, *const d_x = S->buf.gx.u32;
    const double tt = fastf_res_now();
    if (fastf_dev_partner_counts(S->e, x.f, x.c, x.k, sm + SM_FULL, nnz ? d.f : NULL, nnz ? d.c : NULL, sm + SM_NNZ, d_x, NULL, NULL))
        return fastf_res_err("%s: point %s against the full-depth rows of its cell rate and seed: %s", S->verb, point_name, fastf_last_error_copy());
    /* (with --genes fastf_res_point_run has left the point's sum_y and cells in S->buf.h_upg and S->buf.h_cpg) */
    if ((!S->genes && fastf_dev_gene_summary(S->e, nnz ? d.f : NULL, nnz ? d.k : NULL, sm + SM_NNZ, S->n_features, g_c, g_sy, NULL)) ||
        fastf_dev_gene_moments(S->e, nnz ? d.f : NULL, nnz ? d_x : NULL, nnz ? d.k : NULL, sm + SM_NNZ, S->n_features, g_sxy, g_syy, NULL) ||
        fastf_devmem_sync()) return 1;
    if (S->n_features && (fastf_devmem_copy(S->h_gfid.syy, g_syy, (size_t)S->n_features * 8) || fastf_devmem_copy(S->h_gfid.sxy, g_sxy, (size_t)S->n_features * 8) ||
                          (!S->genes && (fastf_devmem_copy(S->h_gfid.sy, g_sy, (size_t)S->n_features * 8) || fastf_devmem_copy(S->h_gfid.c, g_c, (size_t)S->n_features * 4))))) return 1;
    T->gene_fid += fastf_res_now() - tt;
    return 0;
}

int fastf_res_point_compare(res_rate_t *S, const char *point_name, res_times_t *T)
{
    if (fastf_res_point_fidelity(S, point_name, T)) return 1;     /* (the point's rows are still in the row buffer) */
    if (fastf_res_point_gene_fidelity(S, point_name, T)) return 1;
    if (fastf_res_point_neighbors(S, point_name, T)) return 1;
    if (fastf_res_point_labels(S, point_name, T)) return 1;       /* (directly behind the neighbour sets it votes with) */
    if (fastf_res_point_ptime(S, point_name, T)) return 1;        /* (on the same sets) */
    if (fastf_res_point_mapping(S, point_name, T)) return 1;      /* (the point's byte planes against the full rows' planes) */
    if (fastf_res_point_markers(S, point_name, T)) return 1;      /* (on the byte planes those sets were made of) */
    return fastf_res_point_coexpr(S, point_name, T);             /* (on planes of its own) */
}

/* --cells: behind the point.  The full sort and K3u use the engine's workspace, and K3u writes the engine's row regions — the count
 * array and the span tables of the matrix rows — so this runs once fastf_res_point_write has gathered them (resident.h) */
int fastf_res_point_cells(res_rate_t *S, const char *point_name, res_times_t *T)
{
    if (!S->cells) return 0;
    const uint64_t N = S->R->n;
    fastf_engine_t *e = S->e;
    uint64_t *const sm = S->buf.small.u64;
    double tt = fastf_res_now();
    if (!S->sorted) return fastf_res_err("internal error: no sorted keys at point %s", point_name);
    uint64_t *src = S->sorted;
    if (!S->sorted_full) {                                  /* (every key is still there, sorted but for its low bits) */
        int in_other = 0;
        if (fastf_dev_sort(e, src, S->sorted_other, sm + SM_KEYS, N, S->key_bits, 0, &in_other, NULL)) return 1;
        if (in_other) src = S->sorted_other;
    }
    S->sorted = NULL;                                       /* (one use: the next point brings its own) */
    uint64_t *const d_uk = (uint64_t *)S->buf.rows.p; uint32_t *const d_nc = (uint32_t *)(d_uk + N);
    const res_cellsum_v cs = res_cellsum_layout(S->buf.cellsum.p, S->n_cells);
    uint64_t bits = 0;
    if (fastf_dev_umi_rows(e, src, sm + SM_KEYS, N, d_uk, d_nc, sm + SM_UROWS, NULL) ||
        fastf_dev_copy_summary(e, d_uk, d_nc, sm + SM_UROWS, S->n_cells, cs.rpc, cs.npc, cs.spc, cs.hist, NULL) ||
        fastf_dev_error_bits(e, &bits)) return 1;
    if (bits) return fastf_res_err("%s: device error bits 0x%llx in the per-cell stage of point %s", S->verb, (unsigned long long)bits, point_name);
    if (fastf_devmem_copy(S->h_cs.hist, cs.hist, cs.bytes)) return 1;
    T->cells_dev += fastf_res_now() - tt;
    return 0;
}

/* ------------------------------------------------------------------ */
/* replicate seeds: the lists, the names, the rows                     */
/* ------------------------------------------------------------------ */
int fastf_parse_seeds(const char *text, uint32_t *out, uint32_t cap, uint32_t *n_out)
{
    uint32_t n = 0;
    if (n_out) *n_out = 0;
    if (!text || !out || !n_out) return fastf_res_err("null argument");
    if (cap > FASTF_MAX_SEEDS) cap = FASTF_MAX_SEEDS;
    for (const char *p = text;;) {
        const char *q = p;
        while (*q && *q != ',') q++;
        char el[64];
        const size_t len = (size_t)(q - p);
        if (len == 0) return fastf_res_err("--seeds `%s`: empty element", text);
        if (len >= sizeof el) return fastf_res_err("--seeds `%s`: element too long", text);
        memcpy(el, p, len); el[len] = '\0';
        char *end = NULL;
        errno = 0;
        const uint32_t v = (uint32_t)(unsigned int)strtol(el, &end, 0);      /* (the rule of -s) */
        if (errno == ERANGE) return fastf_res_err("--seeds `%s`: numerical result out of range", el);
        if (end == el || *end) return fastf_res_err("--seeds `%s`: expects an integer value", el);
        for (uint32_t j = 0; j < n; j++) if (out[j] == v) return fastf_res_err("--seeds `%s`: %u is listed twice", text, v);
        if (n == cap) return fastf_res_err("--seeds `%s`: more than %u values", text, cap);
        out[n++] = v;
        if (!*q) break;
        p = q + 1;
    }
    *n_out = n;
    return 0;
}

int fastf_reps_seeds(uint32_t first, uint64_t n_reps, uint32_t *out, uint32_t cap, uint32_t *n_out)
{
    if (n_out) *n_out = 0;
    if (!out || !n_out) return fastf_res_err("null argument");
    if (n_reps < 1 || n_reps > FASTF_MAX_SEEDS || n_reps > cap) return fastf_res_err("--reps %llu: expects 1 to %u replicates", (unsigned long long)n_reps, cap < FASTF_MAX_SEEDS ? cap : FASTF_MAX_SEEDS);
    if ((uint64_t)first + n_reps - 1 > 0xFFFFFFFFull)
        return fastf_res_err("--reps %llu from seed %u: the seeds would wrap past 4294967295", (unsigned long long)n_reps, first);
    for (uint32_t k = 0; k < (uint32_t)n_reps; k++) out[k] = first + k;
    *n_out = (uint32_t)n_reps;
    return 0;
}

int fastf_reps_point_dir(const char *point_name, uint32_t seed, char *buf, size_t cap)
{
    if (!point_name || !buf) return fastf_res_err("null argument");
    const int n = snprintf(buf, cap, "%s_s%u", point_name, seed);
    return (n < 0 || (size_t)n >= cap) ? fastf_res_err("directory name too long") : 0;
}

/* `\t mean \t sd \t min \t max` of v[0], v[stride], ..: two passes in list order, the sample sd; kind 0: integers, 1: %.6f, 2: %.1f */
static int reps_stat4(const double *v, uint32_t stride, uint32_t n, int kind, char *buf, size_t cap)
{
    double sum = 0.0, ss = 0.0, lo = v[0], hi = v[0];
    for (uint32_t k = 0; k < n; k++) { const double x = v[(size_t)k * stride]; sum += x; if (x < lo) lo = x; if (x > hi) hi = x; }
    const double mean = sum / (double)n;
    for (uint32_t k = 0; k < n; k++) { const double d = v[(size_t)k * stride] - mean; ss += d * d; }
    char sd[40], a[40], b[40];
    if (n > 1) snprintf(sd, sizeof sd, "%.6f", sqrt(ss / (double)(n - 1))); else snprintf(sd, sizeof sd, "NA");
    if (kind == 0) { snprintf(a, sizeof a, "%llu", (unsigned long long)lo); snprintf(b, sizeof b, "%llu", (unsigned long long)hi); }
    else if (kind == 1) { snprintf(a, sizeof a, "%.6f", lo); snprintf(b, sizeof b, "%.6f", hi); }
    else { snprintf(a, sizeof a, "%.1f", lo); snprintf(b, sizeof b, "%.1f", hi); }
    const int w = snprintf(buf, cap, "\t%.6f\t%s\t%s\t%s", mean, sd, a, b);
    return (w < 0 || (size_t)w >= cap) ? -1 : w;
}
static int reps_row_head(float rate_cell, float rate_depth, uint64_t reads_per_cell, uint32_t n_reps, char *buf, size_t cap)
{
    char second[32];
    if (reads_per_cell) snprintf(second, sizeof second, "%llu", (unsigned long long)reads_per_cell);
    else snprintf(second, sizeof second, "%.3f", (double)rate_depth);
    const int w = snprintf(buf, cap, "%.3f\t%s\t%u", (double)rate_cell, second, n_reps);
    return (w < 0 || (size_t)w >= cap) ? -1 : w;
}

int fastf_reps_summary_row(float rate_cell, float rate_depth, uint64_t reads_per_cell, uint32_t n_cells, const double *metrics, uint32_t n_reps,
                           char *buf, size_t cap)
{
    static const int kind[FASTF_REPS_METRICS] = {0, 0, 0, 0, 1, 2, 2};
    if (!buf || !metrics) return fastf_res_err("null argument");
    if (n_reps < 1 || n_reps > FASTF_MAX_SEEDS) return fastf_res_err("a replicate row takes 1 to %u replicates", FASTF_MAX_SEEDS);
    int n = reps_row_head(rate_cell, rate_depth, reads_per_cell, n_reps, buf, cap);
    if (n >= 0) { const int w = snprintf(buf + n, cap - (size_t)n, "\t%u", n_cells); n = (w < 0 || (size_t)w >= cap - (size_t)n) ? -1 : n + w; }
    for (uint32_t m = 0; m < FASTF_REPS_METRICS && n >= 0; m++) {
        const int w = reps_stat4(metrics + m, FASTF_REPS_METRICS, n_reps, kind[m], buf + n, cap - (size_t)n);
        n = w < 0 ? -1 : n + w;
    }
    if (n < 0 || (size_t)n + 1 >= cap) return fastf_res_err("summary row too long");
    buf[n] = '\n'; buf[n + 1] = '\0';
    return 0;
}

int fastf_genes_reps_row(float rate_cell, float rate_depth, uint64_t reads_per_cell, const uint32_t *genes_detected, uint32_t n_reps,
                         const uint64_t *reps_detected, uint32_t n_features, char *buf, size_t cap)
{
    if (!buf || !genes_detected || (n_features && !reps_detected)) return fastf_res_err("null argument");
    if (n_reps < 1 || n_reps > FASTF_MAX_SEEDS) return fastf_res_err("a replicate row takes 1 to %u replicates", FASTF_MAX_SEEDS);
    double v[FASTF_MAX_SEEDS];
    for (uint32_t k = 0; k < n_reps; k++) v[k] = (double)genes_detected[k];
    uint32_t all = 0, any = 0;
    for (uint32_t g = 0; g < n_features; g++) { all += reps_detected[g] == n_reps; any += reps_detected[g] >= 1; }
    int n = reps_row_head(rate_cell, rate_depth, reads_per_cell, n_reps, buf, cap);
    if (n >= 0) { const int w = reps_stat4(v, 1, n_reps, 0, buf + n, cap - (size_t)n); n = w < 0 ? -1 : n + w; }
    if (n >= 0) { const int w = snprintf(buf + n, cap - (size_t)n, "\t%u\t%u\n", all, any); n = (w < 0 || (size_t)w >= cap - (size_t)n) ? -1 : n + w; }
    return n < 0 ? fastf_res_err("summary row too long") : 0;
}

int fastf_gene_reps_add_host(const uint32_t *cells_per_gene, uint32_t n_features, uint64_t *detected, uint64_t *sum, uint64_t *sumsq)
{
    if (n_features && (!cells_per_gene || !detected || !sum || !sumsq)) return fastf_res_err("null argument");
    for (uint32_t g = 0; g < n_features; g++) {
        const uint64_t c = cells_per_gene[g];
        detected[g] += c != 0; sum[g] += c; sumsq[g] += c * c;
    }
    return 0;
}

/* ------------------------------------------------------------------ */
/* replicate runs: the tables of a run                                 */
/* ------------------------------------------------------------------ */
static void reps_release(res_reps_t *P)
{
    if (P->feat_id) for (uint32_t i = 0; i < P->n_features; i++) free(P->feat_id[i]);
    free(P->feat_id); free(P->m); free(P->n_cells); free(P->gdet); free(P->seen); free(P->h_acc);
    fastf_devmem_free(P->d_acc);
    P->feat_id = NULL; P->m = NULL; P->n_cells = P->gdet = NULL; P->seen = NULL; P->h_acc = NULL; P->d_acc = NULL; P->n_features = 0;
}

int fastf_res_reps_open(res_reps_t *P, int on, const res_verb_t *V, const char *out_dir, const uint32_t *seeds, uint32_t n_seeds, uint32_t n_rates,
                        uint32_t n_list, int genes, int device)
{
    memset(P, 0, sizeof *P);
    if (!on) return 0;
    P->verb = V->name; P->seeds = seeds; P->n_seeds = n_seeds; P->n_rates = n_rates; P->n_list = n_list; P->genes = genes; P->device = device;
    snprintf(P->out_dir, sizeof P->out_dir, "%s", out_dir);
    const size_t cells = (size_t)n_list * n_seeds;
    if (!(P->m = (double *)calloc(cells * FASTF_REPS_METRICS, sizeof *P->m)) || !(P->n_cells = (uint32_t *)calloc(cells, sizeof *P->n_cells)) ||
        !(P->gdet = (uint32_t *)calloc(cells, sizeof *P->gdet)) || !(P->seen = (uint8_t *)calloc(cells, 1))) { reps_release(P); return fastf_res_err("out of memory"); }
    if (fastf_res_table_open(&P->tsv, V, out_dir, TB_REPS)) { reps_release(P); return 1; }
    if (genes && fastf_res_table_open(&P->gtsv, V, out_dir, TB_GENES_REPS)) { fastf_res_tsv_close(&P->tsv, 0); reps_release(P); return 1; }
    P->on = 1;
    return 0;
}

int fastf_res_reps_rate_begin(res_reps_t *P, const fastf_lists_t *L, int on_device)
{
    if (!P->on) return 0;
    const size_t cells = (size_t)P->n_list * P->n_seeds;
    memset(P->seen, 0, cells);
    if (!P->genes) return 0;
    const uint32_t nf = (uint32_t)L->n_features;
    if (!P->feat_id) {                                      /* the first cell rate: the names, the room of the accumulators */
        if (!(P->feat_id = (char **)calloc(nf ? nf : 1, sizeof *P->feat_id)) ||
            !(P->h_acc = (uint64_t *)calloc((size_t)P->n_rates * P->n_list * 3 * nf + 1, sizeof *P->h_acc))) return fastf_res_err("out of memory");
        for (uint32_t i = 0; i < nf; i++) { if (!(P->feat_id[i] = strdup(L->feat_id[i]))) return fastf_res_err("out of memory"); P->n_features = i + 1; }
    }
    if (nf != P->n_features) return fastf_res_err("internal error: the feature list changed between cell rates");
    const size_t bytes = (size_t)P->n_list * 3 * nf * 8;
    if (on_device && nf) {
        if (!P->d_acc && !(P->d_acc = fastf_devmem_alloc(P->device, bytes)))
            return fastf_res_err("%s: the per-gene accumulators of the replicates do not fit: %zu bytes (%s)", P->verb, bytes, fastf_last_error());
        if (fastf_devmem_zero(P->d_acc, bytes)) return 1;
    }
    return 0;
}

int fastf_res_reps_point(res_reps_t *P, uint32_t j, uint32_t k, uint32_t n_cells, const double *metrics)
{
    if (!P->on) return 0;
    if (j >= P->n_list || k >= P->n_seeds) return fastf_res_err("internal error: replicate (%u, %u) outside the grid", j, k);
    const size_t at = (size_t)j * P->n_seeds + k;
    memcpy(P->m + at * FASTF_REPS_METRICS, metrics, FASTF_REPS_METRICS * sizeof *metrics);
    P->n_cells[at] = n_cells; P->seen[at] = 1;
    return 0;
}

int fastf_res_reps_genes(res_reps_t *P, res_rate_t *S, uint32_t j, uint32_t k, const uint32_t *cells_per_gene, uint32_t n_features)
{
    if (!P->on || !P->genes) return 0;
    if (j >= P->n_list || k >= P->n_seeds || P->rate_at >= P->n_rates) return fastf_res_err("internal error: replicate (%u, %u) outside the grid", j, k);
    if (n_features != P->n_features) return fastf_res_err("internal error: the feature list changed between points");
    const uint32_t nf = P->n_features;
    uint32_t d1 = 0;
    for (uint32_t g = 0; g < nf; g++) d1 += cells_per_gene[g] >= 1;
    P->gdet[(size_t)j * P->n_seeds + k] = d1;
    if (S) {                                                /* the device's copy of the same array, behind the point's gene summary */
        if (!nf) return 0;
        if (!P->d_acc) return fastf_res_err("internal error: no per-gene accumulators on the device");
        uint64_t *const a = (uint64_t *)P->d_acc + (size_t)j * 3 * nf;
        return fastf_dev_gene_reps_add(S->e, S->buf.cpg.u32, nf, a, a + nf, a + 2 * (size_t)nf, NULL);
    }
    uint64_t *const a = P->h_acc + ((size_t)P->rate_at * P->n_list + j) * 3 * nf;
    return fastf_gene_reps_add_host(cells_per_gene, nf, a, a + nf, a + 2 * (size_t)nf);
}

int fastf_res_reps_rate_end(res_reps_t *P, float rate_cell, const float *rates_depth, const uint64_t *caps, res_times_t *T)
{
    if (!P->on) return 0;
    const double t0 = fastf_res_now();
    if (P->rate_at >= P->n_rates) return fastf_res_err("internal error: more cell rates than the grid has");
    const uint32_t nf = P->n_features;
    for (uint32_t j = 0; j < P->n_list; j++) {
        const size_t at = (size_t)j * P->n_seeds;
        char row[1536];
        for (uint32_t k = 0; k < P->n_seeds; k++) {
            if (!P->seen[at + k]) return fastf_res_err("internal error: replicate (%u, %u) was not run", j, k);
            if (P->n_cells[at + k] != P->n_cells[at])
                return fastf_res_err("%s: cell rate %.3f sampled %u cells at seed %u and %u at seed %u: the sample size depends on the rate alone", P->verb,
                              (double)rate_cell, P->n_cells[at], P->seeds[0], P->n_cells[at + k], P->seeds[k]);
        }
        const float rd = rates_depth ? rates_depth[j] : 0.0f;
        const uint64_t n = caps ? caps[j] : 0;
        if (fastf_reps_summary_row(rate_cell, rd, n, P->n_cells[at], P->m + at * FASTF_REPS_METRICS, P->n_seeds, row, sizeof row)) return 1;
        fputs(row, P->tsv.f);
        if (P->genes) {
            uint64_t *const a = P->h_acc + ((size_t)P->rate_at * P->n_list + j) * 3 * nf;
            /* the three accumulators of the grid point come to the host once, after its last seed */
            if (P->d_acc && nf && fastf_devmem_copy(a, (const uint64_t *)P->d_acc + (size_t)j * 3 * nf, (size_t)3 * nf * 8)) return 1;
            if (fastf_genes_reps_row(rate_cell, rd, n, P->gdet + at, P->n_seeds, a, nf, row, sizeof row)) return 1;
            fputs(row, P->gtsv.f);
        }
    }
    P->rate_at++;
    if (T) T->reps += fastf_res_now() - t0;
    return 0;
}

/* <out_dir>/<verb>_gene_reps.tsv.gz: per feature and grid point the three accumulators */
static int reps_gene_file(const res_reps_t *P, const float *rates_cell, const float *rates_depth, const uint64_t *caps)
{
    char file[64];
    gtext t = { NULL, 0, 0 };
    const uint32_t nf = P->n_features, np = P->n_rates * P->n_list;
    static const char *const col[3] = {":reps_detected", ":cells_sum", ":cells_sumsq"};
    int bad = fastf_gt_str(&t, "feature");
    for (uint32_t p = 0; p < np && !bad; p++) {
        char name[64];
        const uint32_t i = p / P->n_list, j = p % P->n_list;
        bad = caps ? (!strcmp(P->verb, "level") ? fastf_level_point_dir : fastf_cap_point_dir)(rates_cell[i], caps[j], name, sizeof name) : fastf_sweep_point_dir(rates_cell[i], rates_depth[j], name, sizeof name);
        for (int c = 0; c < 3 && !bad; c++) bad = fastf_gt_str(&t, "\t") || fastf_gt_str(&t, name) || fastf_gt_str(&t, col[c]);
    }
    if (!bad) bad = fastf_gt_str(&t, "\n");
    for (uint32_t g = 0; g < nf && !bad; g++) {
        bad = fastf_gt_str(&t, P->feat_id[g]);
        for (uint32_t p = 0; p < np && !bad; p++)
            for (int c = 0; c < 3 && !bad; c++) bad = fastf_gt_u64(&t, '\t', P->h_acc[((size_t)p * 3 + (size_t)c) * nf + g]);
        if (!bad) bad = fastf_gt_str(&t, "\n");
    }
    snprintf(file, sizeof file, "%s_gene_reps.tsv.gz", P->verb);
    return fastf_res_text_file(P->out_dir, file, &t, bad);
}

/* ok: the per-gene file (its columns named from the grid: rates_cell and ONE of rates_depth / caps), then the tables; otherwise
 * nothing of either is left */
int fastf_res_reps_close_grid(res_reps_t *P, int ok, const float *rates_cell, const float *rates_depth, const uint64_t *caps)
{
    if (!P->on) return 0;
    int rc = 0;
    if (ok && P->rate_at != P->n_rates) rc = fastf_res_err("internal error: %u of %u cell rates were closed", P->rate_at, P->n_rates);
    if (ok && !rc && P->genes) rc = reps_gene_file(P, rates_cell, rates_depth, caps);
    char keep[512]; snprintf(keep, sizeof keep, "%s", fastf_last_error());
    const int bad = rc;
    if (fastf_res_tsv_close(&P->tsv, ok && !rc)) rc = 1;
    if (P->genes && fastf_res_tsv_close(&P->gtsv, ok && !rc)) rc = 1;
    if (bad) fastf_set_error_(keep);
    reps_release(P);
    P->on = 0;
    return rc;
}
int fastf_res_reps_close(res_reps_t *P, int ok) { return fastf_res_reps_close_grid(P, ok, NULL, NULL, NULL); }

uint32_t fastf_res_lists_max_cells(const res_lists_t *l)
{
    size_t m = 0;
    for (uint32_t i = 0; i < l->n; i++) if (l->L[i].n_cells > m) m = l->L[i].n_cells;
    return (uint32_t)m;
}

/* ------------------------------------------------------------------ */
/* the command line                                                    */
/* ------------------------------------------------------------------ */
/* the help text of the three verbs: %1$s the verb, %2$s D->help_resident, %3$s D->help_point, %4$s D->help_intro, %5$s D->help_list */
static void fastf_res_usage(const char *verb, const res_cmd_t *D, FILE *f)
{
    fprintf(f,
            "Usage: fastF %1$s [options]\n\n"
            "%4$s\n\n"
            "    -h, --help            show this help message and exit\n"
            "    -b, --bam=<str>       path to bam file\n"
            "    -f, --feature=<str>   path to feature list file\n"
            "    -a, --barcode=<str>   path to barcode list file\n"
            "    -d, --dbname=<str>    name of database (accepted for compatibility, ignored)\n"
            "    -c, --cell=<list>     rates of cell barcode, comma separated (default 1.0)\n"
            "    %5$s\n"
            "    -o, --out=<str>       path to output directory (default .)\n"
            "    -s, --seed=<int>      seed for random number generator (default 926)\n"
            "        --summary-only    write %1$s.tsv alone\n"
            "        --genes           per-gene detection too: %1$s_genes.tsv, %1$s_gene_cells.tsv.gz and genes.tsv.gz per point\n"
            "        --cells           per-cell reads, saturation and UMI copy numbers too: %1$s_cells.tsv and cells.tsv.gz per point\n"
            "        --fidelity        every point against the full-depth data of the same cells (every read of the sampled cells kept):\n"
            "                          %1$s_fidelity.tsv and fidelity.tsv.gz per point, with the Pearson and the cosine of the RAW counts\n"
            "                          over ALL genes per cell (not log-normalised)%2$s\n"
            "        --gene-fidelity   every point against the full-depth data of the same cells, per GENE: %1$s_gene_fidelity.tsv and\n"
            "                          gene_fidelity.tsv.gz per point, with the Pearson of the RAW counts over ALL sampled cells per gene,\n"
            "                          the dispersion (variance / mean) at full depth and at the point, and the overlap of the 2000\n"
            "                          most variable genes%2$s\n"
            "        --neighbors       every point against the full-depth data of the same cells, BETWEEN the cells: %1$s_neighbors.tsv and\n"
            "                          neighbors.tsv.gz per point, with the share of a cell's 15 nearest neighbours at full depth (cosine of\n"
            "                          the RAW counts over the 2000 most variable genes, decided in exact integers) that it keeps%2$s\n"
            "        --coexpression    every point against the full-depth data of the same cells, BETWEEN the genes: %1$s_coexpr.tsv and\n"
            "                          coexpr.tsv.gz per point, with the share of a gene's 15 strongest co-expression partners at full depth\n"
            "                          (Pearson of the RAW counts among the 2000 most variable genes, decided in exact integers) that it keeps%2$s\n"
            "        --labels=<file>   one `barcode<TAB>label` per line (cell types of the full-depth analysis): %1$s_labels.tsv,\n"
            "                          %1$s_label_classes.tsv and labels.tsv.gz, label_confusion.tsv.gz per point, with the share of labelled\n"
            "                          cells whose 15 nearest neighbours still vote for their own label, at full depth and at the point%2$s\n"
            "        --markers=<N>     with --labels: per label the N (1 to 2000) best marker genes among the 2000 most variable, ranked by the\n"
            "                          exact AUC of the label's cells against the other labelled cells, at full depth and at the point:\n"
            "                          %1$s_markers.tsv and markers.tsv.gz per point%2$s\n"
            "        --mapping         every cell of a point looked up among ALL full-depth cells of the same sample (cosine of the RAW counts over\n"
            "                          the 2000 most variable genes, decided in exact integers): %1$s_mapping.tsv and mapping.tsv.gz per point, with\n"
            "                          the rank of the cell's own full-depth profile, the share of its 15 nearest full-depth cells that are its\n"
            "                          full-depth neighbours and, with --labels, the label they vote for%2$s\n"
            "        --pseudotime=<file>\n"
            "                          one `barcode<TAB>value` per line (a pseudotime or any per-cell score of the full-depth analysis): %1$s_pseudotime.tsv\n"
            "                          and pseudotime.tsv.gz per point, with the value's rank estimated back per cell as the lower median over its 15\n"
            "                          nearest neighbours, at full depth, at the point and, with --mapping, over the full-depth cells it maps among, and\n"
            "                          Kendall's tau-b of the estimate against the value over all pairs of cells, counted exactly%2$s\n"
            "        --seeds=<list>    replicates: the grid at each of 1 to 64 seeds, comma separated, from the one decode; per point and\n"
            "                          seed <out>/c<cell>_%3$s_s<seed>/, one %1$s.tsv row each, and %1$s_reps.tsv with mean, sd, min and max\n"
            "                          of every metric per grid point (with --genes %1$s_genes_reps.tsv and %1$s_gene_reps.tsv.gz in\n"
            "                          place of %1$s_gene_cells.tsv.gz); not with -s or --reps\n"
            "        --reps=<int>      the same at the seeds s, s + 1, .. s + N - 1 (s: -s; N from 1 to 64)\n",
            verb, D->help_resident, D->help_point, D->help_intro, D->help_list);
}

/* returns 0, 1 after an error message, 2 after the help text; -u prints D->u_message and fails */
static int fastf_res_parse_args(int argc, const char **argv, const char *verb, const res_cmd_t *D, res_args_t *out)
{
    /* the options from O_SUMMARY_ONLY on have no short form */
    enum { O_HELP, O_BAM, O_FEATURE, O_BARCODE, O_DBNAME, O_CELL, O_LIST, O_OUT, O_SEED, O_UMICOPIES, O_SUMMARY_ONLY, O_GENES, O_CELLS, O_FIDELITY, O_GENE_FIDELITY,
           O_NEIGHBORS, O_COEXPRESSION, O_MAPPING, O_PSEUDOTIME, O_LABELS, O_MARKERS, O_SEEDS, O_REPS };
    const cli_opt opts[] = {
        {'h', "help", 0}, {'b', "bam", 1}, {'f', "feature", 1}, {'a', "barcode", 1}, {'d', "dbname", 1}, {'c', "cell", 1}, {D->list_short, D->list_long, 1},
        {'o', "out", 1}, {'s', "seed", 1}, {'u', "umicopies", 0}, {0, "summary-only", 0}, {0, "genes", 0}, {0, "cells", 0}, {0, "fidelity", 0}, {0, "gene-fidelity", 0},
        {0, "neighbors", 0}, {0, "coexpression", 0}, {0, "mapping", 0}, {0, "pseudotime", 1}, {0, "labels", 1}, {0, "markers", 1}, {0, "seeds", 1}, {0, "reps", 1}, {0, NULL, 0}};
    const char *seeds_text = NULL, *reps_text = NULL, *markers_text = NULL;
    int have_s = 0;
    out->n_seeds = 0;
    out->bam = out->feat = out->bar = out->list = NULL; out->out = "."; out->cells = "1"; out->seed = 926; out->summary_only = 0; out->genes = 0; out->per_cell = 0; out->fidelity = 0; out->gene_fidelity = 0; out->neighbors = 0; out->coexpression = 0; out->mapping = 0; out->labels = NULL; out->pseudotime = NULL; out->markers = 0;
    cli_scan S = CLI_SCAN(argc, argv, opts, 0);
    for (const cli_opt *o; (o = cli_next(&S));)
        switch (o - opts) {
        case O_HELP: fastf_res_usage(verb, D, stdout); return 2;
        case O_BAM: out->bam = S.val; break;
        case O_FEATURE: out->feat = S.val; break;
        case O_BARCODE: out->bar = S.val; break;
        case O_DBNAME: break;
        case O_CELL: out->cells = S.val; break;
        case O_LIST: out->list = S.val; break;
        case O_OUT: out->out = S.val; break;
        case O_SEED: have_s = 1; out->seed = (unsigned int)cli_int(&S); break;
        case O_UMICOPIES: fprintf(stderr, "\x1b[31mError:\x1b[0m %s\n", D->u_message); return 1;
        case O_SUMMARY_ONLY: out->summary_only = 1; break;
        case O_GENES: out->genes = 1; break;
        case O_CELLS: out->per_cell = 1; break;
        case O_FIDELITY: out->fidelity = 1; break;
        case O_GENE_FIDELITY: out->gene_fidelity = 1; break;
        case O_NEIGHBORS: out->neighbors = 1; break;
        case O_COEXPRESSION: out->coexpression = 1; break;
        case O_MAPPING: out->mapping = 1; break;
        case O_PSEUDOTIME: out->pseudotime = S.val; break;
        case O_LABELS: out->labels = S.val; break;
        case O_MARKERS: markers_text = S.val; break;
        case O_SEEDS: seeds_text = S.val; break;
        case O_REPS: reps_text = S.val; break;
        }
    if (S.err) { if (S.err == CLI_UNKNOWN) fastf_res_usage(verb, D, stderr); return 1; }
    if (markers_text) {                                     /* (refused here: before the verb makes its output directory) */
        char *end = NULL;
        errno = 0;
        const long n = strtol(markers_text, &end, 10);
        if (errno == ERANGE || end == markers_text || *end || n < 1 || n > (long)FASTF_MARKERS_MAX) {
            fprintf(stderr, "error: option `--markers` expects an integer from 1 to %u\n", FASTF_MARKERS_MAX);
            return 1;
        }
        if (!out->labels) { fprintf(stderr, "error: option `--markers` needs `--labels`\n"); return 1; }
        out->markers = (uint32_t)n;
    }
    /* replicates: --seeds lists them, --reps counts them up from -s */
    if (seeds_text && reps_text) { fprintf(stderr, "error: option `--seeds` cannot be combined with `--reps`\n"); return 1; }
    if (seeds_text && have_s) { fprintf(stderr, "error: option `--seeds` cannot be combined with `-s`\n"); return 1; }
    if (seeds_text && fastf_parse_seeds(seeds_text, out->seeds, FASTF_MAX_SEEDS, &out->n_seeds)) { fprintf(stderr, "error: option %s\n", fastf_last_error()); return 1; }
    if (reps_text) {
        char *end = NULL;
        errno = 0;
        const long n = strtol(reps_text, &end, 0);
        if (errno == ERANGE || end == reps_text || *end || n < 1 || n > (long)FASTF_MAX_SEEDS) {
            fprintf(stderr, "error: option `--reps` expects an integer from 1 to %u\n", FASTF_MAX_SEEDS);
            return 1;
        }
        if (fastf_reps_seeds(out->seed, (uint64_t)n, out->seeds, FASTF_MAX_SEEDS, &out->n_seeds)) { fprintf(stderr, "error: option %s\n", fastf_last_error()); return 1; }
    }
    return 0;
}
/* the three input files exist (after the lists are parsed: the order of the messages of the commands) */
static int fastf_res_check_inputs(const res_args_t *a)
{
    if (!a->bam || access(a->bam, F_OK) == -1) { fprintf(stderr, "\x1b[31mError:\x1b[0m bam file: %s does not exist.\n", a->bam ? a->bam : "(null)"); return 1; }
    if (!a->feat || access(a->feat, F_OK) == -1) { fprintf(stderr, "\x1b[31mError:\x1b[0m feature file: %s does not exist.\n", a->feat ? a->feat : "(null)"); return 1; }
    if (!a->bar || access(a->bar, F_OK) == -1) { fprintf(stderr, "\x1b[31mError:\x1b[0m barcode file: %s does not exist.\n", a->bar ? a->bar : "(null)"); return 1; }
    return 0;
}

_Static_assert(FASTF_CAP_SUMMARY_ONLY == FASTF_SWEEP_SUMMARY_ONLY && FASTF_LEVEL_SUMMARY_ONLY == FASTF_SWEEP_SUMMARY_ONLY && FASTF_CAP_GENES == FASTF_SWEEP_GENES &&
               FASTF_LEVEL_GENES == FASTF_SWEEP_GENES && FASTF_CAP_CELLS == FASTF_SWEEP_CELLS && FASTF_LEVEL_CELLS == FASTF_SWEEP_CELLS &&
               FASTF_CAP_FIDELITY == FASTF_SWEEP_FIDELITY && FASTF_LEVEL_FIDELITY == FASTF_SWEEP_FIDELITY && FASTF_CAP_GENE_FIDELITY == FASTF_SWEEP_GENE_FIDELITY &&
               FASTF_LEVEL_GENE_FIDELITY == FASTF_SWEEP_GENE_FIDELITY && FASTF_CAP_NEIGHBORS == FASTF_SWEEP_NEIGHBORS && FASTF_LEVEL_NEIGHBORS == FASTF_SWEEP_NEIGHBORS &&
               FASTF_CAP_COEXPRESSION == FASTF_SWEEP_COEXPRESSION && FASTF_LEVEL_COEXPRESSION == FASTF_SWEEP_COEXPRESSION,
               "the three verbs share one flag word");
/* the flag word of the options (the bits of FASTF_SWEEP_*, which FASTF_CAP_* and FASTF_LEVEL_* repeat) */
static uint32_t fastf_res_args_flags(const res_args_t *a)
{
    return (a->summary_only ? FASTF_SWEEP_SUMMARY_ONLY : 0) | (a->genes ? FASTF_SWEEP_GENES : 0) | (a->per_cell ? FASTF_SWEEP_CELLS : 0) | (a->fidelity ? FASTF_SWEEP_FIDELITY : 0) |
           (a->gene_fidelity ? FASTF_SWEEP_GENE_FIDELITY : 0) | (a->neighbors ? FASTF_SWEEP_NEIGHBORS : 0) | (a->coexpression ? FASTF_SWEEP_COEXPRESSION : 0);
}

/* the "... is generated." lines of a run that succeeded */
static void fastf_res_print_generated(const char *verb, const res_args_t *a)
{
    if (a->genes && a->n_seeds) printf("%s_genes.tsv, %s_genes_reps.tsv and %s_gene_reps.tsv.gz are generated.\n", verb, verb, verb);
    else if (a->genes) printf("%s_genes.tsv and %s_gene_cells.tsv.gz are generated.\n", verb, verb);
    if (a->per_cell) printf("%s_cells.tsv is generated.\n", verb);
    if (a->fidelity) printf("%s_fidelity.tsv is generated.\n", verb);
    if (a->gene_fidelity) printf("%s_gene_fidelity.tsv is generated.\n", verb);
    if (a->neighbors) printf("%s_neighbors.tsv is generated.\n", verb);
    if (a->labels) printf("%s_labels.tsv and %s_label_classes.tsv are generated.\n", verb, verb);
    if (a->markers) printf("%s_markers.tsv is generated.\n", verb);
    if (a->coexpression) printf("%s_coexpr.tsv is generated.\n", verb);
    if (a->mapping) printf("%s_mapping.tsv is generated.\n", verb);
    if (a->pseudotime) printf("%s_pseudotime.tsv is generated.\n", verb);
    if (a->n_seeds) printf("%s_reps.tsv is generated.\n", verb);
    printf("%s.tsv is generated.\n", verb);
}

/* the command of a verb.  The ONE call below is the most general of a verb's six: the parser hands on markers only from 1 to
 * FASTF_MARKERS_MAX and with labels, and mapping only as 0 or 1, so each narrower call it could name does the same */
#define RES_MAX_POINTS 64
int fastf_res_cmd(const res_verb_t *V, const res_cmd_t *D, int argc, const char **argv)
{
    res_args_t A;
    const int prc = fastf_res_parse_args(argc, argv, V->name, D, &A);
    if (prc) return prc == 2 ? 0 : 1;
    const char *list = A.list ? A.list : D->list_default;
    float rc[RES_MAX_POINTS], rd[RES_MAX_POINTS]; uint64_t caps[RES_MAX_POINTS];
    uint32_t n_c = 0, n = 0;
    if (!list) { fprintf(stderr, "\x1b[31mError:\x1b[0m %s\n", D->needs_list); return 1; }
    if (fastf_sweep_parse_rates(A.cells, 1, rc, RES_MAX_POINTS, &n_c) ||
        (D->parse_caps ? D->parse_caps(list, caps, RES_MAX_POINTS, &n) : fastf_sweep_parse_rates(list, 0, rd, RES_MAX_POINTS, &n)) ||
        (V->check_caps ? V->check_caps(rc, n_c, caps, n) : fastf_sweep_check_grid(rc, n_c, rd, n))) {
        fprintf(stderr, "\x1b[31mError:\x1b[0m %s\n", fastf_last_error());
        return 1;
    }
    if (fastf_res_check_inputs(&A)) return 1;
    if (fastf_res_grid_entry(V, 0, A.bam, A.out, A.bar, A.feat, rc, n_c, D->parse_caps ? NULL : rd, D->parse_caps ? caps : NULL, n, A.seeds, A.n_seeds, A.seed,
                             fastf_res_args_flags(&A), A.labels, A.markers, (uint32_t)A.mapping, A.pseudotime)) {
        fprintf(stderr, "\x1b[31mError:\x1b[0m %s failed: %s\n", V->name, fastf_last_error());
        return 1;
    }
    fastf_res_print_generated(V->name, &A);
    return 0;
}
