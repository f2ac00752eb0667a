/*
 * sweep_cmds.c — `fastF sweep`: bam2db over a grid of (cell rate, depth rate) points from ONE decode of the BAM.
 *
 *   cmd_sweep()    -b -a -f -o -c <list> -r <list> [-s seed] [--summary-only]; -d accepted and ignored, -u refused
 *   fastf_sweep()  the same in process
 * Per point <out>/c<rate_cell>_r<rate_depth>/{matrix.mtx.gz, barcodes.tsv.gz, features.tsv.gz} — the bytes `fastF bam2db`
 * writes for that point — and one row of <out>/sweep.tsv.
 *
 * Resident form: the packed records (24 bytes each) stay in device memory.  Per cell rate one engine, the records in its
 * layout, K1a once; the draw stream generated once and compared against every depth threshold in the same pass
 * (fastf_dev_mt_decisions_multi); per depth rate K1b on that point's decision plane, sort, reduce, the per-cell summary
 * (fastf_dev_cell_summary), and — unless --summary-only — the rows gathered into pinned memory for the writers of bam2db.
 * Jobs this form does not cover (keys wider than 64 bits, UMIs beyond 16 bases, several devices) run point by point
 * through bam2db() itself, the summary then read back from each point's matrix.
 */
#define _GNU_SOURCE
#include "host_io.h"

#include <errno.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

/* device memory for this file (umi_engine.hip) */
void *fastf_devmem_alloc(int device, size_t bytes);
void  fastf_devmem_free(void *p);
int   fastf_devmem_copy(void *dst, const void *src, size_t bytes);
int   fastf_devmem_zero(void *dst, size_t bytes);
int   fastf_devmem_sync(void);

static double now_s(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + t.tv_nsec * 1e-9; }
static int sw_err(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static int sw_err(const char *fmt, ...)
{
    char buf[480];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    fastf_set_error_(buf);
    return 1;
}

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
    if (!text || !out || !n_out) return sw_err("null argument");
    for (const char *p = text;;) {
        const char *q = p;
        while (*q && *q != ',') q++;
        char el[64];
        const size_t len = (size_t)(q - p);
        if (len == 0) return sw_err("%s rates `%s`: empty element", what, text);
        if (len >= sizeof el) return sw_err("%s rates `%s`: element too long", what, text);
        memcpy(el, p, len); el[len] = '\0';
        char *end = NULL;
        errno = 0;
        const float v = strtof(el, &end);
        if (errno == ERANGE) return sw_err("%s rate `%s`: numerical result out of range", what, el);
        if (end == el || *end) return sw_err("%s rate `%s`: expects a numerical value", what, el);
        if (isnan(v)) return sw_err("%s rate `%s`: not a number", what, el);
        if (v < 0 || signbit(v)) return sw_err("%s rate `%s`: negative", what, el);
        if (cell_rates && v > 1.0f) return sw_err("cell rate `%s`: sample size must lie in [0, number of barcodes]", el);
        if (n == cap) return sw_err("%s rates `%s`: more than %u values", what, text, cap);
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
    return (n < 0 || (size_t)n >= cap) ? sw_err("directory name too long") : 0;
}

/* two values of one list that print the same at %.3f would share their directories and header lines */
int fastf_sweep_check_grid(const float *rates_cell, uint32_t n_c, const float *rates_depth, uint32_t n_r)
{
    if (!n_c || !n_r || !rates_cell || !rates_depth) return sw_err("sweep: the grid needs at least one cell rate and one depth rate");
    for (int pass = 0; pass < 2; pass++) {
        const float *v = pass ? rates_depth : rates_cell;
        const uint32_t n = pass ? n_r : n_c;
        for (uint32_t i = 0; i < n; i++) {
            if (isnan(v[i]) || v[i] < 0) return sw_err("sweep: %s rate %g is negative or not a number", pass ? "depth" : "cell", (double)v[i]);
            if (!pass && v[i] > 1.0f) return sw_err("sweep: cell rate %g: sample size must lie in [0, number of barcodes]", (double)v[i]);
            char a[32], b[32];
            snprintf(a, sizeof a, "%.3f", (double)v[i]);
            for (uint32_t j = 0; j < i; j++) {
                snprintf(b, sizeof b, "%.3f", (double)v[j]);
                if (!strcmp(a, b)) return sw_err("sweep: %s rates %g and %g both print as %s", pass ? "depth" : "cell", (double)v[j], (double)v[i], a);
            }
        }
    }
    return 0;
}

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
 * form of fastf_dev_cell_summary (the point-by-point path, tests) */
int fastf_sweep_cells_from_coo(const fastf_coo_t *coo, uint32_t n_cells, uint64_t *umis_per_cell, uint32_t *genes_per_cell, uint64_t *umis)
{
    if (!coo || !umis || (n_cells && (!umis_per_cell || !genes_per_cell))) return sw_err("null argument");
    memset(umis_per_cell, 0, (size_t)n_cells * sizeof *umis_per_cell);
    memset(genes_per_cell, 0, (size_t)n_cells * sizeof *genes_per_cell);
    uint64_t total = 0;
    for (size_t i = 0; i < coo->nnz; i++) {
        const uint32_t c = coo->cell[i];
        if (c == 0 || c > n_cells) return sw_err("matrix row %zu names cell %u of %u", i, c, n_cells);
        umis_per_cell[c - 1] += coo->count[i];
        genes_per_cell[c - 1] += coo->count[i] >= 1;
        total += coo->count[i];
    }
    *umis = total;
    return 0;
}

/* one row of sweep.tsv (with its newline) */
int fastf_sweep_summary_row(float rate_cell, float rate_depth, uint32_t seed, const uint64_t counters[3], uint64_t nnz, uint64_t umis,
                            const uint64_t *umis_per_cell, const uint32_t *genes_per_cell, uint32_t n_cells, char *buf, size_t cap)
{
    if (!counters || !buf || (n_cells && (!umis_per_cell || !genes_per_cell))) return sw_err("null argument");
    uint64_t *tmp = (uint64_t *)malloc(((size_t)n_cells + 1) * sizeof *tmp);
    if (!tmp) return sw_err("out of memory");
    memcpy(tmp, umis_per_cell, (size_t)n_cells * sizeof *tmp);
    const double med_u = median_u64(tmp, n_cells);
    for (uint32_t i = 0; i < n_cells; i++) tmp[i] = genes_per_cell[i];
    const double med_g = median_u64(tmp, n_cells);
    free(tmp);
    const double sat = counters[2] ? 1.0 - (double)umis / (double)counters[2] : 0.0;
    const int n = snprintf(buf, cap, "%.3f\t%.3f\t%u\t%u\t%llu\t%llu\t%llu\t%llu\t%llu\t%.6f\t%.1f\t%.1f\n", (double)rate_cell, (double)rate_depth,
                           seed, n_cells, (unsigned long long)counters[0], (unsigned long long)counters[1], (unsigned long long)counters[2],
                           (unsigned long long)nnz, (unsigned long long)umis, sat, med_u, med_g);
    return (n < 0 || (size_t)n >= cap) ? sw_err("summary row too long") : 0;
}

/* ------------------------------------------------------------------ */
/* directories, sweep.tsv                                              */
/* ------------------------------------------------------------------ */
static int make_dir(const char *path)
{
    if (mkdir(path, 0777) == 0 || errno == EEXIST) return 0;
    return sw_err("cannot create directory %s: %s", path, strerror(errno));
}

typedef struct { FILE *f; char tmp[4096], final[4096]; } tsv_out;
static int tsv_open(tsv_out *t, const char *out_dir)
{
    snprintf(t->final, sizeof t->final, "%s/sweep.tsv", out_dir);
    snprintf(t->tmp, sizeof t->tmp, "%s/sweep.tsv.partial", out_dir);
    if (!(t->f = fopen(t->tmp, "w"))) return sw_err("cannot open %s: %s", t->tmp, strerror(errno));
    fputs(fastf_sweep_header(), t->f);
    return 0;
}
/* ok: the table appears under its name; otherwise nothing of it is left */
static int tsv_close(tsv_out *t, int ok)
{
    if (!t->f) return 0;
    const int bad = ferror(t->f) | (fclose(t->f) != 0);
    t->f = NULL;
    if (ok && !bad && rename(t->tmp, t->final) == 0) return 0;
    unlink(t->tmp);
    return ok ? sw_err("cannot write %s", t->final) : 0;
}

/* ------------------------------------------------------------------ */
/* point by point through bam2db()                                     */
/* ------------------------------------------------------------------ */
/* counters, dimensions and rows of a matrix.mtx.gz bam2db() wrote */
static int read_matrix(const char *path, uint64_t counters[3], uint32_t *n_cells, fastf_coo_t *coo, uint32_t **rows_out)
{
    gzFile g = gzopen(path, "rb");
    if (!g) return sw_err("cannot read %s back", path);
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
            if (sscanf(line, "%zu %zu %zu", &nf, &nb, &nnz) != 3) { sw_err("%s: no dimension line", path); goto done; }
            *n_cells = (uint32_t)nb;
            rows = (uint32_t *)malloc((nnz ? nnz : 1) * 12);
            if (!rows) { sw_err("out of memory"); goto done; }
            have_dims = 1;
            continue;
        }
        unsigned f, c, k;
        if (at >= nnz || sscanf(line, "%u %u %u", &f, &c, &k) != 3) { sw_err("%s: malformed row", path); goto done; }
        rows[at] = f; rows[nnz + at] = c; rows[2 * nnz + at] = k; at++;
    }
    if (!have_dims || at != nnz) { sw_err("%s: %zu rows of %zu", path, at, nnz); goto done; }
    coo->feature = rows; coo->cell = rows + nnz; coo->count = rows + 2 * nnz; coo->nnz = nnz;
    *rows_out = rows; rows = NULL;
    rc = 0;
done:
    free(rows);
    gzclose(g);
    return rc;
}

static int sweep_point_by_point(const char *bam, const char *out_dir, const char *barcodes, const char *features,
                                const float *rc_list, uint32_t n_c, const float *rd_list, uint32_t n_r, uint32_t seed, int summary_only, tsv_out *tsv)
{
    const int saved_u = _umi_copies_flag;
    _umi_copies_flag = 0;
    int rc = 1;
    for (uint32_t i = 0; i < n_c; i++)
        for (uint32_t j = 0; j < n_r; j++) {
            char name[64], dir[4096], path[4200];
            if (fastf_sweep_point_dir(rc_list[i], rd_list[j], name, sizeof name)) goto done;
            if (summary_only) snprintf(dir, sizeof dir, "%s/.%s.partial", out_dir, name);      /* (removed again below) */
            else snprintf(dir, sizeof dir, "%s/%s", out_dir, name);
            if (make_dir(dir)) goto done;
            const int brc = bam2db((char *)bam, NULL, dir, (char *)barcodes, (char *)features, rc_list[i], rd_list[j], seed);
            uint64_t counters[3]; uint32_t n_cells = 0; fastf_coo_t coo; uint32_t *rows = NULL;
            snprintf(path, sizeof path, "%s/matrix.mtx.gz", dir);
            int prc = brc ? 1 : read_matrix(path, counters, &n_cells, &coo, &rows);
            if (summary_only) {
                static const char *const files[] = {"matrix.mtx.gz", "barcodes.tsv.gz", "features.tsv.gz"};
                for (int k = 0; k < 3; k++) { snprintf(path, sizeof path, "%s/%s", dir, files[k]); unlink(path); }
                rmdir(dir);
            }
            if (brc) { if (!strstr(fastf_last_error(), "bam2db")) sw_err("bam2db failed at point %s: %s", name, fastf_last_error()); goto done; }
            if (prc) goto done;
            uint64_t *upc = (uint64_t *)calloc((size_t)n_cells + 1, sizeof *upc);
            uint32_t *gpc = (uint32_t *)calloc((size_t)n_cells + 1, sizeof *gpc);
            uint64_t umis = 0;
            char row[512];
            prc = !upc || !gpc || fastf_sweep_cells_from_coo(&coo, n_cells, upc, gpc, &umis) ||
                  fastf_sweep_summary_row(rc_list[i], rd_list[j], seed, counters, coo.nnz, umis, upc, gpc, n_cells, row, sizeof row);
            free(upc); free(gpc); free(rows);
            if (prc) goto done;
            fputs(row, tsv->f);
        }
    rc = 0;
done:
    _umi_copies_flag = saved_u;
    return rc;
}

/* ------------------------------------------------------------------ */
/* resident form                                                       */
/* ------------------------------------------------------------------ */
typedef struct {
    int device;
    uint64_t n, cap;                     /* records held, room */
    uint64_t *cb, *gx; uint32_t *umi, *meta;   /* device arrays of cap entries */
} resident_t;

static void resident_free(resident_t *r)
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
        resident_free(&nr);
        return sw_err("sweep: the records do not fit the device: %llu bytes were needed for %llu records", (unsigned long long)(cap * 24), (unsigned long long)need);
    }
    if (r->n && (fastf_devmem_copy(nr.cb, r->cb, r->n * 8) || fastf_devmem_copy(nr.gx, r->gx, r->n * 8) ||
                 fastf_devmem_copy(nr.umi, r->umi, r->n * 4) || fastf_devmem_copy(nr.meta, r->meta, r->n * 4))) { resident_free(&nr); return 1; }
    resident_free(r);
    *r = nr;
    return 0;
}

static uint32_t bits_for(uint64_t v) { uint32_t b = 0; while (b < 64 && (v >> b)) b++; return b ? b : 1; }

enum { SW_OK = 0, SW_FAIL = 1, SW_NOT_COVERED = 2 };
/* layout of the small device block of one point (u64 words; atomics and plain loads on different 256-byte segments) */
enum { SM_KEYS = 0, SM_CNT = 32, SM_NNZ = 64, SM_BASE = 96, SM_HITS = 128, SM_WORDS_ = 160 };

typedef struct { double lists, decode, engine, block_k1a, planes, device, d2h, summary, write; } sweep_times;

/* one cell rate: the engine, the records in its layout, K1a, the planes, then every depth rate */
static int sweep_cell_rate(const resident_t *R, const fastf_lists_t *L, const uint64_t *cell_keys, const char *bam_label, const char *out_dir,
                           float rate_cell, const float *rd_list, uint32_t n_r, uint32_t seed, int summary_only, int device, FILE *tsv,
                           sweep_times *T)
{
    int rc = SW_FAIL;
    const uint64_t N = R->n;
    const uint32_t n_cells = (uint32_t)L->n_cells;
    fastf_engine_t *e = NULL;
    void *d_blk = NULL, *d_keys = NULL, *d_tmp = NULL, *d_planes = NULL, *d_small = NULL, *d_rows = NULL, *d_upc = NULL, *d_gpc = NULL;
    uint64_t *h_small = NULL, *h_upc = NULL; uint32_t *h_gpc = NULL, *h_rows = NULL; uint64_t h_rows_cap = 0;
    uint64_t *thr = (uint64_t *)malloc(n_r * sizeof *thr);
    double tt = now_s();

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
    if (!thr) { sw_err("out of memory"); goto done; }
    if (cfg.umi_max_bases > 16) { rc = SW_NOT_COVERED; goto done; }
    if (fastf_engine_create(&cfg, &e)) goto done;
    if (fastf_engine_is_wide(e)) { rc = SW_NOT_COVERED; goto done; }
    T->engine += now_s() - tt; tt = now_s();

    uint32_t key_bits = 0;
    {   uint32_t cb, fb, ub; if (fastf_engine_key_bits(e, &cb, &fb, &ub, &key_bits)) goto done; }
    uint64_t blk_bytes = 0, seg_slots = 0;
    if (fastf_dev_block_bytes(e, N, &blk_bytes) || fastf_dev_probe_capacity(e, N, &seg_slots)) goto done;
    const int blocked = blk_bytes != 0 && seg_slots != 0, segmented = seg_slots != 0;
    const uint64_t key_slots = (seg_slots > N ? seg_slots : N) + 64;
    const uint32_t kflags = FASTF_PROBE_REUSE_HITS | FASTF_PROBE_DRAW_BITS | (blocked ? FASTF_PROBE_BLOCKED : 0) | (segmented ? FASTF_PROBE_SEGMENTED : 0);
    const size_t need = (blocked ? blk_bytes : 0) + 2 * key_slots * 8 + N * 12 + ((size_t)n_cells + 1) * 12;
    if (!(d_small = fastf_devmem_alloc(device, SM_WORDS_ * 8)) || !(h_small = (uint64_t *)fastf_pinned_alloc(SM_WORDS_ * 8)) ||
        (blocked && !(d_blk = fastf_devmem_alloc(device, blk_bytes))) ||
        !(d_keys = fastf_devmem_alloc(device, key_slots * 8)) || !(d_tmp = fastf_devmem_alloc(device, key_slots * 8)) ||
        !(d_rows = fastf_devmem_alloc(device, (N ? N : 1) * 12)) ||
        !(d_upc = fastf_devmem_alloc(device, ((size_t)n_cells + 1) * 8)) || !(d_gpc = fastf_devmem_alloc(device, ((size_t)n_cells + 1) * 4)) ||
        !(h_upc = (uint64_t *)fastf_pinned_alloc(((size_t)n_cells + 1) * 8)) || !(h_gpc = (uint32_t *)fastf_pinned_alloc(((size_t)n_cells + 1) * 4))) {
        sw_err("sweep: the working set of cell rate %.3f does not fit: %zu bytes were needed beside the records (%s)", (double)rate_cell, need, fastf_last_error());
        goto done;
    }
    uint64_t *const sm = (uint64_t *)d_small;
    uint32_t *const d_f = (uint32_t *)d_rows, *const d_c = d_f + N, *const d_k = d_c + N;
    if (fastf_devmem_zero(d_small, SM_WORDS_ * 8) || fastf_dev_reserve(e, blocked ? 0 : N, N)) goto done;

    /* the records into the engine's layout, K1a once: the cell scratch and the hit count serve every depth rate */
    if (blocked) {
        if (fastf_dev_block_records(e, R->gx, R->umi, R->meta, N, d_blk, NULL) ||
            fastf_dev_count_hits_blocked(e, R->cb, N, d_blk, sm + SM_HITS, NULL)) goto done;
    } else if (fastf_dev_count_hits(e, R->cb, N, sm + SM_HITS, NULL)) goto done;
    if (fastf_devmem_sync() || fastf_devmem_copy(h_small, d_small, SM_WORDS_ * 8)) goto done;
    const uint64_t H = h_small[SM_HITS];
    T->block_k1a += now_s() - tt; tt = now_s();

    /* the decision planes: the draw stream once, every threshold in the same pass */
    const uint64_t plane_words = ((H + 63) / 64) * 2 + 64;      /* (zeroed slack behind each plane: K1b reads a unit's words unconditionally) */
    if (!(d_planes = fastf_devmem_alloc(device, (size_t)n_r * plane_words * 4)) || fastf_devmem_zero(d_planes, (size_t)n_r * plane_words * 4)) goto done;
    for (uint32_t j = 0; j < n_r; j++) thr[j] = fastf_draw_threshold(rd_list[j]);
    if (fastf_dev_mt_decisions_multi(e, seed, L->mt_skip, H, thr, n_r, (uint32_t *)d_planes, plane_words, NULL)) goto done;
    T->planes += now_s() - tt;

    for (uint32_t j = 0; j < n_r; j++) {
        tt = now_s();
        const uint32_t *plane = (const uint32_t *)d_planes + (size_t)j * plane_words;
        if (fastf_devmem_zero(d_small, SM_HITS * 8)) goto done;
        if (fastf_dev_probe_pack(e, R->cb, blocked ? (const uint64_t *)d_blk : R->gx, R->umi, R->meta, N, plane, H, sm + SM_BASE,
                                 (uint64_t *)d_keys, key_slots, sm + SM_KEYS, sm + SM_CNT, kflags, NULL)) goto done;
        int in_tmp = 0;
        if (fastf_dev_sort(e, (uint64_t *)d_keys, (uint64_t *)d_tmp, sm + SM_KEYS, N, key_bits, FASTF_SORT_SKIP_LOW | (segmented ? FASTF_SORT_SEGMENTED : 0), &in_tmp, NULL)) goto done;
        uint64_t *src = in_tmp ? (uint64_t *)d_tmp : (uint64_t *)d_keys, *other = in_tmp ? (uint64_t *)d_keys : (uint64_t *)d_tmp;
        if (fastf_dev_reduce(e, src, sm + SM_KEYS, N, NULL, NULL, NULL, sm + SM_NNZ, FASTF_SORT_SKIP_LOW | FASTF_REDUCE_SEGMENTED, NULL)) goto done;
        uint64_t bits = 0;
        if (fastf_dev_error_bits(e, &bits)) goto done;
        if (bits & FASTF_ERR_RUN_TOO_LONG) {
            /* deep (cell, feature) groups: sort fully and reduce again, as fastf_engine_finish does (every key is still there, permuted) */
            int in_other = 0;
            if (fastf_dev_clear_error_bits(e, FASTF_ERR_RUN_TOO_LONG, NULL) ||
                fastf_dev_sort(e, src, other, sm + SM_KEYS, N, key_bits, 0, &in_other, NULL)) goto done;
            if (in_other) src = other;
            if (fastf_dev_reduce(e, src, sm + SM_KEYS, N, NULL, NULL, NULL, sm + SM_NNZ, FASTF_REDUCE_SEGMENTED, NULL) || fastf_dev_error_bits(e, &bits)) goto done;
        }
        if (fastf_devmem_copy(h_small, d_small, SM_HITS * 8)) goto done;
        bits |= h_small[SM_CNT + 3];
        if (bits & 4) { rc = SW_NOT_COVERED; goto done; }       /* UMIs longer than the key holds: bam2db() runs such a file again with wider keys */
        if (bits) { sw_err("sweep: device error bits 0x%llx at point c%.3f_r%.3f", (unsigned long long)bits, (double)rate_cell, (double)rd_list[j]); goto done; }
        const uint64_t counters[3] = { N, h_small[SM_CNT + 1], h_small[SM_CNT + 2] };
        const uint64_t nnz = h_small[SM_NNZ];
        if (nnz > N) { sw_err("internal error: %llu matrix rows out of %llu records", (unsigned long long)nnz, (unsigned long long)N); goto done; }
        /* the rows, concatenated on the device, and their per-cell summary */
        if (fastf_dev_rows_gather(e, sm + SM_KEYS, d_f, d_c, d_k, NULL) ||
            fastf_dev_cell_summary(e, nnz ? d_c : NULL, nnz ? d_k : NULL, sm + SM_NNZ, n_cells, (uint64_t *)d_upc, (uint32_t *)d_gpc, NULL) ||
            fastf_devmem_sync()) goto done;
        T->device += now_s() - tt; tt = now_s();
        if (fastf_devmem_copy(h_upc, d_upc, ((size_t)n_cells + 1) * 8) || fastf_devmem_copy(h_gpc, d_gpc, (size_t)n_cells * 4)) goto done;
        char row[512];
        if (fastf_sweep_summary_row(rate_cell, rd_list[j], seed, counters, nnz, h_upc[n_cells], h_upc, h_gpc, n_cells, row, sizeof row)) goto done;
        T->summary += now_s() - tt; tt = now_s();
        if (!summary_only) {
            if (nnz > h_rows_cap) {
                if (h_rows) fastf_pinned_free(h_rows);
                h_rows_cap = nnz + nnz / 8 + 1024;
                if (!(h_rows = (uint32_t *)fastf_pinned_alloc(h_rows_cap * 12))) { h_rows_cap = 0; sw_err("sweep: no pinned memory for %llu matrix rows", (unsigned long long)nnz); goto done; }
            }
            fastf_coo_t coo = { h_rows, h_rows + h_rows_cap, h_rows + 2 * h_rows_cap, (size_t)nnz };
            /* (the gather kernel writes pinned host memory directly: it is the device-to-host copy of the rows) */
            if (nnz && (fastf_dev_rows_gather(e, sm + SM_KEYS, h_rows, h_rows + h_rows_cap, h_rows + 2 * h_rows_cap, NULL) || fastf_devmem_sync())) goto done;
            T->d2h += now_s() - tt; tt = now_s();
            char name[64], dir[4096];
            if (fastf_sweep_point_dir(rate_cell, rd_list[j], name, sizeof name)) goto done;
            snprintf(dir, sizeof dir, "%s/%s", out_dir, name);
            if (make_dir(dir) || fastf_write_outputs(dir, bam_label, rate_cell, rd_list[j], counters, L, &coo, NULL)) goto done;
            T->write += now_s() - tt;
        }
        fputs(row, tsv);
    }
    rc = SW_OK;
done:
    if (e) fastf_engine_destroy(e);
    fastf_devmem_free(d_blk); fastf_devmem_free(d_keys); fastf_devmem_free(d_tmp); fastf_devmem_free(d_planes); fastf_devmem_free(d_small);
    fastf_devmem_free(d_rows); fastf_devmem_free(d_upc); fastf_devmem_free(d_gpc);
    if (h_small) fastf_pinned_free(h_small);
    if (h_upc) fastf_pinned_free(h_upc);
    if (h_gpc) fastf_pinned_free(h_gpc);
    if (h_rows) fastf_pinned_free(h_rows);
    free(thr);
    return rc;
}

static int sweep_resident(const char *bam_file, const char *out_dir, const char *barcodes, const char *features,
                          const float *rc_list, uint32_t n_c, const float *rd_list, uint32_t n_r, uint32_t seed, int summary_only, int device, FILE *tsv)
{
    int rc = SW_FAIL;
    const int prof = getenv("FASTF_PROFILE") != NULL;
    sweep_times T; memset(&T, 0, sizeof T);
    const double t0 = now_s();
    double tt = t0;
    fastf_lists_t *L = (fastf_lists_t *)calloc(n_c, sizeof *L);
    uint64_t **keys = (uint64_t **)calloc(n_c, sizeof *keys);
    fastf_bam_t *bam = NULL;
    resident_t R; memset(&R, 0, sizeof R); R.device = device;
    void *stage = NULL;
    if (!L || !keys) { sw_err("out of memory"); goto done; }

    /* the lists of every cell rate, and ONE dictionary for the records: the first rate's, with the barcodes of the others
     * registered in it — a key then means the same string whichever rate's table it is looked up in */
    for (uint32_t i = 0; i < n_c; i++)
        if (fastf_lists_load(barcodes, features, rc_list[i], seed, &L[i])) { n_c = i; goto done; }
    for (uint32_t i = 0; i < n_c; i++) {
        if (L[i].n_features != L[0].n_features) { sw_err("internal error: the feature list changed between loads"); goto done; }
        if (!(keys[i] = (uint64_t *)malloc((L[i].n_cells ? L[i].n_cells : 1) * sizeof **keys))) { sw_err("out of memory"); goto done; }
        for (size_t k = 0; k < L[i].n_cells; k++) keys[i][k] = fastf_keydict_add(L[0].cell_dict, L[i].barcode[k], strlen(L[i].barcode[k]));
        /* keys wider than 64 bits with the shortest UMI field: that cell rate would need the wide engine */
        if (bits_for(L[i].n_cells) + bits_for(L[i].n_features) + 27 > 64) { rc = SW_NOT_COVERED; goto done; }
    }
    T.lists = now_s() - tt; tt = now_s();

    {   const char *gp = getenv("FASTF_GPU_PARSE");
        bam = fastf_bam_open2(bam_file, 0, 1 | ((gp && gp[0] == '0') ? 0 : 4) | ((device + 1) << 8)); }
    if (!bam) { sw_err("Fail to open BAM file %s (%s)", bam_file, fastf_last_error()); goto done; }
    (void)fastf_bam_enable_device_parse(bam, L[0].cell_dict, L[0].feat_dict);
    const size_t cap = (size_t)4 << 20;
    if (!(stage = fastf_pinned_alloc(cap * 24))) { sw_err("sweep: no pinned staging memory (%s)", fastf_last_error()); goto done; }
    uint64_t *s_cb = (uint64_t *)stage, *s_gx = s_cb + cap; uint32_t *s_umi = (uint32_t *)(s_gx + cap), *s_meta = s_umi + cap;
    for (;;) {
        int on_dev = 0; fastf_batch_t dev; memset(&dev, 0, sizeof dev);
        const long n = fastf_bam_read_batch_dev(bam, L[0].cell_dict, L[0].feat_dict, s_cb, s_gx, s_umi, s_meta, cap, &on_dev, &dev);
        if (n < 0) { sw_err("%s: %s", bam_file, fastf_last_error()); goto done; }
        if (n == 0) break;
        if (R.n + (uint64_t)n >= ((uint64_t)1 << 32) - 1) { sw_err("sweep: more than 2^32 - 2 records: %llu bytes of records are beyond what the device-level calls take", (unsigned long long)((R.n + (uint64_t)n) * 24)); goto done; }
        if (resident_reserve(&R, R.n + (uint64_t)n)) goto done;
        const uint64_t *f_cb = on_dev ? dev.cb_key : s_cb, *f_gx = on_dev ? dev.gx_key : s_gx;
        const uint32_t *f_umi = on_dev ? dev.umi : s_umi, *f_meta = on_dev ? dev.meta : s_meta;
        if (fastf_devmem_copy(R.cb + R.n, f_cb, (size_t)n * 8) || fastf_devmem_copy(R.gx + R.n, f_gx, (size_t)n * 8) ||
            fastf_devmem_copy(R.umi + R.n, f_umi, (size_t)n * 4) || fastf_devmem_copy(R.meta + R.n, f_meta, (size_t)n * 4)) goto done;
        R.n += (uint64_t)n;
    }
    {   uint64_t no_xf = 0, no_gx = 0;
        fastf_bam_stats(bam, NULL, &no_xf, &no_gx);
        if (no_xf || no_gx)
            fprintf(stderr, "Note: %llu records with a CB but no xf tag and %llu with a valid xf but no GX tag were skipped "
                            "(the reference dereferences NULL on them).\n", (unsigned long long)no_xf, (unsigned long long)no_gx); }
    fastf_bam_close(bam); bam = NULL;
    fastf_pinned_free(stage); stage = NULL;
    if (resident_reserve(&R, 1)) goto done;               /* (an empty BAM: the arrays exist) */
    T.decode = now_s() - tt;
    printf("sweep: %llu records resident on the device (%llu bytes), %u x %u points\n", (unsigned long long)R.n, (unsigned long long)(R.n * 24), n_c, n_r);

    for (uint32_t i = 0; i < n_c; i++) {
        rc = sweep_cell_rate(&R, &L[i], keys[i], bam_file, out_dir, rc_list[i], rd_list, n_r, seed, summary_only, device, tsv, &T);
        if (rc != SW_OK) goto done;
    }
    rc = SW_OK;
    if (prof)
        fprintf(stderr, "[sweep] lists %.3f s, decode to resident records %.3f s, engines %.3f s, layout+K1a %.3f s, planes %.3f s, "
                        "per-point device work %.3f s (%.4f s a point), summary D2H+medians %.3f s, rows D2H %.3f s, writers %.3f s, total %.3f s\n",
                T.lists, T.decode, T.engine, T.block_k1a, T.planes, T.device, T.device / (n_c * n_r), T.summary, T.d2h, T.write, now_s() - t0);
done:
    if (bam) fastf_bam_close(bam);
    if (stage) fastf_pinned_free(stage);
    resident_free(&R);
    if (keys) for (uint32_t i = 0; i < n_c; i++) free(keys[i]);
    free(keys);
    if (L) for (uint32_t i = 0; i < n_c; i++) fastf_lists_free(&L[i]);
    free(L);
    return rc;
}

/* ------------------------------------------------------------------ */
/* the command                                                         */
/* ------------------------------------------------------------------ */
int fastf_sweep(const char *bam, const char *out_dir, const char *barcodes, const char *features, const float *rates_cell, uint32_t n_c,
                const float *rates_depth, uint32_t n_r, uint32_t seed, uint32_t flags)
{
    if (!bam || !barcodes || !features) return sw_err("sweep: null argument");
    if (!out_dir) out_dir = ".";
    if (fastf_sweep_check_grid(rates_cell, n_c, rates_depth, n_r)) return 1;
    if (flags & ~(uint32_t)FASTF_SWEEP_SUMMARY_ONLY) return sw_err("sweep: unknown flags 0x%x", flags);
    const int summary_only = (flags & FASTF_SWEEP_SUMMARY_ONLY) != 0;
    if (access(bam, R_OK) == -1) return sw_err("bam file: %s does not exist.", bam);
    if (make_dir(out_dir)) return 1;
    tsv_out tsv; memset(&tsv, 0, sizeof tsv);
    if (tsv_open(&tsv, out_dir)) return 1;

    int dev0 = 0, dev_second = -1, several = 0;
    {   const char *dvs = getenv("FASTF_DEVICES");
        fastf_pick_devices(dvs, getenv("FASTF_DEVICE"), &dev0, &dev_second);
        several = dvs && *dvs && (strchr(dvs, ',') || atoi(dvs) >= 2); }
    int rc = several ? SW_NOT_COVERED : sweep_resident(bam, out_dir, barcodes, features, rates_cell, n_c, rates_depth, n_r, seed, summary_only, dev0, tsv.f);
    if (rc == SW_NOT_COVERED) {
        fprintf(stderr, "sweep: this job is outside the resident form (%s): running bam2db point by point\n",
                several ? "several devices" : "keys wider than 64 bits or UMIs beyond what a 64-bit key holds");
        /* (rows a resident attempt had written are of no use: the table starts again) */
        tsv_close(&tsv, 0);
        if (tsv_open(&tsv, out_dir)) return 1;
        rc = sweep_point_by_point(bam, out_dir, barcodes, features, rates_cell, n_c, rates_depth, n_r, seed, summary_only, &tsv);
    }
    if (rc) { char keep[512]; snprintf(keep, sizeof keep, "%s", fastf_last_error()); tsv_close(&tsv, 0); fastf_set_error_(keep); return 1; }
    return tsv_close(&tsv, 1);
}

static void usage_sweep(FILE *f)
{
    fprintf(f,
            "Usage: fastF sweep [options]\n\n"
            "bam2db over a grid of cell and depth rates from one decode of the bam file: per point <out>/c<cell>_r<depth>/ with the\n"
            "three files of bam2db, and <out>/sweep.tsv with one summary row per point.\n\n"
            "    -h, --help            show this help message and exit\n"
            "    -b, --bam=<str>       path to bam file\n"
            "    -f, --feature=<str>   path to feature list file\n"
            "    -a, --barcode=<str>   path to barcode list file\n"
            "    -d, --dbname=<str>    name of database (accepted for compatibility, ignored)\n"
            "    -c, --cell=<list>     rates of cell barcode, comma separated (default 1.0)\n"
            "    -r, --depth=<list>    rates of depth, comma separated (default 1.0)\n"
            "    -o, --out=<str>       path to output directory (default .)\n"
            "    -s, --seed=<int>      seed for random number generator (default 926)\n"
            "        --summary-only    write sweep.tsv alone\n");
}

struct sopt { char s; const char *l; int has_arg; };
static const struct sopt k_sopts[] = {
    {'h', "help", 0}, {'b', "bam", 1}, {'f', "feature", 1}, {'a', "barcode", 1}, {'d', "dbname", 1}, {'c', "cell", 1}, {'r', "depth", 1},
    {'o', "out", 1}, {'s', "seed", 1}, {'u', "umicopies", 0}, {'S', "summary-only", 0}, {0, NULL, 0}};

#define SWEEP_MAX_RATES 64
int cmd_sweep(int argc, const char **argv)
{
    const char *bam = NULL, *feat = NULL, *bar = NULL, *out = ".", *cells = "1", *depths = "1";
    unsigned int seed = 926;
    int summary_only = 0;
    for (int i = 1; i < argc; i++) {
        const char *a = argv[i];
        const struct sopt *o = NULL;
        const char *val = NULL;
        if (a[0] != '-' || !a[1]) break;
        if (a[1] == '-') {
            if (!a[2]) break;
            const char *eq = strchr(a + 2, '=');
            const size_t nl = eq ? (size_t)(eq - a - 2) : strlen(a + 2);
            for (const struct sopt *k = k_sopts; k->l; k++)
                if (strlen(k->l) == nl && strncmp(k->l, a + 2, nl) == 0) { o = k; break; }
            if (o && eq) val = eq + 1;
        } else {
            for (const struct sopt *k = k_sopts; k->l; k++) if (k->s == a[1] && k->s != 'S') { o = k; break; }
            if (o && o->has_arg && a[2]) val = a + 2;
        }
        if (!o) { fprintf(stderr, "error: unknown option `%s`\n", a); usage_sweep(stderr); return 1; }
        char oname[32];
        if (a[1] == '-') snprintf(oname, sizeof oname, "--%s", o->l); else snprintf(oname, sizeof oname, "-%c", o->s);
        if (o->has_arg && !val) {
            if (i + 1 >= argc) { fprintf(stderr, "error: option `%s` requires a value\n", oname); return 1; }
            val = argv[++i];
        }
        char *end = NULL;
        switch (o->s) {
        case 'h': usage_sweep(stdout); return 0;
        case 'b': bam = val; break;
        case 'f': feat = val; break;
        case 'a': bar = val; break;
        case 'd': break;
        case 'o': out = val; break;
        case 'c': cells = val; break;
        case 'r': depths = val; break;
        case 's': errno = 0; seed = (unsigned int)strtol(val, &end, 0);
                  if (errno == ERANGE) { fprintf(stderr, "error: option `%s` numerical result out of range\n", oname); return 1; }
                  if (*end) { fprintf(stderr, "error: option `%s` expects an integer value\n", oname); return 1; }
                  break;
        case 'u': fprintf(stderr, "\x1b[31mError:\x1b[0m sweep does not write umi.tsv.gz (-u): run bam2db -u for the points that need it.\n"); return 1;
        case 'S': summary_only = 1; break;
        }
    }
    float rc[SWEEP_MAX_RATES], rd[SWEEP_MAX_RATES];
    uint32_t n_c = 0, n_r = 0;
    if (fastf_sweep_parse_rates(cells, 1, rc, SWEEP_MAX_RATES, &n_c) || fastf_sweep_parse_rates(depths, 0, rd, SWEEP_MAX_RATES, &n_r) ||
        fastf_sweep_check_grid(rc, n_c, rd, n_r)) {
        fprintf(stderr, "\x1b[31mError:\x1b[0m %s\n", fastf_last_error());
        return 1;
    }
    if (!bam || access(bam, F_OK) == -1) { fprintf(stderr, "\x1b[31mError:\x1b[0m bam file: %s does not exist.\n", bam ? bam : "(null)"); return 1; }
    if (!feat || access(feat, F_OK) == -1) { fprintf(stderr, "\x1b[31mError:\x1b[0m feature file: %s does not exist.\n", feat ? feat : "(null)"); return 1; }
    if (!bar || access(bar, F_OK) == -1) { fprintf(stderr, "\x1b[31mError:\x1b[0m barcode file: %s does not exist.\n", bar ? bar : "(null)"); return 1; }
    if (fastf_sweep(bam, out, bar, feat, rc, n_c, rd, n_r, seed, summary_only ? FASTF_SWEEP_SUMMARY_ONLY : 0)) {
        fprintf(stderr, "\x1b[31mError:\x1b[0m sweep failed: %s\n", fastf_last_error());
        return 1;
    }
    printf("sweep.tsv is generated.\n");
    return 0;
}
