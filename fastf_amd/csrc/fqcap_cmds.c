/*
 * fqcap_cmds.c — `fqcap`: the FASTQ triple with every cell capped at N reads (not a command of the reference).
 * The definition stands in include/fastf_amd.h.
 *
 * filter with a rate per cell.  R1 is read twice through filter's device windows (filter_host.h, filter_kernels.hpp):
 *   pass 0   counts the matched reads of every cell: the DNA-form cells on the device (fcp_count_kernel, fqcap_kernels.hpp), the
 *            escape-form reads — every one of them — on the host, per escape prefix of the whitelist
 *   between  hits[] comes back in one copy, the host turns it into rate_k = fastf_fqcap_rate(N, h[k], t), one upload
 *   pass 1   filter's R1 pass with fcp_rec_kernel in flt_rec_kernel's place; the host decides the escape-form reads whose draw
 *            passed t by the same rule, with their draws from a copy of the window's draws
 *   pass 2   I1 and R2 against the keep bitmap: filter's mode 1, unchanged
 * Everything that can be refused is refused before the output directory is touched: the arguments, and in pass 0 the long lines
 * and the truncated R1 that filter declares as divergences.  What only a mate file shows (pass 2) comes too late for that: the
 * outputs written so far are removed again.
 */
#define _GNU_SOURCE
#include "filter_host.h"
#include "cli_opts.h"
#include "fqcap_kernels.hpp"

#include <errno.h>
#include <fcntl.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

static void fc_err(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static void fc_err(const char *fmt, ...)
{
    char b[768];
    va_list ap; va_start(ap, fmt); vsnprintf(b, sizeof b, fmt, ap); va_end(ap);
    fastf_set_error_(b);
}

float fastf_fqcap_rate(uint64_t cap, uint64_t hits, float t)
{
    if (hits <= cap) return t;
    const float c = (float)((double)cap / (double)hits);
    return c < t ? c : t;
}

/* ------------------------------------------------------------------ */
/* the two R1 passes as hooks of filter's window loop                    */
/* ------------------------------------------------------------------ */
typedef struct {
    const fl_wl *wl;                     /* its escape prefixes unique */
    uint64_t cap; float t;
    uint64_t *esc_h, *esc_kept;          /* per escape prefix: matched reads, kept reads */
    uint32_t *draws; uint64_t draws_cap, n_rec; int have_draws;   /* pass 1: the window's draws, fetched for its first matched escape */
} fc_ctx;

static long esc_find(const fl_wl *w, const unsigned char *p, uint32_t m)
{
    fl_str k = { (const char *)p, m };
    const fl_str *hit = (const fl_str *)bsearch(&k, w->esc, w->n_esc, sizeof *w->esc, fl_str_cmp);
    return hit ? (long)(hit - w->esc) : -1;
}

static int count_decide(void *vc, fastf_fltdev_t *dev, uint32_t L, const uint32_t *cs, uint64_t n_rec, const fastf_flt_esc_t **esc,
                        uint32_t *n_esc)
{
    (void)vc; (void)cs; (void)n_rec;
    return fastf_fcpdev_count(dev, L, esc, n_esc);
}
static int count_escape(void *vc, fastf_fltdev_t *dev, const unsigned char *p, uint32_t m, uint32_t i)
{
    (void)dev; (void)i;
    fc_ctx *c = (fc_ctx *)vc;
    const long k = esc_find(c->wl, p, m);
    if (k >= 0) c->esc_h[k]++;
    return 0;
}
static int cap_decide(void *vc, fastf_fltdev_t *dev, uint32_t L, const uint32_t *cs, uint64_t n_rec, const fastf_flt_esc_t **esc,
                      uint32_t *n_esc)
{
    fc_ctx *c = (fc_ctx *)vc;
    c->n_rec = n_rec; c->have_draws = 0;
    return fastf_fcpdev_decide(dev, L, c->t, cs, esc, n_esc);
}
static int cap_escape(void *vc, fastf_fltdev_t *dev, const unsigned char *p, uint32_t m, uint32_t i)
{
    fc_ctx *c = (fc_ctx *)vc;
    const long k = esc_find(c->wl, p, m);
    if (k < 0) return 0;
    if (!c->have_draws) {
        if (c->n_rec > c->draws_cap) {
            free(c->draws);
            c->draws_cap = c->n_rec;
            c->draws = (uint32_t *)malloc(c->draws_cap * sizeof *c->draws);
            if (!c->draws) { c->draws_cap = 0; fc_err("out of memory"); return -1; }
        }
        if (fastf_fcpdev_draws(dev, c->draws, c->n_rec)) return -1;
        c->have_draws = 1;
    }
    if (i >= c->n_rec) { fc_err("fqcap: escape %u of a window of %llu reads", i, (unsigned long long)c->n_rec); return -1; }
    const int keep = flt_draw_passes(c->draws[i], fastf_fqcap_rate(c->cap, c->esc_h[k], c->t));
    if (keep) c->esc_kept[k]++;
    return keep;
}

/* ------------------------------------------------------------------ */
/* fqcap_cells.tsv.gz                                                    */
/* ------------------------------------------------------------------ */
typedef struct { fl_str s; uint64_t h, kept; } fc_row;
static int row_cmp(const void *a, const void *b) { return fl_str_cmp(&((const fc_row *)a)->s, &((const fc_row *)b)->s); }

/* the bytes of a barcode as a TSV field: printable ASCII but the backslash as it is, any other byte as \xHH */
static size_t put_barcode(char *o, const fl_str *s)
{
    size_t n = 0;
    for (uint32_t i = 0; i < s->n; i++) {
        const unsigned char ch = (unsigned char)s->p[i];
        if (ch > 0x20 && ch < 0x7f && ch != '\\') o[n++] = (char)ch;
        else n += (size_t)sprintf(o + n, "\\x%02X", ch);
    }
    return n;
}

static int write_cells(const char *dir, char *path, size_t path_cap, const fl_wl *wl, uint32_t L, const uint32_t *hits,
                       const uint32_t *kept, const fc_ctx *c, uint64_t *sum_kept)
{
    size_t n = 0, bytes = 64;
    for (size_t k = 0; k < wl->n_dna; k++) n += hits[k] != 0;
    for (size_t k = 0; k < wl->n_esc; k++) n += c->esc_h[k] != 0;
    fc_row *rows = (fc_row *)malloc((n ? n : 1) * sizeof *rows);
    char *dna = (char *)malloc(wl->n_dna * (size_t)L + 1);
    if (!rows || !dna) { free(rows); free(dna); fc_err("out of memory"); return 1; }
    n = 0;
    for (size_t k = 0; k < wl->n_dna; k++) {
        if (!hits[k]) continue;
        fq_decode_dna(wl->dna[k], L, dna + k * L);
        rows[n].s.p = dna + k * L; rows[n].s.n = L; rows[n].h = hits[k]; rows[n].kept = kept[k];
        n++;
    }
    for (size_t k = 0; k < wl->n_esc; k++) {
        if (!c->esc_h[k]) continue;
        rows[n].s = wl->esc[k]; rows[n].h = c->esc_h[k]; rows[n].kept = c->esc_kept[k];
        n++;
    }
    qsort(rows, n, sizeof *rows, row_cmp);
    for (size_t k = 0; k < n; k++) bytes += 4 * (size_t)rows[k].s.n + 48;
    char *txt = (char *)malloc(bytes);
    if (!txt) { free(rows); free(dna); fc_err("out of memory"); return 1; }
    size_t o = (size_t)sprintf(txt, "barcode\treads\tkept\n");
    *sum_kept = 0;
    for (size_t k = 0; k < n; k++) {
        o += put_barcode(txt + o, &rows[k].s);
        o += (size_t)sprintf(txt + o, "\t%llu\t%llu\n", (unsigned long long)rows[k].h, (unsigned long long)rows[k].kept);
        *sum_kept += rows[k].kept;
    }
    fl_sink s;
    double t = 0;
    int rc = fl_sink_open(&s, dir, "fqcap_cells.tsv.gz", path, path_cap);
    if (!rc) {
        rc = fl_sink_write(&s, (const unsigned char *)txt, o, &t);
        if (fl_sink_close(&s)) rc = 1;
    }
    free(txt); free(rows); free(dna);
    return rc;
}

/* ------------------------------------------------------------------ */
/* the command body                                                      */
/* ------------------------------------------------------------------ */
static const char *const FC_OUT[4] = {"I1.fastq.gz", "R1.fastq.gz", "R2.fastq.gz", "fqcap_cells.tsv.gz"};

int fastf_fqcap(const char *r1, const char *i1, const char *r2, const char *out_dir, const char *whitelist, uint32_t len_cellbarcode,
                uint32_t seed, float rate, uint64_t cap, uint64_t *n_reads, uint64_t *n_matched, uint64_t *n_kept)
{
    if (!r1) { fc_err("fastf_fqcap: the R1 path is required"); return 1; }
    if (!whitelist) { fc_err("fastf_fqcap: a whitelist is required (the cells are its barcodes)"); return 1; }
    if (!cap) { fc_err("fastf_fqcap: the cap must be at least 1 read per cell"); return 1; }
    if ((int32_t)len_cellbarcode < 0) { fc_err("fastf_fqcap: negative barcode length %d", (int32_t)len_cellbarcode); return 1; }
    const char *dir = out_dir ? out_dir : ".";
    const char *in[3] = {i1, r1, r2};
    const int want[4] = {i1 != NULL, 1, r2 != NULL, 1};
    if (!fl_dir_writable(dir, FC_OUT, want, 4)) { fc_err("fastf_fqcap: cannot write the outputs into directory %s", dir); return 1; }

    const int prof = getenv("FASTF_PROFILE") != NULL;
    const double t0 = fl_now();
    fl_wl wl; memset(&wl, 0, sizeof wl);
    fq_src src_s[3], r1_again; fq_src *src[3] = {NULL, NULL, NULL}, *src1 = NULL;
    fl_sink sink_s[3]; fl_sink *sink[3] = {NULL, NULL, NULL};
    char paths[4][4096];
    int made[4] = {0, 0, 0, 0};
    fc_ctx C; memset(&C, 0, sizeof C);
    fl_run R; memset(&R, 0, sizeof R);
    uint32_t *hits = NULL, *kept = NULL;
    float *rates = NULL;
    double t_pass[4] = {0, 0, 0, 0}, t_open = 0, t_mid = 0;
    uint64_t matched = 0;
    int rc = 1;
    memset(src_s, 0, sizeof src_s); memset(sink_s, 0, sizeof sink_s); memset(&r1_again, 0, sizeof r1_again);
    for (int f = 0; f < 4; f++) paths[f][0] = 0;

    if (fl_wl_load(&wl, whitelist, len_cellbarcode, 1)) goto done;
    {   /* one cell per distinct prefix: duplicate lines and lines that share their first len bytes are one entry */
        size_t u = 0;
        for (size_t k = 0; k < wl.n_esc; k++) if (!u || fl_str_cmp(&wl.esc[u - 1], &wl.esc[k])) wl.esc[u++] = wl.esc[k];
        wl.n_esc = u;
    }
    C.wl = &wl; C.cap = cap; C.t = rate;
    C.esc_h = (uint64_t *)calloc(wl.n_esc ? wl.n_esc : 1, sizeof *C.esc_h);
    C.esc_kept = (uint64_t *)calloc(wl.n_esc ? wl.n_esc : 1, sizeof *C.esc_kept);
    hits = (uint32_t *)calloc(wl.n_dna ? wl.n_dna : 1, sizeof *hits);
    kept = (uint32_t *)calloc(wl.n_dna ? wl.n_dna : 1, sizeof *kept);
    rates = (float *)malloc((wl.n_dna ? wl.n_dna : 1) * sizeof *rates);
    if (!C.esc_h || !C.esc_kept || !hits || !kept || !rates) { fc_err("out of memory"); goto done; }
    for (int f = 0; f < 3; f++) {
        if (!in[f]) continue;
        if (fastf_fq_src_open(&src_s[f], in[f])) goto done;
        src[f] = &src_s[f];
    }

    R.W = fastf_fq_window_bytes();
    if (R.W < FLT_HDR) R.W = FLT_HDR;
    R.len = len_cellbarcode; R.rate = rate; R.seed = seed; R.wl = &wl;
    if (fastf_fltdev_create(0, R.W, &R.dev)) goto done;
    t_open = fl_now() - t0;
    R.stage = (unsigned char *)fastf_pinned_alloc(FLT_HDR + R.W + 128);
    if (!R.stage) goto done;
    if (fastf_fltdev_set_whitelist(R.dev, wl.dna, wl.n_dna) || fastf_fcpdev_begin(R.dev)) goto done;

    /* pass 0: h[k] over the whole of R1, no draw, nothing written */
    {
        const double t = fl_now();
        const fl_hooks hk = {1, count_decide, count_escape, &C};
        R.hk = &hk;
        if (fl_file(&R, src[1], 0, ~0ull, in[1], NULL)) goto done;
        t_pass[0] = fl_now() - t;
    }
    if (R.n_reads >> 32) {
        fc_err("%s: %llu reads; the per-cell counters are 32-bit (at most 4294967295 reads; refused)", in[1], (unsigned long long)R.n_reads);
        goto done;
    }
    /* between the passes: one copy down, the rates, one copy up */
    {
        const double t = fl_now();
        if (wl.n_dna && fastf_fcpdev_read(R.dev, 0, hits, wl.n_dna)) goto done;
        for (size_t k = 0; k < wl.n_dna; k++) { rates[k] = fastf_fqcap_rate(cap, hits[k], rate); matched += hits[k]; }
        for (size_t k = 0; k < wl.n_esc; k++) matched += C.esc_h[k];
        if (fastf_fcpdev_set_rates(R.dev, rates, wl.n_dna)) goto done;
        t_mid = fl_now() - t;
    }
    if (fastf_fq_src_open(&r1_again, r1)) goto done;
    src1 = &r1_again;
    for (int f = 0; f < 3; f++) {
        if (!in[f]) continue;
        if (fl_sink_open(&sink_s[f], dir, FC_OUT[f], paths[f], sizeof paths[f])) goto done;
        sink[f] = &sink_s[f]; made[f] = 1;
    }
    /* pass 1: R1 decided per cell */
    {
        const double t = fl_now();
        const fl_hooks hk = {0, cap_decide, cap_escape, &C};
        const uint64_t reads0 = R.n_reads;
        R.hk = &hk;
        if (fl_file(&R, src1, 0, ~0ull, in[1], sink[1])) goto done;
        if (R.n_reads != reads0) { fc_err("%s: %llu reads in the second pass, %llu in the first", in[1], (unsigned long long)R.n_reads, (unsigned long long)reads0); goto done; }
        t_pass[1] = fl_now() - t;
    }
    /* pass 2: the mates against the bitmap */
    R.hk = NULL;
    for (int f = 0; f <= 2; f += 2) {
        if (!src[f]) continue;
        const double t = fl_now();
        if (fl_file(&R, src[f], 1, R.n_reads, in[f], sink[f])) goto done;
        t_pass[f ? 3 : 2] = fl_now() - t;
    }
    {
        uint64_t sum = 0;
        if (wl.n_dna && fastf_fcpdev_read(R.dev, 1, kept, wl.n_dna)) goto done;
        made[3] = 1;
        if (write_cells(dir, paths[3], sizeof paths[3], &wl, len_cellbarcode, hits, kept, &C, &sum)) goto done;
        if (sum != R.n_kept) { fc_err("fqcap: %llu reads kept per cell, %llu written", (unsigned long long)sum, (unsigned long long)R.n_kept); goto done; }
    }
    rc = 0;
    for (int f = 0; f < 3; f++) if (sink[f] && fl_sink_close(sink[f])) rc = 1;
    if (n_reads) *n_reads = R.n_reads;
    if (n_matched) *n_matched = matched;
    if (n_kept) *n_kept = R.n_kept;
    if (prof)
        fprintf(stderr, "[fqcap] %llu reads, %llu matched, %llu kept, cap %llu, window %zu, %d host threads: open %.3f s, R1 count %.3f s, "
                "rates %.3f s, R1 decide %.3f s, I1 %.3f s, R2 %.3f s; inflate/read %.3f s, deflate/write %.3f s, host draws + escapes "
                "%.3f s (%llu escapes)\n", (unsigned long long)R.n_reads, (unsigned long long)matched, (unsigned long long)R.n_kept,
                (unsigned long long)cap, R.W, fastf_host_thread_count(), t_open, t_pass[0], t_mid, t_pass[1], t_pass[2], t_pass[3],
                R.t_fill, R.t_deflate, R.t_host, (unsigned long long)R.n_escapes);
done:
    {
        char keep[768];
        if (rc) snprintf(keep, sizeof keep, "%s", fastf_last_error());
        for (int f = 0; f < 3; f++) { if (sink[f] && sink[f]->f) fclose(sink[f]->f); if (src[f]) fastf_fq_src_close(src[f]); }
        if (src1) fastf_fq_src_close(src1);
        if (rc) for (int f = 0; f < 4; f++) if (made[f]) unlink(paths[f]);      /* no partial outputs behind a refusal */
        fastf_fltdev_destroy(R.dev);
        fastf_pinned_free(R.stage);
        if (rc) fastf_set_error_(keep);
    }
    free(C.esc_h); free(C.esc_kept); free(C.draws); free(hits); free(kept); free(rates);
    fl_wl_free(&wl);
    return rc;
}

/* ------------------------------------------------------------------ */
/* CLI: filter's dialect                                                 */
/* ------------------------------------------------------------------ */
static void fc_usage(void)
{
    printf("Usage: fastF fqcap [options]\n\nFilter fastq files by cell barcode whitelist, every cell capped at N reads.\n\n"
           "A read is of the cell named by the first -l bytes of its R1 sequence line, as filter's whitelist test sees them.\n"
           "A cell with h matched reads keeps each with probability min(rate, N / h) (rate alone where h <= N), drawn read by\n"
           "read from filter's rand() stream: at most N reads per cell in expectation, not exactly.\n\n"
           "    -h, --help              show this help message and exit\n\nBasic options\n"
           "    -I, --I1=<str>          optional, path to sample I1 fastq files\n"
           "    -R, --R1=<str>          required, path to sample R1 fastq files\n"
           "    -r, --R2=<str>          optional, path to sample R2 fastq files\n"
           "    -o, --out=<str>         dir to output fastq files and fqcap_cells.tsv.gz\n"
           "    -w, --whitelist=<str>   required, whitelist of cell barcodes\n"
           "    -n, --reads=<int>       required, reads per cell to cap at (N >= 1)\n"
           "    -l, --len=<int>         length of cell barcode\n"
           "    -s, --seed=<int>        seed for random number generator\n"
           "    -t, --rate=<flt>        optional, rate of reads to keep on top of the cap (absent: the cap alone)\n\n");
}

int cmd_fqcap(int argc, const char **argv)
{
    const char *i1 = NULL, *r1 = NULL, *r2 = NULL, *out = ".", *wlp = NULL, *nval = NULL;
    int32_t len = 16, seed = 926;
    float rate = 2.0f;
    static const cli_opt opts[] = {{'h', "help", 0}, {'I', "I1", 1}, {'R', "R1", 1}, {'r', "R2", 1}, {'o', "out", 1}, {'w', "whitelist", 1},
                                   {'n', "reads", 1}, {'l', "len", 1}, {'s', "seed", 1}, {'t', "rate", 1}, {0, NULL, 0}};
    cli_scan S = CLI_SCAN(argc, argv, opts, CLI_ARGPARSE);
    for (const cli_opt *o; (o = cli_next(&S));)
        switch (o->s) {
        case 'h': fc_usage(); exit(0);
        case 'I': i1 = S.val; break;
        case 'R': r1 = S.val; break;
        case 'r': r2 = S.val; break;
        case 'o': out = S.val; break;
        case 'w': wlp = S.val; break;
        case 'n': nval = S.val; break;
        case 'l': len = (int)cli_int(&S); break;
        case 's': seed = (int)cli_int(&S); break;
        case 't': rate = cli_float(&S); break;
        }
    if (S.err) { if (S.err == CLI_UNKNOWN) fc_usage(); exit(EXIT_FAILURE); }
    if (r1 == NULL) { fprintf(stderr, "\x1b[31mError:\x1b[0m -R: the path to the R1 fastq file is required.\n"); exit(1); }
    if (nval == NULL) { fprintf(stderr, "\x1b[31mError:\x1b[0m -n: the reads per cell to cap at are required.\n"); exit(1); }
    uint64_t cap = 0;
    {
        const char *p = nval;
        int ok = *p != 0;
        for (; *p && ok; p++) {
            if (*p < '0' || *p > '9' || cap > (UINT64_MAX - (uint64_t)(*p - '0')) / 10) ok = 0;
            else cap = cap * 10 + (uint64_t)(*p - '0');
        }
        if (!ok || !cap) { fprintf(stderr, "\x1b[31mError:\x1b[0m -n %s: the cap is a whole number of reads, digits only, at least 1.\n", nval); exit(1); }
    }
    if (wlp == NULL) { fprintf(stderr, "\x1b[31mError:\x1b[0m -w: a whitelist is required (the cells are its barcodes).\n"); exit(1); }
    if (len < 0) { fprintf(stderr, "\x1b[31mError:\x1b[0m -l %d: negative length of cell barcode (refused)\n", len); exit(1); }
    const char *in[3] = {i1, r1, r2};
    const int want[4] = {i1 != NULL, 1, r2 != NULL, 1};
    if (!fl_dir_writable(out, FC_OUT, want, 4)) {
        fprintf(stderr, "\x1b[31mError:\x1b[0m -o: cannot write the outputs into directory %s (refused)\n", out);
        exit(1);
    }
    for (int f = 0; f < 3; f++) {
        if (!in[f]) continue;
        const int fd = open(in[f], O_RDONLY);
        if (fd < 0) { fprintf(stderr, "Cannot open file %s \n", in[f]); exit(1); }
        close(fd);
    }
    uint64_t nr = 0, nm = 0, nk = 0;
    if (fastf_fqcap(r1, i1, r2, out, wlp, (uint32_t)len, (uint32_t)seed, rate, cap, &nr, &nm, &nk)) {
        fprintf(stderr, "ERROR: fastF fqcap: %s\n", fastf_last_error());
        exit(1);
    }
    printf("fqcap: %llu reads, %llu matched, %llu kept (cap %llu reads per cell)\n", (unsigned long long)nr, (unsigned long long)nm,
           (unsigned long long)nk, (unsigned long long)cap);
    return 0;
}
