/*
 * fqcells_cmds.c — `fqcells`: the cells of an R1 FASTQ, called by UMIs per barcode (not a command of the reference).
 * The definition stands in include/fastf_amd.h.
 *
 *   parse      freq's source, windows and device parse with L = l + u (fastf_fq_dna_keys, fastq_cmds.c): a read that is not DNA-form
 *              leaves key 0; nothing is escaped, interned or scattered
 *   histogram  the tag histogram's sort and distinct keys, left on the device (fastf_taghist_finish_device, tag_hist.hpp)
 *   reduce     distinct CB+UMI keys -> (barcode, reads, umis) rows (fqcells_kernels.hpp); the rows come down in one copy an array
 *   call       fastf_fqcells_call below: the order and the rule, on the host threads — every row is written anyway
 *   rows       fqcells.tsv.gz through the chunk-parallel gzip writer, whitelist.txt, fqcells_summary.tsv
 * Nothing is created in the output directory before the whole of R1 went through the parse.
 */
#define _GNU_SOURCE
#include "filter_host.h"
#include "cli_opts.h"
#include "fqcells_kernels.hpp"

#include <errno.h>
#include <fcntl.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

static void qc_err(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static void qc_err(const char *fmt, ...)
{
    char b[768];
    va_list ap; va_start(ap, fmt); vsnprintf(b, sizeof b, fmt, ap); va_end(ap);
    fastf_set_error_(b);
}

/* ------------------------------------------------------------------ */
/* the order and the rule                                                */
/* ------------------------------------------------------------------ */
typedef struct { const uint64_t *bc, *reads; const uint32_t *umis; } qc_tab;

static int qc_before(const qc_tab *t, uint32_t i, uint32_t j)      /* < 0: i ranks before j */
{
    if (t->umis[i] != t->umis[j]) return t->umis[i] > t->umis[j] ? -1 : 1;
    if (t->reads[i] != t->reads[j]) return t->reads[i] > t->reads[j] ? -1 : 1;
    return t->bc[i] < t->bc[j] ? -1 : t->bc[i] > t->bc[j];
}
static int qc_cmp(const void *a, const void *b, void *vt) { return qc_before((const qc_tab *)vt, *(const uint32_t *)a, *(const uint32_t *)b); }

/* idx[0, n) sorted: the nt slices by qsort, then rounds of pairwise merges, all on the host threads */
typedef struct { const qc_tab *t; uint32_t *src, *dst; size_t n; int nt, width; } qc_sort_job;
static size_t qc_cut(const qc_sort_job *j, int c) { return c >= j->nt ? j->n : j->n * (size_t)c / (size_t)j->nt; }
static void qc_sort_worker(void *vp, int w)
{
    qc_sort_job *j = (qc_sort_job *)vp;
    if (!j->width) { qsort_r(j->src + qc_cut(j, w), qc_cut(j, w + 1) - qc_cut(j, w), sizeof *j->src, qc_cmp, (void *)j->t); return; }
    const int c = w * 2 * j->width;                                /* slices [c, c + width) and [c + width, c + 2 width) */
    size_t a = qc_cut(j, c), b = qc_cut(j, c + j->width), o = a;
    const size_t ae = b, be = qc_cut(j, c + 2 * j->width);
    while (a < ae && b < be) j->dst[o++] = qc_before(j->t, j->src[b], j->src[a]) < 0 ? j->src[b++] : j->src[a++];
    while (a < ae) j->dst[o++] = j->src[a++];
    while (b < be) j->dst[o++] = j->src[b++];
}
static int qc_sort(const qc_tab *t, uint32_t *idx, size_t n)
{
    int nt = n < 65536 ? 1 : fastf_host_thread_count();
    if (nt < 1) nt = 1;
    qc_sort_job j = { t, idx, NULL, n, nt, 0 };
    fastf_par_run(nt, qc_sort_worker, &j);
    if (nt == 1) return 0;
    uint32_t *tmp = (uint32_t *)malloc(n * sizeof *tmp);
    if (!tmp) { qc_err("out of memory"); return 1; }
    j.dst = tmp;
    for (j.width = 1; j.width < nt; j.width *= 2) {
        fastf_par_run((nt + 2 * j.width - 1) / (2 * j.width), qc_sort_worker, &j);
        uint32_t *s = j.src; j.src = j.dst; j.dst = s;
    }
    if (j.src != idx) memcpy(idx, j.src, n * sizeof *idx);
    free(tmp);
    return 0;
}

int fastf_fqcells_call(const uint64_t *bc, const uint64_t *reads, const uint32_t *umis, size_t n, int rule, uint64_t arg,
                       uint32_t *rank, uint8_t *called, uint64_t *threshold)
{
    if ((n && (!bc || !reads || !umis)) || !threshold) { qc_err("fastf_fqcells_call: null argument"); return 1; }
    if (rule != 'e' && rule != 'k' && rule != 'm') { qc_err("fastf_fqcells_call: the rule is 'e', 'k' or 'm'"); return 1; }
    if (!arg) { qc_err("fastf_fqcells_call: rule '%c' with the argument 0 (at least 1)", rule); return 1; }
    if (n >= 0xffffffffull) { qc_err("fastf_fqcells_call: %zu barcodes (the ranks are 32-bit)", n); return 1; }
    *threshold = rule == 'm' ? arg : rule == 'e' ? 1 : 0;
    if (!n) return 0;
    const qc_tab t = { bc, reads, umis };
    uint32_t *idx = (uint32_t *)malloc(n * sizeof *idx);
    if (!idx) { qc_err("out of memory"); return 1; }
    for (size_t i = 0; i < n; i++) idx[i] = (uint32_t)i;
    if (qc_sort(&t, idx, n)) { free(idx); return 1; }
    uint64_t T = arg, K = n;                                       /* called iff umis >= T and rank <= K */
    if (rule == 'e') {
        const uint64_t at = arg / 100 + 1 < n ? arg / 100 + 1 : n;
        const uint64_t m = umis[idx[at - 1]];
        T = (m + 5) / 10 > 1 ? (m + 5) / 10 : 1;
        *threshold = T;
    } else if (rule == 'k') {
        K = arg < n ? arg : n; T = 0;
        *threshold = umis[idx[K - 1]];
    }
    for (size_t r = 0; r < n; r++) {
        const uint32_t i = idx[r];
        if (rank) rank[i] = (uint32_t)r + 1;
        if (called) called[i] = (uint8_t)(r < K && umis[i] >= T);
    }
    free(idx);
    return 0;
}

/* ------------------------------------------------------------------ */
/* the rows of fqcells.tsv.gz, formatted slice by slice on the host threads  */
/* ------------------------------------------------------------------ */
static size_t put_u64(char *o, uint64_t v)
{
    char b[20]; size_t n = 0;
    do { b[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    for (size_t k = 0; k < n; k++) o[k] = b[n - 1 - k];
    return n;
}
static size_t put_row(char *o, uint32_t l, uint64_t bc, uint64_t reads, uint32_t umis, uint32_t rank, uint8_t called)
{
    size_t n = l;
    fq_decode_dna(bc, l, o);
    o[n++] = '\t'; n += put_u64(o + n, reads);
    o[n++] = '\t'; n += put_u64(o + n, umis);
    o[n++] = '\t'; n += put_u64(o + n, rank);
    o[n++] = '\t'; o[n++] = (char)('0' + called); o[n++] = '\n';
    return n;
}
#define QC_ROW_MAX (FQ_MAX_DNA + 20 + 10 + 10 + 6)
typedef struct { const uint64_t *bc, *reads; const uint32_t *umis, *rank; const uint8_t *called; size_t n; uint32_t l; int nt;
                 size_t *bytes; char *txt; } qc_text_job;
static void qc_text_worker(void *vp, int w)
{
    qc_text_job *j = (qc_text_job *)vp;
    const size_t lo = j->n * (size_t)w / (size_t)j->nt, hi = j->n * (size_t)(w + 1) / (size_t)j->nt;
    char row[QC_ROW_MAX];
    if (!j->txt) {                                                 /* first turn: the bytes of the slice */
        size_t b = 0;
        for (size_t i = lo; i < hi; i++) b += put_row(row, j->l, j->bc[i], j->reads[i], j->umis[i], j->rank[i], j->called[i]);
        j->bytes[w] = b;
        return;
    }
    char *o = j->txt + j->bytes[w];                                /* second turn: bytes[w] = where the slice starts */
    for (size_t i = lo; i < hi; i++) o += put_row(o, j->l, j->bc[i], j->reads[i], j->umis[i], j->rank[i], j->called[i]);
}
static const char QC_HEADER[] = "barcode\treads\tumis\trank\tcalled\n";
static int qc_rows_text(qc_text_job *j, char **txt, size_t *len)
{
    size_t bytes[65];
    j->nt = j->n < 65536 ? 1 : fastf_host_thread_count();
    if (j->nt < 1) j->nt = 1;
    if (j->nt > 64) j->nt = 64;
    j->bytes = bytes; j->txt = NULL;
    fastf_par_run(j->nt, qc_text_worker, j);
    size_t o = sizeof QC_HEADER - 1;
    for (int w = 0; w < j->nt; w++) { const size_t b = bytes[w]; bytes[w] = o; o += b; }
    j->txt = (char *)malloc(o + 1);
    if (!j->txt) { qc_err("out of memory (%zu bytes of rows)", o); return 1; }
    memcpy(j->txt, QC_HEADER, sizeof QC_HEADER - 1);
    fastf_par_run(j->nt, qc_text_worker, j);
    *txt = j->txt; *len = o;
    return 0;
}

/* ------------------------------------------------------------------ */
/* the command body                                                      */
/* ------------------------------------------------------------------ */
static const char *const QC_OUT[3] = {"fqcells.tsv.gz", "whitelist.txt", "fqcells_summary.tsv"};
static const int QC_WANT[3] = {1, 1, 1};

static int write_file(const char *path, const char *p, size_t len)
{
    FILE *f = fopen(path, "w");
    if (!f) { qc_err("cannot create %s: %s", path, strerror(errno)); return 1; }
    const int bad = fwrite(p, 1, len, f) != len;
    if (fclose(f) || bad) { qc_err("cannot write %s", path); return 1; }
    return 0;
}

int fastf_fqcells(const char *r1, const char *out_dir, uint32_t len_cellbarcode, uint32_t len_umi, int rule, uint64_t arg,
                  fastf_fqcells_summary_t *summary)
{
    if (!r1) { qc_err("fastf_fqcells: the R1 path is required"); return 1; }
    if ((int32_t)len_cellbarcode < 0 || (int32_t)len_umi < 0) { qc_err("fastf_fqcells: negative length (-l %d, -u %d)", (int32_t)len_cellbarcode, (int32_t)len_umi); return 1; }
    if (len_cellbarcode < 1) { qc_err("fastf_fqcells: the cell barcode has at least 1 base"); return 1; }
    if ((uint64_t)len_cellbarcode + len_umi > FQ_MAX_DNA) { qc_err("fastf_fqcells: -l %u + -u %u is more than %u bases (a key holds 31)", len_cellbarcode, len_umi, FQ_MAX_DNA); return 1; }
    if (rule != 'e' && rule != 'k' && rule != 'm') { qc_err("fastf_fqcells: the rule is 'e', 'k' or 'm'"); return 1; }
    if (!arg) { qc_err("fastf_fqcells: rule '%c' with the argument 0 (at least 1)", rule); return 1; }
    const char *dir = out_dir ? out_dir : ".";
    if (!fl_dir_writable(dir, QC_OUT, QC_WANT, 3)) { qc_err("fastf_fqcells: cannot write the outputs into directory %s", dir); return 1; }

    const int prof = getenv("FASTF_PROFILE") != NULL;
    const double t0 = fl_now();
    fq_src src; int src_open = 0;
    fastf_taghist_t *hist = NULL;
    uint64_t *bc = NULL, *reads = NULL; uint32_t *umis = NULL, *rank = NULL; uint8_t *called = NULL;
    char *txt = NULL, *wl = NULL;
    char paths[3][4096];
    int made[3] = {0, 0, 0}, rc = 1;
    size_t B = 0, txt_len = 0;
    double tp[5] = {0, 0, 0, 0, 0}, reduce_ms = 0, t_open = 0, t_table = 0, t_call = 0, t_text = 0, t_write = 0;
    fastf_fqcells_summary_t S; memset(&S, 0, sizeof S);
    S.rule = (uint64_t)rule; S.arg = arg;
    for (int f = 0; f < 3; f++) snprintf(paths[f], sizeof paths[f], "%s/%s", dir, QC_OUT[f]);

    if (fastf_fq_src_open(&src, r1)) goto done;
    src_open = 1;
    if (fastf_taghist_create(0, &hist)) goto done;
    t_open = fl_now() - t0;
    uint64_t n_bytes = 0;
    if (fastf_fq_dna_keys(&src, len_cellbarcode + len_umi, hist, &S.reads, &S.other, &n_bytes, tp)) goto done;
    {
        const double t = fl_now();
        if (fastf_fqcells_table(hist, len_umi, &bc, &reads, &umis, &B, &S.umis, &reduce_ms)) goto done;
        t_table = fl_now() - t;
    }
    S.barcodes = B;
    for (size_t i = 0; i < B; i++) S.counted += reads[i];
    if (S.counted + S.other != S.reads) {
        qc_err("fqcells: %llu counted and %llu other reads of %llu", (unsigned long long)S.counted, (unsigned long long)S.other, (unsigned long long)S.reads);
        goto done;
    }
    {
        const double t = fl_now();
        rank = (uint32_t *)malloc((B ? B : 1) * sizeof *rank); called = (uint8_t *)malloc(B ? B : 1);
        if (!rank || !called) { qc_err("out of memory"); goto done; }
        if (fastf_fqcells_call(bc, reads, umis, B, rule, arg, rank, called, &S.threshold)) goto done;
        for (size_t i = 0; i < B; i++) if (called[i]) { S.called++; S.called_reads += reads[i]; S.called_umis += umis[i]; }
        t_call = fl_now() - t;
    }
    {
        const double t = fl_now();
        qc_text_job j = { bc, reads, umis, rank, called, B, len_cellbarcode, 1, NULL, NULL };
        if (qc_rows_text(&j, &txt, &txt_len)) goto done;
        wl = (char *)malloc(S.called * (size_t)(len_cellbarcode + 1) + 1);
        if (!wl) { qc_err("out of memory"); goto done; }
        char *o = wl;
        for (size_t i = 0; i < B; i++) if (called[i]) { fq_decode_dna(bc[i], len_cellbarcode, o); o[len_cellbarcode] = '\n'; o += len_cellbarcode + 1; }
        t_text = fl_now() - t;
    }
    {
        const double t = fl_now();
        char sum[512];
        const int n = snprintf(sum, sizeof sum, "reads\tcounted\tother\tbarcodes\tumis\trule\targ\tthreshold\tcalled\tcalled_reads\tcalled_umis\n"
                               "%llu\t%llu\t%llu\t%llu\t%llu\t%c\t%llu\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)S.reads,
                               (unsigned long long)S.counted, (unsigned long long)S.other, (unsigned long long)S.barcodes,
                               (unsigned long long)S.umis, rule, (unsigned long long)S.arg, (unsigned long long)S.threshold,
                               (unsigned long long)S.called, (unsigned long long)S.called_reads, (unsigned long long)S.called_umis);
        made[0] = 1;
        if (fastf_write_gz_text(paths[0], txt, txt_len)) { qc_err("cannot write %s", paths[0]); goto done; }
        made[1] = 1;
        if (write_file(paths[1], wl, S.called * (size_t)(len_cellbarcode + 1))) goto done;
        made[2] = 1;
        if (write_file(paths[2], sum, (size_t)n)) goto done;
        t_write = fl_now() - t;
    }
    if (summary) *summary = S;
    rc = 0;
    if (prof) {
        fprintf(stderr, "[fqcells] %llu reads, %llu bytes of text, %llu counted, %llu distinct CB+UMI, %zu barcodes, %llu called, window %zu, "
                "%d host threads\n", (unsigned long long)S.reads, (unsigned long long)n_bytes, (unsigned long long)S.counted,
                (unsigned long long)S.umis, B, (unsigned long long)S.called, fastf_fq_window_bytes(), fastf_host_thread_count());
        fprintf(stderr, "[fqcells] open (HIP runtime + histogram) %.3f s, inflate/read %.3f s, H2D %.3f s (%.1f GB/s), parse %.3f s, pipeline "
                "wall %.3f s, push %.3f s, histogram + reduce + copy %.3f s (reduce window, its allocations and synchronise included, %.3f ms: %.1f GB/s "
                "of %llu x 12 + %zu x 20 bytes; the two passes read 20 bytes a key), call %.3f s, text %.3f s (%zu bytes), write %.3f s\n", t_open, tp[0], tp[1],
                tp[1] > 0 ? (double)n_bytes / tp[1] * 1e-9 : 0.0, tp[2], tp[3], tp[4], t_table, reduce_ms,
                reduce_ms > 0 ? ((double)S.umis * 12 + (double)B * 20) / (reduce_ms * 1e-3) * 1e-9 : 0.0, (unsigned long long)S.umis, B,
                t_call, t_text, txt_len, t_write);
    }
done:
    {
        char keep[768];
        if (rc) snprintf(keep, sizeof keep, "%s", fastf_last_error());
        if (src_open) fastf_fq_src_close(&src);
        if (hist) fastf_taghist_destroy(hist);
        if (rc) { for (int f = 0; f < 3; f++) if (made[f]) unlink(paths[f]); fastf_set_error_(keep); }   /* no partial outputs behind a refusal */
    }
    free(bc); free(reads); free(umis); free(rank); free(called); free(txt); free(wl);
    return rc;
}

/* ------------------------------------------------------------------ */
/* CLI: freq's dialect                                                   */
/* ------------------------------------------------------------------ */
static void qc_usage(void)
{
    printf("Usage: fastF fqcells [options]\n\nCall the cells of an R1 fastq file by UMIs per cell barcode.\n\n"
           "A read counts iff the first -l + -u bytes of its sequence line are all of ACGT; a barcode's UMIs are the distinct\n"
           "-u bases behind it.  Barcodes rank by UMIs, then reads (both descending), then bytes.  Writes fqcells.tsv.gz (every\n"
           "barcode: reads, umis, rank, called), whitelist.txt (the called barcodes, as filter -w and fqcap -w read them) and\n"
           "fqcells_summary.tsv into the output directory.\n\n"
           "    -h, --help          show this help message and exit\n\nBasic options\n"
           "    -R, --R1=<str>      required, path to R1 fastq files\n"
           "    -o, --out=<str>     dir to output the three files\n"
           "    -l, --len=<int>     length of cell barcode (default 16)\n"
           "    -u, --umi=<int>     length of UMI (default 10; -l + -u <= 31)\n\nCalling rule (one of; default -e 3000)\n"
           "    -e, --expect=<int>  expected cells E: T = a tenth (rounded) of the UMIs at rank E / 100 + 1, called iff umis >= T\n"
           "    -k, --top=<int>     the K barcodes of the highest rank\n"
           "    -m, --min=<int>     every barcode of at least M UMIs\n\n");
}

int cmd_fqcells(int argc, const char **argv)
{
    static const cli_opt opts[] = {{'h', "help", 0}, {'R', "R1", 1}, {'o', "out", 1}, {'l', "len", 1}, {'u', "umi", 1},
                                   {'e', "expect", 1}, {'k', "top", 1}, {'m', "min", 1}, {0, NULL, 0}};
    const char *r1 = NULL, *out = ".", *rule_val = NULL;
    int32_t len_cb = 16, len_umi = 10;
    int rule = 0, n_rules = 0;
    cli_scan S = CLI_SCAN(argc, argv, opts, CLI_ARGPARSE);
    for (const cli_opt *o; (o = cli_next(&S));)
        switch (o->s) {
        case 'h': qc_usage(); exit(0);
        case 'R': r1 = S.val; break;
        case 'o': out = S.val; break;
        case 'l': len_cb = (int)cli_int(&S); break;
        case 'u': len_umi = (int)cli_int(&S); break;
        case 'e': case 'k': case 'm': if (rule != o->s) n_rules++; rule = o->s; rule_val = S.val; break;
        }
    if (S.err) { if (S.err == CLI_UNKNOWN) qc_usage(); exit(EXIT_FAILURE); }
    if (r1 == NULL) { fprintf(stderr, "\x1b[31mError:\x1b[0m -R: the path to the R1 fastq file is required.\n"); exit(1); }
    if (len_cb < 0 || len_umi < 0) { fprintf(stderr, "\x1b[31mError:\x1b[0m -l %d -u %d: negative length (refused)\n", len_cb, len_umi); exit(1); }
    if (len_cb < 1) { fprintf(stderr, "\x1b[31mError:\x1b[0m -l %d: the cell barcode has at least 1 base (refused)\n", len_cb); exit(1); }
    if ((int64_t)len_cb + len_umi > (int64_t)FQ_MAX_DNA) {
        fprintf(stderr, "\x1b[31mError:\x1b[0m -l %d -u %d: more than %u bases of barcode and UMI (refused)\n", len_cb, len_umi, FQ_MAX_DNA);
        exit(1);
    }
    if (n_rules > 1) { fprintf(stderr, "\x1b[31mError:\x1b[0m -e, -k and -m: one calling rule at a time (refused)\n"); exit(1); }
    uint64_t arg = 3000;
    if (!rule) rule = 'e';
    else {
        const char *p = rule_val;
        int ok = *p != 0;
        for (arg = 0; *p && ok; p++) {
            if (*p < '0' || *p > '9' || arg > (UINT64_MAX - (uint64_t)(*p - '0')) / 10) ok = 0;
            else arg = arg * 10 + (uint64_t)(*p - '0');
        }
        if (!ok || !arg) { fprintf(stderr, "\x1b[31mError:\x1b[0m -%c %s: a whole number, digits only, at least 1.\n", rule, rule_val); exit(1); }
    }
    if (!fl_dir_writable(out, QC_OUT, QC_WANT, 3)) {
        fprintf(stderr, "\x1b[31mError:\x1b[0m -o: cannot write the outputs into directory %s (refused)\n", out);
        exit(1);
    }
    {
        const int fd = open(r1, O_RDONLY);
        if (fd < 0) { fprintf(stderr, "Cannot open file %s \n", r1); exit(1); }
        close(fd);
    }
    fastf_fqcells_summary_t sum;
    if (fastf_fqcells(r1, out, (uint32_t)len_cb, (uint32_t)len_umi, rule, arg, &sum)) {
        fprintf(stderr, "ERROR: fastF fqcells: %s\n", fastf_last_error());
        exit(1);
    }
    printf("fqcells: %llu reads, %llu counted, %llu barcodes, %llu called (-%c %llu: at least %llu UMIs)\n", (unsigned long long)sum.reads,
           (unsigned long long)sum.counted, (unsigned long long)sum.barcodes, (unsigned long long)sum.called, rule,
           (unsigned long long)sum.arg, (unsigned long long)sum.threshold);
    return 0;
}
