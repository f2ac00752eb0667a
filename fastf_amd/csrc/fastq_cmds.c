/*
 * fastq_cmds.c — `freq` on the tag-histogram engine.
 *
 * Drop-in symbols (same names, signatures and output bytes as the reference):
 *   node *cell_counts(gzFile R1_file, size_t len_cellbarcode, size_t len_umi)   count.c:3-21 (decl. count.h)
 *   int   cmd_freq(int argc, const char **argv)                                 main.c:30-92
 *
 * The reference reads the R1 FASTQ four gzgets() lines at a time (filter.c:15-37), inserts the first L = len_cb + len_umi
 * bytes of every sequence line into its insertion-order BST (filter.c:105-124) and prints the tree in pre-order as
 * "%s,%ld\n" (filter.c:139-148).  As for extract, the output is a function of the distinct strings, their counts and their
 * first occurrences.  Here the host only inflates: the text goes in windows through pinned staging to the device, which
 * frames the lines, checks them and packs one key per read into the histogram's key array (fastq_kernels.hpp); the host
 * turns the few reads that are not exactly L <= 31 bases of ACGT into strings (escape keys), and orders and prints the
 * histogram's result.  No CPU fallback.
 *
 * Declared divergences (the reference's behaviour is undefined or silently wrong there): a line longer than gzgets' 1023
 * bytes, a file that ends right after a header line, and a corrupt or truncated compressed stream are refused (exit 1).
 */
#define _GNU_SOURCE
#include "host_io.h"
#include "cli_opts.h"
#include "fastq_kernels.hpp"

#include <errno.h>
#include <stdarg.h>
#include <fcntl.h>
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>
#include <zlib.h>

int fastf_inflate_raw(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_len);   /* inflate_fast.c */
uint32_t fastf_crc32(const unsigned char *buf, size_t len);                               /* crc32_fast.c */

static double fq_now(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + t.tv_nsec * 1e-9; }
static void fq_err(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static void fq_err(const char *fmt, ...)
{
    char b[512];
    va_list ap; va_start(ap, fmt); vsnprintf(b, sizeof b, fmt, ap); va_end(ap);
    fastf_set_error_(b);
}

/* ------------------------------------------------------------------ */
/* decompressed text, whatever gzopen(path, "r") would read             */
/* ------------------------------------------------------------------ */
/* fq_src: host_io.h */

/* BGZF block at o: 0 and its geometry, or 1 (not a BGZF member) */
static int bgzf_block(const fq_src *s, size_t o, size_t *cdata, size_t *clen, size_t *bsize, uint32_t *isize)
{
    const unsigned char *p = s->map + o;
    if (s->map_len - o < 28 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || p[3] != 4) return 1;
    const size_t xlen = (size_t)p[10] | ((size_t)p[11] << 8);
    if (s->map_len - o < 12 + xlen) return 1;
    size_t bs = 0;
    for (size_t q = 12; q + 4 <= 12 + xlen;) {
        const size_t sl = (size_t)p[q + 2] | ((size_t)p[q + 3] << 8);
        if (p[q] == 'B' && p[q + 1] == 'C' && sl == 2 && q + 6 <= 12 + xlen) { bs = ((size_t)p[q + 4] | ((size_t)p[q + 5] << 8)) + 1; break; }
        q += 4 + sl;
    }
    if (!bs || bs < 12 + xlen + 8 || s->map_len - o < bs) return 1;
    *cdata = o + 12 + xlen; *clen = bs - 12 - xlen - 8; *bsize = bs;
    const unsigned char *t = p + bs - 4;
    *isize = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
    return *isize > 65536;
}

int fastf_fq_src_open(fq_src *s, const char *path)
{
    memset(s, 0, sizeof *s);
    s->fd = open(path, O_RDONLY | O_CLOEXEC);
    if (s->fd < 0) { fq_err("cannot open %s: %s", path, strerror(errno)); return 1; }
    struct stat st;
    if (fstat(s->fd, &st) != 0) { fq_err("cannot stat %s", path); close(s->fd); return 1; }
    unsigned char m[2] = {0, 0};
    const ssize_t got = st.st_size >= 2 ? pread(s->fd, m, 2, 0) : 0;
    s->nt = fastf_host_thread_count();
    if (got != 2 || m[0] != 0x1f || m[1] != 0x8b) { s->kind = FQ_PLAIN; return 0; }      /* zlib's direct mode (gz_look) */
    s->map_len = (size_t)st.st_size;
    s->map = (unsigned char *)mmap(NULL, s->map_len, PROT_READ, MAP_PRIVATE, s->fd, 0);
    if (s->map == MAP_FAILED) { s->map = NULL; fq_err("cannot map %s", path); close(s->fd); return 1; }
    (void)madvise(s->map, s->map_len, MADV_SEQUENTIAL);
    size_t a, b, c; uint32_t d;
    s->kind = bgzf_block(s, 0, &a, &b, &c, &d) == 0 ? FQ_BGZF : FQ_GZIP;
    return 0;
}

void fastf_fq_src_close(fq_src *s)
{
    if (s->z_live) inflateEnd(&s->z);
    if (s->map) munmap(s->map, s->map_len);
    if (s->kind != FQ_GZFILE && s->fd > 0) close(s->fd);
    memset(s, 0, sizeof *s);
}

/* gzip members from s->coff on, as zlib's gzread: a member follows only where the next two bytes are the gzip magic, anything
 * else behind a member is ignored (gz_look); a damaged or truncated member is an error here (zlib: EOF) */
static long gzip_fill(fq_src *s, unsigned char *out, size_t cap)
{
    size_t n = 0;
    if (!s->z_live) {
        if (inflateInit2(&s->z, 15 + 16) != Z_OK) { fq_err("inflateInit2 failed"); return -1; }
        s->z_live = 1; s->z_member_done = 1;
    }
    while (n < cap) {
        if (s->z_member_done) {
            if (s->map_len - s->coff < 2 || s->map[s->coff] != 0x1f || s->map[s->coff + 1] != 0x8b) break;
            inflateReset(&s->z);
            s->z_member_done = 0;
        }
        const size_t in_av = s->map_len - s->coff > (1u << 30) ? (1u << 30) : s->map_len - s->coff;
        const size_t out_av = cap - n > (1u << 30) ? (1u << 30) : cap - n;
        s->z.next_in = s->map + s->coff; s->z.avail_in = (uInt)in_av;
        s->z.next_out = out + n; s->z.avail_out = (uInt)out_av;
        const int r = inflate(&s->z, Z_NO_FLUSH);
        s->coff += in_av - s->z.avail_in;
        n += out_av - s->z.avail_out;
        if (r == Z_STREAM_END) { s->z_member_done = 1; continue; }
        if (r == Z_BUF_ERROR && s->z.avail_out == 0) continue;
        if (r != Z_OK || (in_av == s->z.avail_in && out_av == s->z.avail_out)) {
            fq_err("corrupt or truncated gzip stream at compressed offset %zu (%s)", s->coff, s->z.msg ? s->z.msg : (r == Z_BUF_ERROR ? "unexpected end of file" : "inflate error"));
            return -1;
        }
    }
    return (long)n;
}

typedef struct { const fq_src *s; const size_t *cdata, *clen; const uint32_t *isize, *crc; const size_t *uoff;
                 unsigned char *out; size_t n, next; int err; } bgzf_job;
static void bgzf_worker(void *vp, int w)
{
    (void)w;
    bgzf_job *j = (bgzf_job *)vp;
    z_stream z; memset(&z, 0, sizeof z);
    if (inflateInit2(&z, -15) != Z_OK) { j->err = 1; return; }
    for (;;) {
        size_t i = __atomic_fetch_add(&j->next, 8, __ATOMIC_RELAXED);
        if (i >= j->n || j->err) break;
        const size_t e = i + 8 < j->n ? i + 8 : j->n;
        for (; i < e; i++) {
            unsigned char *o = j->out + j->uoff[i];
            const unsigned char *in = j->s->map + j->cdata[i];
            if (!j->isize[i]) continue;
            /* own decoder first, zlib whenever it declines or the CRC disagrees (host_io.c inflate_worker) */
            if (fastf_inflate_raw(in, j->clen[i], o, j->isize[i]) == 0 && fastf_crc32(o, j->isize[i]) == j->crc[i]) continue;
            inflateReset(&z);
            z.next_in = (unsigned char *)in; z.avail_in = (uInt)j->clen[i];
            z.next_out = o; z.avail_out = j->isize[i];
            const int r = inflate(&z, Z_FINISH);
            if (r != Z_STREAM_END || z.avail_out != 0 || fastf_crc32(o, j->isize[i]) != j->crc[i]) { __atomic_store_n(&j->err, 1, __ATOMIC_RELAXED); break; }
        }
    }
    inflateEnd(&z);
}

static uint32_t rd32(const unsigned char *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

/* BGZF blocks that fit whole into the window, inflated on the host threads; a block that does not fit any more is inflated
 * into the spill and dealt out from there.  A member that is not BGZF hands the rest of the file to gzip_fill. */
static long bgzf_fill(fq_src *s, unsigned char *out, size_t cap)
{
    size_t n = 0;
    if (s->spill_off < s->spill_len) {
        const size_t k = s->spill_len - s->spill_off < cap ? s->spill_len - s->spill_off : cap;
        memcpy(out, s->spill + s->spill_off, k); s->spill_off += k; n += k;
        if (n == cap) return (long)n;
    }
    size_t nb = 0, cb = 1024;
    size_t *cdata = (size_t *)malloc(cb * sizeof *cdata), *clen = (size_t *)malloc(cb * sizeof *clen), *uoff = (size_t *)malloc(cb * sizeof *uoff);
    uint32_t *isize = (uint32_t *)malloc(cb * sizeof *isize), *crc = (uint32_t *)malloc(cb * sizeof *crc);
    long rc = -1;
    int switch_to_gzip = 0;
    if (!cdata || !clen || !uoff || !isize || !crc) { fq_err("out of memory"); goto done; }
    size_t u = n;
    while (s->coff < s->map_len) {
        size_t cd, cl, bs; uint32_t is;
        if (bgzf_block(s, s->coff, &cd, &cl, &bs, &is)) { switch_to_gzip = 1; break; }
        if (u + is > cap) break;
        if (nb == cb) {
            cb *= 2;
            cdata = (size_t *)realloc(cdata, cb * sizeof *cdata); clen = (size_t *)realloc(clen, cb * sizeof *clen);
            uoff = (size_t *)realloc(uoff, cb * sizeof *uoff); isize = (uint32_t *)realloc(isize, cb * sizeof *isize);
            crc = (uint32_t *)realloc(crc, cb * sizeof *crc);
            if (!cdata || !clen || !uoff || !isize || !crc) { fq_err("out of memory"); goto done; }
        }
        cdata[nb] = cd; clen[nb] = cl; isize[nb] = is; crc[nb] = rd32(s->map + s->coff + bs - 8); uoff[nb] = u;
        u += is; nb++;
        s->coff += bs;
    }
    if (nb) {
        bgzf_job j = { s, cdata, clen, isize, crc, uoff, out, nb, 0, 0 };
        int nt = s->nt;
        if ((size_t)nt > (nb + 7) / 8) nt = (int)((nb + 7) / 8);
        fastf_par_run(nt < 1 ? 1 : nt, bgzf_worker, &j);
        if (j.err) { fq_err("corrupt BGZF block in compressed bytes %zu..%zu", cdata[0], s->coff); goto done; }
    }
    n = u;
    if (n < cap && !switch_to_gzip && s->coff < s->map_len) {           /* the next block does not fit: through the spill */
        size_t cd, cl, bs; uint32_t is;
        if (bgzf_block(s, s->coff, &cd, &cl, &bs, &is) == 0) {
            bgzf_job j = { s, &cd, &cl, &is, NULL, NULL, s->spill, 1, 0, 0 };
            uint32_t c = rd32(s->map + s->coff + bs - 8); size_t zero = 0;
            j.crc = &c; j.uoff = &zero;
            bgzf_worker(&j, 0);
            if (j.err) { fq_err("corrupt BGZF block at compressed offset %zu", s->coff); goto done; }
            s->coff += bs;
            s->spill_len = is; s->spill_off = cap - n < is ? cap - n : is;
            memcpy(out + n, s->spill, s->spill_off); n += s->spill_off;
        } else switch_to_gzip = 1;
    }
    if (switch_to_gzip && n < cap) {
        s->kind = FQ_GZIP;
        const long g = gzip_fill(s, out + n, cap - n);
        if (g < 0) goto done;
        n += (size_t)g;
    } else if (switch_to_gzip) s->kind = FQ_GZIP;
    rc = (long)n;
done:
    free(cdata); free(clen); free(uoff); free(isize); free(crc);
    return rc;
}

/* up to cap bytes of text; fewer only at the end of the data.  -1 on error. */
long fastf_fq_src_fill(fq_src *s, unsigned char *out, size_t cap)
{
    size_t n = 0;
    switch (s->kind) {
    case FQ_PLAIN:
        while (n < cap) {
            const ssize_t r = pread(s->fd, out + n, cap - n, (off_t)s->pos);
            if (r < 0) { if (errno == EINTR) continue; fq_err("read error: %s", strerror(errno)); return -1; }
            if (r == 0) break;
            n += (size_t)r; s->pos += (uint64_t)r;
        }
        return (long)n;
    case FQ_GZIP: return gzip_fill(s, out, cap);
    case FQ_BGZF: return bgzf_fill(s, out, cap);
    case FQ_GZFILE:
        while (n < cap) {
            const size_t want = cap - n > (1u << 30) ? (1u << 30) : cap - n;
            const int r = gzread(s->gz, out + n, (unsigned)want);
            if (r < 0) { int e; fq_err("gzread: %s", gzerror(s->gz, &e)); return -1; }
            if (r == 0) break;
            n += (size_t)r;
        }
        return (long)n;
    }
    return -1;
}

/* ------------------------------------------------------------------ */
/* escape strings: one table per run, key = 1 + ordinal                 */
/* ------------------------------------------------------------------ */
typedef struct {
    char *pool; size_t pool_len, pool_cap;
    size_t *off; uint32_t *len; uint64_t n, cap;      /* ordinal -> string */
    uint64_t *slot; uint64_t mask;                    /* open addressing: 1 + ordinal, 0 empty */
} esc_tab;

static uint64_t fq_hash(const unsigned char *p, size_t n)
{
    uint64_t h = 1469598103934665603ull ^ n;
    for (size_t i = 0; i < n; i++) { h ^= p[i]; h *= 1099511628211ull; }
    return h ^ (h >> 29);
}
static int esc_grow(esc_tab *t)
{
    const uint64_t nm = t->mask ? t->mask * 2 + 1 : 1023;
    uint64_t *ns = (uint64_t *)calloc(nm + 1, sizeof *ns);
    if (!ns) return 1;
    for (uint64_t i = 0; i < t->n; i++) {
        uint64_t h = fq_hash((const unsigned char *)t->pool + t->off[i], t->len[i]) & nm;
        while (ns[h]) h = (h + 1) & nm;
        ns[h] = i + 1;
    }
    free(t->slot); t->slot = ns; t->mask = nm;
    return 0;
}
/* key of the string p[0, n); 0 on out of memory */
static uint64_t esc_intern(esc_tab *t, const unsigned char *p, size_t n)
{
    if ((t->n + 1) * 2 > t->mask && esc_grow(t)) return 0;
    uint64_t h = fq_hash(p, n) & t->mask;
    while (t->slot[h]) {
        const uint64_t i = t->slot[h] - 1;
        if (t->len[i] == n && memcmp(t->pool + t->off[i], p, n) == 0) return i + 1;
        h = (h + 1) & t->mask;
    }
    if (t->n == t->cap) {
        t->cap = t->cap ? t->cap * 2 : 1024;
        t->off = (size_t *)realloc(t->off, t->cap * sizeof *t->off); t->len = (uint32_t *)realloc(t->len, t->cap * sizeof *t->len);
        if (!t->off || !t->len) return 0;
    }
    if (t->pool_len + n + 1 > t->pool_cap) {
        while (t->pool_len + n + 1 > t->pool_cap) t->pool_cap = t->pool_cap ? t->pool_cap * 2 : (1u << 16);
        t->pool = (char *)realloc(t->pool, t->pool_cap);
        if (!t->pool) return 0;
    }
    memcpy(t->pool + t->pool_len, p, n); t->pool[t->pool_len + n] = 0;
    t->off[t->n] = t->pool_len; t->len[t->n] = (uint32_t)n; t->pool_len += n + 1;
    t->slot[h] = ++t->n;
    return t->n;
}
static void esc_free(esc_tab *t) { free(t->pool); free(t->off); free(t->len); free(t->slot); memset(t, 0, sizeof *t); }

/* ------------------------------------------------------------------ */
/* one run: text windows -> device keys -> histogram                    */
/* ------------------------------------------------------------------ */
typedef struct {
    uint64_t n_reads;
    uint32_t m;                                       /* distinct strings, in strcmp order: */
    const char **strs; uint64_t *first, *count;
    char *dna_pool; esc_tab esc;
} fq_result;

static void fq_result_free(fq_result *r)
{
    free(r->strs); free(r->first); free(r->count); free(r->dna_pool); esc_free(&r->esc);
    memset(r, 0, sizeof *r);
}

typedef struct { uint64_t *rk; size_t n, cap; } rk_list;
static int rk_push(rk_list *l, uint64_t r, uint64_t k)
{
    if (l->n == l->cap) {
        l->cap = l->cap ? l->cap * 2 : (1u << 16);
        uint64_t *p = (uint64_t *)realloc(l->rk, l->cap * 2 * sizeof *p);
        if (!p) return 1;
        l->rk = p;
    }
    l->rk[2 * l->n] = r; l->rk[2 * l->n + 1] = k; l->n++;
    return 0;
}

/* the escapes of one window: strings from the host's own copy of it (staging = FQ_HDR bytes before the window + the window) */
static int fq_escapes(esc_tab *t, rk_list *l, const unsigned char *staging, uint64_t a, uint64_t len, const fastf_fq_esc_t *e,
                      uint32_t n, uint32_t L)
{
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t s = e[i].s;
        if (s + (FQ_HDR - 1) < a || s > a + len) { fq_err("fastq parse: escape outside its window"); return 1; }
        const unsigned char *p = staging + FQ_HDR + s - a;
        const uint32_t k = fq_escape_len(p, a + len - s, L);
        const uint64_t key = esc_intern(t, p, k);
        if (!key || rk_push(l, e[i].r, key)) { fq_err("out of memory (escape strings)"); return 1; }
    }
    return 0;
}

size_t fastf_fq_window_bytes(void)
{
    const char *e = getenv("FASTF_FQ_WINDOW");
    size_t w = (size_t)32 << 20;
    if (e && *e) {
        char *end = NULL;
        unsigned long long v = strtoull(e, &end, 0);
        if (end && (*end == 'k' || *end == 'K')) v <<= 10; else if (end && (*end == 'm' || *end == 'M')) v <<= 20;
        if (v >= 4096 && v <= ((size_t)1 << 30)) w = (size_t)v;
    }
    return w;
}

static int fq_cmp_str(const void *a, const void *b) { return strcmp(*(const char *const *)a, *(const char *const *)b); }

typedef struct { char *pool; const uint64_t *keys; size_t n; uint32_t L; int nt; } decode_dna_job;
static void decode_dna_worker(void *vp, int w)
{
    decode_dna_job *j = (decode_dna_job *)vp;
    const size_t lo = j->n * (size_t)w / (size_t)j->nt, hi = j->n * (size_t)(w + 1) / (size_t)j->nt;
    for (size_t i = lo; i < hi; i++) { char *o = j->pool + i * (j->L + 1); fq_decode_dna(j->keys[i], j->L, o); o[j->L] = 0; }
}

static int tprof(void) { return getenv("FASTF_PROFILE") != NULL; }

/* after the last window of a text of T bytes: the declared divergences (a line over FQ_MAX_LINE bytes, a file that ends after a header
 * line) and the histogram's limit are refused; *n_reads = the reads of the file.  freq and fqcells (fastf_fq_dna_keys) share it. */
static int fq_end_checks(fastf_fqparse_t *fp, uint64_t T, uint64_t *n_reads)
{
    uint64_t n_nl = 0, line_start = 0, err_rec = 0; uint32_t err = 0;
    if (fastf_fqparse_end(fp, &n_nl, &line_start, &err, &err_rec)) return 1;
    const int open_line = T > line_start;
    if (!(err & FQ_ERR_LONG_LINE) && open_line && T - line_start > FQ_MAX_LINE) { err |= FQ_ERR_LONG_LINE; err_rec = n_nl / 4; }
    if (err & FQ_ERR_LONG_LINE) {
        fq_err("read %llu (line %llu of the file) has a line longer than %u bytes: gzgets(buf, 1024) would split it (refused)",
               (unsigned long long)err_rec + 1, (unsigned long long)err_rec * 4 + 1, FQ_MAX_LINE);
        return 1;
    }
    const uint64_t n_lines = n_nl + (uint64_t)open_line;
    if (n_lines % 4 == 1) {
        fq_err("the file ends after the header line of read %llu: it has no sequence line (the reference reads an "
               "uninitialised buffer there; refused)", (unsigned long long)(n_lines / 4 + 1));
        return 1;
    }
    *n_reads = (n_lines + 3) / 4;
    if (*n_reads >= (1ull << 32) - 1) { fq_err("more than 2^32-2 reads"); return 1; }
    return 0;
}

static int fq_run(fq_src *src, size_t len_cb, size_t len_umi, fq_result *res)
{
    memset(res, 0, sizeof *res);
    /* substring(seq, 0, len_cellbarcode + len_umi) takes an int (filter.c:260): the sum modulo 2^32 */
    const int32_t Li = (int32_t)(uint32_t)(len_cb + len_umi);
    if (Li < 0) { fq_err("len_cellbarcode + len_umi = %d: negative length (malloc(%d) in substring, filter.c:262)", Li, Li + 1); return 1; }
    const uint32_t L = (uint32_t)Li > FQ_HDR ? FQ_HDR : (uint32_t)Li;      /* no key string is longer than a line */
    const int prof = tprof();
    const double t0 = fq_now();
    double t_fill = 0, t_wait_create = 0, t_escape = 0, h2d_ms = 0, parse_ms = 0;
    const size_t W = fastf_fq_window_bytes();
    unsigned char *stage[2] = {NULL, NULL};
    fastf_fqparse_t *fp = NULL;
    fastf_taghist_t *hist = NULL;
    rk_list rk = {0};
    int rc = 1;
    uint64_t win_a[2] = {0, 0}, win_len[2] = {0, 0};
    uint64_t a = 0, known_nl = 0, b_known = 0;
    fastf_taghist_result_t hr;

    /* the HIP runtime and the histogram first: the staging is pinned memory */
    if (fastf_taghist_create(0, &hist)) goto done;
    t_wait_create = fq_now() - t0;
    for (int i = 0; i < 2; i++) {
        stage[i] = (unsigned char *)fastf_pinned_alloc(FQ_HDR + W + 64);
        if (!stage[i]) goto done;
        memset(stage[i], 0, FQ_HDR);
    }
    if (fastf_fqparse_create(hist, W, L, &fp)) goto done;
    for (uint64_t k = 0, last = 0; !last; k++) {
        const int par = (int)(k & 1);
        /* window k - 2 had this staging: its escapes first, then the staging is free */
        const fastf_fq_esc_t *e = NULL; uint32_t ne = 0; uint64_t nl = 0;
        if (k >= 2) {
            if (fastf_fqparse_wait(fp, par, &e, &ne, &nl, &h2d_ms, &parse_ms)) goto done;
            const double te = fq_now();
            if (fq_escapes(&res->esc, &rk, stage[par], win_a[par], win_len[par], e, ne, L)) goto done;
            t_escape += fq_now() - te;
            known_nl = nl; b_known = win_a[par] + win_len[par];
        }
        if (k) memcpy(stage[par], stage[par ^ 1] + win_len[par ^ 1], FQ_HDR);
        const double tf = fq_now();
        const long n = fastf_fq_src_fill(src, stage[par] + FQ_HDR, W);
        t_fill += fq_now() - tf;
        if (n < 0) goto done;
        last = (size_t)n < W;
        /* reads that can have begun by the end of this window: every read takes four '\n' */
        const uint64_t bound = (known_nl + (a + (uint64_t)n - b_known)) / 4 + 2;
        if (fastf_fqparse_submit(fp, stage[par], (size_t)n, a, (int)last, bound)) goto done;
        win_a[par] = a; win_len[par] = (uint64_t)n;
        a += (uint64_t)n;
        if (last) {
            /* the last two windows, oldest first */
            for (int q = 1; q >= 0; q--) {
                const int pp = (int)((k + (uint64_t)q) & 1);          /* q = 1: window k - 1, q = 0: window k */
                if (q == 1 && k == 0) continue;
                if (fastf_fqparse_wait(fp, pp, &e, &ne, &nl, &h2d_ms, &parse_ms)) goto done;
                const double te = fq_now();
                if (fq_escapes(&res->esc, &rk, stage[pp], win_a[pp], win_len[pp], e, ne, L)) goto done;
                t_escape += fq_now() - te;
            }
        }
    }
    const double t_parse_end = fq_now();
    if (fq_end_checks(fp, a, &res->n_reads)) goto done;
    const double th0 = fq_now();
    if (res->n_reads == 0) { rc = 0; goto done; }                   /* no reads: an empty whitelist */
    if (fastf_fqparse_scatter(fp, rk.rk, rk.n, res->n_reads)) goto done;
    {
        uint64_t *d = fastf_taghist_reserve_device(hist, res->n_reads);
        if (!d || fastf_taghist_push_device(hist, d, res->n_reads)) goto done;
    }
    if (fastf_taghist_finish(hist, &hr)) goto done;
    const double t_hist = fq_now() - th0;
    const double tt0 = fq_now();
    {
        const uint32_t m = (uint32_t)hr.n1;
        uint32_t e = 0;
        while (e < m && hr.key1[e] < FQ_DNA_TAG) e++;                /* escape keys first, DNA keys (in strcmp order) behind */
        res->m = m;
        res->strs = (const char **)malloc((m ? m : 1) * sizeof *res->strs);
        res->first = (uint64_t *)malloc((m ? m : 1) * sizeof *res->first);
        res->count = (uint64_t *)malloc((m ? m : 1) * sizeof *res->count);
        const char **es = (const char **)malloc((e ? e : 1) * sizeof *es);
        uint32_t *eidx = (uint32_t *)malloc((e ? e : 1) * sizeof *eidx);
        res->dna_pool = (char *)malloc((size_t)(m - e) * (L + 1) + 1);
        if (!res->strs || !res->first || !res->count || !es || !eidx || !res->dna_pool) { free(es); free(eidx); fq_err("out of memory"); goto done; }
        decode_dna_job dj = { res->dna_pool, hr.key1 + e, m - e, L, m - e < 65536 ? 1 : fastf_host_thread_count() };
        fastf_par_run(dj.nt, decode_dna_worker, &dj);
        for (uint32_t i = 0; i < e; i++) {
            if (hr.key1[i] == 0 || hr.key1[i] > res->esc.n) { free(es); free(eidx); fq_err("fastq parse: unknown escape key"); goto done; }
            es[i] = res->esc.pool + res->esc.off[hr.key1[i] - 1];
        }
        /* escape strings in strcmp order (their indices travel along: sort pointers, then find the index by address) */
        for (uint32_t i = 0; i < e; i++) eidx[i] = i;
        {
            const char **tmp = (const char **)malloc((e ? e : 1) * sizeof *tmp);
            if (!tmp) { free(es); free(eidx); fq_err("out of memory"); goto done; }
            memcpy(tmp, es, (size_t)e * sizeof *tmp);
            qsort(tmp, e, sizeof *tmp, fq_cmp_str);
            /* es[i] are distinct pool addresses in ascending key (= pool) order: the index of tmp[q] by binary search */
            for (uint32_t q = 0; q < e; q++) {
                uint32_t lo = 0, hi = e;
                while (lo < hi) { const uint32_t mid = (lo + hi) / 2; if (es[mid] < tmp[q]) lo = mid + 1; else hi = mid; }
                eidx[q] = lo;
            }
            free(tmp);
        }
        /* merge the two strcmp-ordered runs */
        uint32_t i = 0, j = e, o = 0;
        while (i < e || j < m) {
            const char *dj_s = j < m ? res->dna_pool + (size_t)(j - e) * (L + 1) : NULL;
            uint32_t src_i;
            const char *sv;
            if (i < e && (j >= m || strcmp(es[eidx[i]], dj_s) < 0)) { src_i = eidx[i]; sv = es[src_i]; i++; }
            else { src_i = j; sv = dj_s; j++; }
            res->strs[o] = sv; res->first[o] = hr.first1[src_i]; res->count[o] = hr.count1[src_i]; o++;
        }
        free(es); free(eidx);
    }
    if (prof) {
        fprintf(stderr, "[freq] %llu reads, %llu bytes of text, %u distinct, %llu escapes (%llu strings), window %zu, %d host threads\n",
                (unsigned long long)res->n_reads, (unsigned long long)a, res->m, (unsigned long long)rk.n,
                (unsigned long long)res->esc.n, W, src->nt);
        fprintf(stderr, "[freq] open (HIP runtime + histogram) %.3f s, inflate/read %.3f s, H2D %.3f s (%.1f GB/s), parse %.3f s, "
                "escape strings %.3f s, pipeline wall %.3f s, histogram %.3f s, strings %.3f s\n",
                t_wait_create, t_fill, h2d_ms * 1e-3, h2d_ms > 0 ? (double)a / (h2d_ms * 1e-3) * 1e-9 : 0.0, parse_ms * 1e-3, t_escape,
                t_parse_end - t0 - t_wait_create, t_hist, fq_now() - tt0);
    }
    rc = 0;
done:
    if (rc) { char keep[512]; snprintf(keep, sizeof keep, "%s", fastf_last_error()); fq_result_free(res); fastf_set_error_(keep); }
    fastf_fqparse_destroy(fp);
    /* the result arrays above were copied out of the histogram: it can go */
    if (hist) fastf_taghist_destroy(hist);
    for (int i = 0; i < 2; i++) fastf_pinned_free(stage[i]);
    free(rk.rk);
    return rc;
}

/* fq_run's windows for a caller that wants the DNA-form keys alone (fqcells): the same source, staging, device
 * parse and end-of-file refusals (fq_end_checks), with L = len_cb + len_umi <= 31.  A read that is not DNA-form leaves key 0 in the histogram's key
 * array: no escape list comes to the host, nothing is interned or scattered.  The n_reads keys are pushed into hist (single-tag
 * mode); *n_other = the reads the device put on its escape lists.  t[0..4]: inflate/read, H2D, parse, pipeline wall, push (seconds). */
int fastf_fq_dna_keys(fq_src *src, uint32_t L, fastf_taghist_t *hist, uint64_t *n_reads, uint64_t *n_other, uint64_t *n_bytes, double t[5])
{
    const double t0 = fq_now();
    double t_fill = 0, h2d_ms = 0, parse_ms = 0;
    const size_t W = fastf_fq_window_bytes();
    unsigned char *stage[2] = {NULL, NULL};
    fastf_fqparse_t *fp = NULL;
    int rc = 1;
    uint64_t win_len[2] = {0, 0};
    uint64_t a = 0, known_nl = 0, b_known = 0, b_end[2] = {0, 0}, other = 0;
    *n_reads = 0; *n_other = 0;
    if (L < 1 || L > FQ_MAX_DNA) { fq_err("DNA-form keys hold 1 to %u bases, not %u", FQ_MAX_DNA, L); return 1; }
    for (int i = 0; i < 2; i++) {
        stage[i] = (unsigned char *)fastf_pinned_alloc(FQ_HDR + W + 64);
        if (!stage[i]) goto done;
        memset(stage[i], 0, FQ_HDR);
    }
    if (fastf_fqparse_create(hist, W, L, &fp)) goto done;
    for (uint64_t k = 0, last = 0; !last; k++) {
        const int par = (int)(k & 1);
        uint32_t ne = 0; uint64_t nl = 0;
        if (k >= 2) {                                                  /* window k - 2 had this staging */
            if (fastf_fqparse_wait_count(fp, par, &ne, &nl, &h2d_ms, &parse_ms)) goto done;
            other += ne; known_nl = nl; b_known = b_end[par];
        }
        if (k) memcpy(stage[par], stage[par ^ 1] + win_len[par ^ 1], FQ_HDR);
        const double tf = fq_now();
        const long n = fastf_fq_src_fill(src, stage[par] + FQ_HDR, W);
        t_fill += fq_now() - tf;
        if (n < 0) goto done;
        last = (size_t)n < W;
        const uint64_t bound = (known_nl + (a + (uint64_t)n - b_known)) / 4 + 2;    /* as fq_run: every read takes four '\n' */
        if (fastf_fqparse_zero_keys(fp, bound) || fastf_fqparse_submit(fp, stage[par], (size_t)n, a, (int)last, bound)) goto done;
        win_len[par] = (uint64_t)n;
        a += (uint64_t)n;
        b_end[par] = a;
    }
    for (int q = 0; q < 2; q++) {
        uint32_t ne = 0;
        if (fastf_fqparse_wait_count(fp, q, &ne, NULL, &h2d_ms, &parse_ms)) goto done;
        other += ne;
    }
    const double t_parse_end = fq_now();
    if (fq_end_checks(fp, a, n_reads)) goto done;
    if (*n_reads) {
        uint64_t *d = fastf_taghist_reserve_device(hist, *n_reads);
        if (!d || fastf_taghist_push_device(hist, d, *n_reads)) goto done;
    }
    *n_other = other;
    if (n_bytes) *n_bytes = a;
    if (t) { t[0] = t_fill; t[1] = h2d_ms * 1e-3; t[2] = parse_ms * 1e-3; t[3] = t_parse_end - t0; t[4] = fq_now() - t_parse_end; }
    rc = 0;
done:
    fastf_fqparse_destroy(fp);
    for (int i = 0; i < 2; i++) fastf_pinned_free(stage[i]);
    return rc;
}

static int fq_text(fq_result *r, char **txt, size_t *txt_len)
{
    const double t0 = fq_now();
    uint32_t *order = (uint32_t *)malloc((r->m ? r->m : 1) * sizeof *order);
    if (!order) { fq_err("out of memory"); return 1; }
    fastf_tag_tree_preorder(r->strs, r->first, r->m, order);       /* strs are in strcmp order already: no sort */
    const double t1 = fq_now();
    const int rc = fastf_tag_rows_text_(r->strs, r->count, order, r->m, txt, txt_len);
    free(order);
    if (rc) { fq_err("out of memory (whitelist text)"); return 1; }
    if (!*txt) *txt = (char *)calloc(1, 1);
    if (tprof()) fprintf(stderr, "[freq] tree order %.3f s, text %.3f s (%zu bytes)\n", t1 - t0, fq_now() - t1, *txt_len);
    return 0;
}

int fastf_freq_text(const char *fastq_file, size_t len_cellbarcode, size_t len_umi, char **txt, size_t *txt_len, uint64_t *n_reads)
{
    if (!fastq_file || !txt || !txt_len) { fq_err("null argument"); return 1; }
    fq_src src;
    if (fastf_fq_src_open(&src, fastq_file)) return 1;
    fq_result r;
    int rc = fq_run(&src, len_cellbarcode, len_umi, &r);
    fastf_fq_src_close(&src);
    if (rc) return 1;
    if (n_reads) *n_reads = r.n_reads;
    rc = fq_text(&r, txt, txt_len);
    fq_result_free(&r);
    return rc;
}

node *cell_counts(gzFile R1_file, size_t len_cellbarcode, size_t len_umi)
{
    fq_src src; memset(&src, 0, sizeof src);
    src.kind = FQ_GZFILE; src.gz = R1_file; src.fd = -1; src.nt = 1;
    fq_result r;
    if (fq_run(&src, len_cellbarcode, len_umi, &r)) {
        fprintf(stderr, "ERROR: fastF freq: %s\n", fastf_last_error());
        exit(1);
    }
    node *root = fastf_tag_tree_nodes_(r.strs, r.first, r.count, r.m);
    fq_result_free(&r);
    return root;
}

/* ------------------------------------------------------------------ */
/* CLI: main.c:30-92, the options scanned by cli_opts.c                 */
/* ------------------------------------------------------------------ */
static void fq_usage(void)
{
    printf("Usage: fastF freq [options]\n\nFind all the cell barcode whitelist and their frequencies.\n\n"
           "    -h, --help        show this help message and exit\n\nBasic options\n"
           "    -R, --R1=<str>    path to R1 fastq files\n"
           "    -o, --out=<str>   path to output whitelist\n"
           "    -l, --len=<int>   length of cell barcode\n"
           "    -u, --umi=<int>   length of UMI\n\n");
}

int cmd_freq(int argc, const char **argv)
{
    static const cli_opt opts[] = {{'h', "help", 0}, {'R', "R1", 1}, {'o', "out", 1}, {'l', "len", 1}, {'u', "umi", 1}, {0, NULL, 0}};
    const char *r1 = NULL, *out = NULL;
    size_t len_cb = 16, len_umi = 10;
    cli_scan S = CLI_SCAN(argc, argv, opts, CLI_ARGPARSE);
    for (const cli_opt *o; (o = cli_next(&S));)
        switch (o->s) {
        case 'h': fq_usage(); exit(0);
        case 'R': r1 = S.val; break;
        case 'o': out = S.val; break;
        case 'l': case 'u': {                                     /* an int into the low 4 bytes of a size_t: *(int *)opt->value = ... (argparse.c:88-92) */
            const int iv = (int)cli_int(&S);
            memcpy(o->s == 'l' ? &len_cb : &len_umi, &iv, sizeof iv);
            break; }
        }
    if (S.err) { if (S.err == CLI_UNKNOWN) fq_usage(); exit(EXIT_FAILURE); }
    if (r1 == NULL) { fprintf(stderr, "Please specify the path to R1 fastq files.\n"); exit(1); }   /* main.c:56-60 */
    {   /* gzopen(path, "r") (main.c:62-68) */
        const int fd = open(r1, O_RDONLY);
        if (fd < 0) { fprintf(stderr, "Cannot open file %s \n", r1); exit(1); }
        close(fd);
    }
    char path_out[1024];
    snprintf(path_out, sizeof path_out, "%s/whitelist.txt", out ? out : "(null)");        /* main.c:75-76 */
    {   /* the output's directory must take the file (checked before the input is read; the file itself comes after it) */
        char dir[1024];
        snprintf(dir, sizeof dir, "%s", out ? out : "(null)");
        struct stat st;
        if (stat(dir, &st) != 0 || !S_ISDIR(st.st_mode) || access(dir, W_OK | X_OK) != 0 ||
            (access(path_out, F_OK) == 0 && access(path_out, W_OK) != 0)) {
            fprintf(stderr, "Cannot open file %s \n", path_out);
            exit(1);
        }
    }
    char *txt = NULL; size_t len = 0; uint64_t n = 0;
    if (fastf_freq_text(r1, len_cb, len_umi, &txt, &len, &n)) {
        fprintf(stderr, "ERROR: fastF freq: %s\n", fastf_last_error());
        exit(1);
    }
    FILE *fp = fopen(path_out, "w");
    if (fp == NULL) { fprintf(stderr, "Cannot open file %s \n", path_out); exit(1); }
    if (fwrite(txt, 1, len, fp) != len) { fprintf(stderr, "Cannot write file %s \n", path_out); exit(1); }
    fclose(fp);
    free(txt);
    return 0;
}
