/*
 * filter_cmds.c — `filter` on the device.
 *
 * Drop-in symbols (same names, signatures and output bytes as the reference run sequentially):
 *   void fastF(gzFile in[3], gzFile out[3], node *tree, unsigned len, unsigned seed, float rate, bool all)   filter.c:286-350
 *   int  cmd_filter(int argc, const char **argv)                                                            main.c:94-228
 *
 * The reference reads one record of I1, R1 and R2 per iteration (gzgets, filter.c:15-60), draws (float) rand() / RAND_MAX
 * after srand(seed), and keeps the triple when the draw is below the rate and (-a, or some whitelist line's first len bytes
 * equal the sequence line's first len bytes, strncmp semantics).  A kept read appends "id seq +\n qual" to each output.
 *
 * Here R1 is read first, in windows through pinned staging to the device (filter_kernels.hpp), which frames the records,
 * draws glibc's rand() from chunk start states of the host's jump-ahead, looks the barcode up in the sorted DNA-form whitelist
 * keys, writes a keep bit per read into a bitmap in HBM and compacts the kept records into an output window; the host only
 * inflates, decides the few reads whose barcode is not exactly len <= 31 bases of ACGT (escapes) and deflates the output
 * windows as gzip members on its threads.  Then I1 and R2 are streamed against the bitmap by record index.  Memory: one
 * window of text, the device buffers of one window, and the bitmap (one bit per read).  No CPU fallback.
 *
 * Declared divergences (the reference's behaviour is undefined there): a line longer than gzgets' 1023 bytes, a file that ends
 * partway through a record, corrupt or truncated compressed input, a whitelist line longer than 98 bytes, a negative -l and an
 * -o directory that cannot be written are refused (exit 1).
 */
#define _GNU_SOURCE
#include "filter_host.h"
#include "cli_opts.h"

#include <errno.h>
#include <fcntl.h>
#include <pthread.h>
#include <stdarg.h>
#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>
#include <zlib.h>

#define DEG FLT_RAND_DEG

static void fl_err(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static void fl_err(const char *fmt, ...)
{
    char b[768];
    va_list ap; va_start(ap, fmt); vsnprintf(b, sizeof b, fmt, ap); va_end(ap);
    fastf_set_error_(b);
}

/* ------------------------------------------------------------------ */
/* glibc rand() (TYPE_3): r_0 = seed, r_i = 16807 r_{i-1} mod (2^31 - 1) for i < 31, r_i = r_{i-31} for i = 31..33,    */
/* r_i = r_{i-3} + r_{i-31} mod 2^32 from i = 34 on; output k = r_{k+344} >> 1                                     */
/* ------------------------------------------------------------------ */
/* B[j] = r_{3+j}, j < 31: the first 31 words from which the recurrence alone goes on */
static void rand_init(uint32_t seed, uint32_t B[DEG])           /* __srandom_r's LCG seeding */
{
    uint32_t r[DEG];
    if (seed == 0) seed = 1;
    int32_t word = (int32_t)seed;
    r[0] = (uint32_t)word;
    for (unsigned i = 1; i < DEG; i++) {
        const long hi = word / 127773, lo = word % 127773;
        word = (int32_t)(16807 * lo - 2836 * hi);
        if (word < 0) word += 2147483647;
        r[i] = (uint32_t)word;
    }
    for (unsigned j = 0; j < DEG; j++) B[j] = j + 3 < DEG ? r[j + 3] : r[j + 3 - DEG];
}

/* polynomials modulo x^31 - x^28 - 1 over Z/2^32 */
static void poly_mulmod(const uint32_t *a, const uint32_t *b, uint32_t *out)
{
    uint32_t t[2 * DEG - 1];
    memset(t, 0, sizeof t);
    for (unsigned i = 0; i < DEG; i++) {
        if (!a[i]) continue;
        for (unsigned j = 0; j < DEG; j++) t[i + j] += a[i] * b[j];
    }
    for (unsigned d = 2 * DEG - 2; d >= DEG; d--) { t[d - 3] += t[d]; t[d - DEG] += t[d]; }
    memcpy(out, t, DEG * sizeof *out);
}
static void poly_mulx(uint32_t *c)
{
    const uint32_t top = c[DEG - 1];
    memmove(c + 1, c, (DEG - 1) * sizeof *c);
    c[0] = top; c[28] += top;
}
static void poly_xpow(uint64_t n, uint32_t *out)
{
    uint32_t base[DEG], acc[DEG];
    memset(base, 0, sizeof base); memset(acc, 0, sizeof acc);
    base[1] = 1; acc[0] = 1;
    while (n) {
        if (n & 1) poly_mulmod(acc, base, acc);
        n >>= 1;
        if (n) poly_mulmod(base, base, base);
    }
    memcpy(out, acc, sizeof acc);
}
static uint32_t poly_apply(const uint32_t *c, const uint32_t *r)
{
    uint32_t v = 0;
    for (unsigned j = 0; j < DEG; j++) v += c[j] * r[j];
    return v;
}

/* the generator's state at output q: S[k] = r_{q+344+k} = r_{3 + (q+341+k)}, k < 31 */
void fl_gen_seek(rand_gen *g, uint32_t seed, uint64_t q)
{
    rand_init(seed, g->r0);
    uint32_t c[DEG];
    poly_xpow(q + 341, c);
    for (unsigned k = 0; k < DEG; k++) { g->S[k] = poly_apply(c, g->r0); poly_mulx(c); }
    g->q = q;
}
static void gen_step(rand_gen *g, uint64_t n)
{
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t v = g->S[0] + g->S[28];
        memmove(g->S, g->S + 1, (DEG - 1) * sizeof *g->S);
        g->S[DEG - 1] = v;
    }
    g->q += n;
}
/* the jump of one chunk: row k = x^(FLT_CHUNK + k) mod P (seed-independent) */
static uint32_t g_jump[DEG][DEG];
static void jump_init(void)
{
    uint32_t c[DEG];
    poly_xpow(FLT_CHUNK, c);
    for (unsigned k = 0; k < DEG; k++) { memcpy(g_jump[k], c, sizeof c); poly_mulx(c); }
}
/* start states of the ceil(n / FLT_CHUNK) chunks of outputs q .. q + n - 1 into cs; the generator moves on to q + n */
void fl_gen_chunks(rand_gen *g, uint64_t n, uint32_t *cs)
{
    static pthread_once_t once = PTHREAD_ONCE_INIT;
    pthread_once(&once, jump_init);
    const uint64_t nch = (n + FLT_CHUNK - 1) / FLT_CHUNK;
    for (uint64_t c = 0; c < nch; c++) {
        memcpy(cs + c * DEG, g->S, sizeof g->S);
        if (n - c * FLT_CHUNK >= FLT_CHUNK) {
            uint32_t nx[DEG];
            for (unsigned k = 0; k < DEG; k++) nx[k] = poly_apply(g_jump[k], g->S);
            memcpy(g->S, nx, sizeof nx);
            g->q += FLT_CHUNK;
        } else gen_step(g, n - c * FLT_CHUNK);
    }
}

uint32_t fastf_filter_rand_at(uint32_t seed, uint64_t index)
{
    rand_gen g;
    fl_gen_seek(&g, seed, index);
    return g.S[0] >> 1;
}

int fastf_filter_draws_host(uint32_t seed, uint64_t first, uint64_t n, uint32_t *out)
{
    if (!out && n) { fl_err("null argument"); return 1; }
    rand_gen g;
    fl_gen_seek(&g, seed, first);
    uint32_t S[2 * DEG];
    memcpy(S, g.S, sizeof g.S);
    for (uint64_t i = 0; i < n; i++) {                        /* the recurrence, one word at a time */
        const uint32_t v = S[0];
        out[i] = v >> 1;
        memmove(S, S + 1, (DEG - 1) * sizeof *S);
        S[DEG - 1] = v + S[27];
    }
    return 0;
}

int fastf_filter_draw_passes(uint32_t r, float rate) { return flt_draw_passes(r, rate); }

int fastf_filter_draws(uint32_t seed, uint64_t first, uint64_t n, uint32_t *out)
{
    if (!out && n) { fl_err("null argument"); return 1; }
    rand_gen g;
    fl_gen_seek(&g, seed, first);
    const uint64_t nch = (n + FLT_CHUNK - 1) / FLT_CHUNK;
    uint32_t *cs = (uint32_t *)malloc((nch ? nch : 1) * DEG * sizeof *cs);
    if (!cs) { fl_err("out of memory"); return 1; }
    fl_gen_chunks(&g, n, cs);
    const int rc = fastf_flt_draws_dev(0, cs, n, out);
    free(cs);
    return rc;
}

/* ------------------------------------------------------------------ */
/* whitelist: the first len bytes of every line (strncmp semantics)      */
/* ------------------------------------------------------------------ */
int fl_str_cmp(const void *a, const void *b)
{
    const fl_str *x = (const fl_str *)a, *y = (const fl_str *)b;
    const uint32_t m = x->n < y->n ? x->n : y->n;
    const int c = memcmp(x->p, y->p, m);
    return c ? c : (x->n > y->n) - (x->n < y->n);
}
static int u64_cmp(const void *a, const void *b)
{
    const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
    return (x > y) - (x < y);
}

/* the key of a string s[0, n) cut at len (n <= len: no NUL inside): DNA form or 0 */
static uint64_t dna_key(const unsigned char *s, size_t n, uint32_t len)
{
    if (len > FQ_MAX_DNA || n != len) return 0;
    uint64_t v = 0;
    for (uint32_t i = 0; i < len; i++) {
        const unsigned c = s[i];
        if (c != 'A' && c != 'C' && c != 'G' && c != 'T') return 0;
        v = (v << 2) | (((c >> 1) ^ (c >> 2)) & 3u);
    }
    return FQ_DNA_TAG | v;
}

void fl_wl_free(fl_wl *w) { free(w->dna); free(w->esc); free(w->pool); memset(w, 0, sizeof *w); }

/* lines as fgets(buf, 100) of read_txt returns them (each keeps its '\n'), cut at the first NUL and at len */
static int wl_add_lines(fl_wl *w, const char *const *lines, size_t n_lines, uint32_t len)
{
    w->dna = (uint64_t *)malloc((n_lines ? n_lines : 1) * sizeof *w->dna);
    w->esc = (fl_str *)malloc((n_lines ? n_lines : 1) * sizeof *w->esc);
    if (!w->dna || !w->esc) { fl_err("out of memory (whitelist)"); return 1; }
    for (size_t i = 0; i < n_lines; i++) {
        const char *s = lines[i];
        size_t n = strnlen(s, len);
        const uint64_t k = dna_key((const unsigned char *)s, n, len);
        if (k) w->dna[w->n_dna++] = k;
        else { w->esc[w->n_esc].p = s; w->esc[w->n_esc].n = (uint32_t)n; w->n_esc++; }
    }
    qsort(w->dna, w->n_dna, sizeof *w->dna, u64_cmp);
    size_t u = 0;
    for (size_t i = 0; i < w->n_dna; i++) if (!u || w->dna[u - 1] != w->dna[i]) w->dna[u++] = w->dna[i];
    w->n_dna = u;
    qsort(w->esc, w->n_esc, sizeof *w->esc, fl_str_cmp);
    w->nrow = n_lines;
    return 0;
}

/* get_row + read_txt (filter.c:181-226) of a whitelist file; keys = 0: the row count and the line-length check only */
int fl_wl_load(fl_wl *w, const char *path, uint32_t len, int keys)
{
    memset(w, 0, sizeof *w);
    FILE *f = fopen(path, "rb");
    if (!f) { fl_err("cannot open whitelist %s", path); return 2; }
    size_t cap = 1 << 20, n = 0;
    char *buf = (char *)malloc(cap + 1);
    for (;;) {
        if (!buf) { fclose(f); fl_err("out of memory (whitelist)"); return 1; }
        const size_t got = fread(buf + n, 1, cap - n, f);
        n += got;
        if (n < cap) break;
        cap *= 2;
        buf = (char *)realloc(buf, cap + 1);
    }
    fclose(f);
    buf[n] = 0;
    size_t n_lines = 0;
    for (size_t i = 0; i < n; i++) n_lines += buf[i] == '\n';
    if (n && buf[n - 1] != '\n') n_lines++;
    /* each line into the pool with its '\n' and a NUL behind */
    w->pool = (char *)malloc(n + n_lines + 1);
    const char **lines = (const char **)malloc((n_lines ? n_lines : 1) * sizeof *lines);
    if (!w->pool || !lines) { free(buf); free(lines); fl_err("out of memory (whitelist)"); return 1; }
    size_t o = 0, k = 0;
    for (size_t i = 0; i < n;) {
        const char *nl = (const char *)memchr(buf + i, '\n', n - i);
        const size_t e = nl ? (size_t)(nl - buf) + 1 : n;
        const size_t body = e - i - (nl ? 1 : 0);
        if (body > 98) {
            free(buf); free(lines);
            fl_err("whitelist %s: line %zu has %zu bytes before its newline; fgets(buf, 100) of the reference would split it "
                   "(at most 98 are supported; refused)", path, k + 1, body);
            return 1;
        }
        memcpy(w->pool + o, buf + i, e - i); w->pool[o + e - i] = 0;
        lines[k++] = w->pool + o;
        o += e - i + 1;
        i = e;
    }
    free(buf);
    w->nrow = k;
    const int rc = keys ? wl_add_lines(w, lines, k, len) : 0;
    free(lines);
    return rc;
}

static void tree_walk(const node *t, const char ***v, size_t *n, size_t *cap)
{
    while (t) {
        tree_walk(t->left, v, n, cap);
        if (*n == *cap) { *cap = *cap ? *cap * 2 : 1024; *v = (const char **)realloc(*v, *cap * sizeof **v); if (!*v) return; }
        (*v)[(*n)++] = t->data;
        t = t->right;
    }
}

/* ------------------------------------------------------------------ */
/* output: gzip members appended in order, or the caller's gzFile         */
/* ------------------------------------------------------------------ */
#define GZ_PIECE ((size_t)1 << 20)
typedef struct { const unsigned char *in; size_t len, n; unsigned char **out; size_t *out_len; size_t next; int err; } gz_job;
static void gz_worker(void *vp, int w)
{
    (void)w;
    gz_job *j = (gz_job *)vp;
    for (;;) {
        const size_t i = __atomic_fetch_add(&j->next, 1, __ATOMIC_RELAXED);
        if (i >= j->n) break;
        const size_t o = i * GZ_PIECE, m = j->len - o < GZ_PIECE ? j->len - o : GZ_PIECE;
        const size_t cap = fastf_gz_bound(m);
        j->out[i] = (unsigned char *)malloc(cap);
        j->out_len[i] = j->out[i] ? fastf_gz_member_fast(j->in + o, m, j->out[i], cap) : 0;
        if (!j->out_len[i]) __atomic_store_n(&j->err, 1, __ATOMIC_RELAXED);
    }
}
int fl_sink_write(fl_sink *s, const unsigned char *p, size_t len, double *t_deflate)
{
    if (!s || (!len && (s->gz || s->members))) return 0;
    const double t0 = fl_now();
    s->bytes_in += len;
    if (s->gz) {
        for (size_t o = 0; o < len;) {
            const unsigned m = len - o > (1u << 30) ? (1u << 30) : (unsigned)(len - o);
            if (gzwrite(s->gz, p + o, m) != (int)m) { fl_err("gzwrite failed"); return 1; }
            o += m;
        }
        *t_deflate += fl_now() - t0;
        return 0;
    }
    gz_job j; memset(&j, 0, sizeof j);
    j.in = p; j.len = len; j.n = len ? (len + GZ_PIECE - 1) / GZ_PIECE : 1;
    j.out = (unsigned char **)calloc(j.n, sizeof *j.out); j.out_len = (size_t *)calloc(j.n, sizeof *j.out_len);
    if (!j.out || !j.out_len) { free(j.out); free(j.out_len); fl_err("out of memory"); return 1; }
    int nt = fastf_host_thread_count();
    if ((size_t)nt > j.n) nt = (int)j.n;
    fastf_par_run(nt, gz_worker, &j);
    int rc = j.err ? (fl_err("gzip compression failed for %s", s->path), 1) : 0;
    for (size_t i = 0; i < j.n && !rc; i++)
        if (fwrite(j.out[i], 1, j.out_len[i], s->f) != j.out_len[i]) { fl_err("write error on %s", s->path); rc = 1; }
    for (size_t i = 0; i < j.n; i++) free(j.out[i]);
    free(j.out); free(j.out_len);
    s->members += (int)j.n;
    *t_deflate += fl_now() - t0;
    return rc;
}

/* ------------------------------------------------------------------ */
/* one file through the device                                           */
/* ------------------------------------------------------------------ */
static int esc_hit(const fl_wl *w, const unsigned char *p, size_t n)
{
    fl_str k = { (const char *)p, (uint32_t)n };
    return bsearch(&k, w->esc, w->n_esc, sizeof *w->esc, fl_str_cmp) != NULL;
}

/* mode 0: R1 (decides, *n_reads out; R->hk: another command's decision in filter's place); mode 1: I1 / R2 against the bitmap,
 * reads >= limit ignored.  `name` names the file in messages. */
int fl_file(fl_run *R, fq_src *src, int mode, uint64_t limit, const char *name, fl_sink *sink)
{
    fastf_fltdev_t *dev = R->dev;
    const size_t W = R->W;
    unsigned char *stage = R->stage;
    const fl_hooks *hk = mode == 0 ? R->hk : NULL;
    const int draws = mode == 0 && !(hk && hk->count_only);
    uint32_t *cs = NULL, *hits = NULL;
    size_t hits_cap = 0;
    rand_gen g;
    int rc = 1;
    uint64_t a = 0;
    if (fastf_fltdev_reset(dev)) return 1;
    if (draws) {
        fl_gen_seek(&g, R->seed, 0);
        cs = (uint32_t *)malloc(((W / 4 + 2) / FLT_CHUNK + 2) * DEG * sizeof *cs);
        if (!cs) { fl_err("out of memory"); return 1; }
    }
    memset(stage, 0, FLT_HDR);
    const uint32_t Lc = R->len > 1024 ? 1024 : R->len;
    for (int last = 0; !last;) {
        const double tf = fl_now();
        const long n = fastf_fq_src_fill(src, stage + FLT_HDR, W);
        R->t_fill += fl_now() - tf;
        if (n < 0) { char m[600]; snprintf(m, sizeof m, "%s: %s", name, fastf_last_error()); fl_err("%s", m); goto done; }
        last = (size_t)n < W;
        size_t len = (size_t)n;
        uint64_t tv = ~0ull;
        if (last) {
            const uint64_t T = a + len;
            const unsigned char lastc = len ? stage[FLT_HDR + len - 1] : stage[FLT_HDR - 1];
            if (T && lastc != '\n') { stage[FLT_HDR + len] = '\n'; tv = T; len++; }    /* closes the unterminated last line */
        }
        memset(stage + FLT_HDR + len, 0, 64);
        uint64_t r_lo = 0, n_rec = 0;
        if (fastf_fltdev_parse(dev, stage, len, a, tv, mode == 0 ? ~0ull : limit, &r_lo, &n_rec)) goto done;
        const fastf_flt_esc_t *e = NULL; uint32_t ne = 0;
        if (draws) {
            if (g.q != r_lo) { fl_err("filter: draw stream out of step (%llu vs %llu)", (unsigned long long)g.q, (unsigned long long)r_lo); goto done; }
            const double th = fl_now();
            fl_gen_chunks(&g, n_rec, cs);
            R->t_host += fl_now() - th;
        }
        if (hk ? hk->decide(hk->ctx, dev, R->len, cs, n_rec, &e, &ne)
               : fastf_fltdev_decide(dev, mode, R->all, R->len > 0xffffffffu ? 0xffffffffu : R->len, R->rate, cs, &e, &ne)) goto done;
        uint32_t nh = 0;
        if (ne) {
            const double th = fl_now();
            if (ne > hits_cap) { hits_cap = ne; free(hits); hits = (uint32_t *)malloc(hits_cap * sizeof *hits); if (!hits) { fl_err("out of memory"); goto done; } }
            for (uint32_t k = 0; k < ne; k++) {
                const unsigned char *p = stage + e[k].s1;
                const uint64_t gpos = a + e[k].s1 - FLT_HDR;
                const uint32_t m = fq_escape_len(p, a + len - gpos, Lc);
                const int hit = hk ? hk->escape(hk->ctx, dev, p, m, e[k].i) : esc_hit(R->wl, p, m);
                if (hit < 0) goto done;
                if (hit) hits[nh++] = e[k].i;
            }
            R->n_escapes += ne;
            R->t_host += fl_now() - th;
        }
        if (!(hk && hk->count_only)) {
            const unsigned char *out = NULL; size_t total = 0;
            if (fastf_fltdev_emit(dev, hits, nh, &out, &total)) goto done;
            if (total && fl_sink_write(sink, out, total, &R->t_deflate)) goto done;
        }
        memmove(stage, stage + len, FLT_HDR);                 /* the last FLT_HDR bytes of this window (len >= FLT_HDR or a zero prefix) */
        a += (uint64_t)n;
        if (mode == 1 && r_lo + n_rec >= limit) break;         /* the rest of the file is never read by the reference */
    }
    {
        uint64_t n_nl = 0, n_keep = 0, err_rec = 0; uint32_t err = 0; double ms = 0;
        if (fastf_fltdev_end(dev, &n_nl, &n_keep, &err, &err_rec, &ms)) goto done;
        R->dev_ms += ms;
        if (err && err_rec < limit) {
            fl_err("%s: read %llu (line %llu of the file) has a line longer than %u bytes: gzgets(buf, 1024) would split it (refused)",
                   name, (unsigned long long)err_rec + 1, (unsigned long long)err_rec * 4 + 1, FQ_MAX_LINE);
            goto done;
        }
        if (n_nl % 4 && n_nl / 4 < limit) {
            fl_err("%s: the file ends partway through read %llu (%llu of its 4 lines; the reference reads uninitialised buffers "
                   "there; refused)", name, (unsigned long long)(n_nl / 4 + 1), (unsigned long long)(n_nl % 4));
            goto done;
        }
        if (mode == 0) { R->n_reads = n_nl / 4; R->n_kept = n_keep; }
    }
    rc = 0;
done:
    free(cs); free(hits);
    return rc;
}

/* the three inputs (I1 / R2 may be NULL), outputs into the sinks (NULL for an absent input) */
static int fl_process(fq_src *src[3], const char *const names[3], fl_sink *sink[3], const fl_wl *wl, uint32_t len, uint32_t seed,
                      float rate, int all, uint64_t *n_reads, uint64_t *n_kept)
{
    const int prof = getenv("FASTF_PROFILE") != NULL;
    const double t0 = fl_now();
    fl_run R; memset(&R, 0, sizeof R);
    R.W = fastf_fq_window_bytes();
    if (R.W < FLT_HDR) R.W = FLT_HDR;
    R.len = len; R.all = all; R.rate = rate; R.seed = seed; R.wl = wl;
    int rc = 1;
    if (fastf_fltdev_create(0, R.W, &R.dev)) return 1;
    const double t_open = fl_now() - t0;
    R.stage = (unsigned char *)fastf_pinned_alloc(FLT_HDR + R.W + 128);
    if (!R.stage) goto done;
    if (fastf_fltdev_set_whitelist(R.dev, wl ? wl->dna : NULL, wl ? wl->n_dna : 0)) goto done;
    double t_file[3] = {0, 0, 0};
    {
        const double t = fl_now();
        if (fl_file(&R, src[1], 0, ~0ull, names[1], sink[1])) goto done;
        t_file[1] = fl_now() - t;
    }
    for (int f = 0; f <= 2; f += 2) {
        if (!src[f]) continue;
        const double t = fl_now();
        if (fl_file(&R, src[f], 1, R.n_reads, names[f], sink[f])) goto done;
        t_file[f] = fl_now() - t;
    }
    if (n_reads) *n_reads = R.n_reads;
    if (n_kept) *n_kept = R.n_kept;
    if (prof)
        fprintf(stderr, "[filter] %llu reads, window %zu, %d host threads: open %.3f s, R1 %.3f s, I1 %.3f s, R2 %.3f s; "
                "inflate/read %.3f s, deflate/write %.3f s, host draws + escapes %.3f s (%llu escapes), device %.3f s\n",
                (unsigned long long)R.n_reads, R.W, fastf_host_thread_count(), t_open, t_file[1], t_file[0], t_file[2],
                R.t_fill, R.t_deflate, R.t_host, (unsigned long long)R.n_escapes, R.dev_ms * 1e-3);
    rc = 0;
done:
    if (rc) { char keep[768]; snprintf(keep, sizeof keep, "%s", fastf_last_error()); fastf_fltdev_destroy(R.dev); fastf_set_error_(keep); }
    else fastf_fltdev_destroy(R.dev);
    fastf_pinned_free(R.stage);
    return rc;
}

/* ------------------------------------------------------------------ */
/* entry points                                                          */
/* ------------------------------------------------------------------ */
int fl_sink_open(fl_sink *s, const char *dir, const char *name, char *path, size_t path_cap)
{
    memset(s, 0, sizeof *s);
    snprintf(path, path_cap, "%s/%s", dir, name);
    s->path = path;
    s->f = fopen(path, "wb");
    if (!s->f) { fl_err("cannot open %s for writing: %s", path, strerror(errno)); return 1; }
    return 0;
}
int fl_sink_close(fl_sink *s)
{
    if (!s->f) return 0;
    int rc = 0;
    if (!s->members) {                                        /* nothing kept: still a valid (empty) gzip file */
        double t = 0;
        rc = fl_sink_write(s, (const unsigned char *)"", 0, &t);
    }
    if (fclose(s->f) != 0 && !rc) { fl_err("close error on %s", s->path); rc = 1; }
    s->f = NULL;
    return rc;
}

int fastf_filter(const char *r1, const char *i1, const char *r2, const char *out_dir, const char *whitelist, uint32_t len_cellbarcode,
                 uint32_t seed, float rate, int all_cells, uint64_t *n_reads, uint64_t *n_kept)
{
    if (!r1) { fl_err("fastf_filter: the R1 path is required"); return 1; }
    if (!whitelist && !all_cells) { fl_err("fastf_filter: give a whitelist or all_cells"); return 1; }
    if ((int32_t)len_cellbarcode < 0) { fl_err("fastf_filter: negative barcode length %d", (int32_t)len_cellbarcode); return 1; }
    const char *dir = out_dir ? out_dir : ".";
    fl_wl wl; memset(&wl, 0, sizeof wl);
    fq_src src_s[3]; fq_src *src[3] = {NULL, NULL, NULL};
    fl_sink sink_s[3]; fl_sink *sink[3] = {NULL, NULL, NULL};
    char paths[3][4096];
    const char *in[3] = {i1, r1, r2};
    static const char *const outname[3] = {"I1.fastq.gz", "R1.fastq.gz", "R2.fastq.gz"};
    int rc = 1;
    memset(src_s, 0, sizeof src_s); memset(sink_s, 0, sizeof sink_s);
    if (whitelist && fl_wl_load(&wl, whitelist, len_cellbarcode, 1)) goto done;
    for (int f = 0; f < 3; f++) {
        if (!in[f]) continue;
        if (fastf_fq_src_open(&src_s[f], in[f])) goto done;
        src[f] = &src_s[f];
    }
    for (int f = 0; f < 3; f++) {
        if (!in[f]) continue;
        if (fl_sink_open(&sink_s[f], dir, outname[f], paths[f], sizeof paths[f])) goto done;
        sink[f] = &sink_s[f];
    }
    if (fl_process(src, in, sink, &wl, len_cellbarcode, seed, rate, all_cells, n_reads, n_kept)) goto done;
    rc = 0;
    for (int f = 0; f < 3; f++) if (sink[f] && fl_sink_close(sink[f])) rc = 1;
done:
    for (int f = 0; f < 3; f++) { if (sink[f]) { if (sink[f]->f) fclose(sink[f]->f); } if (src[f]) fastf_fq_src_close(src[f]); }
    fl_wl_free(&wl);
    return rc;
}

void fastF(gzFile file_in[3], gzFile file_out[3], node *tree_whitelist, unsigned int len_cellbarcode, unsigned int seed, float rate,
           bool all_cell)
{
    fl_wl wl; memset(&wl, 0, sizeof wl);
    const char **v = NULL; size_t n = 0, cap = 0;
    tree_walk(tree_whitelist, &v, &n, &cap);
    if (n && !v) { fprintf(stderr, "ERROR: fastF filter: out of memory\n"); exit(1); }
    if ((int32_t)len_cellbarcode < 0) {
        fprintf(stderr, "ERROR: fastF filter: negative barcode length %d (refused)\n", (int32_t)len_cellbarcode);
        exit(1);
    }
    if (wl_add_lines(&wl, v, n, len_cellbarcode)) { fprintf(stderr, "ERROR: fastF filter: %s\n", fastf_last_error()); exit(1); }
    fq_src src_s[3]; fq_src *src[3] = {NULL, NULL, NULL};
    fl_sink sink_s[3]; fl_sink *sink[3] = {NULL, NULL, NULL};
    static const char *const names[3] = {"I1", "R1", "R2"};
    for (int f = 0; f < 3; f++) {
        if (file_in[f] == Z_NULL) continue;
        memset(&src_s[f], 0, sizeof src_s[f]);
        src_s[f].kind = FQ_GZFILE; src_s[f].gz = file_in[f]; src_s[f].fd = -1; src_s[f].nt = 1;
        src[f] = &src_s[f];
        memset(&sink_s[f], 0, sizeof sink_s[f]);
        sink_s[f].gz = file_out[f]; sink_s[f].path = names[f];
        sink[f] = file_out[f] != Z_NULL ? &sink_s[f] : NULL;
    }
    if (!src[1]) { fprintf(stderr, "ERROR: fastF filter: R1 is not open\n"); exit(1); }
    uint64_t nr = 0, nk = 0;
    if (fl_process(src, names, sink, &wl, len_cellbarcode, seed, rate, all_cell, &nr, &nk)) {
        fprintf(stderr, "ERROR: fastF filter: %s\n", fastf_last_error());
        exit(1);
    }
    free(v);
    fl_wl_free(&wl);
}

/* ------------------------------------------------------------------ */
/* CLI: main.c:94-228, the options scanned by cli_opts.c                */
/* ------------------------------------------------------------------ */
static void fl_usage(void)
{
    printf("Usage: fastF filter [options]\n\nFilter fastq file using cell barcode whitelist and read depth.\n\n"
           "    -h, --help              show this help message and exit\n\nBasic options\n"
           "    -I, --I1=<str>          optional, path to sample I1 fastq files\n"
           "    -R, --R1=<str>          required, path to sample R1 fastq files\n"
           "    -r, --R2=<str>          optional, path to sample R2 fastq files\n"
           "    -o, --out=<str>         dir to output fastq files\n"
           "    -w, --whitelist=<str>   whitelist of cell barcodes\n"
           "    -l, --len=<int>         length of cell barcode\n"
           "    -s, --seed=<int>        seed for random number generator\n"
           "    -t, --rate=<flt>        rate of reads to keep after matching cell barcodes\n"
           "    -a, --allcells          keep all reads with cell barcode\n\n");
}

typedef struct { const char *i1, *r1, *r2, *out, *wl; int32_t len; int32_t seed; float rate; int all; } fl_args;

int fl_dir_writable(const char *dir, const char *const names[], const int want[], int n)
{
    struct stat st;
    if (stat(dir, &st) != 0 || !S_ISDIR(st.st_mode) || access(dir, W_OK | X_OK) != 0) return 0;
    for (int f = 0; f < n; f++) {
        if (!want[f]) continue;
        char p[4096];
        snprintf(p, sizeof p, "%s/%s", dir, names[f]);
        if (access(p, F_OK) == 0 && access(p, W_OK) != 0) return 0;
    }
    return 1;
}

int cmd_filter(int argc, const char **argv)
{
    fl_args A; memset(&A, 0, sizeof A);
    A.out = "."; A.len = 16; A.seed = 926; A.rate = 0.f;
    static const cli_opt opts[] = {{'h', "help", 0}, {'I', "I1", 1}, {'R', "R1", 1}, {'r', "R2", 1}, {'o', "out", 1}, {'w', "whitelist", 1},
                                   {'l', "len", 1}, {'s', "seed", 1}, {'t', "rate", 1}, {'a', "allcells", 0}, {0, NULL, 0}};
    cli_scan S = CLI_SCAN(argc, argv, opts, CLI_ARGPARSE);
    for (const cli_opt *o; (o = cli_next(&S));)
        switch (o->s) {
        case 'h': fl_usage(); exit(0);
        case 'I': A.i1 = S.val; break;
        case 'R': A.r1 = S.val; break;
        case 'r': A.r2 = S.val; break;
        case 'o': A.out = S.val; break;
        case 'w': A.wl = S.val; break;
        case 'l': A.len = (int)cli_int(&S); break;
        case 's': A.seed = (int)cli_int(&S); break;
        case 't': A.rate = cli_float(&S); break;
        case 'a': A.all++; break;
        }
    if (S.err) { if (S.err == CLI_UNKNOWN) fl_usage(); exit(EXIT_FAILURE); }
    printf("whitelist: %s\n", A.wl ? A.wl : "(null)");                                     /* main.c:140 */
    if (A.r1 == NULL) {
        fprintf(stderr, "\x1b[31mError:\x1b[0m path to R1 fastq files can not been NULL while filtering .\n");
        exit(1);
    }
    if (A.wl == NULL && !A.all) {
        fprintf(stderr, "\x1b[31mError:\x1b[0m whitelist and --all cell option can not been both NULL at the same time.\n");
        exit(1);
    }
    /* declared divergences: refused before any output is written */
    if (A.len < 0) {
        fprintf(stderr, "\x1b[31mError:\x1b[0m -l %d: negative length of cell barcode (malloc(%d) in substring, filter.c:262; refused)\n",
                A.len, A.len + 1);
        exit(1);
    }
    const char *in[3] = {A.i1, A.r1, A.r2};
    static const char *const outname[3] = {"I1.fastq.gz", "R1.fastq.gz", "R2.fastq.gz"};
    const int want[3] = {A.i1 != NULL, 1, A.r2 != NULL};
    if (!fl_dir_writable(A.out, outname, want, 3)) {
        fprintf(stderr, "\x1b[31mError:\x1b[0m cannot write the outputs into directory %s (gzopen would return NULL; refused)\n", A.out);
        exit(1);
    }
    for (int f = 0; f < 3; f++) {
        if (!in[f]) continue;
        const int fd = open(in[f], O_RDONLY);
        if (fd < 0) { fprintf(stderr, "Cannot open file %s \n", in[f]); exit(1); }
        close(fd);
    }
    if (A.r2 == NULL) printf("TRUE\n");                                                    /* main.c:185-190 */
    if (A.wl != NULL) {
        printf("Reading whitelist...\n");
        fl_wl probe; memset(&probe, 0, sizeof probe);
        const int r = fl_wl_load(&probe, A.wl, (uint32_t)A.len, 0);
        if (r == 2) { printf("\x1b[31mError:\x1b[0m opening %s!\n", A.wl); exit(1); }                /* get_row, filter.c:186-190 */
        if (r) { fprintf(stderr, "\x1b[31mError:\x1b[0m %s\n", fastf_last_error()); exit(1); }
        printf("nrow = %d\n", (int)probe.nrow);
        fl_wl_free(&probe);
    } else {
        printf("Subsample fastq files directly without cell barcode whitelist...\n");
    }
    printf("Processing fastq files...\n");
    fflush(stdout);
    uint64_t nr = 0, nk = 0;
    if (fastf_filter(A.r1, A.i1, A.r2, A.out, A.wl, (uint32_t)A.len, (uint32_t)A.seed, A.rate, A.all, &nr, &nk)) {
        fprintf(stderr, "ERROR: fastF filter: %s\n", fastf_last_error());
        exit(1);
    }
    return 0;
}
