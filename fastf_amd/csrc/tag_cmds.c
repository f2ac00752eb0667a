/*
 * tag_cmds.c — `crb` and `extract` on the tag-histogram engine.
 *
 * Drop-in symbols (same names, signatures and output bytes as the reference):
 *   void     extract_bam(char *bam_file, const char *tag, int type)   extract.c:135-216 (decl. extract.h:26)
 *   CB_node *read_bam(char *bam_file)                                 extract.c:64-133  (decl. extract.h:24)
 *   void     print_CB_node(CB_node *root, gzFile fp)                  extract.c:47-62
 *   void     free_CB_node(CB_node *root)                              extract.c:33-45
 *   int      cmd_crb(int argc, const char **argv)                     main.c:231-286
 *   int      cmd_extract(int argc, const char **argv)                 main.c:364-402
 *
 * The reference inserts every record's tag string into an unbalanced binary search tree (filter.c:105-124,
 * extract.c:3-31) and prints the tree in pre-order.  A tree built by inserting distinct keys in sequence is the
 * Cartesian tree of the keys in strcmp order with "position of first occurrence" as heap priority, so the output
 * is a function of (distinct values, their counts, their first-occurrence positions) — which the device computes
 * with a radix sort + run-length + first-index pass (tag_hist.hpp).  The host side here reads the BAM, packs tag
 * strings into exact 64-bit keys, and turns the device result into the tree order and the output text.
 * No CPU fallback: without a HIP device fastf_taghist_create fails and the commands return an error.
 */
#define _GNU_SOURCE
#include "host_io.h"
#include "cli_opts.h"

#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>
#include <zlib.h>

/* ------------------------------------------------------------------ */
/* insertion-order BST of distinct strings, without inserting          */
/* ------------------------------------------------------------------ */
typedef struct { const char *s; uint64_t first, count; } tag_ent;

static int cmp_ent_idx(const void *a, const void *b, void *ctx)
{
    const tag_ent *ent = (const tag_ent *)ctx;
    return strcmp(ent[*(const uint32_t *)a].s, ent[*(const uint32_t *)b].s);
}

typedef struct { const tag_ent *ent; uint32_t m; int nt; int bad; } order_job;
static void order_worker(void *vp, int w)
{
    order_job *j = (order_job *)vp;
    uint32_t lo = (uint32_t)((uint64_t)j->m * (uint32_t)w / (uint32_t)j->nt), hi = (uint32_t)((uint64_t)j->m * (uint32_t)(w + 1) / (uint32_t)j->nt);
    if (lo == 0) lo = 1;
    for (uint32_t i = lo; i < hi; i++) {
        if (strcmp(j->ent[i - 1].s, j->ent[i].s) >= 0) { __atomic_store_n(&j->bad, 1, __ATOMIC_RELAXED); return; }
        if ((i & 4095) == 0 && __atomic_load_n(&j->bad, __ATOMIC_RELAXED)) return;
    }
}
static int strs_in_order(const tag_ent *ent, uint32_t m)
{
    if (m < 2) return 1;
    order_job j = { ent, m, m < 65536 ? 1 : fastf_host_thread_count(), 0 };
    if (j.nt > 64) j.nt = 64;
    fastf_par_run(j.nt, order_worker, &j);
    return !j.bad;
}

/* Shape of the tree the reference would have built: left/right child (index into ent, -1 = none) and the root.
 * sorted[] receives the strcmp order.  All arrays have m entries. */
/* sorted[] = the entries in strcmp order */
static void sort_strings(const tag_ent *ent, uint32_t m, uint32_t *sorted)
{
    for (uint32_t i = 0; i < m; i++) sorted[i] = i;
    /* the device hands the distinct keys over in key order, which is strcmp order already for tags of one form and length
     * (UB, CB): one parallel pass finds that out, and 11.7 M strings are not sorted again */
    if (!strs_in_order(ent, m)) qsort_r(sorted, m, sizeof *sorted, cmp_ent_idx, (void *)ent);
}
static int32_t bst_shape(const tag_ent *ent, uint32_t m, uint32_t *sorted, int32_t *left, int32_t *right)
{
    sort_strings(ent, m, sorted);
    for (uint32_t i = 0; i < m; i++) left[i] = right[i] = -1;
    /* Cartesian tree (min `first` on top) over the sorted sequence, with the usual right-spine stack */
    uint32_t *stack = (uint32_t *)malloc((m ? m : 1) * sizeof *stack);
    uint32_t top = 0;
    for (uint32_t j = 0; j < m; j++) {
        const uint32_t x = sorted[j];
        int32_t last = -1;
        while (top && ent[stack[top - 1]].first > ent[x].first) last = (int32_t)stack[--top];
        left[x] = last;
        if (top) right[stack[top - 1]] = (int32_t)x;
        stack[top++] = x;
    }
    int32_t root = m ? (int32_t)stack[0] : -1;
    free(stack);
    return root;
}

/* pre-order (node, left, right — filter.c:139-148) of that tree into order[] */
static void bst_preorder(int32_t root, const int32_t *left, const int32_t *right, uint32_t m, uint32_t *order)
{
    int32_t *stack = (int32_t *)malloc((m ? m : 1) * sizeof *stack);
    uint32_t top = 0, k = 0;
    if (root >= 0) stack[top++] = root;
    while (top) {
        const int32_t x = stack[--top];
        order[k++] = (uint32_t)x;
        if (right[x] >= 0) stack[top++] = right[x];
        if (left[x] >= 0) stack[top++] = left[x];
    }
    free(stack);
}

/* The same pre-order without building the tree.  In the Cartesian tree over the strcmp-sorted sequence (smallest `first` on
 * top) the subtree of position j is the open interval between the previous and the next position with a smaller `first`; a node
 * outside that subtree is printed before j iff it lies to the left of it, or is an ancestor to the right of it, and those
 * ancestors are exactly the chain of "next smaller" positions starting at j.  So
 *     rank(j) = (previous smaller position + 1) + (length of j's next-smaller chain),
 * two monotonic-stack sweeps over the sequence — sequential memory, no pointer chasing (11.7 M UB values: 0.07 s against 0.35 s
 * for tree + walk).  sorted[] = the strcmp order (positions -> entries). */
static int preorder_direct(const tag_ent *ent, uint32_t m, const uint32_t *sorted, uint32_t *order)
{
    if (!m) return 0;
    uint64_t *f = (uint64_t *)malloc((size_t)m * sizeof *f);
    uint32_t *pl1 = (uint32_t *)malloc((size_t)m * sizeof *pl1), *stack = (uint32_t *)malloc((size_t)m * sizeof *stack);
    if (!f || !pl1 || !stack) { free(f); free(pl1); free(stack); return 1; }
    for (uint32_t j = 0; j < m; j++) f[j] = ent[sorted[j]].first;
    uint32_t top = 0;
    for (uint32_t j = 0; j < m; j++) {                       /* previous smaller, from the left */
        while (top && f[stack[top - 1]] > f[j]) top--;
        pl1[j] = top ? stack[top - 1] + 1 : 0;
        stack[top++] = j;
    }
    top = 0;
    for (uint32_t j = m; j-- > 0;) {                         /* what is left on the stack IS the next-smaller chain of j */
        while (top && f[stack[top - 1]] > f[j]) top--;
        order[pl1[j] + top] = sorted[j];
        stack[top++] = j;
    }
    free(f); free(pl1); free(stack);
    return 0;
}

/* host-side tree order on its own (exported for the CPU test suite): order[] = pre-order of the insertion-order BST
 * of the m distinct strings whose first occurrences are first[] */
void fastf_tag_tree_preorder(const char *const *strs, const uint64_t *first, uint32_t m, uint32_t *order)
{
    if (!m) return;
    tag_ent *ent = (tag_ent *)calloc(m, sizeof *ent);
    uint32_t *sorted = (uint32_t *)malloc((m ? m : 1) * sizeof *sorted);
    int32_t *left = (int32_t *)malloc((m ? m : 1) * sizeof *left), *right = (int32_t *)malloc((m ? m : 1) * sizeof *right);
    for (uint32_t i = 0; i < m; i++) { ent[i].s = strs[i]; ent[i].first = first[i]; ent[i].count = 1; }
    const int32_t root = bst_shape(ent, m, sorted, left, right);
    /* the direct ranks are what extract / crb print; should the sweep run out of memory, the tree walk gives the same order */
    if (preorder_direct(ent, m, sorted, order)) bst_preorder(root, left, right, m, order);
    free(ent); free(sorted); free(left); free(right);
}

typedef struct { char *p; size_t len, cap; } tbuf;
static void tb_put(tbuf *b, const char *s, size_t n)
{
    if (b->len + n + 1 > b->cap) {
        while (b->len + n + 1 > b->cap) b->cap = b->cap ? b->cap * 2 : (1u << 16);
        b->p = (char *)realloc(b->p, b->cap);
    }
    memcpy(b->p + b->len, s, n);
    b->len += n;
}
static void tb_count(tbuf *b, uint64_t v, char after)     /* ",<count><after>" — "%s,%ld" filter.c:145,166 */
{
    char t[32];
    int i = (int)sizeof t;
    t[--i] = after;
    do { t[--i] = (char)('0' + v % 10); v /= 10; } while (v);
    t[--i] = ',';
    tb_put(b, t + i, sizeof t - (size_t)i);
}

/* "<string>,<count><after>" (print_tree, filter.c:139-148) for ent[order[0..m)], appended to out: every thread formats a slice
 * into its own buffer, the slices are concatenated in order (11.7 M UB values: 0.62 s on one thread) */
typedef struct { const tag_ent *ent; const uint32_t *order; size_t m; char after; int nt; tbuf *part; int err; } rows_job;
static void rows_worker(void *vp, int w)
{
    rows_job *j = (rows_job *)vp;
    const size_t lo = j->m * (size_t)w / (size_t)j->nt, hi = j->m * (size_t)(w + 1) / (size_t)j->nt;
    tbuf *b = &j->part[w];
    b->cap = (hi - lo) * 24 + 64; b->p = (char *)malloc(b->cap); b->len = 0;
    if (!b->p) { j->err = 1; b->cap = 0; return; }
    for (size_t k = lo; k < hi; k++) {
        /* the rows come in tree order, i.e. from all over the entry table and the string pool: ask for them a few rows ahead */
        if (k + 16 < hi) __builtin_prefetch(&j->ent[j->order[k + 16]]);
        if (k + 8 < hi) __builtin_prefetch(j->ent[j->order[k + 8]].s);
        const tag_ent *e = &j->ent[j->order[k]];
        tb_put(b, e->s, strlen(e->s));
        tb_count(b, e->count, j->after);
    }
}
static int rows_text(const tag_ent *ent, const uint32_t *order, size_t m, char after, tbuf *out)
{
    int nt = fastf_host_thread_count();
    if (m < 65536) nt = 1;
    if (nt > 64) nt = 64;
    tbuf part[64]; memset(part, 0, sizeof part);
    rows_job j = { ent, order, m, after, nt, part, 0 };
    fastf_par_run(nt, rows_worker, &j);
    size_t total = 0;
    for (int w = 0; w < nt; w++) total += part[w].len;
    int rc = j.err;
    if (!rc) {
        if (out->len + total + 1 > out->cap) { out->cap = out->len + total + 1; out->p = (char *)realloc(out->p, out->cap); if (!out->p) rc = 1; }
        for (int w = 0; w < nt && !rc; w++) { memcpy(out->p + out->len, part[w].p, part[w].len); out->len += part[w].len; }
    }
    for (int w = 0; w < nt; w++) free(part[w].p);
    return rc;
}

/* the same two steps for another command (freq, fastq_cmds.c): rows "<strs[order[k]]>,<count[order[k]]>\n" (malloc'ed text),
 * and the reference's tree itself, node for node (malloc'ed nodes and strings) */
int fastf_tag_rows_text_(const char *const *strs, const uint64_t *count, const uint32_t *order, size_t m, char **txt, size_t *txt_len)
{
    tag_ent *ent = (tag_ent *)malloc((m ? m : 1) * sizeof *ent);
    if (!ent) return 1;
    for (size_t i = 0; i < m; i++) { ent[i].s = strs[i]; ent[i].first = 0; ent[i].count = count[i]; }
    tbuf out = {0};
    tb_put(&out, "", 0);
    const int rc = rows_text(ent, order, m, '\n', &out);
    free(ent);
    if (rc) { free(out.p); return 1; }
    *txt = out.p; *txt_len = out.len;
    return 0;
}
static node *build_nodes(const tag_ent *ent, uint32_t m, uint32_t *sorted, int32_t *left, int32_t *right);
node *fastf_tag_tree_nodes_(const char *const *strs, const uint64_t *first, const uint64_t *count, uint32_t m)
{
    tag_ent *ent = (tag_ent *)malloc((m ? m : 1) * sizeof *ent);
    uint32_t *sorted = (uint32_t *)malloc((m ? m : 1) * sizeof *sorted);
    int32_t *left = (int32_t *)malloc((m ? m : 1) * sizeof *left), *right = (int32_t *)malloc((m ? m : 1) * sizeof *right);
    node *r = NULL;
    if (ent && sorted && left && right) {
        for (uint32_t i = 0; i < m; i++) { ent[i].s = strs[i]; ent[i].first = first[i]; ent[i].count = count[i]; }
        r = build_nodes(ent, m, sorted, left, right);
    }
    free(ent); free(sorted); free(left); free(right);
    return r;
}

/* ------------------------------------------------------------------ */
/* BAM → device histogram                                              */
/* ------------------------------------------------------------------ */
typedef struct {
    fastf_keydict_t *dict;
    fastf_taghist_t *hist;
    fastf_taghist_result_t res;
    uint64_t n_records, n_undefined;
} tag_run;

static double tnow(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + t.tv_nsec * 1e-9; }
static int tprof(void) { return getenv("FASTF_PROFILE") != NULL; }

static void tag_run_free(tag_run *r)
{
    if (r->hist) fastf_taghist_destroy(r->hist);
    if (r->dict) fastf_keydict_destroy(r->dict);
    memset(r, 0, sizeof *r);
}

typedef struct { fastf_taghist_t *h; int rc; int done; } hist_boot;
static void *hist_boot_main(void *vp)
{
    hist_boot *b = (hist_boot *)vp;
    b->rc = fastf_taghist_create(0, &b->h);
    __atomic_store_n(&b->done, 1, __ATOMIC_RELEASE);
    return NULL;
}

static int tag_run_bam(const char *bam_file, const char *tag1, const char *tag2, int type, tag_run *r)
{
    memset(r, 0, sizeof *r);
    /* the BGZF inflate is shared with the device, as in bam2db() (these commands need one anyway); FASTF_TAGS_GPU_INFLATE=0
     * (or FASTF_GPU_INFLATE=0): host threads only */
    const char *tgi = getenv("FASTF_TAGS_GPU_INFLATE");
    fastf_bam_t *bam = (tgi && tgi[0] == '0') ? fastf_bam_open(bam_file, 0) : fastf_bam_open2(bam_file, 0, 1);
    if (!bam) return 1;
    const size_t cap = (size_t)4 << 20;
    /* Batches of tag keys.  While the histogram handle (HIP runtime, device context: 0.2-0.3 s) is still coming up on its own
     * thread, the batches read meanwhile are kept (up to MAXB of them) and pushed in order once it is there. */
    enum { MAXB = 8 };
    uint64_t *b1[MAXB] = {0}, *b2[MAXB] = {0}; long bn[MAXB] = {0};
    int held = 0, nb = 0;
    int rc = 1;
    double t_read = 0, t_push = 0, t_create = 0, t0;
    hist_boot hb; hb.h = NULL; hb.rc = 1; hb.done = 0;
    pthread_t hb_th; int hb_started = 0;
    r->dict = fastf_keydict_create();
    if (!r->dict) { fastf_set_error_("out of memory"); goto done; }
    hb_started = pthread_create(&hb_th, NULL, hist_boot_main, &hb) == 0;
    if (!hb_started) hist_boot_main(&hb);
    for (;;) {
        if (held == nb) {                                     /* a fresh buffer pair for this batch */
            if (nb == MAXB) { fastf_set_error_("internal: batch ring exhausted"); goto done; }
            b1[nb] = (uint64_t *)malloc(cap * sizeof(uint64_t)); b2[nb] = tag2 ? (uint64_t *)malloc(cap * sizeof(uint64_t)) : NULL;
            if (!b1[nb] || (tag2 && !b2[nb])) { fastf_set_error_("out of memory"); nb++; goto done; }
            nb++;
        }
        double t1 = tnow();
        const long n = fastf_bam_read_tags(bam, r->dict, tag1, tag2, type, b1[held], b2[held], cap, &r->n_undefined);
        t_read += tnow() - t1;
        if (n < 0) goto done;
        bn[held] = n;
        if (n > 0) held++;
        /* hand the kept batches over when the handle is there, when the input has ended, or when no buffer is left */
        const int ready = !hb_started || __atomic_load_n(&hb.done, __ATOMIC_ACQUIRE);
        if (ready || n == 0 || held == MAXB) {
            if (hb_started) { t1 = tnow(); pthread_join(hb_th, NULL); hb_started = 0; t_create = tnow() - t1; }
            if (hb.rc) goto done;
            r->hist = hb.h;
            t1 = tnow();
            for (int i = 0; i < held; i++) {
                if (fastf_taghist_push(r->hist, b1[i], b2[i], (size_t)bn[i])) goto done;
                r->n_records += (uint64_t)bn[i];
            }
            t_push += tnow() - t1;
            held = 0;
        }
        if (n == 0) break;
    }
    t0 = tnow();
    if (fastf_taghist_finish(r->hist, &r->res)) goto done;
    if (tprof()) fprintf(stderr, "[tags] waited %.3f s for the histogram handle, BAM read + tag keys %.3f s, push %.3f s, finish (device) %.3f s\n", t_create, t_read, t_push, tnow() - t0);
    rc = 0;
done:
    if (hb_started) { pthread_join(hb_th, NULL); if (!hb.rc && !r->hist) r->hist = hb.h; }
    for (int i = 0; i < nb; i++) { free(b1[i]); free(b2[i]); }
    fastf_bam_close(bam);
    if (rc) { char keep[512]; snprintf(keep, sizeof keep, "%s", fastf_last_error()); tag_run_free(r); fastf_set_error_(keep); }
    return rc;
}

/* decoded strings of n keys; type 1 keys print as "%d" (extract.c:192).  Every thread decodes a slice of the keys into a pool of
 * its own; the pools travel together as one allocation list (free with pools_free).  Returns NULL on failure. */
typedef struct { char *p[64]; int n; } key_pools;
static void pools_free(key_pools *kp) { if (!kp) return; for (int i = 0; i < kp->n; i++) free(kp->p[i]); free(kp); }
typedef struct { const fastf_keydict_t *d; const uint64_t *keys; size_t n; int type, nt; const char **strs; key_pools *kp; int err; } decode_job;
static void decode_worker(void *vp, int w)
{
    decode_job *j = (decode_job *)vp;
    const size_t lo = j->n * (size_t)w / (size_t)j->nt, hi = j->n * (size_t)(w + 1) / (size_t)j->nt;
    size_t cap = (hi - lo) * 24 + 8192, len = 0;
    char *pool = (char *)malloc(cap);
    size_t *off = (size_t *)malloc((hi - lo + 1) * sizeof *off);
    if (!pool || !off) { free(pool); free(off); j->err = 1; return; }
    for (size_t i = lo; i < hi; i++) {
        if (cap - len < 4200) { cap = cap * 2 + 8192; char *np = (char *)realloc(pool, cap); if (!np) { free(pool); free(off); j->err = 1; return; } pool = np; }
        long l;
        if (j->type == 1) l = snprintf(pool + len, cap - len, "%d", (int)(int32_t)(uint32_t)j->keys[i]);
        else l = fastf_keydict_decode(j->d, j->keys[i], pool + len, cap - len > 4096 ? 4096 : cap - len);
        if (l < 0) {                       /* a tag value longer than 4 KiB: give it all the room it needs */
            cap = cap * 2 + (1u << 20);
            char *np = (char *)realloc(pool, cap); if (!np) { free(pool); free(off); j->err = 1; return; } pool = np;
            l = fastf_keydict_decode(j->d, j->keys[i], pool + len, cap - len);
            if (l < 0) { free(pool); free(off); j->err = 2; return; }
        }
        off[i - lo] = len;
        len += (size_t)l + 1;
    }
    for (size_t i = lo; i < hi; i++) j->strs[i] = pool + off[i - lo];
    free(off);
    j->kp->p[w] = pool;
}
static key_pools *decode_keys(const fastf_keydict_t *d, const uint64_t *keys, size_t n, int type, const char ***strs_out)
{
    key_pools *kp = (key_pools *)calloc(1, sizeof *kp);
    const char **strs = (const char **)malloc((n ? n : 1) * sizeof *strs);
    if (!kp || !strs) { free(kp); free(strs); fastf_set_error_("out of memory"); return NULL; }
    int nt = fastf_host_thread_count();
    if (n < 65536) nt = 1;
    if (nt > 64) nt = 64;
    kp->n = nt;
    decode_job j = { d, keys, n, type, nt, strs, kp, 0 };
    fastf_par_run(nt, decode_worker, &j);
    if (j.err) { pools_free(kp); free(strs); fastf_set_error_(j.err == 2 ? "undecodable tag key" : "out of memory"); return NULL; }
    *strs_out = strs;
    return kp;
}

/* ------------------------------------------------------------------ */
/* extract                                                             */
/* ------------------------------------------------------------------ */
/* tag histogram of a BAM as the bytes of tag_summary.csv; *valid = records that carry the tag (extract.c:185) */
int fastf_extract_text(const char *bam_file, const char *tag, int type, char **csv, size_t *csv_len,
                       uint64_t *n_records, uint64_t *n_valid)
{
    tag_run r;
    if (tag_run_bam(bam_file, tag, NULL, type ? 1 : 0, &r)) return 1;
    /* `switch (type)` has cases 0 and 1 only (extract.c:186-196): any other type counts valid reads and inserts nothing */
    const size_t m = (type == 0 || type == 1) ? r.res.n1 : 0;
    const char **strs = NULL;
    double tp0 = tnow();
    key_pools *pool = decode_keys(r.dict, r.res.key1, m, type ? 1 : 0, &strs);
    const double tp_decode = tnow() - tp0;
    if (!pool) { tag_run_free(&r); return 1; }
    tag_ent *ent = (tag_ent *)malloc((m ? m : 1) * sizeof *ent);
    uint32_t *sorted = (uint32_t *)malloc((m ? m : 1) * sizeof *sorted), *order = (uint32_t *)malloc((m ? m : 1) * sizeof *order);
    int32_t *left = NULL, *right = NULL;
    for (size_t i = 0; i < m; i++) { ent[i].s = strs[i]; ent[i].first = r.res.first1[i]; ent[i].count = r.res.count1[i]; }
    tp0 = tnow();
    sort_strings(ent, (uint32_t)m, sorted);
    const double tp_shape = tnow() - tp0;
    tp0 = tnow();
    if (preorder_direct(ent, (uint32_t)m, sorted, order)) {          /* (out of memory for the sweep: the tree and its walk) */
        left = (int32_t *)malloc((m ? m : 1) * sizeof *left); right = (int32_t *)malloc((m ? m : 1) * sizeof *right);
        bst_preorder(bst_shape(ent, (uint32_t)m, sorted, left, right), left, right, (uint32_t)m, order);
    }
    const double tp_ranks = tnow() - tp0;
    tbuf out = {0};
    tb_put(&out, "", 0);
    if (rows_text(ent, order, m, '\n', &out)) {
        free(out.p); free(ent); free(sorted); free(order); free(left); free(right); free(strs); pools_free(pool);
        tag_run_free(&r);
        fastf_set_error_("out of memory (tag summary text)");
        return 1;
    }
    if (tprof()) fprintf(stderr, "[tags] %zu distinct values: decode %.3f s, strcmp order %.3f s, pre-order ranks %.3f s, text %.3f s\n", m, tp_decode, tp_shape, tp_ranks, tnow() - tp0 - tp_ranks);
    if (!out.p) out.p = (char *)calloc(1, 1);
    *csv = out.p; *csv_len = out.len;
    if (n_records) *n_records = r.n_records;
    if (n_valid) *n_valid = r.res.n_valid + r.n_undefined;
    if (r.n_undefined)
        fprintf(stderr, "Warning: %llu records carry tag %s with a non-string type; the reference passes NULL to strcmp there "
                "(extract.c:189) — skipped\n", (unsigned long long)r.n_undefined, tag);
    free(ent); free(sorted); free(order); free(left); free(right); free(strs); pools_free(pool);
    tag_run_free(&r);
    return 0;
}

void extract_bam(char *bam_file, const char *tag, int type)
{
    char *csv = NULL; size_t len = 0; uint64_t n = 0, valid = 0;
    if (fastf_extract_text(bam_file, tag, type, &csv, &len, &n, &valid)) {
        fprintf(stderr, "ERROR: Cannot open bam file %s (%s)\n", bam_file, fastf_last_error());      /* extract.c:142 */
        exit(1);
    }
    FILE *fp = fopen("tag_summary.csv", "w");                       /* extract.c:200-202 */
    if (!fp || fwrite(csv, 1, len, fp) != len) { fprintf(stderr, "ERROR: Cannot write tag_summary.csv\n"); exit(1); }
    fclose(fp);
    free(csv);
    printf("Processed all %lu reads\n", (unsigned long)(2 * n));    /* total_count is incremented twice per record, :163,165 */
    printf("Valid reads: %lu\n", (unsigned long)valid);             /* :207 */
}

/* ------------------------------------------------------------------ */
/* crb                                                                 */
/* ------------------------------------------------------------------ */
/* reference tree types node / CB_node (filter.h:28-34, extract.h:8-13): fastf_amd.h */

typedef struct {
    tag_run r;
    size_t n_cb;                 /* CBs that occur in at least one valid (CB, CR) record */
    tag_ent *cb;                 /* [n_cb] */
    size_t *cr_lo;               /* [n_cb + 1] slice of cr[] per CB */
    tag_ent *cr;                 /* [n_pairs] */
    key_pools *pool1, *pool2; const char **s1, **s2;
} crb_data;

static void crb_free(crb_data *c)
{
    free(c->cb); free(c->cr_lo); free(c->cr); pools_free(c->pool1); pools_free(c->pool2); free(c->s1); free(c->s2);
    tag_run_free(&c->r);
    memset(c, 0, sizeof *c);
}

static int crb_load(const char *bam_file, crb_data *c)
{
    memset(c, 0, sizeof *c);
    if (tag_run_bam(bam_file, "CB", "CR", 0, &c->r)) return 1;
    const fastf_taghist_result_t *res = &c->r.res;
    c->pool1 = decode_keys(c->r.dict, res->key1, res->n1, 0, &c->s1);
    c->pool2 = c->pool1 ? decode_keys(c->r.dict, res->pair_key2, res->n_pairs, 0, &c->s2) : NULL;
    if (!c->pool1 || !c->pool2) { crb_free(c); return 1; }
    c->cb = (tag_ent *)malloc((res->n1 ? res->n1 : 1) * sizeof *c->cb);
    c->cr_lo = (size_t *)malloc((res->n1 + 1) * sizeof *c->cr_lo);
    c->cr = (tag_ent *)malloc((res->n_pairs ? res->n_pairs : 1) * sizeof *c->cr);
    size_t p = 0;
    for (size_t i = 0; i < res->n1; i++) {                  /* pairs are ordered by key1 rank, so each CB owns a slice */
        if (res->count1[i] == 0) continue;                  /* CB seen only on records without CR */
        c->cb[c->n_cb].s = c->s1[i]; c->cb[c->n_cb].first = res->first1[i]; c->cb[c->n_cb].count = res->count1[i];
        c->cr_lo[c->n_cb] = p;
        while (p < res->n_pairs && res->pair_k1[p] == i) {
            c->cr[p].s = c->s2[p]; c->cr[p].first = res->pair_first[p]; c->cr[p].count = res->pair_count[p];
            p++;
        }
        c->n_cb++;
    }
    c->cr_lo[c->n_cb] = p;
    if (p != res->n_pairs) { fastf_set_error_("crb: pair table is not grouped by CB"); crb_free(c); return 1; }
    /* a record with CB but no (string) CR is a NULL dereference in the reference (extract.c:102-103) */
    const uint64_t n_cb_only = res->n_key1_present - res->n_valid;
    if (n_cb_only || c->r.n_undefined)
        fprintf(stderr, "Warning: %llu records carry CB without a string CR (%llu CB/CR tags of a non-string type); the reference "
                "dereferences NULL there (extract.c:102-103) — skipped\n",
                (unsigned long long)n_cb_only, (unsigned long long)c->r.n_undefined);
    return 0;
}

typedef struct { const crb_data *c; const uint32_t *order; uint32_t m; int nt; tbuf *part; int err; } crb_rows_job;
static void crb_rows_worker(void *vp, int w)
{
    crb_rows_job *j = (crb_rows_job *)vp;
    const crb_data *c = j->c;
    const uint32_t lo = (uint32_t)((uint64_t)j->m * (uint32_t)w / (uint32_t)j->nt), hi = (uint32_t)((uint64_t)j->m * (uint32_t)(w + 1) / (uint32_t)j->nt);
    size_t max_cr = 1;
    for (uint32_t k = lo; k < hi; k++) { const size_t n = c->cr_lo[j->order[k] + 1] - c->cr_lo[j->order[k]]; if (n > max_cr) max_cr = n; }
    uint32_t *sorted = (uint32_t *)malloc(max_cr * sizeof *sorted), *order2 = (uint32_t *)malloc(max_cr * sizeof *order2);
    int32_t *left = (int32_t *)malloc(max_cr * sizeof *left), *right = (int32_t *)malloc(max_cr * sizeof *right);
    tbuf *b = &j->part[w];
    if (!sorted || !order2 || !left || !right) { j->err = 1; free(sorted); free(order2); free(left); free(right); return; }
    for (uint32_t k = lo; k < hi; k++) {
        const uint32_t i = j->order[k];
        tb_put(b, c->cb[i].s, strlen(c->cb[i].s)); tb_put(b, ";", 1);
        const tag_ent *cr = c->cr + c->cr_lo[i];
        const uint32_t mc = (uint32_t)(c->cr_lo[i + 1] - c->cr_lo[i]);
        const int32_t r2 = bst_shape(cr, mc, sorted, left, right);
        bst_preorder(r2, left, right, mc, order2);
        for (uint32_t q = 0; q < mc; q++) {
            tb_put(b, cr[order2[q]].s, strlen(cr[order2[q]].s));
            tb_count(b, cr[order2[q]].count, ';');
        }
        tb_put(b, "\n", 1);
    }
    free(sorted); free(order2); free(left); free(right);
}

/* the bytes print_CB_node would write for the whole tree */
int fastf_crb_text(const char *bam_file, char **txt, size_t *txt_len, uint64_t *n_records)
{
    crb_data c;
    if (crb_load(bam_file, &c)) return 1;
    const uint32_t m = (uint32_t)c.n_cb;
    const double tc0 = tnow();
    uint32_t *sorted = (uint32_t *)malloc((m ? m : 1) * sizeof *sorted), *order = (uint32_t *)malloc((m ? m : 1) * sizeof *order);
    sort_strings(c.cb, m, sorted);
    if (preorder_direct(c.cb, m, sorted, order)) {
        int32_t *left = (int32_t *)malloc((m ? m : 1) * sizeof *left), *right = (int32_t *)malloc((m ? m : 1) * sizeof *right);
        bst_preorder(bst_shape(c.cb, m, sorted, left, right), left, right, m, order);
        free(left); free(right);
    }
    free(sorted);
    /* one row per CB in that order (print_CB_node, extract.c:47-62): the CB, then its own CR tree in pre-order
     * (print_tree_same_row, filter.c:160-169).  The rows are independent: every thread formats a slice of them. */
    int nt = fastf_host_thread_count();
    if (m < 256) nt = 1;
    if (nt > 64) nt = 64;
    tbuf part[64]; memset(part, 0, sizeof part);
    crb_rows_job j = { &c, order, m, nt, part, 0 };
    fastf_par_run(nt, crb_rows_worker, &j);
    tbuf out = {0};
    tb_put(&out, "", 0);
    size_t total = 0;
    for (int w = 0; w < nt; w++) total += part[w].len;
    if (!j.err && out.len + total + 1 > out.cap) { out.cap = out.len + total + 1; out.p = (char *)realloc(out.p, out.cap); if (!out.p) j.err = 1; }
    for (int w = 0; w < nt && !j.err; w++) { memcpy(out.p + out.len, part[w].p, part[w].len); out.len += part[w].len; }
    for (int w = 0; w < nt; w++) free(part[w].p);
    free(order);
    if (j.err) { free(out.p); crb_free(&c); fastf_set_error_("out of memory (crb text)"); return 1; }
    if (tprof()) fprintf(stderr, "[tags] %u CB rows, %zu (CB, CR) pairs: trees + text %.3f s on %d threads\n", m, (size_t)c.cr_lo[c.n_cb], tnow() - tc0, nt);
    if (!out.p) out.p = (char *)calloc(1, 1);
    *txt = out.p; *txt_len = out.len;
    if (n_records) *n_records = c.r.n_records;
    crb_free(&c);
    return 0;
}

static node *build_nodes(const tag_ent *ent, uint32_t m, uint32_t *sorted, int32_t *left, int32_t *right)
{
    int32_t root = bst_shape(ent, m, sorted, left, right);
    if (root < 0) return NULL;
    node **nd = (node **)malloc(m * sizeof *nd);
    for (uint32_t i = 0; i < m; i++) {
        nd[i] = (node *)malloc(sizeof(node));
        nd[i]->data = strdup(ent[i].s); nd[i]->count = (long)ent[i].count;
    }
    for (uint32_t i = 0; i < m; i++) {
        nd[i]->left = left[i] >= 0 ? nd[left[i]] : NULL;
        nd[i]->right = right[i] >= 0 ? nd[right[i]] : NULL;
    }
    node *r = nd[root];
    free(nd);
    return r;
}

/* extract.c:64-133: the tree the reference's read_bam returns, node for node (every node and string is
 * malloc'ed, so the reference's free_CB_node / free_tree_node can release it) */
CB_node *read_bam(char *bam_file)
{
    crb_data c;
    if (crb_load(bam_file, &c)) {
        fprintf(stderr, "ERROR: Cannot open bam file %s (%s)\n", bam_file, fastf_last_error());      /* extract.c:71 */
        exit(1);
    }
    const uint32_t m = (uint32_t)c.n_cb;
    size_t max_cr = 1;
    for (size_t i = 0; i < c.n_cb; i++) if (c.cr_lo[i + 1] - c.cr_lo[i] > max_cr) max_cr = c.cr_lo[i + 1] - c.cr_lo[i];
    const size_t w = m > max_cr ? m : max_cr;
    uint32_t *sorted = (uint32_t *)malloc((w ? w : 1) * sizeof *sorted);
    int32_t *left = (int32_t *)malloc((w ? w : 1) * sizeof *left), *right = (int32_t *)malloc((w ? w : 1) * sizeof *right);
    CB_node **nd = (CB_node **)malloc((m ? m : 1) * sizeof *nd);
    for (uint32_t i = 0; i < m; i++) {
        nd[i] = (CB_node *)malloc(sizeof(CB_node));
        nd[i]->CB = strdup(c.cb[i].s);
        nd[i]->CR = build_nodes(c.cr + c.cr_lo[i], (uint32_t)(c.cr_lo[i + 1] - c.cr_lo[i]), sorted, left, right);
    }
    int32_t root = bst_shape(c.cb, m, sorted, left, right);
    for (uint32_t i = 0; i < m; i++) {
        nd[i]->left = left[i] >= 0 ? nd[left[i]] : NULL;
        nd[i]->right = right[i] >= 0 ? nd[right[i]] : NULL;
    }
    CB_node *r = root >= 0 ? nd[root] : NULL;
    printf("Processed all %lu reads\n", (unsigned long)c.r.n_records);                               /* extract.c:125 */
    free(nd); free(sorted); free(left); free(right);
    crb_free(&c);
    return r;
}

void print_CB_node(CB_node *root, gzFile fp)                 /* extract.c:47-62, iterative */
{
    size_t cap = 64, top = 0, cap2 = 64;
    CB_node **st = (CB_node **)malloc(cap * sizeof *st);
    node **st2 = (node **)malloc(cap2 * sizeof *st2);
    if (root) st[top++] = root;
    while (top) {
        CB_node *c = st[--top];
        gzprintf(fp, "%s;", c->CB);
        size_t t2 = 0;
        if (c->CR) st2[t2++] = c->CR;
        while (t2) {                                         /* print_tree_same_row, filter.c:160-169 */
            node *n = st2[--t2];
            gzprintf(fp, "%s,%ld;", n->data, n->count);
            if (t2 + 2 > cap2) { cap2 *= 2; st2 = (node **)realloc(st2, cap2 * sizeof *st2); }
            if (n->right) st2[t2++] = n->right;
            if (n->left) st2[t2++] = n->left;
        }
        gzprintf(fp, "\n");
        if (top + 2 > cap) { cap *= 2; st = (CB_node **)realloc(st, cap * sizeof *st); }
        if (c->right) st[top++] = c->right;
        if (c->left) st[top++] = c->left;
    }
    free(st); free(st2);
}

static void free_nodes(node *root)
{
    size_t cap = 64, top = 0;
    node **st = (node **)malloc(cap * sizeof *st);
    if (root) st[top++] = root;
    while (top) {
        node *n = st[--top];
        if (top + 2 > cap) { cap *= 2; st = (node **)realloc(st, cap * sizeof *st); }
        if (n->left) st[top++] = n->left;
        if (n->right) st[top++] = n->right;
        free(n->data); free(n);
    }
    free(st);
}

void free_CB_node(CB_node *root)                             /* extract.c:33-45, iterative */
{
    size_t cap = 64, top = 0;
    CB_node **st = (CB_node **)malloc(cap * sizeof *st);
    if (root) st[top++] = root;
    while (top) {
        CB_node *c = st[--top];
        if (top + 2 > cap) { cap *= 2; st = (CB_node **)realloc(st, cap * sizeof *st); }
        if (c->left) st[top++] = c->left;
        if (c->right) st[top++] = c->right;
        free(c->CB); free_nodes(c->CR); free(c);
    }
    free(st);
}

/* ------------------------------------------------------------------ */
/* CLI (the options: cli_opts.c; a parse error ends with EXIT_FAILURE and no usage text) */
/* ------------------------------------------------------------------ */
int cmd_crb(int argc, const char **argv)                     /* main.c:231-286 */
{
    static const cli_opt opts[] = {{'h', "help", 0}, {'b', "bam", 1}, {'o', "out", 1}, {0, NULL, 0}};
    const char *bam = NULL, *out = ".";
    cli_scan S = CLI_SCAN(argc, argv, opts, 0);
    for (const cli_opt *o; (o = cli_next(&S));)
        switch (o->s) {
        case 'h':
            printf("Usage: fastF crb [options]\n\nExtract CR and CB tags from bam file and summarize them with frequencies to a tsv file.\n\n"
                   "    -h, --help        show this help message and exit\n"
                   "    -b, --bam=<str>   path to bam file\n"
                   "    -o, --out=<str>   path to output file\n");
            exit(0);
        case 'b': bam = S.val; break;
        case 'o': out = S.val; break;
        }
    if (S.err) exit(EXIT_FAILURE);
    if (bam == NULL) {
        fprintf(stderr, "\x1b[31mError:\x1b[0m path to bam file can not been NULL while extracting .\n");          /* main.c:253 */
        exit(1);
    }
    {   /* main.c:261-267: the output must be creatable before the BAM is read */
        FILE *probe = fopen(out, "wb");
        if (!probe) { fprintf(stderr, "\x1b[31mError:\x1b[0m can not open file %s\n", out); exit(1); }
        fclose(probe);
    }
    char *txt = NULL; size_t len = 0; uint64_t n = 0;
    if (fastf_crb_text(bam, &txt, &len, &n)) {
        fprintf(stderr, "ERROR: Cannot open bam file %s (%s)\n", bam, fastf_last_error());
        exit(1);
    }
    printf("Processed all %lu reads\n", (unsigned long)n);     /* extract.c:125 */
    printf("Writing to file...\n");                            /* main.c:272 */
    int rc = fastf_write_gz_text(out, txt, len);
    free(txt);
    if (rc) { fprintf(stderr, "\x1b[31mError:\x1b[0m %s\n", fastf_last_error()); return 1; }
    printf("Done.\n");                                         /* main.c:284 */
    return 0;
}

int cmd_extract(int argc, const char **argv)                  /* main.c:364-402 */
{
    static const cli_opt opts[] = {{'h', "help", 0}, {'b', "bam", 1}, {'t', "tag", 1}, {'T', "type", 1}, {0, NULL, 0}};
    const char *bam = NULL, *tag = NULL;
    int type = 0;
    cli_scan S = CLI_SCAN(argc, argv, opts, CLI_NO_ERANGE);
    for (const cli_opt *o; (o = cli_next(&S));)
        switch (o->s) {
        case 'h':
            printf("Usage: fastF extract [options]\n\nExtract the tag of bam file.\n\n"
                   "    -h, --help        show this help message and exit\n"
                   "    -b, --bam=<str>   path to bam file\n"
                   "    -t, --tag=<str>   tag of bam file\n"
                   "    -T, --type=<int>  type of tag, 0: string, 1: integer\n");
            exit(0);
        case 'b': bam = S.val; break;
        case 't': tag = S.val; break;
        case 'T': type = (int)cli_int(&S); break;              /* argparse.c:88-92 */
        }
    if (S.err) exit(EXIT_FAILURE);
    if (!bam || access(bam, F_OK) == -1) {
        fprintf(stderr, "\x1b[31mError:\x1b[0m bam file: %s does not exist.\n", bam ? bam : "(null)");              /* main.c:386 */
        exit(1);
    }
    if (tag == NULL) { fprintf(stderr, "\x1b[31mError:\x1b[0m --tag is required.\n"); exit(1); }                     /* main.c:392 */
    extract_bam((char *)bam, tag, type);
    return 0;
}
