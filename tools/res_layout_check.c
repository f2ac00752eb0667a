/* res_layout_check.c — the carved blocks of the resident pair state (fastf_amd/csrc/res_layout.h) at their boundary counts: every array
 * starts at a multiple of its element size, no two arrays overlap, the last one ends inside the reported bytes, every array can be
 * written through the view inside a malloc of exactly those bytes (built with -fsanitize=address,undefined, which is what notices),
 * and every offset is where the formula written out below puts it — the placement the blocks had before they had a layout header.
 * Includes the layout header alone. */
#include "res_layout.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef struct { const char *name; void *p; size_t elem, n, want_off; } span_t;
#define SPAN(view, field, n, off) { #field, (view).field, sizeof *(view).field, (n), (off) }

static unsigned long n_checked;
static void fail(const char *block, const char *what, const span_t *a, size_t c0, size_t c1, size_t c2)
{
    fprintf(stderr, "%s(%zu, %zu, %zu): %s: %s\n", block, c0, c1, c2, a ? a->name : "(block)", what);
    exit(1);
}

/* base: a malloc of exactly `bytes`; a[]: the arrays of the view in their order */
static void check(const char *block, char *base, size_t bytes, size_t want_bytes, span_t *a, int n, size_t c0, size_t c1, size_t c2)
{
    if (bytes != want_bytes) fail(block, "the bytes of the block moved", NULL, c0, c1, c2);
    for (int i = 0; i < n; i++) {
        const size_t off = (size_t)((char *)a[i].p - base), end = off + a[i].n * a[i].elem;
        if (off != a[i].want_off) fail(block, "the array moved", &a[i], c0, c1, c2);
        if (off % a[i].elem) fail(block, "misaligned", &a[i], c0, c1, c2);
        if (end > bytes) fail(block, "ends behind the block", &a[i], c0, c1, c2);
        for (int j = 0; j < i; j++) {
            const size_t o2 = (size_t)((char *)a[j].p - base), e2 = o2 + a[j].n * a[j].elem;
            if (off < e2 && o2 < end) fail(block, "overlaps an earlier array", &a[i], c0, c1, c2);
        }
        memset(a[i].p, 0xA5, a[i].n * a[i].elem);
    }
    n_checked++;
}
#define ALLOC(bytes) char *const base = (char *)malloc(bytes); if (!base) { fprintf(stderr, "out of memory\n"); exit(2); }

int main(void)
{
    static const size_t CELLS[] = { 0, 1, 3, 4, 5, 65535, 65536 }, FEATURES[] = { 0, 1, 7 }, LABELS[] = { 1, 2, 255 }, KS[] = { 0, 1, 2000 };
    const size_t k = 15, top = 2000;                        /* FASTF_NEIGHBORS_K, FASTF_HVG_TOP */
    for (size_t ci = 0; ci < sizeof CELLS / sizeof *CELLS; ci++) {
        const size_t n = CELLS[ci];
        {   const size_t bytes = res_cellsum_layout(NULL, n).bytes; ALLOC(bytes);
            res_cellsum_v v = res_cellsum_layout(base, n);
            span_t a[] = { SPAN(v, hist, 64, 0), SPAN(v, rpc, n, 512), SPAN(v, npc, n, 512 + 4 * n), SPAN(v, spc, n, 512 + 8 * n) };
            check("cellsum", base, bytes, 512 + n * 12, a, 4, n, 0, 0); free(base); }
        {   const size_t bytes = res_level_layout(NULL, n).bytes; ALLOC(bytes);
            res_level_v v = res_level_layout(base, n);
            span_t a[] = { SPAN(v, lo, n, 0), SPAN(v, hi, n, 8 * n), SPAN(v, probe, n, 16 * n), SPAN(v, ufull, n, 24 * n) };
            check("level", base, bytes, 4 * n * 8, a, 4, n, 0, 0); free(base); }
        {   const size_t bytes = res_fid_layout(NULL, n, 0).bytes; ALLOC(bytes);
            res_fid_v v = res_fid_layout(base, n, 0);
            span_t a[] = { SPAN(v, sxy, n, 0), SPAN(v, syy, n, 8 * n), SPAN(v, sxx, n, 2 * 8 * n) };
            check("fid", base, bytes, n * 24, a, 3, n, 0, 0); free(base); }
        {   const size_t bytes = res_fid_layout(NULL, n, 1).bytes; ALLOC(bytes);
            res_fid_v v = res_fid_layout(base, n, 1);
            span_t a[] = { SPAN(v, sxy, n, 0), SPAN(v, syy, n, 8 * n), SPAN(v, sxx, n, 16 * n), SPAN(v, ufull, n, 24 * n), SPAN(v, gfull, n, 32 * n) };
            check("fid pinned", base, bytes, n * 36, a, 5, n, 0, 0); free(base); }
        for (size_t fi = 0; fi < sizeof FEATURES / sizeof *FEATURES; fi++) {
            const size_t nf = FEATURES[fi], map = ((nf + 1) * 2 + 7) & ~(size_t)7, ix = map + n * 8;
            if (res_nbr_map_bytes(nf) != map) fail("nbr", "the bytes of the slot map moved", NULL, nf, 0, 0);
            {   const size_t bytes = res_nbr_layout(NULL, map, k, n).bytes; ALLOC(bytes);
                res_nbr_v v = res_nbr_layout(base, map, k, n);
                span_t a[] = { SPAN(v, map, nf + 1, 0), SPAN(v, norms, n, map), SPAN(v, idx[0], n * k, ix), SPAN(v, idx[1], n * k, ix + n * k * 4),
                               SPAN(v, cnt[0], n, ix + 2 * n * k * 4), SPAN(v, cnt[1], n, ix + 2 * n * k * 4 + n * 4), SPAN(v, shared, n, ix + 2 * n * k * 4 + 2 * n * 4) };
                check("nbr", base, bytes, map + n * (2 * k * 4 + 3 * 4 + 8), a, 7, map, k, n); free(base); }
            {   const size_t bytes = res_nbr_pin_layout(NULL, map, n, top).bytes; ALLOC(bytes);
                res_nbr_pin_v v = res_nbr_pin_layout(base, map, n, top);
                span_t a[] = { SPAN(v, map, nf + 1, 0), SPAN(v, kf, n, map), SPAN(v, kp, n, map + 4 * n), SPAN(v, sh, n, map + 8 * n), SPAN(v, genes, top, map + 12 * n) };
                check("nbr pinned", base, bytes, map + n * 12 + top * 4, a, 5, map, n, top); free(base); }
        }
        {   const size_t pc = (n + 1) & ~(size_t)1, half = 64 + 8 * pc;      /* --pseudotime: t, then three halves of census, est, valued */
            if (res_pt_cells(n) != pc) fail("pt", "pt_cells moved", NULL, n, 0, 0);
            const size_t bytes = res_pt_layout(NULL, pc).bytes; ALLOC(bytes);
            res_pt_v v = res_pt_layout(base, pc);
            span_t a[] = { SPAN(v, t, pc, 0),
                           SPAN(v, half[0].census, 8, 4 * pc), SPAN(v, half[0].est, pc, 4 * pc + 64), SPAN(v, half[0].valued, pc, 4 * pc + 64 + 4 * pc),
                           SPAN(v, half[1].census, 8, 4 * pc + half), SPAN(v, half[1].est, pc, 4 * pc + half + 64), SPAN(v, half[1].valued, pc, 4 * pc + half + 64 + 4 * pc),
                           SPAN(v, half[2].census, 8, 4 * pc + 2 * half), SPAN(v, half[2].est, pc, 4 * pc + 2 * half + 64), SPAN(v, half[2].valued, pc, 4 * pc + 2 * half + 64 + 4 * pc) };
            if (v.half_bytes != half) fail("pt", "the bytes of a half moved", NULL, pc, 0, 0);
            check("pt", base, bytes, 4 * pc + 3 * half, a, 10, pc, 0, 0); free(base); }
        for (size_t li = 0; li < sizeof LABELS / sizeof *LABELS; li++) {
            const size_t L = LABELS[li], lc = (n + 3) & ~(size_t)3, conf = L * (L + 1) * 4, half = 3 * lc + conf;
            if (res_lab_cells(n) != lc) fail("lab", "lab_cells moved", NULL, n, 0, 0);
            const size_t bytes = res_lab_layout(NULL, lc, L).bytes; ALLOC(bytes);
            res_lab_v v = res_lab_layout(base, lc, L);
            span_t a[] = { SPAN(v, lab, lc, 0),
                           SPAN(v, half[0].pred, lc, lc), SPAN(v, half[0].same, lc, lc + lc), SPAN(v, half[0].labelled, lc, lc + 2 * lc), SPAN(v, half[0].conf, L * (L + 1), lc + 3 * lc),
                           SPAN(v, half[1].pred, lc, lc + half), SPAN(v, half[1].same, lc, lc + half + lc), SPAN(v, half[1].labelled, lc, lc + half + 2 * lc),
                           SPAN(v, half[1].conf, L * (L + 1), lc + half + 3 * lc) };
            if (v.half_bytes != half) fail("lab", "the bytes of a half moved", NULL, lc, L, 0);
            check("lab", base, bytes, lc + 2 * half, a, 9, lc, L, 0); free(base);
        }
    }
    for (size_t fi = 0; fi < sizeof FEATURES / sizeof *FEATURES; fi++) {
        const size_t n = FEATURES[fi] + 1;                  /* (the per-gene arrays have n_features + 1 entries) */
        for (size_t m = n - 1; m <= n; m++) {
            const size_t bytes = res_gfid_layout(NULL, m).bytes; ALLOC(bytes);
            res_gfid_v v = res_gfid_layout(base, m);
            span_t a[] = { SPAN(v, sx, m, 0), SPAN(v, sxx, m, 8 * m), SPAN(v, sy, m, 2 * 8 * m), SPAN(v, syy, m, 3 * 8 * m), SPAN(v, sxy, m, 4 * 8 * m),
                           SPAN(v, cf, m, 5 * 8 * m), SPAN(v, c, m, 5 * 8 * m + 4 * m) };
            check("gfid", base, bytes, m * 48, a, 7, m, 0, 0); free(base);
        }
    }
    for (size_t li = 0; li < sizeof LABELS / sizeof *LABELS; li++) for (size_t ki = 0; ki < sizeof KS / sizeof *KS; ki++) {
        const size_t L = LABELS[li], K = KS[ki], W = L * K, want = L * K * 20 + ((L + 1) & ~(size_t)1) * 4;
        const size_t bytes = res_mk_layout(NULL, L, K).bytes; ALLOC(bytes);
        res_mk_v v = res_mk_layout(base, L, K);
        span_t a[] = { SPAN(v, s2u, W, 0), SPAN(v, sum, W, 8 * W), SPAN(v, det, W, 2 * 8 * W), SPAN(v, npl, L, 2 * 8 * W + 4 * W) };
        if (res_mk_set_bytes(L, K) != ((want + 7) & ~(size_t)7)) fail("mk", "the bytes of a pinned set moved", NULL, L, K, 0);
        check("mk", base, bytes, want, a, 4, L, K, 0); free(base);
    }
    for (size_t fi = 0; fi < sizeof FEATURES / sizeof *FEATURES; fi++) for (size_t ki = 0; ki < sizeof KS / sizeof *KS; ki++) {      /* --coexpression: K genes of A */
        const size_t nf = FEATURES[fi], K = KS[ki], map = res_nbr_map_bytes(nf), ix = K * K * 8 + K * 8 + map;
        {   const size_t bytes = res_cx_layout(NULL, map, k, K).bytes; ALLOC(bytes);
            res_cx_v v = res_cx_layout(base, map, k, K);
            span_t a[] = { SPAN(v, D, K * K, 0), SPAN(v, S, K, K * K * 8), SPAN(v, map, nf + 1, K * K * 8 + K * 8), SPAN(v, idx[0], K * k, ix), SPAN(v, idx[1], K * k, ix + K * k * 4),
                           SPAN(v, cnt[0], K, ix + 2 * K * k * 4), SPAN(v, cnt[1], K, ix + 2 * K * k * 4 + K * 4), SPAN(v, shared, K, ix + 2 * K * k * 4 + 2 * K * 4) };
            check("cx", base, bytes, ix + K * (2 * k * 4 + 3 * 4), a, 8, map, k, K); free(base); }
        {   const size_t bytes = res_cx_pin_layout(NULL, map, K).bytes; ALLOC(bytes);
            res_cx_pin_v v = res_cx_pin_layout(base, map, K);
            span_t a[] = { SPAN(v, map, nf + 1, 0), SPAN(v, kf, K, map), SPAN(v, kp, K, map + 4 * K), SPAN(v, sh, K, map + 8 * K), SPAN(v, genes, K, map + 12 * K) };
            check("cx pinned", base, bytes, map + 16 * K, a, 5, map, K, 0); free(base); }
    }
    {   uint32_t rows[3 * 5]; const res_rows_t r = res_rows(rows, 5);      /* the row triple: N entries apart */
        if (r.f != rows || r.c != rows + 5 || r.k != rows + 10) fail("rows", "the row arrays moved", NULL, 5, 0, 0); }
    printf("res_layout_check: %lu layouts hold\n", n_checked);
    return 0;
}
