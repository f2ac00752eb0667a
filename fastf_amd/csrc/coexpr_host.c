/*
 * coexpr_host.c — co-expression partners against full depth on the host: the range rule, the definition in plain C
 * (fastf_coexpr_from_coo, fastf_coexpr_select) and the per-gene and per-point rows.  The definition is in include/fastf_amd.h, the
 * order in coexpr_order.h.
 */
#define _GNU_SOURCE
#include "fastf_amd.h"
#include "host_io.h"
#include "coexpr_order.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int cx_err(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static int cx_err(const char *fmt, ...)
{
    char buf[480];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    fastf_set_error_(buf);
    return 1;
}

int fastf_coexpr_check_range(uint32_t n_cells, uint64_t max_q)
{
    if (((unsigned __int128)n_cells * max_q) >> 63)
        return cx_err("FASTF_ERR_COEXPR_RANGE: %u cells times a gene's sum of squares %llu over the highly variable genes is 2^63 or more: the order of --coexpression does not hold it",
                      n_cells, (unsigned long long)max_q);
    return 0;
}

/* D_gh <= n (2^(7P) - 1)^2 must stay in u64 */
int fastf_coexpr_check_gram(uint32_t n_cells, uint32_t planes)
{
    if (planes < 1 || planes > FASTF_COEXPR_MAX_PLANES) return cx_err("coexpression: %u planes, from 1 to %u", planes, FASTF_COEXPR_MAX_PLANES);
    const uint64_t top = (1ull << (7u * planes)) - 1u;
    if (((unsigned __int128)n_cells * top * top) >> 64)
        return cx_err("FASTF_ERR_COEXPR_CELLS: %u cells with counts of %u planes: a sum of products does not fit 64 bits", n_cells, planes);
    return 0;
}

static int cmp_u32(const void *a, const void *b) { const uint32_t x = *(const uint32_t *)a, y = *(const uint32_t *)b; return x < y ? -1 : x > y; }

/* the partner sets of D, S over n cells: idx[g * k + s], s < cnt[g], ascending; the other slots UINT32_MAX */
int fastf_coexpr_select(const uint64_t *D, const uint64_t *S, uint32_t n_cells, uint32_t K, uint32_t k, uint32_t *idx, uint32_t *cnt)
{
    if (k < 1 || k > FASTF_COEXPR_MAX_K) return cx_err("coexpression: k = %u, from 1 to %u", k, FASTF_COEXPR_MAX_K);
    if (K > FASTF_COEXPR_MAX_GENES) return cx_err("coexpression: %u genes, at most %u", K, FASTF_COEXPR_MAX_GENES);
    if (K && (!D || !S || !idx || !cnt)) return cx_err("null argument");
    uint64_t max_q = 0;
    for (uint32_t g = 0; g < K; g++) if (D[(size_t)g * K + g] > max_q) max_q = D[(size_t)g * K + g];
    if (fastf_coexpr_check_range(n_cells, max_q)) return 1;
    uint64_t *V = (uint64_t *)malloc(((size_t)K + 1) * sizeof *V);
    if (!V) return cx_err("out of memory");
    for (uint32_t g = 0; g < K; g++) V[g] = (uint64_t)((unsigned __int128)n_cells * D[(size_t)g * K + g] - (unsigned __int128)S[g] * S[g]);
    for (uint32_t g = 0; g < K; g++) {
        uint32_t *const out = idx + (size_t)g * k;
        uint64_t bc[FASTF_COEXPR_MAX_K];
        uint32_t have = 0;
        for (uint32_t h = 0; h < K; h++) {
            const __int128 c = coex_cov(n_cells, D[(size_t)g * K + h], S[g], S[h]);
            if (h == g || c <= 0) continue;
            /* out[0 .. have) in the order of the definition, best first; a later slot never precedes an equal earlier one */
            uint32_t at = have;
            while (at > 0 && coex_precedes((uint64_t)c, V[h], h, bc[at - 1], V[out[at - 1]], out[at - 1])) at--;
            if (at >= k) continue;
            const uint32_t last = have < k ? have : k - 1;
            for (uint32_t s = last; s > at; s--) { out[s] = out[s - 1]; bc[s] = bc[s - 1]; }
            out[at] = h; bc[at] = (uint64_t)c;
            if (have < k) have++;
        }
        qsort(out, have, sizeof *out, cmp_u32);
        for (uint32_t s = have; s < k; s++) out[s] = UINT32_MAX;
        cnt[g] = have;
    }
    free(V);
    return 0;
}

int fastf_coexpr_from_coo(const fastf_coo_t *m, uint32_t n_cells, const uint16_t *slot_map, uint32_t n_features, uint32_t K, uint32_t k,
                          uint32_t *idx, uint32_t *cnt, uint64_t *D_out, uint64_t *S_out)
{
    if (!m || !slot_map || (K && (!idx || !cnt)) || (m->nnz && (!m->feature || !m->cell || !m->count))) return cx_err("null argument");
    if (k < 1 || k > FASTF_COEXPR_MAX_K) return cx_err("coexpression: k = %u, from 1 to %u", k, FASTF_COEXPR_MAX_K);
    if (K > FASTF_COEXPR_MAX_GENES) return cx_err("coexpression: %u genes, at most %u", K, FASTF_COEXPR_MAX_GENES);
    int rc = 1;
    /* the rows with a slot, cell by cell (a counting sort by cell): slot and count */
    size_t *start = (size_t *)calloc((size_t)n_cells + 2, sizeof *start);
    uint64_t *D = D_out ? D_out : (uint64_t *)malloc(((size_t)K * K + 1) * sizeof *D), *S = S_out ? S_out : (uint64_t *)malloc(((size_t)K + 1) * sizeof *S);
    uint32_t *rs = NULL, *rv = NULL;
    if (!start || !D || !S) { cx_err("out of memory"); goto done; }
    memset(D, 0, (size_t)K * K * sizeof *D); memset(S, 0, (size_t)K * sizeof *S);
    size_t kept = 0;
    uint32_t max_count = 0;
    for (size_t r = 0; r < m->nnz; r++) {
        const uint32_t c = m->cell[r] - 1u, f = m->feature[r];
        if (c >= n_cells || f - 1u >= n_features || slot_map[f] >= K) continue;
        start[c + 2]++; kept++;
        if (m->count[r] > max_count) max_count = m->count[r];
    }
    if (max_count >> 21) {
        cx_err("fastf_coexpr_from_coo: FASTF_ERR_NEIGHBOR_COUNT: a count of %u among the highly variable genes needs more than %u planes of 7 bits", max_count, FASTF_COEXPR_MAX_PLANES);
        goto done;
    }
    if (fastf_coexpr_check_gram(n_cells, max_count < (1u << 7) ? 1u : max_count < (1u << 14) ? 2u : 3u)) goto done;
    for (uint32_t c = 0; c < n_cells; c++) start[c + 2] += start[c + 1];
    rs = (uint32_t *)malloc((kept + 1) * sizeof *rs); rv = (uint32_t *)malloc((kept + 1) * sizeof *rv);
    if (!rs || !rv) { cx_err("out of memory"); goto done; }
    for (size_t r = 0; r < m->nnz; r++) {
        const uint32_t c = m->cell[r] - 1u, f = m->feature[r];
        if (c >= n_cells || f - 1u >= n_features || slot_map[f] >= K) continue;
        const size_t at = start[c + 1]++;
        rs[at] = slot_map[f]; rv[at] = m->count[r];
    }
    for (uint32_t c = 0; c < n_cells; c++)                                  /* (start[c] .. start[c + 1]: the rows of cell c) */
        for (size_t a = start[c]; a < start[c + 1]; a++) {
            S[rs[a]] += rv[a];
            uint64_t *const row = D + (size_t)rs[a] * K;
            for (size_t b = start[c]; b < start[c + 1]; b++) row[rs[b]] += (uint64_t)rv[a] * rv[b];
        }
    rc = fastf_coexpr_select(D, S, n_cells, K, k, idx, cnt);
done:
    free(start); free(rs); free(rv);
    if (!D_out) free(D);
    if (!S_out) free(S);
    return rc;
}

/* ------------------------------------------------------------------ */
/* the rows                                                            */
/* ------------------------------------------------------------------ */
const char *fastf_coexpr_header(void) { return "gene\tk_full\tk_point\tshared\n"; }   /* (the per-verb headers: grid_rows.c, GRID_TABLES) */

int fastf_coexpr_row(const char *gene, uint32_t k_full, uint32_t k_point, uint32_t shared, char *buf, size_t cap)
{
    if (!gene || !buf) return cx_err("null argument");
    const int n = snprintf(buf, cap, "%s\t%u\t%u\t%u\n", gene, k_full, k_point, shared);
    return (n < 0 || (size_t)n >= cap) ? cx_err("coexpression row too long") : 0;
}

int fastf_coexpr_summary_row(float rate_cell, float rate_depth, uint64_t list_value, uint32_t seed, uint32_t n_cells, uint32_t hvg_k, uint32_t k,
                             const uint32_t *k_full, const uint32_t *k_point, const uint32_t *shared, char *buf, size_t cap)
{
    if (!buf || (hvg_k && (!k_full || !k_point || !shared))) return cx_err("null argument");
    uint64_t nd = 0, kf = 0, kp = 0, sh = 0, half = 0;
    double kept = 0.0;
    for (uint32_t g = 0; g < hvg_k; g++) {
        kf += k_full[g]; kp += k_point[g]; sh += shared[g];
        if (!k_full[g]) continue;
        nd++;
        kept += (double)shared[g] / (double)k_full[g];
        half += 2ull * shared[g] >= k_full[g];
    }
    char mean[40], second[32];
    if (nd) snprintf(mean, sizeof mean, "%.6f", kept / (double)nd); else snprintf(mean, sizeof mean, "NA");
    if (list_value) snprintf(second, sizeof second, "%llu", (unsigned long long)list_value);
    else snprintf(second, sizeof second, "%.3f", (double)rate_depth);
    const int n = snprintf(buf, cap, "%.3f\t%s\t%u\t%u\t%u\t%u\t%llu\t%llu\t%llu\t%llu\t%s\t%llu\n", (double)rate_cell, second, seed, n_cells, hvg_k, k,
                           (unsigned long long)nd, (unsigned long long)kf, (unsigned long long)kp, (unsigned long long)sh, mean, (unsigned long long)half);
    return (n < 0 || (size_t)n >= cap) ? cx_err("summary row too long") : 0;
}
