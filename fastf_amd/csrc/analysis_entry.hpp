// analysis_entry.hpp — the fastf_dev_* entry points of the grid verbs' analyses (--genes, --cells, --fidelity, --gene-fidelity,
// --neighbors, --mapping, --labels, --pseudotime, --markers, cap's hit counts and decision plane, level's search step): launch wrappers around the kernels
// of the headers below.  Included by umi_engine.hip behind the engine core; what they keep on an engine is its AnalysisState.
#pragma once
#include "cap_kernels.hpp"
#include "level_kernels.hpp"
#include "gene_kernels.hpp"
#include "cells_kernels.hpp"
#include "fidelity_kernels.hpp"
#include "gene_fidelity_kernels.hpp"
#include "neighbors_kernels.hpp"
#include "mapping_kernels.hpp"
#include "coexpr_kernels.hpp"
#include "labels_kernels.hpp"
#include "ptime_kernels.hpp"
#include "markers_kernels.hpp"

// Per-cell summary of COO rows ascending by (cell, feature) (cell_summary_kernel): d_umis_per_cell[c - 1] = sum of the counts of
// cell c, d_genes_per_cell[c - 1] = its rows with count >= 1, d_umis_per_cell[n_cells] = the sum of all counts.  Both arrays are
// cleared here first; *d_nnz rows are read.
extern "C" int fastf_dev_cell_summary(fastf_engine_t* e, const uint32_t* d_cell, const uint32_t* d_count, const uint64_t* d_nnz, uint32_t n_cells,
                                      uint64_t* d_umis_per_cell, uint32_t* d_genes_per_cell, void* stream) FASTF_TRY {
    DEV_ENTRY(!e || !d_nnz || !d_umis_per_cell || (n_cells && !d_genes_per_cell), "null argument");
    hipStream_t s = (hipStream_t)stream;
    HIP_OK(hipMemsetAsync(d_umis_per_cell, 0, ((size_t)n_cells + 1) * sizeof(u64), s));
    if (n_cells) HIP_OK(hipMemsetAsync(d_genes_per_cell, 0, (size_t)n_cells * sizeof(u32), s));
    if (!d_cell || !d_count) return 0;                  // (no row buffer: a reduce of nothing)
    hipLaunchKernelGGL(cell_summary_kernel, dim3(2 * e->grid_cus), dim3(256), 0, s, d_cell, d_count, (const u64*)d_nnz, n_cells,
                       (u64*)d_umis_per_cell, d_genes_per_cell);
    HIP_OK(hipGetLastError());
    dbg_sync(s, "cell summary");
    return 0;
} FASTF_CATCH_INT

// The dynamic-LDS limit of `kernels`, set on the engine's first use of them: the attribute belongs to the current device's function,
// so `done` is a flag of the engine.
template <typename K>
static int lds_attr_once(bool& done, size_t bytes, K* const* kernels, size_t n) {
    if (done) return 0;
    for (size_t i = 0; i < n; ++i) HIP_OK(hipFuncSetAttribute((const void*)kernels[i], hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    done = true;
    return 0;
}

// The launch plan of a ranged histogram (ranged_hist.hpp) over n_bins bins: up to max_ranges ranges of bins_per_range bins take the
// LDS form, each range with its own share of the workgroups (every range reads all rows); <env>=<k> lowers that (0: the general
// form always — tests, A/B runs) and is read at each call.  per_cu: the workgroups a CU holds with lds_bytes of counters each.
struct HistSpec { u32 n_bins, bins_per_range, max_ranges; const char* env; size_t bytes_per_bin; };
struct HistPlan { bool lds_form; u32 n_ranges; size_t lds_bytes; u32 per_cu; };
static HistPlan hist_plan(const HistSpec& sp) {
    u32 max_ranges = sp.max_ranges;
    const char* mr = getenv(sp.env);
    if (mr) max_ranges = std::min<u32>((u32)atoi(mr), max_ranges);
    const u32 n_ranges = (sp.n_bins + sp.bins_per_range - 1) / sp.bins_per_range;
    const size_t lds_bytes = (size_t)std::min<u32>(sp.n_bins, sp.bins_per_range) * sp.bytes_per_bin;
    return {n_ranges <= max_ranges, n_ranges, lds_bytes, lds_bytes <= 80u * 1024u ? 2u : 1u};
}

// One ranged histogram launched: lds_kernel (K<true>) by hist_plan's word, every range with per_cu * CUs / n_ranges workgroups (one
// at the least), else general_kernel (K<false>) with two workgroups a CU; neither with more than max_groups, the workgroups the
// work fills (NO_GROUP_CAP: the row count lives on the device, the grid is sized by the device alone).  The dynamic-LDS limit of the
// LDS form is a whole range's (family: its flag in AnalysisState); n_ranges goes behind `args` as the kernels' last argument.
constexpr u64 NO_GROUP_CAP = ~0ull;
template <typename K, typename... Args>
static int launch_ranged(fastf_engine* e, hipStream_t s, const char* what, K* lds_kernel, K* general_kernel, int family, const HistSpec& sp,
                         u32 threads, u64 max_groups, Args... args) {
    const HistPlan pl = hist_plan(sp);
    if (pl.lds_form) {
        if (lds_attr_once(e->an.attr[family], (size_t)sp.bins_per_range * sp.bytes_per_bin, &lds_kernel, 1)) return 1;
        const u32 groups = (u32)std::max<u64>(1, std::min<u64>(max_groups, (u64)pl.per_cu * e->grid_cus / pl.n_ranges));
        hipLaunchKernelGGL(lds_kernel, dim3(groups * pl.n_ranges), dim3(threads), pl.lds_bytes, s, args..., pl.n_ranges);
    } else {
        hipLaunchKernelGGL(general_kernel, dim3((u32)std::min<u64>(max_groups, 2ull * e->grid_cus)), dim3(threads), 0, s, args..., 1u);
    }
    HIP_OK(hipGetLastError());
    dbg_sync(s, what);
    return 0;
}

// The end of the two joins (fastf_dev_fidelity, fastf_dev_partner_counts): waits for the stream, reads the error word back and fails
// in `fn`'s name when a point row had no partner.
static int join_end(const char* fn, hipStream_t s, const u64* err) {
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(s));
    u64 bits = 0;
    if (copy_d2h(&bits, err, sizeof bits)) return 1;
    if (bits & ERR_NO_PARTNER) return set_err("%s: a point row has no partner among the full rows (device error bits 0x%llx)", fn, (unsigned long long)bits);
    return 0;
}

// --fidelity: a point's rows joined with the full-depth rows of its (cell rate, seed) pair (fidelity_kernel).  Both row sets ascend
// by (cell, feature) and every point row has its partner among the full rows; d_sum_xy[c - 1] = the sum of x * y over the point
// rows of cell c, d_sum_yy[c - 1] = the sum of y * y.  Both arrays are cleared here first; *d_nnz_full and *d_nnz rows are read.
// d_err: the word a missing partner raises FASTF_ERR_NO_PARTNER in (NULL: the engine's own error word).  Synchronises the stream
// and fails when that bit is set in the word, whichever call raised it: clear it to go on.
static_assert(ERR_NO_PARTNER == FASTF_ERR_NO_PARTNER, "the error bit of fidelity_kernel and the ABI's");
extern "C" int fastf_dev_fidelity(fastf_engine_t* e, const uint32_t* d_feature_full, const uint32_t* d_cell_full, const uint32_t* d_count_full,
                                  const uint64_t* d_nnz_full, const uint32_t* d_feature, const uint32_t* d_cell, const uint32_t* d_count,
                                  const uint64_t* d_nnz, uint32_t n_cells, uint64_t* d_sum_xy, uint64_t* d_sum_yy, uint64_t* d_err, void* stream) FASTF_TRY {
    DEV_ENTRY(!e || !d_nnz_full || !d_nnz || (n_cells && (!d_sum_xy || !d_sum_yy)), "null argument");
    hipStream_t s = (hipStream_t)stream;
    if (n_cells) {
        HIP_OK(hipMemsetAsync(d_sum_xy, 0, (size_t)n_cells * sizeof(u64), s));
        HIP_OK(hipMemsetAsync(d_sum_yy, 0, (size_t)n_cells * sizeof(u64), s));
    }
    if (!d_feature || !d_cell || !d_count) return 0;    // (no row buffer: a join of nothing)
    if (!d_feature_full || !d_cell_full || !d_count_full) return set_err("fastf_dev_fidelity: point rows and no full rows");
    u64* const err = d_err ? (u64*)d_err : err_word(e);
    hipLaunchKernelGGL(fidelity_kernel, dim3(FID_BLOCKS_PER_CU * e->grid_cus), dim3(FID_THREADS), 0, s, d_feature_full, d_cell_full, d_count_full,
                       (const u64*)d_nnz_full, d_feature, d_cell, d_count, (const u64*)d_nnz, n_cells, (u64*)d_sum_xy, (u64*)d_sum_yy, err);
    return join_end("fastf_dev_fidelity", s, err);
} FASTF_CATCH_INT

// Per-gene summary of COO rows in any order (gene_summary_kernel): d_cells_per_gene[g - 1] = rows of gene g with count >= 1,
// d_umis_per_gene[g - 1] = the sum of their counts.  Both arrays are cleared here first; *d_nnz rows are read.  The sum of all
// counts is below 2^32 (the LDS form keeps both numbers of a gene in one 64-bit counter).
extern "C" int fastf_dev_gene_summary(fastf_engine_t* e, const uint32_t* d_feature, const uint32_t* d_count, const uint64_t* d_nnz, uint32_t n_features,
                                      uint32_t* d_cells_per_gene, uint64_t* d_umis_per_gene, void* stream) FASTF_TRY {
    DEV_ENTRY(!e || !d_nnz || (n_features && (!d_cells_per_gene || !d_umis_per_gene)), "null argument");
    hipStream_t s = (hipStream_t)stream;
    if (!n_features) return 0;
    HIP_OK(hipMemsetAsync(d_cells_per_gene, 0, (size_t)n_features * sizeof(u32), s));
    HIP_OK(hipMemsetAsync(d_umis_per_gene, 0, (size_t)n_features * sizeof(u64), s));
    if (!d_feature || !d_count) return 0;               // (no row buffer: a reduce of nothing)
    return launch_ranged(e, s, "gene summary", gene_summary_kernel<true>, gene_summary_kernel<false>, AN_GENE_SUMMARY,
                         {n_features, GENE_LDS_GENES, GENE_LDS_RANGES, "FASTF_GENE_LDS_RANGES", sizeof(u64)}, GENE_THREADS, NO_GROUP_CAP,
                         d_feature, d_count, (const u64*)d_nnz, n_features, d_cells_per_gene, (u64*)d_umis_per_gene);
} FASTF_CATCH_INT

// --gene-fidelity: d_x[i] = the count of the full row with the (cell, feature) of point row i (partner_counts_kernel): the join of
// fastf_dev_fidelity, stored per row.  Both row sets ascend by (cell, feature); *d_nnz_full and *d_nnz rows are read, *d_nnz entries of
// d_x are written.  d_err, the synchronisation and the failure on FASTF_ERR_NO_PARTNER: as fastf_dev_fidelity; such a row gets x = 0.
extern "C" int fastf_dev_partner_counts(fastf_engine_t* e, const uint32_t* d_feature_full, const uint32_t* d_cell_full, const uint32_t* d_count_full,
                                        const uint64_t* d_nnz_full, const uint32_t* d_feature, const uint32_t* d_cell, const uint64_t* d_nnz,
                                        uint32_t* d_x, uint64_t* d_err, void* stream) FASTF_TRY {
    DEV_ENTRY(!e || !d_nnz_full || !d_nnz, "null argument");
    hipStream_t s = (hipStream_t)stream;
    if (!d_feature || !d_cell) return 0;                // (no row buffer: a join of nothing)
    if (!d_x) return set_err("fastf_dev_partner_counts: point rows and no partner column");
    if (!d_feature_full || !d_cell_full || !d_count_full) return set_err("fastf_dev_partner_counts: point rows and no full rows");
    u64* const err = d_err ? (u64*)d_err : err_word(e);
    hipLaunchKernelGGL(partner_counts_kernel, dim3(FID_BLOCKS_PER_CU * e->grid_cus), dim3(FID_THREADS), 0, s, d_feature_full, d_cell_full, d_count_full,
                       (const u64*)d_nnz_full, d_feature, d_cell, (const u64*)d_nnz, d_x, err);
    return join_end("fastf_dev_partner_counts", s, err);
} FASTF_CATCH_INT

// --gene-fidelity: per gene the sums of a * b and of b * b over rows (feature, a, b) in any order (gene_moments_kernel):
// d_sum_ab[g - 1] and d_sum_bb[g - 1], u64, n_features entries each, cleared here first; *d_nnz rows are read.  Every sum stays below
// 2^64 (the sum of all counts is below 2^32).  d_sum_ab == NULL: sum_bb alone.  Stream-ordered.
extern "C" int fastf_dev_gene_moments(fastf_engine_t* e, const uint32_t* d_feature, const uint32_t* d_a, const uint32_t* d_b, const uint64_t* d_nnz,
                                      uint32_t n_features, uint64_t* d_sum_ab, uint64_t* d_sum_bb, void* stream) FASTF_TRY {
    DEV_ENTRY(!e || !d_nnz || (n_features && !d_sum_bb), "null argument");
    hipStream_t s = (hipStream_t)stream;
    if (!n_features) return 0;
    if (d_sum_ab) HIP_OK(hipMemsetAsync(d_sum_ab, 0, (size_t)n_features * sizeof(u64), s));
    HIP_OK(hipMemsetAsync(d_sum_bb, 0, (size_t)n_features * sizeof(u64), s));
    if (!d_feature || !d_a || !d_b) return 0;           // (no row buffer: a reduce of nothing)
    return launch_ranged(e, s, "gene moments", gene_moments_kernel<true>, gene_moments_kernel<false>, AN_GENE_MOMENTS,
                         {n_features, GMOM_LDS_GENES, GMOM_LDS_RANGES, "FASTF_GENE_MOMENTS_LDS_RANGES", 2 * sizeof(u64)}, GENE_THREADS, NO_GROUP_CAP,
                         d_feature, d_a, d_b, (const u64*)d_nnz, n_features, (u64*)d_sum_ab, (u64*)d_sum_bb);
} FASTF_CATCH_INT

// --neighbors: the dense byte planes of the rows whose gene is in A (neighbors_kernels.hpp).  d_slot_map: u16[n_features + 1], the slot
// of feature f in A (0 .. K - 1) or 0xFFFF.  The largest count among those rows decides P (one max reduction, read back here):
// 1 plane below 2^7, 2 below 2^14, 3 below 2^21; beyond that the call fails by name.  d_planes == NULL: *planes_out = P alone.  Otherwise
// P * n_pad * K_pad bytes (fastf_neighbors_pad) are zeroed and filled, and planes_bytes must hold them.  Synchronises the stream once.
extern "C" int fastf_dev_neighbor_planes(fastf_engine_t* e, const uint32_t* d_feature, const uint32_t* d_cell, const uint32_t* d_count,
                                         const uint64_t* d_nnz, const uint16_t* d_slot_map, uint32_t n_features, uint32_t n_cells, uint32_t K,
                                         void* d_planes, size_t planes_bytes, uint32_t* planes_out, void* stream) FASTF_TRY {
    DEV_ENTRY(!e || !d_nnz || !planes_out, "null argument");
    hipStream_t s = (hipStream_t)stream;
    if (K > NBR_MAX_GENES) return set_err("fastf_dev_neighbor_planes: %u genes, at most %u", K, NBR_MAX_GENES);
    const bool rows = d_feature && d_cell && d_count && d_slot_map;      // (no row buffer: planes of nothing)
    u32 max_count = 0;
    if (rows) {
        if (e->an.d_nbr.ensure(64)) return 1;
        u32* const d_max = (u32*)e->an.d_nbr.p;
        HIP_OK(hipMemsetAsync(d_max, 0, 64, s));
        hipLaunchKernelGGL(nbr_max_count_kernel, dim3(4 * e->grid_cus), dim3(256), 0, s, d_feature, d_count, (const u64*)d_nnz, d_slot_map, n_features, d_max);
        HIP_OK(hipGetLastError());
        HIP_OK(hipStreamSynchronize(s));
        if (copy_d2h(&max_count, d_max, sizeof max_count)) return 1;
    }
    const u32 P = max_count < (1u << 7) ? 1u : max_count < (1u << 14) ? 2u : max_count < (1u << 21) ? 3u : 4u;
    if (P > NBR_MAX_PLANES)
        return set_err("fastf_dev_neighbor_planes: FASTF_ERR_NEIGHBOR_COUNT: a count of %u among the highly variable genes needs more than %u planes of 7 bits", max_count, NBR_MAX_PLANES);
    *planes_out = P;
    if (!d_planes) return 0;
    uint32_t n_pad = 0, K_pad = 0;
    fastf_neighbors_pad(n_cells, K, &n_pad, &K_pad);
    const size_t need = (size_t)P * n_pad * K_pad;
    if (need > planes_bytes) return set_err("fastf_dev_neighbor_planes: %u planes of %u x %u bytes need %zu bytes, the buffer has %zu", P, n_pad, K_pad, need, planes_bytes);
    HIP_OK(hipMemsetAsync(d_planes, 0, need, s));
    if (rows && K && n_cells) {
        hipLaunchKernelGGL(nbr_planes_kernel, dim3(4 * e->grid_cus), dim3(256), 0, s, d_feature, d_cell, d_count, (const u64*)d_nnz, d_slot_map, n_features,
                           n_cells, K, n_pad, K_pad, P, (unsigned char*)d_planes);
        HIP_OK(hipGetLastError());
    }
    dbg_sync(s, "neighbor planes");
    return 0;
} FASTF_CATCH_INT

// --neighbors: the norms, then the Gram products and the selection (nbr_norms_kernel, nbr_gram_kernel).  d_planes: what
// fastf_dev_neighbor_planes filled for (n_cells, K) with `planes` planes.  d_norms[i] = v_i . v_i (u64, n_cells); *max_norm_out its maximum,
// read back before the selection starts: fastf_neighbors_check_norm refuses 2^42 and beyond and nothing more is launched.  Then
// d_idx[i * k + s], s < d_cnt[i], are the neighbours of cell i (0-based indices, ascending; the other slots 0xFFFFFFFF), k from 1 to 64.
// The dot products come from the i8 MFMA, under FASTF_NEIGHBORS_MFMA=0 from ordinary integer instructions: the same numbers.
extern "C" int fastf_dev_neighbors(fastf_engine_t* e, const void* d_planes, uint32_t planes, uint32_t n_cells, uint32_t K, uint32_t k,
                                   uint32_t* d_idx, uint32_t* d_cnt, uint64_t* d_norms, uint64_t* max_norm_out, void* stream) FASTF_TRY {
    DEV_ENTRY(!e, "null argument");
    hipStream_t s = (hipStream_t)stream;
    if (k < 1 || k > NBR_MAX_K) return set_err("fastf_dev_neighbors: k = %u, from 1 to %u", k, NBR_MAX_K);
    if (planes < 1 || planes > NBR_MAX_PLANES) return set_err("fastf_dev_neighbors: %u planes, from 1 to %u", planes, NBR_MAX_PLANES);
    if (K > NBR_MAX_GENES) return set_err("fastf_dev_neighbors: %u genes, at most %u", K, NBR_MAX_GENES);
    if (max_norm_out) *max_norm_out = 0;
    if (!n_cells) return 0;
    if (!d_planes || !d_idx || !d_cnt || !d_norms) return set_err("fastf_dev_neighbors: null argument");
    uint32_t n_pad = 0, K_pad = 0;
    fastf_neighbors_pad(n_cells, K, &n_pad, &K_pad);
    if (e->an.d_nbr.ensure(64)) return 1;
    u64* const d_max = (u64*)e->an.d_nbr.p + 1;
    HIP_OK(hipMemsetAsync(d_max, 0, sizeof(u64), s));
    hipLaunchKernelGGL(nbr_norms_kernel, dim3(std::min<u32>((n_cells + 3) / 4, 8 * e->grid_cus)), dim3(256), 0, s, (const unsigned char*)d_planes, n_cells, n_pad, K_pad,
                       planes, (u64*)d_norms, d_max);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(s));
    u64 max_norm = 0;
    if (copy_d2h(&max_norm, d_max, sizeof max_norm)) return 1;
    if (max_norm_out) *max_norm_out = max_norm;
    if (fastf_neighbors_check_norm(max_norm)) return 1;
    const char* mf = getenv("FASTF_NEIGHBORS_MFMA");
    const bool mfma = !(mf && mf[0] == '0');
    static constexpr decltype(&nbr_gram_kernel<1, false>) gram[NBR_MAX_PLANES][2] = {     // [planes - 1][mfma]
        {nbr_gram_kernel<1, false>, nbr_gram_kernel<1, true>}, {nbr_gram_kernel<2, false>, nbr_gram_kernel<2, true>}, {nbr_gram_kernel<3, false>, nbr_gram_kernel<3, true>}};
    if (lds_attr_once(e->an.attr[AN_NBR_GRAM], (size_t)NBR_WAVES * nbr_wave_words(NBR_MAX_K) * sizeof(u64), gram[0], 2 * NBR_MAX_PLANES)) return 1;
    hipLaunchKernelGGL(gram[planes - 1][mfma], dim3((n_cells + NBR_ROWS - 1) / NBR_ROWS), dim3(NBR_THREADS), (size_t)NBR_WAVES * nbr_wave_words(k) * sizeof(u64), s,
                       (const unsigned char*)d_planes, n_cells, n_pad, K_pad, k, (const u64*)d_norms, d_idx, d_cnt);
    HIP_OK(hipGetLastError());
    dbg_sync(s, "neighbors");
    return 0;
} FASTF_CATCH_INT

// --neighbors: d_shared[i] = the number of cells in both neighbour sets of cell i (nbr_shared_kernel); the sets as fastf_dev_neighbors
// leaves them, both with the same k.  Stream-ordered.
extern "C" int fastf_dev_neighbors_shared(fastf_engine_t* e, const uint32_t* d_idx_a, const uint32_t* d_cnt_a, const uint32_t* d_idx_b,
                                          const uint32_t* d_cnt_b, uint32_t n_cells, uint32_t k, uint32_t* d_shared, void* stream) FASTF_TRY {
    DEV_ENTRY(!e, "null argument");
    hipStream_t s = (hipStream_t)stream;
    if (k < 1 || k > NBR_MAX_K) return set_err("fastf_dev_neighbors_shared: k = %u, from 1 to %u", k, NBR_MAX_K);
    if (!n_cells) return 0;
    if (!d_idx_a || !d_cnt_a || !d_idx_b || !d_cnt_b || !d_shared) return set_err("fastf_dev_neighbors_shared: null argument");
    hipLaunchKernelGGL(nbr_shared_kernel, dim3((n_cells + 255) / 256), dim3(256), 0, s, d_idx_a, d_cnt_a, d_idx_b, d_cnt_b, n_cells, k, d_shared);
    HIP_OK(hipGetLastError());
    dbg_sync(s, "neighbors shared");
    return 0;
} FASTF_CATCH_INT

// --mapping: the cells of a point looked up among the full-depth cells (mapping_kernels.hpp).  d_planes_point (planes_point planes) and
// d_planes_full (planes_full planes, at least as many: the point's counts are a subsample of the pair's): what fastf_dev_neighbor_planes
// filled for (n_cells, K) from the two row sets; d_norms_full: the norms fastf_dev_neighbors left for the full rows.  First the largest
// point norm (*max_norm_point_out) and the largest full norm are reduced and read back: fastf_neighbors_check_norm refuses either at 2^42
// and beyond and nothing more is launched.  Then d_self_dot[i] = e_ii (u64), and d_idx, d_cnt in the layout fastf_dev_neighbors writes —
// M(i), k from 1 to 64 — and d_self_rank[i] (u32; 0xFFFFFFFF where e_ii == 0).  The dot products come from the i8 MFMA, under
// FASTF_MAPPING_MFMA=0 from ordinary integer instructions: the same numbers.  Synchronises the stream once, before the two kernels.
extern "C" int fastf_dev_mapping(fastf_engine_t* e, const void* d_planes_point, uint32_t planes_point, const void* d_planes_full, uint32_t planes_full,
                                 uint32_t n_cells, uint32_t K, uint32_t k, const uint64_t* d_norms_full, uint32_t* d_idx, uint32_t* d_cnt,
                                 uint64_t* d_self_dot, uint32_t* d_self_rank, uint64_t* max_norm_point_out, void* stream) FASTF_TRY {
    DEV_ENTRY(!e, "null argument");
    hipStream_t s = (hipStream_t)stream;
    if (k < 1 || k > NBR_MAX_K) return set_err("fastf_dev_mapping: k = %u, from 1 to %u", k, NBR_MAX_K);
    if (planes_full < 1 || planes_full > NBR_MAX_PLANES) return set_err("fastf_dev_mapping: %u planes of the full rows, from 1 to %u", planes_full, NBR_MAX_PLANES);
    if (planes_point < 1 || planes_point > planes_full) return set_err("fastf_dev_mapping: %u planes of the point, from 1 to the %u of the full rows", planes_point, planes_full);
    if (K > NBR_MAX_GENES) return set_err("fastf_dev_mapping: %u genes, at most %u", K, NBR_MAX_GENES);
    if (max_norm_point_out) *max_norm_point_out = 0;
    if (!n_cells) return 0;
    if (!d_planes_point || !d_planes_full || !d_norms_full || !d_idx || !d_cnt || !d_self_dot || !d_self_rank) return set_err("fastf_dev_mapping: null argument");
    uint32_t n_pad = 0, K_pad = 0;
    fastf_neighbors_pad(n_cells, K, &n_pad, &K_pad);
    if (e->an.d_nbr.ensure(64)) return 1;
    u64* const d_max = (u64*)e->an.d_nbr.p + 2;                            // (words 2 and 3: the point's, the full rows')
    HIP_OK(hipMemsetAsync(d_max, 0, 2 * sizeof(u64), s));
    hipLaunchKernelGGL(nbr_norms_kernel, dim3(std::min<u32>((n_cells + 3) / 4, 8 * e->grid_cus)), dim3(256), 0, s, (const unsigned char*)d_planes_point, n_cells, n_pad, K_pad,
                       planes_point, (u64*)nullptr, d_max);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(map_max_kernel, dim3(std::min<u32>((n_cells + 255) / 256, 4 * e->grid_cus)), dim3(256), 0, s, (const u64*)d_norms_full, n_cells, d_max + 1);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(s));
    u64 max_norm[2] = {0, 0};
    if (copy_d2h(max_norm, d_max, sizeof max_norm)) return 1;
    if (max_norm_point_out) *max_norm_point_out = max_norm[0];
    if (fastf_neighbors_check_norm(max_norm[1]) || fastf_neighbors_check_norm(max_norm[0])) return 1;
    hipLaunchKernelGGL(map_diag_kernel, dim3(std::min<u32>((n_cells + 3) / 4, 8 * e->grid_cus)), dim3(256), 0, s, (const unsigned char*)d_planes_point, planes_point,
                       (const unsigned char*)d_planes_full, planes_full, n_cells, n_pad, K_pad, (u64*)d_self_dot);
    HIP_OK(hipGetLastError());
    const char* mf = getenv("FASTF_MAPPING_MFMA");
    const bool mfma = !(mf && mf[0] == '0');
    using gram_t = decltype(&map_gram_kernel<1, 1, false>);
    static constexpr gram_t gram[6][2] = {                                  // [pair (PQ, PF), PQ <= PF: PF (PF - 1) / 2 + PQ - 1][mfma]
        {map_gram_kernel<1, 1, false>, map_gram_kernel<1, 1, true>}, {map_gram_kernel<1, 2, false>, map_gram_kernel<1, 2, true>},
        {map_gram_kernel<2, 2, false>, map_gram_kernel<2, 2, true>}, {map_gram_kernel<1, 3, false>, map_gram_kernel<1, 3, true>},
        {map_gram_kernel<2, 3, false>, map_gram_kernel<2, 3, true>}, {map_gram_kernel<3, 3, false>, map_gram_kernel<3, 3, true>}};
    if (lds_attr_once(e->an.attr[AN_MAP_GRAM], (size_t)NBR_WAVES * nbr_wave_words(NBR_MAX_K) * sizeof(u64), gram[0], 12)) return 1;
    hipLaunchKernelGGL(gram[planes_full * (planes_full - 1) / 2 + planes_point - 1][mfma], dim3((n_cells + NBR_ROWS - 1) / NBR_ROWS), dim3(NBR_THREADS),
                       (size_t)NBR_WAVES * nbr_wave_words(k) * sizeof(u64), s, (const unsigned char*)d_planes_point, (const unsigned char*)d_planes_full, n_cells, n_pad, K_pad, k,
                       (const u64*)d_norms_full, (const u64*)d_self_dot, d_idx, d_cnt, d_self_rank);
    HIP_OK(hipGetLastError());
    dbg_sync(s, "mapping");
    return 0;
} FASTF_CATCH_INT

static_assert(COEX_MAX_K == FASTF_COEXPR_MAX_K && COEX_MAX_PLANES == FASTF_COEXPR_MAX_PLANES && COEX_MAX_GENES == FASTF_COEXPR_MAX_GENES && COEX_CHUNK == FASTF_COEXPR_CHUNK,
              "the limits of the co-expression kernels and the ABI's");

// --coexpression: the chunk of cells in effect — FASTF_COEXPR_CHUNK=<cells> lowers the default: 32 .. default - 1 is rounded down to a
// multiple of 32, every other value is ignored (read at each call, it changes no result) — and with it the padded shape of the gene-major planes (coex_pad)
static u32 coex_chunk_knob() {
    const char* ck = getenv("FASTF_COEXPR_CHUNK");
    const long v = ck ? atol(ck) : 0;
    return v >= 32 && v < (long)COEX_CHUNK ? (u32)v & ~31u : COEX_CHUNK;
}
extern "C" void fastf_coexpr_pad(uint32_t n_cells, uint32_t K, uint32_t* K_pad, uint32_t* n_pad, uint32_t* chunk) FASTF_TRY {
    u32 kp = 0, np = 0, ce = 0;
    coex_pad(n_cells, K, coex_chunk_knob(), &kp, &np, &ce);
    if (K_pad) *K_pad = kp;
    if (n_pad) *n_pad = np;
    if (chunk) *chunk = ce;
} FASTF_CATCH_(return)
extern "C" size_t fastf_coexpr_work_bytes(uint32_t n_cells, uint32_t K, uint32_t planes) FASTF_TRY {
    u32 kp = 0, np = 0, ce = 0;
    coex_pad(n_cells, K, coex_chunk_knob(), &kp, &np, &ce);
    return (size_t)planes * kp * np;
} FASTF_CATCH_(return 0)

// --coexpression: the sums of one row set (coexpr_kernels.hpp).  The rows and d_slot_map as fastf_dev_neighbor_planes takes them, `planes`
// what that call returned for them.  d_work: fastf_coexpr_work_bytes(n_cells, K, planes) bytes, 16-byte aligned — the gene-major planes,
// zeroed and filled here.  d_D: u64[K * K], D_gh = sum_i m_ig m_ih, dense, row-major; d_S: u64[K]; both zeroed here.  fastf_coexpr_check_gram
// refuses (n_cells, planes) whose D would leave 64 bits before anything is launched.  The dot products come from the i8 MFMA, under
// FASTF_COEXPR_MFMA=0 from ordinary integer instructions: the same numbers.  Stream-ordered.
extern "C" int fastf_dev_coexpr_sums(fastf_engine_t* e, const uint32_t* d_feature, const uint32_t* d_cell, const uint32_t* d_count, const uint64_t* d_nnz,
                                     const uint16_t* d_slot_map, uint32_t n_features, uint32_t n_cells, uint32_t K, uint32_t planes, void* d_work,
                                     size_t work_bytes, uint64_t* d_D, uint64_t* d_S, void* stream) FASTF_TRY {
    DEV_ENTRY(!e || !d_nnz, "null argument");
    hipStream_t s = (hipStream_t)stream;
    if (K > COEX_MAX_GENES) return set_err("fastf_dev_coexpr_sums: %u genes, at most %u", K, COEX_MAX_GENES);
    if (n_cells > 0xFFFE0000u) return set_err("fastf_dev_coexpr_sums: %u cells: the padded row of a gene does not fit 32 bits", n_cells);
    if (fastf_coexpr_check_gram(n_cells, planes)) return 1;
    if (!K) return 0;
    if (!d_D || !d_S) return set_err("fastf_dev_coexpr_sums: null argument");
    u32 K_pad = 0, n_pad = 0, chunk = 0;
    coex_pad(n_cells, K, coex_chunk_knob(), &K_pad, &n_pad, &chunk);
    const size_t need = (size_t)planes * K_pad * n_pad;
    if (need > work_bytes) return set_err("fastf_dev_coexpr_sums: %u planes of %u x %u bytes need %zu bytes, the buffer has %zu", planes, K_pad, n_pad, need, work_bytes);
    if (!d_work || ((uintptr_t)d_work & 15)) return set_err("fastf_dev_coexpr_sums: the work buffer is 16-byte aligned");
    HIP_OK(hipMemsetAsync(d_D, 0, (size_t)K * K * sizeof(u64), s));
    HIP_OK(hipMemsetAsync(d_S, 0, (size_t)K * sizeof(u64), s));
    if (!n_cells || !d_feature || !d_cell || !d_count || !d_slot_map) return 0;      // (no row buffer: sums of nothing)
    HIP_OK(hipMemsetAsync(d_work, 0, need, s));
    hipLaunchKernelGGL(coex_planes_kernel, dim3(4 * e->grid_cus), dim3(256), 0, s, d_feature, d_cell, d_count, (const u64*)d_nnz, d_slot_map, n_features,
                       n_cells, K, K_pad, n_pad, planes, (unsigned char*)d_work);
    HIP_OK(hipGetLastError());
    const char* mf = getenv("FASTF_COEXPR_MFMA");
    const bool mfma = !(mf && mf[0] == '0');
    static constexpr decltype(&coex_gram_kernel<1, false>) gram[COEX_MAX_PLANES][2] = {   // [planes - 1][mfma]
        {coex_gram_kernel<1, false>, coex_gram_kernel<1, true>}, {coex_gram_kernel<2, false>, coex_gram_kernel<2, true>}, {coex_gram_kernel<3, false>, coex_gram_kernel<3, true>}};
    const u32 n32 = (n_cells + 31u) & ~31u, n_tiles = K_pad / COEX_TILE, n_chunks = n_pad / chunk;
    const u64 n_pairs = (u64)n_tiles * (n_tiles + 1) / 2, n_items = n_pairs * n_chunks, groups = (n_items + COEX_WAVES - 1) / COEX_WAVES;
    if (groups > 0x7FFFFFFFull) return set_err("fastf_dev_coexpr_sums: %llu tiles of %u cells are more than one launch takes", (unsigned long long)n_items, chunk);
    hipLaunchKernelGGL(gram[planes - 1][mfma], dim3((u32)groups), dim3(COEX_THREADS), 0, s, (const unsigned char*)d_work, K, K_pad, n_pad, n32, chunk, n_tiles,
                       n_pairs, n_items, (u64*)d_D);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(coex_sums_kernel, dim3(std::min<u32>((K + 3) / 4, 8 * e->grid_cus)), dim3(256), 0, s, (const unsigned char*)d_work, K, K_pad, n_pad, n32, planes,
                       (u64*)d_S);
    HIP_OK(hipGetLastError());
    dbg_sync(s, "coexpr sums");
    return 0;
} FASTF_CATCH_INT

// --coexpression: the partner sets of D and S over n_cells cells (coex_var_kernel, coex_select_kernel).  V_h = n D_hh - S_h^2 goes into the
// engine's own buffer; the largest D_hh is read back and fastf_coexpr_check_range refuses n_cells * max Q >= 2^63 before the selection is
// launched.  Then d_idx[g * k + s], s < d_cnt[g], are the partners of gene g (slots, ascending; the other slots 0xFFFFFFFF), k from 1 to
// 64, K at most 4096.  Synchronises the stream once, before the selection.  Not re-entrant per engine: V and the maximum share one engine buffer.
extern "C" int fastf_dev_coexpr_select(fastf_engine_t* e, const uint64_t* d_D, const uint64_t* d_S, uint32_t n_cells, uint32_t K, uint32_t k,
                                       uint32_t* d_idx, uint32_t* d_cnt, void* stream) FASTF_TRY {
    DEV_ENTRY(!e, "null argument");
    hipStream_t s = (hipStream_t)stream;
    if (k < 1 || k > COEX_MAX_K) return set_err("fastf_dev_coexpr_select: k = %u, from 1 to %u", k, COEX_MAX_K);
    if (K > COEX_MAX_GENES) return set_err("fastf_dev_coexpr_select: %u genes, at most %u", K, COEX_MAX_GENES);
    if (!K) return 0;
    if (!d_D || !d_S || !d_idx || !d_cnt) return set_err("fastf_dev_coexpr_select: null argument");
    if (e->an.d_coex.ensure(64 + (size_t)COEX_MAX_GENES * sizeof(u64))) return 1;
    u64* const d_max = (u64*)e->an.d_coex.p;
    u64* const d_V = d_max + 8;
    HIP_OK(hipMemsetAsync(d_max, 0, 64, s));
    hipLaunchKernelGGL(coex_var_kernel, dim3((K + 255) / 256), dim3(256), 0, s, (const u64*)d_D, (const u64*)d_S, n_cells, K, d_V, d_max);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(s));
    u64 max_q = 0;
    if (copy_d2h(&max_q, d_max, sizeof max_q)) return 1;
    if (fastf_coexpr_check_range(n_cells, max_q)) return 1;
    hipLaunchKernelGGL(coex_select_kernel, dim3((K + COEX_SEL_THREADS - 1) / COEX_SEL_THREADS), dim3(COEX_SEL_THREADS), (size_t)coex_select_lds(k), s,
                       (const u64*)d_D, (const u64*)d_S, (const u64*)d_V, n_cells, K, k, d_idx, d_cnt);
    HIP_OK(hipGetLastError());
    dbg_sync(s, "coexpr select");
    return 0;
} FASTF_CATCH_INT

// --labels: the label votes of the neighbour sets (label_votes_kernel).  d_idx, d_cnt: what fastf_dev_neighbors wrote for (n_cells, k);
// d_lab: u8[n_cells], 0 unlabelled, 1 .. n_labels.  d_pred, d_same, d_labelled: u8[n_cells]; d_conf: u32[n_labels * (n_labels + 1)],
// zeroed here.  The counts of a workgroup are added up in LDS where they fit it (201 labels and fewer); FASTF_LABELS_LDS=0 takes the
// general form, global atomics alone, for every n_labels (tests, A/B runs).  Stream-ordered.
extern "C" int fastf_dev_label_votes(fastf_engine_t* e, const uint32_t* d_idx, const uint32_t* d_cnt, const uint8_t* d_lab, uint32_t n_cells, uint32_t k,
                                     uint32_t n_labels, uint8_t* d_pred, uint8_t* d_same, uint8_t* d_labelled, uint32_t* d_conf, void* stream) FASTF_TRY {
    DEV_ENTRY(!e, "null argument");
    hipStream_t s = (hipStream_t)stream;
    if (k < 1 || k > LAB_MAX_K) return set_err("fastf_dev_label_votes: k = %u, from 1 to %u", k, LAB_MAX_K);
    if (n_labels > LAB_MAX_LABELS) return set_err("fastf_dev_label_votes: %u labels, at most %u", n_labels, LAB_MAX_LABELS);
    if (n_labels && !d_conf) return set_err("fastf_dev_label_votes: null argument");
    if (n_labels) HIP_OK(hipMemsetAsync(d_conf, 0, (size_t)lab_conf_words(n_labels) * sizeof(u32), s));
    if (!n_cells) return 0;
    if (!d_idx || !d_cnt || !d_lab || !d_pred || !d_same || !d_labelled) return set_err("fastf_dev_label_votes: null argument");
    const char* lf = getenv("FASTF_LABELS_LDS");
    const bool lds_form = lab_conf_fits_lds(n_labels) && !(lf && lf[0] == '0');
    static constexpr decltype(&label_votes_kernel<16, true>) votes[2][3] = {            // [lds form][G = 16, 32, 64: k <= 16, <= 32, beyond]
        {label_votes_kernel<16, false>, label_votes_kernel<32, false>, label_votes_kernel<64, false>},
        {label_votes_kernel<16, true>, label_votes_kernel<32, true>, label_votes_kernel<64, true>}};
    if (lds_form && lds_attr_once(e->an.attr[AN_LABEL_VOTES], LAB_LDS_BYTES, votes[1], 3)) return 1;
    const u32 g = k <= 16 ? 0 : k <= 32 ? 1 : 2;
    const u32 per_pass = LAB_THREADS / (16u << g), blocks_all = (n_cells + per_pass - 1) / per_pass;
    // LDS form: one workgroup a CU at the most: each zeroes and flushes its own copy of the counts
    hipLaunchKernelGGL(votes[lds_form][g], dim3(std::min<u32>(blocks_all, (lds_form ? 1u : 8u) * (u32)e->grid_cus)), dim3(LAB_THREADS),
                       lds_form ? (size_t)lab_conf_words(n_labels) * sizeof(u32) : 0, s, d_idx, d_cnt, d_lab, n_cells, k, n_labels, d_pred, d_same, d_labelled, d_conf);
    HIP_OK(hipGetLastError());
    dbg_sync(s, "label votes");
    return 0;
} FASTF_CATCH_INT

// --pseudotime: per cell the lower median of the ranks its neighbours carry (pt_median_kernel).  d_idx, d_cnt: what fastf_dev_neighbors or
// fastf_dev_mapping wrote for (n_cells, k); d_t: u32[n_cells], 0 without a value.  d_est, d_valued: u32[n_cells].  Stream-ordered.
extern "C" int fastf_dev_ptime_medians(fastf_engine_t* e, const uint32_t* d_idx, const uint32_t* d_cnt, const uint32_t* d_t, uint32_t n_cells, uint32_t k,
                                       uint32_t* d_est, uint32_t* d_valued, void* stream) FASTF_TRY {
    DEV_ENTRY(!e, "null argument");
    hipStream_t s = (hipStream_t)stream;
    if (k < 1 || k > PT_MAX_K) return set_err("fastf_dev_ptime_medians: k = %u, from 1 to %u", k, PT_MAX_K);
    if (!n_cells) return 0;
    if (!d_idx || !d_cnt || !d_t || !d_est || !d_valued) return set_err("fastf_dev_ptime_medians: null argument");
    static constexpr decltype(&pt_median_kernel<16>) medians[3] = {pt_median_kernel<16>, pt_median_kernel<32>, pt_median_kernel<64>};   // k <= 16, <= 32, beyond
    const u32 g = k <= 16 ? 0 : k <= 32 ? 1 : 2;
    const u32 per_pass = PT_THREADS / (16u << g), blocks_all = (n_cells + per_pass - 1) / per_pass;
    hipLaunchKernelGGL(medians[g], dim3(std::min<u32>(blocks_all, 8u * (u32)e->grid_cus)), dim3(PT_THREADS), 0, s, d_idx, d_cnt, d_t, n_cells, k, d_est, d_valued);
    HIP_OK(hipGetLastError());
    dbg_sync(s, "ptime medians");
    return 0;
} FASTF_CATCH_INT

static_assert(PT_TILE == FASTF_PTIME_TILE && PT_OUT_WORDS == FASTF_PTIME_OUT_WORDS && PT_MAX_CELLS == FASTF_PTIME_MAX_CELLS, "the tile and the result block of pt_pairs_kernel and the ABI's");

// --pseudotime: the order census of d_est against d_t over the cells that have both (pt_pairs_kernel): one workgroup per pair of tiles.
// d_out: FASTF_PTIME_OUT_WORDS u64 (conc disc tie_e tie_t tie_both cells shift_sum), zeroed here.  Stream-ordered.
extern "C" int fastf_dev_ptime_census(fastf_engine_t* e, const uint32_t* d_est, const uint32_t* d_t, uint32_t n_cells, uint64_t* d_out, void* stream) FASTF_TRY {
    DEV_ENTRY(!e || !d_out, "null argument");
    hipStream_t s = (hipStream_t)stream;
    if (n_cells > PT_MAX_CELLS) return set_err("fastf_dev_ptime_census: %u cells, at most %u", n_cells, PT_MAX_CELLS);
    HIP_OK(hipMemsetAsync(d_out, 0, PT_OUT_WORDS * sizeof(u64), s));
    if (!n_cells) return 0;
    if (!d_est || !d_t) return set_err("fastf_dev_ptime_census: null argument");
    const u64 tiles = ((u64)n_cells + PT_TILE - 1) / PT_TILE;
    hipLaunchKernelGGL(pt_pairs_kernel, dim3((u32)(tiles * (tiles + 1) / 2)), dim3(PT_THREADS), 0, s, d_est, d_t, n_cells, (u64*)d_out);
    HIP_OK(hipGetLastError());
    dbg_sync(s, "ptime census");
    return 0;
} FASTF_CATCH_INT

static_assert(MK_MAX_LABELS == FASTF_LABELS_MAX && MK_MAX_PLANES == FASTF_MARKER_MAX_PLANES, "the limits of marker_auc_kernel and the ABI's");

// --markers: the accumulator form one call takes for (planes, n_labels): 1 — in LDS beside the bins, 0 — global atomics (what does not
// fit, and everything under FASTF_MARKERS_LDS=0), -1 — the call is refused
extern "C" int fastf_marker_auc_form(uint32_t planes, uint32_t n_labels) FASTF_TRY {
    if (planes < 1 || planes > MK_MAX_PLANES || n_labels < 1 || n_labels > MK_MAX_LABELS) return -1;
    const char* lf = getenv("FASTF_MARKERS_LDS");
    return mk_fits_lds(planes, n_labels) && !(lf && lf[0] == '0') ? 1 : 0;
} FASTF_CATCH_(return -1)

// --markers: per (label, slot of A) 2U, det and sum (marker_auc_kernel) and the cells per label.  d_planes: what fastf_dev_neighbor_planes
// filled for (n_cells, K) with `planes` planes; d_lab: u8[n_cells].  d_s2u, d_sum: u64[n_labels * K]; d_det: u32[n_labels * K];
// d_n_per_label: u32[n_labels]; the four are cleared here.  Three planes (a count of 2^14 and beyond in A) and n_labels outside
// 1 .. FASTF_LABELS_MAX are refused before anything is launched.  FASTF_MARKERS_LDS=0 takes the global-atomic form for every n_labels.
// Stream-ordered.
extern "C" int fastf_dev_marker_auc(fastf_engine_t* e, const void* d_planes, uint32_t planes, uint32_t n_cells, uint32_t K, const uint8_t* d_lab,
                                    uint32_t n_labels, uint64_t* d_s2u, uint32_t* d_det, uint64_t* d_sum, uint32_t* d_n_per_label, void* stream) FASTF_TRY {
    DEV_ENTRY(!e, "null argument");
    hipStream_t s = (hipStream_t)stream;
    if (planes < 1 || planes > MK_MAX_PLANES)
        return set_err("fastf_dev_marker_auc: FASTF_ERR_MARKER_COUNT: %u planes — a count of 2^14 or more among the highly variable genes: the rank table of a gene does not fit the LDS", planes);
    if (n_labels < 1 || n_labels > MK_MAX_LABELS) return set_err("fastf_dev_marker_auc: %u labels, from 1 to %u", n_labels, MK_MAX_LABELS);
    if (K > NBR_MAX_GENES) return set_err("fastf_dev_marker_auc: %u genes, at most %u", K, NBR_MAX_GENES);
    if (!d_n_per_label || (K && (!d_s2u || !d_det || !d_sum))) return set_err("fastf_dev_marker_auc: null argument");
    const size_t words = (size_t)n_labels * K;
    HIP_OK(hipMemsetAsync(d_n_per_label, 0, (size_t)n_labels * sizeof(u32), s));
    if (words) {
        HIP_OK(hipMemsetAsync(d_s2u, 0, words * sizeof(u64), s));
        HIP_OK(hipMemsetAsync(d_det, 0, words * sizeof(u32), s));
        HIP_OK(hipMemsetAsync(d_sum, 0, words * sizeof(u64), s));
    }
    if (!n_cells) return 0;
    if (!d_lab || (K && !d_planes)) return set_err("fastf_dev_marker_auc: null argument");
    hipLaunchKernelGGL(marker_labels_kernel, dim3(std::min<u32>((n_cells + 255u) / 256u, (u32)e->grid_cus)), dim3(256), 0, s, (const unsigned char*)d_lab, n_cells, n_labels, d_n_per_label);
    HIP_OK(hipGetLastError());
    if (!K) return 0;
    const bool lds_form = fastf_marker_auc_form(planes, n_labels) == 1;
    static constexpr decltype(&marker_auc_kernel<1, true>) auc[MK_MAX_PLANES][2] = {    // [planes - 1][lds form]
        {marker_auc_kernel<1, false>, marker_auc_kernel<1, true>}, {marker_auc_kernel<2, false>, marker_auc_kernel<2, true>}};
    if (lds_attr_once(e->an.attr[AN_MARKER_AUC], MK_LDS_BYTES, auc[0], 2 * MK_MAX_PLANES)) return 1;
    uint32_t n_pad = 0, K_pad = 0;
    fastf_neighbors_pad(n_cells, K, &n_pad, &K_pad);
    hipLaunchKernelGGL(auc[planes - 1][lds_form], dim3((K + mk_tile(planes) - 1) / mk_tile(planes)), dim3(MK_THREADS), (size_t)mk_lds_bytes(planes, n_labels, lds_form), s,
                       (const unsigned char*)d_planes, d_lab, d_n_per_label, n_cells, n_pad, K, K_pad, n_labels, (u64*)d_s2u, d_det, (u64*)d_sum);
    HIP_OK(hipGetLastError());
    dbg_sync(s, "marker auc");
    return 0;
} FASTF_CATCH_INT

// Replicate runs: d_cells_per_gene (what fastf_dev_gene_summary left, still on the device) added into the three u64[n_features]
// accumulators of a grid point (gene_reps_kernel).  Nothing is cleared here: the caller zeroes the accumulators before the first seed.
extern "C" int fastf_dev_gene_reps_add(fastf_engine_t* e, const uint32_t* d_cells_per_gene, uint32_t n_features, uint64_t* d_detected,
                                       uint64_t* d_sum, uint64_t* d_sumsq, void* stream) FASTF_TRY {
    DEV_ENTRY(!e || (n_features && (!d_cells_per_gene || !d_detected || !d_sum || !d_sumsq)), "null argument");
    if (!n_features) return 0;
    const u32 grid = std::min<u32>((n_features + GENE_REPS_THREADS - 1) / GENE_REPS_THREADS, 4u * (u32)e->grid_cus);
    hipLaunchKernelGGL(gene_reps_kernel, dim3(grid), dim3(GENE_REPS_THREADS), 0, (hipStream_t)stream, d_cells_per_gene, n_features,
                       (u64*)d_detected, (u64*)d_sum, (u64*)d_sumsq);
    HIP_OK(hipGetLastError());
    dbg_sync((hipStream_t)stream, "gene reps add");
    return 0;
} FASTF_CATCH_INT

// --cells: the -u rows of fastf_dev_umi_rows on this engine reduced along the cell axis and into the copy-number histogram
// (copy_summary_kernel).  The cell field and the non-NULL flag are read from the engine's own key layout.  All four outputs are
// cleared here first; *d_nrows rows are read.  Every per-cell number is below 2^32 (a number of records).
static_assert(COPY_BINS == FASTF_COPY_BINS, "the histogram of copy_summary_kernel and the ABI's");
extern "C" int fastf_dev_copy_summary(fastf_engine_t* e, const uint64_t* d_ukeys, const uint32_t* d_ncopy, const uint64_t* d_nrows, uint32_t n_cells,
                                      uint32_t* d_reads_per_cell, uint32_t* d_null_reads_per_cell, uint32_t* d_single_per_cell, uint64_t* d_hist,
                                      void* stream) FASTF_TRY {
    DEV_ENTRY(!e || !d_ukeys || !d_ncopy || !d_nrows || !d_reads_per_cell || !d_null_reads_per_cell || !d_single_per_cell || !d_hist, "null argument");
    NO_WIDE(e, "fastf_dev_copy_summary");
    hipStream_t s = (hipStream_t)stream;
    if (n_cells) {
        HIP_OK(hipMemsetAsync(d_reads_per_cell, 0, (size_t)n_cells * sizeof(u32), s));
        HIP_OK(hipMemsetAsync(d_null_reads_per_cell, 0, (size_t)n_cells * sizeof(u32), s));
        HIP_OK(hipMemsetAsync(d_single_per_cell, 0, (size_t)n_cells * sizeof(u32), s));
    }
    HIP_OK(hipMemsetAsync(d_hist, 0, ((size_t)COPY_BINS + 1) * sizeof(u64), s));
    const CopyOut out{d_reads_per_cell, d_null_reads_per_cell, d_single_per_cell};
    hipLaunchKernelGGL(copy_summary_kernel, dim3(2 * e->grid_cus), dim3(256), 0, s, (const u64*)d_ukeys, d_ncopy, (const u64*)d_nrows, n_cells,
                       e->L.cell_shift, e->L.umi_bits + e->L.len_bits, out, (u64*)d_hist);
    HIP_OK(hipGetLastError());
    dbg_sync(s, "copy summary");
    return 0;
} FASTF_CATCH_INT

// cap: hits per cell from the cell scratch K1a left (cell_hits_kernel).  Valid right after fastf_dev_count_hits[_blocked] over the
// same n records on the same stream (the FASTF_PROBE_REUSE_HITS contract); d_blocked: the blocked buffer of that call, or
// nullptr for the SoA scratch.  d_hits_per_cell[c - 1] (u32, n_cells entries) is cleared here first.
static CellIn cell_scratch_of(const fastf_engine* e, const void* blk) {
    return blk ? CellIn{blk, blk_run_bytes(e->cell16, e->narrow), blk_cell_off(e->narrow)} : CellIn{e->d_cellidx.p, 0u, 0u};
}
extern "C" int fastf_dev_cell_hits(fastf_engine_t* e, uint64_t n, const void* d_blocked, uint32_t* d_hits_per_cell, void* stream) FASTF_TRY {
    DEV_SINGLE(!e || (e && e->n_cells && !d_hits_per_cell), "null argument");
    if (n >= (1ull << 32)) return set_err("fastf_dev_cell_hits: %llu records: the counters are 32 bits wide", (unsigned long long)n);
    HIP_OK(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    if (!e->n_cells) return 0;
    HIP_OK(hipMemsetAsync(d_hits_per_cell, 0, (size_t)e->n_cells * sizeof(u32), s));
    if (n == 0) return 0;
    if (!d_blocked && e->d_cellidx.bytes < n * (e->cell16 ? 2u : 4u)) return set_err("fastf_dev_cell_hits: no cell scratch for %llu records: fastf_dev_count_hits comes first", (unsigned long long)n);
    const u64 units = (n + BLK_RECS - 1) / BLK_RECS;
    constexpr u32 WAVES = CAP_HITS_THREADS / WAVE;
    return launch_ranged(e, s, "cell hits", cell_hits_kernel<true>, cell_hits_kernel<false>, AN_CAP_HITS,
                         {e->n_cells, CAP_LDS_CELLS, CAP_LDS_RANGES, "FASTF_CAP_LDS_RANGES", sizeof(u32)}, CAP_HITS_THREADS, (units + WAVES - 1) / WAVES,
                         cell_scratch_of(e, d_blocked), e->cell16, n, e->n_cells, d_hits_per_cell);
} FASTF_CATCH_INT

// cap: the decision plane of per-cell thresholds.  The stream init_genrand(seed) + skip is generated as fastf_dev_mt_decisions
// generates it, the raw draws staying in the engine's word buffer; cell_decisions_kernel then sets bit i of d_bits_out =
// draw i < d_thresholds[cell of the i-th CB hit - 1] (u64[n_cells] in device memory, each 0 .. 2^32: the caller's word, the values
// are not read on the host).  The draws of the last (seed, skip) stay in the word buffer: a second call over the same stream — the
// next cap of a cell rate — does not generate them again.  Same layout and size rule as
// fastf_dev_draw_bits.  Valid where fastf_dev_cell_hits is, and leaves that contract intact: a fastf_dev_probe_pack with
// FASTF_PROBE_REUSE_HITS | FASTF_PROBE_DRAW_BITS may follow.  Synchronises the stream.
extern "C" int fastf_dev_cell_decisions(fastf_engine_t* e, uint64_t n, const void* d_blocked, uint32_t seed, uint64_t skip, uint64_t n_draws,
                                        const uint64_t* d_thresholds, uint32_t* d_bits_out, void* stream) FASTF_TRY {
    DEV_SINGLE(!e || (n_draws && (!d_bits_out || !d_thresholds)), "null argument");
    if ((uintptr_t)d_bits_out & 7) return set_err("fastf_dev_cell_decisions: the plane is 8-byte aligned");
    HIP_OK(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    auto sync = [&]() -> int {
        if (hipStreamSynchronize(s) != hipSuccess) return set_err("the generator or decision kernels failed: %s", hipGetErrorString(hipGetLastError()));
        return 0;
    };
    if (!n_draws) return sync();
    HIP_OK(hipMemsetAsync(d_bits_out, 0, (size_t)((n_draws + 63) / 64) * 8, s));
    if (n == 0 || !e->n_cells) return sync();
    if (!d_blocked && e->d_cellidx.bytes < n * (e->cell16 ? 2u : 4u)) return set_err("fastf_dev_cell_decisions: no cell scratch for %llu records: fastf_dev_count_hits comes first", (unsigned long long)n);
    const u64 tiles = (n + K1_TILE - 1) / K1_TILE;
    if (e->d_tilebase.bytes < tiles * sizeof(u64) || e->d_halfhits.bytes < tiles * 16 * sizeof(u32)) return set_err("fastf_dev_cell_decisions: no hit counts for %llu records: fastf_dev_count_hits comes first", (unsigned long long)n);
    // the raw draws: generated once per (seed, skip) — the caps of one cell rate share the stream — and kept while no other
    // generator launch has used the word buffer
    if (!(e->mtwords_kept && e->mtwords_seed == seed && e->mtwords_skip == skip && e->mtwords_n >= n_draws)) {
        fastf_mt_t mt; fastf_mt_seed(&mt, seed); fastf_mt_skip(&mt, skip);
        if (e->d_mtseat.ensure(sizeof mt)) return 1;
        if (copy_h2d_on(e->d_mtseat.p, &mt, sizeof mt, s)) return 1;
        u32 idx = (u32)mt.idx;
        if (launch_mt_decisions_par(e, s, (u32*)e->d_mtseat.p, &idx, e->d_mtwords, nullptr, 0, n_draws, ~0ull, 0, nullptr, true)) return 1;
        e->mtwords_kept = true; e->mtwords_seed = seed; e->mtwords_skip = skip; e->mtwords_n = n_draws;
    }
    const u64 units = (n + BLK_RECS - 1) / BLK_RECS;
    const u32 grid = (u32)std::min<u64>((units + 3) / 4, 8ull * e->grid_cus);
    hipLaunchKernelGGL(cell_decisions_kernel, dim3(grid), dim3(256), 0, s, cell_scratch_of(e, d_blocked), e->cell16, n, (const u64*)e->d_tilebase.p,
                       (const u32*)e->d_halfhits.p, (const u32*)e->d_mtwords.p, n_draws, (const u64*)d_thresholds, e->n_cells, (u64*)d_bits_out);
    HIP_OK(hipGetLastError());
    return sync();
} FASTF_CATCH_INT

// level: one step of the per-cell threshold search (level_step_kernel; the state rules are in include/fastf_amd.h).  d_out[0]
// (and d_out[1] in the initialising form) are cleared here first; the engine's own error word is always one of the two the
// kernel looks at, d_err_in (nullptr: none) the other.  Stream-ordered, no synchronisation.
static_assert(LEVEL_OUT_WORDS == FASTF_LEVEL_OUT_WORDS, "the result block of level_step_kernel and the ABI's");
template <bool INIT>
static int launch_level_step(fastf_engine* e, const u64* d_umis, u32 n_cells, u64 umi_cap, u64* d_lo, u64* d_hi, u64* d_probe, u64* d_out,
                             const u64* d_err_in, hipStream_t s) {
    if (umi_cap < 1) return set_err("level: a UMI cap is at least 1");
    HIP_OK(hipMemsetAsync(d_out, 0, (INIT ? 2 : 1) * sizeof(u64), s));
    const u32 grid = std::max<u32>(1u, (n_cells + LEVEL_THREADS - 1) / LEVEL_THREADS);
    hipLaunchKernelGGL(level_step_kernel<INIT>, dim3(grid), dim3(LEVEL_THREADS), 0, s, d_umis, n_cells, umi_cap, d_lo, d_hi, d_probe, d_out,
                       err_word(e), d_err_in);
    HIP_OK(hipGetLastError());
    dbg_sync(s, INIT ? "level init" : "level step");
    return 0;
}
extern "C" int fastf_dev_level_init(fastf_engine_t* e, const uint64_t* d_umis_full, uint32_t n_cells, uint64_t umi_cap, uint64_t* d_lo, uint64_t* d_hi,
                                    uint64_t* d_probe, uint64_t* d_out, const uint64_t* d_err_in, void* stream) FASTF_TRY {
    DEV_ENTRY(!e || !d_out || (n_cells && (!d_umis_full || !d_lo || !d_hi || !d_probe)), "null argument");
    return launch_level_step<true>(e, (const u64*)d_umis_full, n_cells, umi_cap, (u64*)d_lo, (u64*)d_hi, (u64*)d_probe, (u64*)d_out, (const u64*)d_err_in, (hipStream_t)stream);
} FASTF_CATCH_INT
extern "C" int fastf_dev_level_step(fastf_engine_t* e, const uint64_t* d_umis_per_cell, uint32_t n_cells, uint64_t umi_cap, uint64_t* d_lo, uint64_t* d_hi,
                                    uint64_t* d_probe, uint64_t* d_out, const uint64_t* d_err_in, void* stream) FASTF_TRY {
    DEV_ENTRY(!e || !d_out || (n_cells && (!d_umis_per_cell || !d_lo || !d_hi || !d_probe)), "null argument");
    return launch_level_step<false>(e, (const u64*)d_umis_per_cell, n_cells, umi_cap, (u64*)d_lo, (u64*)d_hi, (u64*)d_probe, (u64*)d_out, (const u64*)d_err_in, (hipStream_t)stream);
} FASTF_CATCH_INT
