// gene_kernels.hpp — the kernel behind `--genes` of `fastF sweep` and `fastF cap` (resident.c): the COO rows of a point reduced
// along the gene axis, the counterpart of cell_summary_kernel (sweep_kernels.hpp).
//
//   gene_summary_kernel   rows (feature, count) in any order -> cells_per_gene[g - 1] = rows of gene g with count >= 1 (the rule of
//                         genes_per_cell), umis_per_gene[g - 1] = the sum of their counts
//   gene_reps_kernel      replicate runs (--seeds, --reps): the cells_per_gene of one (grid point, seed) added into the three u64
//                         accumulators of its grid point
#pragma once
#include "ranged_hist.hpp"

namespace fastf {

// The rows arrive ascending by (cell, feature): the rows of one gene are scattered over the whole array, and the 64 rows of a wave
// are — inside a cell — 64 different genes.  A ranged histogram (ranged_hist.hpp) with two numbers per bin in one 64-bit counter:
//
//   LDS = true    one ds_add_u64 of (1 << 32 | count) per row keeps the rows in the high half and the sum of the counts in the low
//                 half.  Exact as long as the low half cannot carry — the ABI's precondition: the sum of ALL counts is below 2^32
//                 (it is a number of records, and the device-level calls stop at 2^32 - 2 records).  Flushed with one global
//                 atomic per non-zero half of a counter (the two halves go to two arrays).
//   LDS = false   global atomics, two per row (one per array).
// A row with count 0 adds nothing to either number and issues no atomic.  Two or three equal genes among 64 rows (a cell boundary
// inside the item) are left to the atomic unit: aggregating them would cost every item a loop over its distinct genes.
// A feature outside 1 .. n_features writes nothing (as cell_emit).
constexpr u32 GENE_LDS_GENES = 16384, GENE_THREADS = 1024, GENE_LDS_RANGES = 8, GENE_ITEMS = 4;

template <bool LDS>
__device__ __forceinline__ void gene_add(u32 idx, u32 k, u32 n_genes, u64* __restrict__ s_cnt, u32* __restrict__ cells, u64* __restrict__ umis, int lane) {
    const bool hit = idx < n_genes && k != 0u;
    const WaveHits h = wave_hits<true>(hit, idx);
    if (!h.mask) return;                                                   // (uniform)
    u64 v = hit ? ((1ull << 32) | (u64)k) : 0ull;
    if (h.one_bin) v = wave_sum64(v);                                       // (the low half cannot carry: precondition)
    if (h.one_bin ? lane == h.leader : hit) {
        if constexpr (LDS) (void)__hip_atomic_fetch_add(s_cnt + idx, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else { atomicAdd(cells + idx, (u32)(v >> 32)); atomicAdd(umis + idx, v & 0xFFFFFFFFull); }
    }
}

// A wave takes GENE_ITEMS neighbouring items of 64 rows per turn.
struct GeneSummaryHist {
    typedef u64 word;
    static constexpr u32 WORDS = 1, BINS = GENE_LDS_GENES, THREADS = GENE_THREADS;
    static constexpr u64 TURN = (u64)GENE_ITEMS * WAVE;
    const u32* __restrict__ feature; const u32* __restrict__ count; u64 n; u32* __restrict__ cells; u64* __restrict__ umis;
    __device__ __forceinline__ void shift(u32 lo) { cells += lo; umis += lo; }
    template <bool LDS>
    __device__ __forceinline__ void turn(u64 base, u32 lo, u32 n_genes, u64* __restrict__ s_cnt, int lane) const {
        u32 f[GENE_ITEMS], k[GENE_ITEMS];
#pragma unroll
        for (u32 j = 0; j < GENE_ITEMS; ++j) {
            const u64 i = base + j * WAVE + (u64)lane;
            const bool valid = i < n;
            f[j] = valid ? ld_once<FASTF_NT_K3 != 0>(feature + i) : 0u;
            k[j] = valid ? ld_once<FASTF_NT_K3 != 0>(count + i) : 0u;
        }
#pragma unroll
        for (u32 j = 0; j < GENE_ITEMS; ++j) gene_add<LDS>(f[j] - 1u - lo, k[j], n_genes, s_cnt, cells, umis, lane);   // (feature 0 wraps beyond every range)
    }
    __device__ __forceinline__ void flush(u32 i, u64 v) const {
        if (v >> 32) atomicAdd(cells + i, (u32)(v >> 32));
        if (v & 0xFFFFFFFFull) atomicAdd(umis + i, v & 0xFFFFFFFFull);
    }
};

// feature[i] (1-based), count[i]; *n_ptr rows.  The caller has cleared cells_all[0 .. n_features_all) and umis_all[0 .. n_features_all).
template <bool LDS>
__global__ __launch_bounds__(GENE_THREADS) void gene_summary_kernel(const u32* __restrict__ feature, const u32* __restrict__ count, const u64* __restrict__ n_ptr,
                                                                    u32 n_features_all, u32* __restrict__ cells_all, u64* __restrict__ umis_all, u32 n_ranges) {
    extern __shared__ u64 s_gene[];
    ranged_hist<LDS>(GeneSummaryHist{feature, count, *n_ptr, cells_all, umis_all}, n_features_all, n_ranges, s_gene);
}

// Replicates: cells[g] of one seed's point into the accumulators of its grid point — detected[g] += (cells[g] >= 1), sum[g] += cells[g],
// sumsq[g] += cells[g]^2, all u64.  The sum of squares is exact while it stays below 2^64: for the 64 seeds a run takes at most,
// cell counts below 2^29 (5.4e8 cells) — far beyond any barcode list; three adds of 2^31 (3 * 2^62) still fit, a fifth would not.  Elementwise: gene g belongs to one thread, so
// there are no atomics; per gene one 4-byte load of cells, the three accumulators read and written back.  The launch follows the
// point's gene summary on the same stream and the accumulators of a point are touched by one launch at a time.
constexpr u32 GENE_REPS_THREADS = 256;
__global__ __launch_bounds__(GENE_REPS_THREADS) void gene_reps_kernel(const u32* __restrict__ cells, u32 n_features, u64* __restrict__ detected,
                                                                      u64* __restrict__ sum, u64* __restrict__ sumsq) {
    for (u64 g = (u64)blockIdx.x * GENE_REPS_THREADS + threadIdx.x; g < n_features; g += (u64)gridDim.x * GENE_REPS_THREADS) {
        const u64 c = cells[g];
        detected[g] += c != 0 ? 1ull : 0ull;
        sum[g] += c;
        sumsq[g] += c * c;
    }
}

}  // namespace fastf
