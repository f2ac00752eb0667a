// gene_kernels.hpp — the kernel behind `--genes` of `fastF sweep` and `fastF cap` (resident.c): the COO rows of a point reduced
// along the gene axis, the counterpart of cell_summary_kernel (sweep_kernels.hpp).
//
//   gene_summary_kernel   rows (feature, count) in any order -> cells_per_gene[g - 1] = rows of gene g with count >= 1 (the rule of
//                         genes_per_cell), umis_per_gene[g - 1] = the sum of their counts
//   gene_reps_kernel      replicate runs (--seeds, --reps): the cells_per_gene of one (grid point, seed) added into the three u64
//                         accumulators of its grid point
#pragma once
#include "umi_kernels.hpp"

namespace fastf {

// The rows arrive ascending by (cell, feature): the rows of one gene are scattered over the whole array, and the 64 rows of a wave
// are — inside a cell — 64 different genes.  A histogram, as cell_hits_kernel (cap_kernels.hpp) is one, with two numbers per bin.
//
//   LDS = true    workgroup-private counters of 64 bits: one ds_add_u64 of (1 << 32 | count) per row keeps the rows in the high
//                 half and the sum of the counts in the low half.  Exact as long as the low half cannot carry — the ABI's
//                 precondition: the sum of ALL counts is below 2^32 (it is a number of records, and the device-level calls stop
//                 at 2^32 - 2 records).  GENE_LDS_GENES counters = 128 KiB of the CU's 160 KiB: one 1024-thread workgroup per CU;
//                 from 10 240 genes down (80 KiB) two.  A list of up to GENE_LDS_RANGES times as many genes is cut into ranges:
//                 workgroup b counts range b % n_ranges, the workgroups of a range share the rows, every range reads all rows.
//                 Flushed with one global atomic per non-zero half of a counter (the two halves go to two arrays).
//   LDS = false   beyond that: global atomics, two per row (one per array).
// A row with count 0 adds nothing to either number and issues no atomic.  In both forms a 64-row item whose counted rows all name
// ONE gene (a fixture where one gene owns every row; a matrix of one feature) is summed across the wave and costs one atomic per
// array, not 64 serialised ones on one address.  Two or three equal genes among 64 rows (a cell boundary inside the item) are left
// to the atomic unit: aggregating them would cost every item a loop over its distinct genes.
// A feature outside 1 .. n_features writes nothing (as cell_emit).
constexpr u32 GENE_LDS_GENES = 16384, GENE_THREADS = 1024, GENE_LDS_RANGES = 8, GENE_ITEMS = 4;

template <bool LDS>
__device__ __forceinline__ void gene_add(u32 idx, u32 k, u32 n_genes, u64* __restrict__ s_cnt, u32* __restrict__ cells, u64* __restrict__ umis, int lane) {
    const bool hit = idx < n_genes && k != 0u;                              // (a gene below the range wrapped beyond it)
    const u64 rem = __ballot(hit);
    if (!rem) return;                                                      // (uniform)
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)rem) - 1);
    const u32 g0 = (u32)__builtin_amdgcn_readlane((int)idx, leader);
    u64 v = hit ? ((1ull << 32) | (u64)k) : 0ull;
    const bool one_gene = (rem & (rem - 1)) && __ballot(hit && idx == g0) == rem;   // (uniform) several rows, all of one gene
    if (one_gene) v = wave_sum64(v);                                        // (the low half cannot carry: precondition)
    if (one_gene ? lane == leader : hit) {
        if constexpr (LDS) (void)__hip_atomic_fetch_add(s_cnt + idx, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else { atomicAdd(cells + idx, (u32)(v >> 32)); atomicAdd(umis + idx, v & 0xFFFFFFFFull); }
    }
}

// feature[i] (1-based), count[i]; *n_ptr rows.  The caller has cleared cells_all[0 .. n_features_all) and umis_all[0 .. n_features_all).
// n_ranges (LDS form; the grid is a multiple of it): see above; 1 in the general form.  Dynamic LDS (LDS form):
// min(n_features_all, GENE_LDS_GENES) * 8 bytes.
// A wave takes GENE_ITEMS neighbouring items of 64 rows per turn (all loads of a turn are in flight before the first atomic).
template <bool LDS>
__global__ __launch_bounds__(GENE_THREADS) void gene_summary_kernel(const u32* __restrict__ feature, const u32* __restrict__ count, const u64* __restrict__ n_ptr,
                                                                    u32 n_features_all, u32* __restrict__ cells_all, u64* __restrict__ umis_all, u32 n_ranges) {
    extern __shared__ u64 s_gene[];
    const int tid = threadIdx.x, lane = lane_id();
    constexpr u32 WAVES = GENE_THREADS / WAVE;
    const u64 n = *n_ptr;
    const u32 lo = LDS ? (blockIdx.x % n_ranges) * GENE_LDS_GENES : 0u;     // first gene (0-based) of this workgroup's range
    const u32 n_genes = LDS ? (n_features_all - lo < GENE_LDS_GENES ? n_features_all - lo : GENE_LDS_GENES) : n_features_all;
    u32* const cells = cells_all + lo; u64* const umis = umis_all + lo;
    const u32 group = blockIdx.x / n_ranges, groups = gridDim.x / n_ranges;
    if constexpr (LDS) {
        for (u32 i = tid; i < n_genes; i += GENE_THREADS) s_gene[i] = 0;
        __syncthreads();
    }
    constexpr u64 TURN = (u64)GENE_ITEMS * WAVE;
    for (u64 base = ((u64)group * WAVES + (u32)(tid >> 6)) * TURN; base < n; base += (u64)groups * WAVES * TURN) {
        u32 f[GENE_ITEMS], k[GENE_ITEMS];
#pragma unroll
        for (u32 j = 0; j < GENE_ITEMS; ++j) {
            const u64 i = base + j * WAVE + (u64)lane;
            const bool valid = i < n;
            f[j] = valid ? ld_once<FASTF_NT_K3 != 0>(feature + i) : 0u;
            k[j] = valid ? ld_once<FASTF_NT_K3 != 0>(count + i) : 0u;
        }
#pragma unroll
        for (u32 j = 0; j < GENE_ITEMS; ++j) gene_add<LDS>(f[j] - 1u - lo, k[j], n_genes, s_gene, cells, umis, lane);   // (feature 0 wraps beyond every range)
    }
    if constexpr (LDS) {
        __syncthreads();
        for (u32 i = tid; i < n_genes; i += GENE_THREADS) {
            const u64 v = s_gene[i];
            if (v >> 32) atomicAdd(cells + i, (u32)(v >> 32));
            if (v & 0xFFFFFFFFull) atomicAdd(umis + i, v & 0xFFFFFFFFull);
        }
    }
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
