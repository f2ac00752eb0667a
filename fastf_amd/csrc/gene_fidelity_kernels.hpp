// gene_fidelity_kernels.hpp — the kernels of --gene-fidelity (resident.c): a grid point's matrix Y against the full-depth matrix X of
// the same (cell rate, seed) pair, reduced along the gene axis.
//
//   partner_counts_kernel   point rows and full rows, both ascending by (cell, feature), every point row with a partner among the
//                           full rows -> x[i] = the count of the full row with the (cell, feature) of point row i
//   gene_moments_kernel     rows (feature, a, b) in any order -> sum_ab[g - 1] = the sum of a * b over the rows of gene g,
//                           sum_bb[g - 1] = the sum of b * b
//
// On (X, x, x) gene_moments_kernel gives sum_xx, on (Y, x of y, y) sum_xy and sum_yy.  The sums of the counts and the rows with
// count >= 1 per gene are gene_summary_kernel's.
#pragma once
#include "fidelity_kernels.hpp"
#include "gene_kernels.hpp"

namespace fastf {

// The span of a wave and the walk of the full rows are fidelity_kernel's (fid_lower_bound once per span, then fid_partner per turn
// of 64 point rows: every full row of the span's window is read once, by one coalesced load; no row from *m_ptr on is read).  What
// fidelity_kernel folds into a per-cell scan is stored here: one coalesced 4-byte store per point row, x[i] for i < *n_ptr alone.
// A point row without a partner raises ERR_NO_PARTNER and stores x = 0.
__global__ __launch_bounds__(FID_THREADS) void partner_counts_kernel(const u32* __restrict__ xf, const u32* __restrict__ xc, const u32* __restrict__ xk,
                                                                     const u64* __restrict__ m_ptr, const u32* __restrict__ yf, const u32* __restrict__ yc,
                                                                     const u64* __restrict__ n_ptr, u32* __restrict__ x_out, u64* __restrict__ err) {
    const int lane = lane_id();
    const u64 n = *n_ptr, m = *m_ptr;
    const u64 waves = (u64)gridDim.x * (FID_THREADS / WAVE), w = (u64)blockIdx.x * (FID_THREADS / WAVE) + (threadIdx.x >> 6);
    const u64 span = (((n + waves - 1) / waves) + 63) & ~63ull;
    const u64 a = w * span;
    if (a >= n) return;                                                    // (uniform per wave)
    const u64 b = a + span < n ? a + span : n;
    constexpr u32 NONE = 0xFFFFFFFFu;                                      // (an invalid lane's key is above every key of a row)
    u64 cur = fid_lower_bound(xc, xf, m, fid_key(yc, yf, a), lane) & ~63ull;
    u64 ckey = ~0ull; u32 ccnt = 0;
    bool have = false, missing = false;
    for (u64 base = a; base < b; base += WAVE) {
        const u64 i = base + (u64)lane;
        const bool valid = i < b;
        const u32 c = valid ? ld_once<FASTF_NT_K3 != 0>(yc + i) : NONE;
        const u32 f = valid ? ld_once<FASTF_NT_K3 != 0>(yf + i) : NONE;
        const u64 key = ((u64)c << 32) | (u64)f;
        const int n_valid = (int)(b - base < (u64)WAVE ? b - base : (u64)WAVE);
        const u64 last_key = fid_readlane64(key, n_valid - 1);             // the largest key of the turn (uniform)
        u32 x = 0; bool found = !valid;
        fid_partner(xf, xc, xk, m, key, last_key, lane, cur, ckey, ccnt, have, x, found);
        missing |= !found;
        if (valid) x_out[i] = x;
    }
    if (__ballot(missing) && lane == 0) atomicOr(err, ERR_NO_PARTNER);
}

// A ranged histogram (ranged_hist.hpp) with two 64-bit numbers per gene that do not share a word, side by side (sum_ab, sum_bb):
// a * b and b * b both reach 2^64 - 1 under the ABI's precondition (the sum of all counts below 2^32).  One ds_add_u64 (LDS form) or
// global atomic (general form) per word and counted row.
// A row with b == 0 adds nothing to either sum and issues no atomic; one with a == 0 issues none for sum_ab.  Equal genes among 64
// rows short of all of them are left to the atomic unit, as in gene_add.  A feature outside 1 .. n_features writes nothing.
constexpr u32 GMOM_LDS_GENES = GENE_LDS_GENES / 2, GMOM_LDS_RANGES = 2 * GENE_LDS_RANGES;

template <bool LDS>
__device__ __forceinline__ void gmom_add(u32 idx, u32 a, u32 b, u32 n_genes, u64* __restrict__ s_cnt, u64* __restrict__ sum_ab, u64* __restrict__ sum_bb, int lane) {
    const bool hit = idx < n_genes && b != 0u;
    const WaveHits h = wave_hits<true>(hit, idx);
    if (!h.mask) return;                                                   // (uniform)
    u64 ab = hit && sum_ab ? (u64)a * (u64)b : 0ull, bb = hit ? (u64)b * (u64)b : 0ull;   // (no sum_ab asked for: its counters stay 0)
    if (h.one_bin) { ab = wave_sum64(ab); bb = wave_sum64(bb); }           // (neither can carry: precondition)
    if (h.one_bin ? lane == h.leader : hit) {
        if constexpr (LDS) {
            if (ab) (void)__hip_atomic_fetch_add(s_cnt + 2u * idx, ab, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            (void)__hip_atomic_fetch_add(s_cnt + 2u * idx + 1u, bb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
            if (ab) atomicAdd(sum_ab + idx, ab);
            atomicAdd(sum_bb + idx, bb);
        }
    }
}

struct GeneMomentsHist {
    typedef u64 word;
    static constexpr u32 WORDS = 2, BINS = GMOM_LDS_GENES, THREADS = GENE_THREADS;
    static constexpr u64 TURN = (u64)GENE_ITEMS * WAVE;
    const u32* __restrict__ feature; const u32* __restrict__ va; const u32* __restrict__ vb; u64 n; u64* __restrict__ sum_ab; u64* __restrict__ sum_bb;
    __device__ __forceinline__ void shift(u32 lo) { if (sum_ab) sum_ab += lo; sum_bb += lo; }
    template <bool LDS>
    __device__ __forceinline__ void turn(u64 base, u32 lo, u32 n_genes, u64* __restrict__ s_cnt, int lane) const {
        u32 f[GENE_ITEMS], a[GENE_ITEMS], b[GENE_ITEMS];
#pragma unroll
        for (u32 j = 0; j < GENE_ITEMS; ++j) {
            const u64 i = base + j * WAVE + (u64)lane;
            const bool valid = i < n;
            f[j] = valid ? ld_once<FASTF_NT_K3 != 0>(feature + i) : 0u;
            a[j] = valid ? ld_once<FASTF_NT_K3 != 0>(va + i) : 0u;
            b[j] = valid ? ld_once<FASTF_NT_K3 != 0>(vb + i) : 0u;
        }
#pragma unroll
        for (u32 j = 0; j < GENE_ITEMS; ++j) gmom_add<LDS>(f[j] - 1u - lo, a[j], b[j], n_genes, s_cnt, sum_ab, sum_bb, lane);   // (feature 0 wraps beyond every range)
    }
    __device__ __forceinline__ void flush(u32 i, u64 v) const { atomicAdd(((i & 1u) ? sum_bb : sum_ab) + (i >> 1), v); }
};

// feature[i] (1-based), a[i], b[i]; *n_ptr rows.  The caller has cleared ab_all[0 .. n_features_all) and bb_all[0 .. n_features_all).
// ab_all == nullptr: sum_bb alone — no a * b is formed, added or flushed (sum_xx of the full rows needs one sum, not two equal ones).
template <bool LDS>
__global__ __launch_bounds__(GENE_THREADS) void gene_moments_kernel(const u32* __restrict__ feature, const u32* __restrict__ va, const u32* __restrict__ vb,
                                                                    const u64* __restrict__ n_ptr, u32 n_features_all, u64* __restrict__ ab_all,
                                                                    u64* __restrict__ bb_all, u32 n_ranges) {
    extern __shared__ u64 s_gmom[];
    ranged_hist<LDS>(GeneMomentsHist{feature, va, vb, *n_ptr, ab_all, bb_all}, n_features_all, n_ranges, s_gmom);
}

}  // namespace fastf
