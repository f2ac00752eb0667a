// ranged_hist.hpp — the skeleton of the per-bin reductions whose counters live in LDS: cell_hits_kernel (cap_kernels.hpp),
// gene_summary_kernel (gene_kernels.hpp), gene_moments_kernel (gene_fidelity_kernels.hpp).  DESIGN 10p.
//
// Rows in any order are added into a table of n_bins_all bins that the caller has cleared.
//   LDS = true    workgroup-private counters in dynamic LDS, P::BINS bins of P::WORDS words each = 128 KiB of the CU's 160 KiB:
//                 one 1024-thread workgroup per CU (16 waves, 4 per SIMD); a table of 80 KiB and less lets two of them share a
//                 CU, which is then full at 32 waves.  LDS atomics per row; at the end one global atomic per non-zero counter.
//                 A table of up to <kernel>_LDS_RANGES times as many bins is cut into ranges of P::BINS bins: workgroup b counts
//                 range b % n_ranges (the grid is a multiple of n_ranges), the workgroups of one range share the rows among
//                 them, and every range reads all rows — cheap next to what the general form costs.
//   LDS = false   beyond that: global atomics from every workgroup; n_ranges = 1.
// Contention: bins are log-normal in size, and the tests have one bin that owns every row.  In both forms a 64-row item whose
// counted rows all name ONE bin costs one atomic per word (wave_hits below), not 64 serialised ones on one address.  What a
// kernel does about a few equal bins among 64 rows is its add function's business.
//
// A policy P says what differs between the kernels:
//   word, WORDS, BINS     the counter word, words per bin, bins per range
//   THREADS, n, TURN      the workgroup; the length of the input and a wave's share of it per turn, in rows or in blocks of rows
//   shift(lo)             moves the output pointers to the range that starts at bin lo (0-based)
//   turn<LDS>(base, ...)  loads the turn that starts at `base` (all loads in flight before the first atomic) and adds it into s
//                         (LDS form) or the outputs.  A row counts when its bin minus lo is below n_bins as an UNSIGNED number:
//                         a bin below the range wraps beyond it, and so does the "no bin" value.  Nothing else keeps a row out.
//   flush(i, v)           adds the non-zero counter word i of the range (bin i / WORDS) to the outputs
#pragma once
#include "umi_kernels.hpp"

namespace fastf {

// The hits of one 64-row item, all wave-uniform: which lanes count, the first of them, its bin, and whether every hit names that
// bin.  leader, bin and one_bin mean something where mask != 0.  SEVERAL: a single hit is not "one bin" (for callers that fold
// values across the wave, which one row does not need; a caller that adds the population count takes it either way).
struct WaveHits { u64 mask; int leader; u32 bin; bool one_bin; };
template <bool SEVERAL>
__device__ __forceinline__ WaveHits wave_hits(bool hit, u32 bin) {
    WaveHits h{__ballot(hit), 0, 0u, false};
    if (!h.mask) return h;                                                 // (uniform)
    h.leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)h.mask) - 1);
    h.bin = (u32)__builtin_amdgcn_readlane((int)bin, h.leader);
    h.one_bin = (!SEVERAL || (h.mask & (h.mask - 1))) && __ballot(hit && bin == h.bin) == h.mask;
    return h;
}

// s: the kernel's dynamic LDS (LDS form): min(n_bins_all, P::BINS) * P::WORDS words
template <bool LDS, class P>
__device__ __forceinline__ void ranged_hist(P p, u32 n_bins_all, u32 n_ranges, typename P::word* __restrict__ s) {
    const int tid = threadIdx.x, lane = lane_id();
    constexpr u32 WAVES = P::THREADS / WAVE;
    const u32 lo = LDS ? (blockIdx.x % n_ranges) * P::BINS : 0u;           // first bin (0-based) of this workgroup's range
    const u32 n_bins = LDS ? (n_bins_all - lo < P::BINS ? n_bins_all - lo : P::BINS) : n_bins_all;
    const u32 group = blockIdx.x / n_ranges, groups = gridDim.x / n_ranges;
    p.shift(lo);
    if constexpr (LDS) {
        for (u32 i = tid; i < P::WORDS * n_bins; i += P::THREADS) s[i] = 0;
        __syncthreads();
    }
    for (u64 base = ((u64)group * WAVES + (u32)(tid >> 6)) * P::TURN; base < p.n; base += (u64)groups * WAVES * P::TURN)
        p.template turn<LDS>(base, lo, n_bins, s, lane);
    if constexpr (LDS) {
        __syncthreads();
        for (u32 i = tid; i < P::WORDS * n_bins; i += P::THREADS) {
            const typename P::word v = s[i];
            if (v) p.flush(i, v);
        }
    }
}

}  // namespace fastf
