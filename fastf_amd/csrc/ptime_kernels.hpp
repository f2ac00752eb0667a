// ptime_kernels.hpp — the kernels of --pseudotime (resident.c): per cell the lower median of the ranks its neighbours carry, and the exact
// all-pairs order census (Kendall's tau-b) of that estimate against the cells' own ranks.  The definition is in include/fastf_amd.h.
//
//   pt_median_kernel<G>   idx (k slots a cell, cnt[i] of them valid, the others 0xFFFFFFFF), t (u32 per cell, 0: no value)
//                         -> est[i] = the lower median of { t[j] : j in the set of i, t[j] > 0 }, valued[i] = their number (est 0 with none)
//   pt_pairs_kernel       est, t -> out[7] (u64): conc disc tie_e tie_t tie_both cells shift_sum over the cells with t > 0 and est > 0
//
// pt_median_kernel: a cell owns a lane group of G = 16, 32 or 64 lanes, the smallest that holds k, as in label_votes_kernel.  Lane s
// gathers t of neighbour s; the lanes of a group read each other's value by G shuffles and count, each for itself, the valid lanes in
// front of it under the total order (value, slot).  The lane whose position is ceil(c / 2) - 1 holds the lower median.  No lane keeps an
// array and nothing is sorted.
// pt_pairs_kernel: a workgroup owns ONE pair of tiles (a <= b) of PT_TILE cells.  Both tiles are compacted into LDS — the cells that
// are absent leave here, so the pair loop tests nothing but the order — then every thread keeps PT_ROWS cells of tile a in registers
// and walks the cells of tile b, which all lanes read from the same LDS address (a broadcast).  Four classes are counted, the fifth
// is what is left of the pairs of the tile pair.  n x n is never stored: the traffic is 2 * PT_TILE cells per PT_TILE^2 pairs.
#pragma once
#include "umi_kernels.hpp"

namespace fastf {

constexpr u32 PT_THREADS = 256;
constexpr u32 PT_MAX_K = 64;
constexpr u32 PT_TILE = 1024;                                   // the edge of a tile of the census: cells per tile
constexpr u32 PT_ROWS = PT_TILE / PT_THREADS;                   // the cells of tile a one thread keeps
constexpr u32 PT_MAX_TILES = 65535;                             // T (T + 1) / 2 tile pairs stay below 2^31, the grid's limit
constexpr u32 PT_MAX_CELLS = PT_MAX_TILES * PT_TILE;
enum { PT_CONC, PT_DISC, PT_TIE_E, PT_TIE_T, PT_TIE_BOTH, PT_CELLS, PT_SHIFT, PT_OUT_WORDS };
static_assert(PT_TILE % PT_THREADS == 0 && PT_THREADS % 64 == 0, "whole waves, whole rows");
static_assert((u64)PT_ROWS * PT_TILE < (1ull << 32), "a thread's share of a tile pair fits its u32 counters");

// One pass of a workgroup covers PT_THREADS / G cells; the passes of a workgroup are gridDim.x * (PT_THREADS / G) cells apart.  Every
// lane stays in the loop for every pass of its workgroup (a lane without a cell or without a valid slot holds 0): the shuffles and the
// ballot see whole waves.  An index of n and beyond and every slot from cnt[i] on is never used as an index.
template <u32 G>
__global__ __launch_bounds__(PT_THREADS) void pt_median_kernel(const u32* __restrict__ idx, const u32* __restrict__ cnt, const u32* __restrict__ t,
                                                               u32 n, u32 k, u32* __restrict__ est_out, u32* __restrict__ valued_out) {
    static_assert(G == 16 || G == 32 || G == 64, "a lane group is 16, 32 or 64 lanes");
    constexpr u32 PER_PASS = PT_THREADS / G;
    const u32 lane = lane_id(), s = lane & (G - 1u), first = lane & ~(G - 1u);
    const u64 group_mask = (G == 64 ? ~0ull : ((1ull << (G & 63u)) - 1ull)) << first;
    const u32 passes = (n + PER_PASS * gridDim.x - 1u) / (PER_PASS * gridDim.x);
    for (u32 p = 0; p < passes; ++p) {
        const u64 i = ((u64)p * gridDim.x + blockIdx.x) * PER_PASS + threadIdx.x / G;
        const bool cell = i < n;
        u32 v = 0;
        if (cell) {
            const u32 c = cnt[i] < k ? cnt[i] : k;
            if (s < c) {
                const u32 j = idx[i * k + s];
                if (j < n) v = t[j];
            }
        }
        const u32 c_valid = (u32)__popcll(__ballot(v != 0) & group_mask);
        // the valid lanes of the group in front of this one: a smaller value, or the same value in a lower slot
        u32 pos = 0;
#pragma unroll
        for (u32 o = 0; o < G; ++o) {
            const u32 w = (u32)__shfl((int)v, (int)(first + o));
            pos += (w != 0 && (w < v || (w == v && o < s))) ? 1u : 0u;
        }
        if (cell) {
            if (c_valid == 0) { if (s == 0) { est_out[i] = 0; valued_out[i] = 0; } }
            else if (v != 0 && pos == (c_valid + 1u) / 2u - 1u) { est_out[i] = v; valued_out[i] = c_valid; }
        }
    }
}

// The cells base .. base + PT_TILE - 1 that take part (t > 0 and est > 0), in their order, into s_tile as (est, t); returns their
// number, the same in every thread.  s_wave: one word per wave.  Ends behind a barrier: s_tile can be read, s_wave can be used again.
__device__ inline u32 pt_tile_compact(const u32* __restrict__ est, const u32* __restrict__ t, u64 base, u32 n, uint2* s_tile, u32* s_wave) {
    const u32 lane = lane_id(), wave = threadIdx.x >> 6;
    u32 m = 0;
    for (u32 q = 0; q < PT_ROWS; ++q) {
        const u64 i = base + (u64)q * PT_THREADS + threadIdx.x;
        u32 e = 0, r = 0;
        if (i < n) { r = t[i]; e = est[i]; }
        const bool present = r != 0 && e != 0;
        const u64 mask = __ballot(present);
        if (lane == 0) s_wave[wave] = (u32)__popcll(mask);
        __syncthreads();
        u32 off = m;
        for (u32 w = 0; w < PT_THREADS / 64; ++w) { const u32 c = s_wave[w]; off += w < wave ? c : 0u; m += c; }
        if (present) s_tile[off + (u32)__popcll(mask & ((1ull << lane) - 1ull))] = make_uint2(e, r);
        __syncthreads();
    }
    return m;
}

// blockIdx.x = b (b + 1) / 2 + a, a <= b: the pair of tiles of a workgroup
__device__ inline void pt_tile_pair(u32 p, u32& a, u32& b) {
    u64 bb = (u64)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while (bb * (bb + 1) / 2 > p) --bb;
    while ((bb + 1) * (bb + 2) / 2 <= p) ++bb;
    b = (u32)bb; a = (u32)(p - bb * (bb + 1) / 2);
}

// The pairs of the compacted tiles s_a (m_a cells, the rows) and s_b (m_b cells, the columns): row r against every column, in the
// diagonal tile (DIAG: s_a == s_b) against the columns behind it alone, so that every pair i < j is met once.  Per thread and row four
// u32 counters: at most PT_TILE pairs a row.
template <bool DIAG>
__device__ inline void pt_count(const uint2* s_a, u32 m_a, const uint2* s_b, u32 m_b, u32 (&conc)[PT_ROWS], u32 (&disc)[PT_ROWS], u32 (&tie_e)[PT_ROWS], u32 (&tie_t)[PT_ROWS]) {
    u32 re[PT_ROWS], rt[PT_ROWS];
#pragma unroll
    for (u32 q = 0; q < PT_ROWS; ++q) {
        const u32 r = q * PT_THREADS + threadIdx.x;
        const uint2 x = r < m_a ? s_a[r] : make_uint2(0u, 0u);
        re[q] = x.x; rt[q] = x.y;
    }
    for (u32 c = 0; c < m_b; ++c) {
        const uint2 y = s_b[c];                                 // (every lane the same address)
#pragma unroll
        for (u32 q = 0; q < PT_ROWS; ++q) {
            const bool le = re[q] < y.x, ge = re[q] > y.x, lt = rt[q] < y.y, gt = rt[q] > y.y;
            const bool take = !DIAG || c > q * PT_THREADS + threadIdx.x;
            conc[q] += (take && ((le && lt) || (ge && gt))) ? 1u : 0u;
            disc[q] += (take && ((le && gt) || (ge && lt))) ? 1u : 0u;
            tie_e[q] += (take && !le && !ge && (lt || gt)) ? 1u : 0u;
            tie_t[q] += (take && !lt && !gt && (le || ge)) ? 1u : 0u;
        }
    }
}

// out is zeroed by the caller.  A workgroup's counts fit u32 (PT_TILE^2 pairs at the most); what leaves a wave is added up in u64.
__global__ __launch_bounds__(PT_THREADS) void pt_pairs_kernel(const u32* __restrict__ est, const u32* __restrict__ t, u32 n, u64* __restrict__ out) {
    __shared__ uint2 s_a[PT_TILE], s_b[PT_TILE];
    __shared__ u32 s_wave[PT_THREADS / 64];
    __shared__ u64 s_sum[PT_OUT_WORDS];
    u32 a, b;
    pt_tile_pair(blockIdx.x, a, b);
    if (threadIdx.x < PT_OUT_WORDS) s_sum[threadIdx.x] = 0;
    const u32 m_a = pt_tile_compact(est, t, (u64)a * PT_TILE, n, s_a, s_wave);
    const u32 m_b = a == b ? m_a : pt_tile_compact(est, t, (u64)b * PT_TILE, n, s_b, s_wave);
    u32 conc[PT_ROWS] = {}, disc[PT_ROWS] = {}, tie_e[PT_ROWS] = {}, tie_t[PT_ROWS] = {};
    if (a == b) pt_count<true>(s_a, m_a, s_a, m_a, conc, disc, tie_e, tie_t);
    else pt_count<false>(s_a, m_a, s_b, m_b, conc, disc, tie_e, tie_t);
    // the rows beyond m_a held (0, 0) and counted what they met: they are left out here
    u32 v[4] = {0, 0, 0, 0};
    u64 shift = 0;
#pragma unroll
    for (u32 q = 0; q < PT_ROWS; ++q) {
        const u32 r = q * PT_THREADS + threadIdx.x;
        if (r < m_a) {
            v[0] += conc[q]; v[1] += disc[q]; v[2] += tie_e[q]; v[3] += tie_t[q];
            if (a == b) { const uint2 x = s_a[r]; shift += x.x > x.y ? x.x - x.y : x.y - x.x; }
        }
    }
    // a wave's sums: 64 threads x PT_ROWS x PT_TILE pairs at the most, which is 2^18
#pragma unroll
    for (u32 off = 32; off; off >>= 1) {
#pragma unroll
        for (u32 w = 0; w < 4; ++w) v[w] += (u32)__shfl_xor((int)v[w], (int)off);
        shift += (u64)__shfl_xor((long long)shift, (int)off);
    }
    if (lane_id() == 0) {
#pragma unroll
        for (u32 w = 0; w < 4; ++w) if (v[w]) atomicAdd((unsigned long long*)&s_sum[w], (unsigned long long)v[w]);
        if (shift) atomicAdd((unsigned long long*)&s_sum[PT_SHIFT], (unsigned long long)shift);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 pairs = a == b ? (u64)m_a * (m_a - (m_a ? 1u : 0u)) / 2 : (u64)m_a * m_b;
        s_sum[PT_TIE_BOTH] = pairs - s_sum[PT_CONC] - s_sum[PT_DISC] - s_sum[PT_TIE_E] - s_sum[PT_TIE_T];
        if (a == b) s_sum[PT_CELLS] = m_a;
    }
    __syncthreads();
    if (threadIdx.x < PT_OUT_WORDS && s_sum[threadIdx.x]) atomicAdd((unsigned long long*)&out[threadIdx.x], (unsigned long long)s_sum[threadIdx.x]);
}

}  // namespace fastf
