// sweep_kernels.hpp — the two kernels of `fastF sweep` (sweep_cmds.c): a grid of (cell rate, depth rate) points from ONE decode
// of the BAM.  The records, K1a's cell scratch and the MT19937 draw stream are the same for every depth rate of one
// (cell rate, seed); only the threshold the draws are compared against differs.
//
//   draw_planes_kernel    draws -> R decision planes in one pass: plane j, bit i = draws[i] < threshold[j]
//                         (draw_bits_kernel of umi_kernels.hpp does this for one threshold and would read the words R times)
//   cell_summary_kernel   COO rows ascending by (cell, feature) -> per cell the sum of the counts and the number of rows with
//                         count >= 1, plus the grand sum: what the sweep's summary table needs, without the rows leaving the device
#pragma once
#include "umi_kernels.hpp"

namespace fastf {

// ------------------------------------------------------------------------------------
// decision planes
// ------------------------------------------------------------------------------------
constexpr u32 PLANES_MAX = 16;                     // thresholds of one launch (kernel arguments; a longer list takes several launches)
struct PlaneSet { u64 threshold[PLANES_MAX]; u32 n; };

// A wave owns four 64-bit words of every plane per turn, as draw_bits_kernel owns four words of its one ring: each lane
// loads its four draws once, the ballot of `draw < threshold[j]` IS word c of plane j.  Lane j keeps the ballots of plane j
// (a v_cndmask per plane and word), so the R words of one column leave in ONE vector store with R lanes active instead of
// R single-lane stores.  Linear arrays only: plane j starts at planes + j * plane_stride (64-bit words), bit 0 = draw 0, the
// bits of the last word above n are zero (lanes beyond n vote false).
__global__ __launch_bounds__(256) void draw_planes_kernel(const u32* __restrict__ draws, u64 n, const PlaneSet ps, u64* __restrict__ planes, u64 plane_stride) {
    const int lane = lane_id();
    const u64 n_words = (n + 63) >> 6;
    const u64 waves = (u64)gridDim.x * (256 / WAVE), w0 = (u64)blockIdx.x * (256 / WAVE) + (threadIdx.x >> 6);
    constexpr u32 U = 4;
    for (u64 c0 = w0 * U; c0 < n_words; c0 += waves * U) {
        u32 d[U]; bool in[U];
#pragma unroll
        for (u32 u = 0; u < U; ++u) {
            const u64 r = ((c0 + u) << 6) + (u64)lane;
            in[u] = r < n;
            d[u] = ld_once<FASTF_NT_K1B != 0>(draws + (in[u] ? r : 0));
        }
        u64 mine[U] = {0, 0, 0, 0};
        for (u32 j = 0; j < ps.n; ++j) {                                   // (uniform: the thresholds are scalar loads of the kernel arguments)
            const u64 t = ps.threshold[j];
#pragma unroll
            for (u32 u = 0; u < U; ++u) {
                const u64 m = __ballot(in[u] && (u64)d[u] < t);
                if ((u32)lane == j) mine[u] = m;
            }
        }
        if ((u32)lane < ps.n) {
            u64* const col = planes + (u64)lane * plane_stride + c0;
#pragma unroll
            for (u32 u = 0; u < U; ++u)
                if (c0 + u < n_words) col[u] = mine[u];
        }
    }
}

// ------------------------------------------------------------------------------------
// per-cell summary of sorted COO rows
// ------------------------------------------------------------------------------------
// cell[i] (1-based) ascending, count[i]; *n_ptr rows.  umis[c - 1] = sum of the counts of cell c, genes[c - 1] = its rows with
// count >= 1, umis[n_cells] = the sum of all counts.  The caller has cleared umis[0 .. n_cells] and genes[0 .. n_cells).
//
// Every wave owns one contiguous span of the rows (a multiple of 64) and walks it 64 rows a turn.  Rows of one cell are
// neighbours, so a segmented inclusive scan needs no head flags: a lane adds the lane o below it iff that lane holds the same
// cell (sorted: then so do all lanes between).  The last lane of a cell in the turn holds the cell's sum over the turn; the
// cell still open in lane 63 is carried into the next turn in scalar registers.  A cell whose rows all lie inside the span is
// written with one plain store by its last lane; only a cell that also has rows in a neighbouring span (the one before the
// span's first row, the one behind its last) is added with atomics, by every wave that holds a piece of it.
__device__ __forceinline__ void cell_emit(u32 c, u64 u, u32 g, u32 prev_c, u32 next_c, u32 n_cells, u64* __restrict__ umis, u32* __restrict__ genes) {
    if (c - 1u >= n_cells) return;                                         // (a cell index the caller did not size the arrays for: nothing is written)
    if (c == prev_c || c == next_c) { atomicAdd(umis + (c - 1u), u); atomicAdd(genes + (c - 1u), g); }
    else { umis[c - 1u] = u; genes[c - 1u] = g; }
}

__global__ __launch_bounds__(256) void cell_summary_kernel(const u32* __restrict__ cell, const u32* __restrict__ count, const u64* __restrict__ n_ptr,
                                                           u32 n_cells, u64* __restrict__ umis, u32* __restrict__ genes) {
    const int lane = lane_id();
    const u64 n = *n_ptr;
    const u64 waves = (u64)gridDim.x * (256 / WAVE), w = (u64)blockIdx.x * (256 / WAVE) + (threadIdx.x >> 6);
    const u64 span = (((n + waves - 1) / waves) + 63) & ~63ull;
    const u64 a = w * span;
    if (a >= n) return;                                                    // (uniform per wave)
    const u64 b = a + span < n ? a + span : n;
    constexpr u32 NONE = 0xFFFFFFFFu;                                      // no cell: indices are 1-based and below 2^32 - 1
    const u32 prev_c = a > 0 ? cell[a - 1] : NONE, next_c = b < n ? cell[b] : NONE;
    u32 carry_c = NONE, carry_g = 0; u64 carry_u = 0, total = 0;
    for (u64 base = a; base < b; base += WAVE) {
        const u64 i = base + (u64)lane;
        const bool valid = i < b;
        const u32 c = valid ? ld_once<FASTF_NT_K3 != 0>(cell + i) : NONE;
        const u32 k = valid ? ld_once<FASTF_NT_K3 != 0>(count + i) : 0u;
        u64 u = k; u32 g = k ? 1u : 0u;
        total += k;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const u32 co = __shfl_up(c, o, WAVE); const u64 uo = __shfl_up(u, o, WAVE); const u32 go = __shfl_up(g, o, WAVE);
            if (lane >= o && co == c) { u += uo; g += go; }
        }
        const u32 c_next = __shfl_down(c, 1, WAVE);
        // the cell carried in from the turn before: it goes on in this turn's first lanes, or it has ended
        const u32 first_c = (u32)__builtin_amdgcn_readfirstlane((int)c);
        if (carry_c != NONE) {
            if (carry_c == first_c) { if (c == carry_c) { u += carry_u; g += carry_g; } }
            else if (lane == 0) cell_emit(carry_c, carry_u, carry_g, prev_c, next_c, n_cells, umis, genes);
        }
        // lane 63's cell may go on in the next turn: it is carried, not written
        const bool last_of_cell = valid && lane < WAVE - 1 && c_next != c;
        if (last_of_cell) cell_emit(c, u, g, prev_c, next_c, n_cells, umis, genes);
        carry_c = (u32)__builtin_amdgcn_readlane((int)c, WAVE - 1);       // NONE when the turn was not full: the span has ended
        carry_u = ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(u >> 32), WAVE - 1) << 32) | (u64)(u32)__builtin_amdgcn_readlane((int)(u32)u, WAVE - 1);
        carry_g = (u32)__builtin_amdgcn_readlane((int)g, WAVE - 1);
    }
    if (carry_c != NONE && lane == 0) cell_emit(carry_c, carry_u, carry_g, prev_c, next_c, n_cells, umis, genes);
    total = wave_sum64(total);
    if (lane == 0 && total) atomicAdd(umis + n_cells, total);
}

}  // namespace fastf
