// cells_kernels.hpp — the kernel behind `--cells` of `fastF sweep` and `fastF cap` (resident.c): the -u rows of a point (K3u:
// one row per distinct (cell, feature, blob) key with its run length n_copy) reduced along the cell axis and into the
// copy-number histogram.
//
//   copy_summary_kernel   (ukey, n_copy) rows ascending by key -> per cell the reads (sum of n_copy), the reads of its NULL-blob
//                         rows and its non-NULL rows seen once; over all rows the number of non-NULL rows per n_copy
#pragma once
#include "umi_kernels.hpp"

namespace fastf {

constexpr u32 COPY_BINS = 32;                      // = FASTF_COPY_BINS: bins 1 .. 31, the tail bin, and behind it the tail's reads

// The per-cell half is cell_summary_kernel (sweep_kernels.hpp) with three numbers in the scan instead of two: every wave owns one
// contiguous span of the rows (a multiple of 64) and walks it 64 rows a turn; the keys ascend, so the rows of one cell are
// neighbours and a lane adds the lane o below it iff that lane holds the same cell.  The cell still open in lane 63 is carried
// into the next turn in scalar registers; a cell whose rows all lie inside the span is written with plain stores by its last lane,
// only a cell that reaches into a neighbouring span is added with atomics, by every wave that holds a piece of it.
// A cell outside 1 .. n_cells becomes cell 0 at the load: nothing is written for it (rows of two such cells may then share a
// segment, which is of no consequence).  Every per-cell number is below 2^32: it is a number of records.
//
// The histogram half keeps lane-private columns, u32 hist[bin][lane] in LDS (8 KiB a wave): a row is one ds_read + ds_write of
// its own lane's word — bank = lane % 32 whatever the bin, so the 64 lanes never meet, where one LDS atomic per row on 32
// addresses would serialise on the few low bins real data fills (cell_hits_kernel was bound by exactly that).  No lane reads
// another lane's word: at the end of the span every bin is summed across the wave with shuffles, lane b keeps bin b, and the wave
// issues one global 64-bit atomic per non-zero bin.  The reads of the tail rows are summed in a 64-bit register per lane.
struct CopyOut { u32* reads; u32* null_reads; u32* single; };

__device__ __forceinline__ void copy_emit(u32 c, u32 r, u32 z, u32 s, u32 prev_c, u32 next_c, const CopyOut o) {
    if (c == 0u) return;                                                   // (a cell the caller did not size the arrays for)
    if (c == prev_c || c == next_c) {
        atomicAdd(o.reads + (c - 1u), r);
        if (z) atomicAdd(o.null_reads + (c - 1u), z);
        if (s) atomicAdd(o.single + (c - 1u), s);
    } else { o.reads[c - 1u] = r; o.null_reads[c - 1u] = z; o.single[c - 1u] = s; }
}

// the cell of a key as the kernel segments by it: 1 .. n_cells, or 0
__device__ __forceinline__ u32 copy_cell(u64 key, u32 cell_shift, u32 n_cells) {
    const u64 c = key >> cell_shift;
    return c - 1ull < (u64)n_cells ? (u32)c : 0u;
}

// ukeys[i] ascending, ncopy[i]; *n_ptr rows.  The caller has cleared reads / null_reads / single [0 .. n_cells) and
// hist[0 .. COPY_BINS].  nn_shift: the bit of a key that says its blob is not NULL.
__global__ __launch_bounds__(256) void copy_summary_kernel(const u64* __restrict__ ukeys, const u32* __restrict__ ncopy, const u64* __restrict__ n_ptr,
                                                           u32 n_cells, u32 cell_shift, u32 nn_shift, const CopyOut out, u64* __restrict__ hist) {
    __shared__ u32 s_hist[256 / WAVE][COPY_BINS][WAVE];
    const int lane = lane_id();
    const u64 n = *n_ptr;
    const u64 waves = (u64)gridDim.x * (256 / WAVE), w = (u64)blockIdx.x * (256 / WAVE) + (threadIdx.x >> 6);
    const u64 span = (((n + waves - 1) / waves) + 63) & ~63ull;
    const u64 a = w * span;
    if (a >= n) return;                                                    // (uniform per wave; the kernel has no barrier)
    const u64 b = a + span < n ? a + span : n;
    u32 (*const h)[WAVE] = s_hist[threadIdx.x >> 6];
#pragma unroll
    for (u32 k = 0; k < COPY_BINS; ++k) h[k][lane] = 0u;
    constexpr u32 NONE = 0xFFFFFFFFu;                                      // no row: cell indices are below 2^32 - 1
    const u32 prev_c = a > 0 ? copy_cell(ukeys[a - 1], cell_shift, n_cells) : NONE, next_c = b < n ? copy_cell(ukeys[b], cell_shift, n_cells) : NONE;
    u32 carry_c = NONE, carry_r = 0, carry_z = 0, carry_s = 0;
    u64 tail = 0;
    for (u64 base = a; base < b; base += WAVE) {
        const u64 i = base + (u64)lane;
        const bool valid = i < b;
        const u64 key = valid ? ld_once<FASTF_NT_K3 != 0>(ukeys + i) : 0ull;
        const u32 k = valid ? ld_once<FASTF_NT_K3 != 0>(ncopy + i) : 0u;
        const u32 c = valid ? copy_cell(key, cell_shift, n_cells) : NONE;
        const bool nn = ((key >> nn_shift) & 1ull) != 0;
        u32 r = k, z = nn ? 0u : k, s = (nn && k == 1u) ? 1u : 0u;
        if (nn && k) {                                                     // (a row of no reads is in no bin)
            const u32 bin = (k < COPY_BINS ? k : COPY_BINS) - 1u;
            h[bin][lane] += 1u;
            if (k >= COPY_BINS) tail += k;
        }
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const u32 co = __shfl_up(c, o, WAVE), ro = __shfl_up(r, o, WAVE), zo = __shfl_up(z, o, WAVE), so = __shfl_up(s, o, WAVE);
            if (lane >= o && co == c) { r += ro; z += zo; s += so; }
        }
        const u32 c_next = __shfl_down(c, 1, WAVE);
        // the cell carried in from the turn before: it goes on in this turn's first lanes, or it has ended
        const u32 first_c = (u32)__builtin_amdgcn_readfirstlane((int)c);
        if (carry_c != NONE) {
            if (carry_c == first_c) { if (c == carry_c) { r += carry_r; z += carry_z; s += carry_s; } }
            else if (lane == 0) copy_emit(carry_c, carry_r, carry_z, carry_s, prev_c, next_c, out);
        }
        // lane 63's cell may go on in the next turn: it is carried, not written
        const bool last_of_cell = valid && lane < WAVE - 1 && c_next != c;
        if (last_of_cell) copy_emit(c, r, z, s, prev_c, next_c, out);
        carry_c = (u32)__builtin_amdgcn_readlane((int)c, WAVE - 1);       // NONE when the turn was not full: the span has ended
        carry_r = (u32)__builtin_amdgcn_readlane((int)r, WAVE - 1);
        carry_z = (u32)__builtin_amdgcn_readlane((int)z, WAVE - 1);
        carry_s = (u32)__builtin_amdgcn_readlane((int)s, WAVE - 1);
    }
    if (carry_c != NONE && lane == 0) copy_emit(carry_c, carry_r, carry_z, carry_s, prev_c, next_c, out);
    // the columns: bin k summed across the lanes, kept by lane k (a span has fewer than 2^32 rows: no sum wraps)
    u32 mine = 0;
#pragma unroll
    for (u32 k = 0; k < COPY_BINS; ++k) {
        const u32 t = wave_sum32(h[k][lane]);
        if ((u32)lane == k) mine = t;
    }
    if ((u32)lane < COPY_BINS && mine) atomicAdd(hist + lane, (u64)mine);
    tail = wave_sum64(tail);
    if (lane == 0 && tail) atomicAdd(hist + COPY_BINS, tail);
}

}  // namespace fastf
