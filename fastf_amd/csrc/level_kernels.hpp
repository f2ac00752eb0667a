// level_kernels.hpp — the kernel of `fastF level` (level_cmds.c): every cell downsampled to at most M UMIs.  The search for the
// per-cell thresholds runs the kernels that are there (cell_decisions_kernel, K1b, sort, reduce, cell_summary_kernel) once per
// pass; this kernel sits behind cell_summary_kernel and turns one pass's UMIs per cell into the next pass's thresholds:
//
//   level_step_kernel<true>    U_k(2^32) and M -> the state (lo, hi) of every cell, the first probes, cells_capped
//   level_step_kernel<false>   U_k(probe) and M -> the state moved, the next probes, the cells still open
//
// State of cell k (u64 each, 0 .. 2^32): U_k(lo) <= M < U_k(hi) for a capped cell, lo = hi = 2^32 for a cell that loses no read.
// A cell is open while hi - lo > 1; its probe is (lo + hi) / 2; every other cell's probe is 0 — its reads drop out of K1b's
// output, so a pass sorts the open cells' keys alone.  U_k is a non-decreasing step function of the threshold (the kept sets of
// a cell are nested), hence bisection; hi - lo halves per step from 2^32: no cell is open after 32 steps.
#pragma once
#include "umi_kernels.hpp"

namespace fastf {

constexpr u32 LEVEL_THREADS = 256;
constexpr u64 LEVEL_FULL = 1ull << 32;
// the result block of a step (u64 words): cells still open, cells capped (written by the initialising form alone), the error
// bits the step found, and whether it held the state because of them
enum { LEVEL_OPEN = 0, LEVEL_CAPPED = 1, LEVEL_BITS = 2, LEVEL_HELD = 3, LEVEL_OUT_WORDS = 4 };

// One lane per cell: 8 bytes of U read, 16 bytes of state read and written, 8 bytes of probe written — a few hundred KB for
// the largest barcode lists, one launch of a few microseconds.  The counts go through the wave (ballot + popcount) and one
// atomic per wave that has something to add.
// err_a / err_b (either may be nullptr): error words of the pass whose U this step would consume — the engine's and K1b's.
// They are read in stream order behind the kernels that raise them.  If any bit is set, the pass's U is not to be trusted: the
// step leaves lo, hi and the probes as they are, reports the bits and LEVEL_HELD = 1, and the host decides (a run that was too
// long for the group-only sort is sorted fully and stepped again; anything else ends the run).  This is what lets a pass end
// in ONE small device-to-host copy: the host needs no look at the error bits before the step is launched.
// out[LEVEL_OPEN] (and out[LEVEL_CAPPED] in the initialising form) are zeroed by the caller before the launch.
template <bool INIT>
__global__ __launch_bounds__(LEVEL_THREADS) void level_step_kernel(const u64* __restrict__ umis, u32 n_cells, u64 cap, u64* __restrict__ lo,
                                                                   u64* __restrict__ hi, u64* __restrict__ probe, u64* __restrict__ out,
                                                                   const u64* __restrict__ err_a, const u64* __restrict__ err_b) {
    const u32 k = blockIdx.x * LEVEL_THREADS + threadIdx.x;
    const u64 bits = (err_a ? *err_a : 0ull) | (err_b ? *err_b : 0ull);    // (uniform)
    if (k == 0) { out[LEVEL_BITS] = bits; out[LEVEL_HELD] = bits ? 1ull : 0ull; }
    if (bits) return;
    bool open = false, capped = false;
    if (k < n_cells) {
        const u64 u = umis[k];
        u64 l, h;
        if constexpr (INIT) {
            capped = u > cap;
            l = capped ? 0ull : LEVEL_FULL; h = LEVEL_FULL;
        } else {
            l = lo[k]; h = hi[k];
            if (h - l > 1) {                                               // u = U_k((l + h) / 2): the probe of the step before
                const u64 mid = (l + h) >> 1;
                if (u <= cap) l = mid; else h = mid;
            }
        }
        open = h - l > 1;
        lo[k] = l; hi[k] = h;
        probe[k] = open ? (l + h) >> 1 : 0ull;
    }
    const u64 om = __ballot(open);
    if (lane_id() == 0 && om) atomicAdd(out + LEVEL_OPEN, (u64)__popcll(om));
    if constexpr (INIT) {
        const u64 cm = __ballot(capped);
        if (lane_id() == 0 && cm) atomicAdd(out + LEVEL_CAPPED, (u64)__popcll(cm));
    }
}

}  // namespace fastf
