// fidelity_kernels.hpp — the kernel of --fidelity (resident.c): a grid point's matrix Y joined with the full-depth matrix X of the
// same (cell rate, seed) pair, reduced to two exact integers per cell.
//
//   fidelity_kernel   point rows and full rows, both ascending by (cell, feature), every point row with a partner among the full
//                     rows -> per cell sum_xy = sum of x * y over the point's rows and sum_yy = sum of y * y
//
// The same kernel on (X, X) gives sum_xx.  The sums of the counts and the rows with count >= 1 are cell_summary_kernel's.
#pragma once
#include "umi_kernels.hpp"

namespace fastf {

constexpr u64 ERR_NO_PARTNER = 32;                 // a point row whose (cell, feature) is not among the full rows
constexpr u32 FID_THREADS = 256;
constexpr u32 FID_BLOCKS_PER_CU = 4;               // 16 waves a CU: the join's turns are chains of cross-lane steps, more waves hide them

__device__ __forceinline__ u64 fid_key(const u32* __restrict__ cell, const u32* __restrict__ feature, u64 i) {
    return ((u64)cell[i] << 32) | (u64)feature[i];
}
__device__ __forceinline__ u64 fid_readlane64(u64 v, int l) {
    return ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(v >> 32), l) << 32) | (u64)(u32)__builtin_amdgcn_readlane((int)(u32)v, l);
}

// the first full row whose key is not below `key`, by the whole wave: 64 probes a step, evenly spread over what is left, so
// 2^32 rows take six steps.  Invariant: rows below lo have smaller keys, rows from hi on do not.  Every probe lies below m.
__device__ __forceinline__ u64 fid_lower_bound(const u32* __restrict__ xc, const u32* __restrict__ xf, u64 m, u64 key, int lane) {
    u64 lo = 0, hi = m;
    while (lo < hi) {                                                      // (uniform)
        const u64 step = (hi - lo + 63) >> 6;
        const u64 i = lo + (u64)lane * step;
        const bool below = i < hi && fid_key(xc, xf, i) < key;
        const u32 cnt = (u32)__popcll(__ballot(below));
        if (!cnt) { hi = lo; break; }
        const u64 top = lo + (u64)cnt * step;
        lo += (u64)(cnt - 1) * step + 1;
        if (top < hi) hi = top;
    }
    return lo;
}

// One turn of the join's walk (see fidelity_kernel): the partner's count of this lane's `key` into x and found = true; the chunk
// state (cur, ckey, ccnt, have) goes on to the turn behind.  last_key: the largest key of the turn (uniform).
__device__ __forceinline__ void fid_partner(const u32* __restrict__ xf, const u32* __restrict__ xc, const u32* __restrict__ xk, u64 m, u64 key, u64 last_key,
                                            int lane, u64& cur, u64& ckey, u32& ccnt, bool& have, u32& x, bool& found) {
    constexpr u64 KEY_END = ~0ull;                                         // above every key of a row
    for (;;) {                                                             // (uniform)
        if (!have) {
            const u64 j = cur + (u64)lane;
            const bool in = j < m;
            ckey = in ? fid_key(xc, xf, j) : KEY_END;
            ccnt = in ? xk[j] : 0u;
            have = true;
        }
        int pos = 0;                                                       // the chunk lanes below `pos` hold keys below mine
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const u64 kk = __shfl(ckey, pos + s - 1, WAVE);
            if (kk < key) pos += s;
        }
        const u64 kk = __shfl(ckey, pos, WAVE);
        const u32 xx = __shfl(ccnt, pos, WAVE);
        if (!found && kk == key) { x = xx; found = true; }
        const u64 chunk_last = fid_readlane64(ckey, WAVE - 1);
        if (chunk_last >= last_key) break;                                 // every key of the turn has met its place
        cur += WAVE; have = false;
    }
}

__device__ __forceinline__ void fid_emit(u32 c, u64 xy, u64 yy, u32 prev_c, u32 next_c, u32 n_cells, u64* __restrict__ sum_xy, u64* __restrict__ sum_yy) {
    if (c - 1u >= n_cells) return;                                         // (a cell index the caller did not size the arrays for: nothing is written)
    if (c == prev_c || c == next_c) { atomicAdd(sum_xy + (c - 1u), xy); atomicAdd(sum_yy + (c - 1u), yy); }
    else { sum_xy[c - 1u] = xy; sum_yy[c - 1u] = yy; }
}

// xf / xc / xk: the full rows, *m_ptr of them; yf / yc / yk: the point rows, *n_ptr of them; both ascending by the key
// cell << 32 | feature, cells 1-based and below 2^32 - 1.  The caller has cleared sum_xy[0 .. n_cells) and sum_yy[0 .. n_cells).
//
// The span, the segmented scan without head flags, the carried cell and the plain store of a cell that ends inside the span are
// cell_summary_kernel's (sweep_kernels.hpp), with two u64 in the scan.
//
// The join.  The point rows are a subset of the full rows in the same order, so the partners of a span lie in one window of the
// full rows, and that window is walked once, forwards.  One cooperative search (fid_lower_bound) places the span's first key.
// From there the wave holds one chunk of 64 consecutive full rows in registers, a row a lane, loaded coalesced.  A point lane
// finds its key among the chunk's 64 by a lower bound over the lanes — six cross-lane reads of the key and one for the equality
// test — and takes the partner's count by one more.  While the turn's last key is above the chunk's last, the next chunk is
// loaded; a turn that ends inside a chunk leaves it in place for the turn behind it.  Every full row of the window is so read
// once, by one coalesced load, whatever the ratio of the two row counts; nothing is searched in memory after the first key.
// Lanes of a chunk beyond the last full row hold the largest key, which ends every walk: no row from *m_ptr on is read.
// A point lane that has met a chunk whose last key is not below its own and found no partner raises ERR_NO_PARTNER; its row
// then counts with x = 0.
__global__ __launch_bounds__(FID_THREADS) void fidelity_kernel(const u32* __restrict__ xf, const u32* __restrict__ xc, const u32* __restrict__ xk,
                                                               const u64* __restrict__ m_ptr, const u32* __restrict__ yf, const u32* __restrict__ yc,
                                                               const u32* __restrict__ yk, const u64* __restrict__ n_ptr, u32 n_cells,
                                                               u64* __restrict__ sum_xy, u64* __restrict__ sum_yy, u64* __restrict__ err) {
    const int lane = lane_id();
    const u64 n = *n_ptr, m = *m_ptr;
    const u64 waves = (u64)gridDim.x * (FID_THREADS / WAVE), w = (u64)blockIdx.x * (FID_THREADS / WAVE) + (threadIdx.x >> 6);
    const u64 span = (((n + waves - 1) / waves) + 63) & ~63ull;
    const u64 a = w * span;
    if (a >= n) return;                                                    // (uniform per wave)
    const u64 b = a + span < n ? a + span : n;
    constexpr u32 NONE = 0xFFFFFFFFu;                                      // no cell: indices are 1-based and below 2^32 - 1
    constexpr u64 KEY_END = ~0ull;                                         // above every key of a row
    const u32 prev_c = a > 0 ? yc[a - 1] : NONE, next_c = b < n ? yc[b] : NONE;
    // the chunk in registers: full rows cur + lane, cur a multiple of 64 (rows below the span's first partner only have smaller keys)
    u64 cur = fid_lower_bound(xc, xf, m, fid_key(yc, yf, a), lane) & ~63ull;
    u64 ckey = KEY_END; u32 ccnt = 0;
    bool have = false;
    u32 carry_c = NONE; u64 carry_xy = 0, carry_yy = 0;
    bool missing = false;
    for (u64 base = a; base < b; base += WAVE) {
        const u64 i = base + (u64)lane;
        const bool valid = i < b;
        const u32 c = valid ? ld_once<FASTF_NT_K3 != 0>(yc + i) : NONE;
        const u32 f = valid ? ld_once<FASTF_NT_K3 != 0>(yf + i) : NONE;
        const u32 y = valid ? ld_once<FASTF_NT_K3 != 0>(yk + i) : 0u;
        const u64 key = ((u64)c << 32) | (u64)f;                           // (an invalid lane: KEY_END)
        const int n_valid = (int)(b - base < (u64)WAVE ? b - base : (u64)WAVE);
        const u64 last_key = fid_readlane64(key, n_valid - 1);             // the largest key of the turn (uniform)
        u32 x = 0; bool found = !valid;
        fid_partner(xf, xc, xk, m, key, last_key, lane, cur, ckey, ccnt, have, x, found);
        missing |= !found;
        u64 xy = (u64)x * (u64)y, yy = (u64)y * (u64)y;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const u32 co = __shfl_up(c, o, WAVE); const u64 xyo = __shfl_up(xy, o, WAVE); const u64 yyo = __shfl_up(yy, o, WAVE);
            if (lane >= o && co == c) { xy += xyo; yy += yyo; }
        }
        const u32 c_next = __shfl_down(c, 1, WAVE);
        // the cell carried in from the turn before: it goes on in this turn's first lanes, or it has ended
        const u32 first_c = (u32)__builtin_amdgcn_readfirstlane((int)c);
        if (carry_c != NONE) {
            if (carry_c == first_c) { if (c == carry_c) { xy += carry_xy; yy += carry_yy; } }
            else if (lane == 0) fid_emit(carry_c, carry_xy, carry_yy, prev_c, next_c, n_cells, sum_xy, sum_yy);
        }
        // lane 63's cell may go on in the next turn: it is carried, not written
        const bool last_of_cell = valid && lane < WAVE - 1 && c_next != c;
        if (last_of_cell) fid_emit(c, xy, yy, prev_c, next_c, n_cells, sum_xy, sum_yy);
        carry_c = (u32)__builtin_amdgcn_readlane((int)c, WAVE - 1);       // NONE when the turn was not full: the span has ended
        carry_xy = fid_readlane64(xy, WAVE - 1);
        carry_yy = fid_readlane64(yy, WAVE - 1);
    }
    if (carry_c != NONE && lane == 0) fid_emit(carry_c, carry_xy, carry_yy, prev_c, next_c, n_cells, sum_xy, sum_yy);
    if (__ballot(missing) && lane == 0) atomicOr(err, ERR_NO_PARTNER);
}

}  // namespace fastf
