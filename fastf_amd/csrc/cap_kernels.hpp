// cap_kernels.hpp — the two kernels of `fastF cap` (cap_cmds.c): every cell downsampled to at most N reads.  They sit between K1a
// (which leaves every record's cell index in the cell scratch and the hit counts of every 256-record unit) and K1b (which
// consumes one decision bit per CB hit and does not care how the bit was made):
//
//   cell_hits_kernel        cell scratch -> hits_per_cell[c - 1] = records whose CB is sampled cell c (E3 survivors, before xf)
//   cell_decisions_kernel   cell scratch + raw draws + per-cell thresholds -> the decision plane of fastf_dev_draw_bits:
//                           bit i = draws[i] < threshold[cell of the i-th hit]
#pragma once
#include "ranged_hist.hpp"

namespace fastf {

// where K1a left the cell indices: a plain array (run == 0) or the scratch slices of blocked runs (byte `off` of each run)
struct CellIn { const void* p; u32 run; u32 off; };

// ------------------------------------------------------------------------------------
// hits per cell
// ------------------------------------------------------------------------------------
// A ranged histogram (ranged_hist.hpp) over the cell scratch with one u32 counter per cell.  A wave takes one 256-record unit
// per turn; a lane reads four neighbouring entries with one load (the order inside a unit does not matter to a histogram).
// Index 0 = no hit.
// In the general form equal cells are aggregated inside the wave (a leader per distinct cell adds the population count of its
// ballot): one global atomic per distinct cell and 64 records.
// Measured on 200 M resident records (profiles/cap_notes): 25 000 cells in LDS 212 us (1.9 TB/s of scratch: bound
// by the LDS atomics, not by HBM); 50 000 cells in two ranges 394 us; the same 50 000 cells in the general form 9.85 ms — about
// 50 distinct cells per 64 records, bound by device-scope atomics.  Hence the ranges.
constexpr u32 CAP_LDS_CELLS = 32768, CAP_HITS_THREADS = 1024, CAP_LDS_RANGES = 8;

typedef u32 u32x2_t __attribute__((ext_vector_type(2)));
typedef u32 u32x4_t __attribute__((ext_vector_type(4)));

template <bool LDS>
__device__ __forceinline__ void cell_hits_add(u32 c, u32 n_cells, u32* __restrict__ s_cnt, u32* __restrict__ hits, int lane) {
    const bool hit = c - 1u < n_cells;                                     // (0: no hit; an index beyond the table is not counted)
    if constexpr (LDS) {
        const WaveHits h = wave_hits<false>(hit, c);
        if (!h.mask) return;
        if (h.one_bin) { if (lane == h.leader) atomicAdd(s_cnt + (h.bin - 1u), (u32)__popcll(h.mask)); }
        else if (hit) atomicAdd(s_cnt + (c - 1u), 1u);
    } else {
        u64 rem = __ballot(hit);
        while (rem) {                                                      // (uniform) one turn per distinct cell of the item
            const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)rem) - 1);
            const u32 c0 = (u32)__builtin_amdgcn_readlane((int)c, leader);
            const u64 m = __ballot(hit && c == c0);
            if (lane == leader) atomicAdd(hits + (c0 - 1u), (u32)__popcll(m));
            rem &= ~m;
        }
    }
}

struct CellHitsHist {
    typedef u32 word;
    static constexpr u32 WORDS = 1, BINS = CAP_LDS_CELLS, THREADS = CAP_HITS_THREADS;
    static constexpr u64 TURN = 1;                                          // (counted in units)
    CellIn in; bool c16; u64 n_recs, n; u32* __restrict__ hits;
    __device__ __forceinline__ void shift(u32 lo) { hits += lo; }
    template <bool LDS>
    __device__ __forceinline__ void turn(u64 u, u32 lo, u32 n_cells, u32* __restrict__ s_cnt, int lane) const {
        const unsigned char* const p = reinterpret_cast<const unsigned char*>(in.p);
        const unsigned char* const at = in.run ? p + u * in.run + in.off : p + u * BLK_RECS * (c16 ? 2u : 4u);
        const u64 first = u * BLK_RECS + 4u * (u32)lane;
        u32 c[4];
        // (a blocked run is whole even when its unit is not; the entries of records that do not exist are not defined)
        if (in.run || (u + 1) * BLK_RECS <= n_recs) {
            if (c16) {
                const u32x2_t v = ld_once<FASTF_NT_K1B != 0>(reinterpret_cast<const u32x2_t*>(at) + lane);
                c[0] = v.x & 0xFFFFu; c[1] = v.x >> 16; c[2] = v.y & 0xFFFFu; c[3] = v.y >> 16;
            } else {
                const u32x4_t v = ld_once<FASTF_NT_K1B != 0>(reinterpret_cast<const u32x4_t*>(at) + lane);
                c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
            }
        } else {
#pragma unroll
            for (u32 k = 0; k < 4; ++k) c[k] = first + k < n_recs ? get_cell(at, c16, 4u * (u32)lane + k) : 0u;
        }
#pragma unroll
        for (u32 k = 0; k < 4; ++k) cell_hits_add<LDS>(first + k < n_recs && c[k] ? c[k] - lo : 0u, n_cells, s_cnt, hits, lane);
    }
    __device__ __forceinline__ void flush(u32 i, u32 v) const { atomicAdd(hits + i, v); }
};

template <bool LDS>
__global__ __launch_bounds__(CAP_HITS_THREADS) void cell_hits_kernel(const CellIn in, bool c16, u64 n, u32 n_cells_all, u32* __restrict__ hits_all, u32 n_ranges) {
    extern __shared__ u32 s_cnt[];
    ranged_hist<LDS>(CellHitsHist{in, c16, n, (n + BLK_RECS - 1) / BLK_RECS, hits_all}, n_cells_all, n_ranges, s_cnt);
}

// ------------------------------------------------------------------------------------
// per-cell decisions
// ------------------------------------------------------------------------------------
// A wave takes one 256-record unit per turn, four items of 64 records in record order (lane l of item j = record 64 j + l
// of the unit), exactly as K1b walks it.  The hit rank of a record = the unit's base (tile_base of its K1a tile + the
// half_hits of the units in front of it inside the tile) + the hits in front of it inside the unit (ballot + mbcnt): the
// rank is the record's place in the draw stream AND its bit in the plane.
//   draws       read once, 4 bytes per hit: the hit lanes of an item read consecutive words
//   thresholds  u64[n_cells], 0 .. 2^32: a gather from L2 (a few hundred KB at most)
// A hit lane decides `draw < threshold`; the decisions are then brought from record order into rank order with ONE
// ds_permute per item (hit lanes go to lane = their rank inside the item, the others behind them: a permutation of the 64
// lanes), and the ballot of what arrives IS the item's run of bits.
//
// A unit's bits form one run of at most 256 bits at an arbitrary bit offset; its first and last 64-bit word are shared with
// the units next to it.  The words are completed by clearing the plane first (the caller: hipMemsetAsync over exactly
// (n_draws + 63) / 64 words) and OR-ing: the wave keeps the word it is filling in scalar registers and sends it to memory
// with one atomicOr when an item crosses into the next word and at the end of the unit — at most five per unit, two for a
// unit of up to 64 hits, none for a word that stayed zero.  Bytes moved per record: the scratch entry (2 or 4) + per hit
// 4 of draws + 1/8 of the memset + 1/8 (8 bytes per 64 bits) of read-modify-write at L2.  The alternative — a first pass that
// compacts the hit cells by rank (2-4 bytes per hit written and read back) and an elementwise ballot pass over them — moves
// 4 to 8 bytes more per hit and needs a buffer of H entries; it has no atomics.  Measured: 728 us for 200 M records with 90 M hits, 1307 us with 180 M hits
// over the same records — the time follows the hits (the draw load and the dependent threshold gather per hit, nothing of the
// next unit in flight), not the record stream and not the atomics.
// Ranks at or beyond n_draws (a caller's stream that is too short) get no bit: nothing is written beyond the plane.
__global__ __launch_bounds__(256) void cell_decisions_kernel(const CellIn in, bool c16, u64 n, const u64* __restrict__ tile_base,
                                                             const u32* __restrict__ half_hits, const u32* __restrict__ draws, u64 n_draws,
                                                             const u64* __restrict__ thresholds, u32 n_cells, u64* __restrict__ plane) {
    const int lane = lane_id();
    const u64 units = (n + BLK_RECS - 1) / BLK_RECS;
    const u64 waves = (u64)gridDim.x * (256 / WAVE);
    const unsigned char* const p = reinterpret_cast<const unsigned char*>(in.p);
    for (u64 u = (u64)blockIdx.x * (256 / WAVE) + (threadIdx.x >> 6); u < units; u += waves) {
        const u64 t = u >> 4; const u32 place = (u32)u & 15u;
        const u32 hh = half_hits[16ull * t + ((u32)lane & 15u)];
        u64 pos = uniform64(tile_base[t]) + row16_sum_lane15((u32)lane < place ? hh : 0u);     // rank of the unit's first hit
        const unsigned char* const at = in.run ? p + u * in.run + in.off : p + u * BLK_RECS * (c16 ? 2u : 4u);
        u32 c[4];
#pragma unroll
        for (u32 j = 0; j < 4; ++j) {
            const u32 o = j * WAVE + (u32)lane;
            const u32 v = u * BLK_RECS + o < n ? get_cell_once(at, c16, o) : 0u;
            c[j] = v - 1u < n_cells ? v : 0u;
        }
        u64 acc = 0, accw = pos >> 6;                                      // the word being filled, and which one it is (uniform)
        auto flush = [&]() { if (lane == 0 && acc) atomicOr(reinterpret_cast<unsigned long long*>(plane) + accw, (unsigned long long)acc); };
#pragma unroll
        for (u32 j = 0; j < 4; ++j) {
            const bool hit = c[j] != 0;
            const u64 hm = __ballot(hit);
            const u32 h = (u32)__popcll(hm);
            if (!h) continue;                                              // (uniform)
            const u32 rl = rank_below(hm);
            const u64 r = pos + rl;
            u32 keep = 0;
            if (hit && r < n_draws) keep = (u64)ld_once<FASTF_NT_K1B != 0>(draws + r) < thresholds[c[j] - 1u] ? 1u : 0u;
            const u32 dest = hit ? rl : h + (u32)lane - rl;                // record order -> rank order
            const u32 got = (u32)__builtin_amdgcn_ds_permute((int)(dest << 2), (int)keep);
            const u64 cw = __ballot(got != 0);                            // bit k = the decision of the item's k-th hit
            const u32 b = (u32)pos & 63u;
            acc |= cw << b;
            if (b + h >= 64u) { flush(); ++accw; acc = b ? cw >> (64u - b) : 0ull; }
            pos += h;
        }
        flush();
    }
}

}  // namespace fastf
