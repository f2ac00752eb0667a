// coexpr_kernels.hpp — the kernels of --coexpression (resident.c): the co-expression partners of every gene of A, the highly variable
// genes of the (cell rate, seed) pair, at full depth and at a grid point (the definition: include/fastf_amd.h).  Three stages, each
// leaving its result in device memory:
//
//   coex_planes_kernel     rows (cell, feature, count) + the slot map -> P GENE-MAJOR byte planes of K_pad x n_pad: plane p holds bits
//                          7p .. 7p+6 of the count of (slot, cell); the planes were zeroed first.  nbr_planes_kernel with the axes exchanged
//   coex_gram_kernel       the planes -> D_gh = sum_i m_ig m_ih, u64[K x K], dense; the planes are both operands and the reduction runs
//                          over the cells.  Two forms of the dot products: the i8 MFMA and ordinary integer instructions
//   coex_sums_kernel       the planes -> S_g = sum_i m_ig (u64[K])
//   coex_var_kernel        D, S, n -> V_h = n D_hh - S_h^2 (u64[K]) and the largest D_hh
//   coex_select_kernel     D, S, V, n, k -> the partner sets: ONE THREAD per gene walks the slots in ascending order (coex_walk); no lane
//                          talks to another
//
// The part above the HIP guard is plain C++: tools/coex_host.cpp compiles the per-gene walk, the digit recombination and the address of
// a plane byte with g++, and tests/test_coexpr_kernels_host.py checks them against the definition on the CPU.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "coexpr_order.h"

namespace fastf {

constexpr uint32_t COEX_TILE = 32;                                   // genes of a tile of D; K_pad is a multiple of it
constexpr uint32_t COEX_KSTEP = 32;                                  // cells of one 32x32x32 i8 MFMA: a chunk is a multiple of it
constexpr uint32_t COEX_CHUNK = 8192;                                // the cells a wave reduces before it adds into D (FASTF_COEXPR_CHUNK lowers it)
constexpr uint32_t COEX_CHUNK_MAX = 44352;                           // 3 * chunk * 127^2 < 2^31: the i32 accumulator of three digit products
constexpr uint32_t COEX_MAX_K = 64, COEX_MAX_PLANES = 3, COEX_MAX_GENES = 4096;
constexpr uint32_t COEX_NONE = 0xFFFFFFFFu;
static_assert(3ull * COEX_CHUNK_MAX * 127 * 127 < (1ull << 31) && COEX_CHUNK <= 32768 && COEX_CHUNK % COEX_KSTEP == 0, "the accumulator bound of a chunk");

// the padded shape of the planes for a chunk of `chunk` cells (a multiple of 32): K_pad rows, n_pad bytes a row — n_cells rounded up
// to 32, then to a multiple of the chunk in effect, which is never longer than the rounded cells
COEX_FN void coex_pad(uint32_t n_cells, uint32_t K, uint32_t chunk, uint32_t* K_pad, uint32_t* n_pad, uint32_t* chunk_eff) {
    const uint64_t n32 = n_cells ? ((uint64_t)n_cells + 31u) & ~(uint64_t)31u : 32u;
    const uint64_t c = chunk < n32 ? chunk : n32;
    *K_pad = K ? (K + COEX_TILE - 1) / COEX_TILE * COEX_TILE : COEX_TILE;
    *n_pad = (uint32_t)((n32 + c - 1) / c * c);
    *chunk_eff = (uint32_t)c;
}

// the byte of (plane p, slot, 0-based cell) in the planes, and its value for a count
COEX_FN uint64_t coex_plane_at(uint32_t p, uint32_t slot, uint32_t cell, uint32_t K_pad, uint32_t n_pad) {
    return ((uint64_t)p * K_pad + slot) * n_pad + cell;
}
COEX_FN unsigned char coex_digit(uint32_t count, uint32_t p) { return (unsigned char)((count >> (7u * p)) & 127u); }

// sum_t 2^(7t) acc_t: the T = 2P - 1 accumulators of one entry of D (non-negative i32, read as u32) -> its share of D_gh
COEX_FN uint64_t coex_recombine(const int32_t* acc, int T) {
    uint64_t d = 0;
    for (int t = 0; t < T; ++t) d += (uint64_t)(uint32_t)acc[t] << (7 * t);
    return d;
}

// The partners of gene g.  D: u64[K x K], read as D[h * K + g] (D is symmetric: threads of neighbouring g read neighbouring words);
// S, V: u64[K].  The slots h = 0 .. K - 1 are walked in ascending order; a candidate (h != g, c_gh > 0) goes into a free slot, and
// into a full list only in place of its worst entry and only when it strictly precedes that entry — every entry has a lower slot, so
// a tie stays with the entry, which is the slot rule.  The worst entry is found again after every change of a full list.  The k list
// slots of the caller: sc[s * stride] (c) and si[s * stride] (the slot h).  At the end si[0 .. cnt) ascends; returns cnt.
COEX_FN uint32_t coex_walk(const uint64_t* D, const uint64_t* S, const uint64_t* V, uint32_t n, uint32_t K, uint32_t k, uint32_t g,
                           uint64_t* sc, uint32_t* si, uint32_t stride) {
    uint32_t cnt = 0, ws = 0, wi = 0;
    uint64_t wc = 0, wv = 0;                                          // the worst of a full list: its list slot, gene slot, c, V
    const uint64_t Sg = S[g];
    for (uint32_t h = 0; h < K; ++h) {
        if (h == g) continue;
        const __int128 c128 = coex_cov(n, D[(size_t)h * K + g], Sg, S[h]);
        if (c128 <= 0) continue;
        const uint64_t c = (uint64_t)c128;
        bool changed = false;
        if (cnt < k) { sc[(size_t)cnt * stride] = c; si[(size_t)cnt * stride] = h; ++cnt; changed = cnt == k; }
        else if (coex_precedes(c, V[h], h, wc, wv, wi)) { sc[(size_t)ws * stride] = c; si[(size_t)ws * stride] = h; changed = true; }
        if (changed) {                                                // the list is full: its worst entry
            ws = 0; wc = sc[0]; wi = si[0]; wv = V[wi];
            for (uint32_t s = 1; s < k; ++s) {
                const uint64_t cs = sc[(size_t)s * stride]; const uint32_t is = si[(size_t)s * stride]; const uint64_t vs = V[is];
                if (coex_precedes(wc, wv, wi, cs, vs, is)) { ws = s; wc = cs; wi = is; wv = vs; }
            }
        }
    }
    for (uint32_t s = 1; s < cnt; ++s) {                              // by ascending slot (insertion sort of at most 64 entries)
        const uint32_t v = si[(size_t)s * stride];
        uint32_t t = s;
        for (; t > 0 && si[(size_t)(t - 1) * stride] > v; --t) si[(size_t)t * stride] = si[(size_t)(t - 1) * stride];
        si[(size_t)t * stride] = v;
    }
    return cnt;
}

}  // namespace fastf

#ifdef __HIPCC__
#include "neighbors_kernels.hpp"

namespace fastf {

constexpr u32 COEX_WAVES = 4, COEX_THREADS = COEX_WAVES * WAVE;
constexpr u32 COEX_SEL_THREADS = 64;                                  // genes of a workgroup of the selection: k * 64 * 12 bytes of LDS
__host__ __device__ constexpr u32 coex_select_lds(u32 k) { return k * COEX_SEL_THREADS * (u32)(sizeof(u64) + sizeof(u32)); }

// One byte store per plane and row whose gene is in A; (cell, feature) pairs are distinct, so no two rows write one byte.  A row whose
// cell is outside 1 .. n_cells, whose feature is outside 1 .. n_features or whose slot is beyond K writes nothing.
__global__ __launch_bounds__(256) void coex_planes_kernel(const u32* __restrict__ feature, const u32* __restrict__ cell, const u32* __restrict__ count,
                                                          const u64* __restrict__ n_ptr, const unsigned short* __restrict__ slot_map, u32 n_features,
                                                          u32 n_cells, u32 K, u32 K_pad, u32 n_pad, u32 P, unsigned char* __restrict__ planes) {
    const u64 n = *n_ptr;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) {
        const u32 slot = nbr_slot_of(slot_map, feature[i], n_features), c = cell[i] - 1u, v = count[i];
        if (slot >= K || c >= n_cells) continue;
        for (u32 p = 0; p < P; ++p) planes[coex_plane_at(p, slot, c, K_pad, n_pad)] = coex_digit(v, p);
    }
}

// One wave per gene over its row of the planes (n32: the cells rounded up to 32; the bytes behind n_cells are zero).
__global__ __launch_bounds__(256) void coex_sums_kernel(const unsigned char* __restrict__ planes, u32 K, u32 K_pad, u32 n_pad, u32 n32, u32 P,
                                                        u64* __restrict__ S) {
    const int lane = lane_id();
    const u32 waves = gridDim.x * (256 / WAVE);
    const u64 plane_words = (u64)K_pad * n_pad / 4;
    for (u32 g = blockIdx.x * (256 / WAVE) + (threadIdx.x >> 6); g < K; g += waves) {
        const u32* const row = reinterpret_cast<const u32*>(planes + (u64)g * n_pad);
        u64 sum = 0;
        for (u32 w = lane; w < n32 / 4; w += WAVE) {
            u32 d[COEX_MAX_PLANES] = {0, 0, 0};
            for (u32 p = 0; p < P; ++p) d[p] = row[p * plane_words + w];
#pragma unroll
            for (u32 b = 0; b < 4; ++b)
                sum += (u64)((d[0] >> (8 * b)) & 127u) | (u64)((d[1] >> (8 * b)) & 127u) << 7 | (u64)((d[2] >> (8 * b)) & 127u) << 14;
        }
        sum = wave_sum64(sum);
        if (lane == 0) S[g] = sum;
    }
}

// A wave owns one 32 x 32 tile (gt, ht), gt <= ht, of D for one chunk of cells: work item = chunk * n_pairs + pair, four items a
// workgroup; the waves never wait for each other.  One i32 accumulator tile per digit sum a + b, as in nbr_gram_kernel, and the same
// register map: lane l ends with column h = 32 ht + (l & 31) and the rows g = 32 gt + (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).
//   MFMA:  A = the rows of gt, B = the rows of ht, both read as 16 bytes at [row l & 31][cell s + 16 (l >> 5)] for step s.
//   plain: the lane's row h against its 16 rows g, 16 bytes a load, v_dot4 or shifts and multiplies.
// A chunk ends at n32 at the latest (the bytes behind it are zero).  At its end d = sum_t 2^(7t) acc_t is added into D[g][h] and, off
// the diagonal tiles, D[h][g] with 64-bit integer atomics (exact in any order; D was zeroed first); g and h from K on add nothing.
template <int P, bool MFMA>
__global__ __launch_bounds__(COEX_THREADS) void coex_gram_kernel(const unsigned char* __restrict__ planes, u32 K, u32 K_pad, u32 n_pad, u32 n32,
                                                                 u32 chunk, u32 n_tiles, u64 n_pairs, u64 n_items, u64* __restrict__ D) {
    constexpr int T = 2 * P - 1;
    const int lane = lane_id(), w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u64 item = (u64)blockIdx.x * COEX_WAVES + (u32)w;
    if (item >= n_items) return;                                           // (uniform per wave; the kernel has no workgroup barrier)
    u64 pair = item % n_pairs;
    const u32 ck = (u32)(item / n_pairs);
    u32 gt = 0;
    while (pair >= n_tiles - gt) { pair -= n_tiles - gt; ++gt; }           // row gt of the upper triangle has n_tiles - gt tiles
    const u32 ht = gt + (u32)pair;
    const u32 c0 = ck * chunk, c1 = c0 + chunk < n32 ? c0 + chunk : n32;
    const u64 plane_bytes = (u64)K_pad * n_pad;
    const u32 r = (u32)lane & 31u, hf = (u32)lane >> 5;

    nbr_v16i acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0;
    if constexpr (MFMA) {
        const unsigned char* const pa = planes + (u64)(gt * COEX_TILE + r) * n_pad + 16u * hf;
        const unsigned char* const pb = planes + (u64)(ht * COEX_TILE + r) * n_pad + 16u * hf;
        for (u32 s = c0; s < c1; s += COEX_KSTEP) {
            nbr_v4i a[P], b[P];
#pragma unroll
            for (int p = 0; p < P; ++p) {
                a[p] = *reinterpret_cast<const nbr_v4i*>(pa + p * plane_bytes + s);
                b[p] = *reinterpret_cast<const nbr_v4i*>(pb + p * plane_bytes + s);
            }
#pragma unroll
            for (int x = 0; x < P; ++x)
#pragma unroll
                for (int y = 0; y < P; ++y) acc[x + y] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[x], b[y], acc[x + y], 0, 0, 0);
        }
    } else {
        const unsigned char* const pb = planes + (u64)(ht * COEX_TILE + r) * n_pad;
        for (u32 s = c0; s < c1; s += 16) {
            uint4 b[P];
#pragma unroll
            for (int p = 0; p < P; ++p) b[p] = *reinterpret_cast<const uint4*>(pb + p * plane_bytes + s);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const u32 row = gt * COEX_TILE + (u32)(e & 3) + 8u * (u32)(e >> 2) + 4u * hf;
#pragma unroll
                for (int x = 0; x < P; ++x) {
                    const uint4 a = *reinterpret_cast<const uint4*>(planes + x * plane_bytes + (u64)row * n_pad + s);
#pragma unroll
                    for (int y = 0; y < P; ++y) acc[x + y][e] += (int)nbr_dot16(a, b[y]);
                }
            }
        }
    }
    const u32 h = ht * COEX_TILE + r;
    if (h >= K) return;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const u32 g = gt * COEX_TILE + (u32)(e & 3) + 8u * (u32)(e >> 2) + 4u * hf;
        int32_t a[T];
#pragma unroll
        for (int t = 0; t < T; ++t) a[t] = acc[t][e];
        const u64 d = coex_recombine(a, T);
        if (g >= K || d == 0) continue;
        atomicAdd(reinterpret_cast<unsigned long long*>(D + (u64)g * K + h), (unsigned long long)d);
        if (gt != ht) atomicAdd(reinterpret_cast<unsigned long long*>(D + (u64)h * K + g), (unsigned long long)d);
    }
}

// V_h = n D_hh - S_h^2 (exact below the range rule, which the caller checks on *max_q before it selects); *max_q was cleared first
__global__ __launch_bounds__(256) void coex_var_kernel(const u64* __restrict__ D, const u64* __restrict__ S, u32 n, u32 K, u64* __restrict__ V,
                                                       u64* __restrict__ max_q) {
    const u32 h = blockIdx.x * 256 + threadIdx.x;
    if (h >= K) return;
    const u64 q = D[(u64)h * K + h], s = S[h];
    V[h] = (u64)((unsigned __int128)n * q - (unsigned __int128)s * s);
    if (q) atomicMax(reinterpret_cast<unsigned long long*>(max_q), (unsigned long long)q);
}

// One thread per gene: coex_walk on its own k slots of the workgroup's LDS (slot s of thread t at [s * 64 + t]), then idx_out[g * k + s],
// s < cnt_out[g], ascending; the other slots of the row get COEX_NONE.  Dynamic LDS: coex_select_lds(k) bytes.
__global__ __launch_bounds__(COEX_SEL_THREADS) void coex_select_kernel(const u64* __restrict__ D, const u64* __restrict__ S, const u64* __restrict__ V,
                                                                      u32 n, u32 K, u32 k, u32* __restrict__ idx_out, u32* __restrict__ cnt_out) {
    extern __shared__ u64 s_coex[];
    const u32 g = blockIdx.x * COEX_SEL_THREADS + threadIdx.x;
    if (g >= K) return;                                                    // (the kernel has no barrier)
    u64* const sc = s_coex + threadIdx.x;
    u32* const si = reinterpret_cast<u32*>(s_coex + (size_t)k * COEX_SEL_THREADS) + threadIdx.x;
    const u32 cnt = coex_walk(reinterpret_cast<const uint64_t*>(D), reinterpret_cast<const uint64_t*>(S), reinterpret_cast<const uint64_t*>(V), n, K, k, g,
                              reinterpret_cast<uint64_t*>(sc), si, COEX_SEL_THREADS);
    for (u32 s = 0; s < k; ++s) idx_out[(u64)g * k + s] = s < cnt ? si[(size_t)s * COEX_SEL_THREADS] : COEX_NONE;
    cnt_out[g] = cnt;
}

}  // namespace fastf
#endif
