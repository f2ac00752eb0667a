// neighbors_kernels.hpp — the kernels of --neighbors (resident.c): the k nearest neighbours of every sampled cell by the cosine of its
// raw counts over the highly variable genes A of the (cell rate, seed) pair, at full depth and at a grid point.
//
//   nbr_max_count_kernel   rows (feature, count) + the slot map of A -> the largest count of a row whose gene is in A
//   nbr_planes_kernel      sorted rows (cell, feature, count) + the slot map -> P byte planes of n_pad x K_pad: plane p holds bits
//                          7p .. 7p+6 of the count of (cell, slot); the planes were zeroed first
//   nbr_norms_kernel       the planes -> norms[i] = v_i . v_i (u64) and their maximum
//   nbr_gram_kernel        the planes and the norms -> per query row the first k cells j != i with d_ij > 0 by descending cosine,
//                          decided in 128-bit integers; n x n is never stored.  Two forms of the dot products: the i8 MFMA and
//                          ordinary integer instructions
//   nbr_shared_kernel      two index sets (ascending within a row) -> per cell the number of common neighbours
//
// Everything is integer and exact: a count c is the digits c = sum_p 2^(7p) c_p with 0 <= c_p < 128, a dot product is
// d_ij = sum_{a,b} 2^(7(a+b)) s_ab with s_ab = sum_g c_a(i,g) c_b(j,g).  The digits are non-negative i8, every s_ab is at most
// K_pad * 127^2, and the up to three s_ab with the same a + b share one i32 accumulator: 3 * 2048 * 127^2 < 2^27.
#pragma once
#include "umi_kernels.hpp"

namespace fastf {

constexpr u32 NBR_KSTEP = 32;                                   // K of one 32x32x32 i8 MFMA: K_pad is a multiple of it
constexpr u32 NBR_TILE = 32;                                    // query rows of a wave, columns of a column tile
constexpr u32 NBR_WAVES = 4, NBR_THREADS = NBR_WAVES * WAVE;
constexpr u32 NBR_ROWS = NBR_WAVES * NBR_TILE;                  // query rows of a workgroup: n_pad is a multiple of it
constexpr u32 NBR_MAX_K = 64, NBR_MAX_PLANES = 3, NBR_MAX_GENES = 4096;
constexpr u32 NBR_NO_SLOT = 0xFFFFu, NBR_NONE = 0xFFFFFFFFu;
constexpr u32 NBR_TILE_PITCH = NBR_TILE + 1;                    // u64 words per row of the LDS tile (no bank conflicts down a column)
// LDS words (u64) of one wave: the 32 x 32 tile of dot products, k slots of d (u64) and of the cell index (u32) per query row
__host__ __device__ constexpr u32 nbr_wave_words(u32 k) { return NBR_TILE * NBR_TILE_PITCH + k * NBR_TILE + k * NBR_TILE / 2; }

typedef int nbr_v4i __attribute__((ext_vector_type(4)));
typedef int nbr_v16i __attribute__((ext_vector_type(16)));
typedef unsigned __int128 nbr_u128;

__device__ __forceinline__ u32 nbr_slot_of(const unsigned short* __restrict__ slot_map, u32 f, u32 n_features) {
    return f - 1u < n_features ? (u32)slot_map[f] : NBR_NO_SLOT;           // (feature 0 wraps beyond every list)
}

// feature[i], count[i]; *n_ptr rows.  *max_out was cleared by the caller.
__global__ __launch_bounds__(256) void nbr_max_count_kernel(const u32* __restrict__ feature, const u32* __restrict__ count, const u64* __restrict__ n_ptr,
                                                            const unsigned short* __restrict__ slot_map, u32 n_features, u32* __restrict__ max_out) {
    const u64 n = *n_ptr;
    u32 m = 0;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) {
        const u32 c = count[i];
        if (nbr_slot_of(slot_map, feature[i], n_features) != NBR_NO_SLOT && c > m) m = c;
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) { const u32 o = (u32)__shfl_xor((int)m, off); m = o > m ? o : m; }
    if (lane_id() == 0 && m) atomicMax(max_out, m);
}

// One byte store per plane and row whose gene is in A; (cell, feature) pairs are distinct, so no two rows write one byte.  A row whose
// cell is outside 1 .. n_cells, whose feature is outside 1 .. n_features or whose slot is beyond K writes nothing.
__global__ __launch_bounds__(256) void nbr_planes_kernel(const u32* __restrict__ feature, const u32* __restrict__ cell, const u32* __restrict__ count,
                                                         const u64* __restrict__ n_ptr, const unsigned short* __restrict__ slot_map, u32 n_features,
                                                         u32 n_cells, u32 K, u32 n_pad, u32 K_pad, u32 P, unsigned char* __restrict__ planes) {
    const u64 n = *n_ptr, plane_bytes = (u64)n_pad * K_pad;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) {
        const u32 slot = nbr_slot_of(slot_map, feature[i], n_features), c = cell[i] - 1u, v = count[i];
        if (slot >= K || c >= n_cells) continue;
        unsigned char* const at = planes + (u64)c * K_pad + slot;
        for (u32 p = 0; p < P; ++p) at[p * plane_bytes] = (unsigned char)((v >> (7u * p)) & 127u);
    }
}

// One wave per row.  *max_out was cleared by the caller.  norms == nullptr: the maximum alone (mapping_kernels.hpp).
__global__ __launch_bounds__(256) void nbr_norms_kernel(const unsigned char* __restrict__ planes, u32 n, u32 n_pad, u32 K_pad, u32 P,
                                                        u64* __restrict__ norms, u64* __restrict__ max_out) {
    const int lane = lane_id();
    const u32 waves = gridDim.x * (256 / WAVE);
    const u64 plane_bytes = (u64)n_pad * K_pad;
    for (u32 i = blockIdx.x * (256 / WAVE) + (threadIdx.x >> 6); i < n; i += waves) {
        const u32* const row = reinterpret_cast<const u32*>(planes + (u64)i * K_pad);
        u64 sum = 0;
        for (u32 w = lane; w < K_pad / 4; w += WAVE) {
            u32 d[NBR_MAX_PLANES] = {0, 0, 0};
            for (u32 p = 0; p < P; ++p) d[p] = row[p * (plane_bytes / 4) + w];
#pragma unroll
            for (u32 b = 0; b < 4; ++b) {
                const u64 v = (u64)((d[0] >> (8 * b)) & 127u) | (u64)((d[1] >> (8 * b)) & 127u) << 7 | (u64)((d[2] >> (8 * b)) & 127u) << 14;
                sum += v * v;
            }
        }
        sum = wave_sum64(sum);
        if (lane == 0) { if (norms) norms[i] = sum; if (sum) atomicMax(reinterpret_cast<unsigned long long*>(max_out), (unsigned long long)sum); }
    }
}

// j precedes l in the order of query row i: by descending cosine d / sqrt(n_i n), ties by ascending cell index.  n_i cancels:
// d_j^2 n_l > d_l^2 n_j.  d <= 2^42 and n < 2^42 (the host refuses a pair beyond), so both products stay below 2^126.
__device__ __forceinline__ bool nbr_precedes(u64 dj, u64 nj, u32 j, u64 dl, u64 nl, u32 l) {
    const nbr_u128 a = (nbr_u128)dj * dj * nl, b = (nbr_u128)dl * dl * nj;
    return a > b || (a == b && j < l);
}

__device__ __forceinline__ u32 nbr_dot16(const uint4 a, const uint4 b) {
#if __has_builtin(__builtin_amdgcn_udot4)
    return __builtin_amdgcn_udot4(a.w, b.w, __builtin_amdgcn_udot4(a.z, b.z, __builtin_amdgcn_udot4(a.y, b.y, __builtin_amdgcn_udot4(a.x, b.x, 0u, false), false), false), false);
#else
    const u32 x[4] = {a.x, a.y, a.z, a.w}, y[4] = {b.x, b.y, b.z, b.w};
    u32 s = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int k = 0; k < 4; ++k) s += ((x[w] >> (8 * k)) & 255u) * ((y[w] >> (8 * k)) & 255u);
    return s;
#endif
}

// The list of one query row in the wave's LDS slots (column r of s_d and s_i): its entries and the worst of a full list — slot, index, d, norm.
struct NbrList { u32 cnt = 0, ws = 0, wi = 0; u64 wd = 0, wn = 0; };

// Candidate (d, nj, j) offered to the list of k slots; the candidates of a row come in ascending j (step 2 of nbr_gram_kernel).
__device__ __forceinline__ void nbr_list_offer(NbrList& L, u64* s_d, u32* s_i, u32 r, u32 k, const u64* __restrict__ norms, u64 d, u64 nj, u32 j) {
    bool changed = false;
    if (L.cnt < k) { s_d[L.cnt * NBR_TILE + r] = d; s_i[L.cnt * NBR_TILE + r] = j; ++L.cnt; changed = L.cnt == k; }
    else if (nbr_precedes(d, nj, j, L.wd, L.wn, L.wi)) { s_d[L.ws * NBR_TILE + r] = d; s_i[L.ws * NBR_TILE + r] = j; changed = true; }
    if (changed) {                                                         // the list is full: its worst entry
        L.ws = 0; L.wd = s_d[r]; L.wi = s_i[r]; L.wn = norms[L.wi];
        for (u32 s = 1; s < k; ++s) {
            const u64 ds = s_d[s * NBR_TILE + r]; const u32 is = s_i[s * NBR_TILE + r]; const u64 ns = norms[is];
            if (nbr_precedes(L.wd, L.wn, L.wi, ds, ns, is)) { L.ws = s; L.wd = ds; L.wi = is; L.wn = ns; }
        }
    }
}

// The slots sorted by cell index and written: row[s], s < *cnt_out; the other slots of the row get NBR_NONE.
__device__ __forceinline__ void nbr_list_write(const NbrList& L, u32* s_i, u32 r, u32 k, u32* __restrict__ row, u32* __restrict__ cnt_out) {
    for (u32 s = 1; s < L.cnt; ++s) {                                      // by ascending cell index (insertion sort of at most 64 slots)
        const u32 v = s_i[s * NBR_TILE + r];
        u32 t = s;
        for (; t > 0 && s_i[(t - 1) * NBR_TILE + r] > v; --t) s_i[t * NBR_TILE + r] = s_i[(t - 1) * NBR_TILE + r];
        s_i[t * NBR_TILE + r] = v;
    }
    for (u32 s = 0; s < k; ++s) row[s] = s < L.cnt ? s_i[s * NBR_TILE + r] : NBR_NONE;
    *cnt_out = L.cnt;
}

// Step 1 of nbr_gram_kernel for one column tile, and its d into the LDS tile: the 32 x 32 dot products of the rows row0 .. row0 + 31 of
// planes_a (PA planes) with the rows jt .. jt + 31 of planes_b (PB planes), both sets n_pad x K_pad a plane, as u64 in s_tile[row][column].
// The at most min(PA, PB) products with the same a + b share one i32 accumulator.
template <int PA, int PB, bool MFMA>
__device__ __forceinline__ void nbr_tile_dots(const unsigned char* __restrict__ planes_a, const unsigned char* __restrict__ planes_b, u64 plane_bytes, u32 K_pad,
                                              u32 row0, u32 jt, u32 r, u32 h, u64* s_tile) {
    constexpr int T = PA + PB - 1;
    nbr_v16i acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0;
    if constexpr (MFMA) {
        const unsigned char* const pa = planes_a + (u64)(row0 + r) * K_pad + 16u * h;
        const unsigned char* const pb = planes_b + (u64)(jt + r) * K_pad + 16u * h;
        for (u32 s = 0; s < K_pad; s += NBR_KSTEP) {
            nbr_v4i a[PA], b[PB];
#pragma unroll
            for (int p = 0; p < PA; ++p) a[p] = *reinterpret_cast<const nbr_v4i*>(pa + p * plane_bytes + s);
#pragma unroll
            for (int p = 0; p < PB; ++p) b[p] = *reinterpret_cast<const nbr_v4i*>(pb + p * plane_bytes + s);
#pragma unroll
            for (int x = 0; x < PA; ++x)
#pragma unroll
                for (int y = 0; y < PB; ++y) acc[x + y] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[x], b[y], acc[x + y], 0, 0, 0);
        }
    } else {
        const unsigned char* const pb = planes_b + (u64)(jt + r) * K_pad;
        for (u32 s = 0; s < K_pad; s += 16) {
            uint4 b[PB];
#pragma unroll
            for (int p = 0; p < PB; ++p) b[p] = *reinterpret_cast<const uint4*>(pb + p * plane_bytes + s);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const u32 row = row0 + (u32)(e & 3) + 8u * (u32)(e >> 2) + 4u * h;
#pragma unroll
                for (int x = 0; x < PA; ++x) {
                    const uint4 a = *reinterpret_cast<const uint4*>(planes_a + x * plane_bytes + (u64)row * K_pad + s);
#pragma unroll
                    for (int y = 0; y < PB; ++y) acc[x + y][e] += (int)nbr_dot16(a, b[y]);
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        u64 d = 0;
#pragma unroll
        for (int t = 0; t < T; ++t) d += (u64)(u32)acc[t][e] << (7 * t);
        s_tile[((u32)(e & 3) + 8u * (u32)(e >> 2) + 4u * h) * NBR_TILE_PITCH + r] = d;
    }
}

// A wave owns NBR_TILE query rows (a workgroup NBR_ROWS) and streams the column tiles 0, 32, .. in ascending order; the waves of a
// workgroup never wait for each other.  Per column tile:
//   1. the 32 x 32 dot products, one i32 accumulator tile per a + b.  Lane l of both forms ends with column (l & 31) and the rows
//      (reg & 3) + 8 (reg >> 2) + 4 (l >> 5) of the tile in its 16 registers (the C/D map of the 32x32 MFMA).
//        MFMA:  A = the query rows, B = the column rows, both read as 16 bytes at [row l & 31][32 s + 16 (l >> 5)] for k-step s —
//               the same bytes of k on both sides whatever the order of k inside the instruction.
//        plain: the lane's column against its 16 rows, 16 bytes a load, v_dot4 or shifts and multiplies.
//   2. d = sum_t 2^(7t) acc_t in u64 goes through the wave's LDS tile; lane r < 32 then walks the 32 candidates of query row r in
//      ascending cell index and keeps the best k in its slots: a candidate enters a full list only when it strictly precedes the worst
//      entry — every entry has a lower index, so a tie stays with the entry, which is the index rule.  The worst entry is found again
//      after every change of a full list (its norm is read back from norms[]).
// Never candidates: the diagonal, d == 0, columns from n on (padding).  At the end the slots are sorted by cell index and written:
// idx_out[i * k + s], s < cnt_out[i]; the other slots of the row get NBR_NONE.
// Dynamic LDS: NBR_WAVES * nbr_wave_words(k) * 8 bytes.
template <int P, bool MFMA>
__global__ __launch_bounds__(NBR_THREADS) void nbr_gram_kernel(const unsigned char* __restrict__ planes, u32 n, u32 n_pad, u32 K_pad, u32 k,
                                                               const u64* __restrict__ norms, u32* __restrict__ idx_out, u32* __restrict__ cnt_out) {
    extern __shared__ u64 s_nbr[];
    const int lane = lane_id(), w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u32 row0 = (blockIdx.x * NBR_WAVES + (u32)w) * NBR_TILE;
    if (row0 >= n) return;                                                 // (uniform per wave; the kernel has no workgroup barrier)
    u64* const s_tile = s_nbr + (size_t)w * nbr_wave_words(k);
    u64* const s_d = s_tile + NBR_TILE * NBR_TILE_PITCH;
    u32* const s_i = reinterpret_cast<u32*>(s_d + k * NBR_TILE);
    const u64 plane_bytes = (u64)n_pad * K_pad;
    const u32 r = (u32)lane & 31u, h = (u32)lane >> 5;
    const u32 me = row0 + r;                                               // the query row of lanes 0 .. 31 in step 2
    const bool sel = lane < 32 && me < n;
    NbrList L;

    for (u32 jt = 0; jt < n; jt += NBR_TILE) {
        nbr_tile_dots<P, P, MFMA>(planes, planes, plane_bytes, K_pad, row0, jt, r, h, s_tile);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (sel) {
            const u32 cols = n - jt < NBR_TILE ? n - jt : NBR_TILE;
            for (u32 c = 0; c < cols; ++c) {
                const u32 j = jt + c;
                const u64 d = s_tile[r * NBR_TILE_PITCH + c];
                if (j == me || d == 0) continue;
                nbr_list_offer(L, s_d, s_i, r, k, norms, d, norms[j], j);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (sel) {
        nbr_list_write(L, s_i, r, k, idx_out + (u64)me * k, cnt_out + me);
    }
}

// shared[i] = the number of cells in both rows i; the rows ascend by cell index, cnt_a[i] and cnt_b[i] (<= k) entries are read
__global__ __launch_bounds__(256) void nbr_shared_kernel(const u32* __restrict__ idx_a, const u32* __restrict__ cnt_a, const u32* __restrict__ idx_b,
                                                         const u32* __restrict__ cnt_b, u32 n, u32 k, u32* __restrict__ shared) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u32* const a = idx_a + (u64)i * k; const u32* const b = idx_b + (u64)i * k;
    const u32 na = cnt_a[i] < k ? cnt_a[i] : k, nb = cnt_b[i] < k ? cnt_b[i] : k;
    u32 x = 0, y = 0, both = 0;
    while (x < na && y < nb) {
        const u32 va = a[x], vb = b[y];
        both += va == vb; x += va <= vb; y += vb <= va;
    }
    shared[i] = both;
}

}  // namespace fastf
