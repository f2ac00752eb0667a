// mapping_kernels.hpp — the kernels of --mapping (resident.c): every cell of a grid point looked up among ALL full-depth cells of its
// (cell rate, seed) pair, over the highly variable genes A (the definition: include/fastf_amd.h).
//
//   map_max_kernel    a u64 array -> its maximum (the full norms m_j, which the caller brings)
//   map_diag_kernel   row i of the point's planes and of the full rows' planes -> self_dot[i] = e_ii
//   map_gram_kernel   the point's planes (queries), the full rows' planes (candidates), the full norms and self_dot -> per query row the
//                     first k full cells j != i with e_ij > 0 by descending cosine, and self_rank[i] = the candidates j != i that precede i
//
// The planes are those of nbr_planes_kernel (neighbors_kernels.hpp), both sets n_pad x K_pad a plane; the dot products, the order, the
// list in LDS and its walk are that file's (nbr_tile_dots, nbr_precedes, nbr_list_offer, nbr_list_write).  What differs from
// nbr_gram_kernel: the two operands are different matrices, so e_ij != e_ji and the A operand (rows of the tile) must be the point, the
// B operand (columns) the full rows; the norms of the order are the candidates', m_j; and the diagonal tile arrives in the middle of the
// stream, so e_ii is computed beforehand.
#pragma once
#include "neighbors_kernels.hpp"

namespace fastf {

// *max_out was cleared by the caller.
__global__ __launch_bounds__(256) void map_max_kernel(const u64* __restrict__ v, u32 n, u64* __restrict__ max_out) {
    u64 m = 0;
    for (u32 i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) { const u64 x = v[i]; m = x > m ? x : m; }
#pragma unroll
    for (int off = 32; off; off >>= 1) { const u64 o = (u64)__shfl_xor((unsigned long long)m, off); m = o > m ? o : m; }
    if (lane_id() == 0 && m) atomicMax(reinterpret_cast<unsigned long long*>(max_out), (unsigned long long)m);
}

// One wave per row, as nbr_norms_kernel: the counts of both sides recombined from their digits, the products in u64.
__global__ __launch_bounds__(256) void map_diag_kernel(const unsigned char* __restrict__ planes_q, u32 PQ, const unsigned char* __restrict__ planes_f, u32 PF,
                                                       u32 n, u32 n_pad, u32 K_pad, u64* __restrict__ self_dot) {
    const int lane = lane_id();
    const u32 waves = gridDim.x * (256 / WAVE);
    const u64 plane_words = (u64)n_pad * K_pad / 4;
    for (u32 i = blockIdx.x * (256 / WAVE) + (threadIdx.x >> 6); i < n; i += waves) {
        const u32* const rq = reinterpret_cast<const u32*>(planes_q + (u64)i * K_pad);
        const u32* const rf = reinterpret_cast<const u32*>(planes_f + (u64)i * K_pad);
        u64 sum = 0;
        for (u32 w = lane; w < K_pad / 4; w += WAVE) {
            u32 q[NBR_MAX_PLANES] = {0, 0, 0}, f[NBR_MAX_PLANES] = {0, 0, 0};
            for (u32 p = 0; p < PQ; ++p) q[p] = rq[p * plane_words + w];
            for (u32 p = 0; p < PF; ++p) f[p] = rf[p * plane_words + w];
#pragma unroll
            for (u32 b = 0; b < 4; ++b) {
                const u64 y = (u64)((q[0] >> (8 * b)) & 127u) | (u64)((q[1] >> (8 * b)) & 127u) << 7 | (u64)((q[2] >> (8 * b)) & 127u) << 14;
                const u64 x = (u64)((f[0] >> (8 * b)) & 127u) | (u64)((f[1] >> (8 * b)) & 127u) << 7 | (u64)((f[2] >> (8 * b)) & 127u) << 14;
                sum += x * y;
            }
        }
        sum = wave_sum64(sum);
        if (lane == 0) self_dot[i] = sum;
    }
}

// The shape of nbr_gram_kernel: a wave owns NBR_TILE query rows — rows of the POINT — and streams the column tiles — rows of the FULL
// set — in ascending order, without a workgroup barrier.  Lane r < 32 walks the 32 candidates of its query row me = row0 + r:
//   the diagonal and e == 0 are no candidates for the list;
//   with self_dot[me] > 0 every other candidate with e > 0 is compared once more, against (self_dot[me], m_me, me): the candidates
//   that precede the cell's own full-depth profile are counted in the lane's rank;
//   then the walk of nbr_list_offer with the candidates' norms m_j.
// idx_out, cnt_out: as nbr_gram_kernel writes them; rank_out[i] = the count, NBR_NONE when self_dot[i] == 0.
// Dynamic LDS: NBR_WAVES * nbr_wave_words(k) * 8 bytes.
template <int PQ, int PF, bool MFMA>
__global__ __launch_bounds__(NBR_THREADS) void map_gram_kernel(const unsigned char* __restrict__ planes_q, const unsigned char* __restrict__ planes_f, u32 n, u32 n_pad,
                                                               u32 K_pad, u32 k, const u64* __restrict__ norms_f, const u64* __restrict__ self_dot,
                                                               u32* __restrict__ idx_out, u32* __restrict__ cnt_out, u32* __restrict__ rank_out) {
    extern __shared__ u64 s_nbr[];
    const int lane = lane_id(), w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u32 row0 = (blockIdx.x * NBR_WAVES + (u32)w) * NBR_TILE;
    if (row0 >= n) return;                                                 // (uniform per wave; the kernel has no workgroup barrier)
    u64* const s_tile = s_nbr + (size_t)w * nbr_wave_words(k);
    u64* const s_d = s_tile + NBR_TILE * NBR_TILE_PITCH;
    u32* const s_i = reinterpret_cast<u32*>(s_d + k * NBR_TILE);
    const u64 plane_bytes = (u64)n_pad * K_pad;
    const u32 r = (u32)lane & 31u, h = (u32)lane >> 5;
    const u32 me = row0 + r;                                               // the query row of lanes 0 .. 31 in the walk
    const bool sel = lane < 32 && me < n;
    const u64 sd = sel ? self_dot[me] : 0, sm = sel ? norms_f[me] : 0;      // the cell's own full-depth profile as a candidate
    NbrList L;
    u32 rank = 0;

    for (u32 jt = 0; jt < n; jt += NBR_TILE) {
        nbr_tile_dots<PQ, PF, MFMA>(planes_q, planes_f, plane_bytes, K_pad, row0, jt, r, h, s_tile);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (sel) {
            const u32 cols = n - jt < NBR_TILE ? n - jt : NBR_TILE;
            for (u32 c = 0; c < cols; ++c) {
                const u32 j = jt + c;
                const u64 d = s_tile[r * NBR_TILE_PITCH + c];
                if (j == me || d == 0) continue;
                const u64 nj = norms_f[j];
                if (sd) rank += nbr_precedes(d, nj, j, sd, sm, me);
                nbr_list_offer(L, s_d, s_i, r, k, norms_f, d, nj, j);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (sel) {
        nbr_list_write(L, s_i, r, k, idx_out + (u64)me * k, cnt_out + me);
        rank_out[me] = sd ? rank : NBR_NONE;
    }
}

}  // namespace fastf
