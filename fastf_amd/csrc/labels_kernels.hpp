// labels_kernels.hpp — the kernel of --labels (resident.c): the label votes of the k nearest neighbours of every sampled cell, at full
// depth or at a grid point, from the neighbour sets fastf_dev_neighbors left on the device.
//
//   label_votes_kernel<G, LDS>   idx (k slots a cell, cnt[i] of them valid, the others 0xFFFFFFFF), lab (u8 per cell, 0: unlabelled)
//                                -> pred, same, labelled (u8 per cell) and conf[a - 1][b] += 1 for every cell with lab == a >= 1 and pred == b
//
// A cell owns a lane group of G = 16, 32 or 64 lanes, the smallest that holds k: lane s of the group loads the label of neighbour s (a
// byte gather from lab, n bytes that stay in cache).  No lane keeps a vote array: the lanes of a group that hold the same label find
// each other by eight ballots, one per bit of the label, so the votes for a lane's own label are one population count; the winner is
// one group reduction of the key (votes << 8) | (255 - label) — the most votes, ties to the smallest label.  Everything is integer.
// conf: LDS == true — the counts of a workgroup are added up in LDS and flushed with one global atomic per non-zero entry;
// LDS == false — one global atomic per labelled cell (n_labels * (n_labels + 1) words that do not fit the LDS).
#pragma once
#include "umi_kernels.hpp"

namespace fastf {

constexpr u32 LAB_THREADS = 256;
constexpr u32 LAB_MAX_K = 64, LAB_MAX_LABELS = 255, LAB_NONE = 0xFFFFFFFFu;
constexpr u32 LAB_LDS_BYTES = 160u * 1024u;                     // the LDS of a gfx950 CU: the kernel has no other LDS
__host__ __device__ constexpr u32 lab_conf_words(u32 n_labels) { return n_labels * (n_labels + 1u); }
__host__ __device__ constexpr bool lab_conf_fits_lds(u32 n_labels) { return n_labels >= 1 && lab_conf_words(n_labels) * 4u <= LAB_LDS_BYTES; }   // 201 labels and fewer

// One pass of a workgroup covers LAB_THREADS / G cells; the passes of a workgroup are gridDim.x * (LAB_THREADS / G) cells apart.  Every
// lane stays in the loop for every pass of its workgroup (a lane without a cell holds label 0): the ballots see whole waves.
// A label above n_labels counts as unlabelled, an index of n and beyond and every slot from cnt[i] on is never used as an index.
template <u32 G, bool LDS>
__global__ __launch_bounds__(LAB_THREADS) void label_votes_kernel(const u32* __restrict__ idx, const u32* __restrict__ cnt, const unsigned char* __restrict__ lab,
                                                                  u32 n, u32 k, u32 n_labels, unsigned char* __restrict__ pred_out,
                                                                  unsigned char* __restrict__ same_out, unsigned char* __restrict__ labelled_out,
                                                                  u32* __restrict__ conf) {
    static_assert(G == 16 || G == 32 || G == 64, "a lane group is 16, 32 or 64 lanes");
    extern __shared__ u32 s_conf[];
    const u32 words = lab_conf_words(n_labels);
    if (LDS) {
        for (u32 w = threadIdx.x; w < words; w += LAB_THREADS) s_conf[w] = 0;
        __syncthreads();
    }
    constexpr u32 PER_PASS = LAB_THREADS / G;
    const u32 lane = lane_id(), s = lane & (G - 1u);
    const u64 group_mask = (G == 64 ? ~0ull : ((1ull << (G & 63u)) - 1ull)) << (lane & ~(G - 1u));
    const u32 passes = (n + PER_PASS * gridDim.x - 1u) / (PER_PASS * gridDim.x);
    for (u32 p = 0; p < passes; ++p) {
        const u64 i = ((u64)p * gridDim.x + blockIdx.x) * PER_PASS + threadIdx.x / G;
        const bool cell = i < n;
        u32 own = 0, l = 0;
        if (cell) {
            const u32 c = cnt[i] < k ? cnt[i] : k;
            own = lab[i];
            if (own > n_labels) own = 0;
            if (s < c) {
                const u32 j = idx[i * k + s];
                if (j < n) { l = lab[j]; if (l > n_labels) l = 0; }
            }
        }
        // the lanes of the group that hold this lane's label: bit by bit, the lanes whose bit agrees
        u64 peers = group_mask;
#pragma unroll
        for (u32 b = 0; b < 8; ++b) {
            const bool bit = (l >> b) & 1u;
            const u64 set = __ballot(bit);
            peers &= bit ? set : ~set;
        }
        const u32 votes = l ? (u32)__popcll(peers) : 0u;
        const u32 labelled = (u32)__popcll(__ballot(l != 0) & group_mask);
        const u32 same = (u32)__popcll(__ballot(l != 0 && l == own) & group_mask);
        u32 key = l ? (votes << 8) | (255u - l) : 0u;
#pragma unroll
        for (u32 off = G / 2; off; off >>= 1) { const u32 o = (u32)__shfl_xor((int)key, (int)off); key = o > key ? o : key; }
        if (cell && s == 0) {
            const u32 pred = key ? 255u - (key & 255u) : 0u;
            pred_out[i] = (unsigned char)pred; same_out[i] = (unsigned char)same; labelled_out[i] = (unsigned char)labelled;
            if (own) {
                const u32 w = (own - 1u) * (n_labels + 1u) + pred;
                if (LDS) atomicAdd(&s_conf[w], 1u); else atomicAdd(&conf[w], 1u);
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (u32 w = threadIdx.x; w < words; w += LAB_THREADS) { const u32 v = s_conf[w]; if (v) atomicAdd(&conf[w], v); }
    }
}

}  // namespace fastf
