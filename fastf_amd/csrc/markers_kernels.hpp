// markers_kernels.hpp — the kernels of --markers (resident.c): per (label, gene of A) the doubled Mann-Whitney U of the label's cells
// against every other labelled cell, the cells of the label that detect the gene and the sum of their counts, from the dense byte
// planes fastf_dev_neighbor_planes left on the device and lab[] of --labels.
//
//   marker_labels_kernel       lab (u8 per cell) -> n_per_label[a - 1] = the cells with lab == a, a in 1 .. n_labels (cleared by the caller)
//   marker_auc_kernel<P, LDS>  the P planes (n_pad x K_pad, plane p holds bits 7p .. 7p+6), lab, n_per_label -> s2u, sum (u64) and det
//                              (u32), n_labels x K each, [a - 1][slot]
//
// With E(v) the labelled cells of a gene with count v and C(v) those below v,  2U[a][g] = sum_{i in a} (2 C(x_i) + E(x_i)) - n_a^2.
// A workgroup owns a tile of MK_TILE<P> adjacent slots and walks every row twice.  Pass 1 builds E per slot in LDS (128^P bins of u32 a
// slot) from the labelled cells; a scan in place turns E into 2C + E; pass 2 adds each cell's term, its detection and its count to
// [label][slot].  Only NON-ZERO counts touch the LDS: E(0) = n_lab - sum_{v > 0} E(v) (n_lab from n_per_label), and a cell with count 0
// has the term E(0), no detection and no count, so the zero cells of label a enter at the end as (n_a - det[a][g]) * E(0).  At 5 %
// non-zero that takes 95 % of the atomics — all of them on one bin — out of both passes.
// LDS == true: the accumulators of the tile (20 bytes per label and slot) sit beside the histogram and leave by plain stores, once.
// LDS == false: every non-zero entry adds with three global atomics, and the workgroup, which alone owns its slots, reads det back and
// adds the zero cells' share and - n_a^2 (modulo 2^64) with one more.  Everything is integer.
// Rows at n_cells and beyond are never read; slots at K and beyond and labels outside 1 .. n_labels take no part; bit 7 of a plane byte
// is masked off, so no value can index beyond a slot's bins.
#pragma once
#include "umi_kernels.hpp"

namespace fastf {

constexpr u32 MK_THREADS = 256;
constexpr u32 MK_MAX_LABELS = 255, MK_MAX_PLANES = 2;
constexpr u32 MK_LDS_BYTES = 160u * 1024u;                      // the LDS of a gfx950 CU
constexpr u32 MK_UNROLL = 4;                                    // row steps in flight per thread
__host__ __device__ constexpr u32 mk_bins(u32 P) { return P == 1 ? 128u : 16384u; }
// slots of a tile: P = 1 — 32 slots, 16 KB of bins, a lane loads 4 slots of a row and 8 lanes a row's 32 contiguous bytes;
// P = 2 — two slots are 128 KB of bins already, a lane loads the 2 slots of a row from either plane
__host__ __device__ constexpr u32 mk_tile(u32 P) { return P == 1 ? 32u : 2u; }
__host__ __device__ constexpr u32 mk_word(u32 P) { return P == 1 ? 4u : 2u; }           // slots (bytes of a plane row) a lane loads
__host__ __device__ constexpr u32 mk_acc_bytes(u32 P, u32 n_labels) { return mk_tile(P) * n_labels * 20u; }
// the LDS of a workgroup: the bins with one pad word per scan chunk (mk_phys: a thread's chunk starts an odd number of words from its
// neighbour's, so the scan meets no bank conflict), the chunk sums (u32 a thread), n_per_label (256 u32), then — LDS form — s2u, sum, det
__host__ __device__ constexpr u32 mk_chunk(u32 P) { return mk_tile(P) * mk_bins(P) / MK_THREADS; }
__host__ __device__ constexpr u32 mk_base_bytes(u32 P) { return (mk_tile(P) * mk_bins(P) + MK_THREADS) * 4u + MK_THREADS * 4u + 256u * 4u; }
__host__ __device__ constexpr u32 mk_lds_bytes(u32 P, u32 n_labels, bool lds) { return mk_base_bytes(P) + (lds ? mk_acc_bytes(P, n_labels) : 0u); }
// P = 1: 225 labels and fewer; P = 2: every n_labels (2 slots x 255 labels are 10 KB)
__host__ __device__ constexpr bool mk_fits_lds(u32 P, u32 n_labels) { return n_labels >= 1 && mk_base_bytes(P) + mk_acc_bytes(P, n_labels) <= MK_LDS_BYTES; }

__global__ __launch_bounds__(256) void marker_labels_kernel(const unsigned char* __restrict__ lab, u32 n_cells, u32 n_labels, u32* __restrict__ n_per_label) {
    __shared__ u32 s_n[256];
    s_n[threadIdx.x] = 0;
    __syncthreads();
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n_cells; i += (u64)gridDim.x * 256) {
        const u32 a = lab[i];
        if (a - 1u < n_labels) atomicAdd(&s_n[a - 1u], 1u);
    }
    __syncthreads();
    const u32 v = s_n[threadIdx.x];
    if (threadIdx.x < n_labels && v) atomicAdd(&n_per_label[threadIdx.x], v);
}

template <u32 P> __device__ __forceinline__ u32 mk_phys(u32 bin) { return bin + bin / mk_chunk(P); }

// the W slots a lane holds of one row: W bytes of each plane
template <u32 P> struct mk_row_words { u32 w[P]; };

template <u32 P>
__device__ __forceinline__ mk_row_words<P> mk_load(const unsigned char* __restrict__ at, u64 plane_bytes) {
    mk_row_words<P> r;
#pragma unroll
    for (u32 p = 0; p < P; ++p) {
        if (P == 1) r.w[p] = *reinterpret_cast<const u32*>(at + p * plane_bytes);
        else r.w[p] = *reinterpret_cast<const unsigned short*>(at + p * plane_bytes);
    }
    return r;
}

template <u32 P>
__device__ __forceinline__ u32 mk_value(const mk_row_words<P>& r, u32 b) {
    u32 v = (r.w[0] >> (8u * b)) & 127u;
    if (P == 2) v |= ((r.w[P - 1] >> (8u * b)) & 127u) << 7;
    return v;
}

template <u32 P, bool LDS>
__global__ __launch_bounds__(MK_THREADS) void marker_auc_kernel(const unsigned char* __restrict__ planes, const unsigned char* __restrict__ lab,
                                                               const u32* __restrict__ n_per_label, u32 n_cells, u32 n_pad, u32 K, u32 K_pad, u32 n_labels,
                                                               u64* __restrict__ s2u_out, u32* __restrict__ det_out, u64* __restrict__ sum_out) {
    static_assert(P == 1 || P == 2, "one or two planes: the bins of a slot live in LDS");
    constexpr u32 B = mk_bins(P), T = mk_tile(P), W = mk_word(P), LPR = T / W, ROWS = MK_THREADS / LPR;
    constexpr u32 CH = mk_chunk(P), TPS = B / CH;        // bins of a thread's scan chunk; threads per slot
    static_assert(B % CH == 0 && CH >= 1, "a scan chunk stays inside one slot");
    extern __shared__ __attribute__((aligned(16))) u32 s_mem[];
    u32* const s_hist = s_mem;                                  // [T][B] through mk_phys
    u32* const s_part = s_hist + T * B + MK_THREADS;                         // [MK_THREADS]
    u32* const s_na = s_part + MK_THREADS;                      // [256]
    u64* const s_s2u = reinterpret_cast<u64*>(s_na + 256);      // [n_labels][T]   (LDS form; 8-byte aligned: the words before are a multiple of 2)
    u64* const s_sum = s_s2u + (LDS ? T * n_labels : 0u);
    u32* const s_det = reinterpret_cast<u32*>(s_sum + (LDS ? T * n_labels : 0u));

    const u32 tid = threadIdx.x, slot0 = blockIdx.x * T;
    const u64 plane_bytes = (u64)n_pad * K_pad;
    for (u32 w = tid; w < T * B + MK_THREADS; w += MK_THREADS) s_hist[w] = 0;
    s_na[tid] = tid < n_labels ? n_per_label[tid] : 0u;
    if (LDS) for (u32 w = tid; w < T * n_labels; w += MK_THREADS) { s_s2u[w] = 0; s_sum[w] = 0; s_det[w] = 0; }
    __syncthreads();
    u32 n_lab = 0;
    for (u32 a = 0; a < n_labels; ++a) n_lab += s_na[a];        // (a broadcast read per step)

    const u32 lr = tid % LPR, ls0 = lr * W;                     // this lane's first slot inside the tile
    const unsigned char* const col = planes + slot0 + ls0;      // (slot0 + ls0 + W <= K_pad: T divides K_pad)
    u32 live = 0;                                               // the lane's slots below K, one bit each
#pragma unroll
    for (u32 b = 0; b < W; ++b) live |= (slot0 + ls0 + b < K ? 1u : 0u) << b;

    // ---- pass 1: E(v), v > 0, of the labelled cells ----
    for (u64 i0 = tid / LPR; i0 < n_cells; i0 += (u64)ROWS * MK_UNROLL) {
        mk_row_words<P> r[MK_UNROLL] = {};
        u32 a[MK_UNROLL];
#pragma unroll
        for (u32 u = 0; u < MK_UNROLL; ++u) {
            const u64 i = i0 + (u64)u * ROWS;
            a[u] = 0;
            if (i < n_cells) { a[u] = lab[i]; r[u] = mk_load<P>(col + i * K_pad, plane_bytes); }
        }
#pragma unroll
        for (u32 u = 0; u < MK_UNROLL; ++u) {
            if (a[u] - 1u >= n_labels) continue;
#pragma unroll
            for (u32 b = 0; b < W; ++b) {
                const u32 v = mk_value<P>(r[u], b);
                if (v && ((live >> b) & 1u)) atomicAdd(&s_hist[mk_phys<P>((ls0 + b) * B + v)], 1u);
            }
        }
    }
    __syncthreads();

    // ---- the scan in place: bin v of a slot becomes 2 C(v) + E(v); bin 0 was never touched and becomes E(0) ----
    {
        const u32 first = tid * (CH + 1u), slot = tid / TPS;      // (mk_phys of the chunk's first bin)
        u32 part = 0;
        for (u32 w = 0; w < CH; ++w) part += s_hist[first + w];
        s_part[tid] = part;
        __syncthreads();
        u32 before = 0, all = 0;                                // the non-zero bins of the slot before this chunk, and all of them
        for (u32 t = slot * TPS; t < (slot + 1u) * TPS; ++t) { const u32 v = s_part[t]; all += v; before += t < tid ? v : 0u; }
        const u32 e0 = n_lab - all;
        u32 c = e0 + before;                                    // C of the chunk's first bin (the slot's first chunk: of bin 1)
        for (u32 w = 0; w < CH; ++w) {
            if (tid % TPS == 0 && w == 0) { s_hist[first] = e0; continue; }
            const u32 e = s_hist[first + w];
            s_hist[first + w] = 2u * c + e;
            c += e;
        }
    }
    __syncthreads();

    // ---- pass 2: the term, the detection and the count of every non-zero labelled entry ----
    for (u64 i0 = tid / LPR; i0 < n_cells; i0 += (u64)ROWS * MK_UNROLL) {
        mk_row_words<P> r[MK_UNROLL] = {};
        u32 a[MK_UNROLL];
#pragma unroll
        for (u32 u = 0; u < MK_UNROLL; ++u) {
            const u64 i = i0 + (u64)u * ROWS;
            a[u] = 0;
            if (i < n_cells) { a[u] = lab[i]; r[u] = mk_load<P>(col + i * K_pad, plane_bytes); }
        }
#pragma unroll
        for (u32 u = 0; u < MK_UNROLL; ++u) {
            if (a[u] - 1u >= n_labels) continue;
#pragma unroll
            for (u32 b = 0; b < W; ++b) {
                const u32 v = mk_value<P>(r[u], b);
                if (!v || !((live >> b) & 1u)) continue;
                const u32 term = s_hist[mk_phys<P>((ls0 + b) * B + v)];
                if (LDS) {
                    const u32 w = (a[u] - 1u) * T + ls0 + b;
                    atomicAdd(reinterpret_cast<unsigned long long*>(&s_s2u[w]), (unsigned long long)term);
                    atomicAdd(reinterpret_cast<unsigned long long*>(&s_sum[w]), (unsigned long long)v);
                    atomicAdd(&s_det[w], 1u);
                } else {
                    const u64 w = (u64)(a[u] - 1u) * K + slot0 + ls0 + b;
                    atomicAdd(reinterpret_cast<unsigned long long*>(&s2u_out[w]), (unsigned long long)term);
                    atomicAdd(reinterpret_cast<unsigned long long*>(&sum_out[w]), (unsigned long long)v);
                    atomicAdd(&det_out[w], 1u);
                }
            }
        }
    }
    if (!LDS) __threadfence();                                  // (the workgroup's own atomics have landed before det is read back)
    __syncthreads();

    // ---- the zero cells and - n_a^2; [a][slot] so that neighbouring threads write neighbouring slots ----
    for (u32 w = tid; w < T * n_labels; w += MK_THREADS) {
        const u32 a = w / T, ls = w % T, slot = slot0 + ls;
        if (slot >= K) continue;
        const u64 na = s_na[a], e0 = s_hist[mk_phys<P>(ls * B)], at = (u64)a * K + slot;
        if (LDS) {
            const u32 det = s_det[w];
            s2u_out[at] = s_s2u[w] + (na - det) * e0 - na * na;
            sum_out[at] = s_sum[w];
            det_out[at] = det;
        } else {
            const u32 det = atomicAdd(&det_out[at], 0u);
            const u64 add = (na - det) * e0 - na * na;
            if (add) atomicAdd(reinterpret_cast<unsigned long long*>(&s2u_out[at]), (unsigned long long)add);
        }
    }
}

}  // namespace fastf
