// coex_host.cpp — the plain C++ part of fastf_amd/csrc/coexpr_kernels.hpp compiled for the host: the per-gene walk of
// coex_select_kernel, the digit recombination of coex_gram_kernel and the plane byte of coex_planes_kernel, checked on the CPU against
// the definition (tests/test_coexpr_kernels_host.py) before any of it runs on a device.
#include "../fastf_amd/csrc/coexpr_kernels.hpp"
#include <stdlib.h>

using namespace fastf;

extern "C" {
// the selection as the device runs it: V first, then one walk per gene on its own k slots, laid out `stride` apart as in the LDS of a
// workgroup (stride 1: packed).  idx[g * k + s], s < cnt[g], ascending; the other slots 0xFFFFFFFF.  Returns 1 when out of memory.
int coex_host_select(const uint64_t* D, const uint64_t* S, uint32_t n, uint32_t K, uint32_t k, uint32_t stride, uint32_t* idx, uint32_t* cnt) {
    uint64_t* V = (uint64_t*)malloc(((size_t)K + 1) * sizeof *V);
    uint64_t* sc = (uint64_t*)malloc(((size_t)k * stride + 1) * sizeof *sc);
    uint32_t* si = (uint32_t*)malloc(((size_t)k * stride + 1) * sizeof *si);
    if (!V || !sc || !si) { free(V); free(sc); free(si); return 1; }
    for (uint32_t h = 0; h < K; ++h) V[h] = (uint64_t)((unsigned __int128)n * D[(size_t)h * K + h] - (unsigned __int128)S[h] * S[h]);
    for (uint32_t g = 0; g < K; ++g) {
        const uint32_t lane = g % stride;                    // the thread's own column of the slots
        const uint32_t c = coex_walk(D, S, V, n, K, k, g, sc + lane, si + lane, stride);
        for (uint32_t s = 0; s < k; ++s) idx[(size_t)g * k + s] = s < c ? si[(size_t)s * stride + lane] : COEX_NONE;
        cnt[g] = c;
    }
    free(V); free(sc); free(si);
    return 0;
}
uint64_t coex_host_recombine(const int32_t* acc, int T) { return coex_recombine(acc, T); }
// the padded shape for a chunk, the offset of a plane byte and its value
void coex_host_pad(uint32_t n_cells, uint32_t K, uint32_t chunk, uint32_t* K_pad, uint32_t* n_pad, uint32_t* chunk_eff) { coex_pad(n_cells, K, chunk, K_pad, n_pad, chunk_eff); }
uint64_t coex_host_plane_at(uint32_t p, uint32_t slot, uint32_t cell, uint32_t K_pad, uint32_t n_pad) { return coex_plane_at(p, slot, cell, K_pad, n_pad); }
uint32_t coex_host_digit(uint32_t count, uint32_t p) { return coex_digit(count, p); }
uint32_t coex_host_default_chunk(void) { return COEX_CHUNK; }
uint32_t coex_host_chunk_max(void) { return COEX_CHUNK_MAX; }
}
