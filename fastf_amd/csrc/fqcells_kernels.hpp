// fqcells_kernels.hpp — device side of `fqcells`: the tag histogram's distinct CB+UMI keys and their counts
// -> one row per barcode.  Part of the umi_engine.hip translation unit, behind filter_kernels.hpp (whose block-sum scan it uses).
//
// The m1 keys ascend, so the keys of one barcode = (key without its tag bit) >> 2 * len_umi are one contiguous run: its length is
// the barcode's distinct UMIs, the sum of its counts the barcode's reads.
//
//   heads   one workgroup per tile of FQC_TILE keys, a wavefront per FQC_TILE / 4 of them in strips of 64 (one dwordx2 load per
//           key and lane): a key is a head iff its barcode differs from its predecessor's (lane 0 of a strip reads the key before
//           the strip, the first key of all is a head); the tile's heads into bsum[tile]
//   scan    filter's flt_sums_scan_kernel over bsum: rows before every tile, and B = the total
//   rows    the tiles again: row of a key = heads up to and including it - 1; a head writes bc[row]; the lanes of a strip that
//           share a row are one run of lanes, whose first lane adds the run's counts (from the strip's prefix sums) to reads[row]
//           and its length to umis[row] with one atomic each.  A barcode that owns 4^u keys costs one pair of atomics per strip.
//
// Integer adds only: the table does not depend on the order.  bc[], reads[] and umis[] hold one entry per row and FQC_GUARD
// entries behind, which no kernel touches.
#pragma once
#include "filter_kernels.hpp"

#define FQC_TILE 1024u                /* keys per workgroup: 4 wavefronts x FQC_STRIPS strips x 64 lanes */
#define FQC_STRIPS 4u
#define FQC_GUARD 16u                 /* entries behind bc[], reads[] and umis[] */
#define FQC_GUARD_BYTE 0xa5

#if defined(__HIPCC__)
namespace fastf {

__device__ __forceinline__ u64 fqc_barcode(u64 key, u32 shift) { return (key & ~FQ_DNA_TAG) >> shift; }

// strip j of the wavefront that starts at key i0: the lane's key (0 beyond m1) and the strip's head mask
__device__ __forceinline__ u64 fqc_strip_heads(const u64* __restrict__ keys, u64 m1, u64 i, u32 shift, u64* key_out) {
    const bool valid = i < m1;
    const u64 key = valid ? keys[i] : 0;
    u64 prev = __shfl_up(key, 1, 64);
    if ((threadIdx.x & 63) == 0 && valid && i) prev = keys[i - 1];
    *key_out = key;
    return __ballot(valid && (i == 0 || fqc_barcode(prev, shift) != fqc_barcode(key, shift)));
}

__global__ __launch_bounds__(256) void fqc_heads_kernel(const u64* __restrict__ keys, u64 m1, u32 shift, u64* __restrict__ bsum) {
    __shared__ u32 sh[4];
    const u32 lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const u64 i0 = (u64)blockIdx.x * FQC_TILE + wv * (FQC_STRIPS * 64u) + lane;
    u32 heads = 0;
#pragma unroll
    for (u32 j = 0; j < FQC_STRIPS; j++) {
        u64 key;
        heads += (u32)__popcll(fqc_strip_heads(keys, m1, i0 + j * 64u, shift, &key));
    }
    if (lane == 0) sh[wv] = heads;
    __syncthreads();
    if (threadIdx.x == 0) bsum[blockIdx.x] = (u64)sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ __launch_bounds__(256) void fqc_rows_kernel(const u64* __restrict__ keys, const u32* __restrict__ counts, u64 m1, u32 shift,
                                                       const u64* __restrict__ tile_rows, u64* __restrict__ bc,
                                                       u64* __restrict__ reads, u32* __restrict__ umis) {
    __shared__ u32 sh[4];
    const u32 lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const u64 i0 = (u64)blockIdx.x * FQC_TILE + wv * (FQC_STRIPS * 64u) + lane;
    u64 key[FQC_STRIPS], hm[FQC_STRIPS];
    u32 heads = 0;
#pragma unroll
    for (u32 j = 0; j < FQC_STRIPS; j++) {
        hm[j] = fqc_strip_heads(keys, m1, i0 + j * 64u, shift, &key[j]);
        heads += (u32)__popcll(hm[j]);
    }
    if (lane == 0) sh[wv] = heads;
    __syncthreads();
    u64 base = tile_rows[blockIdx.x];                         // heads before this wavefront's first key
    for (u32 k = 0; k < wv; k++) base += sh[k];
    const u64 le = (2ull << lane) - 1;                        // lanes 0 .. lane
#pragma unroll
    for (u32 j = 0; j < FQC_STRIPS; j++) {
        const u64 i = i0 + j * 64u;
        const u64 vm = __ballot(i < m1);
        if (!vm) break;                                       // (uniform: the strips behind are beyond m1 too)
        const u32 c = i < m1 ? counts[i] : 0u;
        const u64 incl = fq_wave_incl((u64)c, FqAdd());
        const u64 below = hm[j] & le, above = hm[j] & ~le;
        const u32 s = below ? 63u - (u32)__clzll((long long)below) : 0u;                    // first lane of my run in this strip
        const u32 e = above ? (u32)__ffsll((unsigned long long)above) - 2u : 63u - (u32)__clzll((long long)vm);   // and its last
        const u64 to_e = __shfl(incl, (int)e, 64);
        const u64 row = base + (u32)__popcll(below) - 1;      // (key 0 is a head: never -1 for a key that exists)
        if (i < m1) {
            if ((hm[j] >> lane) & 1) bc[row] = fqc_barcode(key[j], shift);
            if (lane == s) {
                atomicAdd((unsigned long long*)&reads[row], (unsigned long long)(to_e - (incl - c)));
                atomicAdd(&umis[row], e - s + 1u);
            }
        }
        base += (u32)__popcll(hm[j]);
    }
}

}  // namespace fastf

// ---- host side (fqcells_cmds.c and the tests drive it; include/fastf_amd.h declares the seam) ----
struct FqcBufs { DevBuf bsum, fs, bc, reads, umis; };
struct FqcEvents { hipEvent_t a = nullptr, b = nullptr; ~FqcEvents() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } };
static void fqc_release(FqcBufs& b) { for (DevBuf* d : {&b.bsum, &b.fs, &b.bc, &b.reads, &b.umis}) d->release(); }

// d_keys / d_counts: m1 ascending keys and their counts on the current device.  The three kernels on stream s, waited for; *n_rows
// = B; the table in b.bc / b.reads / b.umis with the guard entries behind.  *ms (may be null): events around all of it — the
// kernels, the synchronise and 8-byte copy of B between them, the allocations of the rows and their clears: a window, not kernel time.
static int fqc_reduce(FqcBufs& b, const u64* d_keys, const u32* d_counts, u64 m1, u32 len_umi, hipStream_t s, u64* n_rows, double* ms) {
    *n_rows = 0;
    if (len_umi > 30) return set_err("fqcells reduce: a UMI of %u bases (a key holds 31 bases, one of them the barcode's)", len_umi);
    const u64 nb = (m1 + FQC_TILE - 1) / FQC_TILE;
    if (nb > 0x7fffffffull) return set_err("fqcells reduce: %llu keys", (unsigned long long)m1);
    const u32 shift = 2 * len_umi;
    FqcEvents ev;
    if (ms) { *ms = 0; HIP_OK(hipEventCreate(&ev.a)); HIP_OK(hipEventCreate(&ev.b)); HIP_OK(hipEventRecord(ev.a, s)); }
    u64 B = 0;
    if (m1) {
        if (b.bsum.ensure(nb * sizeof(u64)) || b.fs.ensure(sizeof(FltState))) return 1;
        hipLaunchKernelGGL(fqc_heads_kernel, dim3((u32)nb), dim3(256), 0, s, d_keys, m1, shift, (u64*)b.bsum.p);
        hipLaunchKernelGGL(flt_sums_scan_kernel, dim3(1), dim3(1024), 0, s, (u64*)b.bsum.p, (u32)nb, (FltState*)b.fs.p);
        HIP_OK(hipGetLastError());
        HIP_OK(hipStreamSynchronize(s));
        if (copy_d2h(&B, &((FltState*)b.fs.p)->total, sizeof B)) return 1;
        if (B == 0 || B > m1) return set_err("fqcells reduce: %llu rows of %llu keys", (unsigned long long)B, (unsigned long long)m1);
    }
    if (b.bc.ensure((B + FQC_GUARD) * sizeof(u64)) || b.reads.ensure((B + FQC_GUARD) * sizeof(u64)) ||
        b.umis.ensure((B + FQC_GUARD) * sizeof(u32))) return 1;
    if (B) {
        HIP_OK(hipMemsetAsync(b.reads.p, 0, B * sizeof(u64), s));
        HIP_OK(hipMemsetAsync(b.umis.p, 0, B * sizeof(u32), s));
    }
    HIP_OK(hipMemsetAsync((u64*)b.bc.p + B, FQC_GUARD_BYTE, FQC_GUARD * sizeof(u64), s));
    HIP_OK(hipMemsetAsync((u64*)b.reads.p + B, FQC_GUARD_BYTE, FQC_GUARD * sizeof(u64), s));
    HIP_OK(hipMemsetAsync((u32*)b.umis.p + B, FQC_GUARD_BYTE, FQC_GUARD * sizeof(u32), s));
    if (B) {
        hipLaunchKernelGGL(fqc_rows_kernel, dim3((u32)nb), dim3(256), 0, s, d_keys, d_counts, m1, shift, (const u64*)b.bsum.p,
                           (u64*)b.bc.p, (u64*)b.reads.p, (u32*)b.umis.p);
        HIP_OK(hipGetLastError());
    }
    if (ms) HIP_OK(hipEventRecord(ev.b, s));
    HIP_OK(hipStreamSynchronize(s));
    float f = 0;
    if (ms && hipEventElapsedTime(&f, ev.a, ev.b) == hipSuccess) *ms = f;
    *n_rows = B;
    return 0;
}

extern "C" size_t fastf_fqcells_tile(void) { return FQC_TILE; }

// The seam: host arrays in (m1 ascending keys, their counts), the reduce's kernels, host arrays out.  bc / reads / umis hold m1 + 16
// entries (the caller cannot know B ahead): rows [0, *n_rows), then the 16 guard entries as the device arrays carry them.
extern "C" int fastf_fqcells_reduce(const uint64_t* keys, const uint32_t* counts, size_t m1, uint32_t len_umi, uint64_t* bc,
                                    uint64_t* reads, uint32_t* umis, size_t* n_rows) FASTF_TRY {
    if ((m1 && (!keys || !counts)) || !bc || !reads || !umis || !n_rows) return set_err("null argument");
    *n_rows = 0;
    HIP_OK(hipSetDevice(0));                                  // (the process's device 0, as the histogram of freq)
    FqcBufs b; DevBuf d_keys, d_counts;
    auto done = [&](int rc) { fqc_release(b); d_keys.release(); d_counts.release(); return rc; };
    if (m1 && (d_keys.ensure(m1 * sizeof(u64)) || d_counts.ensure(m1 * sizeof(u32)) || copy_h2d(d_keys.p, keys, m1 * sizeof(u64)) ||
               copy_h2d(d_counts.p, counts, m1 * sizeof(u32)))) return done(1);
    u64 B = 0;
    if (fqc_reduce(b, (const u64*)d_keys.p, (const u32*)d_counts.p, m1, len_umi, nullptr, &B, nullptr)) return done(1);
    if (copy_d2h(bc, b.bc.p, (B + FQC_GUARD) * sizeof(u64)) || copy_d2h(reads, b.reads.p, (B + FQC_GUARD) * sizeof(u64)) ||
        copy_d2h(umis, b.umis.p, (B + FQC_GUARD) * sizeof(u32))) return done(1);
    *n_rows = (size_t)B;
    return done(0);
} FASTF_CATCH_INT

// the command's steps 2 to 4a: the device-resident finish, the reduce, the table down through the bounce buffer (one copy an array)
extern "C" int fastf_fqcells_table(fastf_taghist_t* h, uint32_t len_umi, uint64_t** bc, uint64_t** reads, uint32_t** umis, size_t* n_rows,
                                   uint64_t* m1_out, double* reduce_ms) FASTF_TRY {
    if (!h || !bc || !reads || !umis || !n_rows) return set_err("null argument");
    *bc = nullptr; *reads = nullptr; *umis = nullptr; *n_rows = 0;
    const uint64_t* d_keys = nullptr; const uint32_t* d_counts = nullptr; uint64_t m1 = 0;
    if (fastf_taghist_finish_device(h, &d_keys, &d_counts, &m1)) return 1;
    if (m1_out) *m1_out = m1;
    FqcBufs b;
    u64 B = 0;
    int rc = fqc_reduce(b, (const u64*)d_keys, (const u32*)d_counts, m1, len_umi, h->ws->s_compute, &B, reduce_ms);
    if (!rc) {
        *bc = (uint64_t*)malloc((B ? B : 1) * sizeof(u64)); *reads = (uint64_t*)malloc((B ? B : 1) * sizeof(u64));
        *umis = (uint32_t*)malloc((B ? B : 1) * sizeof(u32));
        if (!*bc || !*reads || !*umis) rc = set_err("out of memory (%llu barcodes)", (unsigned long long)B);
        else if (B) rc = copy_d2h(*bc, b.bc.p, B * sizeof(u64)) || copy_d2h(*reads, b.reads.p, B * sizeof(u64)) || copy_d2h(*umis, b.umis.p, B * sizeof(u32));
    }
    if (rc) { free(*bc); free(*reads); free(*umis); *bc = nullptr; *reads = nullptr; *umis = nullptr; }
    else *n_rows = (size_t)B;
    fqc_release(b);
    return rc;
} FASTF_CATCH_INT
#endif
