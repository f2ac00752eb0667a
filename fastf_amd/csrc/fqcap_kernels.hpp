// fqcap_kernels.hpp — device side of `fqcap`: filter's windows (filter_kernels.hpp) with a per-cell rate in
// place of the one global rate.  Part of the umi_engine.hip translation unit, behind filter_kernels.hpp.
//
//   count   pass 0, one lane per read of the window: its line starts and DNA-form key as filter's rec kernel takes them, the
//           lower-bound search of the sorted whitelist keys, hits[lo] += 1 on a match; an escape-form read goes to the host's
//           list (every one: no draw takes part in this pass)
//   rec     pass 1, the record table of flt_rec_kernel; a read whose draw passes the global rate t is searched, its draw is
//           tested against rate[lo] (<= t), and a kept read adds one to kept[lo]; escape-form reads that pass t go to the host
//
// Both counters are added wave by wave: the lanes of a wavefront that hold the same index elect their lowest lane, which adds
// their number with one atomic.  A poly-G barcode that owns a third of a window then costs one atomic per wavefront, not 21.
//
// The arrays hits / kept / rate hold one word per whitelist key and FCP_GUARD words behind, which no kernel touches.
#pragma once
#include "filter_kernels.hpp"

#define FCP_GUARD 16u                 /* words behind hits[], kept[] and rate[] */
#define FCP_GUARD_WORD 0xa5a5a5a5u

#if defined(__HIPCC__)
namespace fastf {

#define FCP_NONE 0xffffffffu

// arr[idx] += 1 for every lane whose idx is not FCP_NONE; every lane of the wavefront calls it (no lane has returned)
__device__ __forceinline__ void fcp_wave_add(u32* __restrict__ arr, u32 idx) {
    const u32 lane = threadIdx.x & 63;
    u64 todo = __ballot(idx != FCP_NONE);
    while (todo) {                                            // uniform: one turn per distinct index of the wavefront
        const u32 leader = (u32)__ffsll((unsigned long long)todo) - 1;
        const u32 li = __shfl(idx, (int)leader, 64);
        const u64 same = __ballot(idx == li);
        if (lane == leader) atomicAdd(&arr[li], (u32)__popcll(same));
        todo &= ~same;
    }
}

// pass 0: matched reads per whitelist key
__global__ __launch_bounds__(256) void fcp_count_kernel(FltWin w, FltState* __restrict__ fs, u32* __restrict__ hits) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    u32 idx = FCP_NONE;
    if (i < w.n_rec) {
        FltRec rc;
        if (flt_rec_lines(w, fs, fs->n0, w.r_lo + i, &rc)) {
            const u64 key = flt_rec_key(w, rc);
            if (key) { const u64 lo = flt_wl_find(w, key); if (lo < w.n_wl) idx = (u32)lo; }
            else flt_escape(w, fs, (u32)i, rc.s1);
        }
    }
    fcp_wave_add(hits, idx);
}

// pass 1: the record table and the capped decision
__global__ __launch_bounds__(256) void fcp_rec_kernel(FltWin w, FltState* __restrict__ fs, const float* __restrict__ rate,
                                                      u32* __restrict__ kept) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    u32 idx = FCP_NONE;
    if (i < w.n_rec) {
        const u64 r = w.r_lo + i;
        FltRec rc = {0, 0, 0, 0, 0, 0};
        if (r < w.limit && flt_rec_lines(w, fs, fs->n0, r, &rc)) {
            const u32 d = w.draws[i];
            if (flt_draw_passes(d, w.rate)) {                 // rate[k] <= t: whoever fails t fails every cell's rate
                const u64 key = flt_rec_key(w, rc);
                if (key) { const u64 lo = flt_wl_find(w, key); if (lo < w.n_wl && flt_draw_passes(d, rate[lo])) idx = (u32)lo; }
                else flt_escape(w, fs, (u32)i, rc.s1);
            }
        }
        w.rec[i] = rc;
        w.len_out[i] = idx != FCP_NONE ? rc.olen : 0u;
    }
    fcp_wave_add(kept, idx);
}

}  // namespace fastf

// ---- host side (fqcap_cmds.c and the tests drive it; include/fastf_amd.h declares it) ----
static int fcp_words(const fastf_fltdev* p, size_t* n) {
    if (p->n_wl > 0xfffffff0ull - FCP_GUARD) return set_err("fqcap: %llu whitelist keys (the indices are 32-bit)", (unsigned long long)p->n_wl);
    *n = (size_t)p->n_wl + FCP_GUARD;
    return 0;
}
static int fcp_fill(fastf_fltdev* p, DevBuf& b, bool guard_only) {
    size_t n;
    if (fcp_words(p, &n) || b.ensure(n * 4)) return 1;
    if (!guard_only && p->n_wl) HIP_OK(hipMemsetAsync(b.p, 0, (size_t)p->n_wl * 4, p->s));
    HIP_OK(hipMemsetAsync((u32*)b.p + p->n_wl, FCP_GUARD_WORD & 0xff, FCP_GUARD * 4, p->s));
    return 0;
}

// after set_whitelist: hits[] and kept[] cleared, every rate[] word and all guard words set to FCP_GUARD_WORD
extern "C" int fastf_fcpdev_begin(fastf_fltdev_t* p) FASTF_TRY {
    if (!p) return set_err("null argument");
    HIP_OK(hipSetDevice(p->device));
    if (fcp_fill(p, p->d_hits, false) || fcp_fill(p, p->d_kept, false) || fcp_fill(p, p->d_cellrate, true)) return 1;
    if (p->n_wl) HIP_OK(hipMemsetAsync(p->d_cellrate.p, FCP_GUARD_WORD & 0xff, (size_t)p->n_wl * 4, p->s));
    HIP_OK(hipStreamSynchronize(p->s));
    p->fcp_keys = p->n_wl;
    return 0;
} FASTF_CATCH_INT

// Pass 0 of the parsed window: hits[] += its matched reads per key, the '\n' carry moves on as after filter's emit.  *esc / *n_esc:
// every escape-form read of the window (pinned, valid until the next call).
extern "C" int fastf_fcpdev_count(fastf_fltdev_t* p, uint32_t L, const fastf_flt_esc_t** esc, uint32_t* n_esc) FASTF_TRY {
    if (!p || !n_esc) return set_err("null argument");
    if (p->fcp_keys != p->n_wl) return set_err("fastf_fcpdev_count: fastf_fcpdev_begin comes first");
    HIP_OK(hipSetDevice(p->device));
    FltWin& w = p->w;
    hipStream_t s = p->s;
    FltState* fs = (FltState*)p->d_fstate.p;
    *n_esc = 0; if (esc) *esc = (const fastf_flt_esc_t*)p->h_esc;
    w.mode = 0; w.all = 0; w.L = L; w.rate = 0.f;
    HIP_OK(hipEventRecord(p->ev[0], s));
    if (w.n_rec) hipLaunchKernelGGL(fcp_count_kernel, dim3((u32)((w.n_rec + 255) / 256)), dim3(256), 0, s, w, fs, (u32*)p->d_hits.p);
    hipLaunchKernelGGL(flt_carry_kernel, dim3(1), dim3(1), 0, s, w, (const FqState*)p->d_state.p, fs);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(p->h_fs, fs, sizeof(FltState), hipMemcpyDeviceToHost, s));
    if (flt_sync(p)) return 1;
    const FltState f = *p->h_fs;
    if (f.err & FLT_ERR_ESCAPES) return set_err("fqcap: escape list overflow");
    if (w.n_rec && f.n_esc) {
        HIP_OK(hipMemcpyAsync(p->h_esc, p->d_esc.p, (size_t)f.n_esc * sizeof(FltEsc), hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
    }
    *n_esc = w.n_rec ? f.n_esc : 0;
    return 0;
} FASTF_CATCH_INT

// between the passes: rate[0 .. n) (n = the whitelist's key count; host memory of the caller's) goes up, kept[] is cleared
extern "C" int fastf_fcpdev_set_rates(fastf_fltdev_t* p, const float* rate, size_t n) FASTF_TRY {
    if (!p || (!rate && n)) return set_err("null argument");
    if (n != p->n_wl || p->fcp_keys != p->n_wl) return set_err("fastf_fcpdev_set_rates: %zu rates for %llu keys", n, (unsigned long long)p->n_wl);
    HIP_OK(hipSetDevice(p->device));
    if (n && copy_h2d(p->d_cellrate.p, rate, n * sizeof(float))) return 1;
    if (n) HIP_OK(hipMemsetAsync(p->d_kept.p, 0, n * 4, p->s));
    HIP_OK(hipStreamSynchronize(p->s));
    return 0;
} FASTF_CATCH_INT

// Pass 1 of the parsed window: fastf_fltdev_decide's R1 mode with rate[] per cell under the global rate t; fastf_fltdev_emit follows
extern "C" int fastf_fcpdev_decide(fastf_fltdev_t* p, uint32_t L, float t, const uint32_t* cs, const fastf_flt_esc_t** esc,
                                   uint32_t* n_esc) FASTF_TRY {
    if (!p || p->fcp_keys != p->n_wl) return set_err("fastf_fcpdev_decide: fastf_fcpdev_begin comes first");
    const float* rate = (const float*)p->d_cellrate.p;
    u32* kept = (u32*)p->d_kept.p;
    return flt_decide_with(p, 0, 0, L, t, cs, esc, n_esc, [=](const FltWin& w, FltState* fs, dim3 grid, hipStream_t s) {
        hipLaunchKernelGGL(fcp_rec_kernel, grid, dim3(256), 0, s, w, fs, rate, kept);
    });
} FASTF_CATCH_INT

// the rand() outputs of the window decided last (its reads r_lo ..), n <= its read count
extern "C" int fastf_fcpdev_draws(fastf_fltdev_t* p, uint32_t* out, uint64_t n) FASTF_TRY {
    if (!p || (!out && n)) return set_err("null argument");
    if (n > p->w.n_rec) return set_err("fastf_fcpdev_draws: %llu draws of a window of %llu reads", (unsigned long long)n, (unsigned long long)p->w.n_rec);
    HIP_OK(hipSetDevice(p->device));
    HIP_OK(hipStreamSynchronize(p->s));
    return n ? copy_d2h(out, p->d_draws.p, n * sizeof(u32)) : 0;
} FASTF_CATCH_INT

// which = 0: hits[], 1: kept[], 2: rate[] (its bits); n_words <= keys + FCP_GUARD, the guard words last
extern "C" int fastf_fcpdev_read(fastf_fltdev_t* p, int which, uint32_t* out, size_t n_words) FASTF_TRY {
    if (!p || (!out && n_words) || which < 0 || which > 2) return set_err("fastf_fcpdev_read: bad argument");
    DevBuf& b = which == 0 ? p->d_hits : which == 1 ? p->d_kept : p->d_cellrate;
    if (p->fcp_keys != p->n_wl || n_words > p->n_wl + FCP_GUARD) return set_err("fastf_fcpdev_read: %zu words of %llu", n_words, (unsigned long long)(p->n_wl + FCP_GUARD));
    HIP_OK(hipSetDevice(p->device));
    HIP_OK(hipStreamSynchronize(p->s));
    return n_words ? copy_d2h(out, b.p, n_words * 4) : 0;
} FASTF_CATCH_INT
#endif
