// fastq_kernels.hpp — device side of `freq`: FASTQ text in HBM → one 64-bit key per read, written at the
// read's index straight into the tag histogram's key array (tag_hist.hpp), part of the umi_engine.hip translation unit.
//
// Reference steps replaced (filter.c:15-37 get_fastq, :260-275 substring, count.c:3-21 cell_counts): gzgets() framing of
// four lines per read and strncpy() of the first L = len_cb + len_umi bytes of the sequence line.
//
//   count   one workgroup per 4 KiB tile, 16 bytes per lane (one dwordx4 load): '\n' per tile and the last '\n' of the tile
//   scan    one workgroup: exclusive sums of the tile counts (global line index at every tile) and the start of the line
//           each tile begins in; the carried state (lines before the window, start of the open line) moves on in HBM
//   emit    the tiles again: every '\n' closes line j and opens line j + 1; lines longer than gzgets' 1023 bytes set the
//           error word (first offending read by atomicMin); an opened sequence line (j + 1 = 1 mod 4) of read r = (j + 1) / 4
//           is packed: exactly L <= 31 bytes of [ACGT] -> the DNA form (bit 63 | 2 bits per base, A<C<G<T, so that key
//           order is strcmp order), anything else -> (read, offset) onto the window's escape list, which the host turns
//           into strings with strncpy semantics
//   pending a sequence line whose key bytes run past the window's end is handed to the next window: every window is
//           preceded in its buffer by the last FQ_HDR bytes of the one before, so the next window sees those bytes whole
//
// The functions above the kernels are plain C: fastq_cmds.c (the host's escape strings and key decode) and tools/fq_host.cpp
// (the CPU test suite) compile them as they are.
#pragma once
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define FQ_HD __host__ __device__ __forceinline__
#else
#define FQ_HD static inline
#endif

#define FQ_HDR 1024u                  /* bytes of the previous window in front of every window (host staging and device buffer) */
#define FQ_MAX_LINE 1023u             /* gzgets(buf, 1024): longer lines are split — refused */
#define FQ_DNA_TAG (1ull << 63)       /* DNA-form keys; escape keys are 1 + ordinal in the host's string table (bit 63 clear) */
#define FQ_MAX_DNA 31u
#define FQ_TILE 4096u                 /* bytes per workgroup of the count / emit kernels: 256 lanes x 16 */
#define FQ_PEND_CAP 1024u             /* sequence lines handed to the next window (at most FQ_HDR / 4 + 1 can be) */
#define FQ_ERR_LONG_LINE 1u
#define FQ_ERR_PENDING 2u
#define FQ_ERR_ESCAPES 4u
#define FQ_ERR_KEY_CAP 8u

/* bytes the host would read back for the key string of a sequence line starting at p, with `avail` bytes before the end of the
 * data: strncpy(dst, seq, L) of the gzgets buffer — the line up to and including its '\n', cut at the first NUL and at L */
FQ_HD uint32_t fq_escape_len(const unsigned char *p, uint64_t avail, uint64_t L)
{
    uint64_t n = L < avail ? L : avail;
    if (n > FQ_MAX_LINE) n = FQ_MAX_LINE;
    for (uint32_t i = 0; i < (uint32_t)n; i++) {
        if (p[i] == 0) return i;
        if (p[i] == '\n') return i + 1;
    }
    return (uint32_t)n;
}

/* the per-lane packer.  w[0..8] = the 36 bytes from 4-byte aligned address (s - off), little-endian words, off = s & 3;
 * avail = bytes from s to the end of the data.  Returns the DNA-form key, or 0: the read takes the escape path. */
FQ_HD uint64_t fq_pack_dna(const uint32_t *w, uint32_t off, uint64_t avail, uint32_t L)
{
    if (L > FQ_MAX_DNA || avail < L) return 0;
    uint32_t x[8];
    const uint32_t sh = 8u * off;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int q = 0; q < 8; q++) x[q] = sh ? (w[q] >> sh) | (w[q + 1] << (32u - sh)) : w[q];
    uint64_t v = 0;
    uint32_t bad = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < FQ_MAX_DNA; i++) {
        if (i < L) {
            const uint32_t c = (x[i >> 2] >> (8u * (i & 3u))) & 255u;
            bad |= (uint32_t)(c != 'A' && c != 'C' && c != 'G' && c != 'T');
            v = (v << 2) | (((c >> 1) ^ (c >> 2)) & 3u);          /* A 0, C 1, G 2, T 3 */
        }
    }
    return bad ? 0 : (FQ_DNA_TAG | v);
}

/* the L bases of a DNA-form key into out[0..L) */
FQ_HD void fq_decode_dna(uint64_t key, uint32_t L, char *out)
{
    for (uint32_t i = 0; i < L; i++) out[i] = "ACGT"[(key >> (2u * (L - 1u - i))) & 3u];
}

#if defined(__HIPCC__)
namespace fastf {

// carried in HBM from window to window (one per run)
struct FqState {
    u64 n_nl;                 // '\n' before the current window
    u64 line_start;           // where the line open at the start of the current window began
    u32 n_pend[2];            // sequence lines handed on by the window of that parity
    u32 n_esc;                // escapes of the current window
    u32 err;                  // FQ_ERR_*
    u64 err_rec;              // first read with a line longer than FQ_MAX_LINE
};
struct FqPend { u64 s, r; };  // sequence line at global offset s, read r
struct FqWin {
    const unsigned char* buf; // device: FQ_HDR bytes of the previous window, then the window (64 bytes of slack behind)
    u64 a, len;               // global offset of buf[FQ_HDR], bytes in the window
    u32 last, parity, L;      // L = len_cb + len_umi, capped at 1024
    u64* keys; u64 key_cap;   // the histogram's key array
    FqPend* pend_in; FqPend* pend_out; FqPend* esc; u32 esc_cap;
};

// '\n' in the low / high bit of each byte: exact per-byte zero test of x ^ 0x0a0a0a0a
__device__ __forceinline__ u32 fq_nl_bits(u32 x) {
    const u32 y = x ^ 0x0a0a0a0au;
    const u32 z = ~(((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y | 0x7f7f7f7fu);   // 0x80 where the byte was '\n'
    // gather the four flags into bits 0..3
    return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u);
}
// 16-bit mask of the '\n' among the lane's 16 bytes at buf[o .. o + 16), bytes at or past `valid` masked off
__device__ __forceinline__ u32 fq_lane_mask(const unsigned char* buf, u64 o, u64 valid) {
    if (o >= valid) return 0;
    const uint4 v = *reinterpret_cast<const uint4*>(buf + o);
    u32 m = fq_nl_bits(v.x) | (fq_nl_bits(v.y) << 4) | (fq_nl_bits(v.z) << 8) | (fq_nl_bits(v.w) << 12);
    if (valid - o < 16) m &= (1u << (u32)(valid - o)) - 1u;
    return m;
}

template <typename T, typename Op> __device__ __forceinline__ T fq_wave_incl(T v, Op op) {
    const u32 lane = threadIdx.x & 63;
#pragma unroll
    for (u32 d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(v, d, 64);
        if (lane >= d) v = op(v, t);
    }
    return v;
}
struct FqAdd { __device__ u64 operator()(u64 a, u64 b) const { return a + b; } };
struct FqMax { __device__ u64 operator()(u64 a, u64 b) const { return a > b ? a : b; } };

// exclusive block scan (256 lanes = 4 waves); returns the exclusive value, *total the block's total
template <typename Op> __device__ __forceinline__ u64 fq_block_excl(u64 v, u64 ident, Op op, u64* sh, u64* total) {
    const u32 lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const u64 inc = fq_wave_incl(v, op);
    if (lane == 63) sh[wv] = inc;
    __syncthreads();
    u64 before = ident;
    for (u32 i = 0; i < wv; i++) before = op(before, sh[i]);
    u64 all = ident;
    for (u32 i = 0; i < 4; i++) all = op(all, sh[i]);
    const u64 prev_in_wave = __shfl_up(inc, 1, 64);
    const u64 ex = lane ? op(before, prev_in_wave) : before;
    __syncthreads();
    *total = all;
    return ex;
}

// count: '\n' per tile and 1 + offset of the tile's last '\n' (0: none)
__global__ __launch_bounds__(256) void fq_count_kernel(const unsigned char* __restrict__ buf, u64 len, u32* __restrict__ tile_cnt,
                                                       u64* __restrict__ tile_last) {
    __shared__ u64 sh[4];
    const u64 o = (u64)blockIdx.x * FQ_TILE + threadIdx.x * 16u;
    const u32 m = fq_lane_mask(buf + FQ_HDR, o, len);
    const u64 last = m ? o + (31u - __clz(m)) + 1 : 0;
    u64 tot_c, tot_l;
    (void)fq_block_excl((u64)__popc(m), 0, FqAdd(), sh, &tot_c);
    (void)fq_block_excl(last, 0, FqMax(), sh, &tot_l);
    if (threadIdx.x == 0) { tile_cnt[blockIdx.x] = (u32)tot_c; tile_last[blockIdx.x] = tot_l; }
}

// scan (one workgroup of 1024): tile_base = global index of the first '\n' of every tile, tile_ls = start of the line open at
// its first byte; the carried state moves on to the next window, the window's lists are emptied
__global__ __launch_bounds__(1024) void fq_scan_kernel(u32 n_tiles, u64 a, const u32* __restrict__ tile_cnt,
                                                       const u64* __restrict__ tile_last, u64* __restrict__ tile_base,
                                                       u64* __restrict__ tile_ls, FqState* __restrict__ st, u32 parity) {
    __shared__ u64 sc[16], sl[16];
    const u32 t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const u32 per = (n_tiles + 1023) / 1024, lo = min(n_tiles, t * per), hi = min(n_tiles, lo + per);
    u64 c = 0, l = 0;
    for (u32 i = lo; i < hi; i++) { c += tile_cnt[i]; if (tile_last[i]) l = a + tile_last[i]; }   // l: 1 + global offset
    const u64 ci = fq_wave_incl(c, FqAdd()), li = fq_wave_incl(l, FqMax());
    if (lane == 63) { sc[wv] = ci; sl[wv] = li; }
    __syncthreads();
    const u64 n_nl = st->n_nl, ls0 = st->line_start;
    u64 cb = 0, lb = 0, ct = 0, lt = 0;
    for (u32 i = 0; i < 16; i++) { if (i < wv) { cb += sc[i]; lb = max(lb, sl[i]); } ct += sc[i]; lt = max(lt, sl[i]); }
    const u64 cp = __shfl_up(ci, 1, 64), lp = __shfl_up(li, 1, 64);
    u64 base = n_nl + cb + (lane ? cp : 0), ls = max(ls0, max(lb, lane ? lp : 0));
    for (u32 i = lo; i < hi; i++) {
        tile_base[i] = base; tile_ls[i] = ls;
        base += tile_cnt[i];
        if (tile_last[i]) ls = a + tile_last[i];
    }
    __syncthreads();
    if (t == 0) {
        st->n_nl = n_nl + ct;
        st->line_start = max(ls0, lt);
        st->n_pend[parity] = 0;
        st->n_esc = 0;
    }
}

// the sequence line at global offset s of read r: DNA key into keys[r], or onto the escape list
__device__ __forceinline__ void fq_resolve(const FqWin& w, FqState* st, u64 s, u64 r) {
    if (r >= w.key_cap) { atomicOr(&st->err, FQ_ERR_KEY_CAP); return; }
    const u64 end = w.a + w.len;
    if (w.L <= FQ_MAX_DNA) {
        const u64 o = FQ_HDR + s - w.a;                       // s >= a - (FQ_HDR - 1): inside the buffer
        const u32* p = reinterpret_cast<const u32*>(w.buf + (o & ~3ull));
        u32 x[9];
#pragma unroll
        for (int q = 0; q < 9; q++) x[q] = p[q];
        const u64 key = fq_pack_dna(x, (u32)(o & 3), end > s ? end - s : 0, w.L);
        if (key) { w.keys[r] = key; return; }
    }
    const u32 i = atomicAdd(&st->n_esc, 1u);
    if (i >= w.esc_cap) { atomicOr(&st->err, FQ_ERR_ESCAPES); return; }
    w.esc[i] = FqPend{s, r};
}
__device__ __forceinline__ void fq_seq_line(const FqWin& w, FqState* st, u64 s, u64 r) {
    const u64 need = w.L <= FQ_MAX_DNA ? w.L : FQ_HDR;        // bytes the device (DNA) or the host (escape string) must see
    if (!w.last && s + need > w.a + w.len) {
        const u32 i = atomicAdd(&st->n_pend[w.parity], 1u);
        if (i >= FQ_PEND_CAP) { atomicOr(&st->err, FQ_ERR_PENDING); return; }
        w.pend_out[i] = FqPend{s, r};
        return;
    }
    fq_resolve(w, st, s, r);
}

// the lines the window before handed on (one workgroup; runs after the scan emptied this window's lists)
__global__ __launch_bounds__(256) void fq_pending_kernel(FqWin w, FqState* __restrict__ st) {
    const u32 n = min(st->n_pend[w.parity ^ 1u], FQ_PEND_CAP);
    for (u32 i = threadIdx.x; i < n; i += 256) fq_resolve(w, st, w.pend_in[i].s, w.pend_in[i].r);
}

__global__ __launch_bounds__(256) void fq_emit_kernel(FqWin w, const u64* __restrict__ tile_base, const u64* __restrict__ tile_ls,
                                                      FqState* __restrict__ st) {
    __shared__ u64 sh[4];
    const u64 o = (u64)blockIdx.x * FQ_TILE + threadIdx.x * 16u;
    u32 m = fq_lane_mask(w.buf + FQ_HDR, o, w.len);
    const u64 last = m ? w.a + o + (31u - __clz(m)) + 1 : 0;
    u64 tot;
    const u64 j0 = tile_base[blockIdx.x] + fq_block_excl((u64)__popc(m), 0, FqAdd(), sh, &tot);
    u64 ls = max(tile_ls[blockIdx.x], fq_block_excl(last, 0, FqMax(), sh, &tot));
    u64 j = j0;
    while (m) {
        const u32 b = __ffs(m) - 1;
        m &= m - 1;
        const u64 p = w.a + o + b;                            // '\n' closing line j, which began at ls
        if (p + 1 - ls > FQ_MAX_LINE) { atomicOr(&st->err, FQ_ERR_LONG_LINE); atomicMin((unsigned long long*)&st->err_rec, (unsigned long long)(j >> 2)); }
        ls = p + 1;
        ++j;
        if ((j & 3) == 1) fq_seq_line(w, st, p + 1, j >> 2);
    }
}

// escape keys of the host into the key array
__global__ __launch_bounds__(256) void fq_scatter_kernel(u64* __restrict__ keys, u64 key_cap, const u64* __restrict__ rk, u64 n,
                                                         FqState* __restrict__ st) {
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) {
        const u64 r = rk[2 * i];
        if (r < key_cap) keys[r] = rk[2 * i + 1]; else atomicOr(&st->err, FQ_ERR_KEY_CAP);
    }
}

}  // namespace fastf

// ---- host side of the device parse (fastq_cmds.c drives it; host_io.h declares it) ----
struct fastf_fqparse {
    fastf_taghist* h = nullptr;
    int device = 0;
    size_t window = 0; u32 L = 0; u32 n_tiles_max = 0; u32 esc_cap = 0;
    DevBuf d_buf[2], d_pend[2], d_esc[2], d_state, d_tile_cnt, d_tile_last, d_tile_base, d_tile_ls, d_rk;
    FqState* h_snap = nullptr;                     // pinned: the state after the window of each parity
    fastf_fq_esc_t* h_esc = nullptr; size_t h_esc_cap = 0;     // pinned
    u64* h_rk = nullptr;                                        // pinned chunk of the escape keys' scatter
    hipStream_t s_d2h = nullptr;
    hipEvent_t ev_h2d0[2] = {}, ev_h2d1[2] = {}, ev_p0[2] = {}, ev_p1[2] = {};
    int submitted[2] = {0, 0};
    u32 next_parity = 0;
    u64 key_reserved = 0;                          // the last key_bound / key_cap the key array was reserved for
    u64 key_zeroed = 0;                            // fastf_fqparse_zero_keys: keys [0, key_zeroed) were cleared before any parse wrote there
};
static constexpr size_t FQ_RK_CHUNK = (size_t)1 << 20;

extern "C" void fastf_fqparse_destroy(fastf_fqparse_t* p) FASTF_TRY {
    if (!p) return;
    (void)hipSetDevice(p->device);
    (void)hipDeviceSynchronize();
    DevBuf* all[] = {&p->d_buf[0], &p->d_buf[1], &p->d_pend[0], &p->d_pend[1], &p->d_esc[0], &p->d_esc[1], &p->d_state,
                     &p->d_tile_cnt, &p->d_tile_last, &p->d_tile_base, &p->d_tile_ls, &p->d_rk};
    for (DevBuf* b : all) b->release();
    if (p->h_snap) (void)hipHostFree(p->h_snap);
    if (p->h_esc) (void)hipHostFree(p->h_esc);
    if (p->h_rk) (void)hipHostFree(p->h_rk);
    for (int i = 0; i < 2; i++)
        for (hipEvent_t e : {p->ev_h2d0[i], p->ev_h2d1[i], p->ev_p0[i], p->ev_p1[i]}) if (e) (void)hipEventDestroy(e);
    if (p->s_d2h) (void)hipStreamDestroy(p->s_d2h);
    delete p;
} FASTF_CATCH_VOID

extern "C" int fastf_fqparse_create(fastf_taghist_t* h, size_t window_bytes, uint32_t L, fastf_fqparse_t** out) FASTF_TRY {
    if (!h || !out || window_bytes < 4 * FQ_HDR) return set_err("fastf_fqparse_create: bad argument");
    *out = nullptr;
    fastf_fqparse* p = new fastf_fqparse();
    p->h = h; p->device = h->device; p->window = window_bytes; p->L = L > FQ_HDR ? FQ_HDR : L;
    p->n_tiles_max = (u32)((window_bytes + FQ_TILE - 1) / FQ_TILE);
    p->esc_cap = (u32)std::min<u64>(window_bytes / 4 + 2 * FQ_PEND_CAP, 0xffffffffull);
    auto fail = [&]() { fastf_fqparse_destroy(p); return 1; };
    if (hipSetDevice(p->device) != hipSuccess) { set_err("hipSetDevice failed"); return fail(); }
    for (int i = 0; i < 2; i++)
        if (p->d_buf[i].ensure(FQ_HDR + window_bytes + 64) || p->d_pend[i].ensure(FQ_PEND_CAP * sizeof(FqPend)) ||
            p->d_esc[i].ensure((size_t)p->esc_cap * sizeof(FqPend))) return fail();
    if (p->d_state.ensure(sizeof(FqState)) || p->d_tile_cnt.ensure(p->n_tiles_max * sizeof(u32)) ||
        p->d_tile_last.ensure(p->n_tiles_max * sizeof(u64)) || p->d_tile_base.ensure(p->n_tiles_max * sizeof(u64)) ||
        p->d_tile_ls.ensure(p->n_tiles_max * sizeof(u64)) || p->d_rk.ensure(FQ_RK_CHUNK * 2 * sizeof(u64))) return fail();
    if (hipHostMalloc((void**)&p->h_snap, 2 * sizeof(FqState), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&p->h_rk, FQ_RK_CHUNK * 2 * sizeof(u64), hipHostMallocDefault) != hipSuccess) {
        p->h_snap = nullptr; p->h_rk = nullptr; set_err("hipHostMalloc (fastq parse) failed"); return fail();
    }
    if (hipStreamCreateWithFlags(&p->s_d2h, hipStreamNonBlocking) != hipSuccess) { set_err("hipStreamCreate failed"); return fail(); }
    for (int i = 0; i < 2; i++)
        for (hipEvent_t* e : {&p->ev_h2d0[i], &p->ev_h2d1[i], &p->ev_p0[i], &p->ev_p1[i]})
            if (hipEventCreate(e) != hipSuccess) { *e = nullptr; set_err("hipEventCreate failed"); return fail(); }
    FqState st; memset(&st, 0, sizeof st); st.err_rec = ~0ull;
    if (copy_h2d(p->d_state.p, &st, sizeof st)) return fail();
    *out = p;
    return 0;
} FASTF_CATCH_INT

// Queue one window: H2D of staging[0 .. FQ_HDR + len) (pinned; FQ_HDR bytes of the previous window, then this window's len
// bytes, global offset a) on the copy stream, then count / scan / pending / emit on the histogram's stream.  Windows alternate
// between two parities; the staging and the escape list of a parity stay the caller's until fastf_fqparse_wait on it returned.
// key_bound: more reads than the run can have had by the end of this window.  Returns at once.
extern "C" int fastf_fqparse_submit(fastf_fqparse_t* p, const unsigned char* staging, size_t len, uint64_t a, int last,
                                    uint64_t key_bound) FASTF_TRY {
    if (!p || !staging || len > p->window) return set_err("fastf_fqparse_submit: bad argument");
    if (debug_known_memory(staging, FQ_HDR + len, "fastf_fqparse_submit")) return 1;
    const u32 par = p->next_parity;
    if (p->submitted[par]) return set_err("fastf_fqparse_submit: the window of parity %u was not waited for", par);
    HIP_OK(hipSetDevice(p->device));
    u64* keys = (u64*)fastf_taghist_reserve_device(p->h, key_bound);
    if (!keys) return 1;
    p->key_reserved = key_bound;
    hipStream_t sc = p->h->ws->s_compute, sy = p->h->ws->s_copy;
    HIP_OK(hipEventRecord(p->ev_h2d0[par], sy));
    HIP_OK(hipMemcpyAsync(p->d_buf[par].p, staging, FQ_HDR + len, hipMemcpyHostToDevice, sy));
    HIP_OK(hipEventRecord(p->ev_h2d1[par], sy));
    HIP_OK(hipStreamWaitEvent(sc, p->ev_h2d1[par], 0));
    HIP_OK(hipEventRecord(p->ev_p0[par], sc));
    FqWin w;
    w.buf = (const unsigned char*)p->d_buf[par].p; w.a = a; w.len = len; w.last = last ? 1 : 0; w.parity = par; w.L = p->L;
    w.keys = keys; w.key_cap = key_bound;
    w.pend_in = (FqPend*)p->d_pend[par ^ 1].p; w.pend_out = (FqPend*)p->d_pend[par].p; w.esc = (FqPend*)p->d_esc[par].p;
    w.esc_cap = p->esc_cap;
    FqState* st = (FqState*)p->d_state.p;
    const u32 n_tiles = (u32)((len + FQ_TILE - 1) / FQ_TILE);
    if (n_tiles) hipLaunchKernelGGL(fq_count_kernel, dim3(n_tiles), dim3(256), 0, sc, w.buf, (u64)len, (u32*)p->d_tile_cnt.p, (u64*)p->d_tile_last.p);
    hipLaunchKernelGGL(fq_scan_kernel, dim3(1), dim3(1024), 0, sc, n_tiles, (u64)a, (const u32*)p->d_tile_cnt.p, (const u64*)p->d_tile_last.p,
                       (u64*)p->d_tile_base.p, (u64*)p->d_tile_ls.p, st, par);
    hipLaunchKernelGGL(fq_pending_kernel, dim3(1), dim3(256), 0, sc, w, st);
    if (n_tiles) hipLaunchKernelGGL(fq_emit_kernel, dim3(n_tiles), dim3(256), 0, sc, w, (const u64*)p->d_tile_base.p, (const u64*)p->d_tile_ls.p, st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(&p->h_snap[par], st, sizeof(FqState), hipMemcpyDeviceToHost, sc));
    HIP_OK(hipEventRecord(p->ev_p1[par], sc));
    p->submitted[par] = 1;
    p->next_parity = par ^ 1;
    return 0;
} FASTF_CATCH_INT

// Wait for the window of this parity; *esc: its escapes (pinned host memory of the handle, valid until the next wait),
// *n_nl: '\n' up to the end of that window.  No-op (zero escapes) when nothing of that parity is in flight.
extern "C" int fastf_fqparse_wait(fastf_fqparse_t* p, int parity, const fastf_fq_esc_t** esc, uint32_t* n_esc, uint64_t* n_nl,
                                  double* h2d_ms, double* parse_ms) FASTF_TRY {
    if (!p || parity < 0 || parity > 1) return set_err("fastf_fqparse_wait: bad argument");
    *n_esc = 0; if (esc) *esc = p->h_esc;
    if (!p->submitted[parity]) return 0;
    HIP_OK(hipSetDevice(p->device));
    HIP_OK(hipEventSynchronize(p->ev_p1[parity]));
    p->submitted[parity] = 0;
    const FqState st = p->h_snap[parity];
    if (n_nl) *n_nl = st.n_nl;
    if (st.err & (FQ_ERR_PENDING | FQ_ERR_ESCAPES | FQ_ERR_KEY_CAP))
        return set_err("fastq parse: internal capacity exceeded (error bits %#x)", st.err);
    float ms = 0;
    if (h2d_ms && hipEventElapsedTime(&ms, p->ev_h2d0[parity], p->ev_h2d1[parity]) == hipSuccess) *h2d_ms += ms;
    if (parse_ms && hipEventElapsedTime(&ms, p->ev_p0[parity], p->ev_p1[parity]) == hipSuccess) *parse_ms += ms;
    const u32 n = st.n_esc;
    if (n) {
        if (n > p->h_esc_cap) {
            if (p->h_esc) (void)hipHostFree(p->h_esc);
            p->h_esc = nullptr; p->h_esc_cap = 0;
            const size_t cap = std::max<size_t>(n + n / 2, 1 << 16);
            HIP_OK(hipHostMalloc((void**)&p->h_esc, cap * sizeof(fastf_fq_esc_t), hipHostMallocDefault));
            p->h_esc_cap = cap;
        }
        HIP_OK(hipMemcpyAsync(p->h_esc, p->d_esc[parity].p, (size_t)n * sizeof(FqPend), hipMemcpyDeviceToHost, p->s_d2h));
        HIP_OK(hipStreamSynchronize(p->s_d2h));
    }
    if (esc) *esc = p->h_esc;
    *n_esc = n;
    return 0;
} FASTF_CATCH_INT

// after the last window: the carried state (every window waited for)
extern "C" int fastf_fqparse_end(fastf_fqparse_t* p, uint64_t* n_nl, uint64_t* line_start, uint32_t* err, uint64_t* err_rec) FASTF_TRY {
    if (!p) return set_err("null argument");
    HIP_OK(hipSetDevice(p->device));
    HIP_OK(hipStreamSynchronize(p->h->ws->s_compute));
    FqState st;
    if (copy_d2h(&st, p->d_state.p, sizeof st)) return 1;
    *n_nl = st.n_nl; *line_start = st.line_start; *err = st.err; *err_rec = st.err_rec;
    return 0;
} FASTF_CATCH_INT

// the escape keys: rk = n pairs (read, key), host memory of the caller's; through the handle's pinned chunk into the key array
extern "C" int fastf_fqparse_scatter(fastf_fqparse_t* p, const uint64_t* rk, size_t n, uint64_t key_cap) FASTF_TRY {
    if (!p || (!rk && n)) return set_err("null argument");
    HIP_OK(hipSetDevice(p->device));
    hipStream_t sc = p->h->ws->s_compute;
    u64* keys = (u64*)fastf_taghist_reserve_device(p->h, key_cap);
    if (!keys) return 1;
    p->key_reserved = key_cap;
    for (size_t o = 0; o < n; o += FQ_RK_CHUNK) {
        const size_t m = std::min(FQ_RK_CHUNK, n - o);
        HIP_OK(hipStreamSynchronize(sc));                     // the chunk buffers are free again
        memcpy(p->h_rk, rk + 2 * o, m * 2 * sizeof(u64));
        HIP_OK(hipMemcpyAsync(p->d_rk.p, p->h_rk, m * 2 * sizeof(u64), hipMemcpyHostToDevice, sc));
        hipLaunchKernelGGL(fq_scatter_kernel, dim3((u32)std::min<size_t>((m + 255) / 256, 2048)), dim3(256), 0, sc, keys, (u64)key_cap,
                           (const u64*)p->d_rk.p, (u64)m, (FqState*)p->d_state.p);
        HIP_OK(hipGetLastError());
    }
    HIP_OK(hipStreamSynchronize(sc));
    FqState st;
    if (copy_d2h(&st, p->d_state.p, sizeof st)) return 1;
    if (st.err & FQ_ERR_KEY_CAP) return set_err("fastq parse: escape key out of range");
    return 0;
} FASTF_CATCH_INT

// keys[r_lo .. r_lo + n) of the key array into dst (pinned or not), after everything queued on the histogram's stream; the
// range lies within the last key_bound / key_cap a submit or a scatter reserved (the tests' view of the per-read keys)
extern "C" int fastf_fqparse_fetch_keys(fastf_fqparse_t* p, uint64_t* dst, uint64_t r_lo, uint64_t n) FASTF_TRY {
    if (!p || (!dst && n)) return set_err("null argument");
    if (r_lo > p->key_reserved || n > p->key_reserved - r_lo)
        return set_err("fastf_fqparse_fetch_keys: reads [%llu, %llu + %llu) lie beyond the %llu keys reserved", (unsigned long long)r_lo,
                       (unsigned long long)r_lo, (unsigned long long)n, (unsigned long long)p->key_reserved);
    HIP_OK(hipSetDevice(p->device));
    HIP_OK(hipStreamSynchronize(p->h->ws->s_compute));
    if (n == 0) return 0;
    return copy_d2h(dst, (const u64*)p->h->d_k1.p + p->h->n + r_lo, (size_t)n * sizeof(u64));
} FASTF_CATCH_INT

// ---- the DNA-form keys alone (fqcells): a read that is not DNA-form keeps key 0, "absent", and nothing goes to the host ----
// Before fastf_fqparse_submit with the same key_bound: the keys up to key_bound that no earlier call cleared are set to 0 on the
// histogram's stream, so that a read the parse puts on the escape list leaves 0 in the key array (freq overwrites those slots with
// fastf_fqparse_scatter; here nobody does).  A growth of the key array carries the cleared keys along (th_grow keeps the reserved ones).
extern "C" int fastf_fqparse_zero_keys(fastf_fqparse_t* p, uint64_t key_bound) FASTF_TRY {
    if (!p) return set_err("null argument");
    HIP_OK(hipSetDevice(p->device));
    u64* keys = (u64*)fastf_taghist_reserve_device(p->h, key_bound);
    if (!keys) return 1;
    if (key_bound > p->key_zeroed) {
        HIP_OK(hipMemsetAsync(keys + p->key_zeroed, 0, (size_t)(key_bound - p->key_zeroed) * sizeof(u64), p->h->ws->s_compute));
        p->key_zeroed = key_bound;
    }
    return 0;
} FASTF_CATCH_INT

// fastf_fqparse_wait without the copy of the escape list: *n_esc = how many reads of that window were not DNA-form
extern "C" int fastf_fqparse_wait_count(fastf_fqparse_t* p, int parity, uint32_t* n_esc, uint64_t* n_nl, double* h2d_ms,
                                        double* parse_ms) FASTF_TRY {
    if (!p || !n_esc || parity < 0 || parity > 1) return set_err("fastf_fqparse_wait_count: bad argument");
    *n_esc = 0;
    if (!p->submitted[parity]) return 0;
    HIP_OK(hipSetDevice(p->device));
    HIP_OK(hipEventSynchronize(p->ev_p1[parity]));
    p->submitted[parity] = 0;
    const FqState st = p->h_snap[parity];
    if (n_nl) *n_nl = st.n_nl;
    if (st.err & (FQ_ERR_PENDING | FQ_ERR_ESCAPES | FQ_ERR_KEY_CAP))
        return set_err("fastq parse: internal capacity exceeded (error bits %#x)", st.err);
    float ms = 0;
    if (h2d_ms && hipEventElapsedTime(&ms, p->ev_h2d0[parity], p->ev_h2d1[parity]) == hipSuccess) *h2d_ms += ms;
    if (parse_ms && hipEventElapsedTime(&ms, p->ev_p0[parity], p->ev_p1[parity]) == hipSuccess) *parse_ms += ms;
    *n_esc = st.n_esc;
    return 0;
} FASTF_CATCH_INT
#endif
