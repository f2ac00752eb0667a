// filter_kernels.hpp — device side of `filter`: FASTQ text windows in HBM → record table → keep decision per
// read (R1) or from the keep bitmap (I1 / R2) → compacted "id seq +\n qual" text.  Part of the umi_engine.hip translation unit;
// count and scan of the newlines are freq's (fastq_kernels.hpp).
//
// Reference steps replaced (filter.c:15-60 get_fastq / get_comb_fastq, :228-241 in, :260-285 substring / combine_string,
// :286-350 fastF): four gzgets() lines per read, `(float) rand() / RAND_MAX < rate`, the whitelist tree lookup of the first
// len_cellbarcode bytes of the sequence line, and the "%s%s+\n%s" output of a kept read.
//
//   count / scan   freq's kernels: '\n' per 4 KiB tile, global line index of every tile, carried across windows in HBM
//   nl             every '\n' of the window at its line index (u32 buffer offset); lines longer than gzgets' 1023 bytes set
//                  the error word (first offending read by atomicMin)
//   draw           one lane per chunk of FLT_CHUNK reads: glibc's TYPE_3 rand() expanded from the chunk's start state (31 words,
//                  computed by the host with jump-ahead matrices), ring of 31 words per lane in LDS
//   rec            one lane per read whose last '\n' lies in the window: its four line starts (the newline positions of earlier
//                  windows come from the 4-entry carry), the output length, and the decision: R1 — the draw rule of the
//                  reference and the whitelist (DNA-form key → binary search of the sorted whitelist keys; anything else →
//                  escape list for the host); I1 / R2 — the keep bitmap
//   scan           exclusive sum of the kept lengths (three kernels), window total into the state
//   gather         16 lanes per read: id + seq, "+\n", qual into the compacted output window; R1 also sets the keep bitmap
//
// Every window is preceded in its buffer by the last FLT_HDR bytes of the window before: a record is at most 4 x 1023 bytes,
// so the record whose last '\n' lies in this window starts inside the buffer whenever no line is too long.
#pragma once
#include "fastq_kernels.hpp"

#define FLT_HDR 4096u                 /* bytes of the previous window in front of every window */
#define FLT_CHUNK 2048u               /* draws per lane of the draw kernel (= reads per host chunk state) */
#define FLT_RAND_DEG 31u
#define FLT_ERR_LONG_LINE 1u
#define FLT_ERR_REC_START 2u          /* a record begins before the buffer (only after a long line) */
#define FLT_ERR_ESCAPES 4u
#define FLT_SCAN_BLOCK 1024u

/* the reference's draw rule: (float) rand() / RAND_MAX < rate.  (float) RAND_MAX = 2^31 exactly, so the division is the exact
 * product with 2^-31; the int -> float conversion rounds to nearest even on the host and on the device alike */
FQ_HD int flt_draw_passes(uint32_t r, float rate)
{
    const float f = (float)(int32_t)r * 4.656612873077392578125e-10f;
    return f < rate;
}

#if defined(__HIPCC__)
namespace fastf {

struct FltState {
    u64 n0;                   // '\n' before the current window
    u64 carry[4];             // global offsets of the '\n' with index n0 - 4 .. n0 - 1, at slot index & 3
    u32 err, n_esc;
    u64 err_rec;              // first read with a line longer than FQ_MAX_LINE (or starting before the buffer)
    u64 total;                // output bytes of the current window
    u64 kept;                 // reads kept so far (R1)
};
struct FltRec { u32 s0, s1, s2, s3, e, olen; };   // buffer offsets of the four lines, end of the qual line, output bytes
struct FltEsc { u32 i, s1; };                     // record i of the window: its sequence line takes the host's path

struct FltWin {
    const unsigned char* buf; // FLT_HDR bytes of the previous window, then the window (slack behind)
    u64 a, len;               // global offset of buf[FLT_HDR]; bytes in the window (a virtual '\n' at `tv` included)
    u64 tv;                   // global offset of the virtual '\n' closing an unterminated last line; ~0: none
    u32* pos;                 // '\n' of the window: buffer offsets, by index - n0
    FltRec* rec; u32* len_out; u32* off_out;
    u64 r_lo, n_rec, limit;   // reads r_lo .. r_lo + n_rec - 1 end in this window; reads >= limit are not written
    // R1 decision
    int mode;                 // 0: R1 (draw + whitelist), 1: I1 / R2 (bitmap)
    int all; u32 L; float rate;
    const u32* draws;         // rand() outputs of reads r_lo ..
    const u64* wl; u64 n_wl;  // sorted DNA-form whitelist keys
    FltEsc* esc; u32 esc_cap;
    u32* bitmap;              // keep bit per read
    unsigned char* out; u64 out_cap;
};

__global__ __launch_bounds__(1) void flt_pre_kernel(const FqState* __restrict__ st, FltState* __restrict__ fs) {
    fs->n0 = st->n_nl;
    fs->n_esc = 0;
    fs->total = 0;
}

// every '\n' of the window at its index; the line-length check of gzgets(buf, 1024)
__global__ __launch_bounds__(256) void flt_nl_kernel(FltWin w, const u64* __restrict__ tile_base, const u64* __restrict__ tile_ls,
                                                     FltState* __restrict__ fs) {
    __shared__ u64 sh[4];
    const u64 o = (u64)blockIdx.x * FQ_TILE + threadIdx.x * 16u;
    u32 m = fq_lane_mask(w.buf + FLT_HDR, o, w.len);
    const u64 last = m ? w.a + o + (31u - __clz(m)) + 1 : 0;
    u64 tot;
    const u64 j0 = tile_base[blockIdx.x] + fq_block_excl((u64)__popc(m), 0, FqAdd(), sh, &tot);
    u64 ls = max(tile_ls[blockIdx.x], fq_block_excl(last, 0, FqMax(), sh, &tot));
    const u64 n0 = fs->n0;
    u64 j = j0;
    while (m) {
        const u32 b = __ffs(m) - 1;
        m &= m - 1;
        const u64 p = w.a + o + b;                            // '\n' closing line j, which began at ls
        const u64 line = p + (p == w.tv ? 0 : 1) - ls;        // bytes gzgets hands back for it
        if (line > FQ_MAX_LINE && (j >> 2) < w.limit) {
            atomicOr(&fs->err, FLT_ERR_LONG_LINE);
            atomicMin((unsigned long long*)&fs->err_rec, (unsigned long long)(j >> 2));
        }
        w.pos[j - n0] = (u32)(o + b + FLT_HDR);
        ls = p + 1;
        ++j;
    }
}

// buffer offset of the '\n' with index j (j >= n0 - 4); the carry holds global offsets
__device__ __forceinline__ u64 flt_nl_at(const FltWin& w, const FltState* fs, u64 n0, u64 j) {
    if (j >= n0) return w.pos[j - n0];
    return fs->carry[j & 3] + FLT_HDR - w.a;                 // wraps below zero only for a record that starts before the buffer
}

// the record of read r (its last '\n' lies in the window): buffer offsets of its four lines, the end of its qual line and its
// output bytes.  false: the read begins before the buffer (the error word is set, *rc stays as it was)
__device__ __forceinline__ bool flt_rec_lines(const FltWin& w, FltState* fs, u64 n0, u64 r, FltRec* rc) {
    const u64 buf_end = FLT_HDR + w.len;
    const u64 e0 = r ? flt_nl_at(w, fs, n0, 4 * r - 1) + 1 : FLT_HDR - w.a;   // read 0 begins at global offset 0 (a = 0)
    const u64 e1 = flt_nl_at(w, fs, n0, 4 * r) + 1, e2 = flt_nl_at(w, fs, n0, 4 * r + 1) + 1;
    const u64 e3 = flt_nl_at(w, fs, n0, 4 * r + 2) + 1, q = flt_nl_at(w, fs, n0, 4 * r + 3);
    if (e0 > buf_end || e1 > buf_end || e2 > buf_end || e3 > buf_end) {   // wrapped: begins before the buffer
        atomicOr(&fs->err, FLT_ERR_REC_START);
        atomicMin((unsigned long long*)&fs->err_rec, (unsigned long long)r);
        return false;
    }
    const u64 e = q + (q + w.a - FLT_HDR == w.tv ? 0 : 1);
    *rc = FltRec{(u32)e0, (u32)e1, (u32)e2, (u32)e3, (u32)e, (u32)((e2 - e0) + 2 + (e - e3))};
    return true;
}

// the DNA-form key of the first w.L bytes of the record's sequence line; 0: the read takes the escape path
__device__ __forceinline__ u64 flt_rec_key(const FltWin& w, const FltRec& rc) {
    if (w.L > FQ_MAX_DNA) return 0;
    const u32* p = reinterpret_cast<const u32*>(w.buf + (rc.s1 & ~3u));
    u32 x[9];
#pragma unroll
    for (int t = 0; t < 9; t++) x[t] = p[t];
    return fq_pack_dna(x, rc.s1 & 3u, rc.s2 - rc.s1, w.L);
}

// where `key` stands among the sorted whitelist keys; w.n_wl: it is not among them
__device__ __forceinline__ u64 flt_wl_find(const FltWin& w, u64 key) {
    u64 lo = 0, hi = w.n_wl;
    while (lo < hi) { const u64 mid = (lo + hi) >> 1; if (w.wl[mid] < key) lo = mid + 1; else hi = mid; }
    return lo < w.n_wl && w.wl[lo] == key ? lo : w.n_wl;
}

// record i of the window (sequence line at buffer offset s1) onto the host's list
__device__ __forceinline__ void flt_escape(const FltWin& w, FltState* fs, u32 i, u32 s1) {
    const u32 k = atomicAdd(&fs->n_esc, 1u);
    if (k < w.esc_cap) w.esc[k] = FltEsc{i, s1};
    else atomicOr(&fs->err, FLT_ERR_ESCAPES);
}

// one lane per read of the window: the record table, its output length and its keep decision
__global__ __launch_bounds__(256) void flt_rec_kernel(FltWin w, FltState* __restrict__ fs) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= w.n_rec) return;
    const u64 r = w.r_lo + i;
    const u64 n0 = fs->n0;
    u32 keep = 0;
    FltRec rc = {0, 0, 0, 0, 0, 0};
    if (r < w.limit && flt_rec_lines(w, fs, n0, r, &rc)) {
        if (w.mode == 1) {
            keep = (w.bitmap[r >> 5] >> (r & 31)) & 1u;
        } else if (flt_draw_passes(w.draws[i], w.rate)) {
            if (w.all) keep = 1;
            else {
                const u64 key = flt_rec_key(w, rc);
                if (key) keep = flt_wl_find(w, key) < w.n_wl;
                else flt_escape(w, fs, (u32)i, rc.s1);
            }
        }
    }
    w.rec[i] = rc;
    w.len_out[i] = keep ? rc.olen : 0u;
}

// the host's verdict on escapes: records hit[0 .. n) of the window are kept
__global__ __launch_bounds__(256) void flt_hit_kernel(FltWin w, const u32* __restrict__ hit, u32 n) {
    const u32 k = blockIdx.x * 256 + threadIdx.x;
    if (k < n) { const u32 i = hit[k]; if (i < w.n_rec) w.len_out[i] = w.rec[i].olen; }
}

// exclusive scan of len_out[0 .. n): block sums, one workgroup over the sums, block offsets
__device__ __forceinline__ u64 flt_block_excl1024(u64 v, u64* sh, u64* total) {
    const u32 lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const u64 inc = fq_wave_incl(v, FqAdd());
    if (lane == 63) sh[wv] = inc;
    __syncthreads();
    u64 before = 0, all = 0;
    for (u32 k = 0; k < 16; k++) { if (k < wv) before += sh[k]; all += sh[k]; }
    __syncthreads();
    *total = all;
    return before + inc - v;
}
__global__ __launch_bounds__(1024) void flt_sum_kernel(const u32* __restrict__ len, u64 n, u64* __restrict__ bsum) {
    __shared__ u64 sh[16];
    const u64 i = (u64)blockIdx.x * FLT_SCAN_BLOCK + threadIdx.x;
    u64 tot;
    (void)flt_block_excl1024(i < n ? len[i] : 0, sh, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}
__global__ __launch_bounds__(1024) void flt_sums_scan_kernel(u64* __restrict__ bsum, u32 nb, FltState* __restrict__ fs) {
    __shared__ u64 sh[16];
    const u32 per = (nb + 1023) / 1024, lo = min(nb, threadIdx.x * per), hi = min(nb, lo + per);
    u64 c = 0;
    for (u32 k = lo; k < hi; k++) c += bsum[k];
    u64 tot;
    u64 base = flt_block_excl1024(c, sh, &tot);
    for (u32 k = lo; k < hi; k++) { const u64 v = bsum[k]; bsum[k] = base; base += v; }
    if (threadIdx.x == 0) fs->total = tot;
}
__global__ __launch_bounds__(1024) void flt_off_kernel(const u32* __restrict__ len, u64 n, const u64* __restrict__ bsum,
                                                       u32* __restrict__ off) {
    __shared__ u64 sh[16];
    const u64 i = (u64)blockIdx.x * FLT_SCAN_BLOCK + threadIdx.x;
    u64 tot;
    const u64 ex = flt_block_excl1024(i < n ? len[i] : 0, sh, &tot);
    if (i < n) off[i] = (u32)(bsum[blockIdx.x] + ex);
}

// 16 lanes per read: its output bytes, coalesced across the lanes of a group; the first lane sets the read's keep bit (R1)
__global__ __launch_bounds__(256) void flt_gather_kernel(FltWin w, FltState* __restrict__ fs) {
    const u64 i = (u64)blockIdx.x * 16 + (threadIdx.x >> 4);
    const u32 g = threadIdx.x & 15;
    if (i >= w.n_rec) return;
    const u32 n = w.len_out[i];
    if (!n) return;
    const FltRec rc = w.rec[i];
    if ((u64)w.off_out[i] + n > w.out_cap) { if (g == 0) atomicOr(&fs->err, FLT_ERR_ESCAPES); return; }
    unsigned char* o = w.out + w.off_out[i];
    const u32 n1 = rc.s2 - rc.s0, n3 = rc.e - rc.s3;         // id + seq; qual
    for (u32 k = g; k < n1; k += 16) o[k] = w.buf[rc.s0 + k];
    if (g == 0) { o[n1] = '+'; o[n1 + 1] = '\n'; }
    for (u32 k = g; k < n3; k += 16) o[n1 + 2 + k] = w.buf[rc.s3 + k];
    if (w.mode == 0 && g == 0) {
        const u64 r = w.r_lo + i;
        atomicOr(&w.bitmap[r >> 5], 1u << (r & 31));
        atomicAdd((unsigned long long*)&fs->kept, 1ull);
    }
}

// after the window: the last four '\n' seen so far move into the carry
__global__ __launch_bounds__(1) void flt_carry_kernel(FltWin w, const FqState* __restrict__ st, FltState* __restrict__ fs) {
    const u64 n0 = fs->n0, n1 = st->n_nl;
    for (u64 j = n1 > 4 ? n1 - 4 : 0; j < n1; j++)
        if (j >= n0) fs->carry[j & 3] = w.a + (u64)w.pos[j - n0] - FLT_HDR;
}

// glibc rand(): lane c expands chunk c (FLT_CHUNK outputs) from its start state cs[c * 31 ..] — the words r_{q+344 .. q+374} of
// the recurrence r_i = r_{i-3} + r_{i-31} (mod 2^32), whose outputs are r_i >> 1
__global__ __launch_bounds__(256) void flt_draw_kernel(const u32* __restrict__ cs, u64 n, u32* __restrict__ out) {
    __shared__ u32 ring[FLT_RAND_DEG * 256];
    const u32 t = threadIdx.x;
    const u64 c = (u64)blockIdx.x * 256 + t;
    const u64 lo = c * FLT_CHUNK;
    if (lo >= n) return;
    for (u32 k = 0; k < FLT_RAND_DEG; k++) ring[k * 256 + t] = cs[c * FLT_RAND_DEG + k];
    const u32 m = (u32)min((u64)FLT_CHUNK, n - lo);
    u32 a = 0, b = 28;
    for (u32 u = 0; u < m; u++) {
        const u32 x = ring[a * 256 + t], y = ring[b * 256 + t];
        out[lo + u] = x >> 1;
        ring[a * 256 + t] = x + y;
        a = a == FLT_RAND_DEG - 1 ? 0 : a + 1;
        b = b == FLT_RAND_DEG - 1 ? 0 : b + 1;
    }
}

}  // namespace fastf
#endif

#if defined(__HIPCC__)
// ---- host side of the device path (filter_cmds.c drives it; host_io.h declares it) ----
struct fastf_fltdev {
    int device = 0;
    size_t window = 0; u32 n_tiles_max = 0; u64 rec_cap = 0;
    DevBuf d_buf, d_state, d_fstate, d_tile_cnt, d_tile_last, d_tile_base, d_tile_ls, d_pos, d_rec, d_len, d_off, d_bsum,
           d_draws, d_cs, d_esc, d_hit, d_wl, d_bitmap, d_out;
    DevBuf d_hits, d_kept, d_cellrate;              // fqcap (fqcap_kernels.hpp): per whitelist key, guard words behind
    u64 n_wl = 0, bitmap_words = 0, fcp_keys = ~0ull;   // fcp_keys: the key count hits / kept / rate were sized for
    unsigned char* h_out = nullptr;                 // pinned: the compacted window
    FltEsc* h_esc = nullptr;                        // pinned
    FqState* h_st = nullptr; FltState* h_fs = nullptr;   // pinned snapshots
    hipStream_t s = nullptr;
    hipEvent_t ev[2] = {};
    FltWin w{};
    double dev_ms = 0;
};

extern "C" void fastf_fltdev_destroy(fastf_fltdev_t* p) FASTF_TRY {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->s) (void)hipStreamSynchronize(p->s);
    DevBuf* all[] = {&p->d_buf, &p->d_state, &p->d_fstate, &p->d_tile_cnt, &p->d_tile_last, &p->d_tile_base, &p->d_tile_ls, &p->d_pos,
                     &p->d_rec, &p->d_len, &p->d_off, &p->d_bsum, &p->d_draws, &p->d_cs, &p->d_esc, &p->d_hit, &p->d_wl,
                     &p->d_bitmap, &p->d_out, &p->d_hits, &p->d_kept, &p->d_cellrate};
    for (DevBuf* b : all) b->release();
    if (p->h_out) (void)hipHostFree(p->h_out);
    if (p->h_esc) (void)hipHostFree(p->h_esc);
    if (p->h_st) (void)hipHostFree(p->h_st);
    if (p->h_fs) (void)hipHostFree(p->h_fs);
    for (hipEvent_t e : p->ev) if (e) (void)hipEventDestroy(e);
    if (p->s) (void)hipStreamDestroy(p->s);
    delete p;
} FASTF_CATCH_VOID

static size_t flt_out_cap(size_t window) { return window + window / 4 + FLT_HDR + 64; }

extern "C" int fastf_fltdev_create(int device, size_t window_bytes, fastf_fltdev_t** out) FASTF_TRY {
    if (!out || window_bytes < FLT_HDR || window_bytes > ((size_t)1 << 30)) return set_err("fastf_fltdev_create: bad argument");
    *out = nullptr;
    fastf_fltdev* p = new fastf_fltdev();
    p->device = device; p->window = window_bytes;
    const size_t wb = window_bytes + 1;                       // + the virtual '\n' of an unterminated last line
    p->n_tiles_max = (u32)((wb + FQ_TILE - 1) / FQ_TILE);
    p->rec_cap = wb / 4 + 2;
    auto fail = [&]() { fastf_fltdev_destroy(p); return 1; };
    if (hipSetDevice(device) != hipSuccess) { set_err("hipSetDevice failed"); return fail(); }
    const u64 nb = (p->rec_cap + FLT_SCAN_BLOCK - 1) / FLT_SCAN_BLOCK;
    const u64 nch = (p->rec_cap + FLT_CHUNK - 1) / FLT_CHUNK;
    if (p->d_buf.ensure(FLT_HDR + wb + 128) || p->d_state.ensure(sizeof(FqState)) || p->d_fstate.ensure(sizeof(FltState)) ||
        p->d_tile_cnt.ensure(p->n_tiles_max * sizeof(u32)) || p->d_tile_last.ensure(p->n_tiles_max * sizeof(u64)) ||
        p->d_tile_base.ensure(p->n_tiles_max * sizeof(u64)) || p->d_tile_ls.ensure(p->n_tiles_max * sizeof(u64)) ||
        p->d_pos.ensure((wb + 1) * sizeof(u32)) || p->d_rec.ensure(p->rec_cap * sizeof(FltRec)) ||
        p->d_len.ensure(p->rec_cap * sizeof(u32)) || p->d_off.ensure(p->rec_cap * sizeof(u32)) || p->d_bsum.ensure(nb * sizeof(u64)) ||
        p->d_draws.ensure(p->rec_cap * sizeof(u32)) || p->d_cs.ensure(nch * FLT_RAND_DEG * sizeof(u32)) ||
        p->d_esc.ensure(p->rec_cap * sizeof(FltEsc)) || p->d_hit.ensure(p->rec_cap * sizeof(u32)) ||
        p->d_out.ensure(flt_out_cap(window_bytes)) || p->d_wl.ensure(sizeof(u64)) || p->d_bitmap.ensure(1 << 20)) return fail();
    p->bitmap_words = (1 << 20) / 4;
    if (hipMemset(p->d_bitmap.p, 0, 1 << 20) != hipSuccess) { set_err("hipMemset failed"); return fail(); }
    if (hipHostMalloc((void**)&p->h_out, flt_out_cap(window_bytes), hipHostMallocDefault) != hipSuccess) { p->h_out = nullptr; set_err("hipHostMalloc (filter) failed"); return fail(); }
    if (hipHostMalloc((void**)&p->h_esc, p->rec_cap * sizeof(FltEsc), hipHostMallocDefault) != hipSuccess) { p->h_esc = nullptr; set_err("hipHostMalloc (filter) failed"); return fail(); }
    if (hipHostMalloc((void**)&p->h_st, sizeof(FqState), hipHostMallocDefault) != hipSuccess) { p->h_st = nullptr; set_err("hipHostMalloc (filter) failed"); return fail(); }
    if (hipHostMalloc((void**)&p->h_fs, sizeof(FltState), hipHostMallocDefault) != hipSuccess) { p->h_fs = nullptr; set_err("hipHostMalloc (filter) failed"); return fail(); }
    if (hipStreamCreateWithFlags(&p->s, hipStreamNonBlocking) != hipSuccess) { p->s = nullptr; set_err("hipStreamCreate failed"); return fail(); }
    for (hipEvent_t& e : p->ev) if (hipEventCreate(&e) != hipSuccess) { e = nullptr; set_err("hipEventCreate failed"); return fail(); }
    *out = p;
    return 0;
} FASTF_CATCH_INT

// the sorted DNA-form keys of the whitelist (host memory of the caller's)
extern "C" int fastf_fltdev_set_whitelist(fastf_fltdev_t* p, const uint64_t* keys, size_t n) FASTF_TRY {
    if (!p || (!keys && n)) return set_err("null argument");
    HIP_OK(hipSetDevice(p->device));
    if (p->d_wl.ensure((n ? n : 1) * sizeof(u64))) return 1;
    if (n && copy_h2d(p->d_wl.p, keys, n * sizeof(u64))) return 1;
    p->n_wl = n;
    return 0;
} FASTF_CATCH_INT

// a new file: no '\n' seen, no carry
extern "C" int fastf_fltdev_reset(fastf_fltdev_t* p) FASTF_TRY {
    if (!p) return set_err("null argument");
    HIP_OK(hipSetDevice(p->device));
    HIP_OK(hipStreamSynchronize(p->s));
    FqState st; memset(&st, 0, sizeof st); st.err_rec = ~0ull;
    FltState fs; memset(&fs, 0, sizeof fs); fs.err_rec = ~0ull;
    if (copy_h2d(p->d_state.p, &st, sizeof st) || copy_h2d(p->d_fstate.p, &fs, sizeof fs)) return 1;
    p->dev_ms = 0;
    return 0;
} FASTF_CATCH_INT

static int flt_sync(fastf_fltdev* p) {
    HIP_OK(hipEventRecord(p->ev[1], p->s));
    HIP_OK(hipEventSynchronize(p->ev[1]));
    float ms = 0;
    if (hipEventElapsedTime(&ms, p->ev[0], p->ev[1]) == hipSuccess) p->dev_ms += ms;
    return 0;
}

// One window: staging[0 .. FLT_HDR + len) (pinned: the last FLT_HDR bytes of the window before, then this one's len bytes, a
// virtual '\n' at global offset tv included when tv != ~0) at global offset a.  Frames it on the device and returns the reads
// whose last '\n' lies in it: r_lo .. r_lo + n_rec - 1.  limit: reads from there on are not checked or written.
extern "C" int fastf_fltdev_parse(fastf_fltdev_t* p, const unsigned char* staging, size_t len, uint64_t a, uint64_t tv, uint64_t limit,
                                  uint64_t* r_lo, uint64_t* n_rec) FASTF_TRY {
    if (!p || !staging || len > p->window + 1) return set_err("fastf_fltdev_parse: bad argument");
    HIP_OK(hipSetDevice(p->device));
    hipStream_t s = p->s;
    HIP_OK(hipEventRecord(p->ev[0], s));
    HIP_OK(hipMemcpyAsync(p->d_buf.p, staging, FLT_HDR + len, hipMemcpyHostToDevice, s));
    FqState* st = (FqState*)p->d_state.p;
    FltState* fs = (FltState*)p->d_fstate.p;
    FltWin& w = p->w;
    memset(&w, 0, sizeof w);
    w.buf = (const unsigned char*)p->d_buf.p; w.a = a; w.len = len; w.tv = tv; w.limit = limit;
    w.pos = (u32*)p->d_pos.p; w.rec = (FltRec*)p->d_rec.p; w.len_out = (u32*)p->d_len.p; w.off_out = (u32*)p->d_off.p;
    w.draws = (const u32*)p->d_draws.p; w.wl = (const u64*)p->d_wl.p; w.n_wl = p->n_wl;
    w.esc = (FltEsc*)p->d_esc.p; w.esc_cap = (u32)p->rec_cap; w.out = (unsigned char*)p->d_out.p; w.out_cap = flt_out_cap(p->window);
    const u32 n_tiles = (u32)((len + FQ_TILE - 1) / FQ_TILE);
    hipLaunchKernelGGL(flt_pre_kernel, dim3(1), dim3(1), 0, s, (const FqState*)st, fs);
    // fq_count / fq_scan index the window from buf + FQ_HDR: hand them the buffer shifted so that its window starts there
    const unsigned char* base = w.buf + FLT_HDR - FQ_HDR;
    if (n_tiles) hipLaunchKernelGGL(fq_count_kernel, dim3(n_tiles), dim3(256), 0, s, base, (u64)len, (u32*)p->d_tile_cnt.p, (u64*)p->d_tile_last.p);
    hipLaunchKernelGGL(fq_scan_kernel, dim3(1), dim3(1024), 0, s, n_tiles, (u64)a, (const u32*)p->d_tile_cnt.p, (const u64*)p->d_tile_last.p,
                       (u64*)p->d_tile_base.p, (u64*)p->d_tile_ls.p, st, 0u);
    if (n_tiles) hipLaunchKernelGGL(flt_nl_kernel, dim3(n_tiles), dim3(256), 0, s, w, (const u64*)p->d_tile_base.p, (const u64*)p->d_tile_ls.p, fs);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(p->h_st, st, sizeof(FqState), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(p->h_fs, fs, sizeof(FltState), hipMemcpyDeviceToHost, s));
    if (flt_sync(p)) return 1;
    const u64 n0 = p->h_fs->n0, n1 = p->h_st->n_nl;
    w.r_lo = n0 / 4; w.n_rec = n1 / 4 - n0 / 4;
    if (w.n_rec > p->rec_cap) return set_err("filter: %llu reads end in one window (capacity %llu)", (unsigned long long)w.n_rec, (unsigned long long)p->rec_cap);
    *r_lo = w.r_lo; *n_rec = w.n_rec;
    return 0;
} FASTF_CATCH_INT

static int flt_bitmap_cover(fastf_fltdev* p, u64 reads) {
    const u64 need = (reads + 31) / 32 + 1;
    if (need <= p->bitmap_words) return 0;
    u64 nw = p->bitmap_words;
    while (nw < need) nw *= 2;
    DevBuf nb;
    if (nb.ensure(nw * 4)) return 1;
    HIP_OK(hipMemsetAsync(nb.p, 0, nw * 4, p->s));
    HIP_OK(hipMemcpyAsync(nb.p, p->d_bitmap.p, p->bitmap_words * 4, hipMemcpyDeviceToDevice, p->s));
    HIP_OK(hipStreamSynchronize(p->s));
    p->d_bitmap.release();
    p->d_bitmap = nb;
    nb.p = nullptr; nb.bytes = 0;
    p->bitmap_words = nw;
    return 0;
}

// The decisions of the parsed window.  mode 0 (R1): cs = the start states of its ceil(n_rec / FLT_CHUNK) draw chunks (31 words
// each, the first at read r_lo); *esc / *n_esc: the reads whose barcode the host decides (pinned, valid until the next call).
// mode 1 (I1 / R2): the keep bitmap decides.
// (launch_rec: the record kernel of the window onto the stream — filter's here, fqcap's in fqcap_kernels.hpp)
template <typename LaunchRec>
static int flt_decide_with(fastf_fltdev* p, int mode, int all, uint32_t L, float rate, const uint32_t* cs,
                           const fastf_flt_esc_t** esc, uint32_t* n_esc, LaunchRec launch_rec) {
    if (!p || !n_esc) return set_err("null argument");
    HIP_OK(hipSetDevice(p->device));
    FltWin& w = p->w;
    hipStream_t s = p->s;
    FltState* fs = (FltState*)p->d_fstate.p;
    *n_esc = 0; if (esc) *esc = (const fastf_flt_esc_t*)p->h_esc;
    w.mode = mode; w.all = all; w.L = L; w.rate = rate;
    if (flt_bitmap_cover(p, w.r_lo + w.n_rec)) return 1;
    w.bitmap = (u32*)p->d_bitmap.p;
    if (!w.n_rec) return 0;
    HIP_OK(hipEventRecord(p->ev[0], s));
    if (mode == 0) {
        const u64 nch = (w.n_rec + FLT_CHUNK - 1) / FLT_CHUNK;
        HIP_OK(hipMemcpyAsync(p->d_cs.p, cs, nch * FLT_RAND_DEG * sizeof(u32), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(flt_draw_kernel, dim3((u32)((nch + 255) / 256)), dim3(256), 0, s, (const u32*)p->d_cs.p, w.n_rec, (u32*)p->d_draws.p);
    }
    launch_rec(w, fs, dim3((u32)((w.n_rec + 255) / 256)), s);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(p->h_fs, fs, sizeof(FltState), hipMemcpyDeviceToHost, s));
    if (flt_sync(p)) return 1;
    const FltState f = *p->h_fs;
    if (f.err & FLT_ERR_ESCAPES) return set_err("filter: escape list overflow");
    if (f.n_esc) {
        HIP_OK(hipMemcpyAsync(p->h_esc, p->d_esc.p, (size_t)f.n_esc * sizeof(FltEsc), hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
    }
    *n_esc = f.n_esc;
    return 0;
}

extern "C" int fastf_fltdev_decide(fastf_fltdev_t* p, int mode, int all, uint32_t L, float rate, const uint32_t* cs,
                                   const fastf_flt_esc_t** esc, uint32_t* n_esc) FASTF_TRY {
    return flt_decide_with(p, mode, all, L, rate, cs, esc, n_esc, [](const FltWin& w, FltState* fs, dim3 grid, hipStream_t s) {
        hipLaunchKernelGGL(flt_rec_kernel, grid, dim3(256), 0, s, w, fs);
    });
} FASTF_CATCH_INT

// The window's output: the host's hits (reads i of the window, pinned or not) join the kept reads; then scan, gather and the
// carry.  *out: the compacted text (pinned, valid until the next window), *total its bytes.
extern "C" int fastf_fltdev_emit(fastf_fltdev_t* p, const uint32_t* hit, uint32_t n_hit, const unsigned char** out, size_t* total) FASTF_TRY {
    if (!p || (!hit && n_hit)) return set_err("null argument");
    HIP_OK(hipSetDevice(p->device));
    FltWin& w = p->w;
    hipStream_t s = p->s;
    FltState* fs = (FltState*)p->d_fstate.p;
    *out = p->h_out; *total = 0;
    HIP_OK(hipEventRecord(p->ev[0], s));
    if (n_hit) {
        if (copy_h2d_on(p->d_hit.p, hit, (size_t)n_hit * sizeof(u32), s)) return 1;
        hipLaunchKernelGGL(flt_hit_kernel, dim3((n_hit + 255) / 256), dim3(256), 0, s, w, (const u32*)p->d_hit.p, n_hit);
    }
    if (w.n_rec) {
        const u32 nb = (u32)((w.n_rec + FLT_SCAN_BLOCK - 1) / FLT_SCAN_BLOCK);
        hipLaunchKernelGGL(flt_sum_kernel, dim3(nb), dim3(1024), 0, s, (const u32*)p->d_len.p, w.n_rec, (u64*)p->d_bsum.p);
        hipLaunchKernelGGL(flt_sums_scan_kernel, dim3(1), dim3(1024), 0, s, (u64*)p->d_bsum.p, nb, fs);
        hipLaunchKernelGGL(flt_off_kernel, dim3(nb), dim3(1024), 0, s, (const u32*)p->d_len.p, w.n_rec, (const u64*)p->d_bsum.p, (u32*)p->d_off.p);
        hipLaunchKernelGGL(flt_gather_kernel, dim3((u32)((w.n_rec + 15) / 16)), dim3(256), 0, s, w, fs);
    }
    hipLaunchKernelGGL(flt_carry_kernel, dim3(1), dim3(1), 0, s, w, (const FqState*)p->d_state.p, fs);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(p->h_fs, fs, sizeof(FltState), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    const u64 t = w.n_rec ? p->h_fs->total : 0;
    if (t > flt_out_cap(p->window) || (p->h_fs->err & FLT_ERR_ESCAPES)) return set_err("filter: output window overflow");
    if (t) HIP_OK(hipMemcpyAsync(p->h_out, p->d_out.p, t, hipMemcpyDeviceToHost, s));
    if (flt_sync(p)) return 1;
    *total = t;
    return 0;
} FASTF_CATCH_INT

// after the last window of a file: '\n' seen, reads kept (R1), error word and first offending read; *dev_ms: device time of the file (events around each step)
extern "C" int fastf_fltdev_end(fastf_fltdev_t* p, uint64_t* n_nl, uint64_t* kept, uint32_t* err, uint64_t* err_rec, double* dev_ms) FASTF_TRY {
    if (!p) return set_err("null argument");
    HIP_OK(hipSetDevice(p->device));
    HIP_OK(hipStreamSynchronize(p->s));
    FqState st; FltState fs;
    if (copy_d2h(&st, p->d_state.p, sizeof st) || copy_d2h(&fs, p->d_fstate.p, sizeof fs)) return 1;
    *n_nl = st.n_nl; *kept = fs.kept; *err = fs.err | (st.err & FQ_ERR_LONG_LINE ? FLT_ERR_LONG_LINE : 0); *err_rec = fs.err_rec;
    if (dev_ms) *dev_ms = p->dev_ms;
    return 0;
} FASTF_CATCH_INT

// n rand() outputs from the chunk start states cs (ceil(n / FLT_CHUNK) x 31 words) into out (host memory of the caller's)
extern "C" int fastf_flt_draws_dev(int device, const uint32_t* cs, uint64_t n, uint32_t* out) FASTF_TRY {
    if (!cs || !out) return set_err("null argument");
    HIP_OK(hipSetDevice(device));
    if (!n) return 0;
    const u64 nch = (n + FLT_CHUNK - 1) / FLT_CHUNK;
    DevBuf d_cs, d_out;
    if (d_cs.ensure(nch * FLT_RAND_DEG * sizeof(u32)) || d_out.ensure(n * sizeof(u32))) { d_cs.release(); d_out.release(); return 1; }
    int rc = copy_h2d(d_cs.p, cs, nch * FLT_RAND_DEG * sizeof(u32));
    if (!rc) {
        hipLaunchKernelGGL(flt_draw_kernel, dim3((u32)((nch + 255) / 256)), dim3(256), 0, 0, (const u32*)d_cs.p, (u64)n, (u32*)d_out.p);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = set_err("filter draw kernel failed");
    }
    if (!rc) rc = copy_d2h(out, d_out.p, n * sizeof(u32));
    d_cs.release(); d_out.release();
    return rc;
} FASTF_CATCH_INT
#endif
