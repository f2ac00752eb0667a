"""Host-side mirror of the engine C ABI (include/fastf_amd.h).

Nothing here computes results: every call lands in libfastf_amd.so (HIP kernels on the
device, C on the host).  If the library or a HIP device is missing the calls raise.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Batch, Coo, EngineConfig, FastfError, ListsStruct, MT, UmiRows, check

HAS_CB, HAS_XF, HAS_GX, HAS_UB = 1, 2, 4, 8


def draw_threshold(rate_depth: float) -> int:
    """Integer form of bam2db_ds.c:385-390: a record is kept iff draw < threshold."""
    return int(_lib.lib().fastf_draw_threshold(C.c_float(rate_depth)))


def mt_draws(seed: int, skip: int, n: int) -> np.ndarray:
    """n MT19937 draws after init_genrand(seed) and `skip` discarded draws."""
    L = _lib.lib()
    mt = MT()
    L.fastf_mt_seed(C.byref(mt), seed)
    L.fastf_mt_skip(C.byref(mt), skip)
    out = np.empty(n, dtype=np.uint32)
    L.fastf_mt_fill(C.byref(mt), out.ctypes.data, n)
    return out


def sample_cells(n_cells: int, rate_cell: float, seed: int):
    L = _lib.lib()
    out = np.zeros(max(n_cells, 1), dtype=np.uint64)
    ns, used = C.c_size_t(0), C.c_uint64(0)
    rc = L.fastf_sample_cells(n_cells, C.c_float(rate_cell), seed, out.ctypes.data, C.byref(ns), C.byref(used))
    if rc:
        raise FastfError("sample size must lie in [0, n_cells]")
    return out[:ns.value].copy(), int(used.value)


class Lists:
    """Barcode + feature lists as the reference builds them (bam2db_ds.c:229-337)."""

    def __init__(self, barcodes: bytes, features: bytes, rate_cell=1.0, seed=926):
        self._L = _lib.lib()
        self._s = ListsStruct()
        check(self._L.fastf_lists_load_mem(barcodes, len(barcodes), features, len(features),
                                           C.c_float(rate_cell), seed, C.byref(self._s)))
        s = self._s
        self.n_lines_barcodes = s.n_lines_barcodes
        self.n_sampled_target = s.n_sampled_target
        self.n_cells = s.n_cells
        self.n_features = s.n_features
        self.mt_skip = int(s.mt_skip)
        self.dup_barcodes, self.dup_features = s.dup_barcodes, s.dup_features
        self.cell_keys = np.array([s.cell_key[i] for i in range(s.n_cells)], dtype=np.uint64)
        self.feature_keys = np.array([s.feature_key[i] for i in range(s.n_features)], dtype=np.uint64)
        self.barcodes = [s.barcode[i] for i in range(s.n_cells)]
        self.features = [(s.feat_id[i], s.feat_name[i], s.feat_type[i]) for i in range(s.n_features)]

    @property
    def cell_dict(self):
        return self._s.cell_dict

    @property
    def feat_dict(self):
        return self._s.feat_dict

    def barcodes_text(self) -> bytes:
        return b"".join(b + b"\n" for b in self.barcodes)

    def features_text(self) -> bytes:
        return b"".join(b"\t".join(f) + b"\n" for f in self.features)

    def close(self):
        if self._s is not None:
            self._L.fastf_lists_free(C.byref(self._s))
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_records(lists: Lists, flags, xf, cb, gx, ub, long_umis=False):
    """String-level records → packed SoA via the product's own packer (host_io.c).  long_umis: UMIs of up to 32 bases, a
    fifth array (bases 17..) is returned behind the four"""
    L = _lib.lib()
    if long_umis:
        L.fastf_pack_records_ext.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fastf_pack_records_ext.restype = None
        flags = np.ascontiguousarray(flags, dtype=np.uint8); xf = np.ascontiguousarray(xf, dtype=np.int32)
        cb, gx, ub = (np.ascontiguousarray(a) for a in (cb, gx, ub))
        n = len(flags)
        out = (np.empty(n, np.uint64), np.empty(n, np.uint64), np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.uint32))
        L.fastf_pack_records_ext(lists.cell_dict, lists.feat_dict, n, flags.ctypes.data, xf.ctypes.data, cb.ctypes.data, cb.dtype.itemsize,
                                 gx.ctypes.data, gx.dtype.itemsize, ub.ctypes.data, ub.dtype.itemsize, *(a.ctypes.data for a in out))
        return out
    L.fastf_pack_records.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.fastf_pack_records.restype = None
    flags = np.ascontiguousarray(flags, dtype=np.uint8)
    xf = np.ascontiguousarray(xf, dtype=np.int32)
    cb, gx, ub = (np.ascontiguousarray(a) for a in (cb, gx, ub))
    n = len(flags)
    cb_key = np.empty(n, dtype=np.uint64)
    gx_key = np.empty(n, dtype=np.uint64)
    umi = np.empty(n, dtype=np.uint32)
    meta = np.empty(n, dtype=np.uint32)
    L.fastf_pack_records(lists.cell_dict, lists.feat_dict, n, flags.ctypes.data, xf.ctypes.data,
                         cb.ctypes.data, cb.dtype.itemsize, gx.ctypes.data, gx.dtype.itemsize,
                         ub.ctypes.data, ub.dtype.itemsize,
                         cb_key.ctypes.data, gx_key.ctypes.data, umi.ctypes.data, meta.ctypes.data)
    return cb_key, gx_key, umi, meta


class PinnedBatch:
    """n packed records in pinned host memory (fastf_pinned_alloc): cb_key u64 | gx_key u64 | umi u32 | meta u32,
    as numpy views.  What fastf_engine_push_pinned sends to the device without a staging copy."""

    def __init__(self, n):
        self._L = _lib.lib()
        self.n = int(n)
        self._p = self._L.fastf_pinned_alloc(max(self.n, 1) * 24)
        if not self._p:
            raise FastfError(self._L.fastf_last_error().decode())
        buf = (C.c_uint8 * (max(self.n, 1) * 24)).from_address(self._p)
        raw = np.frombuffer(buf, dtype=np.uint8)
        self.cb_key = raw[:8 * n].view(np.uint64)
        self.gx_key = raw[8 * n:16 * n].view(np.uint64)
        self.umi = raw[16 * n:20 * n].view(np.uint32)
        self.meta = raw[20 * n:24 * n].view(np.uint32)

    def fill(self, off, cb, gx, umi, meta):
        """copy torch device tensors (int64/int32 bit patterns) or numpy arrays into [off, off + len)"""
        def put(dst, src, dt):
            if hasattr(src, "cpu"):
                import torch
                view = torch.from_numpy(dst[off:off + src.numel()].view(dt))
                view.copy_(src)                       # device -> pinned host, no intermediate
            else:
                dst[off:off + len(src)] = src
        put(self.cb_key, cb, np.int64); put(self.gx_key, gx, np.int64)
        put(self.umi, umi, np.int32); put(self.meta, meta, np.int32)

    def batch(self, a=0, b=None):
        b = self.n if b is None else b
        return Batch(self.cb_key[a:b].ctypes.data, self.gx_key[a:b].ctypes.data, self.umi[a:b].ctypes.data,
                     self.meta[a:b].ctypes.data, b - a)

    def close(self):
        if getattr(self, "_p", None):
            self.cb_key = self.gx_key = self.umi = self.meta = None
            self._L.fastf_pinned_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    """fastf_engine_* (host buffers) and fastf_dev_* (device pointers) of include/fastf_amd.h."""

    def __init__(self, cell_keys, feature_keys, rate_depth=1.0, seed=926, mt_skip=0,
                 umi_max_bases=12, n_shards=1, shard_rank=0, device=0,
                 batch_records=0, key_capacity=0, threshold=None, devices=None):
        self._L = _lib.lib()
        self._cell_keys = np.ascontiguousarray(cell_keys, dtype=np.uint64)
        self._feature_keys = np.ascontiguousarray(feature_keys, dtype=np.uint64)
        cfg = EngineConfig()
        cfg.cell_keys = self._cell_keys.ctypes.data
        cfg.n_cells = len(self._cell_keys)
        cfg.feature_keys = self._feature_keys.ctypes.data
        cfg.n_features = len(self._feature_keys)
        cfg.draw_threshold = draw_threshold(rate_depth) if threshold is None else threshold
        cfg.umi_max_bases = umi_max_bases
        cfg.mt_seed, cfg.mt_skip = seed, mt_skip
        cfg.n_shards, cfg.shard_rank = n_shards, shard_rank
        cfg.device = device
        cfg.batch_records, cfg.key_capacity = batch_records, key_capacity
        if devices is not None:                # one engine driving several devices (ordinals may repeat: one-GPU rehearsal)
            self._devices = np.ascontiguousarray(devices, dtype=np.int32)
            cfg.n_devices, cfg.devices = len(self._devices), self._devices.ctypes.data
        h = C.c_void_p()
        check(self._L.fastf_engine_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self.n_shards = n_shards
        cb, fb, ub, tb = (C.c_uint32() for _ in range(4))
        check(self._L.fastf_engine_key_bits(h, C.byref(cb), C.byref(fb), C.byref(ub), C.byref(tb)))
        self.cell_bits, self.feature_bits, self.umi_bits, self.key_bits = cb.value, fb.value, ub.value, tb.value

    @classmethod
    def from_lists(cls, lists: Lists, rate_depth=1.0, seed=926, **kw):
        return cls(lists.cell_keys, lists.feature_keys, rate_depth=rate_depth, seed=seed,
                   mt_skip=lists.mt_skip, **kw)

    # ---- host-buffer streaming API ----
    @staticmethod
    def _batch(cb_key, gx_key, umi, meta, umi_ext=None):
        arrs = (np.ascontiguousarray(cb_key, dtype=np.uint64), np.ascontiguousarray(gx_key, dtype=np.uint64),
                np.ascontiguousarray(umi, dtype=np.uint32), np.ascontiguousarray(meta, dtype=np.uint32),
                None if umi_ext is None else np.ascontiguousarray(umi_ext, dtype=np.uint32))
        b = Batch(arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data, arrs[3].ctypes.data, len(arrs[0]),
                  None if arrs[4] is None else arrs[4].ctypes.data)
        return b, arrs

    def push(self, cb_key, gx_key, umi, meta, draws=None, umi_ext=None):
        """umi_ext: bases 17.. of every UMI (pack_records(..., long_umis=True)) for an engine with umi_max_bases > 16"""
        b, keep = self._batch(cb_key, gx_key, umi, meta, umi_ext)
        if draws is None:
            check(self._L.fastf_engine_push(self._h, C.byref(b)))
        else:
            d = np.ascontiguousarray(draws, dtype=np.uint32)
            check(self._L.fastf_engine_push_draws(self._h, C.byref(b), d.ctypes.data, len(d)))
        del keep

    def push_pinned(self, pb: PinnedBatch, a=0, b=None):
        """zero-copy push of pinned records [a, b); the memory must stay untouched until wait_input() / finish()"""
        bt = pb.batch(a, b)
        check(self._L.fastf_engine_push_pinned(self._h, C.byref(bt)))

    def wait_input(self):
        check(self._L.fastf_engine_wait_input(self._h))

    def lend_rows(self, ptr, nbytes):
        """pinned host memory (address, bytes) the next finish() may place the rows in; 0 / None withdraws the loan"""
        check(self._L.fastf_engine_lend_rows(self._h, ptr or None, nbytes))

    def finish(self, copy=True):
        """copy=False: the arrays are VIEWS of the engine's row buffer (valid until the next reset / finish / close): what a C
        caller of fastf_engine_finish gets, without the 12 bytes per row this wrapper would copy"""
        coo = Coo()
        cnt = (C.c_uint64 * 3)()
        check(self._L.fastf_engine_finish(self._h, C.byref(coo), C.byref(cnt)))
        n = coo.nnz

        def arr(p):
            if not n:
                return np.zeros(0, dtype=np.uint32)
            a = np.ctypeslib.as_array(p, shape=(n,))
            return a.copy() if copy else a
        return dict(feature=arr(coo.feature), cell=arr(coo.cell), count=arr(coo.count), nnz=n,
                    total=int(cnt[0]), sampled=int(cnt[1]), valid=int(cnt[2]))

    def umi_rows(self):
        r = UmiRows()
        check(self._L.fastf_engine_umi_rows(self._h, C.byref(r)))
        n = r.n

        def arr(p, dt=np.uint32):
            return np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dtype=dt)
        return dict(feature=arr(r.feature), cell=arr(r.cell), n_copy=arr(r.n_copy), umi=arr(r.umi),
                    nonnull=arr(r.nonnull, np.uint8), n=n)

    def format_matrix(self, res, bam_label: bytes, rate_cell, rate_depth, n_feature, n_barcode) -> bytes:
        f = np.ascontiguousarray(res["feature"], dtype=np.uint32)
        c = np.ascontiguousarray(res["cell"], dtype=np.uint32)
        k = np.ascontiguousarray(res["count"], dtype=np.uint32)
        coo = Coo(f.ctypes.data_as(C.POINTER(C.c_uint32)), c.ctypes.data_as(C.POINTER(C.c_uint32)),
                  k.ctypes.data_as(C.POINTER(C.c_uint32)), len(f))
        cnt = (C.c_uint64 * 3)(res["total"], res["sampled"], res["valid"])
        out, n = C.c_void_p(), C.c_size_t()
        check(self._L.fastf_format_matrix(bam_label, C.c_float(rate_cell), C.c_float(rate_depth), C.byref(cnt),
                                          n_feature, n_barcode, C.byref(coo), C.byref(out), C.byref(n)))
        try:
            return C.string_at(out, n.value)
        finally:
            _libc_free(out)

    def format_umi_rows(self, rows) -> bytes:
        a = {k: np.ascontiguousarray(rows[k]) for k in ("feature", "cell", "n_copy", "umi", "nonnull")}
        r = UmiRows(a["feature"].ctypes.data_as(C.POINTER(C.c_uint32)), a["cell"].ctypes.data_as(C.POINTER(C.c_uint32)),
                    a["n_copy"].ctypes.data_as(C.POINTER(C.c_uint32)), a["umi"].ctypes.data_as(C.POINTER(C.c_uint32)),
                    a["nonnull"].ctypes.data_as(C.POINTER(C.c_uint8)), rows["n"])
        out, n = C.c_void_p(), C.c_size_t()
        check(self._L.fastf_format_umi_rows(C.byref(r), C.byref(out), C.byref(n)))
        try:
            return C.string_at(out, n.value)
        finally:
            _libc_free(out)

    def reset(self):
        check(self._L.fastf_engine_reset(self._h))

    def reseed(self, seed, skip=0):
        check(self._L.fastf_engine_reseed(self._h, seed, skip))

    # ---- timing of individual kernels (bench roofline leg) ----
    def set_timing(self, on: bool):
        check(self._L.fastf_engine_set_timing(self._h, 1 if on else 0))

    def device_records(self, n_devices=1):
        """records each device of a multi-device engine has been given since the last reset"""
        out = (C.c_uint64 * max(1, n_devices))()
        check(self._L.fastf_engine_device_records(self._h, out, max(1, n_devices)))
        return [int(x) for x in out]

    def get_timing(self, which: int):
        ms, n = C.c_double(), C.c_uint64()
        check(self._L.fastf_engine_get_timing(self._h, which, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # ---- device-level API: arguments are raw device pointers (ints) ----
    def reserve(self, max_records, max_keys):
        check(self._L.fastf_dev_reserve(self._h, max_records, max_keys))

    def dev_count_hits(self, d_cb, n, d_out, stream=0):
        check(self._L.fastf_dev_count_hits(self._h, d_cb, n, d_out, stream))

    def dev_count_hits_blocked(self, d_cb, n, d_blocked, d_out, stream=0):
        check(self._L.fastf_dev_count_hits_blocked(self._h, d_cb, n, d_blocked, d_out, stream))

    def block_bytes(self, n) -> int:
        """bytes of the blocked record buffer (gx | umi | meta | cell scratch per 256-record unit) for n records;
        0 = this engine cannot run the streaming K1b that reads it"""
        v = C.c_uint64()
        check(self._L.fastf_dev_block_bytes(self._h, n, C.byref(v)))
        return int(v.value)

    def dev_block_records(self, d_gx, d_umi, d_meta, n, d_blocked, stream=0):
        check(self._L.fastf_dev_block_records(self._h, d_gx, d_umi, d_meta, n, d_blocked, stream))

    def dev_probe_pack(self, d_cb, d_gx, d_umi, d_meta, n, d_draws, n_draws, d_keys, shard_stride,
                       d_key_counts, d_counters, stream=0, d_draw_base=None, reuse_hits=False, segmented=False, blocked=False,
                       draw_bits=False):
        """reuse_hits: dev_count_hits ran on these very records just before, on the same stream (K1a is skipped);
        segmented: streaming K1b, keys land in per-workgroup regions (probe_capacity slots; sort with segmented=True);
        blocked: d_gx is a blocked record buffer (block_bytes / dev_block_records), d_umi and d_meta are ignored;
        draw_bits: d_draws holds the decisions of n_draws draws (dev_draw_bits), not the 32-bit draws themselves"""
        check(self._L.fastf_dev_probe_pack(self._h, d_cb, d_gx, d_umi, d_meta, n, d_draws, n_draws, d_draw_base,
                                           d_keys, shard_stride, d_key_counts, d_counters,
                                           (1 if reuse_hits else 0) | (2 if segmented else 0) | (8 if blocked else 0) | (16 if draw_bits else 0),
                                           stream))

    @property
    def wide(self) -> bool:
        """keys wider than 64 bits (or UMIs beyond 16 bases): the group word and the rest of the key travel in two words"""
        return bool(self._L.fastf_engine_is_wide(self._h))

    def dev_probe_pack_wide(self, d_cb, d_gx, d_umi, d_meta, d_umi_ext, n, d_draws, n_draws, d_keys, d_vals, shard_stride,
                            d_key_counts, d_counters, stream=0, d_draw_base=None, reuse_hits=False, draw_bits=False):
        """dev_probe_pack for an engine whose keys are wider than 64 bits: group words into d_keys[shard][..], the rest of each key
        into d_vals[shard][..]; d_umi_ext: bases 17.. of the UMIs (0 / None: none)"""
        check(self._L.fastf_dev_probe_pack_wide(self._h, d_cb, d_gx, d_umi, d_meta, d_umi_ext or None, n, d_draws, n_draws, d_draw_base,
                                                d_keys, d_vals, shard_stride, d_key_counts, d_counters,
                                                (1 if reuse_hits else 0) | (16 if draw_bits else 0), stream))

    def dev_adopt_wide(self, d_keys, d_vals, n, stream=0):
        """the n (group word, rest of key) pairs this shard owns into the engine's own store: finish() / umi_rows() follow"""
        check(self._L.fastf_dev_adopt_wide(self._h, d_keys, d_vals, n, stream))

    def dev_draw_bits(self, d_draws, n_draws, d_bits_out, stream=0):
        """bit i of d_bits_out = d_draws[i] < this engine's keep threshold.  The kernel stores whole 64-bit words: d_bits_out must
        be 8-byte aligned and hold ((n_draws + 63) // 64) * 8 bytes = ((n_draws + 63) // 64) * 2 u32 words (include/fastf_amd.h)"""
        check(self._L.fastf_dev_draw_bits(self._h, d_draws, n_draws, d_bits_out, stream))

    def dev_mt_decisions(self, seed, skip, n_draws, d_bits_out, stream=0):
        """the decisions of n_draws draws of init_genrand(seed) + skip from the device's own generator (parallel for large
        counts: jump-ahead), bit i of d_bits_out; same size rule as dev_draw_bits"""
        check(self._L.fastf_dev_mt_decisions(self._h, seed, skip, n_draws, d_bits_out, stream))

    def dev_mt_decisions_multi(self, seed, skip, n_draws, thresholds, d_planes_out, plane_stride_words, stream=0):
        """the decision planes of a sweep: the stream of dev_mt_decisions generated once and compared against every threshold
        (0 .. 2^32) in the same pass; plane j starts plane_stride_words 32-bit words behind plane j - 1 (even, at least
        (n_draws + 63) // 64 * 2) and has the layout of dev_draw_bits.  The engine's own threshold plays no part."""
        t = np.ascontiguousarray(thresholds, dtype=np.uint64)
        check(self._L.fastf_dev_mt_decisions_multi(self._h, seed, skip, n_draws, t.ctypes.data, len(t), d_planes_out,
                                                   plane_stride_words, stream))

    def dev_cell_summary(self, d_cell, d_count, d_nnz, n_cells, d_umis_per_cell, d_genes_per_cell, stream=0):
        """rows ascending by (cell, feature) -> d_umis_per_cell[c - 1] = sum of the counts of cell c (u64, n_cells + 1 entries:
        the last is the sum of all counts), d_genes_per_cell[c - 1] = its rows with count >= 1 (u32); both cleared by the call"""
        check(self._L.fastf_dev_cell_summary(self._h, d_cell, d_count, d_nnz, n_cells, d_umis_per_cell, d_genes_per_cell, stream))

    def dev_gene_summary(self, d_feature, d_count, d_nnz, n_features, d_cells_per_gene, d_umis_per_gene, stream=0):
        """rows in any order -> d_cells_per_gene[g - 1] = rows of feature g (1-based) with count >= 1 (u32), d_umis_per_gene[g - 1] =
        the sum of their counts (u64); n_features entries each, cleared by the call; a feature outside 1 .. n_features adds nothing.
        The sum of all counts is below 2^32"""
        check(self._L.fastf_dev_gene_summary(self._h, d_feature, d_count, d_nnz, n_features, d_cells_per_gene, d_umis_per_gene, stream))

    def dev_gene_reps_add(self, d_cells_per_gene, n_features, d_detected, d_sum, d_sumsq, stream=0):
        """replicate runs: the cells per gene of one seed's point (u32[n_features], what dev_gene_summary left) added into the three
        u64[n_features] accumulators of its grid point: detected += (cells >= 1), sum += cells, sumsq += cells^2; nothing is cleared"""
        check(self._L.fastf_dev_gene_reps_add(self._h, d_cells_per_gene, n_features, d_detected, d_sum, d_sumsq, stream))

    def dev_copy_summary(self, d_ukeys, d_ncopy, d_nrows, n_cells, d_reads_per_cell, d_null_reads_per_cell, d_single_per_cell, d_hist, stream=0):
        """the rows of dev_umi_rows on this engine -> per cell (slot c - 1, u32, n_cells entries each) the sum of n_copy over all its
        rows, that sum over its NULL-blob rows and its non-NULL rows with n_copy == 1; d_hist (u64, COPY_BINS + 1 entries): the
        non-NULL rows with n_copy == k at k - 1, those with n_copy >= COPY_BINS at COPY_BINS - 1, the reads of those behind it.  All
        cleared by the call; the cell and the NULL flag come from the engine's key layout; a cell outside 1 .. n_cells adds nothing
        to the per-cell arrays.  Every per-cell number is below 2^32"""
        check(self._L.fastf_dev_copy_summary(self._h, d_ukeys, d_ncopy, d_nrows, n_cells, d_reads_per_cell, d_null_reads_per_cell,
                                             d_single_per_cell, d_hist, stream))

    def dev_cell_hits(self, n, d_blocked, d_hits_per_cell, stream=0):
        """d_hits_per_cell[c - 1] (u32, n_cells entries, cleared by the call) = records of the last dev_count_hits[_blocked] over
        these n records whose cell index is c; d_blocked: that call's blocked buffer, or 0 / None for the SoA scratch"""
        check(self._L.fastf_dev_cell_hits(self._h, n, d_blocked or None, d_hits_per_cell, stream))

    def dev_cell_decisions(self, n, d_blocked, seed, skip, n_draws, d_thresholds, d_bits_out, stream=0):
        """bit i of d_bits_out = draw i of init_genrand(seed) + skip < d_thresholds[cell of the i-th CB hit - 1] (u64[n_cells] on
        the device, 0 .. 2^32); layout and size rule of dev_draw_bits.  Valid where dev_cell_hits is; dev_probe_pack(reuse_hits,
        draw_bits) over the plane may follow"""
        check(self._L.fastf_dev_cell_decisions(self._h, n, d_blocked or None, seed, skip, n_draws, d_thresholds, d_bits_out, stream))

    def dev_level_init(self, d_umis_full, n_cells, umi_cap, d_lo, d_hi, d_probe, d_out, d_err_in=0, stream=0):
        """level: the state of the threshold search from U_k(2^32) (u64[n_cells] on the device) and the UMI cap: d_lo, d_hi, the first
        probes d_probe (u64[n_cells] each), d_out[0] = cells open, d_out[1] = cells capped, d_out[2] = error bits found, d_out[3] = held"""
        check(self._L.fastf_dev_level_init(self._h, d_umis_full, n_cells, int(umi_cap), d_lo, d_hi, d_probe, d_out, d_err_in or None, stream))

    def dev_level_step(self, d_umis_per_cell, n_cells, umi_cap, d_lo, d_hi, d_probe, d_out, d_err_in=0, stream=0):
        """level: one step of the search: d_umis_per_cell[k] = U_k(d_probe[k]); an open cell moves lo or hi to its probe; the next
        probes into d_probe (0 for a cell that is not open), d_out[0] = cells still open"""
        check(self._L.fastf_dev_level_step(self._h, d_umis_per_cell, n_cells, int(umi_cap), d_lo, d_hi, d_probe, d_out, d_err_in or None, stream))

    def dev_fidelity(self, d_feature_full, d_cell_full, d_count_full, d_nnz_full, d_feature, d_cell, d_count, d_nnz, n_cells, d_sum_xy, d_sum_yy,
                     d_err=0, stream=0):
        """--fidelity: point rows joined with full rows, both ascending by (cell, feature) on the device -> d_sum_xy[c - 1] = the sum of
        x * y over the point rows of cell c, d_sum_yy[c - 1] = the sum of y * y (u64[n_cells] each, cleared by the call).  A point row
        without a partner among the full rows raises bit 32 in *d_err (u64 on the device; 0 / None: the engine's error word) and the
        call raises FastfError; synchronises the stream"""
        check(self._L.fastf_dev_fidelity(self._h, d_feature_full or None, d_cell_full or None, d_count_full or None, d_nnz_full, d_feature or None,
                                         d_cell or None, d_count or None, d_nnz, n_cells, d_sum_xy, d_sum_yy, d_err or None, stream))

    def dev_partner_counts(self, d_feature_full, d_cell_full, d_count_full, d_nnz_full, d_feature, d_cell, d_nnz, d_x, d_err=0, stream=0):
        """--gene-fidelity: d_x[i] (u32) = the count of the full row with the (cell, feature) of point row i; both row sets ascend by
        (cell, feature) on the device.  A point row without a partner gets x = 0, raises bit 32 in *d_err (0 / None: the engine's error
        word) and the call raises FastfError; synchronises the stream"""
        check(self._L.fastf_dev_partner_counts(self._h, d_feature_full or None, d_cell_full or None, d_count_full or None, d_nnz_full, d_feature or None,
                                               d_cell or None, d_nnz, d_x or None, d_err or None, stream))

    def dev_gene_moments(self, d_feature, d_a, d_b, d_nnz, n_features, d_sum_ab, d_sum_bb, stream=0):
        """--gene-fidelity: rows (feature 1-based, a, b) in any order on the device -> d_sum_ab[g - 1] = the sum of a * b, d_sum_bb[g - 1] =
        the sum of b * b (u64[n_features] each, cleared by the call); stream-ordered"""
        check(self._L.fastf_dev_gene_moments(self._h, d_feature or None, d_a or None, d_b or None, d_nnz, n_features, d_sum_ab or None, d_sum_bb or None, stream))

    def dev_neighbor_planes(self, d_feature, d_cell, d_count, d_nnz, d_slot_map, n_features, n_cells, n_genes, d_planes=0, planes_bytes=0, stream=0) -> int:
        """--neighbors: the number of 7-bit planes P the largest count among the rows with a slot needs (FastfError beyond 3) and — d_planes
        given — the P byte planes of sweep.neighbors_pad(n_cells, n_genes) zeroed and filled; synchronises the stream once"""
        p = C.c_uint32()
        check(self._L.fastf_dev_neighbor_planes(self._h, d_feature or None, d_cell or None, d_count or None, d_nnz, d_slot_map or None, n_features, n_cells,
                                                n_genes, d_planes or None, planes_bytes, C.byref(p), stream))
        return p.value

    def dev_neighbors(self, d_planes, planes, n_cells, n_genes, k, d_idx, d_cnt, d_norms, stream=0) -> int:
        """--neighbors: the planes -> d_norms (u64[n_cells]), d_idx (u32[n_cells * k], ascending within a row, 0xFFFFFFFF behind the
        d_cnt[i] entries), d_cnt (u32[n_cells]); returns the largest norm; FastfError at 2^42 and beyond.  FASTF_NEIGHBORS_MFMA=0: the dot
        products from ordinary integer instructions"""
        m = C.c_uint64()
        check(self._L.fastf_dev_neighbors(self._h, d_planes or None, planes, n_cells, n_genes, k, d_idx or None, d_cnt or None, d_norms or None, C.byref(m), stream))
        return m.value

    def dev_neighbors_shared(self, d_idx_a, d_cnt_a, d_idx_b, d_cnt_b, n_cells, k, d_shared, stream=0):
        """--neighbors: d_shared[i] (u32) = the cells in both neighbour sets of cell i; stream-ordered"""
        check(self._L.fastf_dev_neighbors_shared(self._h, d_idx_a or None, d_cnt_a or None, d_idx_b or None, d_cnt_b or None, n_cells, k, d_shared or None, stream))

    def dev_mapping(self, d_planes_point, planes_point, d_planes_full, planes_full, n_cells, n_genes, k, d_norms_full, d_idx, d_cnt, d_self_dot, d_self_rank, stream=0) -> int:
        """--mapping: the planes Engine.dev_neighbor_planes filled from the point's and from the full rows (planes_point <= planes_full) and
        the norms Engine.dev_neighbors left for the full rows -> d_self_dot (u64[n_cells]), d_idx (u32[n_cells * k]) and d_cnt in the layout
        of dev_neighbors, d_self_rank (u32[n_cells], 0xFFFFFFFF where self_dot is 0); returns the largest point norm.  Either largest norm
        at 2^42 and beyond raises FastfError (FASTF_ERR_NEIGHBOR_NORM) before the kernels run.  FASTF_MAPPING_MFMA=0: plain integer form"""
        m = C.c_uint64()
        check(self._L.fastf_dev_mapping(self._h, d_planes_point or None, planes_point, d_planes_full or None, planes_full, n_cells, n_genes, k, d_norms_full or None,
                                        d_idx or None, d_cnt or None, d_self_dot or None, d_self_rank or None, C.byref(m), stream))
        return m.value

    def dev_coexpr_sums(self, d_feature, d_cell, d_count, d_nnz, d_slot_map, n_features, n_cells, n_genes, planes, d_work, work_bytes, d_D, d_S, stream=0):
        """--coexpression: the rows and the slot map as dev_neighbor_planes takes them, `planes` what it returned -> the gene-major planes in
        d_work (sweep.coexpression_work_bytes), d_D (u64[n_genes * n_genes], dense) and d_S (u64[n_genes]), both zeroed by the call;
        FASTF_COEXPR_MFMA=0: the dot products from ordinary integer instructions, FASTF_COEXPR_CHUNK=<cells>: a shorter chunk; stream-ordered"""
        check(self._L.fastf_dev_coexpr_sums(self._h, d_feature or None, d_cell or None, d_count or None, d_nnz, d_slot_map or None, n_features, n_cells, n_genes,
                                            planes, d_work or None, work_bytes, d_D or None, d_S or None, stream))

    def dev_coexpr_select(self, d_D, d_S, n_cells, n_genes, k, d_idx, d_cnt, stream=0):
        """--coexpression: D and S over n_cells cells -> d_idx (u32[n_genes * k], ascending within a row, 0xFFFFFFFF behind the d_cnt[g]
        entries) and d_cnt (u32[n_genes]); FastfError naming FASTF_ERR_COEXPR_RANGE when n_cells * max D_gg >= 2^63; synchronises the stream once"""
        check(self._L.fastf_dev_coexpr_select(self._h, d_D or None, d_S or None, n_cells, n_genes, k, d_idx or None, d_cnt or None, stream))

    def dev_label_votes(self, d_idx, d_cnt, d_lab, n_cells, k, n_labels, d_pred, d_same, d_labelled, d_conf, stream=0):
        """--labels: the neighbour sets Engine.dev_neighbors left (d_idx, d_cnt) and d_lab (u8[n_cells], 0 unlabelled) -> d_pred, d_same,
        d_labelled (u8[n_cells]) and d_conf (u32[n_labels * (n_labels + 1)], zeroed by the call); FASTF_LABELS_LDS=0: the confusion counts
        by global atomics alone; stream-ordered"""
        check(self._L.fastf_dev_label_votes(self._h, d_idx or None, d_cnt or None, d_lab or None, n_cells, k, n_labels, d_pred or None, d_same or None,
                                            d_labelled or None, d_conf or None, stream))

    def dev_ptime_medians(self, d_idx, d_cnt, d_t, n_cells, k, d_est, d_valued, stream=0):
        """--pseudotime: the neighbour lists Engine.dev_neighbors or Engine.dev_mapping left (d_idx, d_cnt) and d_t (u32[n_cells], 0 without a
        value) -> d_est (u32[n_cells], the lower median of the valued neighbours' t, 0 with none) and d_valued (u32[n_cells]); stream-ordered"""
        check(self._L.fastf_dev_ptime_medians(self._h, d_idx or None, d_cnt or None, d_t or None, n_cells, k, d_est or None, d_valued or None, stream))

    def dev_ptime_census(self, d_est, d_t, n_cells, d_out, stream=0):
        """--pseudotime: the order census of d_est against d_t over the cells with both above 0 -> d_out (u64[7]: conc disc tie_e tie_t tie_both
        cells shift_sum, zeroed by the call); one workgroup per pair of tiles of sweep.PTIME_TILE cells; stream-ordered"""
        check(self._L.fastf_dev_ptime_census(self._h, d_est or None, d_t or None, n_cells, d_out or None, stream))

    def dev_marker_auc(self, d_planes, planes, n_cells, K, d_lab, n_labels, d_s2u, d_det, d_sum, d_n_per_label, stream=0):
        """--markers: the byte planes Engine.dev_neighbor_planes left (d_planes, `planes` of them) and d_lab (u8[n_cells]) -> d_s2u, d_sum
        (u64[n_labels * K]), d_det (u32[n_labels * K]) and d_n_per_label (u32[n_labels]), all cleared by the call; FASTF_MARKERS_LDS=0:
        the accumulators by global atomics alone; three planes are refused; stream-ordered"""
        check(self._L.fastf_dev_marker_auc(self._h, d_planes or None, planes, n_cells, K, d_lab or None, n_labels, d_s2u or None, d_det or None,
                                           d_sum or None, d_n_per_label or None, stream))

    def probe_capacity(self, n) -> int:
        """key slots a segmented probe_pack over n records needs; 0 = the streaming form is not available"""
        v = C.c_uint64()
        check(self._L.fastf_dev_probe_capacity(self._h, n, C.byref(v)))
        return int(v.value)

    def dev_set_regions(self, d_counts, n_regions, stride, d_n_out, stream=0):
        """the next segmented dev_sort reads n_regions rows of `stride` key slots, row r holding d_counts[r] keys"""
        check(self._L.fastf_dev_set_regions(self._h, d_counts, n_regions, stride, d_n_out, stream))

    def dev_sort(self, d_keys, d_tmp, d_n, max_n, key_bits=None, stream=0, skip_low=False, segmented=False) -> bool:
        in_tmp = C.c_int(0)
        check(self._L.fastf_dev_sort(self._h, d_keys, d_tmp, d_n, max_n,
                                     self.key_bits if key_bits is None else key_bits,
                                     (2 if skip_low else 0) | (4 if segmented else 0), C.byref(in_tmp), stream))
        return bool(in_tmp.value)

    def dev_reduce(self, d_sorted, d_n, max_n, d_feature, d_cell, d_count, d_nnz, stream=0, skip_low=False, segmented=False):
        """segmented: the rows stay in the engine's row regions (only *d_nnz is written); dev_rows_gather concatenates them"""
        check(self._L.fastf_dev_reduce(self._h, d_sorted, d_n, max_n, d_feature, d_cell, d_count, d_nnz,
                                       (2 if skip_low else 0) | (8 if segmented else 0), stream))

    def dev_rows_gather(self, d_n, feature, cell, count, stream=0):
        """concatenate the row regions of the last dev_reduce into feature/cell/count (device or pinned host pointers)"""
        check(self._L.fastf_dev_rows_gather(self._h, d_n, feature, cell, count, stream))

    @property
    def table_modes(self) -> str:
        c, g = C.c_int(), C.c_int()
        check(self._L.fastf_engine_table_modes(self._h, C.byref(c), C.byref(g)))
        return "cells:%s genes:%s" % ("LDS perfect hash" if c.value else "L2 open addressing",
                                      {0: "L2 open addressing", 1: "LDS bitmap+rank", 2: "LDS direct table"}[g.value])

    @property
    def cell_scratch_bytes(self) -> int:
        b = C.c_uint32()
        check(self._L.fastf_engine_cell_scratch_bytes(self._h, C.byref(b)))
        return b.value

    @property
    def skip_bits(self) -> int:
        b = C.c_uint32()
        check(self._L.fastf_engine_skip_bits(self._h, C.byref(b)))
        return b.value

    def sort_passes(self, skip_low=False) -> int:
        b = C.c_uint32()
        check(self._L.fastf_engine_sort_passes(self._h, 2 if skip_low else 0, C.byref(b)))
        return b.value

    GRID_FAMILIES = ("k1a", "block_records", "draw_bits", "k1b_tiles", "k1b_stream", "scatter_regions", "sort_tiles", "rgn_hist",
                     "k3_windows", "k3_hashed", "giant", "pairs", "rows_gather")

    def grids(self, n_records=0, n_keys=0) -> dict:
        """{family: (workgroups, tiles)} of the step's capped grids for these counts (fastf_engine_grids)"""
        out = (C.c_uint32 * (2 * len(self.GRID_FAMILIES)))()
        check(self._L.fastf_engine_grids(self._h, n_records, n_keys, out))
        return {f: (out[2 * i], out[2 * i + 1]) for i, f in enumerate(self.GRID_FAMILIES)}

    def dev_scan_tiles(self, d_in, T, d_out, d_total=None, d_running=None, d_base=None, slot=0, stream=0):
        check(self._L.fastf_dev_scan_tiles(self._h, d_in, T, d_out, d_total, d_running, d_base, slot, stream))

    def dev_umi_rows(self, d_sorted, d_n, max_n, d_ukeys, d_ncopy, d_nrows, stream=0):
        check(self._L.fastf_dev_umi_rows(self._h, d_sorted, d_n, max_n, d_ukeys, d_ncopy, d_nrows, stream))

    def dev_error_bits(self) -> int:
        b = C.c_uint64()
        check(self._L.fastf_dev_error_bits(self._h, C.byref(b)))
        return int(b.value)

    def dev_clear_error_bits(self, mask, stream=0):
        check(self._L.fastf_dev_clear_error_bits(self._h, mask, stream))

    def close(self):
        if getattr(self, "_h", None):
            self._L.fastf_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _libc_free(ptr):
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(ptr)
