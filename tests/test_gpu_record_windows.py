"""The device record stage (fastf_amd/csrc/gpu_records.hpp: gr_hop_kernel, gr_stitch_kernel, gr_repair_kernel, gr_pack_kernel) driven
through fastf_gpurec_parse with hand-built windows, window by window, against tests/grwin_ref.py (proved against the host build of
the same functions and against the host reader in tests/test_grwin_ref_host.py).  No reader, no file, no inflate: with
`end == data_off` the whole window is the `tail` the caller hands in, at any `start`.  Case K alone goes the production way: a
tail whose last record continues into bytes that fastf_gpuinf_submit_keep inflates behind it.

Asserted per window and parity, all exactly: the return value, status 0, n, handover, no_xf, no_gx, the four SoA arrays (the host
reader's records), the increase of the repair count and of the window count, a fallback count of 0, and the window's bytes
fetched back unchanged.  The window buffers are reserved once for the largest window: the pack kernel's last 16-byte load may pass
`end`, and the reserve's slack is what it reads there.

Order: H (which leaves good records behind a shorter window's `end`, by design), then K, then the rest; nothing but H depends on
what an earlier window left."""
import ctypes as C
import zlib

import numpy as np
import pytest

from fastf_amd import _lib

import grwin_ref as W
from test_gpu_inflate import Blk, _Pinned
from test_gpu_records_host import views
from test_grwin_ref_host import expectation, lists, _host_records

pytestmark = pytest.mark.gpu

GUARD = 0xA5


class Result(C.Structure):
    _fields_ = [("status", C.c_int), ("n", C.c_uint64), ("handover", C.c_uint64), ("no_xf", C.c_uint64), ("no_gx", C.c_uint64),
                ("batch", _lib.Batch)]


class Dev:
    def __init__(self):
        L = self.L = _lib.lib()
        vp, u64 = C.c_void_p, C.c_uint64
        L.fastf_gpuinf_create.restype = vp; L.fastf_gpuinf_create.argtypes = [C.c_int]
        L.fastf_gpuinf_destroy.argtypes = [vp]
        L.fastf_gpuinf_reserve.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_size_t]
        L.fastf_gpuinf_submit_keep.argtypes = [vp, vp, vp, C.c_size_t, C.c_int, vp]
        L.fastf_gpuinf_wait.argtypes = [vp, vp, vp]
        L.fastf_gpurec_parse.argtypes = [vp, C.c_int, C.c_char_p, C.c_size_t, u64, u64, C.c_uint32, vp, vp, C.POINTER(Result)]
        L.fastf_gpurec_fetch.argtypes = [vp, C.c_int, vp, u64, u64]
        L.fastf_gpurec_repairs.restype = u64; L.fastf_gpurec_repairs.argtypes = [vp]
        L.fastf_gpurec_stats.restype = None; L.fastf_gpurec_stats.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
        L.fastf_devmem_copy.argtypes = [vp, vp, C.c_size_t]
        self.g = L.fastf_gpuinf_create(0)
        assert self.g, L.fastf_last_error()
        self.reserve = max(W.case(name)[3] for name in W.ALL_CASES)
        assert L.fastf_gpuinf_reserve(self.g, self.reserve, 1 << 20, 64) == 0, L.fastf_last_error()
        self.hip = C.CDLL(_lib.hip_runtimes_loaded()[0])          # the ONE runtime of this process (by path: no second copy)
        self.vc, self.vf = views(lists())
        self.pin = _Pinned(L)

    def close(self):
        self.L.fastf_gpuinf_destroy(self.g)
        self.pin.free()

    def counts(self):
        w, f = C.c_uint64(), C.c_uint64()
        self.L.fastf_gpurec_stats(self.g, C.byref(w), C.byref(f))
        return self.L.fastf_gpurec_repairs(self.g), w.value, f.value

    def parse(self, parity, tail, data_off, end, n_ref):
        res = Result()
        rc = self.L.fastf_gpurec_parse(self.g, parity, tail, len(tail), data_off, end, n_ref, C.byref(self.vc), C.byref(self.vf), C.byref(res))
        assert rc == 0, self.L.fastf_last_error()
        return res

    def soa(self, batch, n):
        """the first n entries of the four device arrays"""
        out = [np.empty(n, np.uint64), np.empty(n, np.uint64), np.empty(n, np.uint32), np.empty(n, np.uint32)]
        if n:
            for x, src in zip(out, (batch.cb_key, batch.gx_key, batch.umi, batch.meta)):
                assert src and self.hip.hipMemcpy(C.c_void_p(x.ctypes.data), C.c_void_p(src), C.c_size_t(n * x.itemsize), 2) == 0
        return out

    def fetch(self, parity, a, b):
        got = np.zeros(b - a, np.uint8)
        assert self.L.fastf_gpurec_fetch(self.g, parity, got.ctypes.data, a, b) == 0, self.L.fastf_last_error()
        return got.tobytes()


@pytest.fixture(scope="module")
def dev():
    d = Dev()
    yield d
    d.close()


def check_result(dev, res, x, before, where):
    """everything the API returned for one parse against the expectation x"""
    assert res.status == 0, where
    assert (res.n, res.handover, res.no_xf, res.no_gx) == (x["n"], x["handover"], x["no_xf"], x["no_gx"]), where
    assert res.batch.n == res.n
    for g, w, what in zip(dev.soa(res.batch, res.n), x["soa"], ("cb_key", "gx_key", "umi", "meta")):
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, "%s: %s differs first at record %d of %d (offset %d)" % (where, what, bad[0], res.n, x["offsets"][bad[0]])
    after = dev.counts()
    assert (after[0] - before[0], after[1] - before[1], after[2]) == (x["repairs"], x["windows"], 0), where


def check(dev, name, parity):
    b, start, n_ref, end = W.case(name)
    x = expectation(name)
    tail = b[:end - start]
    before = dev.counts()
    res = dev.parse(parity, tail, end, end, n_ref)
    check_result(dev, res, x, before, "%s parity %d" % (name, parity))
    if x["windows"]:                                                        # (under 36 bytes nothing is copied in: all of it is the host's)
        assert dev.fetch(parity, start, end) == tail, name                 # the parse leaves the window alone
    return res


# ---------------------------------------------------------------- H: good records behind `end`
@pytest.mark.parametrize("parity", [0, 1])
def test_H_records_stop_at_end_and_the_soa_behind_n_is_untouched(dev, parity):
    res = check(dev, "H.full", parity)
    n1 = res.n
    ptr = (res.batch.cb_key, res.batch.gx_key, res.batch.umi, res.batch.meta)
    m = n1 + 64
    assert m <= dev.reserve // 36 + 1                                       # the arrays were sized for the reserve: room for the guard
    guard = dev.pin.alloc(8 * m, bytes([GUARD]) * (8 * m))
    for name in ("H.cut", "H.edge"):
        for p, w in zip(ptr, (8, 8, 4, 4)):
            assert dev.L.fastf_devmem_copy(p, guard, w * m) == 0, dev.L.fastf_last_error()
        res = check(dev, name, parity)
        assert (res.batch.cb_key, res.batch.gx_key, res.batch.umi, res.batch.meta) == ptr and res.n < n1
        for a, dt in zip(dev.soa(res.batch, m), (np.uint64, np.uint64, np.uint32, np.uint32)):
            assert (a[res.n:].view(np.uint8) == GUARD).all(), (name, dt)
        # the good records are still there behind `end`
        b, start, _, end = W.case(name)
        assert dev.fetch(parity, end, start + len(b)) == b[end - start:]


# ---------------------------------------------------------------- K: the production shape
def k_window(seed):
    """(stream, cut): a tail of four records and 20 bytes of the fifth; the rest, up to 7 bytes short of the last record's end, is
    what the device inflates"""
    s = W.Stream(seed)
    s.mixed(4)
    cut = s.pos + 20
    s.fill_to(150_000)
    return bytes(s.b[:-7]), cut


def test_K_a_tail_that_continues_into_inflated_blocks(dev):
    kept = []
    for parity, seed, start in ((0, 30, 11), (1, 31, 4099)):
        b, cut = k_window(seed)
        tail, rest = b[:cut], b[cut:]
        data_off, end = start + cut, start + len(b)
        sizes = [65280, 1, 30000, 63]
        sizes.append(len(rest) - sum(sizes))
        assert sizes[-1] > 0
        comp, desc, crc, u = bytearray(), (Blk * len(sizes))(), [], 0
        for i, n in enumerate(sizes):
            co = zlib.compressobj(6, zlib.DEFLATED, -15)
            z = co.compress(rest[u:u + n]) + co.flush()
            comp += b"\x1f\x8b" * 9
            desc[i] = Blk(len(comp), len(z), n, data_off + u)
            comp += z
            crc.append(zlib.crc32(rest[u:u + n]))
            u += n
        cbuf = dev.pin.alloc(len(comp), comp)
        crc = np.asarray(crc, dtype=np.uint32)
        status = (C.c_uint8 * len(sizes))(*([0xFF] * len(sizes)))
        assert dev.L.fastf_gpuinf_submit_keep(dev.g, cbuf, desc, len(sizes), parity, crc.ctypes.data) == 0, dev.L.fastf_last_error()
        assert dev.L.fastf_gpuinf_wait(dev.g, status, None) == 0, dev.L.fastf_last_error()
        assert bytes(status) == bytes(len(sizes))
        img = bytes(start) + b
        x = W.device(img, start, end, W.N_REF)
        assert x["status"] == 0 and x["handover"] < end and x["n"] > 300
        *soa, no_xf, no_gx = _host_records(b[:x["handover"] - start])
        x.update(soa=soa, no_xf=no_xf, no_gx=no_gx)
        before = dev.counts()
        res = dev.parse(parity, tail, data_off, end, W.N_REF)
        check_result(dev, res, x, before, "K parity %d" % parity)
        assert dev.fetch(parity, start, end) == b
        kept.append((res, x))
    # a parity's batch is valid until the second next parse of that parity: both are still whole
    for res, x in kept:
        for g, w in zip(dev.soa(res.batch, res.n), x["soa"]):
            assert np.array_equal(g, w)


# ---------------------------------------------------------------- the rest
@pytest.mark.parametrize("name", W.SMALL_CASES + ("I",))
def test_window(dev, name):
    for parity in (0, 1):
        check(dev, name, parity)


def test_no_window_of_the_module_fell_back(dev):
    repairs, windows, fallbacks = dev.counts()
    assert fallbacks == 0 and windows > 2 * len(W.SMALL_CASES) and repairs > 0
