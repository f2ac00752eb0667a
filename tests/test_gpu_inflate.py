"""BGZF inflate on the device (gpu_frontend.hpp: gpu_inflate2.hpp's lane-per-block decoder + the match resolver) against
zlib, and the BAM reader with FASTF_GPU_INFLATE on against the host-only reader."""
import ctypes as C
import zlib

import numpy as np
import pytest

import deflate_ref as D
import fastf_amd as F
from fastf_amd import synth, _lib
from helpers import Case
from test_gpu_inflate_host import raw_streams, sample_payloads
from test_bam_reader import read_all

pytestmark = pytest.mark.gpu


class Blk(C.Structure):
    _fields_ = [("coff", C.c_uint64), ("clen", C.c_uint32), ("isize", C.c_uint32), ("uoff", C.c_uint64)]


def test_device_inflate_matches_zlib():
    """the two-kernel device inflate: one lane per block decodes to literals + match tokens (gpu_inflate2.hpp), one wave per
    block resolves the matches"""
    import torch  # noqa: F401
    L = _lib.lib()
    L.fastf_gpuinf_create.restype = C.c_void_p; L.fastf_gpuinf_create.argtypes = [C.c_int]
    L.fastf_gpuinf_destroy.argtypes = [C.c_void_p]
    L.fastf_gpuinf_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(7)
    blocks = []
    for data in sample_payloads(rng, 30):
        for comp in raw_streams(data):
            blocks.append((comp, data))
    assert len(blocks) > 800                                          # several slices
    comp_all = bytearray(); desc = (Blk * len(blocks))(); uoff = 0
    for i, (c, d) in enumerate(blocks):
        comp_all += b"\x1f\x8b" * 9                                    # something between the payloads, like BGZF headers
        desc[i] = Blk(len(comp_all), len(c), len(d), uoff)
        comp_all += c; uoff += len(d)
    out_p = L.fastf_pinned_alloc(max(uoff, 1)); assert out_p
    status = (C.c_uint8 * len(blocks))()
    cbuf = L.fastf_pinned_alloc(len(comp_all)); assert cbuf                         # the driver takes pinned compressed bytes
    C.memmove(cbuf, bytes(comp_all), len(comp_all))
    g = L.fastf_gpuinf_create(0); assert g, L.fastf_last_error()
    try:
        for _ in range(2):                                             # second run reuses the slots
            assert L.fastf_gpuinf_run(g, cbuf, desc, len(blocks), out_p, status) == 0, L.fastf_last_error()
            out = C.string_at(out_p, uoff)
            assert bytes(status) == bytes(len(blocks))
            o = 0
            for c, d in blocks:
                assert out[o:o + len(d)] == d
                o += len(d)
        # ordinary (heap) memory on both sides: fastf_gpuinf_run registers the ranges for the call — the compressed bytes up to the
        # end of the last block, where this array ends too — and unregisters them; nothing stays in the ledger
        L.fastf_debug_live_registrations.restype = int
        live0 = L.fastf_debug_live_registrations()
        h_comp = np.frombuffer(bytes(comp_all), dtype=np.uint8).copy()
        h_out = np.zeros(max(uoff, 1), dtype=np.uint8)
        st2 = (C.c_uint8 * len(blocks))()
        assert L.fastf_gpuinf_run(g, h_comp.ctypes.data, desc, len(blocks), h_out.ctypes.data, st2) == 0, L.fastf_last_error()
        assert bytes(st2) == bytes(len(blocks)) and h_out.tobytes() == b"".join(d for _, d in blocks)
        assert L.fastf_debug_live_registrations() == live0
        # a corrupted block is declined (or its CRC will differ), the others are untouched
        bad = bytearray(comp_all); bad[desc[5].coff + 3] ^= 0x5A
        C.memmove(cbuf, bytes(bad), len(bad))
        assert L.fastf_gpuinf_run(g, cbuf, desc, len(blocks), out_p, status) == 0
        out = C.string_at(out_p, uoff)
        o = 0
        for i, (c, d) in enumerate(blocks):
            if i != 5:
                assert status[i] == 0 and out[o:o + len(d)] == d
            o += len(d)
    finally:
        L.fastf_gpuinf_destroy(g)
        L.fastf_pinned_free(out_p)
        L.fastf_pinned_free(cbuf)


@pytest.mark.parametrize("window", [1 << 17, 1 << 22, 128 << 20])
def test_reader_with_device_inflate_gives_the_same_records(tmp_path, monkeypatch, window):
    case = Case(n=120_000, n_bar=300, n_gene=120, umi_pool=128, p_no_cb=0.05, p_unlisted_cb=0.05, p_bad_xf=0.2, p_n_umi=0.02, p_no_ub=0.03)
    lists = case.lists()
    bam = tmp_path / "t.bam"
    shape = lambda i: (91, 1, 0, i * 37 % 100000)
    synth.write_bam(str(bam), case.flags, case.xf, case.cb, case.gx, case.ub, shape=shape)
    monkeypatch.setenv("FASTF_BAM_WINDOW", str(window))
    monkeypatch.setenv("FASTF_GPU_INFLATE", "2")                       # wait for the device: every window goes through it
    monkeypatch.delenv("FASTF_BAM_PROFILE", raising=False)          # (no reader trace in the suite's output)
    got = read_all(bam, lists, cap=50_000)
    for g, w in zip(got, case.packed(lists)):
        np.testing.assert_array_equal(g, w)


# ---- the resolver driven by hand-built token streams (tests/deflate_ref.py; tests/test_inflate_tokens_host.py shows on the CPU
#      what the set holds and that a resolver with one wrong rule would not pass it) ----
GUARD = 0xA5


def _api():
    L = _lib.lib()
    L.fastf_gpuinf_create.restype = C.c_void_p; L.fastf_gpuinf_create.argtypes = [C.c_int]
    L.fastf_gpuinf_destroy.argtypes = [C.c_void_p]
    L.fastf_gpuinf_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.fastf_gpuinf_submit_keep.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.fastf_gpuinf_wait.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.fastf_gpuinf_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]; L.fastf_gpuinf_stats.restype = None
    L.fastf_gpurec_fetch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_uint64]
    return L


_FX = {}


def _fixtures():
    """the fixture set and zlib's output per name, built once per process"""
    if not _FX:
        fx = D.resolver_fixtures(np.random.default_rng(20))
        _FX["fx"] = fx; _FX["exp"] = {name: D.inflate_ref(s) for name, s, _ in fx}
    return _FX["fx"], _FX["exp"]


class _Pinned:
    """pinned host buffers of a test, freed together"""

    def __init__(self, L): self.L = L; self.ps = []

    def alloc(self, n, data=None):
        p = self.L.fastf_pinned_alloc(max(n, 1)); assert p
        self.ps.append(p)
        if data is not None: C.memmove(p, bytes(data), len(data))
        return p

    def free(self):
        for p in self.ps: self.L.fastf_pinned_free(p)
        self.ps = []


def _pack(pin, entries, uoffs):
    """(pinned compressed bytes, descriptors) of blocks (name, stream, isize) at the given output offsets"""
    comp = bytearray(); desc = (Blk * len(entries))()
    for i, (_, s, n) in enumerate(entries):
        comp += b"\x1f\x8b" * 9
        desc[i] = Blk(len(comp), len(s), n, uoffs[i]); comp += s
    return pin.alloc(len(comp), comp), desc


def _guard_blocks(total):
    """blocks that inflate to `total` guard bytes, side by side from offset 0"""
    sizes = [65535] * (total // 65535) + ([total % 65535] if total % 65535 else [])
    entries = []
    for n in sizes:
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        entries.append(("guard", co.compress(bytes([GUARD]) * n) + co.flush(), n))
    return entries, [65535 * i for i in range(len(sizes))]


def _image(entries, uoffs, exp, end):
    img = bytearray([GUARD]) * end
    for (name, _, n), u in zip(entries, uoffs): img[u:u + n] = exp[name]
    return bytes(img)


def _first_wrong(entries, uoffs, exp, got):
    for (name, _, n), u in zip(entries, uoffs):
        if got[u:u + n] != exp[name]: return "block %s at offset %d (uoff & 3 = %d)" % (name, u, u & 3)
    return "guard bytes outside every block"


def test_resolver_fixtures_match_zlib():
    """Every well-formed fixture, at the four values of uoff & 3, in one launch; the launch again with the blocks in reverse
    order (other offsets, other places in the token lists); the first 1, 63, 64, 65 and 257 blocks of the first launch alone.
    The guard bytes: the driver copies a slice's whole output range back, so a gap between two blocks comes back FROM THE
    DEVICE.  A launch of guard-valued blocks over the same range goes first and leaves the device's output buffer full of
    the guard value: a gap that comes back with anything else was written by a kernel outside its block (a last tiny block
    stands behind the gap after the last fixture, so that gap comes back too)."""
    import torch  # noqa: F401
    L = _api()
    fx, exp = _fixtures()
    pin = _Pinned(L)
    g = L.fastf_gpuinf_create(0); assert g, L.fastf_last_error()
    try:
        for run in range(2):
            order = D.device_order(fx)
            if run: order = order[::-1]
            uoffs, end = D.layout(order, phase0=run)
            out_p = pin.alloc(end + 64)
            gb, gu = _guard_blocks(end + 64)
            gc, gd = _pack(pin, gb, gu)
            st = (C.c_uint8 * len(gb))()
            assert L.fastf_gpuinf_run(g, gc, gd, len(gb), out_p, st) == 0, L.fastf_last_error()
            assert bytes(st) == bytes(len(gb)) and C.string_at(out_p, end) == bytes([GUARD]) * end
            cbuf, desc = _pack(pin, order, uoffs)
            status = (C.c_uint8 * len(order))()
            assert L.fastf_gpuinf_run(g, cbuf, desc, len(order), out_p, status) == 0, L.fastf_last_error()
            declined = [order[i][0] for i in range(len(order)) if status[i]]
            assert not declined, declined
            got = C.string_at(out_p, end)
            assert got == _image(order, uoffs, exp, end), _first_wrong(order, uoffs, exp, got)
            if run: continue
            for n in (1, 63, 64, 65, 257):                             # (no multiples of the 64 lanes of phase 1 or the 4 waves of phase 2)
                C.memset(out_p, 0, end)
                status = (C.c_uint8 * n)()
                assert L.fastf_gpuinf_run(g, cbuf, desc, n, out_p, status) == 0, L.fastf_last_error()
                assert bytes(status) == bytes(n)
                got = C.string_at(out_p, end)
                for (name, _, k), u in zip(order[:n], uoffs): assert got[u:u + k] == exp[name], (n, name)
    finally:
        L.fastf_gpuinf_destroy(g)
        pin.free()


def test_malformed_blocks_are_declined_and_neighbours_are_right():
    """streams zlib itself rejects (deflate_ref.declined_fixtures) between well-formed ones, first and last block included: the
    device declines exactly those, and counts them"""
    import torch  # noqa: F401
    L = _api()
    fx, exp = _fixtures()
    bad = D.declined_fixtures()
    for name, s, n in bad: assert D.zlib_declines(s, n), name
    order = [bad[0]]
    for i, e in enumerate(fx):
        order.append(e)
        if i % 4 == 3: order.append(bad[(i // 4) % len(bad)])
    order.append(bad[-1])
    is_bad = [e[0].startswith("decline/") for e in order]
    assert {e[0] for e, b in zip(order, is_bad) if b} == {e[0] for e in bad} and sum(is_bad) >= 10
    uoffs, end = D.layout(order, phase0=1)
    pin = _Pinned(L)
    g = L.fastf_gpuinf_create(0); assert g, L.fastf_last_error()
    try:
        out_p = pin.alloc(end)
        cbuf, desc = _pack(pin, order, uoffs)
        status = (C.c_uint8 * len(order))()
        assert L.fastf_gpuinf_run(g, cbuf, desc, len(order), out_p, status) == 0, L.fastf_last_error()
        got = C.string_at(out_p, end)
        for i, ((name, _, n), u) in enumerate(zip(order, uoffs)):
            if is_bad[i]: assert status[i] != 0, (i, name)
            else: assert status[i] == 0 and got[u:u + n] == exp[name], (i, name)
        nb, nd = C.c_uint64(), C.c_uint64()
        L.fastf_gpuinf_stats(g, C.byref(nb), C.byref(nd))
        assert (nb.value, nd.value) == (len(order), sum(is_bad))
    finally:
        L.fastf_gpuinf_destroy(g)
        pin.free()


def test_keep_mode_fixtures_crc_and_fetch():
    """keep mode: the blocks side by side in the window buffer of either parity from an odd offset on (their lengths put them at
    every uoff & 3), every block's CRC-32 checked on the device, the window read back with fastf_gpurec_fetch — together with
    the guard bytes a first keep-mode launch put in front of the first block and behind the last.  Then two CRC words off by
    one: those two blocks report the CRC bit, no other does."""
    import torch  # noqa: F401
    L = _api()
    fx, exp = _fixtures()
    pin = _Pinned(L)
    g = L.fastf_gpuinf_create(0); assert g, L.fastf_last_error()

    def keep(entries, uoffs, parity, crc):
        cbuf, desc = _pack(pin, entries, uoffs)
        status = (C.c_uint8 * len(entries))(*([0xFF] * len(entries)))
        crc = np.asarray(crc, dtype=np.uint32)
        assert L.fastf_gpuinf_submit_keep(g, cbuf, desc, len(entries), parity, crc.ctypes.data) == 0, L.fastf_last_error()
        assert L.fastf_gpuinf_wait(g, status, None) == 0, L.fastf_last_error()
        return bytes(status)

    try:
        for parity, first in ((0, 4099), (1, 8190)):
            order = D.device_order(fx)
            if parity: order = order[::-1]
            uoffs = [first + sum(e[2] for e in order[:i]) for i in range(len(order))]
            end = uoffs[-1] + order[-1][2]
            assert {u & 3 for u, e in zip(uoffs, order) if e[2] > 1000} == {0, 1, 2, 3}
            gb, gu = _guard_blocks(end + 256)
            assert keep(gb, gu, parity, [zlib.crc32(bytes([GUARD]) * n) for _, _, n in gb]) == bytes(len(gb))
            crc = [zlib.crc32(exp[name]) for name, _, _ in order]
            assert keep(order, uoffs, parity, crc) == bytes(len(order))
            got = np.zeros(end + 256, np.uint8)
            assert L.fastf_gpurec_fetch(g, parity, got.ctypes.data, 0, end + 256) == 0, L.fastf_last_error()
            got = got.tobytes()
            assert got[first:end] == b"".join(exp[name] for name, _, _ in order), _first_wrong(order, uoffs, exp, got)
            assert got[:first] == bytes([GUARD]) * first and got[end:] == bytes([GUARD]) * 256
            part = np.zeros(end - first - 7, np.uint8)                     # (a fetch that begins inside a block)
            assert L.fastf_gpurec_fetch(g, parity, part.ctypes.data, first + 7, end) == 0 and part.tobytes() == got[first + 7:end]
            names = [e[0] for e in order]
            off = sorted((names.index("grid/near"), len(names) - 1 - names[::-1].index("isize3")))
            crc[off[0]] = (crc[off[0]] + 1) & 0xFFFFFFFF; crc[off[1]] = (crc[off[1]] - 1) & 0xFFFFFFFF
            st = keep(order, uoffs, parity, crc)
            assert [i for i in range(len(st)) if st[i]] == off and st[off[0]] == 2 and st[off[1]] == 2
    finally:
        L.fastf_gpuinf_destroy(g)
        pin.free()


CRC_SIZES = (1, 63, 64, 65, 127, 4032, 4033, 65280, 65535)


def _crc_flip_at(isize, where):
    """the byte a flip lands on: byte 0, the last byte, or an end of lane 31's slice of gr_crc_kernel (blocks of 63 bytes or fewer:
    lane (isize - 1) // 2, since lane 31 holds nothing there)"""
    per = (isize + 63) // 64
    lane = 31 if isize > 63 else (isize - 1) // 2
    lo, hi = lane * per, min(lane * per + per, isize)
    assert lo < hi
    return {"first": 0, "last": isize - 1, "slice-first": lo, "slice-last": hi - 1}[where]


def test_keep_mode_crc_covers_every_slice_and_the_short_last_lanes():
    """blocks of 1 to 65535 bytes in one keep-mode launch: with the true CRC-32 every block reports 0; with the CRC-32 of its bytes
    with ONE byte flipped (the first, the last, either end of lane 31's slice) every block reports exactly the CRC bit.  A slice
    that the device left out of its CRC, or a short last lane it read too far, would let one of these pass."""
    import torch  # noqa: F401
    L = _api()
    pin = _Pinned(L)
    rng = np.random.default_rng(31)
    data = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in CRC_SIZES]
    entries = []
    for d in data:
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        entries.append(("crc%d" % len(d), co.compress(d) + co.flush(), len(d)))
    uoffs = [4099 + sum(CRC_SIZES[:i]) for i in range(len(CRC_SIZES))]
    assert {CRC_SIZES[i] - _crc_flip_at(CRC_SIZES[i], "last") for i in range(len(CRC_SIZES))} == {1}
    assert _crc_flip_at(4033, "slice-first") == 31 * 64 and _crc_flip_at(65, "slice-last") == 63 and _crc_flip_at(63, "slice-first") == 31
    g = L.fastf_gpuinf_create(0); assert g, L.fastf_last_error()
    try:
        cbuf, desc = _pack(pin, entries, uoffs)

        def keep(crc):
            status = (C.c_uint8 * len(entries))(*([0xFF] * len(entries)))
            crc = np.asarray(crc, dtype=np.uint32)
            assert L.fastf_gpuinf_submit_keep(g, cbuf, desc, len(entries), 0, crc.ctypes.data) == 0, L.fastf_last_error()
            assert L.fastf_gpuinf_wait(g, status, None) == 0, L.fastf_last_error()
            return list(status)

        assert keep([zlib.crc32(d) for d in data]) == [0] * len(data)
        for where in ("first", "last", "slice-first", "slice-last"):
            crc = []
            for d in data:
                m = bytearray(d); m[_crc_flip_at(len(d), where)] ^= 0x01
                assert zlib.crc32(bytes(m)) != zlib.crc32(d)
                crc.append(zlib.crc32(bytes(m)))
            assert keep(crc) == [2] * len(data), where
    finally:
        L.fastf_gpuinf_destroy(g)
        pin.free()
