"""The plain C++ part of coexpr_kernels.hpp on the CPU (build/libcoex_host.so, compiled by g++ from the header the device compiles):
the per-gene walk of coex_select_kernel against coexpr_ref.partner_sets on every fixture for k = 1, 15 and 64, with the list slots
packed and strided as in the LDS of a workgroup; the digit recombination against Python ints at the i32 bound; the padded shape and
the address of every plane byte."""
import ctypes as C
import os

import numpy as np
import pytest

import coexpr_ref as R
import coexpr_dev_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COEX_HOST = os.path.join(ROOT, "build", "libcoex_host.so")
u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p


@pytest.fixture(scope="module")
def cx():
    L = C.CDLL(COEX_HOST)
    L.coex_host_select.argtypes = [vp, vp, u32, u32, u32, u32, vp, vp]
    L.coex_host_recombine.argtypes = [vp, C.c_int]
    L.coex_host_recombine.restype = u64
    L.coex_host_pad.argtypes = [u32, u32, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    L.coex_host_pad.restype = None
    L.coex_host_plane_at.argtypes = [u32] * 5
    L.coex_host_plane_at.restype = u64
    L.coex_host_digit.argtypes = [u32, u32]
    L.coex_host_digit.restype = u32
    L.coex_host_default_chunk.restype = u32
    L.coex_host_chunk_max.restype = u32
    return L


def walk(cx, D, S, n, k, stride):
    K = len(S)
    d, s = np.array(D, np.uint64).reshape(K, K), np.array(S, np.uint64)
    idx, cnt = np.full((K, k), 7, np.uint32), np.full(K, 7, np.uint32)
    assert cx.coex_host_select(d.ctypes.data, s.ctypes.data, n, K, k, stride, idx.ctypes.data, cnt.ctypes.data) == 0
    assert all((idx[g, cnt[g]:] == 0xFFFFFFFF).all() for g in range(K))
    return X.as_lists(idx, cnt)


def test_the_census_of_the_device_fixtures():
    assert X.census()


@pytest.mark.parametrize("k", X.KS)
@pytest.mark.parametrize("name", sorted(X.ALL))
def test_the_walk_against_the_reference(cx, name, k):
    D, S = X.reference(name)
    n = X.fixture(name)[1]
    want = X.sets(name, k)
    assert walk(cx, D, S, n, k, 1) == want
    assert walk(cx, D, S, n, k, 64) == want


def test_the_walk_keeps_the_lower_slot_across_the_second_64(cx):
    D, S = X.reference("tie_63_64")
    assert walk(cx, D, S, 10, 2, 64)[0] == [1, 63] and walk(cx, D, S, 10, 3, 64)[0] == [1, 63, 64]


def test_recombination_at_the_i32_bound(cx):
    top = 3 * cx.coex_host_chunk_max() * 127 * 127
    assert top < 1 << 31 <= 3 * (cx.coex_host_chunk_max() + 32) * 127 * 127
    assert cx.coex_host_default_chunk() % 32 == 0 and 32 <= cx.coex_host_default_chunk() <= 32768
    rng = np.random.default_rng(3)
    cases = [[top] * 5, [(1 << 31) - 1] * 5, [0] * 5, [1, 0, 0, 0, 0], [0, 0, 0, 0, (1 << 31) - 1], [96 * 127 * 127, 2 * 96 * 127 * 127, 3 * 96 * 127 * 127, 2 * 96 * 127 * 127, 96 * 127 * 127]]
    cases += [[int(v) for v in rng.integers(0, 1 << 31, 5)] for _ in range(200)]
    for acc in cases:
        a = np.array(acc, np.int32)
        for T in (1, 3, 5):
            assert cx.coex_host_recombine(a.ctypes.data, T) == sum(acc[t] << (7 * t) for t in range(T))
    # the digits of two counts multiplied and recombined are their product
    for x, y in ((X.TOP3, X.TOP3), (16384, 127), (128, 16383), (1, X.TOP3)):
        dx, dy = [cx.coex_host_digit(x, p) for p in range(3)], [cx.coex_host_digit(y, p) for p in range(3)]
        assert sum(d << (7 * p) for p, d in enumerate(dx)) == x
        acc = np.zeros(5, np.int32)
        for a in range(3):
            for b in range(3):
                acc[a + b] += dx[a] * dy[b]
        assert cx.coex_host_recombine(acc.ctypes.data, 5) == x * y


def test_padded_shape_and_plane_addresses(cx):
    for n, K, chunk in ((1, 1, 8192), (31, 31, 32), (33, 65, 32), (65, 97, 32), (96, 2, 96), (8224, 2, 8192), (100, 0, 64), (0, 5, 8192), (4000, 2000, 8192)):
        kp, npad, ce = u32(), u32(), u32()
        cx.coex_host_pad(n, K, chunk, C.byref(kp), C.byref(npad), C.byref(ce))
        kp, npad, ce = kp.value, npad.value, ce.value
        n32 = max(32, (n + 31) // 32 * 32)
        assert kp % 32 == 0 and kp >= max(K, 1) and kp - K <= 32 and ce == min(chunk, n32) and npad % ce == 0 and n32 <= npad < n32 + ce
        seen = set()
        for p in range(3):
            for slot in {0, K // 2, max(K, 1) - 1}:
                for cell in {0, n // 2, max(n, 1) - 1}:
                    at = cx.coex_host_plane_at(p, slot, cell, kp, npad)
                    assert at == (p * kp + slot) * npad + cell and at < 3 * kp * npad
                    seen.add(at)
        assert len(seen) == 3 * len({0, K // 2, max(K, 1) - 1}) * len({0, n // 2, max(n, 1) - 1})
