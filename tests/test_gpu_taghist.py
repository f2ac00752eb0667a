"""The tag-histogram seam of crb / extract / freq (csrc/tag_hist.hpp: fastf_taghist_push / reserve_device / push_device / finish)
on the hand-built keys of tests/taghist_ref.py, every array of the result against the numpy reference, bit for bit.  The
fixtures are proved able to see a dropped sort pass, a pair-code digit too few and a missing fill correction in
tests/test_taghist_ref_host.py.  What each group pins:

  mask_*                      th_pass_mask / th_sort: passes over some digits and not others, an odd and an even number of them
  digits_m1_*, digits_m2_*    finish: the varying digits of the pair code from bits_for(m1) and bits_for(m2 - 1)
  fill_*, one_present_*, dead_key1, first_valid_late
                              th_fill_copy_kernel's fill record and the host's correction of the fill key's count
  first_edges                 th_first_index_kernel at workgroup edges and for a key in every workgroup
  extremes                    keys 1 and 2^64 - 1, single bits, a real all-ones key in the scatter's padded last tile
  runs                        reduce_windows_kernel<true>'s window edges seen through this seam
  grid_stride, pair_grid_stride   a second iteration of every grid-capped th_* loop
  grows, pair_grows           th_grow: the copy of the pushed and the reserved keys into a larger array
  one_key1_300k, forty_key1   th_par_for's slices that move to the next change of key1
"""
import ctypes as C

import numpy as np
import pytest

from fastf_amd import _lib, hostmem
from fastf_amd.tags import TagHist
import taghist_ref as T

pytestmark = pytest.mark.gpu

MIXED = "single-tag and tag-pair pushes cannot be mixed"
D2D = 3                                                             # hipMemcpyDeviceToDevice


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    L = _lib.lib()
    L.fastf_devmem_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    hip = C.CDLL(_lib.hip_runtimes_loaded()[0])                     # the ONE runtime of this process (by path: no second copy)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return torch, L, hip


class Hist(TagHist):
    """TagHist plus the device-side entries; device keys come from tensors made by hostmem.to_device"""

    def __init__(self, dev):
        super().__init__()
        self.torch, self.L, self.hip = dev
        self.stream = self.L.fastf_taghist_stream(self.h)
        assert self.stream

    def reserve(self, n):
        d = self.L.fastf_taghist_reserve_device(self.h, n)
        assert d, self.L.fastf_last_error()
        return d

    def write(self, d_dst, d_src, a, b):
        """records [a, b) of the tensor d_src to d_dst, on the histogram's stream"""
        assert 0 <= a < b <= d_src.numel()
        assert self.hip.hipMemcpyAsync(d_dst, d_src.data_ptr() + 8 * a, 8 * (b - a), D2D, self.stream) == 0

    def push_device(self, d, n):
        _lib.check(self.L.fastf_taghist_push_device(self.h, d, n))

    def push_reserved(self, d_src, a, b):
        d = self.reserve(b - a)
        self.write(d, d_src, a, b)
        self.push_device(d, b - a)                                  # the no-copy branch

    def push_foreign(self, d_src, a, b):
        self.push_device(d_src.data_ptr() + 8 * a, b - a)           # the copy branch

    def read(self, d, n):
        """n keys at device address d, through fastf_devmem_copy"""
        back = self.torch.zeros(n, dtype=self.torch.int64, device="cuda")
        self.torch.cuda.synchronize()
        assert self.L.fastf_devmem_copy(back.data_ptr(), d, 8 * n) == 0, self.L.fastf_last_error()
        return hostmem.to_host(back).view(np.uint64)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def check_single(r, name):
    u, c, first = T.want(name)
    k = T.SINGLE[name]["k1"]
    assert (r["n_records"], r["n_valid"], r["n_key1_present"]) == (len(k), int(c.sum()), int(c.sum())), name
    np.testing.assert_array_equal(r["key1"], u, name)
    np.testing.assert_array_equal(r["count1"], c, name)
    np.testing.assert_array_equal(r["first1"], first, name)
    assert "pair_k1" not in r


def check_pairs(r, w, name):
    assert (r["n_records"], r["n_valid"], r["n_key1_present"]) == (w["n_records"], w["n_valid"], w["n_key1_present"]), name
    for what in ("key1", "count1", "first1", "pair_k1", "pair_key2", "pair_count", "pair_first"):
        assert r[what].dtype == w[what].dtype, what
        np.testing.assert_array_equal(r[what], w[what], "%s: %s" % (name, what))


# ---------------------------------------------------------------- host pushes
@pytest.mark.parametrize("name", list(T.SINGLE))
def test_single_fixture_through_host_pushes(dev, name):
    k = T.SINGLE[name]["k1"]
    with Hist(dev) as h:
        for a, b in T.pieces(T.SINGLE[name]):
            h.push(k[a:b])
        check_single(h.finish(), name)


@pytest.mark.parametrize("name", list(T.PAIRS))
def test_pair_fixture_through_host_pushes(dev, name):
    """pair_grows is the growth of both key arrays across two host pushes"""
    f = T.PAIRS[name]
    with Hist(dev) as h:
        for a, b in T.pieces(f):
            h.push(f["k1"][a:b], f["k2"][a:b])
        r = h.finish()
    check_pairs(r, T.want(name), name)
    if name == "dead_key1":                                          # listed at level 1, with no record and no first index
        at = np.searchsorted(r["key1"], f["dead"])
        np.testing.assert_array_equal(r["key1"][at], f["dead"])
        assert (r["count1"][at] == 0).all() and (r["first1"][at] == np.uint64(T.NONE)).all()
        assert int((r["count1"] == 0).sum()) == 3 and not np.isin(r["pair_k1"], at).any()


# ---------------------------------------------------------------- device pushes
@pytest.mark.parametrize("how", ["reserved", "foreign"])
@pytest.mark.parametrize("name", list(T.SINGLE))
def test_single_fixture_through_device_pushes(dev, name, how):
    f = T.SINGLE[name]
    d_src = hostmem.to_device(f["k1"], "cuda")
    with Hist(dev) as h:
        for a, b in T.pieces(f):
            (h.push_reserved if how == "reserved" else h.push_foreign)(d_src, a, b)
        check_single(h.finish(), name)


@pytest.mark.parametrize("how", ["reserved", "foreign"])
@pytest.mark.parametrize("name", ["fill_once", "first_edges", "one_present_last"])
def test_host_push_then_device_push(dev, name, how):
    """the first piece from the host, the others from the device: the first present record of fill_once and of
    one_present_last lies in a device piece (first_present1 = records pushed so far + the kernel's index), first_edges
    has present keys on either side"""
    f = T.SINGLE[name]
    d_src = hostmem.to_device(f["k1"], "cuda")
    (a0, b0), rest = T.pieces(f)[0], T.pieces(f)[1:]
    assert rest and (name == "first_edges") == bool(f["k1"][a0:b0].any())
    with Hist(dev) as h:
        h.push(f["k1"][a0:b0])
        for a, b in rest:
            (h.push_reserved if how == "reserved" else h.push_foreign)(d_src, a, b)
        check_single(h.finish(), name)


# ---------------------------------------------------------------- growth
def test_a_reservation_survives_the_growth_of_the_array(dev):
    f = T.SINGLE["grows"]
    n = len(f["k1"])
    assert n > T.FIRST_ALLOC
    d_src = hostmem.to_device(f["k1"], "cuda")
    with Hist(dev) as h:
        h.write(h.reserve(1000), d_src, 0, 1000)
        d = h.reserve(n)                                            # more than the first allocation: the array grows
        np.testing.assert_array_equal(h.read(d, 1000), f["k1"][:1000])
        h.write(d + 8 * 1000, d_src, 1000, n)
        h.push_device(d, n)
        check_single(h.finish(), "grows")


def test_growth_between_a_host_push_and_a_reservation(dev):
    f = T.SINGLE["grows"]
    n = len(f["k1"])
    d_src = hostmem.to_device(f["k1"], "cuda")
    with Hist(dev) as h:
        h.push(f["k1"][:1000])
        d = h.reserve(n - 1000)
        np.testing.assert_array_equal(h.read(d - 8 * 1000, 1000), f["k1"][:1000])      # the pushed keys moved along
        h.write(d, d_src, 1000, n)
        h.push_device(d, n - 1000)
        check_single(h.finish(), "grows")


# ---------------------------------------------------------------- finish twice, modes
def test_finish_twice_gives_the_same_arrays(dev):
    f = T.SINGLE["fill_once"]
    with Hist(dev) as h:
        h.push(f["k1"])
        r1, r2 = h.finish(), h.finish()
    check_single(r1, "fill_once")
    check_single(r2, "fill_once")
    f = T.PAIRS["dead_key1"]
    with Hist(dev) as h:
        h.push(f["k1"], f["k2"])
        r1, r2 = h.finish(), h.finish()
    check_pairs(r1, T.want("dead_key1"), "dead_key1")
    check_pairs(r2, T.want("dead_key1"), "dead_key1")


def test_a_pair_push_after_a_device_push_is_refused(dev):
    f = T.SINGLE["fill_hot"]
    k = f["k1"]
    d_src = hostmem.to_device(k, "cuda")
    with Hist(dev) as h:
        h.push_foreign(d_src, 0, 1333)
        with pytest.raises(_lib.FastfError, match=MIXED):
            h.push(k[1333:], k[1333:])
        h.push_reserved(d_src, 1333, 3000)                          # the handle goes on in its own mode
        h.push(k[3000:])
        check_single(h.finish(), "fill_hot")


def test_a_device_push_after_a_pair_push_is_refused(dev):
    f = T.PAIRS["first_valid_late"]
    d_src = hostmem.to_device(f["k1"], "cuda")
    with Hist(dev) as h:
        h.push(f["k1"][:350], f["k2"][:350])
        with pytest.raises(_lib.FastfError, match=MIXED):
            h.push_foreign(d_src, 350, 700)
        assert not h.L.fastf_taghist_reserve_device(h.h, 350) and MIXED in h.L.fastf_last_error().decode()
        with pytest.raises(_lib.FastfError, match=MIXED):
            h.push(f["k1"][350:])
        h.push(f["k1"][350:], f["k2"][350:])
        check_pairs(h.finish(), T.want("first_valid_late"), "first_valid_late")
