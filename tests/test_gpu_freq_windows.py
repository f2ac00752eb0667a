"""freq's device parse (csrc/fastq_kernels.hpp: fq_count / fq_scan / fq_pending / fq_emit / fq_scatter) driven through the handle
API fastf_taghist_create -> fastf_fqparse_create -> submit / wait per window -> end -> fastf_fqparse_fetch_keys with hand-built
FASTQ text, read by read and window by window, against tests/fqwin_ref.py (proved against the host build of the kernels' own
functions, and shown to notice each wrong rule, in tests/test_fqwin_ref_host.py).  No subprocess, no gzip, no oracle binary: the
pinned staging is built here as fastq_cmds.c builds it (FQ_HDR bytes of what preceded, the window, 64 zero bytes).

Before every run the device buffers are poisoned: a full window of '\\n' goes through each parity of a throw-away handle, which
is destroyed and created again, so stale newlines lie behind every shorter window; and fastf_fqparse_scatter writes a sentinel
key (bit 63 clear) to every read below the bound and to a guard behind it.  A read the parse never resolved keeps the sentinel;
a changed word at or beyond the bound is a write out of range.

Everything compared is integers and bytes; every comparison is exact."""
import collections
import ctypes as C

import numpy as np
import pytest

from fastf_amd import _lib

import fqwin_ref as Q

pytestmark = pytest.mark.gpu

HDR, TILE = Q.FQ_HDR, Q.TILE
SENTINEL = 0x5A5A5A5A5A5A5A5A
GUARD = 64


class Esc(C.Structure):
    _fields_ = [("s", C.c_uint64), ("r", C.c_uint64)]


def api():
    L = _lib.lib()
    vp, u64, u32, sz = C.c_void_p, C.c_uint64, C.c_uint32, C.c_size_t
    L.fastf_fqparse_create.argtypes = [vp, sz, u32, C.POINTER(vp)]
    L.fastf_fqparse_destroy.argtypes = [vp]
    L.fastf_fqparse_destroy.restype = None
    L.fastf_fqparse_submit.argtypes = [vp, vp, sz, u64, C.c_int, u64]
    L.fastf_fqparse_wait.argtypes = [vp, C.c_int, C.POINTER(C.POINTER(Esc)), C.POINTER(u32), C.POINTER(u64), vp, vp]
    L.fastf_fqparse_end.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u32), C.POINTER(u64)]
    L.fastf_fqparse_scatter.argtypes = [vp, vp, sz, u64]
    L.fastf_fqparse_fetch_keys.argtypes = [vp, vp, u64, u64]
    return L


def new_hist():
    h = C.c_void_p()
    _lib.check(api().fastf_taghist_create(0, C.byref(h)))
    return h


@pytest.fixture(scope="module")
def hist():
    """one histogram for the tests that never push: its key array is only reserved, read r at word r"""
    h = new_hist()
    yield h
    _lib.lib().fastf_taghist_destroy(h)


class Dev:
    """parse handles of window size W and key length L on one histogram, and the two pinned stagings"""

    def __init__(self, hist, W, L):
        self.A, self.h, self.W, self.L, self.p = api(), hist, W, L, None
        self.ptr = [self.A.fastf_pinned_alloc(HDR + W + 64) for _ in range(2)]
        assert all(self.ptr)
        self.stage = [np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(HDR + W + 64,)) for p in self.ptr]

    def __enter__(self):
        return self

    def __exit__(self, *a):
        if self.p:
            self.A.fastf_fqparse_destroy(self.p)
        for p in self.ptr:
            self.A.fastf_pinned_free(p)

    def err(self):
        return self.A.fastf_last_error().decode(errors="replace")

    def _create(self):
        p = C.c_void_p()
        _lib.check(self.A.fastf_fqparse_create(self.h, self.W, self.L, C.byref(p)))
        return p

    def fresh(self):
        """a new handle; the two device buffers of the one before it last held W newlines"""
        if self.p:
            self.A.fastf_fqparse_destroy(self.p)
            self.p = None
        p = self._create()
        for par in (0, 1):
            self.stage[par][:HDR] = 10 if par else 0
            self.stage[par][HDR:HDR + self.W] = 10
            _lib.check(self.A.fastf_fqparse_submit(p, self.ptr[par], self.W, par * self.W, 0, self.W // 2 + 4))
        n_nl = C.c_uint64()
        for par in (0, 1):
            _lib.check(self.A.fastf_fqparse_wait(p, par, None, C.byref(C.c_uint32()), C.byref(n_nl), None, None))
        assert n_nl.value == 2 * self.W
        self.A.fastf_fqparse_destroy(p)
        self.p = self._create()

    def scatter(self, pairs, cap):
        rk = np.ascontiguousarray(pairs, dtype=np.uint64).reshape(-1, 2)
        return self.A.fastf_fqparse_scatter(self.p, rk.ctypes.data if len(rk) else None, len(rk), cap)

    def fetch(self, lo, n):
        out = np.empty(n, dtype=np.uint64)
        assert self.A.fastf_fqparse_fetch_keys(self.p, out.ctypes.data, lo, n) == 0, self.err()
        return out

    def wait(self, par):
        pe, ne, n_nl = C.POINTER(Esc)(), C.c_uint32(), C.c_uint64()
        rc = self.A.fastf_fqparse_wait(self.p, par, C.byref(pe), C.byref(ne), C.byref(n_nl), None, None)
        esc = sorted((pe[q].s, pe[q].r) for q in range(ne.value))           # copied at once: valid until the next wait
        return dict(rc=rc, msg=self.err() if rc else "", esc=esc, n_nl=n_nl.value)

    def run(self, text, lens, bound, stepwise=False):
        """text through the windows `lens` -> (per window dict(rc, msg, esc, n_nl[, keys]), end dict).  stepwise: every window
        is waited for and the keys below `bound` are fetched before the next is submitted; otherwise two windows are in flight
        as in fastq_cmds.c (window k - 2 is waited for when its staging is due again), and a third submit is shown refused."""
        t = Q.as_u8(text)
        assert sum(lens) == len(t) and max(lens) <= self.W
        self.fresh()
        total = bound + GUARD
        assert self.scatter(np.stack([np.arange(total, dtype=np.uint64), np.full(total, SENTINEL, dtype=np.uint64)], axis=1), total) == 0, self.err()
        res, a = [None] * len(lens), 0
        for k, ln in enumerate(lens):
            par, st = k & 1, self.stage[k & 1]
            if k >= 2 and not stepwise:
                if k == 2:
                    assert self.A.fastf_fqparse_submit(self.p, self.ptr[par], ln, a, 0, bound) == 1 and "was not waited for" in self.err()
                res[k - 2] = self.wait(par)
            h = min(a, HDR)
            st[:HDR - h] = 0
            st[HDR - h:HDR] = t[a - h:a]
            st[HDR:HDR + ln] = t[a:a + ln]
            st[HDR + ln:HDR + ln + 64] = 0
            assert self.A.fastf_fqparse_submit(self.p, self.ptr[par], ln, a, int(k == len(lens) - 1), bound) == 0, self.err()
            if stepwise:
                res[k] = self.wait(par)
                res[k]["keys"] = self.fetch(0, bound)
            a += ln
        for k in range(max(len(lens) - 2, 0), len(lens)):
            if res[k] is None:
                res[k] = self.wait(k & 1)
        n_nl, ls, err, rec = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint64()
        _lib.check(self.A.fastf_fqparse_end(self.p, C.byref(n_nl), C.byref(ls), C.byref(err), C.byref(rec)))
        return res, dict(n_nl=n_nl.value, line_start=ls.value, err=err.value, err_rec=rec.value)


def check(dev, f, stepwise=False):
    """fixture f on the device against the model: escapes and n_nl per window, the carried state at the end, and every word of
    the key array up to the guard behind the bound; stepwise: the key array after every window"""
    want, wend = f.expected()
    got, gend = dev.run(f.text, f.lens, f.bound, stepwise)
    exp = np.full(f.bound + GUARD, SENTINEL, dtype=np.uint64)
    for k, (g, w) in enumerate(zip(got, want)):
        where = "%r window %d of %d (a=%d len=%d)" % (f, k, len(want), w["a"], w["len"])
        assert g["rc"] == 0, where + ": " + g["msg"]
        assert g["esc"] == w["esc"], where
        assert g["n_nl"] == w["n_nl"], where
        for r, key in w["keys"].items():
            exp[r] = key
        if stepwise:
            bad = np.flatnonzero(g["keys"] != exp[:f.bound])
            assert not len(bad), "%s: key of read %d is %#x, not %#x" % (where, bad[0], g["keys"][bad[0]], exp[bad[0]])
    assert gend == wend, f
    assert dev.scatter([], f.bound + GUARD) == 0, dev.err()                  # (reserves up to the guard again; writes nothing)
    keys = dev.fetch(0, f.bound + GUARD)
    bad = np.flatnonzero(keys != exp)
    assert not len(bad), "%r: key of read %d is %#x, not %#x (bound %d)" % (f, bad[0], keys[bad[0]], exp[bad[0]], f.bound)
    return want, wend


def check_group(hist, fxs, stepwise=False):
    assert fxs
    for key in sorted({(f.W, f.L) for f in fxs}):
        with Dev(hist, *key) as dev:
            for f in fxs:
                if (f.W, f.L) == key:
                    check(dev, f, stepwise)


# ---------------------------------------------------------------- boundary sweeps
@pytest.mark.parametrize("which", ["s&3=0", "s&3=1", "s&3=2", "s&3=3", "tile edge", "newline ends"])
def test_dna_boundary_sweep(hist, which):
    check_group(hist, [f for f in Q.group("dna_sweep") if f.name.startswith(which)], stepwise=True)


@pytest.mark.parametrize("L", [40, 1024])
def test_escape_boundary_sweep(hist, L):
    fxs = [f for f in Q.group("esc_sweep") if f.L == L]
    assert len(fxs) == 7
    check_group(hist, fxs, stepwise=True)


@pytest.mark.parametrize("L", [40, 5])
def test_most_lines_one_window_hands_on(hist, L):
    fxs = [f for f in Q.group("max_pend") if f.L == L]
    assert max(len(f.expected()[0][0]["pend"]) for f in fxs) == (256 if L == 40 else 2)
    check_group(hist, fxs, stepwise=True)
    check_group(hist, fxs)


def test_zero_length_last_window(hist):
    check_group(hist, Q.group("zero_last"), stepwise=True)


def test_many_windows_with_escapes_in_every_one(hist):
    check_group(hist, Q.group("many_windows"))
    check_group(hist, Q.group("many_windows"), stepwise=True)


@pytest.mark.parametrize("L", [0, 1, 26, 31, 32])
def test_key_kinds(hist, L):
    check_group(hist, [f for f in Q.group("key_kinds") if f.L == L], stepwise=True)


def test_long_lines(hist):
    fxs = Q.group("long_lines")
    check_group(hist, fxs)
    check_group(hist, [f for f in fxs if "offender" in f.name or "boundaries" in f.name], stepwise=True)


def test_more_than_1024_tiles(hist):
    check_group(hist, Q.group("big"))


# ---------------------------------------------------------------- capacity words
def test_capacity_words(hist):
    f = Q.group("many_windows")[0]
    n = Q.n_reads(f.text)
    with Dev(hist, f.W, f.L) as dev:
        # an escape key for a read at key_cap is refused, the one below it is written
        dev.fresh()
        total = n + GUARD
        assert dev.scatter([(r, SENTINEL) for r in range(total)], total) == 0
        assert dev.scatter([(total - 1, 7)], total) == 0
        assert dev.scatter([(total, 9)], total) == 1 and "out of range" in dev.err()
        exp = np.full(total, SENTINEL, dtype=np.uint64)
        exp[total - 1] = 7
        assert np.array_equal(dev.fetch(0, total), exp)
        assert dev.A.fastf_fqparse_fetch_keys(dev.p, np.empty(2, dtype=np.uint64).ctypes.data, total - 1, 2) == 1 and "beyond" in dev.err()
        assert dev.A.fastf_fqparse_fetch_keys(dev.p, None, total, 0) == 0
        # a key_bound one read too small: the error word from wait, the last read's key not written
        bound = n - 1
        want, wend = Q.run(f.text, f.lens, f.L, bound)
        assert wend["err"] == Q.ERR_KEY_CAP and not want[-2]["err"]
        got, gend = dev.run(f.text, f.lens, bound)
        exp = np.full(bound + GUARD, SENTINEL, dtype=np.uint64)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g["n_nl"] == w["n_nl"]
            if w["err"]:
                assert g["rc"] == 1 and "capacity" in g["msg"], k
            else:
                assert g["rc"] == 0 and g["esc"] == w["esc"], k
            for r, key in w["keys"].items():
                exp[r] = key
        assert gend == wend
        assert dev.scatter([], bound + GUARD) == 1                           # (the error word stays; the reservation is made)
        assert np.array_equal(dev.fetch(0, bound + GUARD), exp) and (exp[bound:] == SENTINEL).all()


# ---------------------------------------------------------------- the handoff into the histogram
def test_handoff_into_the_tag_histogram():
    f, = [f for f in Q.group("key_kinds") if f.name == "L=26 whole, two windows"]
    n = Q.n_reads(f.text)
    A = api()
    A.fastf_taghist_reserve_device.argtypes = [C.c_void_p, C.c_size_t]
    A.fastf_taghist_reserve_device.restype = C.c_void_p
    A.fastf_taghist_push_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    A.fastf_taghist_finish.argtypes = [C.c_void_p, C.POINTER(_lib.TagHistResult)]
    h = new_hist()
    try:
        with Dev(h, f.W, f.L) as dev:
            got, gend = dev.run(f.text, f.lens, f.bound)
            per_read = Q.reads(f.text, f.L)
            assert len(per_read) == n and gend["err"] == 0
            # the host's part: escape strings interned in the order they arrive, key = 1 + ordinal
            table, pairs = {}, []
            for g in got:
                for s, r in g["esc"]:
                    pairs.append((r, 1 + table.setdefault(Q.key_string(f.text, s, f.L)[0], len(table))))
            want = [k if k else 1 + table[Q.key_string(f.text, s, f.L)[0]] for s, k in per_read]
            assert len(pairs) == sum(1 for s, k in per_read if not k) > 10 and len(table) > 5
            assert dev.scatter(pairs, n) == 0, dev.err()
            assert dev.fetch(0, n).tolist() == want
            d = A.fastf_taghist_reserve_device(h, n)
            assert d
            _lib.check(A.fastf_taghist_push_device(h, d, n))
            res = _lib.TagHistResult()
            _lib.check(A.fastf_taghist_finish(h, C.byref(res)))
            cnt = collections.Counter(want)
            first = {}
            for r, k in enumerate(want):
                first.setdefault(k, r)
            keys = sorted(cnt)
            assert (res.n_records, res.n_valid, res.n1) == (n, n, len(keys))
            assert [res.key1[i] for i in range(res.n1)] == keys
            assert [res.count1[i] for i in range(res.n1)] == [cnt[k] for k in keys]
            assert [res.first1[i] for i in range(res.n1)] == [first[k] for k in keys]
    finally:
        A.fastf_taghist_destroy(h)
