"""fastf_dev_scan_tiles: the step's tile scan (scan_tiles_kernel<16>, scan_fix_kernel<16>) on hand-built counts, against
numpy.cumsum in uint64.

The contract: entries of at most 4096 (the hits of a K1 tile) — the sums inside a round of 16 384 entries are 32-bit, 16 384 x 4096
= 2^26.  Up to 16 384 entries one workgroup scans in one round; up to 64 x 16 384 one workgroup per chunk and scan_fix_kernel adds
the chunks in front; beyond that one workgroup goes round with a 64-bit carry.  The input is left all zero."""
import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import hostmem

pytestmark = pytest.mark.gpu

CHUNK = 16_384
GUARD32, GUARD64 = np.uint32(0xA5A5_5A5A), np.uint64(0x0123_4567_89AB_CDEF)
SIZES = [1, 15, 16, 17, 1023 * 16, 16_383, 16_384, 16_385, 32_768, 32_769, 49_153, 100_003, 64 * CHUNK, 64 * CHUNK + 1, 1_048_577]


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    cells = np.arange(1, 101, dtype=np.uint64) | (np.uint64(1) << np.uint64(62))
    feats = np.arange(1, 51, dtype=np.uint64) | (np.uint64(2) << np.uint64(62))
    eng = F.Engine(cells, feats, umi_max_bases=12)
    yield torch, eng
    eng.close()


def _scan(torch, eng, counts, total=True, running=None, base=True, slot=0, stream=None):
    """one call; returns (out, total, running after, base) with None where the pointer was null, and checks what every call must
    leave: the input all zero, the guard words behind both arrays as they were"""
    T = len(counts)
    d_in = hostmem.to_device(np.concatenate([counts.astype(np.uint32), np.full(40, GUARD32, np.uint32)]), "cuda")
    d_out = hostmem.to_device(np.full(T + 40, GUARD64, np.uint64), "cuda")
    d_small = hostmem.to_device(np.array([GUARD64, running if running is not None else GUARD64, GUARD64], np.uint64), "cuda")
    p = d_small.data_ptr()
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    eng.dev_scan_tiles(d_in.data_ptr(), T, d_out.data_ptr(), p if total else None, p + 8 if running is not None else None,
                       p + 16 if base else None, slot=slot, stream=s)
    torch.cuda.synchronize()
    a, o, sm = hostmem.to_host(d_in).view(np.uint32), hostmem.to_host(d_out).view(np.uint64), hostmem.to_host(d_small).view(np.uint64)
    assert not a[:T].any(), "the input is not left all zero: %s" % np.flatnonzero(a[:T])[:8]
    assert (a[T:] == GUARD32).all() and (o[T:] == GUARD64).all()
    return o[:T], int(sm[0]) if total else None, int(sm[1]) if running is not None else None, int(sm[2]), sm


def _want(counts):
    c = np.cumsum(counts.astype(np.uint64), dtype=np.uint64)
    return np.concatenate([[np.uint64(0)], c[:-1]]), int(c[-1])


def _counts(T, kind):
    rng = np.random.default_rng(T)
    if kind == "random":
        return rng.integers(0, 4097, size=T).astype(np.uint32)
    if kind == "full":
        return np.full(T, 4096, np.uint32)
    if kind == "last_only":
        c = np.zeros(T, np.uint32); c[-1] = 4096
        return c
    c = rng.integers(1, 4097, size=T).astype(np.uint32)                 # first chunk(s) all zero, later ones not
    c[:CHUNK * (1 if kind == "zero_chunk_1" else 2)] = 0
    return c


@pytest.mark.parametrize("kind", ["random", "full", "last_only"])
@pytest.mark.parametrize("T", SIZES)
def test_scan_matches_cumsum(env, T, kind):
    torch, eng = env
    counts = _counts(T, kind)
    out, total, _, base, sm = _scan(torch, eng, counts, running=None)
    w_out, w_total = _want(counts)
    if (T, kind) == (1_048_577, "full"):
        assert w_total > 1 << 32                                        # 64-bit accumulation, and the multi-round carry of one workgroup
    assert total == w_total
    np.testing.assert_array_equal(out, w_out)
    assert int(sm[1]) == int(GUARD64) and base == int(GUARD64)          # no running total: neither word is touched


@pytest.mark.parametrize("kind", ["zero_chunk_1", "zero_chunk_2"])
@pytest.mark.parametrize("T", [32_769, 49_153, 100_003, 64 * CHUNK])
def test_leading_chunks_of_zeros(env, T, kind):
    """scan_fix_kernel returns early for a chunk with nothing in front of it (off == 0): chunk 1, or chunks 1 and 2"""
    torch, eng = env
    counts = _counts(T, kind)
    assert T > 2 * CHUNK
    out, total, _, _, _ = _scan(torch, eng, counts)
    w_out, w_total = _want(counts)
    assert total == w_total and w_total > 0
    np.testing.assert_array_equal(out, w_out)


@pytest.mark.parametrize("total,running,base", [(True, 7, True), (False, 7, True), (True, 7, False), (False, 7, False), (True, None, False),
                                                (False, None, False), (False, None, True)])
@pytest.mark.parametrize("T", [17, 16_385, 64 * CHUNK + 1])
def test_null_pointer_combinations(env, T, total, running, base):
    """d_total, d_running and d_base may each be null; a word whose pointer is null, and d_base without d_running, stay untouched"""
    torch, eng = env
    counts = _counts(T, "random")
    out, got_total, got_running, got_base, sm = _scan(torch, eng, counts, total=total, running=running, base=base)
    w_out, w_total = _want(counts)
    np.testing.assert_array_equal(out, w_out)
    assert int(sm[0]) == (w_total if total else int(GUARD64))
    assert int(sm[1]) == (running + w_total if running is not None else int(GUARD64))
    assert int(sm[2]) == (running if running is not None and base else int(GUARD64))


def test_running_total_chains_over_three_calls(env):
    """*d_base = *d_running, then *d_running += the sum: three calls with different T, chunked and not (the push path's hit-rank base)"""
    torch, eng = env
    running = 5
    for T in (100_003, 4097, 64 * CHUNK + 1):
        counts = _counts(T, "random")
        _, total, after, base, _ = _scan(torch, eng, counts, running=running)
        assert base == running and after == running + _want(counts)[1] and total == _want(counts)[1]
        running = after


def test_two_slots_back_to_back_on_two_streams(env):
    """the K1 scan (slot 0) and the K3 scan (slot 1) side by side, as the pipelined sharded pass runs them: each slot has its own
    chunk totals"""
    torch, eng = env
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    jobs = []
    for rnd in range(3):
        for slot, (st, T) in enumerate(((s0, 100_003 + rnd), (s1, 49_153 + 16 * rnd))):
            counts = _counts(T, "random")
            d_in = hostmem.to_device(counts, "cuda")
            d_out = torch.zeros(T, dtype=torch.int64, device="cuda")
            d_tot = torch.zeros(1, dtype=torch.int64, device="cuda")
            jobs.append((counts, d_in, d_out, d_tot, slot, st))
    torch.cuda.synchronize()
    for counts, d_in, d_out, d_tot, slot, st in jobs:
        eng.dev_scan_tiles(d_in.data_ptr(), len(counts), d_out.data_ptr(), d_tot.data_ptr(), slot=slot, stream=st.cuda_stream)
    torch.cuda.synchronize()
    for counts, d_in, d_out, d_tot, slot, st in jobs:
        w_out, w_total = _want(counts)
        assert int(d_tot.item()) == w_total
        np.testing.assert_array_equal(hostmem.to_host(d_out).view(np.uint64), w_out)
        assert not hostmem.to_host(d_in).any()


def test_arguments_are_checked(env):
    torch, eng = env
    d = torch.zeros(64, dtype=torch.int64, device="cuda")
    with pytest.raises(F.FastfError):
        eng.dev_scan_tiles(d.data_ptr() + 4, 8, d.data_ptr())           # 16-byte aligned arrays
    with pytest.raises(F.FastfError):
        eng.dev_scan_tiles(d.data_ptr(), 8, d.data_ptr() + 256, slot=2)
    with pytest.raises(F.FastfError):
        eng.dev_scan_tiles(d.data_ptr(), 0, d.data_ptr() + 256)
