"""reduce_hashed_kernel<false> (the 32-bit window set) and giant_groups_kernel on the hand-built keys of tests/k3h_ref.py.  The keys
go up as they are — no dev_sort in front: dev_reduce(skip_low=True) takes any array whose groups are contiguous — so every key sits
on the lane, unit, wave and window the fixture means.  Reference: k3h_ref.expect (plain Python; tests/test_k3h_ref_host.py holds
it against sortreduce_ref.want_rows and shows that no fixture's outcome depends on the order its keys reach the set)."""
import os

import numpy as np
import pytest

from fastf_amd import hostmem
import k3h_ref as K

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif("FASTF_K3_PER_CU" in os.environ, reason="FASTF_K3_PER_CU changes the grid the fixtures are cut for (cached per process)")]

CELLS = np.arange(1, 1001, dtype=np.uint64) | (np.uint64(1) << np.uint64(62))
FEATS = np.arange(1, 501, dtype=np.uint64) | (np.uint64(2) << np.uint64(62))
GUARD = -7
LAYS = {"bases12": (12, 46, K.L12), "bases10": (10, 42, K.L10)}


@pytest.fixture(scope="module")
def engines():
    import torch
    import fastf_amd as F
    assert torch.cuda.is_available()
    assert 3 * torch.cuda.get_device_properties(0).multi_processor_count >= 64      # up to 64 tiles: one workgroup per tile
    made = {}

    def get(kind):
        if kind not in made:
            bases, bits, lay = LAYS[kind]
            eng = F.Engine(CELLS, FEATS, umi_max_bases=bases)
            assert not eng.wide and eng.key_bits == bits and 0 < eng.skip_bits < lay.fs <= 27      # the 32-bit form is the one launched
            made[kind] = eng
        return made[kind], LAYS[kind][2]
    yield torch, get
    for eng in made.values():
        eng.close()


@pytest.fixture(scope="module")
def expected():
    memo = {}

    def get(kind, name):
        if (kind, name) not in memo:
            fx = K.fixtures(LAYS[kind][2])[name]
            memo[kind, name] = K.expect(fx.keys, fx.max_n, fx.lay)
        return memo[kind, name]
    return get


def _run(torch, eng, fx, want, segmented=False):
    rows, flagged, _ = want
    n, max_n = len(fx.keys), fx.max_n
    s = torch.cuda.current_stream().cuda_stream
    pad = np.full(max_n - n, (1 << eng.key_bits) - 1, np.uint64)
    d_keys = hostmem.to_device(np.concatenate([fx.keys, pad]), "cuda")
    d_n = torch.tensor([n], dtype=torch.int64, device="cuda")
    d_nnz = torch.zeros(1, dtype=torch.int64, device="cuda")
    if segmented:
        out = [torch.empty(max_n + 64, dtype=torch.int32).pin_memory() for _ in range(3)]
    else:
        out = [torch.empty(max_n + 64, dtype=torch.int32, device="cuda") for _ in range(3)]
    for t in out:
        t.fill_(GUARD)
    assert eng.dev_error_bits() == 0
    if segmented:
        eng.dev_reduce(d_keys.data_ptr(), d_n.data_ptr(), max_n, 0, 0, 0, d_nnz.data_ptr(), stream=s, skip_low=True, segmented=True)
        eng.dev_rows_gather(d_n.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), stream=s)
    else:
        eng.dev_reduce(d_keys.data_ptr(), d_n.data_ptr(), max_n, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), d_nnz.data_ptr(),
                       stream=s, skip_low=True)
    torch.cuda.synchronize()
    assert bool(eng.dev_error_bits() & 16) == flagged
    f, c, cnt = K.rows_arrays(rows)
    if flagged:                                               # the documented contract: clear the bit, sort fully, reduce again
        assert not segmented
        eng.dev_clear_error_bits(16, s)
        d_tmp = torch.empty_like(d_keys)
        in_tmp = eng.dev_sort(d_keys.data_ptr(), d_tmp.data_ptr(), d_n.data_ptr(), max_n, stream=s)
        src = d_tmp if in_tmp else d_keys
        for t in out:
            t.fill_(GUARD)
        eng.dev_reduce(src.data_ptr(), d_n.data_ptr(), max_n, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), d_nnz.data_ptr(), stream=s)
        torch.cuda.synchronize()
        f, c, cnt = K.reference_rows(fx)                      # (the fixtures' groups ascend: the same rows)
    assert eng.dev_error_bits() == 0
    nnz = int(d_nnz.item())
    assert nnz == len(f)
    got = [t.numpy() if segmented else hostmem.to_host(t) for t in out]
    np.testing.assert_array_equal(got[0][:nnz].astype(np.int64), f)
    np.testing.assert_array_equal(got[1][:nnz].astype(np.int64), c)
    np.testing.assert_array_equal(got[2][:nnz].astype(np.int64), cnt)
    for g in got:
        assert (g[nnz:] == GUARD).all()                       # nothing written behind the last row


NAMES12 = list(K.fixtures(K.L12))
NAMES10 = list(K.fixtures(K.L10))


@pytest.mark.parametrize("name", NAMES12)
def test_k3h_window_fixture(engines, expected, name):
    torch, get = engines
    eng, lay = get("bases12")
    _run(torch, eng, K.fixtures(lay)[name], expected("bases12", name))


@pytest.mark.parametrize("name", NAMES10)
def test_k3h_window_fixture_10_bases(engines, expected, name):
    """the same kernel under the 10-base layout (feat_shift 23: hi has 10 bits).  A step class holds at most 20 values of hi there, so
    no chain of 63 exists; the longest that does is run, and counted exactly"""
    torch, get = engines
    eng, lay = get("bases10")
    _run(torch, eng, K.fixtures(lay)[name], expected("bases10", name))


# one fixture of each family once more: the rows left in the engine's regions, then gathered into pinned host memory
SEGMENTED = ["copies_at_lane0", "singles_unit_edges", "counts_across_units", "set_words_twice", "twin3", "heads_around_nominal_ends",
             "giant_round_boundary_dups", "chain63_rank37"]


@pytest.mark.parametrize("name", SEGMENTED)
def test_k3h_window_fixture_segmented_into_pinned_memory(engines, expected, name):
    torch, get = engines
    eng, lay = get("bases12")
    F = K.fixtures(lay)
    assert {F[n].family for n in SEGMENTED} == {fx.family for fx in F.values()}
    _run(torch, eng, F[name], expected("bases12", name), segmented=True)
