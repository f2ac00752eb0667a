"""K3u — fastf_dev_umi_rows: reduce_windows_kernel<true> + rows_gather_kernel<true> — on fully sorted keys with chosen run
lengths.  Every distinct key is a group of its own here and the count is the run length, so a run longer than a 2048-key
window is an open row carried over equal keys; the reference is np.unique(..., return_counts=True)."""
import numpy as np
import pytest

from fastf_amd import hostmem
import sortreduce_ref as S

pytestmark = pytest.mark.gpu

GUARD_KEY, GUARD_COUNT = np.uint64(0x7E57_7E57_7E57_7E57), -7


@pytest.fixture(scope="module")
def env():
    import torch
    import fastf_amd as F
    assert torch.cuda.is_available()
    cells = np.arange(1, 1001, dtype=np.uint64) | (np.uint64(1) << np.uint64(62))
    feats = np.arange(1, 501, dtype=np.uint64) | (np.uint64(2) << np.uint64(62))
    eng = F.Engine(cells, feats, umi_max_bases=12)
    yield torch, F, eng
    eng.close()


def _umi_rows(torch, eng, keys, max_n):
    n = len(keys)
    assert (np.diff(keys.astype(np.int64)) >= 0).all() and keys.max() < S.POISON
    # behind the n keys the device-side count names: the largest key, up to the caller's bound
    d_keys = hostmem.to_device(np.concatenate([keys, np.full(max_n - n, S.POISON, np.uint64)]), "cuda")
    d_n = torch.tensor([n], dtype=torch.int64, device="cuda")
    d_uk = hostmem.to_device(np.full(max_n + 1, GUARD_KEY, np.uint64), "cuda")
    d_nc = torch.full((max_n + 1,), GUARD_COUNT, dtype=torch.int32, device="cuda")
    d_rows = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    eng.dev_umi_rows(d_keys.data_ptr(), d_n.data_ptr(), max_n, d_uk.data_ptr(), d_nc.data_ptr(), d_rows.data_ptr(), stream=s)
    torch.cuda.synchronize()
    assert eng.dev_error_bits() == 0
    want_k, want_c = S.umi_rows_ref(keys)
    rows = int(d_rows.item())
    assert rows == len(want_k)
    got_k, got_c = hostmem.to_host(d_uk).view(np.uint64), hostmem.to_host(d_nc)
    np.testing.assert_array_equal(got_k[:rows], want_k)
    np.testing.assert_array_equal(got_c[:rows].astype(np.int64), want_c)
    assert (got_k[rows:] == GUARD_KEY).all() and (got_c[rows:] == GUARD_COUNT).all()     # nothing behind the last row
    return d_n


@pytest.mark.parametrize("bound", [1, 7], ids=["tight", "loose7x"])
@pytest.mark.parametrize("name", list(S.UMI_RUN_CASES))
def test_umi_rows_run_lengths(env, name, bound):
    """loose7x: the launch is sized for seven times the key count on the device — the first chunks are empty and a chunk's
    nominal end falls inside a run"""
    torch, F, eng = env
    keys = S.run_keys(name)
    _umi_rows(torch, eng, keys, bound * len(keys))


@pytest.mark.parametrize("bound", [1, 7], ids=["tight", "loose7x"])
def test_umi_rows_null_keys_form_their_own_runs(env, bound):
    torch, F, eng = env
    keys = S.null_run_keys()
    _umi_rows(torch, eng, keys, bound * len(keys))


def test_matrix_gather_after_umi_rows_is_refused(env):
    torch, F, eng = env
    keys = S.run_keys("long_and_short")
    d_n = _umi_rows(torch, eng, keys, len(keys))
    d_f = torch.full((len(keys),), -7, dtype=torch.int32, device="cuda"); d_c = d_f.clone(); d_k = d_f.clone()
    with pytest.raises(F.FastfError, match="other kind"):
        eng.dev_rows_gather(d_n.data_ptr(), d_f.data_ptr(), d_c.data_ptr(), d_k.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (hostmem.to_host(d_f) == -7).all() and (hostmem.to_host(d_k) == -7).all()
    assert eng.dev_error_bits() == 0
