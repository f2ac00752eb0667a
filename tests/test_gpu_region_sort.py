"""The region-map sort — fastf_dev_set_regions, then fastf_dev_sort(FASTF_SORT_SEGMENTED) — on regions named by hand
(seg_scan_kernel, seg_tiles_kernel, seg_region_of / seg_phys, tile_count_kernel<true>, scatter_kernel<-1, true>) against
np.sort of the logical keys.  Every slack slot of the buffer holds a poison key that is all ones in the sorted bits: a kernel
that reads one shows it at the end of its output."""
import numpy as np
import pytest

from fastf_amd import hostmem
import sortreduce_ref as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import fastf_amd as F
    assert torch.cuda.is_available()
    cells = np.arange(1, 1001, dtype=np.uint64) | (np.uint64(1) << np.uint64(62))
    feats = np.arange(1, 501, dtype=np.uint64) | (np.uint64(2) << np.uint64(62))
    eng = F.Engine(cells, feats, umi_max_bases=12)
    assert eng.key_bits == S.KEY_BITS
    yield torch, eng
    eng.close()


@pytest.mark.parametrize("skip_low", [False, True], ids=["full", "skip_low"])
@pytest.mark.parametrize("name", list(S.REGION_CASES))
def test_segmented_sort_of_hand_built_regions(env, name, skip_low, monkeypatch):
    torch, eng = env
    case = S.REGION_CASES[name]
    counts, stride, R = case["counts"], case["stride"], len(case["counts"])
    if case["ipt"]:
        monkeypatch.setenv("FASTF_SORT_IPT", str(case["ipt"]))      # (read at every sort: the tile is ipt * 512 keys)
    n, max_n = int(counts.sum()), R * stride
    rng = np.random.default_rng(R * 1000 + n)
    keys = S.layout_keys(rng, n, umi_values=64 if case["reduce"] else 1 << 24)
    assert not (keys == S.POISON).any()
    d_keys = hostmem.to_device(S.regions_buffer(counts, stride, keys), "cuda")
    guard = np.uint64(0x0123_4567_89AB)
    d_tmp = hostmem.to_device(np.full(max_n, guard, np.uint64), "cuda")
    d_counts = hostmem.to_device(counts.astype(np.uint64), "cuda")
    d_n = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    eng.dev_set_regions(d_counts.data_ptr(), R, stride, d_n.data_ptr(), stream=s)
    in_tmp = eng.dev_sort(d_keys.data_ptr(), d_tmp.data_ptr(), d_n.data_ptr(), max_n, stream=s, skip_low=skip_low, segmented=True)
    torch.cuda.synchronize()
    assert int(d_n.item()) == n
    assert eng.dev_error_bits() == 0
    src = d_tmp if in_tmp else d_keys
    got = hostmem.to_host(src).view(np.uint64)
    if n == 0:                                                      # nothing to sort: the scratch buffer is untouched
        assert (hostmem.to_host(d_tmp).view(np.uint64) == guard).all()
        return
    assert not (got[:n] == S.POISON).any()
    if skip_low:
        skip = eng.skip_bits
        assert 0 < skip < S.FS
        assert (np.diff((got[:n] >> np.uint64(skip)).astype(np.int64)) >= 0).all()      # sorted on the bits above skip_bits
        np.testing.assert_array_equal(np.sort(got[:n]), np.sort(keys))                   # a permutation of the logical keys
    else:
        np.testing.assert_array_equal(got[:n], np.sort(keys))
    if case["reduce"]:
        d_f = torch.empty(max_n, dtype=torch.int32, device="cuda"); d_c = torch.empty_like(d_f); d_k = torch.empty_like(d_f)
        d_nnz = torch.zeros(1, dtype=torch.int64, device="cuda")
        eng.dev_reduce(src.data_ptr(), d_n.data_ptr(), max_n, d_f.data_ptr(), d_c.data_ptr(), d_k.data_ptr(), d_nnz.data_ptr(),
                       stream=s, skip_low=skip_low)
        torch.cuda.synchronize()
        assert eng.dev_error_bits() == 0
        f, c, k = S.want_rows(keys)
        assert int(d_nnz.item()) == len(f)
        np.testing.assert_array_equal(hostmem.to_host(d_f)[:len(f)].astype(np.int64), f)
        np.testing.assert_array_equal(hostmem.to_host(d_c)[:len(f)].astype(np.int64), c)
        np.testing.assert_array_equal(hostmem.to_host(d_k)[:len(f)].astype(np.int64), k)
