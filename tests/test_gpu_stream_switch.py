"""FASTF_NO_STREAM_K1B is read when an engine is created and stays with that engine: the sizes it hands out
(fastf_dev_block_bytes, fastf_dev_probe_capacity) and the K1b it launches afterwards cannot disagree, whatever the
environment does in between.  Engine shape of tests/test_gpu_region_sort.py (1000 cell keys, 500 feature keys, 12 UMI bases,
gene table in LDS), records from the generator of test_gpu_parity.py::test_resident_pass_streaming_k1b_matches_oracle."""
import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import hostmem
from helpers import Case

pytestmark = pytest.mark.gpu

N = 4097       # one record past a 4096-record K1 tile: the last 256-record unit holds one record


def _resident_pass(eng, d, draws, n, dev, want_stream):
    """count hits -> probe/filter/pack -> sort -> reduce through ShardedPass (G = 1), from the blocked layout where the
    engine has one; returns (hits, sampled, valid) and the rows"""
    from fastf_amd.dist import HipStages, ShardedPass
    st = HipStages(eng, dev)
    sp = ShardedPass(st, n, dev)
    blk = st.block(d[1], d[2], d[3], n)
    assert (blk is not None) == want_stream
    if blk is not None:
        sp.run(d[0], blk, None, None, n, draws)
    else:
        sp.run(d[0], d[1], d[2], d[3], n, draws)
    rows = sp.local_coo()
    hits, sampled, valid, err = sp.global_counters()
    assert err == 0
    assert sp.st.segmented == want_stream
    return (hits, sampled, valid), rows


def test_the_switch_is_read_at_create_and_stays_with_the_engine(monkeypatch):
    import torch
    monkeypatch.delenv("FASTF_NO_STREAM_K1B", raising=False)
    case = Case(n=N, n_bar=1000, n_gene=500, rate_cell=0.5, rate_depth=0.5, p_unlisted_cb=0.2, p_bad_xf=0.2, p_n_umi=0.02)
    ora = case.oracle()
    lists = case.lists()
    dev = torch.device("cuda", 0)
    d = [hostmem.to_device(x, dev) for x in case.packed(lists)]
    draws = hostmem.to_device(F.mt_draws(case.seed, lists.mt_skip, case.n), dev)
    make = lambda: F.Engine.from_lists(lists, rate_depth=case.rate_depth, seed=case.seed, umi_max_bases=12)
    engines = []
    try:
        a = make(); engines.append(a)
        assert "LDS" in a.table_modes.split("genes:")[1]
        sizes = (a.block_bytes(N), a.probe_capacity(N))
        assert sizes[0] > 0 and sizes[1] > 0

        monkeypatch.setenv("FASTF_NO_STREAM_K1B", "1")
        assert (a.block_bytes(N), a.probe_capacity(N)) == sizes           # A keeps what it was created with
        b = make(); engines.append(b)
        assert (b.block_bytes(N), b.probe_capacity(N)) == (0, 0)
        res_a = _resident_pass(a, d, draws, N, dev, want_stream=True)     # the streaming K1b on blocked records
        res_b = _resident_pass(b, d, draws, N, dev, want_stream=False)    # the tile form
        assert res_a[0] == res_b[0]
        for x, y in zip(res_a[1], res_b[1]):
            np.testing.assert_array_equal(x, y)
        for (counters, (f, c, k)) in (res_a, res_b):
            assert counters[1:] == (ora["sampled"], ora["valid"])
            assert len(f) == ora["nnz"]
            np.testing.assert_array_equal(c, ora["cell"].astype(np.int64))
            np.testing.assert_array_equal(f, ora["feature"].astype(np.int64))
            np.testing.assert_array_equal(k, ora["count"].astype(np.int64))

        monkeypatch.delenv("FASTF_NO_STREAM_K1B")
        c3 = make(); engines.append(c3)
        assert (c3.block_bytes(N), c3.probe_capacity(N)) == sizes
    finally:
        for e in engines:
            e.close()
