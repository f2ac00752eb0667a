"""Narrow blocked runs (gx32 | um32 | cell scratch, 10 or 12 bytes per record) against the wide ones (18 or 20 bytes):
both layouts bit for bit against the oracle, through the device-level calls and through fastf_engine_push; the lists that
must keep the wide runs; records the narrowing maps to "cannot match"; a UMI the engine cannot hold."""
import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import hostmem, synth
from helpers import Case, assert_matches_oracle
from test_gpu_parity import CASES

pytestmark = pytest.mark.gpu

NARROW_RUNS, WIDE_RUNS = (2560, 3072), (4608, 5120)


def run_bytes(eng):
    """bytes of one 256-record unit of the engine's blocked layout (0: no blocked layout)"""
    return eng.block_bytes(256)


def device_pass(eng, case, lists, recs=None):
    """the blocked resident pass (fastf_dev_block_records -> K1a -> K1b -> sort -> reduce), two steps; (coo, counters)"""
    import torch
    from fastf_amd.dist import HipStages, ShardedPass
    dev = torch.device("cuda", 0)
    cbk, gxk, umi, meta = recs if recs is not None else case.packed(lists)
    d = [hostmem.to_device(x, dev) for x in (cbk, gxk, umi, meta)]
    draws = hostmem.to_device(F.mt_draws(case.seed, lists.mt_skip, case.n), dev)
    st = HipStages(eng, dev)
    sp = ShardedPass(st, case.n, dev)
    blk = st.block(d[1], d[2], d[3], case.n)
    assert blk is not None
    for dr in (draws, sp.prepare_draws(draws)):
        sp.run(d[0], blk, None, None, case.n, dr)
    return sp.local_coo(), sp.global_counters()


def assert_coo(coo, counters, ora):
    f, c, k = coo
    hits, sampled, valid, err = counters
    assert err == 0
    assert (sampled, valid) == (ora["sampled"], ora["valid"])
    np.testing.assert_array_equal(c, ora["cell"].astype(np.int64))
    np.testing.assert_array_equal(f, ora["feature"].astype(np.int64))
    np.testing.assert_array_equal(k, ora["count"].astype(np.int64))


@pytest.fixture(params=["narrow", "wide"])
def layout(request, monkeypatch):
    if request.param == "wide":
        monkeypatch.setenv("FASTF_BLOCK_WIDE", "1")
    else:
        monkeypatch.delenv("FASTF_BLOCK_WIDE", raising=False)
    return request.param


@pytest.mark.parametrize("name", list(CASES))
def test_cases_in_both_layouts_match_oracle(name, layout):
    case = Case(**CASES[name])
    ora = case.oracle()
    lists = case.lists()
    eng = F.Engine.from_lists(lists, rate_depth=case.rate_depth, seed=case.seed, umi_max_bases=12)
    try:
        rb = run_bytes(eng)
        if rb == 0:                                      # gene list not in LDS: no blocked layout, nothing narrow
            assert "LDS" not in eng.table_modes.split("genes:")[1]
        else:
            assert rb in (NARROW_RUNS if layout == "narrow" else WIDE_RUNS)
            coo, counters = device_pass(eng, case, lists)
            assert_coo(coo, counters, ora)
        eng.push(*case.packed(lists))
        assert_matches_oracle(eng.finish(), ora, eng, case, lists, eng.umi_rows())
    finally:
        eng.close()


def test_records_the_narrowing_maps_to_no_match(layout):
    """gx key 0 (no GX tag), a key of another family, family keys whose number is 2^32 - 1, 2^32 or more: counters and rows
    as the oracle has them"""
    case = Case(n=60_000, n_bar=300, n_gene=200, rate_depth=0.8, umi_pool=128, data_seed=3)
    rng = np.random.default_rng(4)
    odd = [b"", b"ENSMUSG00000000005", b"ENSG04294967295", b"ENSG04294967296", b"ENSG04294967297", b"ENSG99999999999",
           b"ENSG00000000000"]
    gx = case.gx.astype("S%d" % max(case.gx.dtype.itemsize, 20))
    pick = rng.random(case.n) < 0.3
    gx[pick] = np.array(odd, dtype=gx.dtype)[rng.integers(0, len(odd), int(pick.sum()))]
    case.gx = gx
    ora = case.oracle()
    assert ora["valid"] > 1000
    lists = case.lists()
    recs = case.packed(lists)
    fam = int(recs[1][~pick][0]) >> 44
    keys = recs[1][pick].astype(np.uint64)
    assert (keys == 0).any() and ((keys >> np.uint64(44)) != fam).any()
    assert (((keys >> np.uint64(44)) == fam) & ((keys & np.uint64(0xFFFFFFFFFFF)) >= np.uint64(0xFFFFFFFF))).any()
    eng = F.Engine.from_lists(lists, rate_depth=case.rate_depth, seed=case.seed, umi_max_bases=12)
    try:
        assert run_bytes(eng) in (NARROW_RUNS if layout == "narrow" else WIDE_RUNS)
        coo, counters = device_pass(eng, case, lists, recs)
        assert_coo(coo, counters, ora)
        assert counters[0] == ora["total"]
        eng.push(*recs)
        assert_matches_oracle(eng.finish(), ora, eng, case, lists, eng.umi_rows())
    finally:
        eng.close()


def _one_long_umi(umi_len_of_one):
    bt, ft, bar, genes = synth.make_lists(10, 5, seed=5)
    flags, xf, cb, gx, ub = synth.make_records(5000, bar, genes, seed=6, umi_len=12)
    ub = ub.astype("S%d" % max(ub.dtype.itemsize, umi_len_of_one + 1))
    ub[2500] = b"ACGT" * (umi_len_of_one // 4) + b"ACGT"[:umi_len_of_one % 4]
    return bt, ft, flags, xf, synth.as_cstr(cb), synth.as_cstr(gx), synth.as_cstr(ub)


def test_a_13_base_umi_on_a_12_base_engine_raises_the_same_error_in_both_layouts(monkeypatch):
    bt, ft, flags, xf, cb, gx, ub = _one_long_umi(13)
    lists = F.Lists(bt, ft, 1.0, 926)
    recs = F.pack_records(lists, flags, xf, cb, gx, ub)
    msgs, errs = {}, {}
    for lay in ("narrow", "wide"):
        if lay == "wide":
            monkeypatch.setenv("FASTF_BLOCK_WIDE", "1")
        eng = F.Engine.from_lists(lists, umi_max_bases=12)
        try:
            assert run_bytes(eng) in (NARROW_RUNS if lay == "narrow" else WIDE_RUNS)
            case = Case(n=1, n_bar=2, n_gene=2)
            case.n, case.seed = len(flags), 926
            _, counters = device_pass(eng, case, lists, recs)
            errs[lay] = counters[3]
        finally:
            eng.close()
        eng = F.Engine.from_lists(lists, umi_max_bases=12)
        try:
            eng.push(*recs)
            with pytest.raises(F.FastfError) as ei:
                eng.finish()
            msgs[lay] = str(ei.value)
        finally:
            eng.close()
    assert errs["narrow"] == errs["wide"] != 0
    assert msgs["narrow"] == msgs["wide"]
    assert "umi_max_bases" in msgs["narrow"]


def test_lists_that_keep_the_wide_runs():
    # two gene families (the mixed-name list of test_gpu_parity: ENSG and ENSMUSG ids and escape-form names)
    bars = [b"%016d-1" % i for i in range(20)]
    genes = [b"ENSG%011d" % (1000 + 7 * i) for i in range(40)] + [b"ENSMUSG%011d" % (5 + 3 * i) for i in range(10)] + [b"GFP"]
    bt = b"".join(b + b"\n" for b in bars)
    ft = b"".join(g + b"\tname\tGene Expression\n" for g in genes)
    eng = F.Engine.from_lists(F.Lists(bt, ft, 1.0, 926), umi_max_bases=12)
    try:
        assert "LDS" in eng.table_modes.split("genes:")[1]
        assert run_bytes(eng) in WIDE_RUNS
    finally:
        eng.close()
    # the largest listed number 2^32 - 1 (narrow needs vmin + range <= 2^32 - 1), and one below that limit
    for start, want in ((4294967295 - 9, WIDE_RUNS), (4294967294 - 9, NARROW_RUNS)):
        bt, ft, _, _ = synth.make_lists(20, 10, seed=3, gene_start=start)
        eng = F.Engine.from_lists(F.Lists(bt, ft, 1.0, 926), umi_max_bases=12)
        try:
            assert run_bytes(eng) in want, start
        finally:
            eng.close()
    # 13..16 UMI bases
    bt, ft, _, _ = synth.make_lists(20, 10, seed=3)
    for umax, want in ((12, NARROW_RUNS), (13, WIDE_RUNS), (16, WIDE_RUNS)):
        eng = F.Engine.from_lists(F.Lists(bt, ft, 1.0, 926), umi_max_bases=umax)
        try:
            assert run_bytes(eng) in want, umax
        finally:
            eng.close()


def test_gene_numbers_at_the_narrow_limit_match_oracle():
    """listed numbers up to 2^32 - 2 (gx32 = number + 1 up to 2^32 - 1), records that name 2^32 - 1 and 2^32 among them"""
    case = Case(n=40_000, n_bar=100, n_gene=30, gene_start=4294967294 - 29, umi_pool=64, rate_depth=0.9, data_seed=8)
    rng = np.random.default_rng(9)
    pick = rng.random(case.n) < 0.1
    odd = np.array([b"ENSG04294967295", b"ENSG04294967296"], dtype=case.gx.dtype)
    case.gx[pick] = odd[rng.integers(0, 2, int(pick.sum()))]
    ora = case.oracle()
    lists = case.lists()
    eng = F.Engine.from_lists(lists, rate_depth=case.rate_depth, seed=case.seed, umi_max_bases=12)
    try:
        assert run_bytes(eng) in NARROW_RUNS
        coo, counters = device_pass(eng, case, lists)
        assert_coo(coo, counters, ora)
        eng.push(*case.packed(lists))
        assert_matches_oracle(eng.finish(), ora, eng, case, lists, eng.umi_rows())
    finally:
        eng.close()


def test_32_bit_cell_scratch_in_the_narrow_layout(monkeypatch):
    monkeypatch.setenv("FASTF_CELL_SCRATCH_32", "1")
    case = Case(**CASES["mixed"])
    ora = case.oracle()
    lists = case.lists()
    eng = F.Engine.from_lists(lists, rate_depth=case.rate_depth, seed=case.seed, umi_max_bases=12)
    try:
        assert run_bytes(eng) == 3072
        coo, counters = device_pass(eng, case, lists)
        assert_coo(coo, counters, ora)
        eng.push(*case.packed(lists))
        assert_matches_oracle(eng.finish(), ora, eng, case, lists, eng.umi_rows())
    finally:
        eng.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 511, 4095, 4096, 4097, 12 * 256 - 1, 12 * 256, 12 * 256 + 1, 24 * 256 + 3,
                               16 * 4096 - 255, 16 * 4096 + 1])
def test_narrow_record_counts_around_unit_tile_and_round_sizes(n):
    case = Case(n=n, n_bar=64, n_gene=40, rate_depth=0.5, umi_pool=16, p_no_cb=0.0, p_unlisted_cb=0.0)
    ora = case.oracle()
    lists = case.lists()
    eng = F.Engine.from_lists(lists, rate_depth=case.rate_depth, seed=case.seed, umi_max_bases=12)
    try:
        assert run_bytes(eng) in NARROW_RUNS
        coo, counters = device_pass(eng, case, lists)
        assert_coo(coo, counters, ora)
    finally:
        eng.close()


@pytest.mark.parametrize("pinned", [False, True])
def test_multi_chunk_push_with_a_partial_last_unit(pinned):
    """chunks of 20 000 records (78 whole units and 32 records), pushes cut at odd places; from pageable and from pinned host
    memory"""
    case = Case(n=150_003, n_bar=800, n_gene=400, rate_depth=0.7, umi_pool=256, p_unlisted_cb=0.1, p_bad_xf=0.1)
    ora = case.oracle()
    lists = case.lists()
    eng = F.Engine.from_lists(lists, rate_depth=case.rate_depth, seed=case.seed, batch_records=20_000, umi_max_bases=12)
    try:
        assert run_bytes(eng) in NARROW_RUNS
        recs = case.packed(lists)
        pb = None
        if pinned:
            pb = F.PinnedBatch(case.n)
            pb.fill(0, *recs)
        cuts = [0, 1, 4097, 50_000, 50_001, 120_000, 150_003]
        for a, b in zip(cuts[:-1], cuts[1:]):
            if pinned:
                eng.push_pinned(pb, a, b)
            else:
                eng.push(*[x[a:b] for x in recs])
        assert_matches_oracle(eng.finish(), ora, eng, case, lists, eng.umi_rows())
    finally:
        eng.close()
        if pb is not None:
            pb.close()
