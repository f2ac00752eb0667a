"""tests/k1b_ref.py on the CPU: the reference reproduces the oracle's counters and matrix on two small cases (so the contract it
states is the reference program's), the fixtures of tests/test_gpu_k1b_gating.py hold the shapes they are there for, and every
wrong placement rule (k1b_ref.DEFECTS) changes the expected output of some fixture: the device tests would fail for these bugs."""
import numpy as np
import pytest

import fastf_amd as F
from fastf_amd.dist import owner_of_cell
from helpers import Case
from oracle import oracle as O
import k1b_ref as K
import lookup_ref as R
from sortreduce_ref import want_rows


@pytest.mark.parametrize("G", [1, 4])
def test_reference_agrees_with_the_oracle(G):
    case = Case(n=6000 + G, n_bar=300, n_gene=200, rate_depth=0.5, data_seed=10 + G, p_no_cb=0.05, p_unlisted_cb=0.1, p_bad_xf=0.1,
                p_n_umi=0.05, p_no_ub=0.05, umi_pool=2000)
    ora = case.oracle()
    lists = case.lists()
    cbk, gxk, umi, meta = case.packed(lists)
    cell, feat = R.cell_index(lists.cell_keys, cbk), R.gene_lookup(lists.feature_keys, gxk)
    hits = int((cell > 0).sum())
    assert 0 < hits < case.n and ((meta & K.XF_OK) == 0).any() and ((meta & K.HAS_UB) == 0).any() and ((meta & K.UMI_NONNULL) == 0).any()
    bits = (O.mt_stream(case.seed, hits, skip=lists.mt_skip).astype(np.uint64) < np.uint64(F.draw_threshold(case.rate_depth))).astype(np.uint8)
    L = K.Layout(K.bits_for(lists.n_cells), K.bits_for(lists.n_features), 12)
    res = K.k1b(cell, feat, umi, meta, bits, 0, hits, L, n_shards=G)
    assert res.err == 0
    assert res.counters == (hits, ora["sampled"], ora["valid"]) and ora["total"] == case.n      # (the oracle's total counts every read)
    assert 0 < ora["valid"] < ora["sampled"] < hits
    for s in range(G):
        if G > 1:
            assert (owner_of_cell((res.keys[s] >> np.uint64(L.cs)).astype(np.int64), G) == s).all()
    f, c, k = want_rows(np.concatenate(res.keys), fs=L.fs, cs=L.cs, feat_bits=L.feature_bits)
    np.testing.assert_array_equal(f, ora["feature"].astype(np.int64))
    np.testing.assert_array_equal(c, ora["cell"].astype(np.int64))
    np.testing.assert_array_equal(k, ora["count"].astype(np.int64))
    # the same decisions found unit by unit, and at a rank base inside a longer stream
    keep, short = K.plain_decisions(cell > 0, bits, 0, hits)
    k2, s2 = K.place_units(cell > 0, bits, 0, hits)
    assert (keep == k2).all() and not short.any() and not s2.any()
    longer = np.concatenate([np.ones(37, np.uint8), bits])
    assert K.k1b(cell, feat, umi, meta, longer, 37, 37 + hits, L, n_shards=G).counters == res.counters


def _records():
    n_cells = 1000
    gx, umi, meta, ext, cell_if_hit = K.build_records(n_cells, np.arange(1, 5010, dtype=np.uint64), np.array([0, 7000], np.uint64))
    feat = np.where(gx < 5010, gx, 0).astype(np.int64)               # (here a listed key IS its feature index)
    return gx, umi, meta, cell_if_hit, feat


def _expected(fx, rec, L, defect=None):
    gx, umi, meta, cell_if_hit, feat = rec
    mask = fx.mask()
    cell = np.where(mask, cell_if_hit[:fx.n], 0)
    return K.k1b(cell, feat[:fx.n], umi[:fx.n], meta[:fx.n], fx.stream(), fx.base, fx.n_draws(), L, defect=defect)


def _same(a, b):
    return a.counters == b.counters and a.err == b.err and len(a.keys[0]) == len(b.keys[0]) and (a.keys[0] == b.keys[0]).all()


def test_unit_placement_agrees_with_the_plain_rule_on_every_fixture():
    for fx in K.fixtures():
        mask, bits = fx.mask(), fx.stream()
        a, b = K.plain_decisions(mask, bits, fx.base, fx.n_draws()), K.place_units(mask, bits, fx.base, fx.n_draws())
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and not a[1].any(), fx.name


def test_fixture_census():
    fxs = K.fixtures()
    assert len({f.name for f in fxs}) == len(fxs)
    assert {f.n for f in fxs} == set(K.LENGTHS) and {f.hits for f in fxs} == set(K.HIT_PATTERNS)
    assert {f.bits for f in fxs} == set(K.BIT_PATTERNS) and {f.base for f in fxs} == set(K.BASES)
    seen = set()
    rec = _records()
    gx, umi, meta, cell_if_hit, feat = rec
    for fx in fxs:
        mask, bits, nd = fx.mask(), fx.stream(), fx.n_draws()
        seen.add("stream % 64 == 0" if nd % 64 == 0 and nd else "stream % 64 != 0")
        units = (fx.n + K.UNIT - 1) // K.UNIT
        per = np.array([int(mask[u * K.UNIT:(u + 1) * K.UNIT].sum()) for u in range(units)])
        rank0 = fx.base + np.concatenate([[0], np.cumsum(per)[:-1]])
        for u in range(units):
            if per[u] == K.UNIT and rank0[u] & 31 in (1, 31): seen.add("full unit at bit %d" % (rank0[u] & 31))
            if per[u] == K.UNIT and (rank0[u] & 31) + K.UNIT > 256: seen.add("ninth word")
            if per[u] == 0 and 0 < u < units - 1 and per[u - 1] == K.UNIT and per[u + 1] == K.UNIT: seen.add("empty unit between full ones")
            if per[u] == 1 and mask[u * K.UNIT]: seen.add("one hit at lane 0")
            if per[u] == 1 and u * K.UNIT + 255 < fx.n and mask[u * K.UNIT + 255]: seen.add("one hit at lane 255")
            if per[u] and nd and rank0[u] >> 5 == (nd - 1) >> 5: seen.add("rank0 in the last word")
            if per[u] and u % 16 and per[u // 16 * 16:u].sum() == 0: seen.add("earlier units of the tile hold 0 hits")
            if per[u] and u % 16 and (per[u // 16 * 16:u] == K.UNIT).all(): seen.add("earlier units of the tile hold 256 hits")
        tiles = (fx.n + K.TILE - 1) // K.TILE
        pt = [int(mask[t * K.TILE:(t + 1) * K.TILE].sum()) for t in range(tiles)]
        if any(pt[t] == 0 and pt[t + 1] > 0 for t in range(tiles - 1)): seen.add("empty tile in front of a tile with hits")
        if fx.base % 32: seen.add("draw_base % 32 != 0")
        # the drop reasons, on hits
        keep, _ = K.plain_decisions(mask, bits, fx.base, nd)
        m = meta[:fx.n].astype(np.int64)
        ok = lambda bit: (m & bit) != 0
        good = mask & ok(K.XF_OK) & ok(K.HAS_UB) & (feat[:fx.n] > 0)
        if (good & ~keep).any(): seen.add("dropped: no bit")
        if (mask & keep & ~ok(K.XF_OK)).any(): seen.add("dropped: bad xf")
        if (mask & keep & ok(K.XF_OK) & (feat[:fx.n] == 0)).any(): seen.add("dropped: no feature")
        if (mask & keep & ok(K.XF_OK) & (feat[:fx.n] > 0) & ~ok(K.HAS_UB)).any(): seen.add("dropped: no UB")
        if (mask & ok(K.UMI_TOOLONG) & ~good).any(): seen.add("too long on a dropped record")
        if (good & keep & ~ok(K.UMI_NONNULL)).any(): seen.add("NULL UMI kept")
        assert not (good & ok(K.UMI_TOOLONG)).any()                  # (bit 4 stays down in the fixtures: test_gpu_k1b_gating raises it on its own)
    want = {"stream % 64 == 0", "stream % 64 != 0", "full unit at bit 1", "full unit at bit 31", "ninth word", "empty unit between full ones",
            "one hit at lane 0", "one hit at lane 255", "rank0 in the last word", "earlier units of the tile hold 0 hits",
            "earlier units of the tile hold 256 hits", "empty tile in front of a tile with hits", "draw_base % 32 != 0", "dropped: no bit",
            "dropped: bad xf", "dropped: no feature", "dropped: no UB", "too long on a dropped record", "NULL UMI kept"}
    assert want <= seen, sorted(want - seen)
    # a too-long UMI on a kept record: the error-path streams of the device test (one record, its bit set and clear)
    L = K.Layout(10, 13, 12)
    one = np.array([K.XF_OK | K.HAS_UB | K.UMI_NONNULL | K.UMI_TOOLONG | 3 << 4])
    for bit, err in ((1, K.ERR_UMI_TOOLONG), (0, 0)):
        r = K.k1b([5], [9], np.array([256], np.uint32), one, [bit], 0, 1, L)
        assert (r.err, r.counters) == (err, (1, bit, bit))
    assert K.too_long(L, np.array([255, 256], np.uint32), np.array([one[0] & ~K.UMI_TOOLONG] * 2)).tolist() == [True, False]
    assert K.too_long(L, np.array([256], np.uint32), np.array([K.UMI_NONNULL | 4 << 4])).tolist() == [True]


def test_each_wrong_rule_changes_some_fixture():
    rec = _records()
    L = K.Layout(10, 13, 12)
    fxs = K.fixtures()
    good = {fx.name: _expected(fx, rec, L) for fx in fxs}
    assert all(r.err == 0 for r in good.values())
    for defect in K.DEFECTS:
        caught = [fx.name for fx in fxs if not _same(good[fx.name], _expected(fx, rec, L, defect))]
        assert caught, "no fixture notices the defect %s" % defect
        print("%s: caught by %d fixtures, first %s" % (defect, len(caught), ", ".join(caught[:4])))


def test_error_bits_of_the_reference():
    rec = _records()
    gx, umi, meta, cell_if_hit, feat = rec
    L = K.Layout(10, 13, 12)
    fx = K.Fixture(4097, "all", "random", 33)
    full = _expected(fx, rec, L)
    short = K.k1b(cell_if_hit[:fx.n], feat[:fx.n], umi[:fx.n], meta[:fx.n], fx.stream()[:-1], fx.base, fx.n_draws() - 1, L)
    assert short.err == K.ERR_DRAWS_SHORT and short.counters[0] == full.counters[0] and short.counters[1] in (full.counters[1], full.counters[1] - 1)
    n_keys = len(full.keys[0])
    assert K.k1b(cell_if_hit[:fx.n], feat[:fx.n], umi[:fx.n], meta[:fx.n], fx.stream(), fx.base, fx.n_draws(), L, shard_stride=n_keys - 1).err == K.ERR_KEYS_FULL
    assert K.k1b(cell_if_hit[:fx.n], feat[:fx.n], umi[:fx.n], meta[:fx.n], fx.stream(), fx.base, fx.n_draws(), L, shard_stride=n_keys).err == 0
    r8 = K.k1b(cell_if_hit[:fx.n], feat[:fx.n], umi[:fx.n], meta[:fx.n], fx.stream(), fx.base, fx.n_draws(), L, n_shards=8)
    assert sum(len(k) for k in r8.keys) == n_keys and np.array_equal(np.sort(np.concatenate(r8.keys)), full.keys[0])
