"""The helpers of tests/sortreduce_ref.py on the host: the chain builders against the restated hashes, the regions buffer, and a
census of the fixtures the GPU tests run, so that they cannot silently shrink."""
import numpy as np
import pytest

import sortreduce_ref as S


@pytest.mark.parametrize("rank", [0, 1, 2047])
def test_wide_chain_values_share_slot_and_step(rank):
    for umi_bits, len_bits in ((48, 3), (47, 4), (42, 2)):
        v = S.wide_chain_values(umi_bits, len_bits, 200, seed=5)
        assert len(set(v.tolist())) == 200
        assert all(int(x) >> (umi_bits + len_bits) == 1 for x in v)                 # non-NULL, nothing above the flag
        assert len({S.wide_slot_step(x, rank) for x in v}) == 1
        assert len({int(x) & 4095 for x in v}) == 1
    a, b = S.wide_chain_values(48, 3, 64, seed=1), S.wide_chain_values(48, 3, 64, seed=2)
    assert S.wide_slot_step(a[0], rank) != S.wide_slot_step(b[0], rank) or set(a.tolist()) != set(b.tolist())


@pytest.mark.parametrize("rank", [0, 1, 2047])
def test_slot64_chain_values_share_slot_and_step(rank):
    for feat_shift in (36, 33):
        v = S.slot64_chain_values(feat_shift, 200, seed=9, rank=rank)
        assert len(set(v.tolist())) == 200
        assert all(int(x) >> (feat_shift - 1) == 1 for x in v)
        assert len({S.slot64_slot_step(x, rank) for x in v}) == 1
    # the sum carries the rank: a chain built for one rank is none under another
    v = S.slot64_chain_values(36, 200, seed=9, rank=0)
    assert len({S.slot64_slot_step(x, 5) for x in v}) > 1


def test_restated_hashes_on_worked_values():
    # WIDE: x = flag | hi word 1 | low 12 bits 5: f = 0x9E3779B1 + 0x80 * 0x85EBCA77 mod 2^32
    x = (1 << 51) | (1 << 12) | 5
    f = (0x9E3779B1 + 0x80 * 0x85EBCA77) & 0xFFFFFFFF
    assert S.wide_slot_step(x, 0) == ((5 ^ (f >> 8)) & 4095, ((f >> 20) & 62) | 1)
    assert S.wide_slot_step(x, 3)[0] == (5 ^ (f >> 8) ^ (3 * 0x9E5)) & 4095
    hh = (7 * 0x9E3779B1 + 8 * 0x85EBCA77 + 2 * 0xC2B2AE3D) & 0xFFFFFFFF
    hh ^= hh >> 15
    assert S.slot64_slot_step((8 << 32) | 7, 2) == (hh & 4095, ((hh >> 20) & 62) | 1)


def test_regions_buffer_round_trips():
    rng = np.random.default_rng(3)
    for counts, stride in (([3, 0, 5, 5, 0], 5), ([1], 1), ([0, 0, 2], 7), (rng.integers(0, 9, size=300), 8)):
        counts = np.asarray(counts)
        keys = rng.integers(0, 1 << 40, size=int(counts.sum()), dtype=np.uint64)
        buf = S.regions_buffer(counts, stride, keys)
        assert len(buf) == len(counts) * stride
        np.testing.assert_array_equal(S.regions_logical(buf, counts, stride), keys)
        assert int((buf == S.POISON).sum()) == len(buf) - len(keys)
        for r, c in enumerate(counts):                                              # row r: its keys at the front, poison behind
            assert (buf[r * stride + c:(r + 1) * stride] == S.POISON).all()
            assert (buf[r * stride:r * stride + c] != S.POISON).all()
    with pytest.raises(AssertionError):
        S.regions_buffer([4], 3, np.zeros(4, np.uint64))


# name: (keys, regions, empty regions, tiles that cross more than two regions, regions that end on a tile edge)
REGION_CENSUS = {
    "one_short": (5000, 1, 0, 0, 0),
    "one_full": (4096, 1, 0, 0, 1),
    "dist8": (118845, 8, 0, 0, 0),
    "full8": (24000, 8, 0, 0, 0),
    "empties_first_last_run5": (2900, 11, 8, 0, 0),
    "all_empty_but_one": (2000, 16, 15, 0, 0),
    "all_empty": (0, 6, 6, 0, 0),
    "many_small": (10005, 5000, 0, 20, 7),
    "many_small_every_other_empty": (5008, 5000, 2500, 10, 5),
    "scan_carry_1023": (7161, 1023, 0, 14, 1),
    "scan_carry_1024": (7168, 1024, 0, 14, 2),
    "scan_carry_1025": (7175, 1025, 0, 14, 2),
    "scan_carry_2049": (14343, 2049, 0, 28, 4),
    "prefix_edges": (4909, 9, 0, 0, 4),
    "prefix_edges_ipt7": (4909, 9, 0, 2, 1),
    "prefix_edges_ipt8": (4909, 9, 0, 1, 1),
    "tail_three_empty_head": (1500, 5, 3, 0, 0),
    "loose_stride": (13929, 8, 0, 0, 0),
}


def test_region_fixture_census():
    assert set(S.REGION_CASES) == set(REGION_CENSUS)
    for name, c in S.REGION_CASES.items():
        tile = S.SORT_THREADS * (c["ipt"] or 1)
        assert (int(c["counts"].sum()),) + S.region_census(c["counts"], tile) == REGION_CENSUS[name], name
        assert c["counts"].max() <= c["stride"]
    C = S.REGION_CASES
    assert C["one_full"]["counts"][0] == C["one_full"]["stride"] and (C["full8"]["counts"] == C["full8"]["stride"]).all()
    assert C["loose_stride"]["stride"] == 8 * C["loose_stride"]["counts"].max()
    e = C["empties_first_last_run5"]["counts"]
    assert e[0] == 0 and e[-1] == 0 and (e[3:8] == 0).all() and e[2] and e[8]
    ends = set(np.cumsum(C["prefix_edges"]["counts"]).tolist())
    assert {512, 1023, 1025, 1536, 2559, 3584, 4096, 4609} <= ends
    t = C["tail_three_empty_head"]["counts"]                        # tile 1 = keys 512..1023: the tail of region 0, three empty, region 4
    assert 512 < t[0] < 1024 and (t[1:4] == 0).all() and t[0] + t[4] > 1024
    assert sum(1 for c in C.values() if c["reduce"]) == 2


# name: (keys, rows, runs of 2047, of 2048, of 2049, runs longer than a window)
UMI_CENSUS = {
    "one_key": (1, 1, 0, 0, 0, 0),
    "singles": (70_000, 70_000, 0, 0, 0, 0),
    "window_edges": (122_940, 120, 20, 20, 20, 20),
    "window_at_key_zero": (5048, 3001, 0, 1, 0, 0),
    "long_and_short": (16_101, 6, 0, 0, 0, 3),
    "one_long_run": (300_000, 1, 0, 0, 0, 1),
    "one_then_2047": (122_880, 120, 60, 0, 0, 0),
}


def test_umi_run_fixture_census():
    assert set(S.UMI_RUN_CASES) == set(UMI_CENSUS)
    for name, runs in S.UMI_RUN_CASES.items():
        k = S.run_keys(name)
        assert (np.diff(k.astype(np.int64)) >= 0).all() and k.max() < S.POISON
        u, c = S.umi_rows_ref(k)
        assert c.tolist() == list(runs), name
        assert (len(k), len(u)) + tuple(int((c == L).sum()) for L in (2047, 2048, 2049)) + (int((c > S.K3_TILE).sum()),) == UMI_CENSUS[name], name
    assert S.run_keys("window_at_key_zero")[0] == 0
    k = S.null_run_keys()
    u, c = S.umi_rows_ref(k)
    nulls = ((u >> np.uint64(26)) & np.uint64(1)) == 0
    assert c[nulls].tolist() == [1, 3, 2048, 2500, 2] and len(u) == 25 and len(k) == 14_809


def test_wide_reference_on_a_worked_example():
    lay = S.WideLayout(24)
    assert (lay.umi_bits, lay.len_bits, lay.nn_shift) == (48, 3, 51)
    g1, g2 = (3 << 9) | 4, (3 << 9) | 5
    a, b = int(lay.value(0xABCD_1234_5678)), int(lay.value(0xABCD_1234_5679))
    k = np.array([g2, g1, g1, g1, g2, g1, g2], np.uint64)
    v = np.array([a, b, a, b, 0, 0, 0], np.uint64)
    (f, c, n), (uf, uc, ncopy, umi, nn) = S.wide_rows_ref(k, v, lay)
    assert f.tolist() == [4, 5] and c.tolist() == [3, 3] and n.tolist() == [2, 1]
    assert uf.tolist() == [4, 4, 4, 5, 5] and uc.tolist() == [3] * 5
    assert ncopy.tolist() == [1, 1, 2, 2, 1] and nn.tolist() == [0, 1, 1, 0, 1]
    assert umi.tolist() == [0, 0xABCD_1234, 0xABCD_1234, 0, 0xABCD_1234]                # the first 16 of 24 bases
    lay12, lay32 = S.WideLayout(12), S.WideLayout(32)
    assert (lay12.umi_bits, lay12.len_bits, lay12.nn_shift) == (24, 2, 26)
    assert (lay32.sub_bits, lay32.umi_bits, lay32.len_bits, lay32.nn_shift) == (17, 47, 4, 51)
    # beyond 24 bases the sorted word carries the first 17 bits of the bases: two sub-groups of one (cell, feature) are one matrix row
    k = np.array([(g1 << 17) | 1, (g1 << 17) | 2, (g1 << 17) | 1, g1 << 17], np.uint64)
    v = np.array([int(lay32.value(9)), int(lay32.value(9)), int(lay32.value(9)), 0], np.uint64)
    (f, c, n), (uf, uc, ncopy, umi, nn) = S.wide_rows_ref(k, v, lay32)
    assert f.tolist() == [4] and c.tolist() == [3] and n.tolist() == [2]
    assert ncopy.tolist() == [1, 2, 1] and nn.tolist() == [0, 1, 1]
    assert umi.tolist() == [0, (1 << 47 | 9) >> 32, (2 << 47 | 9) >> 32]


def test_wide_special_pairs_census():
    for bases in (12, 24, 32):
        lay = S.WideLayout(bases)
        k, v = S.wide_special_pairs(lay)
        _, (uf, uc, ncopy, umi, nn) = S.wide_rows_ref(k, v, lay)
        c = ncopy.tolist()
        assert len(k) == 20_258 and len(c) == 15
        assert c.count(2047) == 1 and c.count(2048) == 2 and c.count(2049) == 2 and c.count(10_000) == 1
        assert int((nn == 0).sum()) == 4                                             # NULL pairs are rows too
