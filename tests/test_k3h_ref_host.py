"""tests/k3h_ref.py on the host: its rows against sortreduce_ref.want_rows for every fixture, the order-independence condition
that lets the reference alone decide, slot32 against a bit-by-bit restatement, the chain and partition builders, a census of what
each fixture reaches, and the reference mutants: every listed way of being wrong changes the expectation of a named fixture."""
import numpy as np
import pytest

import k3h_ref as K

LAYS = {"bases12": K.L12, "bases10": K.L10}


@pytest.fixture(scope="module")
def expected():
    return {(ln, name): K.expect(fx.keys, fx.max_n, lay) for ln, lay in LAYS.items() for name, fx in K.fixtures(lay).items()}


@pytest.mark.parametrize("ln", list(LAYS))
def test_rows_agree_with_the_window_free_reference_and_no_outcome_depends_on_order(expected, ln):
    lay = LAYS[ln]
    for name, fx in K.fixtures(lay).items():
        k = fx.keys
        grp = k >> np.uint64(lay.fs)
        assert (np.diff(grp.astype(np.int64)) >= 0).all(), name                     # groups contiguous and ascending
        rows, flagged, indep = expected[ln, name]
        f, c, cnt = K.rows_arrays(rows)
        wf, wc, wcnt = K.reference_rows(fx)
        np.testing.assert_array_equal(f, wf, err_msg=name)
        np.testing.assert_array_equal(c, wc, err_msg=name)
        np.testing.assert_array_equal(cnt, wcnt, err_msg=name)
        assert all(indep), name


def _slot32_bits(x, r):
    """slot32 once more, bit by bit: shift-and-add products kept to 24-bit operands and 32-bit results"""
    def bits(v, n):
        return [(v >> i) & 1 for i in range(n)]

    def mul24(a, b):
        acc = 0
        for i, bit in enumerate(bits(a, 24)):
            if bit:
                acc = (acc + (sum(bb << j for j, bb in enumerate(bits(b, 24))) << i)) % (1 << 32)
        return acc
    hi = sum(b << i for i, b in enumerate(bits(x, 32)[13:]))
    f = mul24(hi, 0x9E3779)
    g = mul24(r, 0x9E5)
    slot = sum((bits(x, 13)[i] ^ bits(f, 21)[8 + i] ^ bits(g, 13)[i]) << i for i in range(13))
    step = 1 | sum(bits(f, 26)[21 + i] << (1 + i) for i in range(5))
    word = hi + r * 32768 + 67108864
    return slot, step, word


def test_slot32_against_a_second_restatement():
    rng = np.random.default_rng(11)
    xs = rng.integers(0, 1 << 27, size=3000).tolist() + [0, 1, (1 << 27) - 1, 1 << 26, 1 << 13, (1 << 13) - 1]
    rs = rng.integers(0, 2048, size=len(xs)).tolist()
    rs[:4] = [0, 1, 2047, 1024]
    for x, r in zip(xs, rs):
        assert K.slot32(x, r) == _slot32_bits(x, r), (x, r)
    # worked by hand: hi = 1: f = 0x9E3779, slot = lo ^ (f >> 8 & 8191) = 5 ^ 0x1E37, step = (f >> 20 & 62) | 1 = 9
    assert K.slot32((1 << 13) | 5, 0) == (5 ^ 0x1E37, 9, 1 | (1 << 26))
    assert K.slot32((1 << 13) | 5, 3)[0] == 5 ^ 0x1E37 ^ (3 * 0x9E5 & 8191) and K.slot32((1 << 13) | 5, 3)[2] == 1 | (3 << 15) | (1 << 26)
    assert (1 << 14) - 1 < 1 << 15 and 2047 << 15 < 1 << 26 and 63 << 26 < 1 << 32          # hi, rank and probe number do not meet


def test_chain32_and_step_classes():
    sizes = sorted(len(v) for v in K.step_classes(K.L12).values())
    assert len(sizes) == 32 and sizes[0] == 253 and sizes[-1] == 258 and sum(sizes) == 8192
    sizes10 = sorted(len(v) for v in K.step_classes(K.L10).values())
    assert len(sizes10) == 32 and sizes10[0] == 14 and sizes10[-1] == 20 and sum(sizes10) == 512    # no chain of 63 exists with 10 bases
    for lay, m in ((K.L12, 200), (K.L12, 63), (K.L10, 20)):
        x = K.chain32(m, 1234, lay)
        assert len(set(x.tolist())) == m and all((int(v) >> lay.nn) == 1 for v in x)
        for r in (0, 1, 37, 2047):
            assert len({K.slot32(v, r)[:2] for v in x}) == 1
            assert K.slot32(x[0], r)[0] == 1234 ^ (r * 0x9E5 & 8191)
            assert len(set(K.chain_walk(int(x[0]), r))) == 63                        # the 63 slots of a walk are distinct
        assert len({K.slot32(v, 0)[2] for v in x}) == m                              # ... and the words of its members too
    a = K.hi_alias_pair(4000)
    assert len(a) == 2 and a[0] != a[1] and (a[0] >> 13) & 0xFF == (a[1] >> 13) & 0xFF and K.slot32(a[0], 5)[:2] == K.slot32(a[1], 5)[:2]


def test_one_partition_keys_and_giant_partition():
    g = K.L12.group(0)
    k = K.one_partition_keys(g, 3, 0, 4200)
    assert len(set(k.tolist())) == 4200
    assert sum(K.giant_partition(g | (1 << 26) | (u << 2) | 3, 3) == 0 for u in range(12_599)) == 4200        # UMIs 0 .. 12 598 scanned
    assert all(K.giant_partition(v, 3) == 0 and (int(v) >> 27) == g >> 27 and (int(v) >> 26) & 1 for v in k)
    k1 = K.one_partition_keys(g, 3, 2, 50)
    assert all(K.giant_partition(v, 3) == 2 for v in k1)
    # the 64-bit multiply by hand: key 1, 3 partitions: hh = 0x9E3779B97F4A7C15, (0x9E3779B9 * 3) >> 32 = 1
    assert K.giant_partition(1, 3) == 1 and K.giant_partition(0, 7) == 0
    assert sorted({K.giant_partition(v, 43) for v in range(1, 5000)}) == list(range(43))


def _census(fx):
    wins, how, empty, lims = K.geometry(fx.keys, fx.max_n, fx.lay, detail=True)
    copy0 = set()
    for (b, base, cut, giant, ln, parts) in wins:
        if not giant:
            L = K.Lanes(fx.keys, base, cut, fx.lay)
            copy0 |= {int(p) // 64 for p in np.flatnonzero(L.same & (L.pos < cut)) if p % 64 == 0}
    return (len(fx.keys), len(wins), how.count("giant"), how.count("stop"), how.count("last"), how.count("end"), tuple(empty), tuple(sorted(copy0)))


# name: (keys, windows, giant windows, cuts that are stops at the nominal end, cuts at the last head, cuts at the end of the
#        data, chunks without rows, units with a copy of the neighbour in front at lane 0)
CENSUS = {
    "copies_at_lane0": (2048, 1, 0, 0, 0, 1, (), (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 13, 16, 20, 24, 28)),
    "copies_key0_first": (2048, 1, 0, 0, 0, 1, (), (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 13, 16, 20, 24, 28)),
    "singles_2048": (2048, 1, 0, 0, 0, 1, (), ()),
    "singles_unit_edges": (2048, 1, 0, 0, 0, 1, (), ()),
    "single_then_equal_pair": (2048, 1, 0, 0, 0, 1, (), (8, 25)),
    "counts_across_units": (2048, 1, 0, 0, 0, 1, (), ()),
    "one_then_2046": (2092, 3, 0, 1, 1, 1, (), ()),
    "set_words": (148, 1, 0, 0, 0, 1, (), ()),
    "set_words_twice": (1262, 1, 0, 0, 0, 1, (), ()),
    "twin2": (2200, 2, 0, 0, 1, 1, (1,), ()),
    "twin3": (6600, 6, 0, 2, 3, 1, (3,), ()),
    "twins_after_giant": (8496, 5, 1, 1, 2, 1, (1, 4), ()),
    "twins_after_flag": (2200, 2, 0, 0, 1, 1, (1,), ()),
    "last_head_at_2047": (2082, 3, 0, 1, 1, 1, (), ()),
    "last_head_at_1": (2065, 3, 1, 0, 1, 1, (), ()),
    "group_2048_then_more": (2055, 2, 1, 0, 0, 1, (), ()),
    "group_2048_ends_data": (2053, 2, 0, 0, 1, 1, (1,), ()),
    "group_2048_alone": (2048, 1, 0, 0, 0, 1, (), ()),
    "groups_2047_2049": (4103, 4, 1, 1, 1, 1, (), ()),
    "heads_around_nominal_ends": (9692, 7, 0, 4, 2, 1, (), (17, 24)),
    "chunk_inside_a_giant": (10000, 5, 1, 2, 1, 1, (1,), ()),
    "first_head_511_512_513_in": (7857, 7, 0, 3, 3, 1, (), ()),
    "giant_ends_at_nominal_end": (5096, 3, 1, 0, 1, 1, (1,), ()),
    "giant_ends_beyond_nominal_end": (5200, 3, 1, 0, 1, 1, (1,), ()),
    "bound_seven_times": (3000, 3, 0, 1, 1, 1, (0, 1, 2, 3, 4, 6, 7, 8, 9), ()),
    "giant_nulls": (3014, 2, 1, 0, 0, 1, (), ()),
    "giant_round_boundary_dups": (5006, 2, 1, 0, 0, 1, (1,), ()),
    "giant_partition_4096": (4203, 2, 1, 0, 0, 1, (1,), ()),
    "giant_partition_4097": (4203, 2, 1, 0, 0, 1, (1,), ()),
    "giant_65536": (65539, 2, 1, 0, 0, 1, tuple(range(1, 32)), ()),
    "giant_65537": (65540, 2, 1, 0, 0, 1, tuple(range(1, 32)), ()),
    "chain62_rank0": (254, 1, 0, 0, 0, 1, (), ()),
    "chain62_rank37": (587, 1, 0, 0, 0, 1, (), ()),
    "chain63_rank0": (255, 1, 0, 0, 0, 1, (), ()),
    "chain63_rank37": (588, 1, 0, 0, 0, 1, (), ()),
    "chain64_rank0": (256, 1, 0, 0, 0, 1, (), ()),
    "chain64_rank37": (589, 1, 0, 0, 0, 1, (), ()),
    "chain200_rank0": (392, 1, 0, 0, 0, 1, (), ()),
    "chain200_rank37": (725, 1, 0, 0, 0, 1, (), ()),
    "two_chains": (212, 1, 0, 0, 0, 1, (), ()),
    "walk_over_same_hi": (10240, 9, 0, 4, 4, 1, (), (1, 2, 3, 4, 5, 6, 7, 8, 9)),
}


def test_fixture_census():
    F = K.fixtures(K.L12)
    assert set(F) == set(CENSUS)
    for name, fx in F.items():
        assert _census(fx) == CENSUS[name], name
    assert {fx.family for fx in F.values()} == {"neighbour copies", "single heads", "counts across units", "set words", "twin windows", "cuts",
                                                "giant groups", "chains"}
    # what the names promise
    wins, how, empty, lims = K.geometry(F["heads_around_nominal_ends"].keys, 5 * K.TILE, detail=True)
    assert [w[1] + w[2] for w, h in zip(wins, how) if h == "stop"] == [2048, 4147, 6145, 8192]        # at, after (4095 is before), after, at
    assert K.TILE in lims and any(0 < v < K.TILE for v in lims)                                       # the nominal end inside a window: lim = 2048 and below
    wins = K.geometry(F["first_head_511_512_513_in"].keys, F["first_head_511_512_513_in"].max_n)
    assert {2048 + 511, 4096 + 512, 6144 + 513} <= {w[1] for w in wins}
    assert [w[3:] for w in K.geometry(F["group_2048_then_more"].keys, 2055)][0] == (True, 2048, 2)
    assert [w[4] for w in K.geometry(F["giant_65536"].keys, 65_539) if w[3]] == [65_536]
    assert [w[4] for w in K.geometry(F["giant_65537"].keys, 65_540) if w[3]] == [65_537]
    assert [w[4] for w in K.geometry(F["giant_ends_at_nominal_end"].keys, 5096) if w[3]] == [3596]
    assert F["copies_key0_first"].keys[0] == 0
    L = K.Lanes(F["singles_2048"].keys, 0, 2048, K.L12)
    assert L.n_rows == 2048 and int(L.probe.sum()) == int((L.dist & (L.pos % 64 == 63)).sum()) > 20
    # the twin pairs: the window of one group repeats the key bits of the first window's rank-0 group
    for name, off in (("twin2", 0), ("twin3", 0), ("twin3", 4400), ("twins_after_giant", 4096), ("twins_after_flag", 0)):
        k = F[name].keys
        xm = np.uint64((1 << 27) - 1)
        differ = np.flatnonzero((k[off + 1500:off + 1800] & xm) != (k[off:off + 300] & xm))
        assert differ.tolist() == ([63] if name == "twins_after_flag" else [])      # (the 64th member of the chain is left out)
        assert (off, 1500, False, 0, 0) in [w[1:] for w in K.geometry(k, F[name].max_n)]
        assert (off + 1500, 700, False, 0, 0) in [w[1:] for w in K.geometry(k, F[name].max_n)]


def _mut(**kw):
    r = dict(K.RULES)
    r.update(kw)
    return r


# mutant: (what the reference does wrong, fixtures whose expectation it must change)
MUTANTS = {
    "hi kept to 8 bits in the word": (_mut(hi_mask=0xFF), ["set_words", "set_words_twice"]),
    "row rank left out of the word": (_mut(rank_in_word=False), ["set_words", "set_words_twice"]),
    "probe number left out of the word": (_mut(probe_in_word=False), ["walk_over_same_hi"]),
    "62 tries": (_mut(max_tries=62), ["chain63_rank0", "chain63_rank37", "two_chains"]),
    "64 tries": (_mut(max_tries=64), ["chain64_rank0", "chain64_rank37"]),
    "set not cleared between windows": (_mut(clear_set=False), ["twin2", "twin3", "twins_after_giant", "twins_after_flag"]),
    "copy shortcut applied across a head": (_mut(copy_across_head=True), ["single_then_equal_pair"]),
    "single shortcut at lane 63 with a non-head behind it": (_mut(single_at_lane63=True), ["counts_across_units"]),
    "cut at the first head beyond the nominal end": (_mut(stop_beyond=True), ["heads_around_nominal_ends"]),
    "giant-length limit one lower": (_mut(giant_max=K.GIANT_MAX - 1), ["giant_65536"]),
    "giant-length limit one higher": (_mut(giant_max=K.GIANT_MAX + 1), ["giant_65537"]),
    "partition from the low half of the product": (_mut(part_low_half=True), ["giant_partition_4097"]),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_reference_mutants_change_a_named_fixture(expected, mutant):
    rules, names = MUTANTS[mutant]
    F = K.fixtures(K.L12)
    for name in names:
        fx = F[name]
        rows, flagged, _ = K.expect(fx.keys, fx.max_n, K.L12, rules)
        good_rows, good_flag, _ = expected["bases12", name]
        assert (rows, flagged) != (good_rows, good_flag), (mutant, name)
