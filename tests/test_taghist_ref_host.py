"""tests/taghist_ref.py on the host: the references against a dict loop, a census of the fixtures the GPU tests run (so that
they cannot silently shrink), and a restatement of the device pipeline of csrc/tag_hist.hpp — fill, a stable LSD sort over the
masked digits only, run lengths, first index, fill correction — that equals the reference on every fixture and stops doing so
on some fixture when one of its rules is made wrong: the fixtures can see those faults."""
import numpy as np
import pytest

import taghist_ref as T

U = np.uint64


# ---------------------------------------------------------------- the references against a dict loop
def loop_single(keys):
    cnt, first = {}, {}
    for i, k in enumerate(keys.tolist()):
        if k:
            cnt[k] = cnt.get(k, 0) + 1
            first.setdefault(k, i)
    u = sorted(cnt)
    return u, [cnt[k] for k in u], [first[k] for k in u]


def loop_pairs(k1, k2):
    cnt, first, c1, f1 = {}, {}, {}, {}
    for i, (a, b) in enumerate(zip(k1.tolist(), k2.tolist())):
        if a:
            c1.setdefault(a, 0)
        if a and b:
            cnt[(a, b)] = cnt.get((a, b), 0) + 1
            first.setdefault((a, b), i)
            c1[a] += 1
            f1.setdefault(a, i)
    u1, up = sorted(c1), sorted(cnt)
    return dict(n_records=len(k1), n_valid=sum(cnt.values()), n_key1_present=sum(1 for a in k1.tolist() if a),
                key1=u1, count1=[c1[a] for a in u1], first1=[f1.get(a, T.NONE) for a in u1],
                pair_k1=[u1.index(a) for a, _ in up], pair_key2=[b for _, b in up], pair_count=[cnt[p] for p in up],
                pair_first=[first[p] for p in up])


def same_pairs(got, want):
    assert set(got) == set(want)
    for k in want:
        if isinstance(want[k], int):
            assert got[k] == want[k], k
        else:
            assert np.asarray(got[k]).tolist() == list(want[k]), k


def test_want_single_equals_the_dict_loop():
    rng = np.random.default_rng(1)
    cases = [np.zeros(0, U), np.zeros(5, U), np.array([7], U), np.array([0, (1 << 64) - 1, 1, 0, 1], U)]
    for pool, n, p in ((1, 50, 0.3), (7, 300, 0.1), (200, 1000, 0.0), (1000, 500, 0.5)):
        k = rng.integers(1, 1 << 64, pool, dtype=U, endpoint=False)[rng.integers(0, pool, n)]
        k[rng.random(n) < p] = 0
        cases.append(k)
    cases += [T.SINGLE[name]["k1"] for name in T.SINGLE if len(T.SINGLE[name]["k1"]) < T.BIG]
    assert len(cases) == 8 + 20
    for k in cases:
        u, c, f = T.want_single(k)
        assert (u.dtype, c.dtype, f.dtype) == (U, U, U)
        assert (u.tolist(), c.tolist(), f.tolist()) == loop_single(k)


def test_want_pairs_equals_the_dict_loop():
    rng = np.random.default_rng(2)
    z = np.zeros(4, U)
    cases = [(np.zeros(0, U), np.zeros(0, U)), (z, z), (z + U(3), z), (z, z + U(3)), (np.array([5, 5, 0, 9], U), np.array([0, 2, 2, 0], U))]
    for p1, p2, n in ((1, 1, 20), (3, 40, 400), (60, 2, 400), (300, 300, 800)):
        a = rng.integers(1, 1 << 64, p1, dtype=U, endpoint=False)[rng.integers(0, p1, n)]
        b = rng.integers(1, 1 << 64, p2, dtype=U, endpoint=False)[rng.integers(0, p2, n)]
        a[rng.random(n) < 0.1] = 0
        b[rng.random(n) < 0.2] = 0
        cases.append((a, b))
    small = [name for name in T.PAIRS if len(T.PAIRS[name]["k1"]) < T.BIG]
    assert len(small) == 10
    cases += [(T.PAIRS[name]["k1"], T.PAIRS[name]["k2"]) for name in small]
    for a, b in cases:
        same_pairs(T.want_pairs(a, b), loop_pairs(a, b))


# ---------------------------------------------------------------- census
# name: (n, distinct keys, pass mask, count of the fill key, absent records)
SINGLE_CENSUS = {
    "mask_d0": (1537, 220, 0x01, 10, 77), "mask_d1": (1537, 220, 0x02, 5, 77), "mask_d2": (1537, 221, 0x04, 8, 77),
    "mask_d3": (1537, 221, 0x08, 8, 77), "mask_d4": (1537, 220, 0x10, 6, 77), "mask_d5": (1537, 220, 0x20, 7, 77),
    "mask_d6": (1537, 220, 0x40, 11, 77), "mask_d7": (1537, 221, 0x80, 9, 77),
    "mask_d07": (1537, 403, 0x81, 5, 77), "mask_d67": (1537, 404, 0xC0, 7, 77), "mask_d135": (1537, 404, 0x2A, 6, 77),
    "mask_d0246": (1537, 406, 0x55, 4, 77), "mask_all_but_3": (1537, 413, 0xF7, 3, 77), "mask_all": (1537, 415, 0xFF, 6, 77),
    "fill_once": (2901, 41, 0xFF, 1, 1500), "fill_hot": (4000, 31, 0xFF, 3600, 200),
    "one_present_first": (1000, 1, 0x00, 1, 999), "one_present_last": (1000, 1, 0x00, 1, 999),
    "first_edges": (769, 7, 0xFF, 375, 35), "extremes": (1347, 76, 0xFF, 17, 23), "runs": (10_049, 3002, 0x7F, 5000, 0),
    "grid_stride": (2_097_153, 3000, 0x23, 677, 105_727), "grows": (4_194_309, 50, 0x04, 81_486, 126_004),
}
# name: (n, m1, m2, pairs, mask of key1, of key2, of the code's low word, of its high word, count of the fill pair, records
#        that are no valid pair, key1 values with no valid pair)
PAIR_CENSUS = {
    "digits_m1_1": (2000, 1, 300, 300, 0x00, 0xFF, 0x03, 0x10, 9, 168, 0),
    "digits_m1_255": (2000, 255, 300, 1809, 0xFF, 0xFF, 0x03, 0x10, 1, 163, 0),
    "digits_m1_256": (2000, 256, 300, 1802, 0xFF, 0xFF, 0x03, 0x30, 1, 173, 0),
    "digits_m1_257": (2000, 257, 300, 1790, 0xFF, 0xFF, 0x03, 0x30, 1, 191, 0),
    "digits_m1_65535": (70_000, 65_535, 300, 69_508, 0xFF, 0xFF, 0x03, 0x30, 1, 480, 0),
    "digits_m1_65536": (70_000, 65_536, 300, 69_550, 0xFF, 0xFF, 0x03, 0x70, 1, 441, 0),
    "digits_m2_1": (2000, 300, 1, 300, 0xFF, 0x00, 0x01, 0x30, 5, 164, 0),
    "digits_m2_2": (2000, 300, 2, 565, 0xFF, 0xFF, 0x01, 0x30, 4, 163, 0),
    "digits_m2_256": (2000, 300, 256, 1825, 0xFF, 0xFF, 0x01, 0x30, 1, 157, 0),
    "digits_m2_257": (2000, 300, 257, 1813, 0xFF, 0xFF, 0x03, 0x30, 1, 166, 0),
    "digits_m2_65536": (70_000, 300, 65_536, 69_541, 0xFF, 0xFF, 0x03, 0x30, 1, 446, 0),
    "digits_m2_65537": (70_000, 300, 65_537, 69_538, 0xFF, 0xFF, 0x07, 0x30, 1, 445, 0),
    "dead_key1": (2000, 23, 60, 960, 0xFF, 0xFF, 0x01, 0x10, 3, 152, 3),
    "first_valid_late": (2200, 31, 41, 816, 0xFF, 0xFF, 0x01, 0x10, 1, 832, 0),
    "one_key1_300k": (300_100, 3, 300_000, 300_020, 0xA1, 0xFF, 0x07, 0x10, 1, 40, 0),
    "forty_key1": (320_000, 40, 74_458, 300_000, 0xFF, 0xFF, 0x07, 0x10, 2, 2000, 0),
    "pair_grid_stride": (2_097_153, 700, 900, 598_961, 0xFF, 0xFF, 0x03, 0x30, 1, 204_978, 0),
    "pair_grows": (4_194_309, 50, 60, 3000, 0x08, 0x40, 0x01, 0x10, 1292, 247_358, 0),
}


def test_single_fixture_census():
    assert list(T.SINGLE) == list(SINGLE_CENSUS)
    for name, f in T.SINGLE.items():
        c = T.census(f)
        assert (c["n"], c["m1"], c["mask"], c["fill_count"], c["absent"]) == SINGLE_CENSUS[name], name
    S = T.SINGLE
    for name, digits in T.MASKS.items():
        k = S["mask_" + name]["k1"]
        assert T.census(S["mask_" + name])["mask"] == sum(1 << q for q in digits)          # exactly the intended passes
        assert len(k) == 3 * T.SORT_TILE + 1 and k[-1] != 0                                # one key in the last tile
        p = k[k != 0]
        for q in range(8):
            d = np.unique((p >> U(8 * q)) & U(255))
            if q in digits:
                assert len(d) >= 200 and d[0] == 0x00 and d[-1] == 0xFF
            else:
                assert d.tolist() == [T.CONST_BYTES[q]] and T.CONST_BYTES[q] != 0
    assert len(set(T.CONST_BYTES)) == 8
    assert {bin(T.census(S["mask_" + m])["mask"]).count("1") % 2 for m in T.MASKS} == {0, 1}     # the result in either buffer
    k = S["fill_once"]["k1"]
    assert (k[:900] == 0).all() and k[900] != 0 and int((k == k[900]).sum()) == 1 and int((k[901:] == 0).sum()) == 600
    k = S["fill_hot"]["k1"]
    assert int((k == k[np.flatnonzero(k)[0]]).sum()) == len(k) * 9 // 10
    assert np.flatnonzero(S["one_present_first"]["k1"]).tolist() == [0] and np.flatnonzero(S["one_present_last"]["k1"]).tolist() == [999]
    f = S["first_edges"]
    u, c, first = T.want_single(f["k1"])
    assert len(f["k1"]) == 3 * 256 + 1 and sorted(first.tolist()) == [0, 3, 255, 256, 511, 512, 768]
    assert np.flatnonzero(f["k1"] == f["k1"][3]).tolist() == [3, 257, 513]               # one copy in every workgroup of 256 records
    k = S["extremes"]["k1"]
    have = set(k.tolist())
    assert {1, 2, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 2, (1 << 64) - 1} | {1 << b for b in range(64)} <= have
    for q in range(8):
        assert any(a ^ (1 << (8 * q)) in have and a != 1 << (8 * q) and a >> 8 for a in have if not a & (1 << (8 * q)) and bin(a).count("1") > 8)
    assert len(k) % T.SORT_TILE not in (0, 1) and k[-1] == U((1 << 64) - 1)
    k = S["runs"]["k1"]
    assert (np.diff(k.astype(np.float64)) >= 0).all()
    assert T.want_single(k)[1].tolist() == [5000] + [1] * 3000 + [2049]
    f = S["grid_stride"]
    k = f["k1"]
    assert len(k) == (1 << 21) + 1 and np.flatnonzero(k == U(f["last"])).tolist() == [len(k) - 1]
    at = np.flatnonzero(k == U(f["mid"]))
    assert at[0] == 1 << 20 and len(at) > 100
    assert len(S["grows"]["k1"]) == T.FIRST_ALLOC + 5 and S["grows"]["cuts"] == [1000]


def test_pair_fixture_census():
    assert list(T.PAIRS) == list(PAIR_CENSUS)
    P = T.PAIRS
    for name, f in P.items():
        c = T.census(f)
        assert (c["n"], c["m1"], c["m2"], c["pairs"], c["mask1"], c["mask2"], c["code_lo"], c["code_hi"], c["fill_count"], c["absent"],
                c["dead_key1"]) == PAIR_CENSUS[name], name
        if name.startswith("digits_"):
            w = T.want(name)
            m1, m2 = c["m1"], c["m2"]
            assert (w["count1"] > 0).all() and len(np.unique(w["pair_key2"])) == m2        # every rank occurs in a valid pair
            u2 = np.unique(f["k2"][f["k2"] != 0])
            assert (w["pair_k1"][0], w["pair_key2"][0]) == (0, u2[0]) and (w["pair_k1"][-1], w["pair_key2"][-1]) == (m1 - 1, u2[-1])
    hi = {m: T.code_masks(m, 300)[1] for m in T.DIGIT_EDGES_M1}
    lo = {m: T.code_masks(300, m)[0] for m in T.DIGIT_EDGES_M2}
    assert hi[1] == hi[255] == 0x10 and hi[256] == hi[257] == hi[65535] == 0x30 and hi[65536] == 0x70      # the passes differ across each edge
    assert lo[1] == lo[2] == lo[256] == 0x01 and lo[257] == lo[65536] == 0x03 and lo[65537] == 0x07
    f, w = P["dead_key1"], T.want("dead_key1")
    dead = w["key1"][w["count1"] == 0]
    assert dead.tolist() == f["dead"].tolist() and dead[0] == w["key1"][0] and dead[2] == w["key1"][-1]
    assert f["k1"][np.flatnonzero(f["k1"])[0]] == dead[1] and (w["first1"][w["count1"] == 0] == U(T.NONE)).all()
    f = P["first_valid_late"]
    valid = (f["k1"] != 0) & (f["k2"] != 0)
    assert not valid[:700].any() and valid[700] and (f["k1"][:700:2] != 0).all() and (f["k2"][1:700:2] != 0).all()
    w = T.want("one_key1_300k")
    assert np.bincount(w["pair_k1"]).tolist() == [10, 300_000, 10] and 300_000 >= 1 << 18
    w = T.want("forty_key1")
    per = np.bincount(w["pair_k1"])
    assert len(per) == 40 and per.min() == 1 and per.max() > 70_000 and per.sum() == 300_000
    for name, cut in (("pair_grid_stride", None), ("pair_grows", 1000)):
        assert len(P[name]["k1"]) > 1 << 21 and (cut is None or P[name]["cuts"] == [cut])
    assert len(P["pair_grows"]["k1"]) == T.FIRST_ALLOC + 5


# ---------------------------------------------------------------- the device pipeline, restated
def lsd_distinct(keys, fill_idx, mask):
    """th_distinct: absent keys take the key of record fill_idx, stable passes over the digits of `mask` only, run lengths"""
    a = np.where(keys == 0, keys[fill_idx], keys)
    for q in range(8):
        if (mask >> q) & 1:
            a = a[np.argsort(((a >> U(8 * q)) & U(255)).astype(np.uint8), kind="stable")]
    head = np.concatenate([[True], a[1:] != a[:-1]])
    at = np.flatnonzero(head)
    return a[at], np.diff(np.concatenate([at, [len(a)]])).astype(U)


def first_index(keys, u):
    """th_first_index_kernel: the smallest record index per row, the row found by lower bound"""
    idx = np.flatnonzero(keys)
    first = np.full(len(u), 0xFFFF_FFFF, U)
    np.minimum.at(first, np.minimum(np.searchsorted(u, keys[idx]), len(u) - 1), idx.astype(U))
    return first


def correct_fill(u, c, fill, n_absent, on):
    """the host's correction; None where fastf_taghist_finish reports "fill key lost" """
    if not (on and n_absent):
        return c
    at = int(np.searchsorted(u, fill))
    if at >= len(u) or u[at] != fill or c[at] <= n_absent:
        return None
    c = c.copy()
    c[at] -= U(n_absent)
    return c


def pipeline_single(keys, drop_digit=None, fill_correction=True):
    present = np.flatnonzero(keys)
    if not len(present):
        return np.zeros(0, U), np.zeros(0, U), np.zeros(0, U)
    mask = T.pass_mask(T.varying_of(keys))
    if drop_digit is not None:
        assert (mask >> drop_digit) & 1
        mask &= ~(1 << drop_digit)
    u, c = lsd_distinct(keys, present[0], mask)
    c = correct_fill(u, c, keys[present[0]], len(keys) - len(present), fill_correction)
    return None if c is None else (u, c, first_index(keys, u))


def pipeline_pairs(k1, k2, m1_bits=lambda m1: T.bits_for(m1), m2_bits=lambda m2: T.bits_for(m2 - 1 if m2 else 0), fill_correction=True):
    n = len(k1)
    valid = np.flatnonzero((k1 != 0) & (k2 != 0))
    out = dict(n_records=n, n_valid=len(valid), n_key1_present=int((k1 != 0).sum()))
    u1, _ = lsd_distinct(k1, np.flatnonzero(k1)[0], T.pass_mask(T.varying_of(k1)))
    u2, _ = lsd_distinct(k2, np.flatnonzero(k2)[0], T.pass_mask(T.varying_of(k2)))
    m1, m2 = len(u1), len(u2)
    code = np.zeros(n, U)
    code[valid] = ((np.searchsorted(u1, k1[valid]).astype(U) + U(1)) << U(32)) | np.searchsorted(u2, k2[valid]).astype(U)
    varying = ((1 << m2_bits(m2)) - 1) | (((1 << m1_bits(m1)) - 1) << 32)
    up, cp = lsd_distinct(code, valid[0], T.pass_mask(varying))
    cp = correct_fill(up, cp, code[valid[0]], n - len(valid), fill_correction)
    if cp is None:
        return None
    pf = first_index(code, up)
    a, b = (up >> U(32)).astype(np.int64) - 1, (up & U(0xFFFF_FFFF)).astype(np.int64)
    if a.min() < 0 or a.max() >= m1 or b.max() >= m2:
        return None                                                 # "pair code out of range"
    c1, f1 = np.zeros(m1, U), np.full(m1, T.NONE, U)
    np.add.at(c1, a, cp)
    np.minimum.at(f1, a, pf)
    out.update(key1=u1, count1=c1, first1=f1, pair_k1=a.astype(np.uint32), pair_key2=u2[b], pair_count=cp, pair_first=pf)
    return out


def single_equal(got, name):
    return got is not None and all(np.array_equal(g, w) for g, w in zip(got, T.want(name)))


def pairs_equal(got, name):
    w = T.want(name)
    return got is not None and all(np.array_equal(got[k], w[k]) if isinstance(w[k], np.ndarray) else got[k] == w[k] for k in w)


def test_the_restated_pipeline_equals_the_reference_on_every_fixture():
    for name, f in T.SINGLE.items():
        assert single_equal(pipeline_single(f["k1"]), name), name
    for name, f in T.PAIRS.items():
        assert pairs_equal(pipeline_pairs(f["k1"], f["k2"]), name), name


def test_each_dropped_digit_changes_its_mask_fixture():
    for name, digits in T.MASKS.items():
        for q in digits:
            assert not single_equal(pipeline_single(T.SINGLE["mask_" + name]["k1"], drop_digit=q), "mask_" + name), (name, q)
    assert not single_equal(pipeline_single(T.SINGLE["extremes"]["k1"], drop_digit=7), "extremes")


def test_one_bit_too_few_for_rank1_changes_the_fixtures_at_its_edges():
    wrong = lambda m1: T.bits_for(m1 - 1)                                                # noqa: E731
    changed = {m: not pairs_equal(pipeline_pairs(T.PAIRS["digits_m1_%d" % m]["k1"], T.PAIRS["digits_m1_%d" % m]["k2"], m1_bits=wrong), "digits_m1_%d" % m)
               for m in T.DIGIT_EDGES_M1}
    assert changed == {1: False, 255: False, 256: True, 257: False, 65535: False, 65536: True}


def test_one_bit_too_few_for_rank2_changes_the_fixtures_at_its_edges():
    wrong = lambda m2: T.bits_for(max(m2 - 2, 0))                                        # noqa: E731
    changed = {m: not pairs_equal(pipeline_pairs(T.PAIRS["digits_m2_%d" % m]["k1"], T.PAIRS["digits_m2_%d" % m]["k2"], m2_bits=wrong), "digits_m2_%d" % m)
               for m in T.DIGIT_EDGES_M2}
    assert changed == {1: False, 2: False, 256: False, 257: True, 65536: False, 65537: True}


def test_a_missing_fill_correction_changes_every_fixture_with_absent_records():
    for name, f in T.SINGLE.items():
        if len(f["k1"]) < T.BIG:
            assert single_equal(pipeline_single(f["k1"], fill_correction=False), name) == (T.census(f)["absent"] == 0), name
    for name in ("dead_key1", "first_valid_late", "digits_m1_1", "digits_m2_65537"):
        assert not pairs_equal(pipeline_pairs(T.PAIRS[name]["k1"], T.PAIRS[name]["k2"], fill_correction=False), name), name


@pytest.mark.parametrize("name", ["fill_once", "first_edges", "grid_stride"])
def test_pieces_cover_the_stream(name):
    f = T.SINGLE[name]
    p = T.pieces(f)
    assert p[0][0] == 0 and p[-1][1] == len(f["k1"]) and all(a[1] == b[0] for a, b in zip(p, p[1:])) and len(p) == len(f["cuts"]) + 1
