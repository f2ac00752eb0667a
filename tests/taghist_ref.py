"""Hand-built keys for the tag-histogram seam (csrc/tag_hist.hpp: fastf_taghist_push / reserve_device / push_device / finish)
with their numpy references (uint64, bit-exact).

No tests here: tests/test_taghist_ref_host.py checks the references against a dict loop, takes a census of the fixtures and
shows that a host restatement of the device pipeline with one rule wrong changes some fixture's result;
tests/test_gpu_taghist.py runs the fixtures on the device.

A fixture is a dict: k1 (and k2 for the pair fixtures): the keys of the records, 0 = tag absent; cuts: the record indices at
which the stream is cut into pushes.  SINGLE and PAIRS map names to fixtures; a fixture is built when it is first asked for
(four of them have more than two million records) and kept."""
from collections.abc import Mapping

import numpy as np

U = np.uint64
NONE = (1 << 64) - 1                     # first1 of a key1 that never met a present key2
SORT_TILE = 512                          # keys of a sort tile at the smallest ipt (umi_kernels.hpp: SORT_THREADS)
FIRST_ALLOC = 1 << 22                    # th_grow's first allocation, in keys


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def want_single(keys):
    """(distinct present keys ascending, their counts, record index of each key's first occurrence), all uint64"""
    keys = np.asarray(keys, U)
    idx = np.flatnonzero(keys)
    u, first, cnt = np.unique(keys[idx], return_index=True, return_counts=True)
    return u, cnt.astype(U), idx[first].astype(U)


def want_pairs(k1, k2):
    """the two levels of the pair histogram as fastf_taghist_finish reports them.  Level 2: one entry per distinct
    (key1, key2) of the valid records (both present), ordered by (key1, key2): pair_k1 (index into key1), pair_key2,
    pair_count, pair_first.  Level 1: every distinct present key1 ascending, count1 / first1 over the valid records only:
    a key1 that never met a present key2 has count 0 and first NONE."""
    k1, k2 = np.asarray(k1, U), np.asarray(k2, U)
    idx = np.flatnonzero((k1 != 0) & (k2 != 0))
    u1, u2 = np.unique(k1[k1 != 0]), np.unique(k2[k2 != 0])
    m2 = max(len(u2), 1)
    code = np.searchsorted(u1, k1[idx]).astype(np.int64) * m2 + np.searchsorted(u2, k2[idx]).astype(np.int64)     # dense ranks
    uc, first, cnt = np.unique(code, return_index=True, return_counts=True)
    pair_k1, pair_first = uc // m2, idx[first].astype(U)
    count1 = np.zeros(len(u1), U)
    np.add.at(count1, pair_k1, cnt.astype(U))
    first1 = np.full(len(u1), NONE, U)
    np.minimum.at(first1, pair_k1, pair_first)
    return dict(n_records=len(k1), n_valid=len(idx), n_key1_present=int((k1 != 0).sum()),
                key1=u1, count1=count1, first1=first1, pair_k1=pair_k1.astype(np.uint32),
                pair_key2=u2[uc % m2] if len(uc) else np.zeros(0, U), pair_count=cnt.astype(U), pair_first=pair_first)


# ---------------------------------------------------------------------------------------------------------------------
# what the device derives from the keys, restated
# ---------------------------------------------------------------------------------------------------------------------
def bits_for(v):
    """bits needed to hold 0..v, at least one (umi_engine.hip)"""
    return max(int(v).bit_length(), 1)


def pass_mask(varying):
    """th_pass_mask: bit q set iff digit q (bits 8q..8q+7) of `varying` is not zero"""
    return sum(1 << q for q in range(8) if (int(varying) >> (8 * q)) & 255)


def varying_of(keys):
    """OR ^ AND of the present keys (0 if there is none)"""
    p = np.asarray(keys, U)
    p = p[p != 0]
    return int(np.bitwise_or.reduce(p) ^ np.bitwise_and.reduce(p)) if len(p) else 0


def code_masks(m1, m2):
    """pass masks of the two words of the pair code (rank1 + 1) << 32 | rank2, as finish derives them: (low, high)"""
    return pass_mask((1 << bits_for(m2 - 1 if m2 else 0)) - 1), pass_mask(((1 << bits_for(m1)) - 1) << 32)


def census(f):
    """what a fixture holds, so that tests/test_taghist_ref_host.py can pin it"""
    k1 = f["k1"]
    if "k2" not in f:
        u, c, first = want_single(k1)
        present = np.flatnonzero(k1)
        fill = int(c[np.searchsorted(u, k1[present[0]])]) if len(present) else 0
        return dict(n=len(k1), m1=len(u), mask=pass_mask(varying_of(k1)), fill_count=fill, absent=len(k1) - len(present))
    k2 = f["k2"]
    w = want_pairs(k1, k2)
    m1, m2 = len(w["key1"]), len(np.unique(k2[k2 != 0]))
    fill = 0
    if w["n_valid"]:
        at = int(np.flatnonzero(w["pair_first"] == w["pair_first"].min())[0])       # the pair of the first valid record
        fill = int(w["pair_count"][at])
    lo, hi = code_masks(m1, m2)
    return dict(n=len(k1), m1=m1, m2=m2, pairs=len(w["pair_k1"]), mask1=pass_mask(varying_of(k1)), mask2=pass_mask(varying_of(k2)),
                code_lo=lo, code_hi=hi, fill_count=fill, absent=len(k1) - w["n_valid"], dead_key1=int((w["count1"] == 0).sum()))


# ---------------------------------------------------------------------------------------------------------------------
# single-tag fixtures
# ---------------------------------------------------------------------------------------------------------------------
MASKS = {"d0": (0,), "d1": (1,), "d2": (2,), "d3": (3,), "d4": (4,), "d5": (5,), "d6": (6,), "d7": (7,),
         "d07": (0, 7), "d67": (6, 7), "d135": (1, 3, 5), "d0246": (0, 2, 4, 6), "all_but_3": (0, 1, 2, 4, 5, 6, 7),
         "all": (0, 1, 2, 3, 4, 5, 6, 7)}
CONST_BYTES = (0x5A, 0x3C, 0xA7, 0x19, 0xE1, 0x42, 0x8D, 0x76)       # the byte of digit q where it does not vary


def _const_key(digits_inside):
    return sum(CONST_BYTES[q] << (8 * q) for q in range(8) if q not in digits_inside)


def _mask_fixture(digits, seed):
    """n = 1537 = three tiles of 512 and one key: the digits named take 220 values (0x00 and 0xFF among them), each digit on
    its own, over a pool of 400 keys, every other digit holds its byte of CONST_BYTES; for every digit named, two more keys
    differ from pool key 0 in that digit only, so that no pass can be left out unseen; about 5 % of the records are absent"""
    r = np.random.default_rng(seed)
    n, pool_n = 3 * SORT_TILE + 1, 400
    vals = np.concatenate([[0x00, 0xFF], 1 + r.choice(254, size=218, replace=False)]).astype(U)
    pool = np.full(pool_n, _const_key(digits), U)
    for q in digits:
        pool |= vals[r.permutation(pool_n) % 220] << U(8 * q)
    pool = np.concatenate([pool] + [pool[:1] ^ U(flip << (8 * q)) for q in digits for flip in (0x55, 0xAA)])
    assert pool.min() > 0
    pool_n = len(pool)
    k = pool[np.concatenate([r.permutation(pool_n), r.integers(0, pool_n, n - pool_n)])]
    r.shuffle(k)
    k[r.choice(n - 1, size=77, replace=False)] = 0                   # (the one key of the last tile stays)
    return dict(k1=k, cuts=[SORT_TILE + 1])


def _pool(r, m, bits=62):
    """m distinct non-zero keys, unordered"""
    v = np.unique(r.integers(1, 1 << bits, size=m + m // 8 + 8, dtype=U))
    assert len(v) >= m
    return r.permutation(v)[:m]


def _fill_once(r):
    pool = _pool(r, 41)
    rest = pool[1:][r.integers(0, 40, 2000)]
    rest[r.choice(2000, size=600, replace=False)] = 0
    return dict(k1=np.concatenate([np.zeros(900, U), pool[:1], rest]), cuts=[500, 1800])


def _fill_hot(r):
    n, pool = 4000, _pool(r, 31)
    k = np.full(n, pool[0], U)
    other = r.choice(np.arange(1, n), size=400, replace=False)
    k[other[:200]] = 0
    k[other[200:]] = pool[1:][r.integers(0, 30, 200)]
    return dict(k1=k, cuts=[1333])


def _one_present(at):
    k = np.zeros(1000, U)
    k[at] = U(0x00C0FFEE12345678)
    return dict(k1=k, cuts=[400])


def _first_edges(r):
    """n = 3 * 256 + 1: th_first_index_kernel's workgroups hold records [0, 256), [256, 512), [512, 768) and record 768.  Six
    keys have their first occurrences at 0, 255, 256, 511, 512 and n - 1; a seventh is first seen at record 3 and again at
    the first record of each later workgroup that no edge key claims (257 and 513: the last workgroup is record n - 1
    alone).  Every other record repeats a key that was first seen before it, or is absent."""
    n = 3 * 256 + 1
    edges, spans = [0, 255, 256, 511, 512, n - 1], [3, 257, 513]
    keys = _pool(r, 7)
    k = np.zeros(n, U)
    k[edges] = keys[:6]
    k[spans] = keys[6]
    taken = set(edges + spans)
    for i in range(n):
        if i in taken or r.random() < 0.05:
            continue
        seen = [keys[j] for j, e in enumerate(edges) if e < i]
        k[i] = seen[r.integers(0, len(seen))]
    return dict(k1=k, cuts=[255], edges=edges, spans=spans)


def _extremes(r):
    """the ends of the key range, the 64 single-bit keys and, for every byte, two keys that differ in that byte's low bit
    only; shuffled, n no multiple of 512, and a 2^64 - 1 in the last, partial tile"""
    base = 0x6A3C_A496_C0E2_4E82                                     # (every byte's low bit is clear)
    assert all(not (base >> (8 * q)) & 1 for q in range(8))
    vals = [1, 2, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 2, (1 << 64) - 1] + [1 << b for b in range(64)]
    for q in range(8):
        vals += [base, base | (1 << (8 * q))]
    vals = np.array(vals, U)
    k = np.repeat(vals, r.integers(1, 5, len(vals)))
    k = np.concatenate([k, np.zeros(23, U), vals[r.integers(0, len(vals), 1100)]])
    r.shuffle(k)
    k = np.concatenate([k, [U((1 << 64) - 1)]])
    assert len(k) % SORT_TILE not in (0, 1) and len(k) > 2 * SORT_TILE
    return dict(k1=k, cuts=[len(k) // 2])


def _runs(r):
    """one key 5000 times, 3000 keys once each, one key 2049 times, ascending: K3u's window edges through this seam"""
    mid = np.sort(_pool(r, 3000, bits=40)) + U(1 << 41)
    return dict(k1=np.concatenate([np.full(5000, 77, U), mid, np.full(2049, 1 << 50, U)]), cuts=[5000, 8000])


def _grid_stride(r):
    """n = 2^21 + 1: a second iteration of every grid-capped th_* loop.  3000 distinct keys that vary in digits 0, 1 and 5;
    one occurs at record n - 1 only, one is first seen at record 2^20 (the first record of th_fill_copy_kernel's second
    iteration) and again behind it; 5 % absent"""
    n = (1 << 21) + 1
    ends = [0x0000, 0xFFFF, 0x00FF, 0xFF00]
    v = np.concatenate([ends, r.choice(np.setdiff1d(np.arange(1 << 16), ends), size=2996, replace=False)]).astype(U)
    d5 = (v * U(37) + U(11)) & U(255)
    d5[:2] = [0x00, 0xFF]
    pool = U(_const_key((0, 1, 5))) | v | (d5 << U(40))
    assert len(np.unique(pool)) == 3000
    last, mid, pool = pool[2998], pool[2999], pool[:2998]
    k = pool[r.integers(0, 2998, n)]
    behind = (1 << 20) + 1 + r.choice((1 << 20) - 1, size=500, replace=False)
    k[behind] = mid
    k[r.random(n) < 0.05] = 0
    k[1 << 20], k[behind[0]], k[n - 1] = mid, mid, last
    return dict(k1=k, cuts=[700_001], last=int(last), mid=int(mid))


def _grows(r):
    """n = 2^22 + 5 > th_grow's first allocation, pushed as 1000 + the rest; 50 distinct keys that vary in digit 2 only"""
    n = FIRST_ALLOC + 5
    pool = U(_const_key((2,))) | (r.choice(256, size=50, replace=False).astype(U) << U(16))
    k = pool[r.integers(0, 50, n)]
    k[r.random(n) < 0.03] = 0
    return dict(k1=k, cuts=[1000])


def _build_single(name):
    seed = 7000 + sorted(SINGLE_NAMES).index(name)
    if name.startswith("mask_"):
        return _mask_fixture(MASKS[name[5:]], seed)
    r = np.random.default_rng(seed)
    return {"fill_once": _fill_once, "fill_hot": _fill_hot, "one_present_first": lambda r: _one_present(0),
            "one_present_last": lambda r: _one_present(999), "first_edges": _first_edges, "extremes": _extremes, "runs": _runs,
            "grid_stride": _grid_stride, "grows": _grows}[name](r)


SINGLE_NAMES = ["mask_" + m for m in MASKS] + ["fill_once", "fill_hot", "one_present_first", "one_present_last", "first_edges",
                                               "extremes", "runs", "grid_stride", "grows"]


# ---------------------------------------------------------------------------------------------------------------------
# pair fixtures
# ---------------------------------------------------------------------------------------------------------------------
DIGIT_EDGES_M1 = (1, 255, 256, 257, 65535, 65536)
DIGIT_EDGES_M2 = (1, 2, 256, 257, 65536, 65537)


def _digits(r, m1, m2):
    """exactly m1 distinct key1 and m2 distinct key2, every one of them in a valid pair, (smallest, smallest) and (largest,
    largest) among the pairs; the records beyond that cover are random, some with a tag absent"""
    n = 70_000 if max(m1, m2) > 60_000 else 2000
    v1, v2 = np.sort(_pool(r, m1)), np.sort(_pool(r, m2))
    cover = max(m1, m2)
    a = np.concatenate([np.arange(cover) % m1, [m1 - 1], r.integers(0, m1, n - cover - 1)])
    b = np.concatenate([np.arange(cover) % m2, [m2 - 1], r.integers(0, m2, n - cover - 1)])
    k1, k2 = v1[a], v2[b]
    free = cover + 1 + np.flatnonzero(r.random(n - cover - 1) < 0.1)
    k1[free[0::2]] = 0
    k2[free[1::2]] = 0
    p = r.permutation(n)
    return dict(k1=k1[p], k2=k2[p], cuts=[n // 3])


def _dead_key1(r):
    """three key1 values whose key2 is always absent — the smallest key1, the largest, and the first present key1 of the
    stream (the fill key of the key1 sort) — among twenty live ones"""
    n = 2000
    v1, v2 = np.sort(_pool(r, 23)), _pool(r, 60)
    dead, live = v1[[0, 22, 11]], np.delete(v1, [0, 11, 22])
    k1, k2 = live[r.integers(0, 20, n)], v2[r.integers(0, 60, n)]
    at = r.choice(np.arange(2, n), size=150, replace=False)
    k1[at[:90]], k2[at[:90]] = dead[r.integers(0, 3, 90)], 0
    k1[at[90:93]], k2[at[90:93]] = dead, 0                           # each of the three at least once
    k1[at[93:120]] = 0
    k2[at[120:]] = 0
    k1[0], k2[0] = 0, v2[0]
    k1[1], k2[1] = dead[2], 0
    return dict(k1=k1, k2=k2, cuts=[777], dead=np.sort(dead))


def _first_valid_late(r):
    """the first 700 records miss one of the two tags by turns; record 700 is the first valid pair and the only copy of it"""
    n = 2200
    v1, v2 = _pool(r, 31), _pool(r, 41)
    k1, k2 = v1[1:][r.integers(0, 30, n)], v2[1:][r.integers(0, 40, n)]
    k1[1:700:2] = 0
    k2[0:700:2] = 0
    k1[700], k2[700] = v1[0], v2[0]
    late = 701 + np.flatnonzero(r.random(n - 701) < 0.1)
    k1[late[0::2]] = 0
    k2[late[1::2]] = 0
    return dict(k1=k1, k2=k2, cuts=[350, 700])


def _one_key1_300k(r):
    """one key1 with 300 000 distinct key2 (th_par_for's slices all fall inside one key1), ten pairs of a smaller and ten of a
    larger key1 around it"""
    v2 = _pool(r, 300_000)
    k2 = np.concatenate([v2, v2[:20], v2[r.integers(0, 300_000, 80)]])
    k1 = np.concatenate([np.full(300_000, 1 << 40, U), np.full(10, 5, U), np.full(10, 1 << 60, U), np.full(80, 1 << 40, U)])
    k1[300_020:300_040] = 0
    k2[300_040:300_060] = 0
    p = r.permutation(len(k1))
    return dict(k1=k1[p], k2=k2[p], cuts=[100_000])


def _forty_key1(r):
    """40 key1 values whose numbers of distinct key2 grow by a third from one to the next, 300 000 pairs in all"""
    w = 1.33 ** np.arange(40)
    sizes = np.maximum(1, np.floor(w / w.sum() * 300_000)).astype(np.int64)
    sizes[-1] += 300_000 - sizes.sum()
    v1, v2 = r.permutation(np.sort(_pool(r, 40))), _pool(r, int(sizes.max()))
    a = np.repeat(np.arange(40), sizes)
    b = np.concatenate([np.arange(s) for s in sizes])
    extra = r.integers(0, 300_000, 20_000)
    a, b = np.concatenate([a, a[extra]]), np.concatenate([b, b[extra]])
    k1, k2 = v1[a], v2[b]
    k1[300_000:301_000] = 0                                          # (among the extra copies: every pair stays)
    k2[301_000:302_000] = 0
    p = r.permutation(len(k1))
    return dict(k1=k1[p], k2=k2[p], cuts=[160_000], sizes=sizes)


def _pair_random(r, n, m1, m2, p1, p2, cuts, narrow=False):
    if narrow:                                                       # key1 varies in digit 3 only, key2 in digit 6 only
        v1 = U(_const_key((3,))) | (r.choice(256, size=m1, replace=False).astype(U) << U(24))
        v2 = U(_const_key((6,))) | (r.choice(256, size=m2, replace=False).astype(U) << U(48))
    else:
        v1, v2 = _pool(r, m1), _pool(r, m2)
    k1, k2 = v1[r.integers(0, m1, n)], v2[r.integers(0, m2, n)]
    k1[r.random(n) < p1] = 0
    k2[r.random(n) < p2] = 0
    return dict(k1=k1, k2=k2, cuts=cuts)


def _build_pairs(name):
    r = np.random.default_rng(9000 + sorted(PAIR_NAMES).index(name))
    if name.startswith("digits_m1_"):
        return _digits(r, int(name[10:]), 300)
    if name.startswith("digits_m2_"):
        return _digits(r, 300, int(name[10:]))
    return {"dead_key1": _dead_key1, "first_valid_late": _first_valid_late, "one_key1_300k": _one_key1_300k, "forty_key1": _forty_key1,
            "pair_grid_stride": lambda r: _pair_random(r, (1 << 21) + 1, 700, 900, 0.06, 0.04, [900_000]),
            "pair_grows": lambda r: _pair_random(r, FIRST_ALLOC + 5, 50, 60, 0.03, 0.03, [1000], narrow=True)}[name](r)


PAIR_NAMES = (["digits_m1_%d" % m for m in DIGIT_EDGES_M1] + ["digits_m2_%d" % m for m in DIGIT_EDGES_M2] +
              ["dead_key1", "first_valid_late", "one_key1_300k", "forty_key1", "pair_grid_stride", "pair_grows"])


class _Fixtures(Mapping):
    """name -> fixture, built from its fixed seed when first asked for"""

    def __init__(self, names, build):
        self._names, self._build, self._made = list(names), build, {}

    def __getitem__(self, name):
        if name not in self._made:
            if name not in self._names:
                raise KeyError(name)
            f = self._build(name)
            f["k1"] = np.ascontiguousarray(f["k1"], U)
            f["k1"].setflags(write=False)
            if "k2" in f:
                f["k2"] = np.ascontiguousarray(f["k2"], U)
                f["k2"].setflags(write=False)
                assert len(f["k1"]) == len(f["k2"])
            assert all(0 < c < len(f["k1"]) for c in f["cuts"]) and sorted(f["cuts"]) == f["cuts"]
            self._made[name] = f
        return self._made[name]

    def __iter__(self):
        return iter(self._names)

    def __len__(self):
        return len(self._names)


SINGLE = _Fixtures(SINGLE_NAMES, _build_single)
PAIRS = _Fixtures(PAIR_NAMES, _build_pairs)
BIG = 10_000                                                         # fixtures below this many records also meet the dict loop


def pieces(f):
    """(start, end) of the pushes of a fixture"""
    edges = [0] + list(f["cuts"]) + [len(f["k1"])]
    return list(zip(edges[:-1], edges[1:]))


_want = {}


def want(name):
    """the reference result of a fixture, computed once"""
    if name not in _want:
        _want[name] = want_single(SINGLE[name]["k1"]) if name in SINGLE_NAMES else want_pairs(PAIRS[name]["k1"], PAIRS[name]["k2"])
    return _want[name]
