"""Hand-built keys for the region-map sort, K3u and the wide-key kernels, with their numpy references (uint64, bit-exact).

No tests here: tests/test_sortreduce_ref_host.py checks these helpers and takes a census of the fixtures,
tests/test_gpu_region_sort.py, test_gpu_umi_rows.py and test_gpu_wide_pairs.py run them on the device."""
import numpy as np

U = np.uint64
M32 = (1 << 32) - 1
SORT_THREADS = 512                       # keys of a sort tile = ipt * 512 (umi_kernels.hpp)
K3_TILE = 2048                           # keys of a K3 window
UW_TILE = 2048                           # pairs of a pair_*_kernel tile

# the fixture engine of test_gpu_kernels.py: 1000 cells x 500 features, 12 bases:  [cell 10][feature 9][nonnull 1][umi 24][len 2]
FS, CS, KEY_BITS = 27, 36, 46
POISON = U((1 << KEY_BITS) - 1)          # all ones in the sorted bits; no fixture key equals it (cell 1023 is not listed)


# ---------------------------------------------------------------------------------------------------------------------
# the region-map sort
# ---------------------------------------------------------------------------------------------------------------------
def regions_buffer(counts, stride, keys, poison=POISON):
    """the n_regions * stride slot buffer: row r holds counts[r] keys (taken from `keys` in order) at its front, every other
    slot holds `poison`"""
    counts = np.asarray(counts, np.int64)
    assert len(counts) and counts.min() >= 0 and counts.max() <= stride and int(counts.sum()) == len(keys)
    buf = np.full(len(counts) * stride, poison, np.uint64)
    buf[_slots(counts, stride)] = np.asarray(keys, np.uint64)
    return buf


def regions_logical(buf, counts, stride):
    """the keys of a regions_buffer back, regions back to back"""
    return np.asarray(buf, np.uint64)[_slots(np.asarray(counts, np.int64), stride)]


def _slots(counts, stride):
    prefix = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return np.repeat(np.arange(len(counts), dtype=np.int64) * stride - prefix, counts) + np.arange(int(counts.sum()), dtype=np.int64)


def layout_keys(rng, n, n_groups=None, umi_values=1 << 24, null_frac=0.1):
    """n keys of the fixture engine's layout in random order: listed cells and features only, so none equals POISON"""
    n_groups = max(1, n // 6) if n_groups is None else n_groups
    ids = rng.choice(1000 * 500, size=min(n_groups, 1000 * 500), replace=False)
    g = rng.integers(0, len(ids), size=n)
    cell = (ids // 500 + 1).astype(np.uint64)[g]; feat = (ids % 500 + 1).astype(np.uint64)[g]
    nonnull = (rng.random(n) > null_frac).astype(np.uint64)
    umi = rng.integers(0, umi_values, size=n, dtype=np.uint64) * nonnull
    return (cell << U(CS)) | (feat << U(FS)) | (nonnull << U(26)) | (umi << U(2)) | (U(3) * nonnull)


def want_rows(keys, fs=FS, cs=CS, feat_bits=9):
    """matrix rows of narrow keys: (feature, cell, distinct non-NULL keys) per (cell, feature), ascending"""
    keys = np.asarray(keys, np.uint64)
    ug = np.unique(keys >> U(fs))
    uk = np.unique(keys[(keys >> U(fs - 1)) & U(1) == 1])
    want = np.zeros(len(ug), dtype=np.int64)
    np.add.at(want, np.searchsorted(ug, uk >> U(fs)), 1)
    return (ug & U((1 << feat_bits) - 1)).astype(np.int64), (ug >> U(cs - fs)).astype(np.int64), want


def _region_cases():
    r = np.random.default_rng(20240)
    small = r.integers(1, 4, size=5000)
    alt = small.copy(); alt[1::2] = 0
    dist = r.integers(10_000, 20_001, size=8)
    loose = r.integers(1000, 3001, size=8)
    # prefix sums 512, 1023, 1025, 1536, 2559, 3584, 4096, 4609: k * 512, k * 512 - 1, k * 512 + 1, and the tiles of ipt 7 and 8
    edges = [512, 511, 2, 511, 1023, 1025, 512, 513, 300]
    C = {}

    def add(name, counts, stride, ipt=None, reduce=False):
        C[name] = dict(counts=np.asarray(counts, np.int64), stride=int(stride), ipt=ipt, reduce=reduce)
    add("one_short", [5000], 6000)
    add("one_full", [4096], 4096)
    add("dist8", dist, 20_480, reduce=True)
    add("full8", [3000] * 8, 3000)
    add("empties_first_last_run5", [0, 0, 700, 0, 0, 0, 0, 0, 1300, 900, 0], 1500)
    add("all_empty_but_one", [0] * 9 + [2000] + [0] * 6, 2000)
    add("all_empty", [0] * 6, 1000)
    add("many_small", small, 4, reduce=True)
    add("many_small_every_other_empty", alt, 4)
    for R in (1023, 1024, 1025, 2049):
        add("scan_carry_%d" % R, [7] * R, 8)
    add("prefix_edges", edges, 1100)
    add("prefix_edges_ipt7", edges, 1100, ipt=7)
    add("prefix_edges_ipt8", edges, 1100, ipt=8)
    add("tail_three_empty_head", [700, 0, 0, 0, 800], 1000)
    add("loose_stride", loose, 8 * int(loose.max()))
    return C


REGION_CASES = _region_cases()


def region_census(counts, tile):
    """(regions, empty regions, sort tiles whose keys come from more than two regions, regions that end on a tile edge)"""
    counts = np.asarray(counts, np.int64)
    n = int(counts.sum())
    rid = np.repeat(np.arange(len(counts)), counts)
    many = sum(1 for t in range(0, n, tile) if len(np.unique(rid[t:t + tile])) > 2)
    ends = np.cumsum(counts)[counts > 0]
    return len(counts), int((counts == 0).sum()), many, int((ends % tile == 0).sum())


# ---------------------------------------------------------------------------------------------------------------------
# K3u: one row per distinct key of fully sorted keys, its count the run length
# ---------------------------------------------------------------------------------------------------------------------
def umi_rows_ref(sorted_keys):
    return np.unique(np.asarray(sorted_keys, np.uint64), return_counts=True)


UMI_RUN_CASES = {
    "one_key": [1],
    "singles": [1] * 70_000,
    "window_edges": [2047, 1, 2048, 1, 2049, 1] * 20,
    "window_at_key_zero": [2048] + [1] * 3000,
    "long_and_short": [5000, 1, 1, 7000, 4096, 3],
    "one_long_run": [300_000],
    "one_then_2047": [1, 2047] * 60,
}


def run_keys(name):
    """sorted keys below POISON with the run lengths of UMI_RUN_CASES[name]; window_at_key_zero starts at key 0"""
    runs = np.asarray(UMI_RUN_CASES[name], np.int64)
    rng = np.random.default_rng(len(runs) * 7919 + int(runs.sum()))
    m = len(runs)
    u = np.unique(rng.integers(1, (1 << KEY_BITS) - 1, size=2 * m + 16, dtype=np.uint64))
    k = np.sort(rng.permutation(u)[:m])
    if name == "window_at_key_zero":
        k[0] = 0
    return np.repeat(k, runs)


def null_run_keys():
    """(cell, feature) groups whose NULL keys (flag clear: the group bits alone) form runs of their own in front of the
    group's UMIs: run lengths 1, 3, 2048 and 2500 of NULL keys, each followed by UMI runs"""
    out = []
    for i, nulls in enumerate([1, 3, 2048, 2500, 2]):
        g = (U(5 + i) << U(CS)) | (U(7 + 3 * i) << U(FS))
        out.append(np.full(nulls, g, np.uint64))
        for j, copies in enumerate([1, 2, 2047, 1]):
            out.append(np.full(copies, g | (U(1) << U(26)) | (U(100 + j) << U(2)) | U(3), np.uint64))
    k = np.concatenate(out)
    assert (np.diff(k.astype(np.int64)) >= 0).all()
    return k


# ---------------------------------------------------------------------------------------------------------------------
# keys wider than 64 bits: (group word, value) pairs
# ---------------------------------------------------------------------------------------------------------------------
class WideLayout:
    """what an engine with wide keys packs: group word k = (cell << feat_bits | feature) [<< 17 | the UMI's first bases, beyond
    24 bases], value v = flag << (umi_bits + len_bits) | umi << len_bits | blob bytes, 0 for a NULL UMI"""

    def __init__(self, umi_max_bases, feat_bits=9):
        self.feat_bits = feat_bits
        self.sub_bits = 0
        if umi_max_bases > 24:
            self.sub_bits, self.umi_bits, self.len_bits, self.max_len = 17, 47, 4, 8
        else:
            self.umi_bits = 2 * umi_max_bases
            self.max_len = (umi_max_bases + 3) // 4
            self.len_bits = self.max_len.bit_length()
        self.nn_shift = self.umi_bits + self.len_bits
        self.flag = 1 << self.nn_shift

    def value(self, umi, length=None):
        umi = np.asarray(umi, np.uint64)
        ln = self.max_len if length is None else length
        return U(self.flag) | (umi << U(self.len_bits)) | U(ln)


def wide_rows_ref(k, v, lay):
    """(matrix rows, -u rows) of (group word, value) pairs.  Matrix rows as dist_doubles.NumpyWideStages.reduce_wide forms them:
    (feature, cell, distinct non-NULL pairs) per (cell, feature).  -u rows: the distinct (k, v) pairs in (k, v) order, NULL
    pairs included: (feature, cell, n_copy, umi = the first 16 bases, nonnull)"""
    k = np.asarray(k, np.uint64); v = np.asarray(v, np.uint64)
    n = len(k)
    assert (((v >> U(lay.nn_shift)) & U(1)) == (v != 0)).all()          # a fixture value is 0 or carries the flag
    order = np.lexsort((v, k))
    k, v = k[order], v[order]
    new = np.ones(n, dtype=bool)
    new[1:] = (k[1:] != k[:-1]) | (v[1:] != v[:-1])
    g = k >> U(lay.sub_bits)
    ug = np.unique(g)
    cnt = np.zeros(len(ug), dtype=np.int64)
    np.add.at(cnt, np.searchsorted(ug, g[new & (v != 0)]), 1)
    fmask = U((1 << lay.feat_bits) - 1)
    matrix = ((ug & fmask).astype(np.int64), (ug >> U(lay.feat_bits)).astype(np.int64), cnt)
    pos = np.flatnonzero(new)
    uk, uv = k[pos], v[pos]
    n_copy = np.diff(np.concatenate([pos, [n]])).astype(np.int64)
    nonnull = ((uv >> U(lay.nn_shift)) & U(1)).astype(np.int64)
    if lay.sub_bits:
        bases = ((uk & U((1 << lay.sub_bits) - 1)) << U(lay.umi_bits)) | ((uv & U(lay.flag - 1)) >> U(lay.len_bits))
        umi = bases >> U(32)
    else:
        field = (uv >> U(lay.len_bits)) & U((1 << lay.umi_bits) - 1)
        umi = field >> U(lay.umi_bits - 32) if lay.umi_bits > 32 else field << U(32 - lay.umi_bits)
    ug2 = uk >> U(lay.sub_bits)
    urows = ((ug2 & fmask).astype(np.int64), (ug2 >> U(lay.feat_bits)).astype(np.int64), n_copy, umi.astype(np.int64), nonnull)
    return matrix, urows


def wide_groups(rng, n_groups):
    """distinct group words cell << 9 | feature of listed cells and features, in random order"""
    ids = rng.choice(1000 * 500, size=n_groups, replace=False)
    return ((ids // 500 + 1).astype(np.uint64) << U(9)) | (ids % 500 + 1).astype(np.uint64)


def wide_pairs(sizes, lay, seed, pool=None, null_frac=0.1):
    """shuffled (k, v) pairs with the given group sizes; pool: UMIs drawn from that many values (None: the whole field)"""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, np.int64)
    k = np.repeat(wide_groups(rng, len(sizes)), sizes)
    n = len(k)
    span = 1 << min(lay.umi_bits, 62)
    umi = rng.integers(0, span, size=n, dtype=np.uint64) if pool is None else rng.integers(0, span, size=pool, dtype=np.uint64)[rng.integers(0, pool, size=n)]
    v = np.where(rng.random(n) < null_frac, U(0), lay.value(umi))
    if lay.sub_bits:                                     # the sorted word carries the UMI's first 17 bases (0 for a NULL UMI)
        k = (k << U(lay.sub_bits)) | np.where(v != 0, rng.integers(0, 3, size=n, dtype=np.uint64) << U(15), U(0))
    p = rng.permutation(n)
    return k[p], v[p]


def wide_special_pairs(lay, seed=77):
    """pairs at the places where the pair kernels and the two sorts branch: equal k with v differing in the top UMI bit only and
    in bit 0 only, equal v under neighbouring k, NULL-only groups, runs of 2047 / 2048 / 2049 identical pairs (the UW_TILE
    edges), one pair 10 000 times"""
    rng = np.random.default_rng(seed)
    g = np.sort(wide_groups(rng, 40))
    base = int(lay.value(U(0x5A5A5A))) & ~0xF
    top = 1 << (lay.nn_shift - 1)
    ks, vs = [], []

    def put(kk, vv, copies=1):
        ks.append(np.full(copies, kk, np.uint64)); vs.append(np.full(copies, vv, np.uint64))
    put(g[0], base); put(g[0], base | top, 2); put(g[0], base | 1, 3); put(g[0], base | top | 1)
    put(g[1], base | 2); put(g[1] + U(1), base | 2); put(g[1] - U(1), base | 2, 2)      # neighbouring group words: other features
    put(g[3], 0, 5); put(g[4], 0, 1); put(g[5], 0, 2049)
    put(g[6], base | 4, 2047); put(g[6], base | 6, 2048); put(g[7], base | 4, 2049); put(g[7], 0, 2048)
    put(g[8], base | 8, 10_000)
    k, v = np.concatenate(ks), np.concatenate(vs)
    if lay.sub_bits:
        k = k << U(lay.sub_bits)
    p = rng.permutation(len(k))
    return k[p], v[p]


# ---------------------------------------------------------------------------------------------------------------------
# probe chains of the window sets of reduce_hashed_kernel
# ---------------------------------------------------------------------------------------------------------------------
A_MUL, B_MUL, C_MUL = 0x9E3779B1, 0x85EBCA77, 0xC2B2AE3D
A_INV = pow(A_MUL, -1, 1 << 32)


def wide_slot_step(x, r):
    """first slot and step of value x of the group with row rank r in the window set of the WIDE branch (4096 slots)"""
    hi = int(x) >> 12
    f = ((hi & M32) * A_MUL + (hi >> 32) * B_MUL) & M32
    return ((int(x) & M32) ^ (f >> 8) ^ (r * 0x9E5)) & 4095, ((f >> 20) & 62) | 1


def slot64_slot_step(x, r):
    """the same for the SLOT64 form of narrow keys (UMIs of 13 to 16 bases): x = the key bits below the feature"""
    hh = ((int(x) & M32) * A_MUL + (int(x) >> 32) * B_MUL + r * C_MUL) & M32
    hh ^= hh >> 15
    return hh & 4095, ((hh >> 20) & 62) | 1


def _free_bits(rng, m, fixed_mask):
    """m distinct 32-bit words that agree in the bits of fixed_mask"""
    free = [b for b in range(32) if not (fixed_mask >> b) & 1]
    assert m <= 1 << len(free)
    fixed = int(rng.integers(0, 1 << 32)) & fixed_mask
    out = []
    for c in rng.choice(1 << len(free), size=m, replace=False):
        w = fixed
        for i, b in enumerate(free):
            w |= ((int(c) >> i) & 1) << b
        out.append(w)
    return out


def wide_chain_values(umi_bits, len_bits, m, seed):
    """m distinct non-NULL values that share the first slot and the step of the WIDE branch, whatever the row rank: the bits of
    x above 44 hold the NULL flag only, f agrees in bits 8-19 (slot) and 21-25 (step), the multiplier of u32(hi) is odd and
    inverts, and the low 12 bits are the same"""
    assert umi_bits + len_bits >= 44
    rng = np.random.default_rng(seed)
    top = 1 << (umi_bits + len_bits - 44)                               # hi >> 32: the flag
    lo = int(rng.integers(0, 4096))
    fixed_mask = (0xFFF << 8) | (0x1F << 21)
    vals = [(top << 44) | ((((f - top * B_MUL) * A_INV) & M32) << 12) | lo for f in _free_bits(rng, m, fixed_mask)]
    return np.array(vals, dtype=np.uint64)


def slot64_chain_values(feat_shift, m, seed, rank=0):
    """m distinct non-NULL x (feat_shift bits: flag, UMI, length) that share the first slot and the step of the SLOT64 form in a
    group of row rank `rank`: hh ^= hh >> 15 is a bijection (undone by hh ^ hh >> 15 ^ hh >> 30), the sum inverts on the low
    word of x; the bits of x above 32 hold the flag only"""
    assert 33 <= feat_shift <= 64
    rng = np.random.default_rng(seed)
    xhi = 1 << (feat_shift - 33)
    fixed_mask = 0xFFF | (0x1F << 21)
    vals = []
    for y in _free_bits(rng, m, fixed_mask):
        hh = (y ^ (y >> 15) ^ (y >> 30)) & M32
        vals.append((xhi << 32) | (((hh - xhi * B_MUL - rank * C_MUL) * A_INV) & M32))
    return np.array(vals, dtype=np.uint64)
