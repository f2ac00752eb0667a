"""Keys wider than 64 bits on hand-built (group word, value) pairs: fastf_dev_adopt_wide -> finish() -> umi_rows(), i.e. the pair
sort (scatter_kernel<-1, false, true>, the two stable LSD sorts behind the -u rows), reduce_hashed_kernel<true, true> with
giant_groups_kernel on the values, pair_heads / pair_rows / pair_copies, and the exact fallback of fastf_engine_finish when the
window set or the giant-group list cannot hold a group.  Reference: sortreduce_ref.wide_rows_ref (numpy, uint64, bit-exact)."""
import os

import numpy as np
import pytest

from fastf_amd import hostmem
import sortreduce_ref as S

pytestmark = pytest.mark.gpu

CELLS = np.arange(1, 1001, dtype=np.uint64) | (np.uint64(1) << np.uint64(62))
FEATS = np.arange(1, 501, dtype=np.uint64) | (np.uint64(2) << np.uint64(62))


@pytest.fixture(scope="module")
def engines():
    import torch
    import fastf_amd as F
    assert torch.cuda.is_available()
    made = {}

    def get(kind):
        if kind not in made:
            if kind == "forced12":                          # 12 bases would fit 64 bits: the switch is read when the engine is created
                os.environ["FASTF_FORCE_WIDE_KEYS"] = "1"
                try:
                    made[kind] = (F.Engine(CELLS, FEATS, umi_max_bases=12), S.WideLayout(12))
                finally:
                    del os.environ["FASTF_FORCE_WIDE_KEYS"]
            else:
                bases = {"bases24": 24, "bases32": 32}[kind]
                made[kind] = (F.Engine(CELLS, FEATS, umi_max_bases=bases), S.WideLayout(bases))
            assert made[kind][0].wide
        return made[kind]
    yield torch, F, get
    for eng, _ in made.values():
        eng.close()


def _check(torch, eng, lay, k, v):
    n = len(k)
    eng.reset()
    d_k, d_v = hostmem.to_device(k, "cuda"), hostmem.to_device(v, "cuda")
    eng.dev_adopt_wide(d_k.data_ptr(), d_v.data_ptr(), n, stream=torch.cuda.current_stream().cuda_stream)
    res = eng.finish()
    rows = eng.umi_rows()
    (f, c, cnt), (uf, uc, ncopy, umi, nn) = S.wide_rows_ref(k, v, lay)
    assert res["nnz"] == len(f)
    np.testing.assert_array_equal(res["feature"].astype(np.int64), f)
    np.testing.assert_array_equal(res["cell"].astype(np.int64), c)
    np.testing.assert_array_equal(res["count"].astype(np.int64), cnt)
    assert rows["n"] == len(uf)
    np.testing.assert_array_equal(rows["cell"].astype(np.int64), uc)
    np.testing.assert_array_equal(rows["feature"].astype(np.int64), uf)
    np.testing.assert_array_equal(rows["n_copy"].astype(np.int64), ncopy)
    np.testing.assert_array_equal(rows["nonnull"].astype(np.int64), nn)
    np.testing.assert_array_equal(rows["umi"].astype(np.int64), umi)
    return res


SIZES = {
    "threes": [3] * 50_000,
    "window_edges": [2047, 1, 2047, 5, 900] * 30,
    "one_window": [100, 2048, 100],
    "one_giant": [40_000],
    "ramp": list(range(1, 600)),
    "giants_beyond_the_narrow_limit": [70_000, 9, 65_537, 1],          # (the narrow path stops at 65 536; the wide one at 4 M)
    "list_nearly_full": [2100] * 1900,                                  # 3800 work items of the 4096-item list
}


# every shape with heavy duplication (UMIs from a pool of 200) and with nearly all UMIs distinct on the 24-base engine; the forced
# 12-base engine (another value layout, the same kernels) runs the smaller shapes
GROUP_CASES = [("bases24", name, pool) for name in SIZES for pool in (200, None)] + \
              [("forced12", name, 200) for name in ("window_edges", "one_window", "one_giant", "ramp", "giants_beyond_the_narrow_limit")] + \
              [("forced12", "window_edges", None)]


@pytest.mark.parametrize("kind,name,pool", GROUP_CASES, ids=["%s-%s-%s" % (k, n, "pool%d" % p if p else "distinct") for k, n, p in GROUP_CASES])
def test_wide_pairs_group_sizes(engines, kind, name, pool):
    torch, F, get = engines
    eng, lay = get(kind)
    k, v = S.wide_pairs(SIZES[name], lay, seed=len(name) * 31 + (pool or 0), pool=pool)
    _check(torch, eng, lay, k, v)


@pytest.mark.parametrize("kind", ["bases24", "forced12", "bases32"])
def test_wide_special_pairs(engines, kind):
    """pairs that differ in one bit of v only, equal v under neighbouring k, NULL-only groups, runs of 2047 / 2048 / 2049
    identical pairs and one pair 10 000 times, alone and among 20 000 groups of three"""
    torch, F, get = engines
    eng, lay = get(kind)
    k, v = S.wide_special_pairs(lay)
    _check(torch, eng, lay, k, v)
    k2, v2 = S.wide_pairs([3] * 20_000, lay, seed=12, pool=200)
    rng = np.random.default_rng(4)
    p = rng.permutation(len(k) + len(k2))
    _check(torch, eng, lay, np.concatenate([k, k2])[p], np.concatenate([v, v2])[p])


@pytest.mark.parametrize("sizes,pool", [([3] * 20_000, 200), ([2047, 1, 2049, 700] * 10, None), ([40_000, 5], 3000)])
def test_wide_pairs_with_sub_groups(engines, sizes, pool):
    """beyond 24 bases the sorted word carries the UMI's first bases: K3's rows per sub-group are merged by merge_sub_rows"""
    torch, F, get = engines
    eng, lay = get("bases32")
    k, v = S.wide_pairs(sizes, lay, seed=99 + len(sizes), pool=pool)
    _check(torch, eng, lay, k, v)


@pytest.mark.parametrize("name,sizes,pool", [("list_overflows", [2100] * 2100, 200),            # 4200 work items: more than the list holds
                                             ("group_beyond_4M", [(1 << 22) + 1, 7], 5000)])    # longer than giant_groups_kernel is given
def test_wide_groups_beyond_the_giant_path_are_exact(engines, name, sizes, pool):
    """what the group-only reduce cannot hold (ERR_RUN_TOO_LONG) goes through the exact fallback of fastf_engine_finish: the
    pairs are sorted fully and the distinct non-NULL pairs of every group counted; the engine serves the next job as usual"""
    torch, F, get = engines
    eng, lay = get("bases24")
    k, v = S.wide_pairs(sizes, lay, seed=len(name), pool=pool)
    _check(torch, eng, lay, k, v)
    k, v = S.wide_pairs([3] * 1000, lay, seed=1, pool=200)
    _check(torch, eng, lay, k, v)


def _chain_pairs(lay, m, with_chain=True):
    k, v = S.wide_pairs([9] * 500, lay, seed=500 + m, pool=None)
    chain = S.wide_chain_values(lay.umi_bits, lay.len_bits, m, seed=m)
    if not with_chain:                                      # the same shape with ordinary values in the chain's place
        chain = lay.value(np.random.default_rng(m).integers(0, 1 << lay.umi_bits, size=m, dtype=np.uint64))
    g = np.uint64((1000 << 9) | 500)                        # a group of its own (the last cell and feature: among the 500 with luck only)
    keep = k != g
    ck = np.full(m + 10, g, np.uint64)
    cv = np.concatenate([chain, chain[:7], np.zeros(3, np.uint64)])     # a few copies and NULLs beside the chain
    rng = np.random.default_rng(m)
    p = rng.permutation(int(keep.sum()) + m + 10)
    return np.concatenate([k[keep], ck])[p], np.concatenate([v[keep], cv])[p]


@pytest.mark.parametrize("m", [63, 64, 200])
def test_wide_probe_chain_is_counted_exactly(engines, m):
    """m distinct UMIs of one (cell, feature) that share first slot and step in the window set of reduce_hashed_kernel<true, true>:
    a probe chain ends after 63 tries, so the 64th cannot be placed — a valid input of m reads, which the exact fallback counts.
    63 is what a chain holds: the set itself counts it (finish() shows no flag on this path: the count is what is asserted)"""
    torch, F, get = engines
    eng, lay = get("bases24")
    k, v = _chain_pairs(lay, m)
    res = _check(torch, eng, lay, k, v)
    i = np.flatnonzero((res["cell"] == 1000) & (res["feature"] == 500))
    assert len(i) == 1 and res["count"][i[0]] == m


@pytest.mark.parametrize("m", [63, 64, 200])
def test_narrow_slot64_probe_chain_raises_and_the_full_sort_is_exact(m):
    """the same chain in the SLOT64 form of narrow keys (16 bases): the group-only reduce raises ERR_RUN_TOO_LONG (bit 16), the
    documented full sort and reduce is exact.  The chain's group is the first of the keys: row rank 0 of the first window.
    A chain of 63 is held: no bit is raised and the group-only reduce itself is exact."""
    import torch
    import fastf_amd as F
    eng = F.Engine(CELLS, FEATS, umi_max_bases=16)
    try:
        assert not eng.wide and eng.key_bits == 55 and 0 < eng.skip_bits < 36
        fs, cs = 36, 45
        rng = np.random.default_rng(m)
        x = S.slot64_chain_values(fs, m, seed=m, rank=0)
        ids = rng.choice(999 * 500, size=300, replace=False) + 500            # cells 2.., so (cell 1, feature 1) sorts first
        g = rng.integers(0, 300, size=4000)
        cell = (ids // 500 + 1).astype(np.uint64)[g]; feat = (ids % 500 + 1).astype(np.uint64)[g]
        nonnull = (rng.random(4000) > 0.1).astype(np.uint64)
        umi = rng.integers(0, 1 << 32, size=4000, dtype=np.uint64) * nonnull
        others = (cell << np.uint64(cs)) | (feat << np.uint64(fs)) | (nonnull << np.uint64(35)) | (umi << np.uint64(3)) | (np.uint64(4) * nonnull)
        chain = (np.uint64(1) << np.uint64(cs)) | (np.uint64(1) << np.uint64(fs)) | np.concatenate([x, x[:5]])
        if m == 63:
            # whether 63 members fit depends on nothing else sitting on the chain's walk: a group of 2100 keys sorts right behind
            # the chain's and is still open at the end of the first window, which is then cut at its head and holds the chain alone
            big = rng.choice(1 << 32, size=2100, replace=False).astype(np.uint64)
            others = np.concatenate([others, (np.uint64(1) << np.uint64(cs)) | (np.uint64(2) << np.uint64(fs)) | (np.uint64(1) << np.uint64(35)) | (big << np.uint64(3)) | np.uint64(4)])
        keys = np.concatenate([others, chain])[rng.permutation(len(others) + m + 5)]
        n = len(keys)
        d_keys = hostmem.to_device(keys, "cuda"); d_tmp = torch.empty_like(d_keys)
        d_n = torch.tensor([n], dtype=torch.int64, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        in_tmp = eng.dev_sort(d_keys.data_ptr(), d_tmp.data_ptr(), d_n.data_ptr(), n, stream=s, skip_low=True)
        src = d_tmp if in_tmp else d_keys
        d_f = torch.empty(n, dtype=torch.int32, device="cuda"); d_c = torch.empty_like(d_f); d_k = torch.empty_like(d_f)
        d_nnz = torch.zeros(1, dtype=torch.int64, device="cuda")
        eng.dev_reduce(src.data_ptr(), d_n.data_ptr(), n, d_f.data_ptr(), d_c.data_ptr(), d_k.data_ptr(), d_nnz.data_ptr(), stream=s, skip_low=True)
        torch.cuda.synchronize()
        assert eng.dev_error_bits() == (16 if m > 63 else 0)
        if m > 63:
            eng.dev_clear_error_bits(16, s)
            other = d_keys if in_tmp else d_tmp
            in_other = eng.dev_sort(src.data_ptr(), other.data_ptr(), d_n.data_ptr(), n, stream=s)
            src = other if in_other else src
            eng.dev_reduce(src.data_ptr(), d_n.data_ptr(), n, d_f.data_ptr(), d_c.data_ptr(), d_k.data_ptr(), d_nnz.data_ptr(), stream=s)
            torch.cuda.synchronize()
            assert eng.dev_error_bits() == 0
        f, c, cnt = S.want_rows(keys, fs=fs, cs=cs)
        assert int(d_nnz.item()) == len(f) and f[0] == 1 and c[0] == 1 and cnt[0] == m
        np.testing.assert_array_equal(hostmem.to_host(d_f)[:len(f)].astype(np.int64), f)
        np.testing.assert_array_equal(hostmem.to_host(d_c)[:len(f)].astype(np.int64), c)
        np.testing.assert_array_equal(hostmem.to_host(d_k)[:len(f)].astype(np.int64), cnt)
    finally:
        eng.close()
