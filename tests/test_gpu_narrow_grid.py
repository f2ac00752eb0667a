"""The step's grid-capped kernels with more tiles than workgroups.

Every engine here is created under FASTF_GRID_CUS = 1 or 3 ("Grid switches"), so a workgroup walks its tile loop three
times and more where the rest of the suite walks it once.  Each test first asks fastf_engine_grids for the kernels it claims and
requires tiles >= 3 * workgroups (K3: at least 5 windows in every chunk): a condition, not a measurement.  Every comparison is
exact, against numpy, sortreduce_ref.want_rows or the oracle."""
import os

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import hostmem
from helpers import Case, assert_matches_oracle
import lookup_ref as R_
import sortreduce_ref as S
from test_gpu_parity import CASES, STREAM_CASES, WIDE_CASES

pytestmark = pytest.mark.gpu

U = np.uint64
WIDTHS = ["1", "3"]
CELLS = np.arange(1, 1001, dtype=np.uint64) | (U(1) << U(62))
FEATS = np.arange(1, 501, dtype=np.uint64) | (U(2) << U(62))
W = S.K3_TILE


def _engine(monkeypatch, width, bases=12, **env):
    monkeypatch.setenv("FASTF_GRID_CUS", width)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return F.Engine(CELLS, FEATS, umi_max_bases=bases)


def _trips(eng, families, n_records=0, n_keys=0, least=3):
    g = eng.grids(n_records, n_keys)
    for f in families:
        wg, tiles = g[f]
        assert wg > 0 and tiles >= least * wg, "%s: %d tiles on %d workgroups is no %d trips" % (f, tiles, wg, least)
    return g


def _chunks(eng, family, n_keys, least=5):
    """the chunk edges of K3 (k3_chunk_start: (T b / G) windows), every chunk of at least `least` windows"""
    G, T = eng.grids(0, n_keys)[family]
    cuts = [min((T * b // G) * W, n_keys) for b in range(G + 1)]
    assert G > 0 and min(np.diff(cuts)) >= least * W, "%s: chunks %s" % (family, np.diff(cuts) // W)
    return cuts


def _dev(torch, a):
    return hostmem.to_device(a, "cuda")


# ---------------------------------------------------------------------------------------------------------------------
# the query itself
# ---------------------------------------------------------------------------------------------------------------------
def test_default_grids_are_the_expressions_of_the_launches(capsys):
    """with no switch set the query reports min(tiles, k * CUs) with the device's CU count: the expressions the launches carried
    before they moved into helpers, restated here for the families that do not depend on the table images"""
    import torch
    assert "FASTF_GRID_CUS" not in os.environ and "FASTF_TILE_GRID_CAP" not in os.environ and "FASTF_K3_PER_CU" not in os.environ
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    eng = F.Engine(CELLS, FEATS, umi_max_bases=12)
    try:
        for n in (100_000, 10_000_000, 200_000_000):
            g = eng.grids(n, n)
            with capsys.disabled():
                print("\n[grids] n = %d: %s" % (n, g))
            slots = 4 * cus
            rounds = max(1, -(-n // (slots * 512 * 7)))
            ipt = min(7, max(1, -(-n // (rounds * slots * 512))))
            T = -(-n // (ipt * 512))
            assert g["sort_tiles"] == (min((T + 7) & ~7, (32 * cus) & ~7), T)
            win = -(-n // W)
            assert g["k3_windows"] == (min(win, 4 * cus, 4096), win)
            assert g["k3_hashed"] == (min(win, 4 * cus, 4096, 3 * cus), win)
            assert g["rows_gather"][0] == g["k3_hashed"][0]
            assert g["giant"] == (cus + 1, 0)
            assert g["pairs"] == (min(win, 16 * cus), win)
            R = -(-n // 65536)
            assert g["rgn_hist"] == (min(R, 8 * cus), R)
            units = -(-n // 256)
            assert g["block_records"] == (min((units + 3) // 4, 16 * cus), (units + 3) // 4)
            assert g["draw_bits"] == (min((n + 255) // 256 + 1, 8 * cus), (-(-n // 64) + 15) // 16)
            tiles = -(-n // 4096)
            assert g["k1a"][1] in (tiles, (tiles + 1) // 2) and g["k1b_tiles"][1] == tiles
            # the K1 forms of this engine's tables: barcodes in the L2 table behind the LDS miss filter (four K1a workgroups per CU); genes
            # in LDS, gb = 1 to 3 K1b workgroups per CU by the image, the streaming form at most two, with 16 or 12 waves and about four units a wave
            assert eng.table_modes.startswith("cells:L2") and "genes:LDS" in eng.table_modes
            su = tiles * 16
            assert g["k1a"] == (min(tiles, 4 * cus), tiles)
            assert (g["k1b_tiles"], g["k1b_stream"]) in [((min(tiles, gb * cus), tiles), (max(1, min(-(-su // (4 * w)), min(gb, 2) * cus)), -(-su // w)))
                                                         for gb, w in ((1, 16), (2, 12), (3, 12))]
            assert g["scatter_regions"] == (min((2 * g["k1b_stream"][0] + 7) & ~7, (32 * cus) & ~7), 2 * g["k1b_stream"][0])
    finally:
        eng.close()


def test_an_engine_keeps_its_width_when_another_is_created(monkeypatch):
    monkeypatch.setenv("FASTF_GRID_CUS", "1")
    monkeypatch.setenv("FASTF_TILE_GRID_CAP", "16")
    monkeypatch.setenv("FASTF_K3_PER_CU", "2")
    a = F.Engine(CELLS, FEATS, umi_max_bases=12)
    for k in ("FASTF_GRID_CUS", "FASTF_TILE_GRID_CAP", "FASTF_K3_PER_CU"):
        monkeypatch.delenv(k)
    b = F.Engine(CELLS, FEATS, umi_max_bases=12)
    try:
        ga, gb = a.grids(300_000, 300_000), b.grids(300_000, 300_000)
        assert ga["sort_tiles"][0] == 16 and ga["k3_windows"][0] == 2 and ga["k3_hashed"][0] == 2 and ga["giant"][0] == 2
        assert gb["sort_tiles"][0] > 16 and gb["k3_windows"][0] > 2 and gb["giant"][0] > 2
        monkeypatch.setenv("FASTF_GRID_CUS", "100000")             # clamped to the device's
        c = F.Engine(CELLS, FEATS, umi_max_bases=12)
        monkeypatch.setenv("FASTF_GRID_CUS", "0")                  # ... and to 1
        d = F.Engine(CELLS, FEATS, umi_max_bases=12)
        assert c.grids(300_000, 300_000) == gb and d.grids(0, 300_000)["giant"][0] == 2
        monkeypatch.setenv("FASTF_TILE_GRID_CAP", "3")             # the floor of the XCD stride: a multiple of 8, at least 8
        e = F.Engine(CELLS, FEATS, umi_max_bases=12)
        assert e.grids(0, 300_000)["sort_tiles"][0] == 8
        c.close(); d.close(); e.close()
        assert a.grids(300_000, 300_000) == ga
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------------
# K2 on the second and later tiles of a workgroup
# ---------------------------------------------------------------------------------------------------------------------
def _sort_check(torch, eng, keys, key_bits, skip_low):
    """dev_sort of `keys`; both buffers carry half as many guard words again behind the keys"""
    n = len(keys)
    guard = U(0x5A5A_0123_4567_89AB)
    slack = n // 2 + 64
    d_keys = _dev(torch, np.concatenate([keys, np.full(slack, guard, np.uint64)]))
    d_tmp = _dev(torch, np.full(n + slack, guard, np.uint64))
    d_n = torch.tensor([n], dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    in_tmp = eng.dev_sort(d_keys.data_ptr(), d_tmp.data_ptr(), d_n.data_ptr(), n, key_bits=None if skip_low else key_bits, stream=s,
                          skip_low=skip_low)
    torch.cuda.synchronize()
    assert eng.dev_error_bits() == 0
    a, b = hostmem.to_host(d_keys).view(np.uint64), hostmem.to_host(d_tmp).view(np.uint64)
    assert (a[n:] == guard).all() and (b[n:] == guard).all()
    got = (b if in_tmp else a)[:n]
    if skip_low:
        assert (np.diff((got >> U(eng.skip_bits)).astype(np.int64)) >= 0).all()
        np.testing.assert_array_equal(np.sort(got), np.sort(keys))
    else:
        np.testing.assert_array_equal(got, np.sort(keys))


def _tile_geometry(eng, n):
    wg, T = eng.grids(0, n)["sort_tiles"]
    tile = next(k * 512 for k in range(1, 9) if -(-n // (k * 512)) == T)
    return wg, T, tile


def _shaped_keys(eng, n, bits, shapes, seed):
    """keys whose tiles take the digit shapes `shapes` by turns ALONG THE WALK of a workgroup (it takes the tiles r, r + S, .. of
    its XCD's range, S = grid / 8): 'zero' every digit 0, 'uniform', 'ones' every digit 255 — the padding digit of a partial tile"""
    wg, T, tile = _tile_geometry(eng, n)
    chunk, S_ = (T + 7) // 8, wg // 8
    rng = np.random.default_rng(seed)
    t = np.arange(n) // tile
    trip = (t % chunk) // S_
    shape = np.asarray(shapes)[trip % len(shapes)]
    mask = U((1 << bits) - 1) if bits < 64 else U(0xFFFF_FFFF_FFFF_FFFF)
    k = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * U(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
    k = np.where(shape == "zero", U(0), np.where(shape == "ones", U(0xFFFF_FFFF_FFFF_FFFF), k)) & mask
    assert len(set(shape.tolist())) == len(set(shapes))
    return k


# 384 and 385 tiles of 512 keys: an exact multiple of the tile and one key more (the partial tile is the last one its workgroup
# walks, after full ones); the sizes of test_dev_sort_matches_numpy that make three trips at both widths
@pytest.mark.parametrize("skip_low", [False, True], ids=["full", "skip_low"])
@pytest.mark.parametrize("n,bits", [(196_608, 64), (196_609, 64), (196_608 + 513, 33), (300_000, 64), (1_000_000, 56)])
@pytest.mark.parametrize("width", WIDTHS)
def test_sort_with_opposite_digit_shapes_on_consecutive_tiles(monkeypatch, width, n, bits, skip_low):
    import torch
    eng = _engine(monkeypatch, width)
    try:
        _trips(eng, ["sort_tiles"], n_keys=n)
        if skip_low:
            bits = eng.key_bits
        _sort_check(torch, eng, _shaped_keys(eng, n, bits, ["zero", "uniform", "ones"], n + bits), bits, skip_low)
    finally:
        eng.close()


@pytest.mark.parametrize("skip_low", [False, True], ids=["full", "skip_low"])
@pytest.mark.parametrize("width", WIDTHS)
def test_sort_digit_that_occurs_only_in_the_last_partial_tile(monkeypatch, width, skip_low):
    import torch
    eng = _engine(monkeypatch, width)
    try:
        n = 196_608 + 5
        _trips(eng, ["sort_tiles"], n_keys=n)
        bits = eng.key_bits if skip_low else 64
        k = _shaped_keys(eng, n, bits, ["zero", "ones"], 5)
        k[-5:] = U(0x7777_7777_7777_7777) & U((1 << bits) - 1 if bits < 64 else 0xFFFF_FFFF_FFFF_FFFF)
        _sort_check(torch, eng, k, bits, skip_low)
    finally:
        eng.close()


@pytest.mark.parametrize("skip_low", [False, True], ids=["full", "skip_low"])
@pytest.mark.parametrize("width", WIDTHS)
def test_segmented_first_pass_over_long_regions_with_empty_ones_between(monkeypatch, width, skip_low):
    """tile_count_kernel<true> and scatter_kernel<-1, true> through the region map: regions of more than three sort tiles, runs of
    empty regions between them, a workgroup several tiles deep (tests/test_gpu_region_sort.py's runner at a narrow grid)"""
    import torch
    eng = _engine(monkeypatch, width)
    try:
        rng = np.random.default_rng(11)
        counts = np.zeros(400, np.int64)
        counts[::4] = rng.integers(1537, 2400, size=100)           # > 3 tiles of 512 keys; three empty regions behind each
        counts[398] = 1
        stride, R, n = 2400, len(counts), int(counts.sum())
        max_n = R * stride
        _trips(eng, ["sort_tiles"], n_keys=n)
        keys = S.layout_keys(rng, n)
        d_keys = _dev(torch, S.regions_buffer(counts, stride, keys))
        guard = U(0x0123_4567_89AB)
        d_tmp = _dev(torch, np.full(max_n, guard, np.uint64))
        d_counts = _dev(torch, counts.astype(np.uint64))
        d_n = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        eng.dev_set_regions(d_counts.data_ptr(), R, stride, d_n.data_ptr(), stream=s)
        in_tmp = eng.dev_sort(d_keys.data_ptr(), d_tmp.data_ptr(), d_n.data_ptr(), max_n, stream=s, skip_low=skip_low, segmented=True)
        torch.cuda.synchronize()
        assert int(d_n.item()) == n and eng.dev_error_bits() == 0
        got = hostmem.to_host(d_tmp if in_tmp else d_keys).view(np.uint64)[:n]
        assert not (got == S.POISON).any()
        if skip_low:
            assert (np.diff((got >> U(eng.skip_bits)).astype(np.int64)) >= 0).all()
            np.testing.assert_array_equal(np.sort(got), np.sort(keys))
        else:
            np.testing.assert_array_equal(got, np.sort(keys))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# K3 in its steady state: chunks of many windows
# ---------------------------------------------------------------------------------------------------------------------
class Lay:
    """key layout of the 1000 x 500 fixture engine with UMIs of `bases` bases: [cell 10][feature 9][nonnull 1][umi][len]"""
    def __init__(self, bases):
        nbytes = (bases + 3) // 4
        self.len_bits = int(nbytes).bit_length()
        self.umi_bits = 2 * bases
        self.fs = 1 + self.umi_bits + self.len_bits
        self.cs = self.fs + 9
        self.len_full = nbytes


N_K3 = 72 * W           # width 1: 4 (hashed 3) chunks of 18 (24) windows; width 3: 12 (9) chunks of 6 (8)


def _groups_to_keys(lay, sizes, kinds, seed, shuffle):
    """groups of the given sizes, group ids ascending; kind 'distinct': every key its own UMI, 'dup': one UMI, 'few': 5 UMIs and a
    tenth NULL keys; shuffle: the keys of a group in random order (what a group-only sort leaves)"""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, np.int64)
    m = len(sizes)
    ids = np.sort(rng.choice(1000 * 500, size=m, replace=False))
    gid = ((ids // 500 + 1).astype(np.uint64) << U(lay.cs)) | ((ids % 500 + 1).astype(np.uint64) << U(lay.fs))
    out = []
    for g, (sz, kind) in enumerate(zip(sizes.tolist(), kinds)):
        if kind == "distinct":
            umi = rng.choice(1 << min(lay.umi_bits, 22), size=sz, replace=False).astype(np.uint64)
            nn = np.ones(sz, np.uint64)
        elif kind == "dup":
            umi = np.full(sz, 12345, np.uint64); nn = np.ones(sz, np.uint64)
        else:
            umi = rng.integers(0, 5, size=sz, dtype=np.uint64) * U(0x3_0101) & U((1 << lay.umi_bits) - 1)
            nn = (rng.random(sz) > 0.1).astype(np.uint64)
        k = gid[g] | (nn << U(lay.fs - 1)) | ((umi << U(lay.len_bits)) | U(lay.len_full)) * nn
        out.append(rng.permutation(k) if shuffle else np.sort(k))
    return np.concatenate(out)


def _sizes_from_edges(edges):
    return np.diff(np.asarray(sorted(set(edges)), np.int64))


def _steady_cases(cuts):
    """group edges placed against the chunk edges `cuts` (multiples of the window): name -> (sizes, kinds)"""
    n = cuts[-1]
    C = {}
    c1 = cuts[1]
    # a group that opens in window 2 of chunk 0 and closes in window 4; groups of two and more keys everywhere else
    e = list(range(0, W + 1000, 4)) + [W + 1000, 3 * W + 500] + list(range(3 * W + 500, n, 50)) + [n]
    kinds = ["few"] * (len(set(e)) - 1)
    kinds[len(range(0, W + 1000, 4))] = "dup"                      # (one key 3596 times: the run K3u carries, too)
    C["carried_opens_in_window_2_closes_in_4"] = (_sizes_from_edges(e), kinds)
    # groups that end exactly on a window's last key, one key past it, and one key short of it
    sz = [W, W + 1, W - 1, 1, W, 1, W - 1, 2 * W, 2 * W + 1, 1, 2 * W - 1]
    C["ends_on_and_one_past_a_windows_last_key"] = (np.asarray((sz * (n // sum(sz) + 1)), np.int64), "few")
    # every later chunk's first head lies 1500 and more keys behind its nominal start: the start search iterates
    e = [0] + [x for c in cuts[1:-1] for x in (c - 10, c + 1500 + 64 * cuts.index(c))] + list(range(0, n, 700)) + [n]
    e = [x for x in e if not any(c - 10 < x < c + 1500 + 64 * cuts.index(c) for c in cuts[1:-1])]
    C["first_head_far_behind_the_nominal_start"] = (_sizes_from_edges(e), "few")
    # chunk 1 holds no head at all: one group covers it whole and chunk 0 carries on past its nominal end
    e = list(range(0, c1 - 300, 97)) + [c1 - 300, cuts[2] + 77] + list(range(cuts[2] + 77, n, 33)) + [n]
    C["a_chunk_without_a_head"] = (_sizes_from_edges(e), "few")
    # windows by turns all-distinct and all-duplicate: a set left full, then nearly empty, for the next window
    m = n // W
    C["windows_all_distinct_then_all_duplicate"] = (np.full(m, W, np.int64), ["distinct", "dup"] * (m // 2) + ["distinct"] * (m % 2))
    # a group of 5000 keys (beyond a window: the giant list of the hashed forms) in the middle window of every chunk
    e = [0, n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        mid = (a + b) // 2 // W * W + 300
        e += list(range(a, mid, 61)) + [mid, mid + 5000] + list(range(mid + 5000, b, 7))
    C["giant_group_in_the_middle_window"] = (_sizes_from_edges(e), "distinct")
    return C


STEADY = ["carried_opens_in_window_2_closes_in_4", "ends_on_and_one_past_a_windows_last_key", "first_head_far_behind_the_nominal_start",
          "a_chunk_without_a_head", "windows_all_distinct_then_all_duplicate", "giant_group_in_the_middle_window"]
# form -> (UMI bases of the engine, query family, skip_low)
K3_FORMS = {"windows": (12, "k3_windows", False), "umi_rows": (12, "k3_windows", False), "hashed32": (12, "k3_hashed", True),
            "hashed64": (14, "k3_hashed", True)}


def _case_keys(eng, lay, fam, name, shuffle, seed=1):
    cuts = _chunks(eng, fam, N_K3)
    sizes, kinds = _steady_cases(cuts)[name]
    sizes = np.asarray(sizes, np.int64)
    sizes = sizes[np.cumsum(sizes) <= N_K3]
    kinds = [kinds] * len(sizes) if isinstance(kinds, str) else kinds[:len(sizes)]
    keys = _groups_to_keys(lay, sizes, kinds, seed, shuffle)
    pad = N_K3 - len(keys)
    if pad:                                                        # (fill up with one last group)
        last = (U(1001) << U(lay.cs)) | (U(1) << U(lay.fs)) | (U(1) << U(lay.fs - 1)) | U(lay.len_full)
        keys = np.concatenate([keys, np.full(pad, last, np.uint64)])
    assert len(keys) == N_K3
    return keys


def _reduce(torch, eng, keys, skip_low):
    n = len(keys)
    d_keys = _dev(torch, keys)
    d_n = torch.tensor([n], dtype=torch.int64, device="cuda")
    out = [torch.full((n + 64,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
    d_nnz = torch.zeros(1, dtype=torch.int64, device="cuda")
    eng.dev_reduce(d_keys.data_ptr(), d_n.data_ptr(), n, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), d_nnz.data_ptr(),
                   stream=torch.cuda.current_stream().cuda_stream, skip_low=skip_low)
    torch.cuda.synchronize()
    assert eng.dev_error_bits() == 0
    nnz = int(d_nnz.item())
    got = [hostmem.to_host(t) for t in out]
    for g in got:
        assert (g[max(nnz, 0):] == -7).all()
    return nnz, [g[:nnz].astype(np.int64) for g in got]


@pytest.mark.parametrize("name", STEADY)
@pytest.mark.parametrize("form", list(K3_FORMS))
@pytest.mark.parametrize("width", WIDTHS)
def test_k3_steady_state(monkeypatch, width, form, name):
    import torch
    bases, fam, skip_low = K3_FORMS[form]
    eng = _engine(monkeypatch, width, bases=bases)
    try:
        lay = Lay(bases)
        assert eng.key_bits == lay.cs + 10 and (eng.skip_bits > 0) and (lay.fs > 27) == (form == "hashed64")
        keys = _case_keys(eng, lay, fam, name, shuffle=skip_low)
        if form == "umi_rows":
            n = len(keys)
            d_keys = _dev(torch, keys)
            d_n = torch.tensor([n], dtype=torch.int64, device="cuda")
            d_uk = torch.full((n + 64,), -7, dtype=torch.int64, device="cuda")
            d_nc = torch.full((n + 64,), -7, dtype=torch.int32, device="cuda")
            d_nr = torch.zeros(1, dtype=torch.int64, device="cuda")
            eng.dev_umi_rows(d_keys.data_ptr(), d_n.data_ptr(), n, d_uk.data_ptr(), d_nc.data_ptr(), d_nr.data_ptr(),
                             stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert eng.dev_error_bits() == 0
            uk, nc = S.umi_rows_ref(keys)
            assert int(d_nr.item()) == len(uk)
            np.testing.assert_array_equal(hostmem.to_host(d_uk).view(np.uint64)[:len(uk)], uk)
            np.testing.assert_array_equal(hostmem.to_host(d_nc)[:len(uk)].astype(np.int64), nc)
            assert (hostmem.to_host(d_nc)[len(uk):] == -7).all()
            return
        f, c, k = S.want_rows(keys, fs=lay.fs, cs=lay.cs)
        nnz, got = _reduce(torch, eng, keys, skip_low)
        assert nnz == len(f)
        np.testing.assert_array_equal(got[0], f)
        np.testing.assert_array_equal(got[1], c)
        np.testing.assert_array_equal(got[2], k)
        if skip_low:                                               # the same groups, their keys in another order: the same rows
            rev = keys[::-1]
            nnz2, got2 = _reduce(torch, eng, rev[np.argsort(rev >> U(lay.fs), kind="stable")], skip_low)
            assert nnz2 == nnz
            for a, b in zip(got, got2):
                np.testing.assert_array_equal(a, b)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# K1a on later tiles; the tile counts return to zero
# ---------------------------------------------------------------------------------------------------------------------
def _hits_case(pattern, n, wg_tiles, ck):
    """barcode keys of n records: listed in `ck` (a hit) in the 4096-record tiles the pattern names, unlisted elsewhere"""
    rng = np.random.default_rng(n)
    tile = np.arange(n) // 4096
    T = int(tile[-1]) + 1
    if pattern == "every_other_tile":
        on = tile % 2 == 1
    elif pattern == "last_tiles":                                  # every workgroup's last turn (`wg_tiles` tiles) and nothing else
        on = tile >= T - wg_tiles
    else:
        on = rng.random(n) < 0.6
    cell = rng.integers(0, 1000, size=n)
    cb = np.where(on, np.asarray(ck, np.uint64)[cell], U(0x7FFF_0000_0000_0123) + rng.integers(0, 1000, size=n).astype(np.uint64))
    return cb.astype(np.uint64), np.bincount(cell[on], minlength=1000)


@pytest.mark.parametrize("env", [{}, {"FASTF_LDS_CELLS": "0"}, {"FASTF_CELL_SCRATCH_32": "1"}], ids=["lds", "filtered", "u32_scratch"])
@pytest.mark.parametrize("pattern", ["every_other_tile", "last_tiles", "mixed"])
@pytest.mark.parametrize("width", WIDTHS)
def test_k1a_hits_on_later_tiles_and_a_second_shorter_step(monkeypatch, width, pattern, env):
    """count_hits over 150 tiles, then over 40 on the same engine: the second total is right only if the scan left the tile counts
    all zero; the cell indices of both through dev_cell_hits"""
    import torch
    from test_lookup_host import lists_of
    lists = lists_of(1000)                                         # (barcodes the LDS perfect hash takes)
    monkeypatch.setenv("FASTF_GRID_CUS", width)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = F.Engine.from_lists(lists, umi_max_bases=12)
    try:
        assert eng.table_modes.startswith("cells:L2" if "FASTF_LDS_CELLS" in env else "cells:LDS") and eng.cell_scratch_bytes == (4 if "FASTF_CELL_SCRATCH_32" in env else 2)
        assert (R_.cell_index(lists.cell_keys, lists.cell_keys) == np.arange(1, 1001)).all()      # cell c is key c - 1 of the list
        n1, n2 = 150 * 4096 - 77, 40 * 4096 + 1
        g = _trips(eng, ["k1a"], n_records=n1)
        _trips(eng, ["k1a"], n_records=n2)
        s = torch.cuda.current_stream().cuda_stream
        d_out = torch.zeros(1, dtype=torch.int64, device="cuda")
        d_per = torch.zeros(1000, dtype=torch.int32, device="cuda")
        for n in (n1, n2):
            # (a turn of the LDS form is 16 chunks of 512 records: two tiles a workgroup)
            turn_tiles = 2 if "LDS" in eng.table_modes.split(" genes:")[0] else 1
            cb, per_cell = _hits_case(pattern, n, turn_tiles * g["k1a"][0], lists.cell_keys)
            d_cb = _dev(torch, cb)
            eng.dev_count_hits(d_cb.data_ptr(), n, d_out.data_ptr(), stream=s)
            eng.dev_cell_hits(n, 0, d_per.data_ptr(), stream=s)
            torch.cuda.synchronize()
            assert int(d_out.item()) == int(per_cell.sum())
            np.testing.assert_array_equal(hostmem.to_host(d_per).astype(np.int64), per_cell)
        assert eng.dev_error_bits() == 0
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# the whole step against the oracle
# ---------------------------------------------------------------------------------------------------------------------
# c1_half with 300 k records and tile_plus_one with 72 tiles and one record (the sizes at which K1a makes three trips at width 3)
NARROW_CASES = dict(CASES, c1_half=dict(CASES["c1_half"], n=300_000), tile_plus_one=dict(CASES["tile_plus_one"], n=72 * 4096 + 1))
ENGINE_RUNS = [("c1_half", {}), ("mixed", {}), ("skewed", {}), ("tile_plus_one", {}), ("huge_groups", {}),
               ("mixed", {"FASTF_LDS_TABLES": "0"}), ("mixed", {"FASTF_LDS_CELLS": "0"}), ("mixed", {"FASTF_NO_STREAM_K1B": "1"}),
               ("mixed", {"FASTF_SORT_SKIP_BITS": "0"}), ("skewed", {"FASTF_NO_REGION_WALK": "1"})]


@pytest.mark.parametrize("name,env", ENGINE_RUNS, ids=["%s%s" % (n, "".join("-" + k[6:] + v for k, v in e.items())) for n, e in ENGINE_RUNS])
@pytest.mark.parametrize("width", WIDTHS)
def test_engine_matches_oracle_at_a_narrow_grid(monkeypatch, width, name, env):
    """push, finish and umi_rows.  The sort's cap at its floor of 8 workgroups and one K3 workgroup per CU, so that the keys that
    survive (25 to 100 % of the records) still make three trips; claimed per run: the K1a and K1b forms it launches, the sort
    tiles, the K3 form of its matrix rows with five windows a chunk, and reduce_windows_kernel<true> of umi_rows"""
    monkeypatch.setenv("FASTF_GRID_CUS", width)
    monkeypatch.setenv("FASTF_TILE_GRID_CAP", "8")
    monkeypatch.setenv("FASTF_K3_PER_CU", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    case = Case(**NARROW_CASES[name])
    ora = case.oracle()
    lists = case.lists()
    eng = F.Engine.from_lists(lists, rate_depth=case.rate_depth, seed=case.seed, umi_max_bases=12)
    try:
        n_keys = int(ora["valid"])
        lds = env.get("FASTF_LDS_TABLES") != "0"              # (without: probe_cells_kernel and filter_pack_kernel<false>, a workgroup per tile)
        stream = lds and "FASTF_NO_STREAM_K1B" not in env
        fams = ["draw_bits", "sort_tiles"] + (["k1a"] if lds else []) + (["k1b_stream", "block_records"] if stream else ["k1b_tiles"] if lds else [])
        _trips(eng, fams, n_records=case.n, n_keys=n_keys)
        _chunks(eng, "k3_hashed" if eng.skip_bits else "k3_windows", n_keys)
        _chunks(eng, "k3_windows", n_keys)
        assert (eng.skip_bits == 0) == ("FASTF_SORT_SKIP_BITS" in env)
        eng.push(*case.packed(lists))
        assert_matches_oracle(eng.finish(), ora, eng, case, lists, eng.umi_rows())
    finally:
        eng.close()


@pytest.mark.parametrize("width", WIDTHS)
def test_wide_keys_match_oracle_at_a_narrow_grid(monkeypatch, width):
    """scatter_kernel<-1, false, true> (values beside the keys), reduce_hashed_kernel<true, true>, the pair kernels"""
    monkeypatch.setenv("FASTF_GRID_CUS", width)
    kw, umi_max, bits = WIDE_CASES["200k barcodes x 70k genes, 16-base UMIs"]
    case = Case(**kw)
    ora = case.oracle()
    lists = case.lists()
    eng = F.Engine.from_lists(lists, rate_depth=case.rate_depth, seed=case.seed, umi_max_bases=umi_max)
    try:
        assert eng.key_bits == bits > 64
        n_keys = int(ora["valid"])
        # (the pair kernels' 2048-key tiles: three trips at width 1 only — 16 workgroups per CU)
        _trips(eng, ["sort_tiles", "pairs"] if width == "1" else ["sort_tiles"], n_keys=n_keys)
        _chunks(eng, "k3_hashed", n_keys)
        eng.push(*case.packed(lists))
        assert_matches_oracle(eng.finish(), ora, eng, case, lists, eng.umi_rows())
    finally:
        eng.close()


@pytest.mark.parametrize("width", WIDTHS)
def test_20_base_umis_match_oracle_at_a_narrow_grid(monkeypatch, width):
    monkeypatch.setenv("FASTF_GRID_CUS", width)
    case = Case(umi_len=20, n=200_000, n_bar=2000, n_gene=900, rate_cell=0.7, rate_depth=0.8, dup_factor=3.0, p_no_cb=0.03,
                p_unlisted_cb=0.05, p_bad_xf=0.1, p_n_umi=0.02)
    ora = case.oracle()
    lists = case.lists()
    monkeypatch.setenv("FASTF_TILE_GRID_CAP", "8")
    eng = F.Engine.from_lists(lists, rate_depth=case.rate_depth, seed=case.seed, umi_max_bases=24)
    try:
        assert eng.wide
        n_keys = int(ora["valid"])
        _trips(eng, ["k1a", "k1b_tiles", "draw_bits", "sort_tiles"], n_records=case.n, n_keys=n_keys)   # (wide keys take the tile K1b)
        _chunks(eng, "k3_hashed", n_keys)
        cb, gx, umi, meta, ext = case.packed_long(lists)
        assert ext.any()
        eng.push(cb, gx, umi, meta, umi_ext=ext)
        assert_matches_oracle(eng.finish(), ora, eng, case, lists, eng.umi_rows())
    finally:
        eng.close()


def _resident_pass(case, forms, claimed, steps=2):
    """tests/test_gpu_parity.py's resident pass: K1a, the streaming (or tile) K1b, the region sort, K3 through ShardedPass"""
    import torch
    from fastf_amd.dist import HipStages, ShardedPass
    ora = case.oracle()
    lists = case.lists()
    cbk, gxk, umi, meta = case.packed(lists)
    dev = torch.device("cuda", 0)
    d = [hostmem.to_device(x, dev) for x in (cbk, gxk, umi, meta)]
    draws = hostmem.to_device(F.mt_draws(case.seed, lists.mt_skip, case.n), dev)
    for form in forms:
        eng = F.Engine.from_lists(lists, rate_depth=case.rate_depth, seed=case.seed, umi_max_bases=12)
        try:
            _trips(eng, claimed, n_records=case.n)
            st = HipStages(eng, dev)
            sp = ShardedPass(st, case.n, dev)
            blk = st.block(d[1], d[2], d[3], case.n) if form == "blocked" else None
            assert (blk is not None) == (form == "blocked")
            dr = sp.prepare_draws(draws)
            for _ in range(steps):
                if blk is not None:
                    sp.run(d[0], blk, None, None, case.n, dr)
                else:
                    sp.run(d[0], d[1], d[2], d[3], case.n, dr)
            f, c, k = sp.local_coo()
            hits, sampled, valid, err = sp.global_counters()
            assert err == 0 and sp.st.segmented
            assert (sampled, valid) == (ora["sampled"], ora["valid"])
            np.testing.assert_array_equal(c, ora["cell"].astype(np.int64))
            np.testing.assert_array_equal(f, ora["feature"].astype(np.int64))
            np.testing.assert_array_equal(k, ora["count"].astype(np.int64))
        finally:
            eng.close()


@pytest.mark.parametrize("name", ["c3 shape", "u32 cell scratch"])
@pytest.mark.parametrize("width", WIDTHS)
def test_resident_pass_at_a_narrow_grid(monkeypatch, width, name):
    """(scatter_regions_kernel walks the regions the streaming K1b leaves, two per workgroup of it: at a narrow grid that is a few
    regions of many sort tiles each — its inner loop goes round, not its outer one)"""
    monkeypatch.setenv("FASTF_GRID_CUS", width)
    _resident_pass(Case(**STREAM_CASES[name]), ("blocked", "soa"), ["k1a", "k1b_stream", "block_records"])


# around a unit (256), a tile (4096) and a round of a 12-wave workgroup, as tests/test_gpu_parity.py has them; the last three make
# three and more trips at both widths
@pytest.mark.parametrize("n", [257, 4097, 12 * 256 + 1, 16 * 4096 + 1, 36 * 12 * 256 - 1, 36 * 12 * 256 + 1, 40 * 4096 + 257])
@pytest.mark.parametrize("width", WIDTHS)
def test_streaming_k1b_record_counts_at_a_narrow_grid(monkeypatch, width, n):
    monkeypatch.setenv("FASTF_GRID_CUS", width)
    _resident_pass(Case(n=n, n_bar=64, n_gene=40, rate_depth=0.5, umi_pool=16, p_no_cb=0.0, p_unlisted_cb=0.0), ("blocked", "soa"),
                   ["k1b_stream"] if n >= 100_000 else [])


# ---------------------------------------------------------------------------------------------------------------------
# K1b on later tiles: which hit ranks are kept (tests/k1b_ref.py), two steps on one engine
# ---------------------------------------------------------------------------------------------------------------------
K1B_N = 40 * 4096 + 257                  # 41 tiles (21 pairs: three trips of six LDS workgroups), 642 units


@pytest.mark.parametrize("form", ["stream blocked narrow", "stream SoA", "stream, 32-bit cell scratch", "tile, LDS genes, direct table"])
@pytest.mark.parametrize("width", WIDTHS)
def test_k1b_keeps_the_right_hit_ranks_on_later_tiles_and_in_a_second_shorter_step(monkeypatch, width, form):
    """tests/test_gpu_k1b_gating.py's rig on 164 097 records built as k1b_ref builds them (every non-NULL UMI names its record, so the
    keys say which hit ranks were kept): hits in every other unit against a random decision stream, then — fewer tiles, same engine —
    hits from the second tile on against a stream with one decision set per word.  A tile base, a unit's rank base or a tile count
    that is wrong or stale on a later tile keeps other records."""
    import k1b_ref as K
    import lookup_ref as R
    import test_gpu_k1b_gating as TG
    monkeypatch.setenv("FASTF_GRID_CUS", width)
    rig = TG.Rig(monkeypatch, form)
    try:
        eng = rig.eng
        _trips(eng, ["k1a", "k1b_tiles" if rig.call == "tile" else "k1b_stream"] + (["block_records"] if rig.call == "blocked" else []),
               n_records=37 * 4096 + 1)
        # the same records, more of them (the rig's own stop at 40 001)
        unl = np.concatenate([np.zeros(1, np.uint64), R.pack_gx(rig.lists, R.id_strings(b"ENSG", 11, [1000 + o for o in (97, 190, 224, 319)]))]).astype(np.uint64)
        rig.gx, rig.umi, rig.meta, rig.ext, rig.cell_if_hit = K.build_records(TG.N_CELLS_K1B, rig.lists.feature_keys, unl, n=K1B_N, blob_bytes=rig.blob)
        rig.feat = R.gene_lookup(rig.lists.feature_keys, rig.gx)
        rig.d_gx, rig.d_umi, rig.d_meta = (hostmem.to_device(a, "cuda") for a in (rig.gx, rig.umi, rig.meta))
        for n, hits, bits, base in ((K1B_N, "alt_empty_full", "random", 33), (37 * 4096 + 1, "tile0_empty", "one_set", 1_000_003)):
            fx = K.Fixture(n, hits, bits, base)
            mask, stream, nd = fx.mask(), fx.stream(), fx.n_draws()
            want = rig.want(n, mask, stream, base, nd)
            assert want.err == 0 and 1000 < sum(len(k) for k in want.keys) < int(mask.sum())
            got = rig.run(n, rig.cb(mask), rig.bits_on_device(stream), nd, base)
            rig.check(got, want, fx.name)
            assert got[3][3] == 0 and eng.dev_error_bits() == 0
    finally:
        rig.close()


@pytest.mark.parametrize("name,n_cells,env,lds,per_cu,csb", [c for c in __import__("test_gpu_lookup").K1A_CASES
                                                             if c[0] in ("lds two per CU", "lds one per CU", "filter + L2", "32-bit scratch by necessity")],
                         ids=["lds2", "lds1", "filter", "u32"])
@pytest.mark.parametrize("width", WIDTHS)
def test_k1a_cell_index_of_near_miss_keys_on_later_tiles(monkeypatch, width, name, n_cells, env, lds, per_cu, csb):
    """tests/lookup_ref.py's near-miss barcodes (slot twins, low-word twins, family and low-16 near misses, filter passers, L2 chains)
    through tests/test_gpu_lookup.py's runner, the stream repeated to 150 tiles: the cell index of every record, blocked and SoA"""
    import torch
    import lookup_ref as R
    import test_gpu_lookup as TL
    lists = TL.lists_of(n_cells)
    ck = lists.cell_keys
    monkeypatch.setenv("FASTF_GRID_CUS", width)
    eng = TL._engine(monkeypatch, lists, env)
    try:
        n = 150 * 4096 - 77
        _trips(eng, ["k1a", "block_records"], n_records=n)
        assert eng.cell_scratch_bytes == csb
        img, p = TL.cell_image(ck)
        table = None if lds else R.l2_table(ck)
        filt = None if lds or "FASTF_NO_CELL_FILTER" in env else R.filter_bits(ck)
        rng = np.random.default_rng(n_cells)
        sets = R.cb_near_misses(lists, img, p, rng, table, filt)
        cb = np.resize(TL._k1a_streams(ck, sets, rng)[-1], n)
        TL._k1a_run(torch, eng, n_cells, csb, cb, R.cell_index(ck, cb), False)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# reduce_hashed_kernel<true, true> in its steady state: built (group word, value) pairs through adopt + finish
# ---------------------------------------------------------------------------------------------------------------------
def _wide_pairs_of(lay, sizes, kinds, seed):
    """pairs of S.WideLayout with the given group sizes, group words ascending, kinds as _groups_to_keys has them"""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, np.int64)
    ids = np.sort(rng.choice(1000 * 500, size=len(sizes), replace=False))
    gw = ((ids // 500 + 1).astype(np.uint64) << U(9)) | (ids % 500 + 1).astype(np.uint64)
    vs = []
    for sz, kind in zip(sizes.tolist(), kinds):
        if kind == "distinct":
            v = lay.value(rng.choice(1 << 40, size=sz, replace=False).astype(np.uint64))
        elif kind == "dup":
            v = lay.value(np.full(sz, 0x12_3456_789A, np.uint64))
        else:
            v = np.where(rng.random(sz) < 0.1, U(0), lay.value(rng.integers(0, 5, size=sz, dtype=np.uint64) * U(0x1_0000_0301)))
        vs.append(v.astype(np.uint64))
    return np.repeat(gw, sizes), np.concatenate(vs)


@pytest.mark.parametrize("name", STEADY)
@pytest.mark.parametrize("width", WIDTHS)
def test_k3_steady_state_of_wide_keys(monkeypatch, width, name):
    """the cases of test_k3_steady_state on a 24-base engine: the pairs go up sorted by group word (the engine's stable sort keeps
    them where they are), so every group sits against the chunk edges of reduce_hashed_kernel<true, true> as built; the matrix rows
    and the -u rows (the pair kernels, the sort with values) against S.wide_rows_ref"""
    import torch
    import test_gpu_wide_pairs as TW
    monkeypatch.setenv("FASTF_GRID_CUS", width)
    eng = F.Engine(CELLS, FEATS, umi_max_bases=24)
    try:
        assert eng.wide
        lay = S.WideLayout(24)
        _trips(eng, ["sort_tiles", "pairs"] if width == "1" else ["sort_tiles"], n_keys=N_K3)     # (pairs: 16 workgroups per CU)
        cuts = _chunks(eng, "k3_hashed", N_K3)
        sizes, kinds = _steady_cases(cuts)[name]
        sizes = np.asarray(sizes, np.int64)
        sizes = sizes[np.cumsum(sizes) <= N_K3]
        kinds = [kinds] * len(sizes) if isinstance(kinds, str) else kinds[:len(sizes)]
        if int(sizes.sum()) < N_K3:
            sizes, kinds = np.append(sizes, N_K3 - int(sizes.sum())), kinds + ["few"]
        k, v = _wide_pairs_of(lay, sizes, kinds, 3)
        assert len(k) == N_K3
        TW._check(torch, eng, lay, k, v)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# rgn_hist_kernel and the outer loop of scatter_regions_kernel: a push after finish, 24 regions of 65 536 keys on 8 workgroups
# ---------------------------------------------------------------------------------------------------------------------
def test_push_after_finish_walks_24_rebased_regions_on_8_workgroups(monkeypatch):
    """tests/test_gpu_parity.py's push after finish at width 1 with the tile cap at its floor: the 1.56 M keys of the first finish
    become 24 regions (rebase_store), rgn_hist_kernel counts them on 8 workgroups, and the next sort's first pass
    (scatter_regions_kernel, 8 workgroups) walks them and the new chunk's regions: three trips of both outer loops"""
    monkeypatch.setenv("FASTF_GRID_CUS", "1")
    monkeypatch.setenv("FASTF_TILE_GRID_CAP", "8")
    case = Case(n=1_600_000, n_bar=2000, n_gene=900, umi_pool=512)
    ora = case.oracle()
    lists = case.lists()
    eng = F.Engine.from_lists(lists, rate_depth=case.rate_depth, seed=case.seed)
    try:
        packed = case.packed(lists)
        a = 1_560_000
        eng.push(*(x[:a] for x in packed))
        first = eng.finish()
        n_keys = int(first["valid"])
        g = _trips(eng, ["rgn_hist"], n_keys=n_keys)
        R_ = g["rgn_hist"][1]
        assert R_ >= 24 and eng.grids(0, 65536 * 8)["sort_tiles"][0] == 8          # scatter_regions: tile_grid(R) = 8 for R regions and more
        eng.push(*(x[a:] for x in packed))
        res = eng.finish()
        assert_matches_oracle(res, ora, eng, case, lists, eng.umi_rows())
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# the analysis kernels: one pass at width 1, the fixtures and references of their own modules
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def narrow100(monkeypatch):
    """the 100 x 50 engine of the analysis modules at width 1 (their spans are cut from gridDim: many turns per wave)"""
    monkeypatch.setenv("FASTF_GRID_CUS", "1")
    eng = F.Engine(np.arange(1, 101, dtype=np.uint64) | (U(1) << U(62)), np.arange(1, 51, dtype=np.uint64) | (U(2) << U(62)), umi_max_bases=12)
    assert eng.grids(0, 1 << 20)["giant"][0] == 2
    yield eng
    eng.close()


def test_cell_summary_at_width_1(narrow100):
    import torch
    import test_gpu_sweep as T
    for name in ("a_cell_of_200000_rows", "cells_65536", "every_cell_one_row", "cells_1"):
        T.test_cell_summary_against_numpy((torch, [narrow100]), name)


def test_copy_summary_at_width_1(monkeypatch):
    """tests/cells_ref.py's fixtures built for a launch of one CU, through tests/test_gpu_cells.py's checker"""
    import torch
    import test_gpu_cells as T
    monkeypatch.setenv("FASTF_GRID_CUS", "1")
    small = F.Engine(CELLS, FEATS, umi_max_bases=12)
    big = F.Engine(np.arange(1, 70_001, dtype=np.uint64) | (U(1) << U(62)), FEATS, umi_max_bases=12)
    import cells_ref as R
    try:
        for name in R.fixture_names(1):                           # (lane63 places cells on turn 100 of a wave: built for 16 CUs' waves)
            keys, k, n_cells = R.fixture(name, 16 if name == "lane63" else 1)
            lay = R.layout_of(name)
            want = R.from_keys(keys, k, n_cells, lay)
            d_uk = _dev(torch, np.concatenate([keys, np.full(R.PAD, (3 << lay.cs) | (1 << (lay.fs - 1)), np.uint64)]))
            d_nc = _dev(torch, np.concatenate([k, np.full(R.PAD, 9, np.uint32)]))
            d_n = _dev(torch, np.array([len(keys)], np.uint64))
            T._summary(torch, big if lay is R.BIG else small, d_uk.data_ptr(), d_nc.data_ptr(), d_n.data_ptr(), n_cells, want, name)
    finally:
        small.close(); big.close()


def test_fidelity_at_width_1(narrow100):
    import test_gpu_fidelity as T
    for which in (3, 7, 10):
        T.test_the_join_at_the_sizes_where_the_path_changes(narrow100, which)
    T.test_one_cell_owning_every_row_over_several_spans(narrow100)
    T.test_a_window_of_full_rows_much_larger_than_the_span(narrow100)


def test_partner_counts_and_gene_moments_at_width_1(narrow100, monkeypatch):
    import test_gpu_gene_fidelity as T
    for name in ("rows5", "rows10", "every50", "one_cell"):
        T.test_partner_counts(narrow100, name)
    for form in ("lds", "general"):
        for name in ("list36601", "big", "rows65"):
            T.test_gene_moments(narrow100, name, form, monkeypatch)


def test_gene_summary_at_width_1(narrow100, monkeypatch):
    import torch
    import test_gpu_genes as T
    for lds_ranges in (None, "0"):
        for n_features in (16385, 36601):
            T.test_gene_summary_against_numpy((torch, narrow100), n_features, lds_ranges, monkeypatch)
        monkeypatch.delenv("FASTF_GENES_LDS_RANGES", raising=False)


def test_cell_hits_and_decisions_at_width_1(monkeypatch):
    import test_gpu_cap as T
    monkeypatch.setenv("FASTF_GRID_CUS", "1")
    monkeypatch.delenv("FASTF_BLOCK_WIDE", raising=False)
    T.test_cell_hits_against_bincount("narrow", 50_000, None, monkeypatch)
    T.test_cell_hits_against_bincount("soa", 70_000, "0", monkeypatch)
    monkeypatch.delenv("FASTF_CAP_LDS_RANGES", raising=False)
    T.test_cell_decisions_against_the_stream_below_each_cells_threshold("narrow", 3)


def test_level_step_at_width_1(narrow100):
    import test_gpu_level as T
    for n_cells in (65, 70_000):
        T.test_init_against_the_twin(narrow100, n_cells)
        T.test_a_whole_search_finds_the_m_plus_first_birth(narrow100, n_cells)


def test_label_votes_and_marker_auc_at_width_1(narrow100, monkeypatch):
    import test_gpu_labels as TL
    import test_gpu_markers as TM
    for form in TL.FORMS:
        TL.test_votes_against_the_reference(narrow100, 1000, 15, 30, form, monkeypatch)
        TL.test_votes_against_the_reference(narrow100, 65, 64, 7, form, monkeypatch)
    for form in TM.FORMS:
        for P in (1, 2):
            TM.test_tables_against_the_reference(narrow100, 257, 33, 128, P, form, monkeypatch)
            TM.test_tables_against_the_reference(narrow100, 129, 500, 3, P, form, monkeypatch)
