"""--neighbors on the host: the host twin (fastf_neighbors_from_coo) against neighbors_ref on random and hand-built matrices whose ties
straddle the cut at k, the factored-out ranking of the highly variable genes against gene_fidelity_ref, the rows, headers and NA rules
of both files, the 2^42 refusal, flag 512 beside the refused bits, the help texts and refusals — and the fixtures the device tests
(test_gpu_neighbors) run, with a census of what they cover."""
import math
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, cap, level, sweep, synth
import gene_fidelity_ref as G
import neighbors_ref as N


# ---- fixtures: name -> (rows (feature, cell, count) ascending by (cell, feature), n_cells, n_features, genes of A in slot order, k) ----
def rows_of_dense(m, genes, n_features, outside=None):
    """the rows of a dense n x len(genes) matrix laid on the features genes[s] + 1; outside: extra (cell0, gene0, count) rows on other features"""
    cells, feats, counts = [], [], []
    for c in range(m.shape[0]):
        for s in range(m.shape[1]):
            if m[c, s]:
                cells.append(c + 1); feats.append(int(genes[s]) + 1); counts.append(int(m[c, s]))
    for c, g, v in outside or []:
        assert g not in set(int(x) for x in genes)
        cells.append(c + 1); feats.append(g + 1); counts.append(v)
    o = np.lexsort((feats, cells))
    return tuple(np.asarray(a, np.uint32)[o] for a in (feats, cells, counts))


def random_fixture(n, K, k, seed, max_count=4, density=0.3, plant=None):
    rng = np.random.default_rng(seed)
    n_features = K + 7
    genes = rng.permutation(n_features)[:K]                 # slots are not in feature order, seven features stay outside A
    m = (rng.integers(1, max_count + 1, (n, K)) * (rng.random((n, K)) < density)).astype(np.int64)
    if plant is not None and n:                             # one count at a plane edge; its cell stays below a norm of 2^42
        c = n // 2
        m[c, :] = 0
        m[c, K // 2] = plant
        m[c, 0] += 3
    others = [g for g in range(n_features) if g not in set(genes.tolist())]
    outside = [(int(rng.integers(0, n)), others[int(rng.integers(0, len(others)))], 1 << 20) for _ in range(min(n, 5))] if n else []
    outside = list({(c, g): (c, g, v) for c, g, v in outside}.values())
    return rows_of_dense(m, genes, n_features, outside), n, n_features, genes, k


def scaled_pair():
    """v and 3v have the same cosine to every third cell; in doubles the two cosines to q differ in the last bit.  The one whose double is
    larger gets the HIGHER index, so a float comparison picks it and the exact order picks the other"""
    rng = np.random.default_rng(5)
    for _ in range(10_000):
        q, v = rng.integers(1, 40, 6), rng.integers(1, 40, 6)
        d, nq, nv = int(q @ v), int(q @ q), int(v @ v)
        c1, c3 = d / math.sqrt(nq * nv), (3 * d) / math.sqrt(nq * 9 * nv)
        if c1 != c3:
            return q, v, c1, c3
    raise AssertionError("no pair found")


def tie_fixture(name):
    K = 6
    genes = np.array([4, 0, 5, 2, 1, 3])
    if name == "duplicates":                                # k = 3: cell 1 is closest to cell 0, then five equal cells: the two lowest indices enter
        m = np.array([[1, 1, 0, 0, 0, 0], [2, 2, 0, 0, 0, 0]] + [[1, 0, 0, 0, 0, 0]] * 5 + [[0, 0, 0, 7, 0, 0]], np.int64)
        return rows_of_dense(m, genes, K), len(m), K, genes, 3
    if name == "scaled":                                    # k = 2: one closer cell, then v against 3v for the last slot
        q, v, c1, c3 = scaled_pair()
        lo, hi = (v, 3 * v) if c3 > c1 else (3 * v, v)      # hi: the larger double, at the higher index
        m = np.array([q, 2 * q, lo, hi, [0, 0, 0, 0, 0, 1]], np.int64)
        return rows_of_dense(m, genes, K), len(m), K, genes, 2
    if name == "all_identical":
        m = np.array([[3, 0, 1, 0, 2, 0]] * 40, np.int64)
        return rows_of_dense(m, genes, K), len(m), K, genes, 15
    if name == "zero_and_outside":                          # cell 2 has no count at all, cell 3 counts only outside A
        m = np.array([[1, 2, 0, 0, 0, 0], [0, 2, 1, 0, 0, 0], [0] * 6, [0] * 6, [1, 0, 0, 0, 0, 3]], np.int64)
        g8 = np.array([4, 0, 5, 2, 1, 3])
        return rows_of_dense(m, g8, 8, [(3, 6, 9), (3, 7, 2), (0, 7, 5)]), len(m), 8, g8, 15
    if name == "all_zero":
        return rows_of_dense(np.zeros((9, K), np.int64), genes, K + 1, [(c, K, 4) for c in range(9)]), 9, K + 1, genes, 15
    if name == "no_rows":
        z = np.zeros(0, np.uint32)
        return (z, z, z), 5, K, genes, 15
    raise KeyError(name)


TIE_FIXTURES = ("duplicates", "scaled", "all_identical", "zero_and_outside", "all_zero", "no_rows")
N_SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 129, 257)         # around the wave's 32 rows, two tiles, the workgroup's 128 rows, two workgroups
K_SIZES = (1, 31, 32, 33, 63, 64, 65, 2000)                 # around the MFMA's K step of 32 bytes
PLANE_EDGES = (127, 128, 16383, 16384, (1 << 21) - 1)
DEVICE_FIXTURES = {}
for _n in N_SIZES:
    DEVICE_FIXTURES["n%d" % _n] = (lambda n=_n: random_fixture(n, 33, 15, 100 + n))
for _K in K_SIZES:
    DEVICE_FIXTURES["K%d" % _K] = (lambda K=_K: random_fixture(65, K, 15, 200 + K, density=0.3 if K < 100 else 0.02))
for _k in (1, 64):
    DEVICE_FIXTURES["k%d" % _k] = (lambda k=_k: random_fixture(129, 64, k, 300 + k))
for _c in PLANE_EDGES:
    DEVICE_FIXTURES["count%d" % _c] = (lambda c=_c: random_fixture(33, 33, 15, 400 + c % 97, plant=c))
DEVICE_FIXTURES["three_planes_dense"] = lambda: random_fixture(40, 40, 15, 500, max_count=40_000, density=0.5)
for _t in TIE_FIXTURES:
    DEVICE_FIXTURES[_t] = (lambda t=_t: tie_fixture(t))
_BUILT, _REFS = {}, {}


def fixture(name):
    if name not in _BUILT:
        _BUILT[name] = DEVICE_FIXTURES[name]()
    return _BUILT[name]


def reference(name):
    """computed once, shared by the host and the device tests"""
    if name not in _REFS:
        rows, n, nf, genes, k = fixture(name)
        _REFS[name] = N.neighbor_sets(rows, n, genes, k)
    return _REFS[name]


def planes_needed(name):
    rows, n, nf, genes, k = fixture(name)
    inside = np.isin(rows[0].astype(np.int64) - 1, genes)
    top = int(rows[2][inside].max()) if inside.any() else 0
    return 1 if top < 128 else 2 if top < 16384 else 3


def as_lists(idx, cnt):
    return [[int(v) for v in idx[i, :cnt[i]]] for i in range(len(cnt))]


def test_census_of_the_device_fixtures():
    assert {fixture("n%d" % n)[1] for n in N_SIZES} == set(N_SIZES)
    assert {len(fixture("K%d" % K)[3]) for K in K_SIZES} == set(K_SIZES)
    assert {fixture(n)[4] for n in DEVICE_FIXTURES} >= {1, 2, 3, 15, 64}
    assert [planes_needed("count%d" % c) for c in PLANE_EDGES] == [1, 2, 2, 3, 3] and planes_needed("three_planes_dense") == 3
    assert planes_needed("n257") == 1 and planes_needed("all_zero") == 1       # (the counts of 2^20 outside A do not count)
    for name in DEVICE_FIXTURES:
        rows, n, nf, genes, k = fixture(name)
        key = rows[1].astype(np.int64) << 32 | rows[0].astype(np.int64)
        assert (key[1:] > key[:-1]).all(), name
        sets, norms = reference(name)
        assert max(norms, default=0) < 1 << 42, name
    sets, _ = reference("n257")
    assert min(len(s) for s in sets) == 15                  # the lists are full: the cut is exercised
    assert max(len(s) for s in reference("k64")[0]) == 64
    assert max(reference("count%d" % PLANE_EDGES[-1])[1]) > 1 << 41


@pytest.mark.parametrize("name", sorted(DEVICE_FIXTURES))
def test_the_host_twin_against_the_reference(name):
    rows, n, nf, genes, k = fixture(name)
    sets, norms = reference(name)
    idx, cnt, nn = sweep.neighbors_from_coo(rows, n, sweep.neighbors_slot_map(genes, nf), k)
    assert as_lists(idx, cnt) == sets and [int(v) for v in nn] == norms
    assert all((idx[i, cnt[i]:] == N.NONE).all() for i in range(n))
    o = np.random.default_rng(1).permutation(len(rows[0]))   # the rows in any order
    idx2, cnt2, _ = sweep.neighbors_from_coo(tuple(a[o] for a in rows), n, sweep.neighbors_slot_map(genes, nf), k)
    assert (idx2 == idx).all() and (cnt2 == cnt).all()


def test_the_ties_straddle_the_cut():
    sets, _ = reference("duplicates")
    assert sets[0] == [1, 2, 3]                             # a reversed index rule gives [1, 5, 6]
    assert sets[7] == []                                    # nothing in common with anybody
    q, v, c1, c3 = scaled_pair()
    assert c1 != c3 and abs(c1 - c3) <= 2 * math.ulp(c1)    # equal cosines whose doubles differ in the last bit
    sets, norms = reference("scaled")
    assert sets[0] == [1, 2]                                # the exact tie goes to the lower index; the larger double sits at index 3
    rows, n, nf, genes, k = fixture("scaled")
    m = N.dense(rows, n, genes)
    d = lambda i, j: int(m[i].dot(m[j]))                    # noqa: E731
    assert d(0, 2) ** 2 * norms[3] == d(0, 3) ** 2 * norms[2]
    assert d(0, 3) / math.sqrt(norms[0] * norms[3]) > d(0, 2) / math.sqrt(norms[0] * norms[2])
    sets, _ = reference("all_identical")
    assert sets[0] == list(range(1, 16)) and sets[39] == list(range(15)) and sets[20] == [j for j in range(16) if j != 20][:15]
    sets, _ = reference("zero_and_outside")
    assert sets[2] == [] and sets[3] == [] and all(2 not in s and 3 not in s for s in sets) and sets[0] == [1, 4]
    assert reference("all_zero")[0] == [[]] * 9 and reference("no_rows")[0] == [[]] * 5


@pytest.mark.parametrize("n_genes", [1, 3, 2001])
def test_the_ranking_of_a_and_k_genes(n_genes):
    """fastf_hvg_rank against gene_fidelity_ref.hvg, and the twin on the A it gives: 1, 3 and 2001 eligible genes (2000 enter)"""
    rng = np.random.default_rng(n_genes)
    n = 12
    m = (rng.integers(1, 5, (n, n_genes)) * (rng.random((n, n_genes)) < 0.6)).astype(np.int64)
    m[0, :] = 1
    m[:, : min(3, n_genes)] = np.arange(1, n + 1)[:, None]   # (equal dispersions: the index rule ranks them)
    rows = rows_of_dense(m, np.arange(n_genes), n_genes)
    want = N.hvg_of_rows(rows, n, n_genes)
    sx, sxx = m.sum(0).astype(np.uint64), (m * m).sum(0).astype(np.uint64)
    genes, n_defined = sweep.hvg_rank(n, sx, sxx)
    assert [int(g) for g in genes] == want and n_defined == n_genes and len(genes) == min(n_genes, 2000)
    idx, cnt, _ = sweep.neighbors_from_coo(rows, n, sweep.neighbors_slot_map(genes, n_genes), 4)
    assert as_lists(idx, cnt) == N.neighbor_sets(rows, n, want, 4)[0]
    g1, nd1 = sweep.hvg_rank(1, sx, sxx)                    # n < 2: no dispersion is defined
    assert len(g1) == 0 and nd1 == 0


def test_the_slot_map_and_the_padding():
    sm = sweep.neighbors_slot_map([3, 0], 5)
    assert sm.tolist() == [0xFFFF, 1, 0xFFFF, 0xFFFF, 0, 0xFFFF]
    for bad in ([5], [1, 1]):
        with pytest.raises(F.FastfError, match="outside the list or named twice"):
            sweep.neighbors_slot_map(bad, 5)
    with pytest.raises(F.FastfError, match="at most 2000"):
        sweep.neighbors_slot_map(list(range(2001)), 3000)
    assert sweep.neighbors_pad(1, 1) == (128, 32) and sweep.neighbors_pad(128, 32) == (128, 32) and sweep.neighbors_pad(129, 33) == (256, 64)
    assert sweep.neighbors_pad(0, 0) == (128, 32) and sweep.neighbors_pad(50_000, 2000) == (50_048, 2016)
    L = _lib.lib()
    a, b = np.array([1, 4, 9], np.uint32), np.array([0, 4, 5, 9, 11], np.uint32)
    assert L.fastf_neighbors_shared(a.ctypes.data, 3, b.ctypes.data, 5) == 2 and L.fastf_neighbors_shared(a.ctypes.data, 0, b.ctypes.data, 5) == 0


def test_the_range_rule():
    sweep.neighbors_check_norm((1 << 42) - 1)
    for v in (1 << 42, (1 << 64) - 1):
        with pytest.raises(F.FastfError, match="FASTF_ERR_NEIGHBOR_NORM"):
            sweep.neighbors_check_norm(v)
    genes = np.array([0, 1])
    ok = rows_of_dense(np.array([[(1 << 21) - 1, 2047], [1, 1]], np.int64), genes, 2)
    idx, cnt, nn = sweep.neighbors_from_coo(ok, 2, sweep.neighbors_slot_map(genes, 2), 1)
    assert int(nn[0]) == ((1 << 21) - 1) ** 2 + 2047 ** 2 < 1 << 42 and as_lists(idx, cnt) == [[1], [0]]
    bad = rows_of_dense(np.array([[1 << 21, 0], [1, 1]], np.int64), genes, 2)
    with pytest.raises(F.FastfError, match="FASTF_ERR_NEIGHBOR_NORM"):
        sweep.neighbors_from_coo(bad, 2, sweep.neighbors_slot_map(genes, 2), 1)
    for k in (0, 65):
        with pytest.raises(F.FastfError, match="from 1 to 64"):
            sweep.neighbors_from_coo(ok, 2, sweep.neighbors_slot_map(genes, 2), k)


def test_headers_rows_and_the_na_rules():
    assert sweep.neighbors_header() == "\t".join(sweep.POINT_NEIGHBORS_COLUMNS) + "\n"
    for mod, verb in ((sweep, "sweep"), (cap, "cap"), (level, "level")):
        assert mod.neighbors_header(verb) == "\t".join(mod.NEIGHBORS_COLUMNS) + "\n" and mod.NEIGHBORS == 512
    assert cap.NEIGHBORS_COLUMNS[1] == "reads_per_cell" and level.NEIGHBORS_COLUMNS[1] == "umi_cap" and sweep.NEIGHBORS_COLUMNS[1] == "rate_depth"
    assert sweep.neighbors_row("AAAC-1", 15, 14, 5) == "AAAC-1\t15\t14\t5\t0.333333\n"
    assert sweep.neighbors_row("AAAC-1", 0, 0, 0) == "AAAC-1\t0\t0\t0\tNA\n"
    assert sweep.neighbors_row("x", 3, 0, 0) == "x\t3\t0\t0\t0.000000\n"
    rng = np.random.default_rng(3)
    for n in (1, 2, 10, 11, 40):
        kf = rng.integers(0, 16, n); kf[0] = 7
        kp = np.minimum(kf, rng.integers(0, 16, n))
        sh = np.minimum(kp, rng.integers(0, 16, n))
        want = N.summary_fields(["0.500", "0.250"], 926, 33, 15, kf.tolist(), kp.tolist(), sh.tolist())
        got = sweep.neighbors_summary_row(0.5, 0.25, 926, 33, kf, kp, sh)
        assert got.endswith("\n")
        N.assert_fields(got[:-1].split("\t"), want, 7)
        assert cap.neighbors_summary_row(0.5, 40, 926, 33, kf, kp, sh).split("\t")[:3] == ["0.500", "40", "926"]
        assert level.neighbors_summary_row(0.5, 7, 5, 33, kf, kp, sh).split("\t")[:3] == ["0.500", "7", "5"]
    z = np.zeros(4, np.uint32)
    assert sweep.neighbors_summary_row(1, 1, 1, 0, z, z, z) == "1.000\t1.000\t1\t4\t0\t15\t0\tNA\tNA\tNA\t0.000000\n"
    e = np.zeros(0, np.uint32)
    assert sweep.neighbors_summary_row(1, 1, 1, 0, e, e, e) == "1.000\t1.000\t1\t0\t0\t15\t0\tNA\tNA\tNA\tNA\n"
    # the percentile rule of <verb>_fidelity.tsv: the lower of the two middle values is not the median; p10 = sorted[floor(0.1 (n - 1))]
    kf, sh = np.full(4, 10, np.uint32), np.array([1, 2, 3, 10], np.uint32)
    assert sweep.neighbors_summary_row(1, 1, 1, 9, kf, kf, sh).split("\t")[6:10] == ["4", "0.250000", "0.100000", "0.400000"]


def test_the_flag_bits_and_the_refusals(tmp_path):
    one, p_one = sweep._floats([1])
    caps = np.array([5], np.uint64)
    L = _lib.lib()
    seeds = caps.astype(np.uint32)
    calls = (lambda fl: L.fastf_sweep(b"x", b"y", b"b", b"f", p_one, 1, p_one, 1, 926, fl),
             lambda fl: L.fastf_cap(b"x", b"y", b"b", b"f", p_one, 1, caps.ctypes.data, 1, 926, fl),
             lambda fl: L.fastf_level(b"x", b"y", b"b", b"f", p_one, 1, caps.ctypes.data, 1, 926, fl),
             lambda fl: L.fastf_sweep_reps(b"x", b"y", b"b", b"f", p_one, 1, p_one, 1, seeds.ctypes.data, 1, fl),
             lambda fl: L.fastf_cap_reps(b"x", b"y", b"b", b"f", p_one, 1, caps.ctypes.data, 1, seeds.ctypes.data, 1, fl),
             lambda fl: L.fastf_level_reps(b"x", b"y", b"b", b"f", p_one, 1, caps.ctypes.data, 1, seeds.ctypes.data, 1, fl))
    for call in calls:
        for flags in (4 | 512, 16 | 512, 64 | 512, 256 | 512, 1024, 512 | 1024):      # bits 4, 16, 64 and 256 are still nobody's beside the new bit
            with pytest.raises(F.FastfError, match="unknown flags"):
                _lib.check(call(flags))
        for flags in (512, 512 | 128 | 32 | 8 | 2 | 1):     # bit 512 is known: the call gets as far as the missing file
            with pytest.raises(F.FastfError, match="does not exist"):
                _lib.check(call(flags))
    assert sweep._flags(False, False, False, False, False, True) == 512 and level._flags(True, False, False, neighbors=True) == 513
    bt, ft, bar, genes = synth.make_lists(5, 3)
    fl, xf, cb, gx, ub = synth.make_records(20, bar, genes)
    bam, b, f = tmp_path / "x.bam", tmp_path / "b.tsv", tmp_path / "f.tsv"
    synth.write_bam(str(bam), fl, xf, cb, gx, ub)
    b.write_bytes(bt); f.write_bytes(ft)
    several = dict(os.environ, FASTF_DEVICES="0,1")
    for k, (verb, extra) in enumerate([("sweep", ["-r", "0.5"]), ("cap", ["-n", "5"]), ("level", ["-m", "5"])]):
        out = tmp_path / ("out%d" % k)
        for more in ([], ["--fidelity", "--gene-fidelity"]):
            r = subprocess.run([_lib.cli_path(), verb, "--neighbors", "-o", str(out), "-a", str(b), "-f", str(f), "-b", str(bam)] + extra + more,
                               capture_output=True, text=True, timeout=60, env=several)
            assert r.returncode == 1 and "several devices" in r.stderr, r.stderr
            assert "%s: --neighbors needs the resident form" % verb in r.stderr
            assert not out.exists()                         # refused before the output directory is made
        r = subprocess.run([_lib.cli_path(), verb, "--help"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and "--neighbors" in r.stdout and "%s_neighbors.tsv" % verb in r.stdout and "BETWEEN the cells" in r.stdout
        assert "--gene-fidelity" in r.stdout and "15 nearest neighbours" in r.stdout
        for opt in ("-N", "--neighbours", "--neighbor"):    # the long form alone
            r = subprocess.run([_lib.cli_path(), verb, opt, "-o", str(out)], capture_output=True, text=True, timeout=60)
            assert r.returncode == 1 and "unknown option" in r.stderr
    os.environ["FASTF_DEVICES"] = "0,1"
    try:
        with pytest.raises(F.FastfError, match="sweep: --neighbors needs the resident form.*several devices"):
            sweep.sweep(bam, tmp_path / "o", b, f, [1], [1], neighbors=True)
        with pytest.raises(F.FastfError, match="cap: --neighbors needs the resident form.*several devices"):
            cap.cap_reps(bam, tmp_path / "o", b, f, [1], [5], [1, 2], neighbors=True)
        with pytest.raises(F.FastfError, match="level: --neighbors needs the resident form.*several devices"):
            level.level(bam, tmp_path / "o", b, f, [1], [5], neighbors=True)
    finally:
        del os.environ["FASTF_DEVICES"]
    assert not (tmp_path / "o").exists()
