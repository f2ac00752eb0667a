"""--gene-fidelity, the parts that need no device: the host twin against the numpy reference, the missing-partner error, the NA rules,
the tie rule and K of the ranking, headers and rows, the median and p10 rule, the flag on the three verbs and the refusals — and the
builders of the fixtures tests/test_gpu_gene_fidelity.py runs on the device, with a census that shows every named edge in the data."""
import os
import re
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, cap, level, sweep, synth
import gene_fidelity_ref as G
from test_fidelity_host import nested_pair

GMOM_LDS_GENES, GMOM_LDS_RANGES = 8192, 16                  # gene_fidelity_kernels.hpp (pinned below against the source)
LDS_LIMIT = GMOM_LDS_GENES * GMOM_LDS_RANGES
MI355X_WAVES = 4 * 256 * 4                                  # FID_BLOCKS_PER_CU workgroups on each of 256 CUs, four waves each


# ---- the fixtures of the device tests (numpy alone) ----
def sorted_rows(rng, n_rows, n_cells, n_features=4000):
    """n_rows distinct (cell, feature) pairs ascending, counts 0 .. 50 with zeros among them"""
    keys = np.unique(rng.integers(0, n_cells * n_features, size=int(n_rows * 1.3) + 16))
    while len(keys) < n_rows:
        keys = np.unique(np.concatenate([keys, rng.integers(0, n_cells * n_features, size=n_rows)]))
    keys = np.sort(rng.choice(keys, size=n_rows, replace=False))
    return (keys % n_features + 1, keys // n_features + 1, rng.integers(0, 51, size=n_rows))


def subset(rng, full, keep):
    sel = rng.random(len(full[0])) < keep if not isinstance(keep, np.ndarray) else keep
    y = np.minimum(full[2][sel], rng.integers(0, 51, size=int(sel.sum())))
    return (full[0][sel], full[1][sel], y)


def partner_row_counts(waves):
    w = 64 * waves                                          # up to here every wave's span is 64 rows, one turn; behind it 128, two turns
    return [0, 1, 63, 64, 65, 255, 256, 257, w - 1, w, w + 1]


PARTNER_FIXTURES = ["rows%d" % k for k in range(11)] + ["equal", "first", "last", "every50", "one_cell"]
MISSING_FIXTURES = ["missing_first", "missing_middle", "missing_last", "no_full_rows"]


def partner_fixture(name, waves):
    """(full, point): the point a row subset of the full rows, but for the MISSING_FIXTURES, where one point row has lost its partner"""
    rng = np.random.default_rng(sum(name.encode()))
    if name.startswith("rows"):
        n = partner_row_counts(waves)[int(name[4:])]
        full = sorted_rows(rng, 3 * n + 5, 700)
        sel = np.zeros(len(full[0]), bool)
        sel[rng.choice(len(sel), size=n, replace=False)] = True
        return full, subset(rng, full, sel)
    if name == "one_cell":                                  # spans of three turns, one cell over all of them
        n = 64 * waves * 2 + 777
        full = (np.arange(1, n + 1), np.full(n, 4), rng.integers(0, 20, size=n))
        return full, subset(rng, full, 0.7)
    if name == "every50":
        full = sorted_rows(rng, 400_000, 500, n_features=3000)
        sel = np.zeros(len(full[0]), bool)
        sel[::50] = True
        return full, subset(rng, full, sel)
    full = sorted_rows(rng, 20_000, 90, n_features=900)
    if name == "equal":
        return full, full
    if name in ("first", "last"):
        at = 0 if name == "first" else len(full[0]) - 1
        full[2][at] = 9
        return full, tuple(a[at:at + 1].copy() for a in full)
    point = subset(rng, full, 0.5)
    if name == "no_full_rows":
        return tuple(a[:0] for a in full), point
    where = {"missing_first": 0, "missing_middle": len(point[0]) // 2, "missing_last": len(point[0]) - 1}[name]
    gone = (full[1] == point[1][where]) & (full[0] == point[0][where])
    assert gone.sum() == 1
    return tuple(a[~gone] for a in full), point


MOMENT_LISTS = [1, 3, GMOM_LDS_GENES - 1, GMOM_LDS_GENES, GMOM_LDS_GENES + 1, 36_601, LDS_LIMIT + 1]
MOMENT_FIXTURES = ["list%d" % n for n in MOMENT_LISTS] + ["one_gene", "big"] + ["rows%d" % n for n in (0, 1, 63, 64, 65)]


def moments_fixture(name):
    """(feature, a, b, n_features): rows in no order; features 0 and n_features + 1 among them, rows with b == 0, the last gene"""
    rng = np.random.default_rng(sum(name.encode()))
    if name == "one_gene":                                  # one gene owns every row: the wave-wide shortcut, whole items of one address
        n = 5000
        return np.full(n, 2), rng.integers(0, 1000, size=n), rng.integers(0, 1000, size=n), 3
    if name == "big":                                       # a sum past 2^63 under counts that sum below 2^32
        return np.array([5, 5, 1]), np.array([4_000_000_000, 3, 7]), np.array([4_000_000_000, 3, 0]), 5
    if name.startswith("rows"):
        n, nf = int(name[4:]), 50
        return rng.integers(0, nf + 2, size=n), rng.integers(0, 100, size=n), rng.integers(0, 100, size=n), nf
    nf = int(name[4:])
    n = 30_000
    f = rng.integers(0, nf + 2, size=n)                     # 0 and nf + 1 are outside the list
    f[:8] = [0, nf + 1, nf, nf, 1, 1, 0, nf + 1]
    a, b = rng.integers(0, 3000, size=n), rng.integers(0, 3000, size=n)
    b[rng.random(n) < 0.2] = 0
    b[2], b[3] = 11, 0                                      # the last gene: one counted row, one with b == 0
    return f, a, b, nf


def last_range_fixture(nf):
    """(feature, a, b) for a list of nf genes, 16 x 8192 or one more — the most the LDS form takes, and the first list of the general
    form: 200 rows in a row on the last gene of the seventh range (whole 64-row items of one gene), then, shuffled, 3000 random rows
    and seven rows each (two with b == 0) on the first and the last gene of every range and on the features 0, nf + 1 and 2^32 - 1"""
    rng = np.random.default_rng(nf)
    special = [0, nf + 1, 0xFFFFFFFF]
    for lo in range(0, nf, GMOM_LDS_GENES):
        special += [lo + 1, min(lo + GMOM_LDS_GENES, nf)]
    f = np.concatenate([rng.integers(1, nf + 1, size=3000), np.repeat(np.array(special, np.int64), 7)])
    a = np.concatenate([rng.integers(0, 3000, size=3000), np.tile([5, 0, 1, 2, 9, 3, 1], len(special))])
    b = np.concatenate([rng.integers(0, 3000, size=3000), np.tile([3, 0, 1, 2, 0, 5, 1], len(special))])
    order = rng.permutation(len(f))
    stretch = 200
    return (np.concatenate([np.full(stretch, 7 * GMOM_LDS_GENES), f[order]]), np.concatenate([rng.integers(0, 1000, size=stretch), a[order]]),
            np.concatenate([rng.integers(1, 1000, size=stretch), b[order]]))


@pytest.mark.parametrize("nf", [LDS_LIMIT, LDS_LIMIT + 1])
def test_census_of_the_last_range_fixture(nf):
    """the reference alone, against a plain loop over the rows: every edge gene has its sums, the features outside the list add nothing"""
    f, a, b = last_range_fixture(nf)
    assert 3000 < len(f) < 4000 and (f[:200] == 7 * GMOM_LDS_GENES).all() and (b[:200] > 0).all()
    want_ab, want_bb = [0] * nf, [0] * nf
    for g, x, y in zip(f.tolist(), a.tolist(), b.tolist()):
        if 1 <= g <= nf:
            want_ab[g - 1] += x * y
            want_bb[g - 1] += y * y
    assert G.gene_sums(f, a, b, nf) == (want_ab, want_bb)
    assert sum((f == g).sum() for g in (0, nf + 1, 0xFFFFFFFF)) == 21
    for lo in range(0, nf, GMOM_LDS_GENES):                 # 16 ranges, or 16 and a seventeenth of one gene
        for g in (lo + 1, min(lo + GMOM_LDS_GENES, nf)):
            assert want_bb[g - 1] >= 40 and want_ab[g - 1] >= 21 and ((f == g) & (b == 0)).sum() >= 2
    assert (nf + GMOM_LDS_GENES - 1) // GMOM_LDS_GENES == (16 if nf == LDS_LIMIT else 17)


def test_census_of_the_device_fixtures():
    src = open(os.path.join(os.path.dirname(__file__), "..", "fastf_amd", "csrc", "gene_fidelity_kernels.hpp")).read()
    assert "GMOM_LDS_GENES = GENE_LDS_GENES / 2, GMOM_LDS_RANGES = 2 * GENE_LDS_RANGES" in src
    gk = open(os.path.join(os.path.dirname(__file__), "..", "fastf_amd", "csrc", "gene_kernels.hpp")).read()
    assert re.search(r"GENE_LDS_GENES = %d\b" % (2 * GMOM_LDS_GENES), gk) and re.search(r"GENE_LDS_RANGES = %d\b" % (GMOM_LDS_RANGES // 2), gk)
    w = MI355X_WAVES
    assert partner_row_counts(w)[-3:] == [64 * w - 1, 64 * w, 64 * w + 1]
    for k, n in enumerate(partner_row_counts(300)):
        full, point = partner_fixture("rows%d" % k, 300)
        assert len(point[0]) == n and len(full[0]) == 3 * n + 5
        assert n < 64 or (0 in point[2] and 0 in full[2])   # zero-count rows on both sides
    full, point = partner_fixture("equal", w)
    assert point is full
    for name, at in (("first", 0), ("last", -1)):
        full, point = partner_fixture(name, w)
        assert len(point[0]) == 1 and (point[0][0], point[1][0]) == (full[0][at], full[1][at]) and point[2][0] == 9
    full, point = partner_fixture("every50", w)
    assert len(point[0]) * 50 == len(full[0])
    full, point = partner_fixture("one_cell", 300)
    assert len(np.unique(point[1])) == 1 and len(point[0]) > 64 * 300
    for name in PARTNER_FIXTURES[11:]:
        G.partner_counts(*partner_fixture(name, 300))      # (asserts order and partners)
    for name in MISSING_FIXTURES:
        full, point = partner_fixture(name, w)
        kx, ky = G.R._keys(full[1], full[0]), G.R._keys(point[1], point[0])
        lost = np.nonzero(~np.isin(ky, kx))[0]
        if name == "no_full_rows":
            assert len(kx) == 0 and len(lost) == len(ky) > 0
        else:
            assert list(lost) == [{"missing_first": 0, "missing_middle": len(ky) // 2, "missing_last": len(ky) - 1}[name]]
    assert MOMENT_LISTS == [1, 3, 8191, 8192, 8193, 36_601, 131_073] and 36_601 > 4 * GMOM_LDS_GENES
    for n in MOMENT_LISTS:
        f, a, b, nf = moments_fixture("list%d" % n)
        assert nf == n and f.min() == 0 and f.max() == nf + 1 and (b == 0).sum() > 1000 and (b[f == nf] > 0).any()
        ab, bb = G.gene_sums(f, a, b, nf)
        assert bb[nf - 1] > 0 and bb[0] > 0                 # the last gene of the last range, the first of the first
    f, a, b, nf = moments_fixture("one_gene")
    assert (f == 2).all() and len(f) > 64 * 4
    f, a, b, nf = moments_fixture("big")
    ab, bb = G.gene_sums(f, a, b, nf)
    assert ab[4] > 2 ** 63 and bb[4] > 2 ** 63 and int(a.sum()) < 2 ** 32 and int(b.sum()) < 2 ** 32 and ab[0] == bb[0] == 0
    assert [len(moments_fixture("rows%d" % n)[0]) for n in (0, 1, 63, 64, 65)] == [0, 1, 63, 64, 65]


# ---- the host twin ----
def _twin(full, point, nf):
    return dict(zip(G.INT_COLUMNS, ([int(v) for v in arr] for arr in sweep.gene_fidelity_from_coo(full, point, nf))))


@pytest.mark.parametrize("shape", [(1, 1, 1.0, 1.0), (1, 40, 0.5, 0.5), (7, 1, 0.6, 0.7), (50, 30, 0.3, 0.5), (300, 200, 0.05, 0.2), (40, 25, 0.4, 0.0),
                                   (40, 25, 0.4, 1.0)])
def test_the_host_twin_against_the_reference(shape):
    n_cells, n_features, density, keep = shape
    rng = np.random.default_rng(n_cells * 1000 + n_features)
    full, point = nested_pair(rng, n_cells, n_features, density, keep, big=n_cells == 50)
    mom = G.moments(full, point, n_features)
    assert _twin(full, point, n_features) == mom
    if n_cells >= 40:
        assert 0 in full[2] and (keep == 0.0 or 0 in point[2])     # zero counts on both sides
    if n_cells == 50:
        assert max(mom["sum_xx"]) > 2 ** 63 and int(np.asarray(full[2], np.int64).sum()) < 2 ** 32
    self_ = _twin(full, full, n_features)                   # the full rows with themselves
    assert self_["sum_xy"] == self_["sum_xx"] == self_["sum_yy"] == mom["sum_xx"] and self_["sum_y"] == mom["sum_x"]
    # sum_x / cells_full and sum_y / cells are the per-gene summary's
    for rows, s, c in ((full, "sum_x", "cells_full"), (point, "sum_y", "cells")):
        cpg, upg = sweep.genes_from_coo(rows[0], rows[2], n_features)
        assert [int(v) for v in upg] == mom[s] and [int(v) for v in cpg] == mom[c]
    # a list shorter than the features named: the rows beyond it add nothing
    if n_features > 1:
        short = _twin(full, point, n_features - 1)
        assert all(short[c] == mom[c][:-1] for c in G.INT_COLUMNS)


def test_a_missing_partner_is_an_error():
    full = (np.array([1, 3, 5, 2]), np.array([1, 1, 1, 2]), np.array([4, 5, 6, 7]))
    ok = (np.array([3, 2]), np.array([1, 2]), np.array([1, 1]))
    sweep.gene_fidelity_from_coo(full, ok, 5)
    for bad in [(np.array([2]), np.array([1]), np.array([1])), (np.array([1]), np.array([3]), np.array([1])),
                (np.array([3, 4]), np.array([1, 2]), np.array([1, 1])), (np.array([1]), np.array([0]), np.array([1]))]:
        with pytest.raises(F.FastfError, match="no partner"):
            sweep.gene_fidelity_from_coo(full, bad, 5)
    none = (np.zeros(0), np.zeros(0), np.zeros(0))
    with pytest.raises(F.FastfError, match="no partner"):
        sweep.gene_fidelity_from_coo(none, ok, 5)
    out = sweep.gene_fidelity_from_coo(full, none, 5)
    assert [int(v) for v in out[0]] == [4, 7, 5, 0, 6] and not any(out[k].any() for k in (1, 3, 5, 6))


def _row(n, ints, name="ENSG01"):
    return sweep.gene_fidelity_row(name, n, *ints).rstrip("\n").split("\t")


def test_headers_the_mirrors_and_the_rows():
    assert sweep.gene_fidelity_header() == "\t".join(sweep.POINT_GENE_FIDELITY_COLUMNS) + "\n"
    assert sweep.POINT_GENE_FIDELITY_COLUMNS == ("feature",) + G.INT_COLUMNS + ("pearson", "disp_full", "disp")
    tail = ("seed", "n_cells", "genes_full", "genes_defined", "median_pearson", "p10_pearson", "mean_pearson", "hvg_k", "hvg_overlap")
    for mod, second in ((sweep, "rate_depth"), (cap, "reads_per_cell"), (level, "umi_cap")):
        assert mod.GENE_FIDELITY_COLUMNS == ("rate_cell", second) + tail
        assert mod.gene_fidelity_header(mod.__name__.split(".")[-1]) == "\t".join(mod.GENE_FIDELITY_COLUMNS) + "\n"
        assert mod.GENE_FIDELITY == 128 and mod.FIDELITY == 32
    assert sweep.HVG_TOP == G.HVG_TOP == 2000
    for sym in ("fastf_dev_partner_counts", "fastf_dev_gene_moments", "fastf_gene_fidelity_from_coo", "fastf_gene_fidelity_metrics", "fastf_gene_fidelity_row",
                "fastf_gene_fidelity_header", "fastf_sweep_gene_fidelity_header", "fastf_cap_gene_fidelity_header", "fastf_level_gene_fidelity_header",
                "fastf_gene_fidelity_summary_row"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(_lib.lib(), sym)
    names = _lib.lib().fastf_kernel_names().decode().split(",")
    assert "partner_counts_kernel" in names and "gene_moments_kernel" in names and "fidelity_kernel" in names
    assert hasattr(F.Engine, "dev_partner_counts") and hasattr(F.Engine, "dev_gene_moments")
    rng = np.random.default_rng(3)
    n_cells, nf = 30, 40
    full, point = nested_pair(rng, n_cells, nf, 0.5, 0.6)
    mom = G.moments(full, point, nf)
    want = G.gene_rows(["g%d" % g for g in range(nf)], n_cells, mom)
    for g in range(nf):
        line = sweep.gene_fidelity_row("g%d" % g, n_cells, *[mom[c][g] for c in G.INT_COLUMNS])
        assert line.endswith("\n")
        G.assert_fields(line[:-1].split("\t"), want[g], 8, g)
        got = sweep.gene_fidelity_metrics(n_cells, *[mom[c][g] for c in ("sum_x", "sum_y", "sum_xx", "sum_yy", "sum_xy")])
        ref = G.metrics(n_cells, *[mom[c][g] for c in ("sum_x", "sum_y", "sum_xx", "sum_yy", "sum_xy")])
        assert got[1:] == ref[1:]                           # the ranking values: the same doubles, bit for bit
        assert (got[0] is None) == (ref[0] is None) and (got[0] is None or abs(got[0] - ref[0]) < 1e-12)
    assert sum(1 for w in want if w[8] != "NA") > 20


def test_the_na_rules():
    # order: sum_x sum_y cells_full cells sum_xx sum_yy sum_xy
    # n = 1: one cell has no variance, and no dispersion either
    assert _row(1, (7, 3, 1, 1, 49, 9, 21))[8:] == ["NA", "NA", "NA"]
    # a gene absent at full depth (and so at the point)
    assert _row(10, (0, 0, 0, 0, 0, 0, 0)) == ["ENSG01"] + ["0"] * 7 + ["NA", "NA", "NA"]
    # present at full depth, absent at the point: only disp_full
    got = _row(10, (6, 0, 2, 0, 20, 0, 0))
    assert got[8] == "NA" and got[10] == "NA" and got[9] == "%.6f" % ((10 * 20 - 36) / (9 * 6.0))
    # constant across the cells (every cell 2 at full, 1 at the point): no variance, dispersion 0
    assert _row(10, (20, 10, 10, 10, 40, 10, 20))[8:] == ["NA", "0.000000", "0.000000"]
    # constant at the point only
    got = _row(4, (10, 4, 4, 4, 30, 4, 10))
    assert got[8] == "NA" and got[9] != "NA" and got[10] == "0.000000"
    # point == full: pearson 1, the same dispersion twice
    got = _row(10, (6, 6, 2, 2, 20, 20, 20))
    assert got[8] == "1.000000" and got[9] == got[10]
    # a negative pearson: n = 2, x = (5, 1), y = (0, 1)
    assert G.metrics(2, 6, 1, 26, 1, 1)[0] == -1.0 and _row(2, (6, 1, 2, 1, 26, 1, 1))[8] == "-1.000000"
    # sums beyond 2^63 stay exact
    big = (4_000_000_001, 4_000_000_000, 2, 1, 16 * 10 ** 18 + 1, 16 * 10 ** 18, 16 * 10 ** 18)
    G.assert_fields(_row(3, big), G.gene_rows(["ENSG01"], 3, {c: [v] for c, v in zip(G.INT_COLUMNS, big)})[0], 8)


def _summary(n, mom, mod=sweep, second=0.1, seed=926):
    arr = [np.array(mom[c], dtype=np.uint64) for c in ("sum_x", "sum_y", "sum_xx", "sum_yy", "sum_xy")]
    return mod.gene_fidelity_summary_row(0.5, second, seed, n, *arr)


def _mom(rows):
    """rows of (sum_x, sum_y, sum_xx, sum_yy, sum_xy) -> the dict of the reference (the two cell counts play no part in the table)"""
    cols = list(zip(*rows)) if rows else [()] * 5
    out = {c: list(v) for c, v in zip(("sum_x", "sum_y", "sum_xx", "sum_yy", "sum_xy"), cols)}
    out["cells_full"] = out["cells"] = [0] * len(rows)
    return out


def _overlap_with_ties_by_descending_index(n, mom):
    """hvg_overlap under the WRONG tie rule (the higher index first): what a fixture must tell apart from the right one"""
    m = G._all_metrics(n, mom)
    a = sorted((g for g in range(len(m)) if m[g][1] is not None), key=lambda g: (-m[g][1], -g))
    b = sorted((g for g in range(len(m)) if m[g][2] is not None), key=lambda g: (-m[g][2], -g))
    K = min(G.HVG_TOP, len(a))
    return len(set(a[:K]) & set(b[:K])) / K


# rows of (sum_x, sum_y, sum_xx, sum_yy, sum_xy) over n = 10 cells: disp_full 4.07 / 3.33 / 1.67, disp 2.37 / 2.22 / 1.11
_HI = (30, 12, 200, 40, 80)
_TIE = (20, 10, 100, 30, 50)                                # disp_full 3.33, disp 2.22
_LOW_Y = (20, 10, 100, 20, 40)                              # ties with _TIE at full depth, the strictly lowest disp
_LOW_X = (20, 10, 70, 30, 40)                               # ties with _TIE at the point, the strictly lowest disp_full


@pytest.mark.parametrize("at", [(0, 2000), (1000, 1001), (7, 1500)])
@pytest.mark.parametrize("which", ["tie_full_q_low", "tie_full_p_low", "tie_point_q_low", "tie_point_p_low"])
def test_the_tie_rule_of_the_ranking(which, at):
    """2001 genes, all defined on both sides, K = 2000: each ranking drops exactly one gene.  Genes p < q tie for the LAST place of one
    ranking, and one of them alone is last in the other: ascending index keeps p in the tied ranking, so the overlap is 1 when q is
    the other ranking's loser and 1999 / 2000 when p is — and the other way round under a reversed tie rule.  The C row must give the
    reference's value in every placement of the pair"""
    n = 10
    p, q = at
    low = _LOW_Y if which.startswith("tie_full") else _LOW_X
    rows = [_HI] * (G.HVG_TOP + 1)
    rows[p], rows[q] = (_TIE, low) if which.endswith("q_low") else (low, _TIE)
    mom = _mom(rows)
    m = G._all_metrics(n, mom)
    col = 1 if which.startswith("tie_full") else 2         # the ranking with the tie, the other has a strict loser
    assert m[p][col] == m[q][col] < min(v[col] for g, v in enumerate(m) if g not in at)
    assert min(range(len(m)), key=lambda g: m[g][3 - col]) == (q if which.endswith("q_low") else p)
    assert all(v is not None for row in m for v in row[1:])
    K, A, B, ov = G.hvg(n, mom)
    assert K == 2000 and len(A) == len(B) == 2000
    tied, strict = (A, B) if col == 1 else (B, A)
    assert p in tied and q not in tied                      # ascending index: p keeps the last place
    right = 1.0 if which.endswith("q_low") else 1999 / 2000
    wrong = _overlap_with_ties_by_descending_index(n, mom)
    assert ov == right and wrong == (1999 / 2000 if which.endswith("q_low") else 1.0) and wrong != right
    got = _summary(n, mom)[:-1].split("\t")
    G.assert_fields(got, G.summary_fields(["0.500", "0.100"], 926, n, mom), 6)
    assert got[-2:] == ["2000", "%.6f" % right]             # "1.000000" / "0.999500": 5e-4 apart, TOL is 1.5e-6


def test_ties_inside_and_outside_the_cut():
    """a tie that does not straddle the cut changes nothing, and a list shorter than K has no cut"""
    n = 10
    lo = (10, 5, 20, 7, 10)
    for order in ([_TIE, _TIE, _HI], [_HI, _TIE, _TIE], [_TIE, _HI, _TIE]):
        mom = _mom(order + [lo] * (G.HVG_TOP - 2))          # 2001 genes: the last `lo` is ranked out of both
        K, A, B, ov = G.hvg(n, mom)
        assert K == 2000 and A == B and A[-1] == 1999 and 2000 not in A
        want = G.summary_fields(["0.500", "0.100"], 926, n, mom)
        G.assert_fields(_summary(n, mom)[:-1].split("\t"), want, 6)
        assert want[-2:] == ["2000", "1.000000"]
    mom = _mom([_TIE, _TIE, (20, 30, 100, 200, 60)])
    mom["sum_x"][2], mom["sum_xx"][2], mom["sum_xy"][2] = 0, 0, 0      # gene 2 undefined at full depth: K = 2, A the tie, B = gene 2 and the tie's lower index
    assert G.hvg(n, mom) == (2, [0, 1], [2, 0], 0.5)
    G.assert_fields(_summary(n, mom)[:-1].split("\t"), G.summary_fields(["0.500", "0.100"], 926, n, mom), 6)


@pytest.mark.parametrize("n_genes", [3, 2001])
def test_k_and_a_point_with_fewer_defined_genes(n_genes):
    rng = np.random.default_rng(n_genes)
    n_cells = 12
    full, point = nested_pair(rng, n_cells, n_genes, 0.6, 0.6, zero_rate=0.0)
    mom = G.moments(full, point, n_genes)
    K, A, B, ov = G.hvg(n_cells, mom)
    assert K == min(2000, n_genes) and len(B) == min(K, sum(1 for v in mom["sum_y"] if v))
    want = G.summary_fields(["0.500", "0.100"], 926, n_cells, mom)
    G.assert_fields(_summary(n_cells, mom)[:-1].split("\t"), want, 6)
    assert want[9] == str(K) and (n_genes == 3 or 0 < ov < 1)
    # the point loses most genes: fewer than K have a dispersion there
    for g in range(2, n_genes):
        mom["sum_y"][g] = mom["sum_yy"][g] = mom["sum_xy"][g] = 0
    K2, A2, B2, ov2 = G.hvg(n_cells, mom)
    assert K2 == K and len(B2) == 2 and ov2 == len(set(A2) & {0, 1}) / K
    G.assert_fields(_summary(n_cells, mom)[:-1].split("\t"), G.summary_fields(["0.500", "0.100"], 926, n_cells, mom), 6)


@pytest.mark.parametrize("n_defined", [0, 1, 2, 25])
def test_the_median_and_p10_rule(n_defined):
    rng = np.random.default_rng(70 + n_defined)
    n_cells, nf = 14, n_defined + 3
    full, point = nested_pair(rng, n_cells, nf, 0.9, 0.7, zero_rate=0.0)
    mom = G.moments(full, point, nf)
    for g in range(n_defined, nf):                         # the last three genes: undefined (absent at the point; absent at full; constant)
        for c in G.INT_COLUMNS:
            mom[c][g] = 0
    mom["sum_x"][n_defined], mom["sum_xx"][n_defined] = 9, 41
    mom["sum_x"][nf - 1], mom["sum_xx"][nf - 1], mom["sum_y"][nf - 1], mom["sum_yy"][nf - 1], mom["sum_xy"][nf - 1] = 28, 56, 14, 14, 28
    want = G.summary_fields(["0.500", "0.100"], 926, n_cells, mom)
    got = _summary(n_cells, mom)
    assert got.endswith("\n")
    G.assert_fields(got[:-1].split("\t"), want, 6, n_defined)
    assert want[5] == str(n_defined) and want[3] == str(n_cells) and want[4] == str(n_defined + 2)
    pe = sorted(p for p, _, _ in G._all_metrics(n_cells, mom) if p is not None)
    assert len(pe) == n_defined
    if n_defined == 0:
        assert want[6:9] == ["NA"] * 3 and want[9] == "2"
    else:
        assert want[7] == "%.6f" % pe[int(0.1 * (n_defined - 1))] and (n_defined < 25 or pe[2] != pe[0])
        assert want[6] == "%.6f" % (pe[n_defined // 2] if n_defined & 1 else (pe[n_defined // 2 - 1] + pe[n_defined // 2]) / 2)
    assert _summary(n_cells, mom, cap, 40).split("\t")[:3] == ["0.500", "40", "926"]
    assert _summary(n_cells, mom, level, 7, 5).split("\t")[:3] == ["0.500", "7", "5"]
    z = np.zeros(0, np.uint64)
    assert sweep.gene_fidelity_summary_row(1, 1, 1, 0, z, z, z, z, z) == "1.000\t1.000\t1\t0\t0\t0\tNA\tNA\tNA\t0\tNA\n"


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
        for flags in (4 | 128, 16 | 128, 64 | 128, 256, 128 | 256):      # bits 4, 16 and 64 are still nobody's beside the new bit
            with pytest.raises(F.FastfError, match="unknown flags"):
                _lib.check(call(flags))
        for flags in (128, 128 | 32 | 8 | 2 | 1):            # bit 128 is known: the call gets as far as the missing file
            with pytest.raises(F.FastfError, match="does not exist"):
                _lib.check(call(flags))
    bt, ft, bar, genes = synth.make_lists(5, 3)
    fl, xf, cb, gx, ub = synth.make_records(20, bar, genes)
    bam, b, f = tmp_path / "x.bam", tmp_path / "b.tsv", tmp_path / "f.tsv"
    synth.write_bam(str(bam), fl, xf, cb, gx, ub)
    b.write_bytes(bt); f.write_bytes(ft)
    several = dict(os.environ, FASTF_DEVICES="0,1")
    for k, (verb, extra) in enumerate([("sweep", ["-r", "0.5"]), ("cap", ["-n", "5"]), ("level", ["-m", "5"])]):
        out = tmp_path / ("out%d" % k)
        r = subprocess.run([_lib.cli_path(), verb, "--gene-fidelity", "-o", str(out), "-a", str(b), "-f", str(f), "-b", str(bam)] + extra,
                           capture_output=True, text=True, timeout=60, env=several)
        assert r.returncode == 1 and "several devices" in r.stderr, r.stderr
        assert "%s: --gene-fidelity needs the resident form" % verb in r.stderr
        assert not out.exists()                             # refused before the output directory is made
        r = subprocess.run([_lib.cli_path(), verb, "--help"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and "--gene-fidelity" in r.stdout and "%s_gene_fidelity.tsv" % verb in r.stdout and "per GENE" in r.stdout
        assert "--fidelity " in r.stdout and "RAW counts" in r.stdout
        for opt in ("-F", "-Q", "--gene_fidelity"):         # the long form alone
            r = subprocess.run([_lib.cli_path(), verb, opt, "-o", str(out)], capture_output=True, text=True, timeout=60)
            assert r.returncode == 1 and "unknown option" in r.stderr
    os.environ["FASTF_DEVICES"] = "0,1"
    try:
        with pytest.raises(F.FastfError, match="--gene-fidelity needs the resident form"):
            sweep.sweep(bam, tmp_path / "o", b, f, [1], [1], gene_fidelity=True)
        with pytest.raises(F.FastfError, match="cap: --gene-fidelity needs the resident form.*several devices"):
            cap.cap_reps(bam, tmp_path / "o", b, f, [1], [5], [1, 2], gene_fidelity=True)
        with pytest.raises(F.FastfError, match="level: --gene-fidelity needs the resident form.*several devices"):
            level.level(bam, tmp_path / "o", b, f, [1], [5], gene_fidelity=True)
        with pytest.raises(F.FastfError, match="--fidelity and --gene-fidelity need the resident form"):
            sweep.sweep(bam, tmp_path / "o", b, f, [1], [1], fidelity=True, gene_fidelity=True)
    finally:
        del os.environ["FASTF_DEVICES"]
    assert not (tmp_path / "o").exists()
