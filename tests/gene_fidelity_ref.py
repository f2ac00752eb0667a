"""The reference for --gene-fidelity: the seven integers per gene from two COO matrices with numpy, in Python ints (the join is
fidelity_ref.moments': the keys of both row sets, one searchsorted), the three metrics and the ranking of the highly variable genes by
the formulas of include/fastf_amd.h, and the rows of gene_fidelity.tsv.gz and <verb>_gene_fidelity.tsv from them.  The full matrix of a
pair is fidelity_ref.full_matrix's."""
import math

import numpy as np

import fidelity_ref as R

INT_COLUMNS = ("sum_x", "sum_y", "cells_full", "cells", "sum_xx", "sum_yy", "sum_xy")
TOL = R.TOL
HVG_TOP = 2000


def partner_counts(full, point):
    """x of every point row (Python ints); asserts what fidelity_ref.moments asserts"""
    xf, xc, xk = (np.asarray(a, np.int64) for a in full)
    yf, yc, _ = (np.asarray(a, np.int64) for a in point)
    kx, ky = R._keys(xc, xf), R._keys(yc, yf)
    assert (kx[1:] > kx[:-1]).all() and (ky[1:] > ky[:-1]).all(), "rows not ascending by (cell, feature)"
    at = np.searchsorted(kx, ky)
    assert len(ky) == 0 or (at.max() < len(kx) and (kx[at] == ky).all()), "a point row without a partner"
    return xk[at] if len(ky) else np.zeros(0, np.int64)


def gene_sums(feature, a, b, n_features):
    """(sum of a * b, sum of b * b) per gene as lists of Python ints; a feature outside 1 .. n_features adds nothing"""
    f = np.asarray(feature, np.int64)
    ok = (f >= 1) & (f <= n_features)
    ao, bo = np.asarray(a, np.int64).astype(object)[ok], np.asarray(b, np.int64).astype(object)[ok]
    ab, bb = np.zeros(n_features, dtype=object), np.zeros(n_features, dtype=object)
    np.add.at(ab, f[ok] - 1, ao * bo)
    np.add.at(bb, f[ok] - 1, bo * bo)
    return [int(v) for v in ab], [int(v) for v in bb]


def moments(full, point, n_features):
    """full, point: (feature, cell, count) ascending by (cell, feature), the point a row subset of the full rows.  Returns a dict of
    seven lists of Python ints, one entry per gene"""
    xf, _, xk = (np.asarray(a, np.int64) for a in full)
    yf, _, yk = (np.asarray(a, np.int64) for a in point)
    x_of_y = partner_counts(full, point)
    out = {}
    one_x, one_y = np.ones(len(xk), np.int64), np.ones(len(yk), np.int64)
    out["sum_x"] = gene_sums(xf, xk, one_x, n_features)[0]
    out["sum_y"] = gene_sums(yf, yk, one_y, n_features)[0]
    out["cells_full"] = gene_sums(xf, one_x, (xk >= 1).astype(np.int64), n_features)[1]
    out["cells"] = gene_sums(yf, one_y, (yk >= 1).astype(np.int64), n_features)[1]
    out["sum_xx"] = gene_sums(xf, xk, xk, n_features)[1]
    out["sum_xy"], out["sum_yy"] = gene_sums(yf, x_of_y, yk, n_features)
    return out


def metrics(n, sum_x, sum_y, sum_xx, sum_yy, sum_xy):
    """(pearson, disp_full, disp), None where undefined; exact integers up to the one conversion to double each"""
    num = n * sum_xy - sum_x * sum_y
    dx, dy = n * sum_xx - sum_x ** 2, n * sum_yy - sum_y ** 2
    assert dx >= 0 and dy >= 0
    pearson = None if dx == 0 or dy == 0 else float(num) / (math.sqrt(float(dx)) * math.sqrt(float(dy)))
    disp_full = None if n < 2 or sum_x == 0 else float(dx) / (float(n - 1) * float(sum_x))
    disp = None if n < 2 or sum_y == 0 else float(dy) / (float(n - 1) * float(sum_y))
    return pearson, disp_full, disp


def _all_metrics(n, mom):
    return [metrics(n, mom["sum_x"][g], mom["sum_y"][g], mom["sum_xx"][g], mom["sum_yy"][g], mom["sum_xy"][g]) for g in range(len(mom["sum_x"]))]


def _f(v):
    return "NA" if v is None else "%.6f" % v


def gene_rows(names, n, mom):
    """the fields of every row of gene_fidelity.tsv.gz"""
    m = _all_metrics(n, mom)
    return [[nm] + [str(mom[c][g]) for c in INT_COLUMNS] + [_f(v) for v in m[g]] for g, nm in enumerate(names)]


def hvg(n, mom):
    """(K, A, B, overlap): the two rankings as lists of 0-based gene indices, the overlap None when K == 0"""
    m = _all_metrics(n, mom)
    a = sorted((g for g in range(len(m)) if m[g][1] is not None), key=lambda g: (-m[g][1], g))
    b = sorted((g for g in range(len(m)) if m[g][2] is not None), key=lambda g: (-m[g][2], g))
    K = min(HVG_TOP, len(a))
    A, B = a[:K], b[:min(K, len(b))]
    return K, A, B, (len(set(A) & set(B)) / K if K else None)


def summary_fields(lead, seed, n, mom):
    """the fields of a row of <verb>_gene_fidelity.tsv"""
    m = _all_metrics(n, mom)
    pe = sorted(p for p, _, _ in m if p is not None)
    stats = [R.median(pe), pe[int(math.floor(0.1 * (len(pe) - 1)))], sum(pe) / len(pe)] if pe else [None] * 3
    K, _, _, overlap = hvg(n, mom)
    genes_full = sum(1 for v in mom["sum_x"] if v > 0)
    return list(lead) + [str(seed), str(n), str(genes_full), str(len(pe))] + [_f(v) for v in stats] + [str(K), _f(overlap)]


def assert_fields(got, want, n_exact, what=""):
    """the first n_exact fields and every later integer or NA field exactly, the floats within TOL absolute"""
    assert len(got) == len(want), (what, got, want)
    assert got[:n_exact] == want[:n_exact], (what, got, want)
    for g, w in zip(got[n_exact:], want[n_exact:]):
        if "." not in w or "." not in g:
            assert g == w, (what, got, want)
        else:
            assert len(g.split(".")[1]) == 6 and abs(float(g) - float(w)) <= TOL, (what, got, want)


full_matrix = R.full_matrix
