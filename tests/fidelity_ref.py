"""The reference for --fidelity: the seven integers per cell from two COO matrices with numpy, in Python ints, the two metrics by
the formula of include/fastf_amd.h, and the rows of fidelity.tsv.gz and <verb>_fidelity.tsv from them.

The full matrix of a (case, cell rate, seed) comes from the unchanged oracle the way cap_ref builds its points: every hit kept, the
oracle at rate_depth 1.0, no draw of 0xFFFFFFFF among the hits (level_ref.Hits asserts it and runs exactly that)."""
import math

import numpy as np

import level_ref

INT_COLUMNS = ("umis_full", "umis", "genes_full", "genes", "sum_xx", "sum_yy", "sum_xy")
TOL = 1.5e-6                                                # half a unit of the sixth printed decimal plus double rounding


def _keys(cell, feature):
    return (np.asarray(cell, np.uint64) << np.uint64(32)) | np.asarray(feature, np.uint64)


def moments(full, point, n_cells):
    """full, point: (feature, cell, count) ascending by (cell, feature), the point a row subset of the full rows.  Returns a dict of
    seven lists of Python ints, one entry per cell"""
    xf, xc, xk = (np.asarray(a, np.int64) for a in full)
    yf, yc, yk = (np.asarray(a, np.int64) for a in point)
    kx, ky = _keys(xc, xf), _keys(yc, yf)
    assert (kx[1:] > kx[:-1]).all() and (ky[1:] > ky[:-1]).all(), "rows not ascending by (cell, feature)"
    at = np.searchsorted(kx, ky)
    assert len(ky) == 0 or (at.max() < len(kx) and (kx[at] == ky).all()), "a point row without a partner"
    x_of_y = xk[at] if len(ky) else np.zeros(0, np.int64)
    out = {k: [0] * n_cells for k in INT_COLUMNS}

    def add(name, cell, values):
        acc = np.zeros(n_cells, dtype=object)
        np.add.at(acc, cell - 1, values.astype(object))
        out[name] = [int(v) for v in acc]
    add("umis_full", xc, xk); add("umis", yc, yk)
    add("genes_full", xc, (xk >= 1).astype(np.int64)); add("genes", yc, (yk >= 1).astype(np.int64))
    add("sum_xx", xc, xk.astype(object) * xk.astype(object)); add("sum_yy", yc, yk.astype(object) * yk.astype(object))
    add("sum_xy", yc, x_of_y.astype(object) * yk.astype(object))
    return out


def metrics(umis_full, umis, sum_xx, sum_yy, sum_xy, G):
    """(pearson, cosine), None where undefined; exact integers up to the one conversion to double"""
    num = G * sum_xy - umis_full * umis
    dx, dy = G * sum_xx - umis_full ** 2, G * sum_yy - umis ** 2
    assert dx >= 0 and dy >= 0
    pearson = None if dx == 0 or dy == 0 else float(num) / (math.sqrt(float(dx)) * math.sqrt(float(dy)))
    cosine = None if sum_xx == 0 or sum_yy == 0 else float(sum_xy) / (math.sqrt(float(sum_xx)) * math.sqrt(float(sum_yy)))
    return pearson, cosine


def _f(v):
    return "NA" if v is None else "%.6f" % v


def cell_rows(names, mom, G):
    """the fields of every row of fidelity.tsv.gz"""
    rows = []
    for k, nm in enumerate(names):
        ints = [mom[c][k] for c in INT_COLUMNS]
        p, c = metrics(mom["umis_full"][k], mom["umis"][k], mom["sum_xx"][k], mom["sum_yy"][k], mom["sum_xy"][k], G)
        rows.append([nm] + [str(v) for v in ints] + [_f(p), _f(c)])
    return rows


def median(v):
    v = sorted(v)
    n = len(v)
    return v[n // 2] if n & 1 else (v[n // 2 - 1] + v[n // 2]) / 2.0


def summary_fields(lead, seed, mom, G):
    """the fields of a row of <verb>_fidelity.tsv"""
    n_cells = len(mom["umis"])
    pc = [metrics(mom["umis_full"][k], mom["umis"][k], mom["sum_xx"][k], mom["sum_yy"][k], mom["sum_xy"][k], G) for k in range(n_cells)]
    defined = [(p, c) for p, c in pc if p is not None]
    assert all(c is not None for _, c in defined)
    if defined:
        pe = sorted(p for p, _ in defined)
        stats = [median(pe), pe[int(math.floor(0.1 * (len(pe) - 1)))], sum(pe) / len(pe), median([c for _, c in defined])]
    else:
        stats = [None] * 4
    su, suf, sg, sgf = (sum(mom[k]) for k in ("umis", "umis_full", "genes", "genes_full"))
    kept = [su / suf if suf else None, sg / sgf if sgf else None]
    return list(lead) + [str(seed), str(n_cells), str(len(defined))] + [_f(v) for v in stats + kept]


def assert_fields(got, want, n_exact, what=""):
    """the first n_exact fields exactly, the others within TOL absolute (NA exactly)"""
    assert len(got) == len(want), (what, got, want)
    assert got[:n_exact] == want[:n_exact], (what, got, want)
    for g, w in zip(got[n_exact:], want[n_exact:]):
        if w == "NA" or g == "NA":
            assert g == w, (what, got, want)
        else:
            assert len(g.split(".")[1]) == 6 and abs(float(g) - float(w)) <= TOL, (what, got, want)


_FULL = {}


def full_matrix(name, case, rate_cell, seed):
    """the full matrix of a pair as ((feature, cell, count), n_cells, the barcodes of the sampled cells, G)"""
    key = (name, float(np.float32(rate_cell)), seed)
    if key not in _FULL:
        h = level_ref.Hits(case, b"x.bam", rate_cell, seed)
        ora = h.ora_full
        names = ora["barcodes"].decode().split("\n")[:-1]
        G = len(ora["features"].decode().split("\n")) - 1
        _FULL[key] = ((ora["feature"].astype(np.int64), ora["cell"].astype(np.int64), ora["count"].astype(np.int64)), h.n_cells, names, G, h)
    return _FULL[key]
