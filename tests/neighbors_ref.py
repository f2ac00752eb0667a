"""The reference for --neighbors, brute force: the dot products of the cells over the genes of A as Python ints, the order of the
candidates of a cell by cross-multiplication (d_ij^2 n_l against d_il^2 n_j, then the cell index) — no float takes part until the
printed ratio — and the rows of neighbors.tsv.gz and <verb>_neighbors.tsv by the text of include/fastf_amd.h.  A is ranked by
gene_fidelity_ref.hvg from the sums of the full matrix."""
import functools
import math

import numpy as np

import fidelity_ref as R
import gene_fidelity_ref as G

K_DEFAULT = 15
NONE = 0xFFFFFFFF


def dense(rows, n_cells, genes):
    """the n_cells x len(genes) matrix (object dtype, Python ints) of (feature, cell, count) rows restricted to genes (0-based, slot order)"""
    slot = {int(g): s for s, g in enumerate(genes)}
    m = np.zeros((n_cells, max(len(genes), 1)), dtype=object)
    for f, c, v in zip(*(np.asarray(a, np.int64) for a in rows)):
        if 1 <= c <= n_cells and int(f) - 1 in slot:
            m[int(c) - 1, slot[int(f) - 1]] += int(v)
    return m


def sets_of_dense(m, k):
    """(neighbour lists ascending by index, norms) of a dense matrix of Python ints.  The dot products are exact (int64 where they fit,
    Python ints otherwise).  The order is decided by cross-multiplied Python ints alone; doubles only drop the candidates of a cell
    whose cosine lies more than 1e-9 below its k-th largest — a double cosine is off by a few 1e-16, so none of them can be among the
    first k"""
    n = m.shape[0]
    small = n == 0 or (int(m.max()) < 1 << 21 and int((m * m).sum(1).max()) < 1 << 62)
    d = (m.astype(np.int64) @ m.astype(np.int64).T) if small else m.dot(m.T)
    norms = [int(d[i, i]) for i in range(n)]
    root = np.sqrt(np.array(norms, dtype=np.float64))
    out = []
    for i in range(n):
        row = [int(v) for v in d[i]]
        valid = [j for j in range(n) if j != i and row[j] > 0]
        if len(valid) > k:
            cos = np.array([row[j] / (root[i] * root[j]) for j in valid])
            floor = np.sort(cos)[-k] - 1e-9
            valid = [j for j, c in zip(valid, cos) if c >= floor]

        def before(j, l):                                   # -1: j precedes l
            a, b = row[j] ** 2 * norms[l], row[l] ** 2 * norms[j]
            return -1 if a > b or (a == b and j < l) else 1
        out.append(sorted(sorted(valid, key=functools.cmp_to_key(before))[:k]))
    return out, norms


def neighbor_sets(rows, n_cells, genes, k=K_DEFAULT):
    return sets_of_dense(dense(rows, n_cells, genes), k)


def hvg_of_rows(rows, n_cells, n_features):
    """A of a full matrix: gene indices (0-based) in rank order"""
    f, _, v = (np.asarray(a, np.int64) for a in rows)
    one = np.ones(len(v), np.int64)
    mom = {"sum_x": G.gene_sums(f, v, one, n_features)[0], "sum_xx": G.gene_sums(f, v, v, n_features)[1]}
    mom["sum_y"], mom["sum_yy"], mom["sum_xy"] = mom["sum_x"], mom["sum_xx"], mom["sum_xx"]
    return G.hvg(n_cells, mom)[1]


def per_cell(full_sets, point_sets):
    """(k_full, k_point, shared) lists"""
    return ([len(a) for a in full_sets], [len(b) for b in point_sets], [len(set(a) & set(b)) for a, b in zip(full_sets, point_sets)])


def _f(v):
    return "NA" if v is None else "%.6f" % v


def cell_rows(barcodes, k_full, k_point, shared):
    return [[bc, str(a), str(b), str(s), _f(s / a if a else None)] for bc, a, b, s in zip(barcodes, k_full, k_point, shared)]


def summary_fields(lead, seed, hvg_k, k, k_full, k_point, shared):
    n = len(k_full)
    ov = sorted(s / a for a, s in zip(k_full, shared) if a)
    stats = [R.median(ov), ov[int(math.floor(0.1 * (len(ov) - 1)))], sum(ov) / len(ov)] if ov else [None] * 3
    return list(lead) + [str(seed), str(n), str(hvg_k), str(k), str(len(ov))] + [_f(v) for v in stats] + [_f(sum(k_point) / n if n else None)]


assert_fields = G.assert_fields
full_matrix = R.full_matrix
