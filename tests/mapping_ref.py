"""The reference for --mapping, brute force, by the text of include/fastf_amd.h: e_ij = <y_i, x_j> of the point's cells against ALL
full-depth cells over the genes of A as Python ints, the order of the candidates by cross-multiplication (e_ij^2 m_l against e_il^2 m_j,
then the cell index), M(i), self_dot, self_rank, hood, the votes over M — and the rows of mapping.tsv.gz and <verb>_mapping.tsv.  Doubles
only drop the candidates more than 1e-9 below the k-th cosine from the LIST, as neighbors_ref does; the rank is counted with exact ints
alone.  Below: the fixtures the host and the device tests share, each with its census (test_mapping_host runs it on the CPU)."""
import functools
import math

import numpy as np

import fidelity_ref as R
import labels_ref as LR
import neighbors_ref as N
import test_neighbors_host as H

K_DEFAULT = 15
NONE = 0xFFFFFFFF


def mapping_of_dense(mx, my, k):
    """(M lists ascending by index, self_dot, self_rank with None for NA, the full norms) of the dense full matrix mx and point matrix my"""
    n = mx.shape[0]
    if n == 0:
        return [], [], [], []
    small = max(int(mx.max()), int(my.max())) < 1 << 21 and max(int((mx * mx).sum(1).max()), int((my * my).sum(1).max())) < 1 << 62
    e = (my.astype(np.int64) @ mx.astype(np.int64).T) if small else my.dot(mx.T)
    m = [int(v) for v in (mx * mx).sum(1)]
    root = np.sqrt(np.array(m, dtype=np.float64))
    lists, sd, rank = [], [], []
    for i in range(n):
        row = [int(v) for v in e[i]]

        def before(j, l):                                   # -1: j precedes l
            a, b = row[j] ** 2 * m[l], row[l] ** 2 * m[j]
            return -1 if a > b or (a == b and j < l) else 1
        cand = [j for j in range(n) if j != i and row[j] > 0]
        sd.append(row[i])
        rank.append(sum(1 for j in cand if before(j, i) < 0) if row[i] > 0 else None)
        if len(cand) > k:
            cos = np.array([row[j] / root[j] for j in cand])       # (|y_i| is the same for all of them)
            floor = np.sort(cos)[-k] * (1 - 1e-9)
            cand = [j for j, c in zip(cand, cos) if c >= floor]
        lists.append(sorted(sorted(cand, key=functools.cmp_to_key(before))[:k]))
    return lists, sd, rank, m


def mapping(full, point, n_cells, genes, k=K_DEFAULT):
    return mapping_of_dense(N.dense(full, n_cells, genes), N.dense(point, n_cells, genes), k)


def hood(lists, full_sets):
    return [len(set(a) & set(b)) for a, b in zip(lists, full_sets)]


def _f(v):
    return "NA" if v is None else "%.6f" % v


def cell_rows(barcodes, lists, sd, rank, full_sets, names=None, pred=None):
    hd = hood(lists, full_sets)
    return [[bc, str(sd[i]), "NA" if rank[i] is None else str(rank[i]), str(len(lists[i])), str(len(full_sets[i])), str(hd[i]),
             names[pred[i]] if names is not None else "NA"] for i, bc in enumerate(barcodes)]


def summary_fields(lead, seed, hvg_k, k, lists, sd, rank, full_sets, lab=None, votes=None):
    """votes: (pred, same, labelled, conf) of labels_ref.votes over the lists"""
    n = len(sd)
    rk = sorted(r for r in rank if r is not None)
    hd = [h / len(s) for h, s in zip(hood(lists, full_sets), full_sets) if s]
    out = list(lead) + [str(seed), str(n), str(hvg_k), str(k), str(len(rk))]
    if rk:
        out += [_f(sum(1 for r in rk if r == 0) / len(rk)), _f(sum(1 for r in rk if r < k) / len(rk)), _f(R.median(rk)), str(rk[int(math.floor(0.9 * (len(rk) - 1)))])]
    else:
        out += ["NA"] * 4
    out.append(_f(sum(hd) / len(hd) if hd else None))
    if lab is None:
        return out + ["NA", "NA"]
    ids = [i for i, x in enumerate(lab) if x >= 1]
    same, labelled = sum(votes[1][i] for i in ids), sum(votes[2][i] for i in ids)
    return out + [str(len(ids)), _f(same / labelled if labelled else None)]


# ---- fixtures: name -> (full rows, point rows, n_cells, n_features, genes of A in slot order, k); rows ascend by (cell, feature) ----
GENES6 = np.array([4, 0, 5, 2, 1, 3])


def _pair(mx, my, genes, nf, k, outside_x=None, outside_y=None):
    return H.rows_of_dense(np.asarray(mx, np.int64), genes, nf, outside_x), H.rows_of_dense(np.asarray(my, np.int64), genes, nf, outside_y), len(mx), nf, genes, k


def _thin(m, seed, keep=0.6):
    """a subsample: every unit of a count kept with probability `keep`"""
    return np.random.default_rng(seed).binomial(np.asarray(m, np.int64), keep)


def _random(n, K, k, seed, density=0.3, max_count=4, keep=0.6):
    rows, n, nf, genes, _ = H.random_fixture(n, K, k, seed, max_count=max_count, density=density)
    mx = N.dense(rows, n, genes).astype(np.int64)
    return rows, H.rows_of_dense(_thin(mx, seed + 1, keep), genes, nf), n, nf, genes, k


def _build(name):
    if name == "same":                                      # point == full; cell 7 copies cell 2, cell 30 is twice cell 11
        rng = np.random.default_rng(41)
        m = (rng.integers(1, 5, (40, 12)) * (rng.random((40, 12)) < 0.4)).astype(np.int64)
        m[7], m[30] = m[2], 2 * m[11]
        g = rng.permutation(15)[:12]
        return _pair(m, m, g, 15, 15)
    if name in ("duplicates", "duplicates_without"):        # x_0 == x_2; both queries are the same thinned vector.  _without: cell 2 has no counts
        v, w, u = [5, 3, 0, 2, 0, 1], [0, 4, 4, 0, 1, 0], [1, 0, 0, 6, 2, 0]
        y = [3, 2, 0, 1, 0, 0]
        mx = [v, w, v if name == "duplicates" else [0] * 6, u, [2, 2, 2, 2, 2, 2]]
        my = [y, [0, 2, 3, 0, 0, 0], y if name == "duplicates" else [0] * 6, [1, 0, 0, 3, 1, 0], [1, 1, 0, 1, 1, 1]]
        return _pair(mx, my, GENES6, 6, 3)
    if name == "scaled":                                    # k = 2: q's nearest is 2q, then v against 3v for the last slot (test_neighbors_host)
        q, v, c1, c3 = H.scaled_pair()
        lo, hi = (v, 3 * v) if c3 > c1 else (3 * v, v)
        mx = np.array([q, 2 * q, lo, hi, [0, 0, 0, 0, 0, 1]], np.int64)
        my = mx.copy(); my[1:] = _thin(mx[1:], 3)
        return _pair(mx, my, GENES6, 6, 2)
    if name == "outside_A":                                 # point cell 5 kept nothing inside A (it has counts outside)
        rows, n, nf, genes, k = H.random_fixture(33, 10, 15, 610)
        mx = N.dense(rows, n, genes).astype(np.int64)
        my = _thin(mx, 611); my[5] = 0
        others = [g for g in range(nf) if g not in set(genes.tolist())]
        return rows, H.rows_of_dense(my, genes, nf, [(5, others[0], 3), (5, others[1], 1)]), n, nf, genes, k
    if name == "misses_own_top":                            # y_0 kept one read, on the gene that is x_1's alone
        mx = [[9, 9, 1, 0, 0, 0], [0, 0, 5, 0, 0, 0], [1, 0, 0, 2, 0, 0]]
        my = [[0, 0, 1, 0, 0, 0], [0, 0, 2, 0, 0, 0], [1, 0, 0, 1, 0, 0]]
        return _pair(mx, my, GENES6, 6, 15)
    if name == "few":                                       # fewer than k candidates
        return _random(5, 6, 15, 620, density=0.6)
    if name == "k1":
        return _random(40, 20, 1, 630)
    if name == "k64":
        return _random(129, 40, 64, 640, density=0.5)
    if name.startswith("count"):                            # a full count at a plane edge, the point on one plane
        c = int(name[5:])
        rows, n, nf, genes, k = H.random_fixture(33, 33, 15, 400 + c % 97, plant=c)
        mx = N.dense(rows, n, genes).astype(np.int64)
        return rows, H.rows_of_dense(np.minimum(_thin(mx, 650 + c % 97, 0.7), 127), genes, nf), n, nf, genes, k
    if name == "three_by_two":                              # three planes against two
        rows, n, nf, genes, k = H.random_fixture(40, 40, 15, 500, max_count=40_000, density=0.5)
        mx = N.dense(rows, n, genes).astype(np.int64)
        return rows, H.rows_of_dense(np.minimum(_thin(mx, 660, 0.3), 16383), genes, nf), n, nf, genes, k
    if name == "point_bigger":                              # the point's norms above the full ones: no subsample, the call is general
        rows, n, nf, genes, k = H.random_fixture(33, 12, 15, 670)
        mx = N.dense(rows, n, genes).astype(np.int64)
        return rows, H.rows_of_dense(3 * mx + (mx > 0), genes, nf), n, nf, genes, k
    if name == "asymmetric":                                # e_ij != e_ji for most pairs: a swapped A/B operand or a transposed C/D map changes every list
        return _random(65, 33, 15, 680, density=0.5, max_count=9, keep=0.4)
    if name in ("zero_point", "zero_full"):
        rows, n, nf, genes, k = H.random_fixture(33, 10, 15, 690)
        z = np.zeros(0, np.uint32)
        return (rows, (z, z, z), n, nf, genes, k) if name == "zero_point" else ((z, z, z), rows, n, nf, genes, k)
    if name == "no_rows":
        z = np.zeros(0, np.uint32)
        return (z, z, z), (z, z, z), 5, 6, GENES6, 15
    raise KeyError(name)


FIXTURES = ("same", "duplicates", "duplicates_without", "scaled", "outside_A", "misses_own_top", "few", "k1", "k64") + \
    tuple("count%d" % c for c in H.PLANE_EDGES) + ("three_by_two", "point_bigger", "asymmetric", "zero_point", "zero_full", "no_rows")
_BUILT, _REFS = {}, {}


def fixture(name):
    if name not in _BUILT:
        _BUILT[name] = _build(name)
    return _BUILT[name]


def reference(name):
    """computed once, shared by the host and the device tests"""
    if name not in _REFS:
        full, point, n, nf, genes, k = fixture(name)
        _REFS[name] = mapping(full, point, n, genes, k)
    return _REFS[name]


def planes_needed(rows, genes):
    inside = np.isin(rows[0].astype(np.int64) - 1, genes)
    top = int(rows[2][inside].max()) if inside.any() else 0
    return 1 if top < 128 else 2 if top < 16384 else 3


def census():
    """every fixture hits the case it is there for"""
    lists, sd, rank, m = reference("same")
    full, point, n, nf, genes, k = fixture("same")
    mx = N.dense(full, n, genes)
    par = lambda i, j: int(mx[i].dot(mx[j])) ** 2 == m[i] * m[j] and m[i] > 0     # noqa: E731  (parallel vectors)
    assert [r for r in rank] == [sum(1 for j in range(i) if par(i, j)) if m[i] else None for i in range(n)]
    assert rank[7] == 1 and rank[2] == 0 and rank[30] == 1 and rank[11] == 0 and sum(1 for r in rank if r) == 2 and min(m) > 0
    assert min(len(s) for s in lists) == 15                 # the lists are full: the cut is exercised
    _, _, rank, _ = reference("duplicates")
    _, _, rank0, _ = reference("duplicates_without")
    assert rank[2] == rank[0] + 1                           # the identical full cell at the LOWER index is one more in front
    assert rank[0] == rank0[0] and rank[0] is not None      # the identical full cell at the HIGHER index changes nothing
    q, v, c1, c3 = H.scaled_pair()
    lists, sd, rank, m = reference("scaled")
    full, point, n, nf, genes, k = fixture("scaled")
    mx, my = N.dense(full, n, genes), N.dense(point, n, genes)
    e = lambda i, j: int(my[i].dot(mx[j]))                  # noqa: E731
    assert lists[0] == [1, 2] and rank[0] == 0              # the exact tie goes to the lower index; the larger double sits at index 3
    assert e(0, 2) ** 2 * m[3] == e(0, 3) ** 2 * m[2] and e(0, 3) / math.sqrt(m[3]) != e(0, 2) / math.sqrt(m[2]) and c1 != c3
    assert abs(c1 - c3) <= 2 * math.ulp(c1)
    lists, sd, rank, _ = reference("outside_A")
    assert sd[5] == 0 and rank[5] is None and lists[5] == [] and fixture("outside_A")[1][1].tolist().count(6) == 2
    assert sum(1 for r in rank if r is not None) >= 25
    lists, sd, rank, _ = reference("misses_own_top")
    assert sd[0] > 0 and rank[0] >= 1 and lists[0][0] == 1
    lists, _, _, _ = reference("few")
    assert 0 < max(len(s) for s in lists) < fixture("few")[5]
    assert fixture("k1")[5] == 1 and max(len(s) for s in reference("k1")[0]) == 1
    assert max(len(s) for s in reference("k64")[0]) == 64
    pairs = {name: (planes_needed(fixture(name)[1], fixture(name)[4]), planes_needed(fixture(name)[0], fixture(name)[4])) for name in FIXTURES}
    assert [pairs["count%d" % c] for c in H.PLANE_EDGES] == [(1, 1), (1, 2), (1, 2), (1, 3), (1, 3)] and pairs["three_by_two"] == (2, 3)
    assert max(reference("count%d" % H.PLANE_EDGES[-1])[3]) > 1 << 41
    full, point, n, nf, genes, k = fixture("point_bigger")
    mx, my = N.dense(full, n, genes), N.dense(point, n, genes)
    assert all(int(my[i].dot(my[i])) > int(mx[i].dot(mx[i])) for i in range(n) if mx[i].any())
    full, point, n, nf, genes, k = fixture("asymmetric")
    mx, my = N.dense(full, n, genes).astype(np.int64), N.dense(point, n, genes).astype(np.int64)
    e = my @ mx.T
    assert (e != e.T).sum() > 0.9 * n * (n - 1)             # e_ij != e_ji for most pairs
    assert reference("asymmetric")[0] != mapping(point, full, n, genes, k)[0]      # the operands swapped: other lists
    assert all(r is None for r in reference("zero_point")[2]) and all(r is None for r in reference("zero_full")[2])
    assert reference("no_rows")[0] == [[]] * 5
    for name in FIXTURES:
        full, point, n, nf, genes, k = fixture(name)
        for rows in (full, point):
            key = rows[1].astype(np.int64) << 32 | rows[0].astype(np.int64)
            assert (key[1:] > key[:-1]).all(), name
        assert max(reference(name)[3], default=0) < 1 << 42, name
