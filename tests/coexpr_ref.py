"""The co-expression partners by brute force in Python ints (the definition of include/fastf_amd.h): from a COO matrix
(feature 1-based, cell 1-based, count) and a slot map.  No numpy arithmetic and no floating point takes part in a result; floats
appear only in the census, to show what a float compare would have chosen.  The module ends with the fixtures of the tests and a
census of the cases they must contain."""
import math
import random
from fractions import Fraction
from functools import cmp_to_key

import numpy as np

NONE = 0xFFFF


def slot_map(genes, nf):
    sm = [NONE] * (nf + 1)
    for s, g in enumerate(genes):
        sm[g + 1] = s
    return np.array(sm, np.uint16)


def columns(rows, n, genes, nf):
    """m[slot][cell] as Python ints"""
    sm = slot_map(genes, nf)
    m = [[0] * n for _ in genes]
    for f, c, v in zip(*rows):
        f, c, v = int(f), int(c), int(v)
        if 1 <= f <= nf and 1 <= c <= n and sm[f] < len(genes):
            m[int(sm[f])][c - 1] = v
    return m


def sums(m, n):
    """(D, S): D[g][h] = sum_i m_ig m_ih, S[g] = sum_i m_ig"""
    K = len(m)
    S = [sum(col) for col in m]
    D = [[0] * K for _ in range(K)]
    for g in range(K):
        nz = [(i, v) for i, v in enumerate(m[g]) if v]
        for h in range(g, K):
            D[g][h] = D[h][g] = sum(v * m[h][i] for i, v in nz)
    return D, S


def candidates(D, S, n, g):
    """[(h, c, V_h)] with c > 0, in slot order"""
    K = len(S)
    out = []
    for h in range(K):
        c = n * D[g][h] - S[g] * S[h]
        if h != g and c > 0:
            out.append((h, c, n * D[h][h] - S[h] * S[h]))
    return out


def ordered(cands, bits=None):
    """the candidates in the order of the definition; bits: the products cut to that many bits (what a too narrow compare would do)"""
    if bits is None:
        return sorted(cands, key=lambda t: (-Fraction(t[1] * t[1], t[2]), t[0]))
    mask = (1 << bits) - 1

    def cmp(a, b):
        x, y = (a[1] * a[1] * b[2]) & mask, (b[1] * b[1] * a[2]) & mask
        return -1 if x > y or (x == y and a[0] < b[0]) else 1
    return sorted(cands, key=cmp_to_key(cmp))


def partner_sets(D, S, n, k, bits=None):
    """per slot the ascending list of its partners"""
    return [sorted(t[0] for t in ordered(candidates(D, S, n, g), bits)[:k]) for g in range(len(S))]


def max_q(D):
    return max((D[g][g] for g in range(len(D))), default=0)


def in_range(D, n):
    return n * max_q(D) < 1 << 63


def per_gene(full_sets, point_sets):
    kf = [len(a) for a in full_sets]
    kp = [len(b) for b in point_sets]
    sh = [len(set(a) & set(b)) for a, b in zip(full_sets, point_sets)]
    return kf, kp, sh


def summary_fields(lead, seed, n, k, kf, kp, sh):
    """the fields of one per-point row; the mean as a Fraction (compared within half a unit of the last printed digit)"""
    defined = [g for g in range(len(kf)) if kf[g]]
    mean = sum(Fraction(sh[g], kf[g]) for g in defined) / len(defined) if defined else None
    return list(lead) + [str(seed), str(n), str(len(kf)), str(k), str(len(defined)), str(sum(kf)), str(sum(kp)), str(sum(sh)), mean,
                         str(sum(1 for g in defined if 2 * sh[g] >= kf[g]))]


# ---- the fixtures: name -> (rows, n, nf, genes, k) ----
def _rows_of_columns(cols, genes):
    f, c, v = [], [], []
    for s, col in enumerate(cols):
        for i, x in enumerate(col):
            if x:
                f.append(genes[s] + 1); c.append(i + 1); v.append(x)
    return np.array(f, np.uint32), np.array(c, np.uint32), np.array(v, np.uint32)


def _random(seed, K, n, top, density, nf_extra=3):
    """K genes scattered over K + nf_extra features, counts up to top, and rows of features outside A and of cells outside 1 .. n"""
    r = random.Random(seed)
    nf = K + nf_extra
    genes = r.sample(range(nf), K)
    cols = [[r.randint(1, top) if r.random() < density else 0 for _ in range(n)] for _ in range(K)]
    f, c, v = _rows_of_columns(cols, genes)
    others = [g for g in range(nf) if g not in genes]
    extra_f = [others[0] + 1] * min(n, 3) + [genes[0] + 1, nf + 1, 0]
    extra_c = list(range(1, min(n, 3) + 1)) + [n + 1, 1, 1]
    rows = (np.concatenate([f, np.array(extra_f, np.uint32)]), np.concatenate([c, np.array(extra_c, np.uint32)]),
            np.concatenate([v, np.full(len(extra_f), 100, np.uint32)]))
    return rows, n, nf, genes, None


def _build():
    F = {}

    def put(name, cols, k, genes=None):
        genes = list(range(len(cols))) if genes is None else genes
        F[name] = (_rows_of_columns(cols, genes), len(cols[0]), max(genes) + 2, genes, k)

    # two identical columns straddle the cut at rank k: for slot 0 the slots 2 and 3 tie for the second place
    base = [3, 1, 4, 1, 5, 9, 2, 6, 5, 3]
    put("duplicates", [base, [3, 1, 4, 1, 5, 9, 2, 6, 5, 4], [2, 1, 4, 0, 5, 7, 2, 6, 1, 3], [2, 1, 4, 0, 5, 7, 2, 6, 1, 3], [1, 0, 0, 2, 1, 3, 0, 0, 9, 1]], 2)
    # slot 2 = 3 x slot 1: equal Pearson with slot 0; the doubles differ in the last bit and the larger sits at slot 2
    put("proportional", PROPORTIONAL, 1)
    put("zero_cov", [[1, 1, 0, 0], [1, 0, 1, 0], [2, 1, 0, 0]], 15)
    put("negative", [[2, 0, 2, 0, 1], [0, 3, 0, 3, 0], [3, 0, 2, 0, 2]], 15)
    put("degenerate", [[2, 2, 2, 2, 2, 2], [0, 0, 0, 0, 0, 0], [1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 6, 5], [0, 0, 1, 0, 0, 7]], 15, genes=[4, 1, 0, 6, 2])
    put("few_candidates", [[1, 2, 3, 0, 0, 1], [1, 2, 4, 0, 0, 1], [0, 2, 3, 1, 0, 1], [5, 0, 0, 3, 6, 0]], 15)
    put("one_gene", [[1, 0, 2, 5]], 15)
    put("one_cell", [[3], [2], [0]], 15)
    put("edges", [[127, 128, 16383, 16384, (1 << 21) - 1, 1, 0, 5], [128, 127, 16384, 16383, (1 << 21) - 1, 0, 1, 5], [1, 0, 127, 128, 16383, 16384, 0, 0],
                  [0, 0, 0, 0, 0, 0, 3, 1], [(1 << 21) - 1, 0, 0, 0, 0, 0, 0, 0]], 2)
    F["k1"] = _random(11, 40, 50, 6, 0.5)[:4] + (1,)
    F["k15"] = _random(12, 70, 65, 9, 0.4)[:4] + (15,)
    F["k64"] = _random(13, 129, 33, 200, 0.3)[:4] + (64,)
    F["wide"] = _random(WIDE_SEED, 24, 64, 1 << 20, 0.9)[:4] + (5,)
    F["empty"] = ((np.zeros(0, np.uint32),) * 3, 9, 6, [0, 3, 4], 15)
    return F


PROPORTIONAL = [[9, 1, 4, 1, 7, 7], [7, 6, 3, 1, 7, 0], [21, 18, 9, 3, 21, 0]]
WIDE_SEED = 0


FIXTURES = _build()
_REF = {}


def reference(name):
    """(D, S, sets) of a fixture, computed once"""
    if name not in _REF:
        rows, n, nf, genes, k = FIXTURES[name]
        D, S = sums(columns(rows, n, genes, nf), n)
        _REF[name] = (D, S, partner_sets(D, S, n, k))
    return _REF[name]


def census():
    """what the fixtures contain, by name of the case -> the fixtures showing it"""
    found = {"wide_changes_a_set": [], "tie_by_slot": [], "zero_cov": [], "negative_cov": [], "zero_variance": [], "float_differs": []}
    for name, (rows, n, nf, genes, k) in FIXTURES.items():
        D, S, sets = reference(name)
        K = len(S)
        assert in_range(D, n), name
        for g in range(K):
            cands = ordered(candidates(D, S, n, g))
            if any(t[1] * t[1] * u[2] >= 1 << 128 for t in cands for u in cands) and partner_sets(D, S, n, k, 128)[g] != sets[g]:
                found["wide_changes_a_set"].append(name)
            if len(cands) > k and cands[k - 1][1] ** 2 * cands[k][2] == cands[k][1] ** 2 * cands[k - 1][2]:
                found["tie_by_slot"].append(name)
                Vg = n * D[g][g] - S[g] * S[g]
                a, b = [t[1] / math.sqrt(float(Vg) * float(t[2])) for t in (cands[k - 1], cands[k])]
                if b > a:
                    found["float_differs"].append(name)
            for h in range(K):
                c = n * D[g][h] - S[g] * S[h]
                if h != g and c == 0 and D[g][h]:
                    found["zero_cov"].append(name)
                if c < 0:
                    found["negative_cov"].append(name)
            if n * D[g][g] == S[g] * S[g]:
                found["zero_variance"].append(name)
    return {k: sorted(set(v)) for k, v in found.items()}
