"""Fixtures for the device half of --coexpression on top of coexpr_ref.FIXTURES: gene and cell counts around the 32 x 32 tile of the
Gram kernel and the 64 genes of a selection workgroup, one fixture on each side of every digit-plane boundary, a tie at the cut between
slots 63 and 64, and `saturated`, whose accumulators are as full as three planes can make them.  name -> (rows, n, nf, genes, k) as in
coexpr_ref; the references are computed once.  The module ends with a census of what the fixtures must contain."""
import numpy as np

import coexpr_ref as R

TOP3 = (1 << 21) - 1


def planes_of(rows, n, nf, genes):
    """the digit planes the largest count among the rows with a slot needs"""
    m = R.columns(rows, n, genes, nf)
    top = max((v for col in m for v in col), default=0)
    return 1 if top < 1 << 7 else 2 if top < 1 << 14 else 3


def _build():
    F = {}

    def put(name, cols, k, genes=None):
        genes = list(range(len(cols))) if genes is None else genes
        F[name] = (R._rows_of_columns(cols, genes), len(cols[0]), max(genes) + 2, genes, k)

    # K and n around the tile (32), two tiles (64) and the workgroup of the selection (64): name K<genes>_n<cells>
    F["K31_n33"] = R._random(31, 31, 33, 6, 0.5)[:4] + (15,)
    F["K32_n31"] = R._random(32, 32, 31, 100, 0.6)[:4] + (15,)
    F["K33_n65"] = R._random(33, 33, 65, 300, 0.4)[:4] + (15,)
    F["K64_n33"] = R._random(64, 64, 33, 9, 0.5)[:4] + (15,)
    F["K65_n65"] = R._random(65, 65, 65, 12, 0.45)[:4] + (15,)
    F["K97_n31"] = R._random(97, 97, 31, 20000, 0.5)[:4] + (15,)
    # one fixture on each side of a plane boundary: the largest count is the name
    shape = [[1, 0, 2, 3, 1, 0, 5], [2, 1, 0, 3, 1, 1, 4], [0, 3, 1, 0, 2, 2, 0], [4, 0, 1, 1, 0, 3, 1]]
    for top in (127, 128, 16383, 16384, TOP3):
        cols = [list(c) for c in shape]
        cols[0][3] = top; cols[1][3] = top - 1; cols[2][0] = top
        put("top%d" % top, cols, 2)
    # the cut of gene 0 at k = 2 falls between slots 63 and 64, which hold one column: 63 stays, 64 (of the second 64 genes) goes
    base, near, dup = [3, 1, 4, 1, 5, 9, 2, 6, 5, 3], [3, 1, 4, 1, 5, 9, 2, 6, 5, 4], [2, 1, 4, 0, 5, 7, 2, 6, 1, 3]
    cols = [[0] * 10 if s % 2 == 0 else [2] * 10 for s in range(66)]
    cols[0], cols[1], cols[63], cols[64] = base, near, dup, list(dup)
    put("tie_63_64", cols, 2)
    return F


FIXTURES = _build()
# every count the largest three planes hold, n = 96 — D = n (2^21 - 1)^2 everywhere: the fullest accumulators a chunk of 96 cells can have.
# n * max Q = 96^2 (2^21 - 1)^2 < 2^56 is inside the range rule; both genes are constant, so V = 0 and nobody has a partner
SATURATED = (R._rows_of_columns([[TOP3] * 96, [TOP3] * 96], [0, 1]), 96, 3, [0, 1], 15)
ALL = dict(R.FIXTURES)
ALL.update(FIXTURES)
KS = (1, 15, 64)
_REF, _SETS = {}, {}


def fixture(name):
    return SATURATED if name == "saturated" else ALL[name]


def reference(name):
    """(D, S) of a fixture as Python ints, computed once"""
    if name not in _REF:
        rows, n, nf, genes, _ = fixture(name)
        _REF[name] = R.sums(R.columns(rows, n, genes, nf), n)
    return _REF[name]


def sets(name, k):
    """the partner sets of a fixture for k, computed once"""
    if (name, k) not in _SETS:
        D, S = reference(name)
        _SETS[(name, k)] = R.partner_sets(D, S, fixture(name)[1], k)
    return _SETS[(name, k)]


def point_rows(rows):
    """a grid point made of a fixture: every count above 1 lowered by one, every third row dropped"""
    keep = np.arange(len(rows[0])) % 3 != 2
    return rows[0][keep], rows[1][keep], (rows[2] - (rows[2] > 1))[keep]


def as_lists(idx, cnt):
    return [[int(v) for v in idx[g, :cnt[g]]] for g in range(len(cnt))]


def census():
    """each fixture contains what it is named for"""
    for name, (rows, n, nf, genes, k) in FIXTURES.items():
        D, S = reference(name)
        assert R.in_range(D, n), name
        if name.startswith("K"):
            assert (len(genes), n) == tuple(int(x[1:]) for x in name.split("_")), name
        if name.startswith("top"):
            top = int(name[3:])
            assert max(int(v) for v in rows[2]) == top and planes_of(rows, n, nf, genes) == (1 if top < 128 else 2 if top < 16384 else 3), name
    assert {len(f[3]) for f in FIXTURES.values()} >= {31, 32, 33, 64, 65, 97} and {f[1] for f in FIXTURES.values()} >= {31, 33, 65}
    assert {planes_of(*FIXTURES[n][:4]) for n in ("K31_n33", "K33_n65", "K97_n31")} == {1, 2, 3}
    # the tie: ranks 2 and 3 of gene 0 are slots 63 and 64 with equal products; the set keeps 63
    rows, n, nf, genes, k = FIXTURES["tie_63_64"]
    D, S = reference("tie_63_64")
    cands = R.ordered(R.candidates(D, S, n, 0))
    assert k == 2 and [t[0] for t in cands[:3]] == [1, 63, 64] and cands[1][1] ** 2 * cands[2][2] == cands[2][1] ** 2 * cands[1][2]
    assert sets("tie_63_64", 2)[0] == [1, 63]
    # saturated: the sums are what three full planes give
    rows, n, nf, genes, _ = SATURATED
    D, S = reference("saturated")
    assert D == [[n * TOP3 * TOP3] * 2] * 2 and S == [n * TOP3] * 2 and R.in_range(D, n) and planes_of(rows, n, nf, genes) == 3
    assert 3 * 96 * 127 * 127 < 1 << 31 and sets("saturated", 15) == [[], []]
    assert "wide" in ALL and "saturated" not in ALL
    return True
