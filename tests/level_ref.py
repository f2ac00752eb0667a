"""The reference for one point of `fastF level`, built on the unchanged oracle as tests/cap_ref.py is.

A threshold vector T (one integer in [0, 2^32] per sampled cell) is applied as cap_ref applies its own: keep = mt_stream < T[cell],
the has-CB flag of every hit that is not kept cleared, the oracle run on the masked records at rate_depth 1.0.  U_k(T) is then a
column sum of the oracle's matrix.

T[k] = max { T : U_k(T) <= M } is computed in numpy for all cells at once.  U_k changes only where T passes a draw of one of cell k's
hits, so min { T : U_k(T) > M } is d + 1 for one of those draws d and T[k] = d: the search bisects, per cell, the INDEX into the
cell's sorted draws (about log2 of the deepest cell's hits oracle runs instead of 32), probing every cell that is still open at once
and every other cell at 0.  The result is then PROVED against the definition with two more oracle runs, which do not depend on how T
was found: at T every column sum is <= M, and at min(T + 1, 2^32) every capped cell's column sum is > M."""
import re

import numpy as np

from oracle import oracle as O
from cap_ref import hits_of, realised
from sweep_ref import expected_row

FULL = np.uint64(1 << 32)


class Hits:
    """what every point of one (case, cell rate, seed) shares: the hits, their draws, U_k(2^32)"""

    def __init__(self, case, bam_label, rate_cell, seed):
        self.case, self.label, self.seed = case, bam_label, seed
        self.rc = float(np.float32(rate_cell))
        self.probe, self.cell, self.h, self.skip = hits_of(case, self.rc, seed, bam_label)
        self.n_cells = len(self.h)
        self.H = int(self.h.sum())
        self.stream = O.mt_stream(seed, self.H, self.skip).astype(np.uint64)
        assert not (self.stream == np.uint64(0xFFFFFFFF)).any(), "seed %d draws 0xFFFFFFFF among the first %d: pick another" % (seed, self.H)
        self.hit_at = np.nonzero(self.cell > 0)[0]
        self.hit_cell = self.cell[self.hit_at] - 1                        # 0-based cell of every hit, in file order
        # the draws of every cell, ascending: cell k's are sd[off[k] : off[k + 1]]
        order = np.lexsort((self.stream, self.hit_cell))
        self.sd = self.stream[order]
        self.off = np.searchsorted(self.hit_cell[order], np.arange(self.n_cells + 1))
        self.ora_full, _, self.u_full = self.run(np.full(self.n_cells, FULL, np.uint64))
        assert self.ora_full["sampled"] == self.H

    def masked_flags(self, T):
        keep = self.stream < np.asarray(T, np.uint64)[self.hit_cell]
        flags = np.array(self.case.flags, dtype=np.uint8, copy=True)
        flags[self.hit_at[~keep]] &= np.uint8(~O.HAS_CB & 0xFF)
        return flags, keep

    def run(self, T, umi_copies=False):
        """(the oracle's run with hit i of cell k kept iff draw[i] < T[k], keep, the column sums U_k(T))"""
        c = self.case
        flags, keep = self.masked_flags(T)
        ora = O.run_bam2db(c.bt, c.ft, flags, c.xf, c.cb, c.gx, c.ub, self.rc, 1.0, self.seed, self.label, umi_copies)
        assert ora["sampled"] == int(keep.sum()) and ora["total"] == len(flags)
        u = np.zeros(self.n_cells, np.int64)
        np.add.at(u, ora["cell"].astype(np.int64) - 1, ora["count"].astype(np.int64))
        return ora, keep, u

    def thresholds(self, M):
        """T[k] by bisection of the index into each capped cell's sorted draws, every open cell probed in the same oracle run"""
        capped = self.u_full > M
        n = (self.off[1:] - self.off[:-1]).astype(np.int64)
        lo = np.zeros(self.n_cells, np.int64)                             # U(sd[i] + 1) <= M for every i < lo
        hi = np.where(capped, n - 1, 0)                                   # U(sd[hi] + 1) > M: the largest draw + 1 keeps every hit
        runs = 0
        while True:
            open_ = capped & (lo < hi)
            if not open_.any():
                break
            mid = (lo + hi) // 2
            T = np.zeros(self.n_cells, np.uint64)
            T[open_] = self.sd[self.off[:-1][open_] + mid[open_]] + np.uint64(1)
            _, _, u = self.run(T)
            gt = u > M
            hi = np.where(open_ & gt, mid, hi)
            lo = np.where(open_ & ~gt, mid + 1, lo)
            runs += 1
            assert runs <= 40
        T = np.full(self.n_cells, FULL, np.uint64)
        T[capped] = self.sd[self.off[:-1][capped] + lo[capped]]
        return T, capped


def point(hits: Hits, M):
    """dict: matrix / barcodes / features (expected bytes), row (the level.tsv fields), T, u_full, u (the thresholds.tsv.gz columns),
    thresholds (its decompressed bytes), cells_capped, keep, ora"""
    M = int(M)
    T, capped = hits.thresholds(M)
    ora, keep, u = hits.run(T)
    # the proof against the definition
    assert (u <= M).all(), "a column sum above M at T"
    _, _, u1 = hits.run(np.minimum(T + np.uint64(1), FULL))
    assert (u1[capped] > M).all(), "a capped cell whose T + 1 still fits M: T is not the maximum"
    assert (T[~capped] == FULL).all() and (u[~capped] == hits.u_full[~capped]).all()
    sampled = int(keep.sum())
    frac = realised(sampled, hits.H)
    matrix, n_sub = re.subn(rb'(%\t"rate_depth": )[^,\n]*,', lambda m: m.group(1) + b"%.3f," % frac, ora["matrix"], count=1)
    assert n_sub == 1
    n_capped = int(capped.sum())
    row = expected_row(matrix, hits.rc, 0.0, hits.seed)
    row[1] = str(M)
    row += [str(hits.H), str(n_capped), "%.6f" % frac]
    names = ora["barcodes"].decode().split("\n")[:-1]
    assert len(names) == hits.n_cells
    text = "barcode\tthreshold\tumis_full\tumis\n" + "".join("%s\t%d\t%d\t%d\n" % (nm, int(t), int(a), int(b)) for nm, t, a, b in zip(names, T, hits.u_full, u))
    return dict(matrix=matrix, barcodes=ora["barcodes"], features=ora["features"], hits=hits.H, cells_capped=n_capped, sampled=sampled,
                realised=frac, row=row, T=T, u_full=hits.u_full, u=u, capped=capped, keep=keep, thresholds=text.encode(), ora=ora)
