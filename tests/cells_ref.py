"""The reference for `--cells` of sweep and cap, and the fixtures of its tests.

numpy restates the per-cell reads and the copy-number histogram twice: from (ukeys, ncopy) in the fixture layout of
tests/sortreduce_ref.py (cell = key >> CS, non-NULL flag = bit 26) — what fastf_dev_copy_summary reads — and from the oracle's
-u rows (umi_cell / umi_ncopy / umi_text, a NULL row is the one whose text is NULL) — what the commands must print.  The fixture
builders are shared by tests/test_cells_host.py (the census, without a GPU) and tests/test_gpu_cells.py."""
import numpy as np

import sortreduce_ref as S
from sweep_ref import parse_matrix

U = np.uint64
BINS = 32                                                    # FASTF_COPY_BINS
NN_BIT = S.FS - 1                                            # bit 26: the blob is not NULL
CUS = 256                                                    # an MI355X; the launch is 2 workgroups of 4 waves per CU
PAD = 1000                                                   # rows behind *d_nrows that must not be read


def launch_waves(cus=CUS):
    return 2 * cus * 4


def summary(cell, ncopy, nonnull, n_cells):
    """(reads, null_reads, single — int64[n_cells] — and hist as a list of BINS + 1 python ints) by the rules of the header"""
    c = np.asarray(cell, dtype=np.int64); k = np.asarray(ncopy, dtype=np.int64); nn = np.asarray(nonnull).astype(bool)
    ok = (c >= 1) & (c <= n_cells)
    reads, nulls, single = (np.zeros(n_cells, np.int64) for _ in range(3))
    np.add.at(reads, c[ok] - 1, k[ok])
    np.add.at(nulls, c[ok & ~nn] - 1, k[ok & ~nn])
    np.add.at(single, c[ok & nn & (k == 1)] - 1, 1)
    kk = k[nn & (k >= 1)]
    hist = [int((kk == b).sum()) for b in range(1, BINS)] + [int((kk >= BINS).sum()), int(kk[kk >= BINS].sum())]
    return reads, nulls, single, hist


class Layout:
    """feature shift, cell shift and the largest cell a key of the layout holds; the flag sits below the feature"""
    def __init__(self, fs, cs, cell_bits):
        self.fs, self.cs, self.max_cell = fs, cs, (1 << cell_bits) - 1


FIXTURE = Layout(S.FS, S.CS, 10)                             # 1000 cells x 500 features, 12 bases
BIG = Layout(27, 36, 17)                                     # 70 000 cells x 500 features, 12 bases: [cell 17][feature 9][1][24][2]


def from_keys(ukeys, ncopy, n_cells, lay=FIXTURE):
    ukeys = np.asarray(ukeys, np.uint64)
    return summary((ukeys >> U(lay.cs)).astype(np.int64), ncopy, (ukeys >> U(lay.fs - 1)) & U(1), n_cells)


def from_oracle(ora, n_cells):
    """from O.run_bam2db(..., umi_copies=True)"""
    nn = np.array([t != b"NULL" for t in ora["umi_text"]], dtype=bool)
    return summary(ora["umi_cell"], ora["umi_ncopy"], nn, n_cells)


def table_row(lead, seed, reads, nulls, single, hist):
    """the fields of a <verb>_cells.tsv row; lead: the first two columns as text"""
    med = "%.1f" % (float(np.median(reads)) if len(reads) else 0.0)
    return list(lead) + [str(seed), str(int(reads.sum())), str(int(nulls.sum())), str(sum(hist[:BINS])), str(int(single.sum())), med] + [str(h) for h in hist]


def point_lines(barcodes_txt: bytes, matrix_txt: bytes, reads, nulls, single):
    """the lines of a decompressed cells.tsv.gz: umis and genes per cell from the point's matrix, as sweep.tsv's medians take them"""
    names = barcodes_txt.decode().split("\n")
    assert names[-1] == ""
    names = names[:-1]
    _, _, n_cells, _, cell, count = parse_matrix(matrix_txt)
    assert n_cells == len(names) == len(reads)
    upc = np.zeros(n_cells, np.int64); np.add.at(upc, cell - 1, count)
    gpc = np.zeros(n_cells, np.int64); np.add.at(gpc, (cell - 1)[count >= 1], 1)
    out = ["barcode\treads\tnull_umi_reads\tumis\tgenes\tsingleton_umis\tsaturation"]
    for i, nm in enumerate(names):
        sat = "%.6f" % (1.0 - float(upc[i]) / float(reads[i])) if reads[i] else "0.000000"
        out.append("\t".join([nm, str(int(reads[i])), str(int(nulls[i])), str(int(upc[i])), str(int(gpc[i])), str(int(single[i])), sat]))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# fixtures: sorted distinct keys with chosen n_copy
# ---------------------------------------------------------------------------------------------------------------------
def make_keys(cell, nonnull=None, feature=None, lay=FIXTURE):
    """ascending distinct keys of the fixture layout for the given (non-decreasing) cells: within a cell the NULL rows first, one
    per feature, then the UMIs 0, 1, 2, … of feature `feature`"""
    cell = np.asarray(cell, np.int64)
    n = len(cell)
    assert (np.diff(cell) >= 0).all() and (n == 0 or (cell.min() >= 0 and cell.max() <= lay.max_cell))
    nonnull = np.ones(n, bool) if nonnull is None else np.asarray(nonnull, bool)
    start = np.r_[0, np.flatnonzero(np.diff(cell)) + 1] if n else np.zeros(0, np.int64)
    rank = np.arange(n) - np.repeat(start, np.diff(np.r_[start, n]))          # place of the row in its cell
    key = cell.astype(np.uint64) << U(lay.cs)
    f = np.full(n, 3 if feature is None else feature, np.int64)
    # NULL rows: feature = rank + 1 (below feature 3's UMIs only while few: asserted by the sort check), no flag
    nul = ~nonnull
    assert not nul.any() or (rank[nul] < 2).all()
    key = np.where(nul, key | ((rank + 1).astype(np.uint64) << U(lay.fs)),
                   key | (f.astype(np.uint64) << U(lay.fs)) | (U(1) << U(lay.fs - 1)) | (rank.astype(np.uint64) << U(2)) | U(3))
    assert rank.max(initial=0) < 1 << 24
    assert (np.diff(key.astype(np.int64)) > 0).all(), "fixture keys must ascend strictly"
    return key.astype(np.uint64)


def _rng(name):
    return np.random.default_rng(sum(name.encode()) * 977 + len(name))


def row_counts(cus=CUS):
    w = launch_waves(cus)
    return [0, 1, 63, 64, 65, w * 64 - 1, w * 64 + 1]


N_CELLS = [1, 3, 1000, 70_000]


def layout_of(name):
    return BIG if name.endswith("_70000") else FIXTURE


def fixture(name, cus=CUS):
    """(ukeys u64[], ncopy u32[], n_cells) of the fixture `name`, in the layout layout_of(name): the fixture engine's, or — the
    list of 70 000 cells — the layout of an engine with that many cells
      rows_<n>_<n_cells>   n rows over the cells 1 .. n_cells at random (sorted), n_copy 1 .. 5 mostly and 40 now and then, NULL
                           rows at the head of the odd cells
      one_cell             a launch's waves x 64 + 1 rows of cell 2: the carry crosses every span edge
      one_row_each         cells 1 .. 1000, exactly one row each
      gaps                 n_cells 1000 with rows on cells 3-5, 400, 998 alone: no rows at the front, in the middle, at n_cells
      lane63               waves x 128 rows; cells of two rows on lane 63 of a turn and lane 0 of the next, inside a span and across spans
      copies               n_copy 1, 31, 32, 33 and 2^31 in separate cells, a tail sum past 2^32
      hot_bin              100 001 rows, all n_copy == 1
      out_of_range         n_cells 3 with rows on cells 0, 1, 3, 4 and 1023"""
    rng = _rng(name)
    if name.startswith("rows_"):
        _, n, n_cells = name.split("_"); n = int(n); n_cells = int(n_cells)
        cell = np.sort(rng.integers(1, n_cells + 1, size=n))
        start = np.r_[True, np.diff(cell) != 0] if n else np.zeros(0, bool)
        nonnull = ~(start & (cell % 2 == 1))
        k = rng.integers(1, 6, size=n)
        k[rng.random(n) < 0.02] = 40
    elif name == "one_cell":
        n, n_cells = launch_waves(cus) * 64 + 1, 3
        cell = np.full(n, 2); nonnull = np.ones(n, bool); nonnull[0] = False
        k = rng.integers(1, 4, size=n)
    elif name == "one_row_each":
        n_cells = 1000
        cell = np.arange(1, 1001); nonnull = rng.random(1000) < 0.8
        k = rng.integers(1, 4, size=1000)
    elif name == "gaps":
        n_cells = 1000
        cell = np.sort(np.concatenate([rng.integers(3, 6, size=150), np.full(70, 400), np.full(5, 998)]))
        nonnull = np.ones(len(cell), bool)
        k = rng.integers(1, 4, size=len(cell))
    elif name == "lane63":
        # waves x 128 rows: every wave walks two turns.  Cells of two rows on (lane 63, lane 0 of the next turn) inside a span — the
        # carry — and across a span edge — the atomics —, long cells between them
        n, n_cells = launch_waves(cus) * 128, 1000
        cuts = sorted({63, 65, 127, 129} | {128 * j + 63 for j in (5, 100)} | {128 * j + 65 for j in (5, 100)} | {128 * 7 + 127, 128 * 7 + 129})
        cell = np.zeros(n, np.int64); cell[cuts] = 1
        cell = np.cumsum(cell) + 1
        nonnull = np.ones(n, bool)
        k = rng.integers(1, 4, size=n)
    elif name == "copies":
        n_cells = 1000
        vals = [1, 31, 32, 33, 1 << 31, 1 << 31, (1 << 31) + 5, 2, 33]
        cell = np.arange(10, 10 + len(vals)); nonnull = np.ones(len(vals), bool)
        k = np.array(vals, np.int64)
    elif name == "hot_bin":
        n, n_cells = 100_001, 1000
        cell = np.sort(rng.integers(1, 1001, size=n)); nonnull = np.ones(n, bool)
        k = np.ones(n, np.int64)
    elif name == "out_of_range":
        n_cells = 3
        cell = np.concatenate([np.full(4, 0), np.full(5, 1), np.full(6, 3), np.full(7, 4), np.full(70, 1023)])
        nonnull = np.ones(len(cell), bool); nonnull[[0, 4, 9, 15, 22]] = False
        k = rng.integers(1, 4, size=len(cell)); k[-3:] = 50
    else:
        raise KeyError(name)
    return make_keys(cell, nonnull, lay=layout_of(name)), np.asarray(k, np.int64).astype(np.uint32), n_cells


def fixture_names(cus=CUS):
    return (["rows_%d_%d" % (n, 1000) for n in row_counts(cus)] + ["rows_5001_%d" % c for c in N_CELLS] +
            ["one_cell", "one_row_each", "gaps", "lane63", "copies", "hot_bin", "out_of_range"])
