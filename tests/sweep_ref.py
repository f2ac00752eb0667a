"""numpy restatement of a sweep.tsv row: every column recomputed from the decompressed matrix.mtx of the point."""
import re

import numpy as np


def parse_matrix(txt: bytes):
    """(counters [total, sampled, valid], n_features, n_cells, feature, cell, count) of a matrix.mtx"""
    lines = txt.decode().split("\n")
    assert lines[-1] == ""
    head = [ln for ln in lines if ln.startswith("%")]
    body = [ln for ln in lines[:-1] if not ln.startswith("%")]
    cnt = [int(re.search(r'"%s": (\d+)' % k, "\n".join(head)).group(1)) for k in ("total_n_FastQ", "sampled_n_FastQ", "sampled_valid_n_FastQ")]
    nf, nb, nnz = (int(x) for x in body[0].split())
    rows = np.array([[int(x) for x in ln.split()] for ln in body[1:]], dtype=np.int64).reshape(-1, 3)
    assert len(rows) == nnz
    return cnt, nf, nb, rows[:, 0], rows[:, 1], rows[:, 2]


def expected_row(matrix_txt: bytes, rate_cell, rate_depth, seed):
    cnt, _, n_cells, _, cell, count = parse_matrix(matrix_txt)
    upc = np.bincount(cell - 1, weights=None if not len(cell) else count, minlength=n_cells).astype(np.int64) if len(cell) else np.zeros(n_cells, np.int64)
    gpc = np.bincount((cell - 1)[count >= 1], minlength=n_cells) if len(cell) else np.zeros(n_cells, np.int64)
    umis = int(count.sum())
    sat = "%.6f" % (1.0 - umis / cnt[2]) if cnt[2] else "0.000000"
    med = lambda a: "%.1f" % (float(np.median(a)) if len(a) else 0.0)  # noqa: E731
    return ["%.3f" % float(np.float32(rate_cell)), "%.3f" % float(np.float32(rate_depth)), str(seed), str(n_cells), str(cnt[0]), str(cnt[1]),
            str(cnt[2]), str(len(cell)), str(umis), sat, med(upc), med(gpc)]
