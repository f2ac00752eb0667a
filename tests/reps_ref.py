"""numpy restatement of the replicate tables of `fastF sweep` / `fastF cap` (--seeds, --reps): a row of <verb>_reps.tsv from the
rows of <verb>.tsv at the seeds of a grid point, the three per-gene accumulators of <verb>_gene_reps.tsv.gz, a row of
<verb>_genes_reps.tsv, and the order of the rows and the names of the point directories of a replicate run."""
import numpy as np

METRICS = ("sampled_reads", "sampled_valid_reads", "nnz", "umis", "saturation", "median_umis_per_cell", "median_genes_per_cell")
_FMT = {"saturation": "%.6f", "median_umis_per_cell": "%.1f", "median_genes_per_cell": "%.1f"}


def order(rates_cell, seeds, second):
    """[(rate_cell, seed, second)] as <verb>.tsv lists them: cell rates outer, the seeds as listed, then the verb's own list"""
    return [(rc, s, x) for rc in rates_cell for s in seeds for x in second]


def point_name(rate_cell, second, seed, caps=False):
    base = ("c%.3f_n%d" % (float(np.float32(rate_cell)), int(second))) if caps else \
           ("c%.3f_r%.3f" % (float(np.float32(rate_cell)), float(np.float32(second))))
    return "%s_s%d" % (base, seed)


def stat4(values, fmt="%d"):
    """[mean, sd, min, max] as text: mean and sample sd (divisor n - 1) in float64, two passes in list order, %.6f; `NA` at one value;
    min and max in the metric's own format"""
    v = [float(x) for x in values]
    n = len(v)
    total = 0.0
    for x in v:
        total += x
    mean = total / n
    ss = 0.0
    for x in v:
        ss += (x - mean) * (x - mean)
    sd = "%.6f" % np.sqrt(ss / (n - 1)) if n > 1 else "NA"
    lo, hi = min(v), max(v)
    if fmt == "%d":
        lo, hi = int(lo), int(hi)
    return ["%.6f" % mean, sd, fmt % lo, fmt % hi]


def metrics_of(matrix_fields):
    """the seven metrics of one <verb>.tsv row (its fields as text: the columns of sweep.tsv, cap.tsv's first twelve) recomputed in
    float64 from its integer columns where the table prints a rounded number: the saturation"""
    f = matrix_fields
    valid, nnz, umis = int(f[6]), int(f[7]), int(f[8])
    sat = 1.0 - umis / valid if valid else 0.0
    return [int(f[5]), valid, nnz, umis, sat, float(f[10]), float(f[11])]


def reps_row(first_two, rows):
    """the fields of a <verb>_reps.tsv row from the <verb>.tsv rows (lists of text fields) of its seeds in list order"""
    n_cells = {r[3] for r in rows}
    assert len(n_cells) == 1, "the replicates disagree on n_cells"
    m = [metrics_of(r) for r in rows]
    out = list(first_two) + [str(len(rows)), rows[0][3]]
    for k, name in enumerate(METRICS):
        out += stat4([x[k] for x in m], _FMT.get(name, "%d"))
    return out


def gene_accumulate(cells_per_gene_by_seed):
    """(reps_detected, cells_sum, cells_sumsq) — exact Python integers per gene — of the cells-per-gene arrays of the seeds"""
    n = len(cells_per_gene_by_seed[0])
    det, tot, sq = [0] * n, [0] * n, [0] * n
    for cells in cells_per_gene_by_seed:
        assert len(cells) == n
        for g, c in enumerate(cells):
            c = int(c)
            det[g] += c >= 1
            tot[g] += c
            sq[g] += c * c
    return det, tot, sq


def genes_reps_row(first_two, cells_per_gene_by_seed):
    det, _, _ = gene_accumulate(cells_per_gene_by_seed)
    n = len(cells_per_gene_by_seed)
    detected = [sum(1 for c in cells if int(c) >= 1) for cells in cells_per_gene_by_seed]
    return list(first_two) + [str(n)] + stat4(detected) + [str(sum(1 for d in det if d == n)), str(sum(1 for d in det if d >= 1))]


def close(a: str, b: str) -> bool:
    """two printed means or sds: equal text, or within 1e-6 absolute + 1e-9 relative (six printed decimals, sums in double over at
    most 64 values)"""
    if a == b:
        return True
    if "NA" in (a, b):
        return False
    x, y = float(a), float(b)
    return abs(x - y) <= 1e-6 + 1e-9 * max(abs(x), abs(y))


def assert_reps_row(got, want, what="", lead=4):
    """means and sds by close(), everything else as text; lead: the columns in front of the first mean (3 in <verb>_genes_reps.tsv)"""
    assert len(got) == len(want), (what, got, want)
    for i, (g, w) in enumerate(zip(got, want)):
        stat = lead <= i < lead + 4 * ((len(want) - lead) // 4) and (i - lead) % 4 in (0, 1)
        assert (close(g, w) if stat else g == w), (what, i, g, w)
