"""The reference for `--genes` of sweep and cap, and the fixtures of its tests.

numpy restates the per-gene summary (np.bincount on feature - 1: with the counts as weights, and over the rows with count >= 1), the
rows of sweep_genes.tsv / cap_genes.tsv and the three files of a point from the decompressed matrix.mtx of that point.  The fixture
builders are shared by tests/test_genes_host.py (the census: every fixture holds what it was built to hold, asserted without a GPU)
and tests/test_gpu_genes.py (fastf_dev_gene_summary on them)."""
import numpy as np

from sweep_ref import parse_matrix

# the launch of fastf_dev_gene_summary as analysis_entry.hpp sizes it (gene_kernels.hpp), on the 256 CUs of an MI355X
LDS_GENES, THREADS, MAX_RANGES, ITEMS, CUS = 16384, 1024, 8, 4, 256
N_FEATURES = [1, 3, 16384, 16385, 36601, 140_000]
PAD = 1000                                                   # rows behind *d_nnz that must not be read


def per_gene(feature, count, n_features):
    """(cells per gene, umis per gene) as int64; rows whose feature is outside 1 .. n_features add nothing"""
    f = np.asarray(feature, dtype=np.int64)
    k = np.asarray(count, dtype=np.int64)
    ok = (f >= 1) & (f <= n_features)
    f, k = f[ok] - 1, k[ok]
    umis = np.zeros(n_features, np.int64)
    np.add.at(umis, f, k)                                    # (bincount's weights are doubles: exact only below 2^53, and slower to trust)
    assert n_features == 0 or (umis == np.bincount(f, weights=k, minlength=n_features).astype(np.int64)).all()
    cells = np.bincount(f[k >= 1], minlength=n_features).astype(np.int64)
    return cells, umis


def table_fields(cells, umis):
    """the four numbers of a genes row"""
    return [str(int((cells >= 1).sum())), str(int((cells >= 3).sum())), str(int((cells >= 10).sum())), str(int(umis.max()) if len(umis) else "0")]


def expected_genes_row(matrix_txt: bytes, lead, seed):
    """lead: the first two columns as text"""
    _, nf, _, feature, _, count = parse_matrix(matrix_txt)
    cells, umis = per_gene(feature, count, nf)
    return list(lead) + [str(seed)] + table_fields(cells, umis), cells, umis


def feature_ids(features_txt: bytes):
    """the first field of every line of a decompressed features.tsv"""
    lines = features_txt.decode().split("\n")
    assert lines[-1] == ""
    return [ln.split("\t")[0] for ln in lines[:-1]]


def launch(n_features, lds_ranges_env=None):
    """(lds form?, ranges, workgroups per range, waves that share the rows) of the launch for n_features"""
    n_ranges = (n_features + LDS_GENES - 1) // LDS_GENES
    max_ranges = MAX_RANGES if lds_ranges_env is None else min(int(lds_ranges_env), MAX_RANGES)
    if n_ranges <= max_ranges:
        per_cu = 2 if min(n_features, LDS_GENES) * 8 <= 80 * 1024 else 1
        groups = max(1, per_cu * CUS // n_ranges)
        return True, n_ranges, groups, groups * (THREADS // 64)
    return False, 1, 2 * CUS, 2 * CUS * (THREADS // 64)


def row_counts(n_features):
    """0, 1, 63, 64, 65, and one less and one more than a multiple of the launch's waves x 64 (both forms), and of a whole turn of
    the LDS form (waves x 64 x ITEMS) where that stays small"""
    out = [0, 1, 63, 64, 65]
    for env in (None, "0"):
        w = launch(n_features, env)[3]
        out += [w * 64 - 1, w * 64 + 1]
    w = launch(n_features)[3]
    if w * 64 * ITEMS <= 600_000:
        out += [w * 64 * ITEMS - 1, w * 64 * ITEMS + 1]
    return sorted(set(out))


def _rng(name, n_features):
    return np.random.default_rng(sum(name.encode()) * 131 + n_features)


def fixture(name, n_features):
    """(feature u32[], count u32[]) of the fixture `name` for a list of n_features genes.
      rows_<n>   n rows, genes uniform over the list, a fifth of the counts 0
      edges      rows (some with count 0) on genes 1, 16 384, 16 385, the first and last gene of every range of 16 384 and the last
                 gene of the list, on features 0, n_features + 1 and 2^32 - 1, among random rows
      one_gene   100 001 rows, all on one gene (16 385, or the last gene of a shorter list), a tenth of the counts 0
      big_sum    a gene whose sum passes 2^31 while the sum of all counts stays below 2^32"""
    rng = _rng(name, n_features)
    if name.startswith("rows_"):
        n = int(name[5:])
        f = rng.integers(1, n_features + 1, size=n)
        k = rng.integers(0, 5, size=n)
    elif name == "edges":
        special = [1, 16384, 16385, n_features, 0, n_features + 1, 0xFFFFFFFF]
        for lo in range(0, n_features, LDS_GENES):
            special += [lo + 1, min(lo + LDS_GENES, n_features)]
        special = [g for g in special if g <= n_features + 1 or g == 0xFFFFFFFF]
        sp = np.repeat(np.array(special, dtype=np.int64), 7)
        f = np.concatenate([rng.integers(1, n_features + 1, size=3000), sp])
        k = np.concatenate([rng.integers(0, 4, size=3000), np.tile([3, 0, 1, 2, 0, 5, 1], len(special))])
        order = rng.permutation(len(f))
        f, k = f[order], k[order]
    elif name == "one_gene":
        n = 100_001
        f = np.full(n, min(16385, n_features))
        k = rng.integers(0, 10, size=n).clip(0, 3)
        k[rng.random(n) < 0.1] = 0
    elif name == "big_sum":
        g = min(2, n_features)
        f = np.concatenate([np.full(3, g), rng.integers(1, n_features + 1, size=197)])
        k = np.concatenate([np.full(3, 900_000_000), rng.integers(0, 4, size=197)])
    else:
        raise KeyError(name)
    return f.astype(np.uint32), k.astype(np.uint32)


def fixture_names(n_features):
    return ["rows_%d" % n for n in row_counts(n_features)] + ["edges", "one_gene", "big_sum"]
