"""Python mirror of `fastF sweep` (include/fastf_amd.h: fastf_sweep and its host pieces): bam2db over a grid of
(cell rate, depth rate) points from one decode of the BAM.  Nothing here computes results: every call lands in the library."""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import Coo, UmiRows

SUMMARY_ONLY = 1      # FASTF_SWEEP_SUMMARY_ONLY
GENES = 2             # FASTF_SWEEP_GENES
CELLS = 8             # FASTF_SWEEP_CELLS
FIDELITY = 32         # FASTF_SWEEP_FIDELITY
GENE_FIDELITY = 128   # FASTF_SWEEP_GENE_FIDELITY
HVG_TOP = 2000        # FASTF_HVG_TOP
NEIGHBORS = 512       # FASTF_SWEEP_NEIGHBORS
NEIGHBORS_K = 15      # FASTF_NEIGHBORS_K
COEXPRESSION = 4096   # FASTF_SWEEP_COEXPRESSION
COEXPRESSION_K = 15   # FASTF_COEXPR_K
COEXPRESSION_CHUNK = 8192   # FASTF_COEXPR_CHUNK
LABELS_MAX = 255      # FASTF_LABELS_MAX
MARKERS_MAX = 2000    # FASTF_MARKERS_MAX
COPY_BINS = 32        # FASTF_COPY_BINS
COLUMNS = ("rate_cell", "rate_depth", "seed", "n_cells", "total_reads", "sampled_reads", "sampled_valid_reads", "nnz", "umis",
           "saturation", "median_umis_per_cell", "median_genes_per_cell")
GENES_COLUMNS = ("rate_cell", "rate_depth", "seed", "genes_detected", "genes_min_cells_3", "genes_min_cells_10", "max_gene_umis")
CELLS_TAIL_COLUMNS = (("seed", "valid_reads", "null_umi_reads", "umis", "singleton_umis", "median_reads_per_cell")
                      + tuple("copies_%d" % k for k in range(1, COPY_BINS)) + ("copies_%d_plus" % COPY_BINS, "reads_copies_%d_plus" % COPY_BINS))
CELLS_COLUMNS = ("rate_cell", "rate_depth") + CELLS_TAIL_COLUMNS
FIDELITY_TAIL_COLUMNS = ("seed", "n_cells", "cells_defined", "median_pearson", "p10_pearson", "mean_pearson", "median_cosine", "umis_kept", "genes_kept")
FIDELITY_COLUMNS = ("rate_cell", "rate_depth") + FIDELITY_TAIL_COLUMNS
POINT_FIDELITY_COLUMNS = ("barcode", "umis_full", "umis", "genes_full", "genes", "sum_xx", "sum_yy", "sum_xy", "pearson", "cosine")     # <point dir>/fidelity.tsv.gz
GENE_FIDELITY_TAIL_COLUMNS = ("seed", "n_cells", "genes_full", "genes_defined", "median_pearson", "p10_pearson", "mean_pearson", "hvg_k", "hvg_overlap")
GENE_FIDELITY_COLUMNS = ("rate_cell", "rate_depth") + GENE_FIDELITY_TAIL_COLUMNS
POINT_GENE_FIDELITY_COLUMNS = ("feature", "sum_x", "sum_y", "cells_full", "cells", "sum_xx", "sum_yy", "sum_xy", "pearson", "disp_full", "disp")     # <point dir>/gene_fidelity.tsv.gz
NEIGHBORS_TAIL_COLUMNS = ("seed", "n_cells", "hvg_k", "k", "cells_defined", "median_overlap", "p10_overlap", "mean_overlap", "mean_k_point")
NEIGHBORS_COLUMNS = ("rate_cell", "rate_depth") + NEIGHBORS_TAIL_COLUMNS
POINT_NEIGHBORS_COLUMNS = ("barcode", "k_full", "k_point", "shared", "overlap")     # <point dir>/neighbors.tsv.gz
COEXPRESSION_TAIL_COLUMNS = ("seed", "n_cells", "hvg_k", "k", "genes_defined", "sum_k_full", "sum_k_point", "sum_shared", "mean_kept", "genes_half_kept")
COEXPRESSION_COLUMNS = ("rate_cell", "rate_depth") + COEXPRESSION_TAIL_COLUMNS
POINT_COEXPRESSION_COLUMNS = ("gene", "k_full", "k_point", "shared")     # the per-gene rows
MAPPING_TAIL_COLUMNS = ("seed", "n_cells", "hvg_k", "k", "cells_defined", "self_top1", "self_topk", "median_self_rank", "p90_self_rank", "mean_hood",
                        "cells_labelled", "accuracy_map")
MAPPING_COLUMNS = ("rate_cell", "rate_depth") + MAPPING_TAIL_COLUMNS
POINT_MAPPING_COLUMNS = ("barcode", "self_dot", "self_rank", "k_map", "k_full", "hood", "pred_map")     # <point dir>/mapping.tsv.gz
MAPPING_K = 15
PSEUDOTIME_TAIL_COLUMNS = ("seed", "n_cells", "k", "cells_valued") + tuple("%s_%s" % (c, m) for m in ("full", "point", "map") for c in ("cells", "conc", "disc", "tau", "shift"))
PSEUDOTIME_COLUMNS = ("rate_cell", "rate_depth") + PSEUDOTIME_TAIL_COLUMNS
POINT_PSEUDOTIME_COLUMNS = ("barcode", "rank", "est_full", "valued_full", "est_point", "valued_point", "est_map", "valued_map")     # <point dir>/pseudotime.tsv.gz
PTIME_TILE = 1024         # FASTF_PTIME_TILE: the tile edge of the device census
PTIME_OUT_WORDS = 7       # conc disc tie_e tie_t tie_both cells shift_sum
MAPPING_NO_RANK = 0xFFFFFFFF
LABELS_TAIL_COLUMNS = ("seed", "n_cells", "k", "n_labels", "cells_labelled", "agree_full", "agree_point", "accuracy_full", "accuracy_point", "kept",
                       "purity_full", "purity_point")
LABELS_COLUMNS = ("rate_cell", "rate_depth") + LABELS_TAIL_COLUMNS
LABEL_CLASSES_TAIL_COLUMNS = ("seed", "label", "cells", "correct_full", "correct_point", "predicted_full", "predicted_point")
LABEL_CLASSES_COLUMNS = ("rate_cell", "rate_depth") + LABEL_CLASSES_TAIL_COLUMNS
POINT_LABELS_COLUMNS = ("barcode", "label", "pred_full", "pred_point", "same_full", "labelled_full", "same_point", "labelled_point")     # <point dir>/labels.tsv.gz
MARKERS_TAIL_COLUMNS = ("seed", "label", "n_in", "n_out", "top", "kept", "auc_full_mean", "auc_point_mean")
MARKERS_COLUMNS = ("rate_cell", "rate_depth") + MARKERS_TAIL_COLUMNS
POINT_MARKERS_COLUMNS = ("label", "gene", "rank_full", "rank_point", "auc_full", "auc_point", "det_in_full", "det_out_full", "det_in_point", "det_out_point",
                         "mean_in_point")     # <point dir>/markers.tsv.gz
POINT_CELLS_COLUMNS = ("barcode", "reads", "null_umi_reads", "umis", "genes", "singleton_umis", "saturation")     # <point dir>/cells.tsv.gz


def _floats(v):
    a = np.ascontiguousarray(v, dtype=np.float32)
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


def _flags(summary_only, genes, cells, fidelity=False, gene_fidelity=False, neighbors=False, coexpression=False):
    return ((SUMMARY_ONLY if summary_only else 0) | (GENES if genes else 0) | (CELLS if cells else 0) | (FIDELITY if fidelity else 0)
            | (GENE_FIDELITY if gene_fidelity else 0) | (NEIGHBORS if neighbors else 0) | (COEXPRESSION if coexpression else 0))


def _markers_n(markers) -> int:
    """N of markers=N as the u32 the C call takes: what is no integer or does not fit goes over as 0, which the call refuses by name"""
    try:
        n = int(markers)
    except (TypeError, ValueError):
        return 0
    return n if 0 <= n < (1 << 32) and n == markers else 0


def _caps(values):
    """a list of caps as the (array, pointer) pair _grid_call takes"""
    a = np.ascontiguousarray(values, dtype=np.uint64)
    return a, a.ctypes.data


def _grid_call(verb, bam, out, barcodes, features, rates_cell, values, seeds, seed, flags, labels, markers, mapping, pseudotime):
    """the C call of <verb>() (seeds None: the run at `seed`) and <verb>_reps() (the replicate run over seeds); values: the verb's list as
    (array, pointer).  It is fastf_<verb>_pseudotime, the most general entry point, with None for a path that is absent.  Two requests
    are refused through the call that names them: markers=N with no N the call takes goes to fastf_<verb>_markers as 0, and an empty
    list of seeds with no option beside it to fastf_<verb>_reps (with one, n_seeds == 0 is the run at seed 0, as the header says)"""
    L = _lib.lib()
    enc = lambda p: None if p is None else os.fspath(p).encode()  # noqa: E731
    rc, prc = _floats(rates_cell)
    sd = None if seeds is None else np.ascontiguousarray([int(x) % (1 << 32) for x in seeds], dtype=np.uint32)
    grid = (enc(bam), enc(out), enc(barcodes), enc(features), prc, len(rc), values[1], len(values[0]), None if sd is None else sd.ctypes.data,
            0 if sd is None else len(sd))
    if markers is not None and _markers_n(markers) == 0:
        _lib.check(getattr(L, "fastf_%s_markers" % verb)(*grid, flags, seed % (1 << 32), enc(labels), 0))
    elif sd is not None and not len(sd) and labels is None and markers is None and not mapping and pseudotime is None:
        _lib.check(getattr(L, "fastf_%s_reps" % verb)(*grid, flags))
    else:
        _lib.check(getattr(L, "fastf_%s_pseudotime" % verb)(*grid, flags, seed % (1 << 32), enc(labels), 0 if markers is None else _markers_n(markers),
                                                            int(bool(mapping)), enc(pseudotime)))


def sweep(bam, out, barcodes, features, rates_cell, rates_depth, seed: int = 926, summary_only: bool = False, genes: bool = False,
          cells: bool = False, fidelity: bool = False, gene_fidelity: bool = False, neighbors: bool = False, labels=None, markers=None, coexpression: bool = False, mapping: bool = False,
               pseudotime=None):
    """`fastF sweep -b bam -a barcodes -f features -o out -c rates_cell -r rates_depth -s seed [--summary-only] [--genes] [--cells]`;
    returns the rows of out/sweep.tsv as dicts of strings (read_table); genes=True also leaves out/sweep_genes.tsv
    (read_genes_table), out/sweep_gene_cells.tsv.gz and a genes.tsv.gz per point directory; cells=True also leaves
    out/sweep_cells.tsv (read_cells_table) and a cells.tsv.gz per point directory; fidelity=True also leaves out/sweep_fidelity.tsv
    (read_fidelity_table) and a fidelity.tsv.gz per point directory (read_point_fidelity): every point against the full-depth data
    of the same cells; gene_fidelity=True the same comparison per gene: out/sweep_gene_fidelity.tsv (read_gene_fidelity_table) and a
    gene_fidelity.tsv.gz per point directory (read_point_gene_fidelity); neighbors=True the comparison between the cells:
    out/sweep_neighbors.tsv (read_neighbors_table) and a neighbors.tsv.gz per point directory (read_point_neighbors); labels=<path>
    (`--labels`: one barcode<TAB>label per line) the label votes of those neighbours: out/sweep_labels.tsv (read_labels_table),
    out/sweep_label_classes.tsv (read_label_classes_table) and labels.tsv.gz (read_point_labels), label_confusion.tsv.gz per point directory;
    markers=N (`--markers`, with labels) the N best marker genes per label by exact AUC: out/sweep_markers.tsv (read_markers_table) and a
    markers.tsv.gz per point directory (read_point_markers); coexpression=True (`--coexpression`) the comparison between the genes:
    out/sweep_coexpr.tsv (read_coexpression_table) and a coexpr.tsv.gz per point directory (read_point_coexpression); mapping=True
    (`--mapping`) every point cell looked up among the full-depth cells: out/sweep_mapping.tsv (read_mapping_table) and a mapping.tsv.gz
    per point directory (read_point_mapping); pseudotime=<path> (`--pseudotime`: one barcode<TAB>value per line) the order of the cells along
    that value, estimated back from the neighbour sets: out/sweep_pseudotime.tsv (read_pseudotime_table) and a pseudotime.tsv.gz per point
    directory (read_point_pseudotime)"""
    _grid_call("sweep", bam, out, barcodes, features, rates_cell, _floats(rates_depth), None, seed,
               _flags(summary_only, genes, cells, fidelity, gene_fidelity, neighbors, coexpression), labels, markers, mapping, pseudotime)
    return read_table(os.path.join(os.fspath(out), "sweep.tsv"))


def sweep_reps(bam, out, barcodes, features, rates_cell, rates_depth, seeds, summary_only: bool = False, genes: bool = False,
               cells: bool = False, fidelity: bool = False, gene_fidelity: bool = False, neighbors: bool = False, labels=None, markers=None, coexpression: bool = False, mapping: bool = False,
               pseudotime=None):
    """`fastF sweep ... --seeds seeds`: a replicate run (one seed included) — the points in out/<point>_s<seed>/, one row of
    out/sweep.tsv per (cell rate, seed, depth rate), which are returned (read_table), and out/sweep_reps.tsv (read_reps_table);
    genes=True leaves out/sweep_genes.tsv, out/sweep_genes_reps.tsv (read_genes_reps_table) and out/sweep_gene_reps.tsv.gz"""
    _grid_call("sweep", bam, out, barcodes, features, rates_cell, _floats(rates_depth), seeds, 0,
               _flags(summary_only, genes, cells, fidelity, gene_fidelity, neighbors, coexpression), labels, markers, mapping, pseudotime)
    return read_table(os.path.join(os.fspath(out), "sweep.tsv"))


def read_fidelity_table(path, columns=FIDELITY_COLUMNS):
    """the rows of sweep_fidelity.tsv as dicts of strings"""
    return read_cells_table(path, columns)


def read_point_fidelity(path):
    """the rows of a point's fidelity.tsv.gz as dicts of strings"""
    import gzip
    lines = gzip.decompress(open(path, "rb").read()).decode().split("\n")
    assert lines[0].split("\t") == list(POINT_FIDELITY_COLUMNS) and lines[-1] == ""
    return [dict(zip(POINT_FIDELITY_COLUMNS, ln.split("\t"))) for ln in lines[1:-1]]


def fidelity_header(verb: str = "") -> str:
    """the header of fidelity.tsv.gz, or with verb "sweep" / "cap" / "level" of <verb>_fidelity.tsv"""
    return getattr(_lib.lib(), "fastf_%sfidelity_header" % (verb + "_" if verb else ""))().decode()


def fidelity_row(barcode, umis_full, umis, genes_full, genes, sum_xx, sum_yy, sum_xy, n_features) -> str:
    """one row of fidelity.tsv.gz (with its newline) from the seven integers of a cell and the number of features"""
    buf = C.create_string_buffer(512)
    _lib.check(_lib.lib().fastf_fidelity_row(barcode.encode() if isinstance(barcode, str) else barcode, int(umis_full), int(umis), int(genes_full),
                                             int(genes), int(sum_xx), int(sum_yy), int(sum_xy), int(n_features), buf, len(buf)))
    return buf.value.decode()


def fidelity_summary_row(rate_cell, rate_depth, seed, umis_full, umis, genes_full, genes, sum_xx, sum_yy, sum_xy, n_features, list_value: int = 0) -> str:
    """one row of <verb>_fidelity.tsv (with its newline); list_value >= 1: that integer in the second column (cap, level)"""
    a64 = [np.ascontiguousarray(a, dtype=np.uint64) for a in (umis_full, umis, sum_xx, sum_yy, sum_xy)]
    g = [np.ascontiguousarray(a, dtype=np.uint32) for a in (genes_full, genes)]
    n = len(a64[0])
    assert all(len(a) == n for a in a64 + g)
    buf = C.create_string_buffer(640)
    _lib.check(_lib.lib().fastf_fidelity_summary_row(float(rate_cell), float(rate_depth), int(list_value), int(seed) % (1 << 32), a64[0].ctypes.data,
                                                     a64[1].ctypes.data, g[0].ctypes.data, g[1].ctypes.data, a64[2].ctypes.data, a64[3].ctypes.data,
                                                     a64[4].ctypes.data, n, int(n_features), buf, len(buf)))
    return buf.value.decode()


def fidelity_from_coo(full, point, n_cells: int):
    """(sum_xy u64[n_cells], sum_yy u64[n_cells]) of a point COO joined with the full COO — each a (feature, cell, count) triple ascending by
    (cell, feature): the host form of Engine.dev_fidelity; raises FastfError on a point row without a partner"""
    p32 = C.POINTER(C.c_uint32)
    keep, coos = [], []
    for f, c, k in (full, point):
        arrs = [np.ascontiguousarray(a, dtype=np.uint32) for a in (f, c, k)]
        assert len(arrs[0]) == len(arrs[1]) == len(arrs[2])
        keep.append(arrs)
        coos.append(Coo(arrs[0].ctypes.data_as(p32), arrs[1].ctypes.data_as(p32), arrs[2].ctypes.data_as(p32), len(arrs[0])))
    sxy, syy = np.zeros(max(n_cells, 1), np.uint64), np.zeros(max(n_cells, 1), np.uint64)
    _lib.check(_lib.lib().fastf_fidelity_from_coo(C.byref(coos[0]), C.byref(coos[1]), n_cells, sxy.ctypes.data, syy.ctypes.data))
    return sxy[:n_cells], syy[:n_cells]


def read_gene_fidelity_table(path, columns=GENE_FIDELITY_COLUMNS):
    """the rows of sweep_gene_fidelity.tsv as dicts of strings"""
    return read_cells_table(path, columns)


def read_point_gene_fidelity(path):
    """the rows of a point's gene_fidelity.tsv.gz as dicts of strings"""
    import gzip
    lines = gzip.decompress(open(path, "rb").read()).decode().split("\n")
    assert lines[0].split("\t") == list(POINT_GENE_FIDELITY_COLUMNS) and lines[-1] == ""
    return [dict(zip(POINT_GENE_FIDELITY_COLUMNS, ln.split("\t"))) for ln in lines[1:-1]]


def gene_fidelity_header(verb: str = "") -> str:
    """the header of gene_fidelity.tsv.gz, or with verb "sweep" / "cap" / "level" of <verb>_gene_fidelity.tsv"""
    return getattr(_lib.lib(), "fastf_%sgene_fidelity_header" % (verb + "_" if verb else ""))().decode()


def gene_fidelity_metrics(n_cells, sum_x, sum_y, sum_xx, sum_yy, sum_xy):
    """(pearson, disp_full, disp) of a gene over n_cells sampled cells, None where undefined"""
    v = [C.c_double(), C.c_double(), C.c_double()]
    d = _lib.lib().fastf_gene_fidelity_metrics(int(n_cells), int(sum_x), int(sum_y), int(sum_xx), int(sum_yy), int(sum_xy), *[C.byref(x) for x in v])
    return tuple(v[k].value if d & (1 << k) else None for k in range(3))


def gene_fidelity_row(feature, n_cells, sum_x, sum_y, cells_full, cells, sum_xx, sum_yy, sum_xy) -> str:
    """one row of gene_fidelity.tsv.gz (with its newline) from the seven integers of a gene and the number of sampled cells"""
    buf = C.create_string_buffer(640)
    _lib.check(_lib.lib().fastf_gene_fidelity_row(feature.encode() if isinstance(feature, str) else feature, int(n_cells), int(sum_x), int(sum_y),
                                                  int(cells_full), int(cells), int(sum_xx), int(sum_yy), int(sum_xy), buf, len(buf)))
    return buf.value.decode()


def gene_fidelity_summary_row(rate_cell, rate_depth, seed, n_cells, sum_x, sum_y, sum_xx, sum_yy, sum_xy, list_value: int = 0) -> str:
    """one row of <verb>_gene_fidelity.tsv (with its newline), the ranking of the highly variable genes included; list_value >= 1: that
    integer in the second column (cap, level)"""
    a = [np.ascontiguousarray(x, dtype=np.uint64) for x in (sum_x, sum_y, sum_xx, sum_yy, sum_xy)]
    n = len(a[0])
    assert all(len(x) == n for x in a)
    buf = C.create_string_buffer(640)
    _lib.check(_lib.lib().fastf_gene_fidelity_summary_row(float(rate_cell), float(rate_depth), int(list_value), int(seed) % (1 << 32), int(n_cells),
                                                          a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, a[4].ctypes.data, n,
                                                          buf, len(buf)))
    return buf.value.decode()


def gene_fidelity_from_coo(full, point, n_features: int):
    """the seven per-gene arrays (sum_x, sum_y, cells_full, cells, sum_xx, sum_yy, sum_xy: u64[n_features] each) of a point COO and the
    full COO — each a (feature, cell, count) triple ascending by (cell, feature): the host form of Engine.dev_partner_counts,
    Engine.dev_gene_moments and Engine.dev_gene_summary together; raises FastfError on a point row without a partner"""
    p32 = C.POINTER(C.c_uint32)
    keep, coos = [], []
    for f, c, k in (full, point):
        arrs = [np.ascontiguousarray(x, dtype=np.uint32) for x in (f, c, k)]
        assert len(arrs[0]) == len(arrs[1]) == len(arrs[2])
        keep.append(arrs)
        coos.append(Coo(arrs[0].ctypes.data_as(p32), arrs[1].ctypes.data_as(p32), arrs[2].ctypes.data_as(p32), len(arrs[0])))
    out = [np.zeros(max(n_features, 1), np.uint64) for _ in range(7)]
    _lib.check(_lib.lib().fastf_gene_fidelity_from_coo(C.byref(coos[0]), C.byref(coos[1]), n_features, *[x.ctypes.data for x in out]))
    return tuple(x[:n_features] for x in out)


def read_neighbors_table(path, columns=NEIGHBORS_COLUMNS):
    """the rows of sweep_neighbors.tsv as dicts of strings"""
    return read_cells_table(path, columns)


def read_point_neighbors(path):
    """the rows of a point's neighbors.tsv.gz as dicts of strings"""
    import gzip
    lines = gzip.decompress(open(path, "rb").read()).decode().split("\n")
    assert lines[0].split("\t") == list(POINT_NEIGHBORS_COLUMNS) and lines[-1] == ""
    return [dict(zip(POINT_NEIGHBORS_COLUMNS, ln.split("\t"))) for ln in lines[1:-1]]


def neighbors_header(verb: str = "") -> str:
    """the header of neighbors.tsv.gz, or with verb "sweep" / "cap" / "level" of <verb>_neighbors.tsv"""
    return getattr(_lib.lib(), "fastf_%sneighbors_header" % (verb + "_" if verb else ""))().decode()


def hvg_rank(n_cells, sums, sums_sq):
    """(genes, n_defined): the highly variable genes (0-based, rank order, at most HVG_TOP) of per-gene sums and sums of squares over
    n_cells cells — the ranking --gene-fidelity and --neighbors share — and the number of genes whose dispersion is defined"""
    a = np.ascontiguousarray(sums, dtype=np.uint64)
    b = np.ascontiguousarray(sums_sq, dtype=np.uint64)
    assert len(a) == len(b)
    genes = np.zeros(HVG_TOP, np.uint32)
    nd = C.c_uint32()
    K = _lib.lib().fastf_hvg_rank(int(n_cells), a.ctypes.data, b.ctypes.data, len(a), genes.ctypes.data, C.addressof(nd))
    if K == 0xFFFFFFFF:
        raise MemoryError("fastf_hvg_rank")
    return genes[:K].copy(), nd.value


def neighbors_slot_map(genes, n_features: int):
    """u16[n_features + 1]: the rank of every feature (1-based) in genes, 0xFFFF where it has none"""
    g = np.ascontiguousarray(genes, dtype=np.uint32)
    out = np.zeros(n_features + 1, np.uint16)
    _lib.check(_lib.lib().fastf_neighbors_slot_map(g.ctypes.data, len(g), n_features, out.ctypes.data))
    return out


def neighbors_pad(n_cells: int, n_genes: int):
    """(n_pad, K_pad): the padded shape of the device's byte planes"""
    a, b = C.c_uint32(), C.c_uint32()
    _lib.lib().fastf_neighbors_pad(n_cells, n_genes, C.byref(a), C.byref(b))
    return a.value, b.value


def neighbors_check_norm(max_norm: int):
    """raises FastfError naming FASTF_ERR_NEIGHBOR_NORM when max_norm >= 2^42"""
    _lib.check(_lib.lib().fastf_neighbors_check_norm(int(max_norm)))


def neighbors_from_coo(coo, n_cells: int, slot_map, k: int = NEIGHBORS_K):
    """(idx u32[n_cells, k], cnt u32[n_cells], norms u64[n_cells]) of a (feature, cell, count) COO restricted to the features with a slot:
    the host form of Engine.dev_neighbor_planes and Engine.dev_neighbors together"""
    p32 = C.POINTER(C.c_uint32)
    f, c, v = [np.ascontiguousarray(x, dtype=np.uint32) for x in coo]
    assert len(f) == len(c) == len(v)
    m = Coo(f.ctypes.data_as(p32), c.ctypes.data_as(p32), v.ctypes.data_as(p32), len(f))
    sm = np.ascontiguousarray(slot_map, dtype=np.uint16)
    idx = np.zeros((max(n_cells, 1), k), np.uint32)
    cnt = np.zeros(max(n_cells, 1), np.uint32)
    norms = np.zeros(max(n_cells, 1), np.uint64)
    _lib.check(_lib.lib().fastf_neighbors_from_coo(C.byref(m), n_cells, sm.ctypes.data, len(sm) - 1, k, idx.ctypes.data, cnt.ctypes.data, norms.ctypes.data))
    return idx[:n_cells], cnt[:n_cells], norms[:n_cells]


def neighbors_row(barcode, k_full, k_point, shared) -> str:
    """one row of neighbors.tsv.gz (with its newline)"""
    buf = C.create_string_buffer(512)
    _lib.check(_lib.lib().fastf_neighbors_row(barcode.encode() if isinstance(barcode, str) else barcode, int(k_full), int(k_point), int(shared), buf, len(buf)))
    return buf.value.decode()


def neighbors_summary_row(rate_cell, rate_depth, seed, hvg_k, k_full, k_point, shared, list_value: int = 0, k: int = NEIGHBORS_K) -> str:
    """one row of <verb>_neighbors.tsv (with its newline); list_value >= 1: that integer in the second column (cap, level)"""
    a = [np.ascontiguousarray(x, dtype=np.uint32) for x in (k_full, k_point, shared)]
    n = len(a[0])
    assert all(len(x) == n for x in a)
    buf = C.create_string_buffer(640)
    _lib.check(_lib.lib().fastf_neighbors_summary_row(float(rate_cell), float(rate_depth), int(list_value), int(seed) % (1 << 32), n, int(hvg_k), int(k),
                                                      a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, buf, len(buf)))
    return buf.value.decode()


def read_mapping_table(path, columns=MAPPING_COLUMNS):
    """the rows of sweep_mapping.tsv as dicts of strings"""
    return read_cells_table(path, columns)


def read_point_mapping(path):
    """the rows of a point's mapping.tsv.gz as dicts of strings"""
    import gzip
    lines = gzip.decompress(open(path, "rb").read()).decode().split("\n")
    assert lines[0].split("\t") == list(POINT_MAPPING_COLUMNS) and lines[-1] == ""
    return [dict(zip(POINT_MAPPING_COLUMNS, ln.split("\t"))) for ln in lines[1:-1]]


def mapping_header(verb: str = "") -> str:
    """the header of mapping.tsv.gz, or with verb "sweep" / "cap" / "level" of <verb>_mapping.tsv"""
    return getattr(_lib.lib(), "fastf_%smapping_header" % (verb + "_" if verb else ""))().decode()


def mapping_from_coo(full, point, n_cells: int, slot_map, k: int = MAPPING_K):
    """(idx u32[n_cells, k], cnt u32[n_cells], self_dot u64[n_cells], self_rank u32[n_cells]) of the point's (feature, cell, count) COO
    looked up among the cells of the full one, both restricted to the features with a slot: the host form of Engine.dev_neighbor_planes
    on both and Engine.dev_mapping together.  self_rank is MAPPING_NO_RANK where self_dot is 0"""
    p32 = C.POINTER(C.c_uint32)
    keep, coos = [], []
    for coo in (full, point):
        arrs = [np.ascontiguousarray(x, dtype=np.uint32) for x in coo]
        assert len(arrs[0]) == len(arrs[1]) == len(arrs[2])
        keep.append(arrs)
        coos.append(Coo(arrs[0].ctypes.data_as(p32), arrs[1].ctypes.data_as(p32), arrs[2].ctypes.data_as(p32), len(arrs[0])))
    sm = np.ascontiguousarray(slot_map, dtype=np.uint16)
    idx = np.zeros((max(n_cells, 1), max(k, 1)), np.uint32)
    cnt = np.zeros(max(n_cells, 1), np.uint32)
    sd = np.zeros(max(n_cells, 1), np.uint64)
    rank = np.zeros(max(n_cells, 1), np.uint32)
    _lib.check(_lib.lib().fastf_mapping_from_coo(C.byref(coos[0]), C.byref(coos[1]), n_cells, sm.ctypes.data, len(sm) - 1, k, idx.ctypes.data, cnt.ctypes.data,
                                                 sd.ctypes.data, rank.ctypes.data))
    return idx[:n_cells], cnt[:n_cells], sd[:n_cells], rank[:n_cells]


def mapping_row(barcode, self_dot, self_rank, k_map, k_full, hood, pred_map=None) -> str:
    """one row of mapping.tsv.gz (with its newline); self_rank None or MAPPING_NO_RANK and pred_map None print NA"""
    _b = lambda x: x.encode() if isinstance(x, str) else x  # noqa: E731
    buf = C.create_string_buffer(512)
    _lib.check(_lib.lib().fastf_mapping_row(_b(barcode), int(self_dot), MAPPING_NO_RANK if self_rank is None else int(self_rank), int(k_map), int(k_full), int(hood),
                                            None if pred_map is None else _b(pred_map), buf, len(buf)))
    return buf.value.decode()


def mapping_summary_row(rate_cell, rate_depth, seed, hvg_k, self_dot, self_rank, k_full, hood, lab=None, same_map=None, labelled_map=None, list_value: int = 0,
                        k: int = MAPPING_K) -> str:
    """one row of <verb>_mapping.tsv (with its newline); lab None: a run without labels; list_value >= 1: that integer in the second column"""
    sd = np.ascontiguousarray(self_dot, dtype=np.uint64)
    a = [np.ascontiguousarray(x, dtype=np.uint32) for x in (self_rank, k_full, hood)]
    n = len(sd)
    assert all(len(x) == n for x in a)
    b = [None, None, None] if lab is None else [np.ascontiguousarray(x, dtype=np.uint8) for x in (lab, same_map, labelled_map)]
    assert lab is None or all(len(x) == n for x in b)
    buf = C.create_string_buffer(640)
    _lib.check(_lib.lib().fastf_mapping_summary_row(float(rate_cell), float(rate_depth), int(list_value), int(seed) % (1 << 32), n, int(hvg_k), int(k), sd.ctypes.data,
                                                    a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, *[None if x is None else x.ctypes.data for x in b], buf, len(buf)))
    return buf.value.decode()


def read_coexpression_table(path, columns=COEXPRESSION_COLUMNS):
    """the per-point co-expression rows of a table as dicts of strings"""
    return read_cells_table(path, columns)


def read_point_coexpression(path):
    """the per-gene co-expression rows of a gzipped table as dicts of strings"""
    import gzip
    lines = gzip.decompress(open(path, "rb").read()).decode().split("\n")
    assert lines[0].split("\t") == list(POINT_COEXPRESSION_COLUMNS) and lines[-1] == ""
    return [dict(zip(POINT_COEXPRESSION_COLUMNS, ln.split("\t"))) for ln in lines[1:-1]]


def coexpression_header(verb: str = "") -> str:
    """the header of the per-gene rows, or with verb "sweep" / "cap" / "level" of the per-point rows"""
    return getattr(_lib.lib(), "fastf_%scoexpr_header" % (verb + "_" if verb else ""))().decode()


def coexpression_pad(n_cells: int, n_genes: int):
    """(K_pad, n_pad, chunk): the shape of the gene-major byte planes of Engine.dev_coexpr_sums and the cells of a chunk, under the
    FASTF_COEXPR_CHUNK in effect"""
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    _lib.lib().fastf_coexpr_pad(n_cells, n_genes, C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def coexpression_work_bytes(n_cells: int, n_genes: int, planes: int) -> int:
    """the bytes of the work buffer of Engine.dev_coexpr_sums"""
    return int(_lib.lib().fastf_coexpr_work_bytes(n_cells, n_genes, planes))


def coexpression_check_range(n_cells: int, max_q: int):
    """raises FastfError naming FASTF_ERR_COEXPR_RANGE when n_cells * max_q >= 2^63"""
    _lib.check(_lib.lib().fastf_coexpr_check_range(int(n_cells), int(max_q)))


def coexpression_from_coo(coo, n_cells: int, slot_map, n_genes: int, k: int = COEXPRESSION_K):
    """(idx u32[n_genes, k], cnt u32[n_genes], D u64[n_genes, n_genes], S u64[n_genes]) of a (feature, cell, count) COO restricted to the
    features with a slot below n_genes: the definition in plain C on the host"""
    p32 = C.POINTER(C.c_uint32)
    f, c, v = [np.ascontiguousarray(x, dtype=np.uint32) for x in coo]
    assert len(f) == len(c) == len(v)
    m = Coo(f.ctypes.data_as(p32), c.ctypes.data_as(p32), v.ctypes.data_as(p32), len(f))
    sm = np.ascontiguousarray(slot_map, dtype=np.uint16)
    K = int(n_genes)
    idx = np.zeros((max(K, 1), k), np.uint32)
    cnt = np.zeros(max(K, 1), np.uint32)
    D = np.zeros((max(K, 1), max(K, 1)), np.uint64)
    S = np.zeros(max(K, 1), np.uint64)
    _lib.check(_lib.lib().fastf_coexpr_from_coo(C.byref(m), n_cells, sm.ctypes.data, len(sm) - 1, K, k, idx.ctypes.data, cnt.ctypes.data,
                                                D.ctypes.data if K else None, S.ctypes.data if K else None))
    return idx[:K], cnt[:K], D[:K, :K], S[:K]


def coexpression_select(D, S, n_cells: int, k: int = COEXPRESSION_K):
    """(idx, cnt): the partner sets of the sums of products D (u64[K, K]) and the sums S (u64[K]) over n_cells cells, on the host"""
    D = np.ascontiguousarray(D, dtype=np.uint64)
    S = np.ascontiguousarray(S, dtype=np.uint64)
    K = len(S)
    assert D.shape == (K, K) or (K == 0 and D.size == 0)
    idx = np.zeros((max(K, 1), k), np.uint32)
    cnt = np.zeros(max(K, 1), np.uint32)
    _lib.check(_lib.lib().fastf_coexpr_select(D.ctypes.data if K else None, S.ctypes.data if K else None, int(n_cells), K, k, idx.ctypes.data, cnt.ctypes.data))
    return idx[:K], cnt[:K]


def coexpression_row(gene, k_full, k_point, shared) -> str:
    """one per-gene row (with its newline)"""
    buf = C.create_string_buffer(512)
    _lib.check(_lib.lib().fastf_coexpr_row(gene.encode() if isinstance(gene, str) else gene, int(k_full), int(k_point), int(shared), buf, len(buf)))
    return buf.value.decode()


def coexpression_summary_row(rate_cell, rate_depth, seed, n_cells, k_full, k_point, shared, list_value: int = 0, k: int = COEXPRESSION_K) -> str:
    """one per-point row (with its newline) over the genes of the three arrays; list_value >= 1: that integer in the second column"""
    a = [np.ascontiguousarray(x, dtype=np.uint32) for x in (k_full, k_point, shared)]
    K = len(a[0])
    assert all(len(x) == K for x in a)
    buf = C.create_string_buffer(640)
    _lib.check(_lib.lib().fastf_coexpr_summary_row(float(rate_cell), float(rate_depth), int(list_value), int(seed) % (1 << 32), int(n_cells), K, int(k),
                                                   a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, buf, len(buf)))
    return buf.value.decode()


def read_labels_table(path, columns=LABELS_COLUMNS):
    """the rows of sweep_labels.tsv as dicts of strings"""
    return read_cells_table(path, columns)


def read_label_classes_table(path, columns=LABEL_CLASSES_COLUMNS):
    """the rows of sweep_label_classes.tsv as dicts of strings"""
    return read_cells_table(path, columns)


def read_point_labels(path):
    """the rows of a point's labels.tsv.gz as dicts of strings"""
    import gzip
    lines = gzip.decompress(open(path, "rb").read()).decode().split("\n")
    assert lines[0].split("\t") == list(POINT_LABELS_COLUMNS) and lines[-1] == ""
    return [dict(zip(POINT_LABELS_COLUMNS, ln.split("\t"))) for ln in lines[1:-1]]


def labels_header(verb: str = "", classes: bool = False) -> str:
    """the header of labels.tsv.gz, or with verb "sweep" / "cap" / "level" of <verb>_labels.tsv (classes: of <verb>_label_classes.tsv)"""
    return getattr(_lib.lib(), "fastf_%slabel%s_header" % (verb + "_" if verb else "", "_classes" if classes else "s"))().decode()


class Labels:
    """a labels file loaded against a barcode list file (fastf_labels_load): names[0] == "NA", names[1 .. n_labels] ascending bytewise"""

    def __init__(self, labels_file, barcodes_file):
        self._h = C.c_void_p()
        _lib.check(_lib.lib().fastf_labels_load(os.fspath(labels_file).encode(), os.fspath(barcodes_file).encode(), C.byref(self._h)))
        L = _lib.lib()
        self.n_labels = L.fastf_labels_count(self._h)
        self.names = [L.fastf_labels_name(self._h, k) for k in range(self.n_labels + 1)]
        self.known, self.unknown = L.fastf_labels_known(self._h), L.fastf_labels_unknown(self._h)

    def id(self, barcode) -> int:
        return _lib.lib().fastf_labels_id(self._h, barcode.encode() if isinstance(barcode, str) else barcode)

    def assign(self, barcodes):
        """lab (u8) of a list of barcodes"""
        b = [x.encode() if isinstance(x, str) else x for x in barcodes]
        arr = (C.c_char_p * max(len(b), 1))(*b)
        lab = np.zeros(max(len(b), 1), np.uint8)
        _lib.check(_lib.lib().fastf_labels_assign(self._h, arr, len(b), lab.ctypes.data))
        return lab[:len(b)]

    def close(self):
        if self._h:
            _lib.lib().fastf_labels_free(self._h)
            self._h = C.c_void_p()

    __del__ = close


def label_votes(idx, cnt, lab, k: int, n_labels: int):
    """(pred, same, labelled u8[n], conf u32[n_labels, n_labels + 1]) of neighbour sets idx (u32[n, k]), cnt (u32[n]) and labels lab
    (u8[n]): the host form of Engine.dev_label_votes"""
    cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
    n = len(cnt)
    idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
    lab = np.ascontiguousarray(lab, dtype=np.uint8)
    assert len(idx) == n * k and len(lab) == n
    out = [np.zeros(max(n, 1), np.uint8) for _ in range(3)]
    conf = np.full(max(n_labels * (n_labels + 1), 1), 0xDEADBEEF, np.uint32)
    _lib.check(_lib.lib().fastf_label_votes(idx.ctypes.data, cnt.ctypes.data, lab.ctypes.data, n, k, n_labels, out[0].ctypes.data, out[1].ctypes.data,
                                            out[2].ctypes.data, conf.ctypes.data))
    return out[0][:n], out[1][:n], out[2][:n], conf[:n_labels * (n_labels + 1)].reshape(n_labels, n_labels + 1)


def _b(x):
    return x.encode() if isinstance(x, str) else x


def labels_row(barcode, label, pred_full, pred_point, same_full, labelled_full, same_point, labelled_point) -> str:
    """one row of labels.tsv.gz (with its newline)"""
    buf = C.create_string_buffer(512)
    _lib.check(_lib.lib().fastf_labels_row(_b(barcode), _b(label), _b(pred_full), _b(pred_point), int(same_full), int(labelled_full), int(same_point),
                                           int(labelled_point), buf, len(buf)))
    return buf.value.decode()


def label_confusion_header(names) -> str:
    """names[0] is "NA" and not read; names[1:] the labels"""
    arr = (C.c_char_p * len(names))(*[_b(x) for x in names])
    buf = C.create_string_buffer(64 + 64 * len(names))
    _lib.check(_lib.lib().fastf_label_confusion_header(arr, len(names) - 1, buf, len(buf)))
    return buf.value.decode()


def label_confusion_row(label, cells, conf_row) -> str:
    c = np.ascontiguousarray(conf_row, dtype=np.uint32)
    buf = C.create_string_buffer(128 + 12 * len(c))
    _lib.check(_lib.lib().fastf_label_confusion_row(_b(label), int(cells), c.ctypes.data, len(c) - 1, buf, len(buf)))
    return buf.value.decode()


def labels_summary_row(rate_cell, rate_depth, seed, k, n_labels, lab, pred_full, pred_point, same_full, labelled_full, same_point, labelled_point,
                       conf_full, conf_point, list_value: int = 0) -> str:
    """one row of <verb>_labels.tsv (with its newline); list_value >= 1: that integer in the second column (cap, level)"""
    a = [np.ascontiguousarray(x, dtype=np.uint8) for x in (lab, pred_full, pred_point, same_full, labelled_full, same_point, labelled_point)]
    cf, cp = (np.ascontiguousarray(x, dtype=np.uint32).reshape(-1) for x in (conf_full, conf_point))
    n = len(a[0])
    assert all(len(x) == n for x in a) and len(cf) == len(cp) == n_labels * (n_labels + 1)
    buf = C.create_string_buffer(640)
    _lib.check(_lib.lib().fastf_labels_summary_row(float(rate_cell), float(rate_depth), int(list_value), int(seed) % (1 << 32), n, int(k), int(n_labels),
                                                   *[x.ctypes.data for x in a], cf.ctypes.data, cp.ctypes.data, buf, len(buf)))
    return buf.value.decode()


def label_classes_row(rate_cell, rate_depth, seed, label, a, n_labels, lab, conf_full, conf_point, list_value: int = 0) -> str:
    """one row of <verb>_label_classes.tsv (with its newline) for label a (1 .. n_labels)"""
    lab = np.ascontiguousarray(lab, dtype=np.uint8)
    cf, cp = (np.ascontiguousarray(x, dtype=np.uint32).reshape(-1) for x in (conf_full, conf_point))
    buf = C.create_string_buffer(640)
    _lib.check(_lib.lib().fastf_label_classes_row(float(rate_cell), float(rate_depth), int(list_value), int(seed) % (1 << 32), _b(label), int(a), len(lab),
                                                  int(n_labels), lab.ctypes.data, cf.ctypes.data, cp.ctypes.data, buf, len(buf)))
    return buf.value.decode()


def read_pseudotime_table(path, columns=None):
    """the rows of sweep_pseudotime.tsv as dicts of strings"""
    return read_cells_table(path, PSEUDOTIME_COLUMNS if columns is None else columns)


def read_point_pseudotime(path):
    """the rows of a point's pseudotime.tsv.gz as dicts of strings"""
    import gzip
    lines = gzip.decompress(open(path, "rb").read()).decode().split("\n")
    assert lines[0].split("\t") == list(POINT_PSEUDOTIME_COLUMNS) and lines[-1] == ""
    return [dict(zip(POINT_PSEUDOTIME_COLUMNS, ln.split("\t"))) for ln in lines[1:-1]]


def pseudotime_header(verb: str = "") -> str:
    """the header of pseudotime.tsv.gz, or with verb "sweep" / "cap" / "level" of <verb>_pseudotime.tsv"""
    return getattr(_lib.lib(), "fastf_%s_pseudotime_header" % verb if verb else "fastf_ptime_header")().decode()


class Pseudotime:
    """a pseudotime file loaded against a barcode list file (fastf_ptime_load): known, unknown — the lines whose barcode is / is not
    listed; valued — the lines of a listed barcode that carry a value"""

    def __init__(self, ptime_file, barcodes_file):
        self._h = C.c_void_p()
        _lib.check(_lib.lib().fastf_ptime_load(os.fspath(ptime_file).encode(), os.fspath(barcodes_file).encode(), C.byref(self._h)))
        L = _lib.lib()
        self.known, self.unknown, self.valued = L.fastf_ptime_known(self._h), L.fastf_ptime_unknown(self._h), L.fastf_ptime_valued(self._h)

    def assign(self, barcodes):
        """(t u32[n], m): the doubled midranks of a list of barcodes among those of them with a value (0 without), and their number"""
        b = [x.encode() if isinstance(x, str) else x for x in barcodes]
        arr = (C.c_char_p * max(len(b), 1))(*b)
        t = np.zeros(max(len(b), 1), np.uint32)
        m = C.c_uint32()
        _lib.check(_lib.lib().fastf_ptime_assign(self._h, arr, len(b), t.ctypes.data, C.byref(m)))
        return t[:len(b)], m.value

    def close(self):
        if self._h:
            _lib.lib().fastf_ptime_free(self._h)
            self._h = C.c_void_p()

    __del__ = close


def ptime_medians(idx, cnt, t, k: int):
    """(est, valued u32[n]) of neighbour lists idx (u32[n, k]), cnt (u32[n]) and ranks t (u32[n]): the host form of Engine.dev_ptime_medians"""
    cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
    n = len(cnt)
    idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
    t = np.ascontiguousarray(t, dtype=np.uint32)
    assert len(idx) == n * k and len(t) == n
    out = [np.full(max(n, 1), 0xDEADBEEF, np.uint32) for _ in range(2)]
    _lib.check(_lib.lib().fastf_ptime_medians(idx.ctypes.data, cnt.ctypes.data, t.ctypes.data, n, k, out[0].ctypes.data, out[1].ctypes.data))
    return out[0][:n], out[1][:n]


def ptime_census(est, t):
    """u64[7] (conc disc tie_e tie_t tie_both cells shift_sum) of est against t: the host form of Engine.dev_ptime_census, O(n^2)"""
    est, t = (np.ascontiguousarray(x, dtype=np.uint32) for x in (est, t))
    assert len(est) == len(t)
    out = np.full(PTIME_OUT_WORDS, 0xDEADBEEF, np.uint64)
    _lib.check(_lib.lib().fastf_ptime_census(est.ctypes.data, t.ctypes.data, len(t), out.ctypes.data))
    return out


def ptime_row(barcode, rank, est_full, valued_full, est_point, valued_point, est_map=None, valued_map=None) -> str:
    """one row of pseudotime.tsv.gz (with its newline); est_map None: a run without --mapping"""
    buf = C.create_string_buffer(512)
    mapping = est_map is not None
    _lib.check(_lib.lib().fastf_ptime_row(_b(barcode), int(rank), int(est_full), int(valued_full), int(est_point), int(valued_point),
                                          int(est_map) if mapping else 0, int(valued_map) if mapping else 0, int(mapping), buf, len(buf)))
    return buf.value.decode()


def ptime_summary_row(rate_cell, rate_depth, seed, n_cells, cells_valued, census_full, census_point, census_map=None, list_value: int = 0,
                      k: int = NEIGHBORS_K) -> str:
    """one row of <verb>_pseudotime.tsv (with its newline); census_map None: a run without --mapping; list_value >= 1: that integer in the second column"""
    c = [None if x is None else np.ascontiguousarray(x, dtype=np.uint64) for x in (census_full, census_point, census_map)]
    assert all(x is None or len(x) == PTIME_OUT_WORDS for x in c)
    buf = C.create_string_buffer(640)
    _lib.check(_lib.lib().fastf_ptime_summary_row(float(rate_cell), float(rate_depth), int(list_value), int(seed) % (1 << 32), int(n_cells), int(k), int(cells_valued),
                                                  *[None if x is None else x.ctypes.data for x in c], buf, len(buf)))
    return buf.value.decode()


def read_markers_table(path, columns=MARKERS_COLUMNS):
    """the rows of sweep_markers.tsv as dicts of strings"""
    return read_cells_table(path, columns)


def read_point_markers(path):
    """the rows of a point's markers.tsv.gz as dicts of strings"""
    import gzip
    lines = gzip.decompress(open(path, "rb").read()).decode().split("\n")
    assert lines[0].split("\t") == list(POINT_MARKERS_COLUMNS) and lines[-1] == ""
    return [dict(zip(POINT_MARKERS_COLUMNS, ln.split("\t"))) for ln in lines[1:-1]]


def markers_header(verb: str = "") -> str:
    """the header of markers.tsv.gz, or with verb "sweep" / "cap" / "level" of <verb>_markers.tsv"""
    return getattr(_lib.lib(), "fastf_%smarkers_header" % (verb + "_" if verb else ""))().decode()


def marker_planes(counts, n_planes: int, pad_byte: int = 0):
    """the byte planes of a dense count array (n_cells x K, values below 128 ** n_planes) in the layout of Engine.dev_neighbor_planes:
    u8[n_planes, n_pad, K_pad], plane p holds bits 7p .. 7p+6; the padding rows and slots hold pad_byte"""
    counts = np.asarray(counts, dtype=np.uint64)
    n, K = counts.shape
    n_pad, K_pad = neighbors_pad(n, K)
    pl = np.full((n_planes, n_pad, K_pad), pad_byte, np.uint8)
    for p in range(n_planes):
        pl[p, :n, :K] = ((counts >> np.uint64(7 * p)) & np.uint64(127)).astype(np.uint8)
    return pl


def marker_auc(planes, n_planes: int, n_cells: int, K: int, lab, n_labels: int):
    """(s2u u64[n_labels, K], det u32[n_labels, K], sum u64[n_labels, K], n_per_label u32[n_labels]) of byte planes (marker_planes) and
    labels lab (u8[n_cells]): the host form of Engine.dev_marker_auc"""
    planes = np.ascontiguousarray(planes, dtype=np.uint8)
    lab = np.ascontiguousarray(lab, dtype=np.uint8)
    n_pad, K_pad = neighbors_pad(n_cells, K)
    assert len(lab) == n_cells and (n_planes > 3 or planes.size >= n_planes * n_pad * K_pad)
    words = max(n_labels * K, 1)
    s2u, det, sm = np.full(words, 0xDEADBEEF, np.uint64), np.full(words, 0xDEADBEEF, np.uint32), np.full(words, 0xDEADBEEF, np.uint64)
    npl = np.full(max(n_labels, 1), 0xDEADBEEF, np.uint32)
    _lib.check(_lib.lib().fastf_marker_auc(planes.ctypes.data, n_planes, n_cells, K, lab.ctypes.data if n_cells else None, n_labels, s2u.ctypes.data,
                                           det.ctypes.data, sm.ctypes.data, npl.ctypes.data))
    W = n_labels * K
    return s2u[:W].reshape(n_labels, K), det[:W].reshape(n_labels, K), sm[:W].reshape(n_labels, K), npl[:n_labels]


def marker_auc_form(n_planes: int, n_labels: int) -> int:
    """1: a device call keeps its accumulators in LDS, 0: it adds by global atomics (FASTF_MARKERS_LDS=0 included), -1: it is refused"""
    return int(_lib.lib().fastf_marker_auc_form(n_planes, n_labels))


def marker_rank(s2u, n_per_label, genes=None):
    """rank u32[n_labels, K] (from 1; 0: the label has no ranking) of s2u (u64[n_labels, K]) by descending s2u, ties by ascending
    genes[slot] (None: by slot)"""
    s2u = np.ascontiguousarray(s2u, dtype=np.uint64)
    n_labels, K = s2u.shape
    npl = np.ascontiguousarray(n_per_label, dtype=np.uint32)
    assert len(npl) == n_labels
    g = None if genes is None else np.ascontiguousarray(genes, dtype=np.uint32)
    assert g is None or len(g) == K
    rank = np.full(max(n_labels * K, 1), 0xDEADBEEF, np.uint32)
    _lib.check(_lib.lib().fastf_marker_rank(s2u.ctypes.data, npl.ctypes.data, None if g is None else g.ctypes.data, K, n_labels, rank.ctypes.data))
    return rank[:n_labels * K].reshape(n_labels, K)


def markers_row(label, gene, n_in, n_out, rank_full, rank_point, s2u_full, s2u_point, det_in_full, det_out_full, det_in_point, det_out_point,
                sum_in_point) -> str:
    """one row of markers.tsv.gz (with its newline); gene None: the NA row of a label without a ranking"""
    buf = C.create_string_buffer(512)
    _lib.check(_lib.lib().fastf_markers_row(_b(label), None if gene is None else _b(gene), int(n_in), int(n_out), int(rank_full), int(rank_point), int(s2u_full),
                                            int(s2u_point), int(det_in_full), int(det_out_full), int(det_in_point), int(det_out_point), int(sum_in_point),
                                            buf, len(buf)))
    return buf.value.decode()


def markers_summary_rows(rate_cell, rate_depth, seed, names, top_n, n_per_label, rank_full, rank_point, s2u_full, s2u_point, list_value: int = 0) -> str:
    """the n_labels + 1 rows of one point of <verb>_markers.tsv; names[0] is "NA" and not read"""
    npl = np.ascontiguousarray(n_per_label, dtype=np.uint32)
    rf, rp = (np.ascontiguousarray(x, dtype=np.uint32) for x in (rank_full, rank_point))
    sf, sp = (np.ascontiguousarray(x, dtype=np.uint64) for x in (s2u_full, s2u_point))
    L, K = sf.shape
    assert len(names) == L + 1 and len(npl) == L and rf.shape == rp.shape == sp.shape == (L, K)
    arr = (C.c_char_p * len(names))(*[_b(x) for x in names])
    buf = C.create_string_buffer(256 * (L + 1))
    _lib.check(_lib.lib().fastf_markers_summary_rows(float(rate_cell), float(rate_depth), int(list_value), int(seed) % (1 << 32), arr, L, K, int(top_n),
                                                     npl.ctypes.data, rf.ctypes.data, rp.ctypes.data, sf.ctypes.data, sp.ctypes.data, buf, len(buf)))
    return buf.value.decode()


REPS_METRICS = ("sampled_reads", "sampled_valid_reads", "nnz", "umis", "saturation", "median_umis_per_cell", "median_genes_per_cell")
_STAT4 = lambda m: tuple("%s_%s" % (m, t) for t in ("mean", "sd", "min", "max"))  # noqa: E731
REPS_TAIL_COLUMNS = ("n_reps", "n_cells") + sum((_STAT4(m) for m in REPS_METRICS), ())
REPS_COLUMNS = ("rate_cell", "rate_depth") + REPS_TAIL_COLUMNS
GENES_REPS_TAIL_COLUMNS = ("n_reps",) + _STAT4("genes_detected") + ("genes_in_all_reps", "genes_in_any_rep")
GENES_REPS_COLUMNS = ("rate_cell", "rate_depth") + GENES_REPS_TAIL_COLUMNS


def read_reps_table(path, columns=REPS_COLUMNS):
    """the rows of sweep_reps.tsv as dicts of strings"""
    return read_cells_table(path, columns)


def read_genes_reps_table(path, columns=GENES_REPS_COLUMNS):
    """the rows of sweep_genes_reps.tsv as dicts of strings"""
    return read_cells_table(path, columns)


def parse_seeds(text: str):
    """a comma-separated list of seeds as the command reads --seeds; raises FastfError on what it refuses"""
    out = np.zeros(64, dtype=np.uint32)
    n = C.c_uint32()
    _lib.check(_lib.lib().fastf_parse_seeds(text.encode(), out.ctypes.data, len(out), C.byref(n)))
    return out[:n.value].copy()


def reps_seeds(first: int, n_reps: int):
    """the seeds of --reps n_reps with -s first; raises FastfError where they would wrap past 2^32 - 1"""
    out = np.zeros(64, dtype=np.uint32)
    n = C.c_uint32()
    _lib.check(_lib.lib().fastf_reps_seeds(int(first) % (1 << 32), int(n_reps), out.ctypes.data, len(out), C.byref(n)))
    return out[:n.value].copy()


def reps_point_dir(point_name: str, seed: int) -> str:
    buf = C.create_string_buffer(96)
    _lib.check(_lib.lib().fastf_reps_point_dir(point_name.encode(), int(seed) % (1 << 32), buf, len(buf)))
    return buf.value.decode()


def reps_header() -> str:
    return _lib.lib().fastf_sweep_reps_header().decode()


def genes_reps_header() -> str:
    return _lib.lib().fastf_sweep_genes_reps_header().decode()


def reps_summary_row(rate_cell, rate_depth, n_cells, metrics, reads_per_cell: int = 0) -> str:
    """one row of sweep_reps.tsv (with its newline) from metrics[k][m] (replicate k, metric m of REPS_METRICS);
    reads_per_cell >= 1: a row of cap_reps.tsv"""
    m = np.ascontiguousarray(metrics, dtype=np.float64).reshape(-1, len(REPS_METRICS))
    buf = C.create_string_buffer(2048)
    _lib.check(_lib.lib().fastf_reps_summary_row(float(rate_cell), float(rate_depth), int(reads_per_cell), int(n_cells), m.ctypes.data, len(m), buf, len(buf)))
    return buf.value.decode()


def genes_reps_row(rate_cell, rate_depth, genes_detected, reps_detected, reads_per_cell: int = 0) -> str:
    """one row of sweep_genes_reps.tsv (with its newline); reads_per_cell >= 1: a row of cap_genes_reps.tsv"""
    gd = np.ascontiguousarray(genes_detected, dtype=np.uint32)
    rdt = np.ascontiguousarray(reps_detected, dtype=np.uint64)
    buf = C.create_string_buffer(512)
    _lib.check(_lib.lib().fastf_genes_reps_row(float(rate_cell), float(rate_depth), int(reads_per_cell), gd.ctypes.data, len(gd), rdt.ctypes.data, len(rdt),
                                               buf, len(buf)))
    return buf.value.decode()


def gene_reps_add_host(cells_per_gene, detected, total, sumsq):
    """the host form of Engine.dev_gene_reps_add: the three u64 arrays are added to in place"""
    c = np.ascontiguousarray(cells_per_gene, dtype=np.uint32)
    for a in (detected, total, sumsq):
        assert a.dtype == np.uint64 and a.flags.c_contiguous and len(a) == len(c)
    _lib.check(_lib.lib().fastf_gene_reps_add_host(c.ctypes.data, len(c), detected.ctypes.data, total.ctypes.data, sumsq.ctypes.data))


def read_table(path):
    lines = open(path).read().split("\n")
    assert lines[0].split("\t") == list(COLUMNS) and lines[-1] == ""
    return [dict(zip(COLUMNS, ln.split("\t"))) for ln in lines[1:-1]]


def read_genes_table(path):
    """the rows of sweep_genes.tsv as dicts of strings"""
    lines = open(path).read().split("\n")
    assert lines[0].split("\t") == list(GENES_COLUMNS) and lines[-1] == ""
    return [dict(zip(GENES_COLUMNS, ln.split("\t"))) for ln in lines[1:-1]]


def read_cells_table(path, columns=CELLS_COLUMNS):
    """the rows of sweep_cells.tsv as dicts of strings"""
    lines = open(path).read().split("\n")
    assert lines[0].split("\t") == list(columns) and lines[-1] == ""
    return [dict(zip(columns, ln.split("\t"))) for ln in lines[1:-1]]


def cells_header() -> str:
    return _lib.lib().fastf_sweep_cells_header().decode()


def copies_from_umi_rows(cell, n_copy, nonnull, n_cells: int):
    """(reads per cell, NULL-UMI reads per cell, singleton UMIs per cell — u32[n_cells] each — and hist u64[COPY_BINS + 1]) of -u
    rows: the host form of Engine.dev_copy_summary"""
    c = np.ascontiguousarray(cell, dtype=np.uint32)
    k = np.ascontiguousarray(n_copy, dtype=np.uint32)
    nn = np.ascontiguousarray(nonnull, dtype=np.uint8)
    assert len(c) == len(k) == len(nn)
    z = np.zeros(len(c), dtype=np.uint32)
    p32 = C.POINTER(C.c_uint32)
    rows = UmiRows(z.ctypes.data_as(p32), c.ctypes.data_as(p32), k.ctypes.data_as(p32), z.ctypes.data_as(p32), nn.ctypes.data_as(C.POINTER(C.c_uint8)), len(c))
    r, nr, sg = (np.zeros(max(n_cells, 1), np.uint32) for _ in range(3))
    hist = np.zeros(COPY_BINS + 1, np.uint64)
    _lib.check(_lib.lib().fastf_copies_from_umi_rows(C.byref(rows), n_cells, r.ctypes.data, nr.ctypes.data, sg.ctypes.data, hist.ctypes.data))
    return r[:n_cells], nr[:n_cells], sg[:n_cells], hist


def cells_summary_row(rate_cell, rate_depth, seed, reads, null_reads, single, hist, reads_per_cell: int = 0) -> str:
    """one row of sweep_cells.tsv (with its newline); reads_per_cell >= 1: a row of cap_cells.tsv"""
    r = np.ascontiguousarray(reads, dtype=np.uint32)
    nr = np.ascontiguousarray(null_reads, dtype=np.uint32)
    sg = np.ascontiguousarray(single, dtype=np.uint32)
    h = np.ascontiguousarray(hist, dtype=np.uint64)
    assert len(r) == len(nr) == len(sg) and len(h) == COPY_BINS + 1
    buf = C.create_string_buffer(1024)
    _lib.check(_lib.lib().fastf_cells_summary_row(float(rate_cell), float(rate_depth), int(reads_per_cell), seed, r.ctypes.data, nr.ctypes.data,
                                                  sg.ctypes.data, len(r), h.ctypes.data, buf, len(buf)))
    return buf.value.decode()


def parse_rates(text: str, cell_rates: bool = False):
    """a comma-separated list of rates as the command reads -c (cell_rates) and -r; raises FastfError on what it refuses"""
    out = np.zeros(64, dtype=np.float32)
    n = C.c_uint32()
    _lib.check(_lib.lib().fastf_sweep_parse_rates(text.encode(), int(cell_rates), out.ctypes.data_as(C.POINTER(C.c_float)), len(out), C.byref(n)))
    return out[:n.value].copy()


def check_grid(rates_cell, rates_depth):
    rc, prc = _floats(rates_cell)
    rd, prd = _floats(rates_depth)
    _lib.check(_lib.lib().fastf_sweep_check_grid(prc, len(rc), prd, len(rd)))


def point_dir(rate_cell: float, rate_depth: float) -> str:
    buf = C.create_string_buffer(64)
    _lib.check(_lib.lib().fastf_sweep_point_dir(float(rate_cell), float(rate_depth), buf, len(buf)))
    return buf.value.decode()


def header() -> str:
    return _lib.lib().fastf_sweep_header().decode()


def cells_from_coo(cell, count, n_cells: int):
    """(umis per cell u64[n_cells], genes per cell u32[n_cells], umis) of rows ascending by cell: the host form of
    Engine.dev_cell_summary"""
    c = np.ascontiguousarray(cell, dtype=np.uint32)
    k = np.ascontiguousarray(count, dtype=np.uint32)
    f = np.zeros(len(c), dtype=np.uint32)
    p32 = C.POINTER(C.c_uint32)
    coo = Coo(f.ctypes.data_as(p32), c.ctypes.data_as(p32), k.ctypes.data_as(p32), len(c))
    upc, gpc, tot = np.zeros(max(n_cells, 1), np.uint64), np.zeros(max(n_cells, 1), np.uint32), C.c_uint64()
    _lib.check(_lib.lib().fastf_sweep_cells_from_coo(C.byref(coo), n_cells, upc.ctypes.data, gpc.ctypes.data, C.byref(tot)))
    return upc[:n_cells], gpc[:n_cells], int(tot.value)


def genes_from_coo(feature, count, n_features: int):
    """(cells per gene u32[n_features], umis per gene u64[n_features]) of rows in any order: the host form of
    Engine.dev_gene_summary"""
    f = np.ascontiguousarray(feature, dtype=np.uint32)
    k = np.ascontiguousarray(count, dtype=np.uint32)
    c = np.zeros(len(f), dtype=np.uint32)
    p32 = C.POINTER(C.c_uint32)
    coo = Coo(f.ctypes.data_as(p32), c.ctypes.data_as(p32), k.ctypes.data_as(p32), len(f))
    cpg, upg = np.zeros(max(n_features, 1), np.uint32), np.zeros(max(n_features, 1), np.uint64)
    _lib.check(_lib.lib().fastf_sweep_genes_from_coo(C.byref(coo), n_features, cpg.ctypes.data, upg.ctypes.data))
    return cpg[:n_features], upg[:n_features]


def genes_header() -> str:
    return _lib.lib().fastf_sweep_genes_header().decode()


def genes_summary_row(rate_cell, rate_depth, seed, cells_per_gene, umis_per_gene, reads_per_cell: int = 0) -> str:
    """one row of sweep_genes.tsv (with its newline); reads_per_cell >= 1: a row of cap_genes.tsv"""
    cpg = np.ascontiguousarray(cells_per_gene, dtype=np.uint32)
    upg = np.ascontiguousarray(umis_per_gene, dtype=np.uint64)
    buf = C.create_string_buffer(256)
    _lib.check(_lib.lib().fastf_genes_summary_row(float(rate_cell), float(rate_depth), int(reads_per_cell), seed, cpg.ctypes.data, upg.ctypes.data,
                                                  len(cpg), buf, len(buf)))
    return buf.value.decode()


def summary_row(rate_cell, rate_depth, seed, counters, nnz, umis, umis_per_cell, genes_per_cell) -> str:
    """one row of sweep.tsv (with its newline)"""
    upc = np.ascontiguousarray(umis_per_cell, dtype=np.uint64)
    gpc = np.ascontiguousarray(genes_per_cell, dtype=np.uint32)
    cnt = (C.c_uint64 * 3)(*[int(x) for x in counters])
    buf = C.create_string_buffer(512)
    _lib.check(_lib.lib().fastf_sweep_summary_row(float(rate_cell), float(rate_depth), seed, C.byref(cnt), int(nnz), int(umis),
                                                  upc.ctypes.data, gpc.ctypes.data, len(upc), buf, len(buf)))
    return buf.value.decode()
