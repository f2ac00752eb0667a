"""Python mirror of `fastF level` (include/fastf_amd.h: fastf_level and its host pieces): every cell downsampled to at most M UMIs,
exactly, over a grid of (cell rate, UMI cap) points from one decode of the BAM.  Nothing here computes results: every call lands in
the library."""
import ctypes as C
import gzip
import os

import numpy as np

from . import _lib
from . import cap as _cap
from . import sweep as _sweep

SUMMARY_ONLY = 1      # FASTF_LEVEL_SUMMARY_ONLY
GENES = 2             # FASTF_LEVEL_GENES
CELLS = 8             # FASTF_LEVEL_CELLS
FIDELITY = 32         # FASTF_LEVEL_FIDELITY
GENE_FIDELITY = 128   # FASTF_LEVEL_GENE_FIDELITY
NEIGHBORS = 512       # FASTF_LEVEL_NEIGHBORS
COEXPRESSION = 4096   # FASTF_LEVEL_COEXPRESSION


def _renamed(columns):
    return tuple("umi_cap" if c == "reads_per_cell" else c for c in columns)


COLUMNS = _renamed(_cap.COLUMNS)
GENES_COLUMNS = _renamed(_cap.GENES_COLUMNS)
CELLS_COLUMNS = _renamed(_cap.CELLS_COLUMNS)
REPS_COLUMNS = _renamed(_cap.REPS_COLUMNS)
GENES_REPS_COLUMNS = _renamed(_cap.GENES_REPS_COLUMNS)
FIDELITY_COLUMNS = _renamed(_cap.FIDELITY_COLUMNS)
fidelity_row, fidelity_from_coo, read_point_fidelity = _sweep.fidelity_row, _sweep.fidelity_from_coo, _sweep.read_point_fidelity
GENE_FIDELITY_COLUMNS = _renamed(_cap.GENE_FIDELITY_COLUMNS)
gene_fidelity_row, gene_fidelity_from_coo, read_point_gene_fidelity = _sweep.gene_fidelity_row, _sweep.gene_fidelity_from_coo, _sweep.read_point_gene_fidelity
gene_fidelity_metrics = _sweep.gene_fidelity_metrics
NEIGHBORS_COLUMNS = _renamed(_cap.NEIGHBORS_COLUMNS)
LABELS_COLUMNS = _renamed(_cap.LABELS_COLUMNS)
LABEL_CLASSES_COLUMNS = _renamed(_cap.LABEL_CLASSES_COLUMNS)
MARKERS_COLUMNS = _renamed(_cap.MARKERS_COLUMNS)
COEXPRESSION_COLUMNS = _renamed(_cap.COEXPRESSION_COLUMNS)
MAPPING_COLUMNS = _renamed(_cap.MAPPING_COLUMNS)
PSEUDOTIME_COLUMNS = _renamed(_cap.PSEUDOTIME_COLUMNS)
read_point_pseudotime = _sweep.read_point_pseudotime
POINT_MAPPING_COLUMNS = _sweep.POINT_MAPPING_COLUMNS
mapping_from_coo, mapping_row, read_point_mapping = _sweep.mapping_from_coo, _sweep.mapping_row, _sweep.read_point_mapping
read_point_coexpression = _sweep.read_point_coexpression
neighbors_row, neighbors_from_coo, read_point_neighbors = _sweep.neighbors_row, _sweep.neighbors_from_coo, _sweep.read_point_neighbors
THRESHOLDS_COLUMNS = ("barcode", "threshold", "umis_full", "umis")
parse_seeds, reps_seeds, reps_point_dir = _sweep.parse_seeds, _sweep.reps_seeds, _sweep.reps_point_dir      # (one rule for the three verbs)
_flags = _sweep._flags      # (one flag word for the three verbs)


def level(bam, out, barcodes, features, rates_cell, umi_caps, seed: int = 926, summary_only: bool = False, genes: bool = False, cells: bool = False,
          fidelity: bool = False, gene_fidelity: bool = False, neighbors: bool = False, labels=None, markers=None, coexpression: bool = False, mapping: bool = False,
        pseudotime=None):
    """`fastF level -b bam -a barcodes -f features -o out -c rates_cell -m umi_caps -s seed [--summary-only] [--genes] [--cells]`; returns
    the rows of out/level.tsv as dicts of strings (read_table); genes / cells: the files cap.cap() leaves, under the names level_*; fidelity:
    out/level_fidelity.tsv (read_fidelity_table) and a fidelity.tsv.gz per point directory; gene_fidelity: out/level_gene_fidelity.tsv
    (read_gene_fidelity_table) and a gene_fidelity.tsv.gz per point directory; neighbors: out/level_neighbors.tsv (read_neighbors_table)
    and a neighbors.tsv.gz per point directory; labels=<path> (`--labels`): out/level_labels.tsv (read_labels_table),
    out/level_label_classes.tsv (read_label_classes_table) and labels.tsv.gz, label_confusion.tsv.gz per point directory"""
    _sweep._grid_call("level", bam, out, barcodes, features, rates_cell, _sweep._caps(umi_caps), None, seed,
                      _sweep._flags(summary_only, genes, cells, fidelity, gene_fidelity, neighbors, coexpression), labels, markers, mapping, pseudotime)
    return read_table(os.path.join(os.fspath(out), "level.tsv"))


def level_reps(bam, out, barcodes, features, rates_cell, umi_caps, seeds, summary_only: bool = False, genes: bool = False, cells: bool = False,
               fidelity: bool = False, gene_fidelity: bool = False, neighbors: bool = False, labels=None, markers=None, coexpression: bool = False, mapping: bool = False,
        pseudotime=None):
    """`fastF level ... --seeds seeds`: a replicate run (one seed included) — the points in out/<point>_s<seed>/, one row of
    out/level.tsv per (cell rate, seed, UMI cap), which are returned, and out/level_reps.tsv (read_reps_table)"""
    _sweep._grid_call("level", bam, out, barcodes, features, rates_cell, _sweep._caps(umi_caps), seeds, 0,
                      _sweep._flags(summary_only, genes, cells, fidelity, gene_fidelity, neighbors, coexpression), labels, markers, mapping, pseudotime)
    return read_table(os.path.join(os.fspath(out), "level.tsv"))


def _read(path, columns):
    lines = open(path).read().split("\n")
    assert lines[0].split("\t") == list(columns) and lines[-1] == ""
    return [dict(zip(columns, ln.split("\t"))) for ln in lines[1:-1]]


def read_table(path):
    """the rows of level.tsv as dicts of strings"""
    return _read(path, COLUMNS)


def read_genes_table(path):
    return _read(path, GENES_COLUMNS)


def read_cells_table(path):
    return _sweep.read_cells_table(path, CELLS_COLUMNS)


def read_fidelity_table(path):
    return _sweep.read_cells_table(path, FIDELITY_COLUMNS)


def fidelity_header(verb: str = "level") -> str:
    return _sweep.fidelity_header(verb)


def fidelity_summary_row(rate_cell, umi_cap, seed, umis_full, umis, genes_full, genes, sum_xx, sum_yy, sum_xy, n_features) -> str:
    """one row of level_fidelity.tsv (with its newline)"""
    return _sweep.fidelity_summary_row(rate_cell, 0.0, seed, umis_full, umis, genes_full, genes, sum_xx, sum_yy, sum_xy, n_features, list_value=int(umi_cap))


def read_gene_fidelity_table(path):
    return _sweep.read_cells_table(path, GENE_FIDELITY_COLUMNS)


def gene_fidelity_header(verb: str = "level") -> str:
    return _sweep.gene_fidelity_header(verb)


def gene_fidelity_summary_row(rate_cell, umi_cap, seed, n_cells, sum_x, sum_y, sum_xx, sum_yy, sum_xy) -> str:
    """one row of level_gene_fidelity.tsv (with its newline)"""
    return _sweep.gene_fidelity_summary_row(rate_cell, 0.0, seed, n_cells, sum_x, sum_y, sum_xx, sum_yy, sum_xy, list_value=int(umi_cap))


def read_neighbors_table(path):
    return _sweep.read_cells_table(path, NEIGHBORS_COLUMNS)


def read_pseudotime_table(path):
    """the rows of level_pseudotime.tsv as dicts of strings"""
    return _sweep.read_cells_table(path, PSEUDOTIME_COLUMNS)


def read_mapping_table(path):
    """the rows of level_mapping.tsv as dicts of strings"""
    return _sweep.read_cells_table(path, MAPPING_COLUMNS)


def mapping_header(verb: str = "level") -> str:
    return _sweep.mapping_header(verb)


def mapping_summary_row(rate_cell, umi_cap, seed, hvg_k, self_dot, self_rank, k_full, hood, lab=None, same_map=None, labelled_map=None) -> str:
    """one row of level_mapping.tsv (with its newline)"""
    return _sweep.mapping_summary_row(rate_cell, 0.0, seed, hvg_k, self_dot, self_rank, k_full, hood, lab, same_map, labelled_map, list_value=int(umi_cap))


def read_coexpression_table(path):
    return _sweep.read_cells_table(path, COEXPRESSION_COLUMNS)


def neighbors_header(verb: str = "level") -> str:
    return _sweep.neighbors_header(verb)


def neighbors_summary_row(rate_cell, umi_cap, seed, hvg_k, k_full, k_point, shared) -> str:
    """one row of level_neighbors.tsv (with its newline)"""
    return _sweep.neighbors_summary_row(rate_cell, 0.0, seed, hvg_k, k_full, k_point, shared, list_value=int(umi_cap))


def read_labels_table(path):
    return _sweep.read_cells_table(path, LABELS_COLUMNS)


def read_label_classes_table(path):
    return _sweep.read_cells_table(path, LABEL_CLASSES_COLUMNS)


def read_markers_table(path):
    return _sweep.read_cells_table(path, MARKERS_COLUMNS)


def read_reps_table(path):
    return _sweep.read_cells_table(path, REPS_COLUMNS)


def read_genes_reps_table(path):
    return _sweep.read_cells_table(path, GENES_REPS_COLUMNS)


def read_thresholds(path):
    """thresholds.tsv.gz of a point: (barcodes, T[k], U_k(2^32), U_k(T[k])) — a list of str and three uint64 arrays"""
    lines = gzip.decompress(open(path, "rb").read()).decode().split("\n")
    assert lines[0].split("\t") == list(THRESHOLDS_COLUMNS) and lines[-1] == ""
    rows = [ln.split("\t") for ln in lines[1:-1]]
    col = lambda i: np.array([int(r[i]) for r in rows], dtype=np.uint64)  # noqa: E731
    return [r[0] for r in rows], col(1), col(2), col(3)


def header() -> str:
    return _lib.lib().fastf_level_header().decode()


def genes_header() -> str:
    return _lib.lib().fastf_level_genes_header().decode()


def cells_header() -> str:
    return _lib.lib().fastf_level_cells_header().decode()


def reps_header() -> str:
    return _lib.lib().fastf_level_reps_header().decode()


def genes_reps_header() -> str:
    return _lib.lib().fastf_level_genes_reps_header().decode()


def parse_caps(text: str):
    """a comma-separated list of UMI caps as the command reads -m; raises FastfError on what it refuses"""
    out = np.zeros(64, dtype=np.uint64)
    n = C.c_uint32()
    _lib.check(_lib.lib().fastf_level_parse_caps(text.encode(), out.ctypes.data, len(out), C.byref(n)))
    return out[:n.value].copy()


def check_grid(rates_cell, umi_caps):
    rc = np.ascontiguousarray(rates_cell, dtype=np.float32)
    m = np.ascontiguousarray(umi_caps, dtype=np.uint64)
    _lib.check(_lib.lib().fastf_level_check_grid(rc.ctypes.data_as(C.POINTER(C.c_float)), len(rc), m.ctypes.data, len(m)))


def point_dir(rate_cell: float, umi_cap: int) -> str:
    buf = C.create_string_buffer(64)
    _lib.check(_lib.lib().fastf_level_point_dir(float(rate_cell), int(umi_cap), buf, len(buf)))
    return buf.value.decode()


def summary_row(rate_cell, umi_cap, seed, counters, nnz, umis, umis_per_cell, genes_per_cell, hits, cells_capped) -> str:
    """one row of level.tsv (with its newline)"""
    upc = np.ascontiguousarray(umis_per_cell, dtype=np.uint64)
    gpc = np.ascontiguousarray(genes_per_cell, dtype=np.uint32)
    cnt = (C.c_uint64 * 3)(*[int(x) for x in counters])
    buf = C.create_string_buffer(640)
    _lib.check(_lib.lib().fastf_level_summary_row(float(rate_cell), int(umi_cap), seed, C.byref(cnt), int(nnz), int(umis),
                                                  upc.ctypes.data, gpc.ctypes.data, len(upc), int(hits), int(cells_capped), buf, len(buf)))
    return buf.value.decode()
