"""Python mirror of `fastF cap` (include/fastf_amd.h: fastf_cap and its host pieces): every cell downsampled to at most N reads,
over a grid of (cell rate, cap) points from one decode of the BAM.  Nothing here computes results: every call lands in the library."""
import ctypes as C
import os

import numpy as np

from . import _lib
from . import sweep as _sweep

SUMMARY_ONLY = 1      # FASTF_CAP_SUMMARY_ONLY
GENES = 2             # FASTF_CAP_GENES
CELLS = 8             # FASTF_CAP_CELLS
FIDELITY = 32         # FASTF_CAP_FIDELITY
GENE_FIDELITY = 128   # FASTF_CAP_GENE_FIDELITY
NEIGHBORS = 512       # FASTF_CAP_NEIGHBORS
COEXPRESSION = 4096   # FASTF_CAP_COEXPRESSION
COLUMNS = ("rate_cell", "reads_per_cell", "seed", "n_cells", "total_reads", "sampled_reads", "sampled_valid_reads", "nnz", "umis",
           "saturation", "median_umis_per_cell", "median_genes_per_cell", "hits", "cells_capped", "realised_depth")
GENES_COLUMNS = ("rate_cell", "reads_per_cell", "seed", "genes_detected", "genes_min_cells_3", "genes_min_cells_10", "max_gene_umis")
CELLS_COLUMNS = ("rate_cell", "reads_per_cell") + _sweep.CELLS_TAIL_COLUMNS
FIDELITY_COLUMNS = ("rate_cell", "reads_per_cell") + _sweep.FIDELITY_TAIL_COLUMNS
fidelity_row, fidelity_from_coo, read_point_fidelity = _sweep.fidelity_row, _sweep.fidelity_from_coo, _sweep.read_point_fidelity
GENE_FIDELITY_COLUMNS = ("rate_cell", "reads_per_cell") + _sweep.GENE_FIDELITY_TAIL_COLUMNS
gene_fidelity_row, gene_fidelity_from_coo, read_point_gene_fidelity = _sweep.gene_fidelity_row, _sweep.gene_fidelity_from_coo, _sweep.read_point_gene_fidelity
gene_fidelity_metrics = _sweep.gene_fidelity_metrics
NEIGHBORS_COLUMNS = ("rate_cell", "reads_per_cell") + _sweep.NEIGHBORS_TAIL_COLUMNS
LABELS_COLUMNS = ("rate_cell", "reads_per_cell") + _sweep.LABELS_TAIL_COLUMNS
LABEL_CLASSES_COLUMNS = ("rate_cell", "reads_per_cell") + _sweep.LABEL_CLASSES_TAIL_COLUMNS
MARKERS_COLUMNS = ("rate_cell", "reads_per_cell") + _sweep.MARKERS_TAIL_COLUMNS
COEXPRESSION_COLUMNS = ("rate_cell", "reads_per_cell") + _sweep.COEXPRESSION_TAIL_COLUMNS
MAPPING_COLUMNS = ("rate_cell", "reads_per_cell") + _sweep.MAPPING_TAIL_COLUMNS
PSEUDOTIME_COLUMNS = ("rate_cell", "reads_per_cell") + _sweep.PSEUDOTIME_TAIL_COLUMNS
read_point_pseudotime = _sweep.read_point_pseudotime
POINT_MAPPING_COLUMNS = _sweep.POINT_MAPPING_COLUMNS
mapping_from_coo, mapping_row, read_point_mapping = _sweep.mapping_from_coo, _sweep.mapping_row, _sweep.read_point_mapping
read_point_coexpression = _sweep.read_point_coexpression
neighbors_row, neighbors_from_coo, read_point_neighbors = _sweep.neighbors_row, _sweep.neighbors_from_coo, _sweep.read_point_neighbors
copies_from_umi_rows = _sweep.copies_from_umi_rows      # (the host twin is one function for both verbs)


def cap(bam, out, barcodes, features, rates_cell, caps, seed: int = 926, summary_only: bool = False, genes: bool = False, cells: bool = False,
        fidelity: bool = False, gene_fidelity: bool = False, neighbors: bool = False, labels=None, markers=None, coexpression: bool = False, mapping: bool = False,
        pseudotime=None):
    """`fastF cap -b bam -a barcodes -f features -o out -c rates_cell -n caps -s seed [--summary-only] [--genes] [--cells]`; returns the
    rows of out/cap.tsv as dicts of strings (read_table); genes=True also leaves out/cap_genes.tsv (read_genes_table),
    out/cap_gene_cells.tsv.gz and a genes.tsv.gz per point directory; cells=True also leaves out/cap_cells.tsv (read_cells_table) and
    a cells.tsv.gz per point directory; fidelity=True also leaves out/cap_fidelity.tsv (read_fidelity_table) and a fidelity.tsv.gz per
    point directory; gene_fidelity=True out/cap_gene_fidelity.tsv (read_gene_fidelity_table) and a gene_fidelity.tsv.gz per point directory;
    neighbors=True out/cap_neighbors.tsv (read_neighbors_table) and a neighbors.tsv.gz per point directory; labels=<path> (`--labels`)
    out/cap_labels.tsv (read_labels_table), out/cap_label_classes.tsv (read_label_classes_table) and labels.tsv.gz,
    label_confusion.tsv.gz per point directory"""
    _sweep._grid_call("cap", bam, out, barcodes, features, rates_cell, _sweep._caps(caps), None, seed,
                      _sweep._flags(summary_only, genes, cells, fidelity, gene_fidelity, neighbors, coexpression), labels, markers, mapping, pseudotime)
    return read_table(os.path.join(os.fspath(out), "cap.tsv"))


def cap_reps(bam, out, barcodes, features, rates_cell, caps, seeds, summary_only: bool = False, genes: bool = False, cells: bool = False,
             fidelity: bool = False, gene_fidelity: bool = False, neighbors: bool = False, labels=None, markers=None, coexpression: bool = False, mapping: bool = False,
        pseudotime=None):
    """`fastF cap ... --seeds seeds`: a replicate run (one seed included) — the points in out/<point>_s<seed>/, one row of out/cap.tsv
    per (cell rate, seed, cap), which are returned (read_table), and out/cap_reps.tsv (read_reps_table); genes=True leaves
    out/cap_genes.tsv, out/cap_genes_reps.tsv (read_genes_reps_table) and out/cap_gene_reps.tsv.gz"""
    _sweep._grid_call("cap", bam, out, barcodes, features, rates_cell, _sweep._caps(caps), seeds, 0,
                      _sweep._flags(summary_only, genes, cells, fidelity, gene_fidelity, neighbors, coexpression), labels, markers, mapping, pseudotime)
    return read_table(os.path.join(os.fspath(out), "cap.tsv"))


REPS_COLUMNS = ("rate_cell", "reads_per_cell") + _sweep.REPS_TAIL_COLUMNS
GENES_REPS_COLUMNS = ("rate_cell", "reads_per_cell") + _sweep.GENES_REPS_TAIL_COLUMNS
parse_seeds, reps_seeds, reps_point_dir = _sweep.parse_seeds, _sweep.reps_seeds, _sweep.reps_point_dir      # (one rule for both verbs)


def read_fidelity_table(path):
    """the rows of cap_fidelity.tsv as dicts of strings"""
    return _sweep.read_cells_table(path, FIDELITY_COLUMNS)


def fidelity_header(verb: str = "cap") -> str:
    return _sweep.fidelity_header(verb)


def fidelity_summary_row(rate_cell, reads_per_cell, seed, umis_full, umis, genes_full, genes, sum_xx, sum_yy, sum_xy, n_features) -> str:
    """one row of cap_fidelity.tsv (with its newline)"""
    return _sweep.fidelity_summary_row(rate_cell, 0.0, seed, umis_full, umis, genes_full, genes, sum_xx, sum_yy, sum_xy, n_features, list_value=int(reads_per_cell))


def read_gene_fidelity_table(path):
    """the rows of cap_gene_fidelity.tsv as dicts of strings"""
    return _sweep.read_cells_table(path, GENE_FIDELITY_COLUMNS)


def gene_fidelity_header(verb: str = "cap") -> str:
    return _sweep.gene_fidelity_header(verb)


def gene_fidelity_summary_row(rate_cell, reads_per_cell, seed, n_cells, sum_x, sum_y, sum_xx, sum_yy, sum_xy) -> str:
    """one row of cap_gene_fidelity.tsv (with its newline)"""
    return _sweep.gene_fidelity_summary_row(rate_cell, 0.0, seed, n_cells, sum_x, sum_y, sum_xx, sum_yy, sum_xy, list_value=int(reads_per_cell))


def read_neighbors_table(path):
    """the rows of cap_neighbors.tsv as dicts of strings"""
    return _sweep.read_cells_table(path, NEIGHBORS_COLUMNS)


def read_pseudotime_table(path):
    """the rows of cap_pseudotime.tsv as dicts of strings"""
    return _sweep.read_cells_table(path, PSEUDOTIME_COLUMNS)


def read_mapping_table(path):
    """the rows of cap_mapping.tsv as dicts of strings"""
    return _sweep.read_cells_table(path, MAPPING_COLUMNS)


def mapping_header(verb: str = "cap") -> str:
    return _sweep.mapping_header(verb)


def mapping_summary_row(rate_cell, reads_per_cell, seed, hvg_k, self_dot, self_rank, k_full, hood, lab=None, same_map=None, labelled_map=None) -> str:
    """one row of cap_mapping.tsv (with its newline)"""
    return _sweep.mapping_summary_row(rate_cell, 0.0, seed, hvg_k, self_dot, self_rank, k_full, hood, lab, same_map, labelled_map, list_value=int(reads_per_cell))


def read_coexpression_table(path):
    """the rows of cap_coexpr.tsv as dicts of strings"""
    return _sweep.read_cells_table(path, COEXPRESSION_COLUMNS)


def neighbors_header(verb: str = "cap") -> str:
    return _sweep.neighbors_header(verb)


def neighbors_summary_row(rate_cell, reads_per_cell, seed, hvg_k, k_full, k_point, shared) -> str:
    """one row of cap_neighbors.tsv (with its newline)"""
    return _sweep.neighbors_summary_row(rate_cell, 0.0, seed, hvg_k, k_full, k_point, shared, list_value=int(reads_per_cell))


def read_labels_table(path):
    """the rows of cap_labels.tsv as dicts of strings"""
    return _sweep.read_cells_table(path, LABELS_COLUMNS)


def read_label_classes_table(path):
    """the rows of cap_label_classes.tsv as dicts of strings"""
    return _sweep.read_cells_table(path, LABEL_CLASSES_COLUMNS)


def read_markers_table(path):
    """the rows of cap_markers.tsv as dicts of strings"""
    return _sweep.read_cells_table(path, MARKERS_COLUMNS)


def read_reps_table(path):
    """the rows of cap_reps.tsv as dicts of strings"""
    return _sweep.read_cells_table(path, REPS_COLUMNS)


def read_genes_reps_table(path):
    """the rows of cap_genes_reps.tsv as dicts of strings"""
    return _sweep.read_cells_table(path, GENES_REPS_COLUMNS)


def reps_header() -> str:
    return _lib.lib().fastf_cap_reps_header().decode()


def genes_reps_header() -> str:
    return _lib.lib().fastf_cap_genes_reps_header().decode()


def reps_summary_row(rate_cell, reads_per_cell, n_cells, metrics) -> str:
    """one row of cap_reps.tsv (with its newline)"""
    return _sweep.reps_summary_row(rate_cell, 0.0, n_cells, metrics, reads_per_cell=int(reads_per_cell))


def read_table(path):
    lines = open(path).read().split("\n")
    assert lines[0].split("\t") == list(COLUMNS) and lines[-1] == ""
    return [dict(zip(COLUMNS, ln.split("\t"))) for ln in lines[1:-1]]


def read_genes_table(path):
    """the rows of cap_genes.tsv as dicts of strings"""
    lines = open(path).read().split("\n")
    assert lines[0].split("\t") == list(GENES_COLUMNS) and lines[-1] == ""
    return [dict(zip(GENES_COLUMNS, ln.split("\t"))) for ln in lines[1:-1]]


def read_cells_table(path):
    """the rows of cap_cells.tsv as dicts of strings"""
    return _sweep.read_cells_table(path, CELLS_COLUMNS)


def cells_header() -> str:
    return _lib.lib().fastf_cap_cells_header().decode()


def cells_summary_row(rate_cell, reads_per_cell, seed, reads, null_reads, single, hist) -> str:
    """one row of cap_cells.tsv (with its newline)"""
    return _sweep.cells_summary_row(rate_cell, 0.0, seed, reads, null_reads, single, hist, reads_per_cell=int(reads_per_cell))


def genes_header() -> str:
    return _lib.lib().fastf_cap_genes_header().decode()


def parse_caps(text: str):
    """a comma-separated list of caps as the command reads -n; raises FastfError on what it refuses"""
    out = np.zeros(64, dtype=np.uint64)
    n = C.c_uint32()
    _lib.check(_lib.lib().fastf_cap_parse_caps(text.encode(), out.ctypes.data, len(out), C.byref(n)))
    return out[:n.value].copy()


def check_grid(rates_cell, caps):
    rc = np.ascontiguousarray(rates_cell, dtype=np.float32)
    n = np.ascontiguousarray(caps, dtype=np.uint64)
    _lib.check(_lib.lib().fastf_cap_check_grid(rc.ctypes.data_as(C.POINTER(C.c_float)), len(rc), n.ctypes.data, len(n)))


def point_dir(rate_cell: float, reads_per_cell: int) -> str:
    buf = C.create_string_buffer(64)
    _lib.check(_lib.lib().fastf_cap_point_dir(float(rate_cell), int(reads_per_cell), buf, len(buf)))
    return buf.value.decode()


def header() -> str:
    return _lib.lib().fastf_cap_header().decode()


def thresholds(hits, reads_per_cell: int):
    """T[k] of include/fastf_amd.h from the hits per cell: 2^32 where hits[k] <= reads_per_cell, else
    fastf_draw_threshold((float)(reads_per_cell / hits[k]))"""
    h = np.ascontiguousarray(hits, dtype=np.uint32)
    t = np.zeros(max(len(h), 1), dtype=np.uint64)
    _lib.check(_lib.lib().fastf_cap_thresholds(h.ctypes.data, len(h), int(reads_per_cell), t.ctypes.data))
    return t[:len(h)]


def realised(sampled: int, hits: int) -> float:
    return float(_lib.lib().fastf_cap_realised(int(sampled), int(hits)))


def summary_row(rate_cell, reads_per_cell, seed, counters, nnz, umis, umis_per_cell, genes_per_cell, hits, cells_capped) -> str:
    """one row of cap.tsv (with its newline)"""
    upc = np.ascontiguousarray(umis_per_cell, dtype=np.uint64)
    gpc = np.ascontiguousarray(genes_per_cell, dtype=np.uint32)
    cnt = (C.c_uint64 * 3)(*[int(x) for x in counters])
    buf = C.create_string_buffer(640)
    _lib.check(_lib.lib().fastf_cap_summary_row(float(rate_cell), int(reads_per_cell), seed, C.byref(cnt), int(nnz), int(umis),
                                                upc.ctypes.data, gpc.ctypes.data, len(upc), int(hits), int(cells_capped), buf, len(buf)))
    return buf.value.decode()
