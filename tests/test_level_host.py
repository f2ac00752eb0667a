"""`fastF level`, the parts that need no device: list parsing, the grid check, directory names, every header against cap's with the
one column renamed, a level.tsv row against numpy, the Python mirror's column tuples, and the error exits of the command line."""
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, cap, level, synth
from cap_ref import realised


def test_list_parsing_and_its_refusals():
    np.testing.assert_array_equal(level.parse_caps("1,5,40,1000000"), [1, 5, 40, 1000000])
    np.testing.assert_array_equal(level.parse_caps("18446744073709551615"), [2 ** 64 - 1])
    np.testing.assert_array_equal(level.parse_caps(",".join(str(i) for i in range(1, 65))), np.arange(1, 65))
    for bad in ["", ",", "1,", ",1", "1,,2", "0", "5,0", "-1", "+3", "1.5", "7 ", " 7", "x", "3,3", "18446744073709551616",
                ",".join(str(i) for i in range(1, 66))]:
        with pytest.raises(F.FastfError) as ei:
            level.parse_caps(bad)
        assert "UMIs per cell" in str(ei.value) and "reads per cell" not in str(ei.value), str(ei.value)


def test_grid_check():
    level.check_grid([0.5, 1], [1, 2])
    for rc, m in [([], [1]), ([1], []), ([1], [0]), ([1], [4, 4]), ([0.5, 0.5001], [1]), ([1.5], [1]), ([-0.1], [1])]:
        with pytest.raises(F.FastfError) as ei:
            level.check_grid(rc, m)
        assert str(ei.value).startswith("level: ") and "cap:" not in str(ei.value), str(ei.value)


def test_directory_names():
    assert level.point_dir(0.5, 40) == "c0.500_m40" and level.point_dir(1, 1000000) == "c1.000_m1000000"
    assert level.point_dir(np.float32(0.3), 1) == "c0.300_m1"
    assert level.reps_point_dir(level.point_dir(0.5, 7), 927) == "c0.500_m7_s927"


def test_every_header_is_caps_with_the_one_column_renamed():
    pairs = [(level.header(), cap.header()), (level.genes_header(), cap.genes_header()), (level.cells_header(), cap.cells_header()),
             (level.reps_header(), cap.reps_header()), (level.genes_reps_header(), cap.genes_reps_header())]
    for got, theirs in pairs:
        a, b = got.rstrip("\n").split("\t"), theirs.rstrip("\n").split("\t")
        assert got.endswith("\n") and len(a) == len(b)
        assert a[1] == "umi_cap" and b[1] == "reads_per_cell" and a[0] == b[0] == "rate_cell" and a[2:] == b[2:]
    assert "median_reads_per_cell" in level.cells_header()                 # (a column that only contains the old name keeps it)
    assert level.header().split("\t")[12:] == ["hits", "cells_capped", "realised_depth\n"]


def test_the_python_mirrors_column_tuples():
    assert level.header() == "\t".join(level.COLUMNS) + "\n"
    assert level.genes_header() == "\t".join(level.GENES_COLUMNS) + "\n"
    assert level.cells_header() == "\t".join(level.CELLS_COLUMNS) + "\n"
    assert level.reps_header() == "\t".join(level.REPS_COLUMNS) + "\n"
    assert level.genes_reps_header() == "\t".join(level.GENES_REPS_COLUMNS) + "\n"
    for mine, theirs in [(level.COLUMNS, cap.COLUMNS), (level.GENES_COLUMNS, cap.GENES_COLUMNS), (level.CELLS_COLUMNS, cap.CELLS_COLUMNS),
                         (level.REPS_COLUMNS, cap.REPS_COLUMNS), (level.GENES_REPS_COLUMNS, cap.GENES_REPS_COLUMNS)]:
        assert mine == tuple("umi_cap" if c == "reads_per_cell" else c for c in theirs) and mine.count("umi_cap") == 1
    assert (level.SUMMARY_ONLY, level.GENES, level.CELLS) == (1, 2, 8)
    assert level.THRESHOLDS_COLUMNS == ("barcode", "threshold", "umis_full", "umis")
    assert F.level is level and "level" in F.__all__


def test_one_row_against_numpy():
    rng = np.random.default_rng(6)
    upc = rng.integers(0, 41, size=1000).astype(np.uint64)
    gpc = rng.integers(0, 30, size=1000).astype(np.uint32)
    counters = (123456, 50000, 41000)
    umis, hits = int(upc.sum()), 77777
    row = level.summary_row(0.5, 40, 926, counters, 31234, umis, upc, gpc, hits, 17)
    want = ["0.500", "40", "926", "1000", "123456", "50000", "41000", "31234", str(umis), "%.6f" % (1.0 - umis / 41000),
            "%.1f" % float(np.median(upc)), "%.1f" % float(np.median(gpc)), "77777", "17", "%.6f" % realised(50000, 77777)]
    assert row == "\t".join(want) + "\n"
    assert row == cap.summary_row(0.5, 40, 926, counters, 31234, umis, upc, gpc, hits, 17)
    row0 = level.summary_row(1, 3, 1, (0, 0, 0), 0, 0, np.zeros(0, np.uint64), np.zeros(0, np.uint32), 0, 0)
    assert row0.split("\t")[-1] == "1.000000\n" and row0.split("\t")[9] == "0.000000"


TABLES = ("level.tsv", "level_genes.tsv", "level_cells.tsv", "level_reps.tsv", "level_genes_reps.tsv", "level_gene_cells.tsv.gz", "level_gene_reps.tsv.gz")


def _no_table(out):
    return not out.exists() or [n for n in os.listdir(out) if n.startswith("level")] == []


def test_error_exits_leave_no_table(tmp_path):
    bt, ft, bar, genes = synth.make_lists(5, 3)
    fl, xf, cb, gx, ub = synth.make_records(20, bar, genes)
    bam, b, f = tmp_path / "x.bam", tmp_path / "b.tsv", tmp_path / "f.tsv"
    synth.write_bam(str(bam), fl, xf, cb, gx, ub)
    b.write_bytes(bt); f.write_bytes(ft)
    base = ["-a", str(b), "-f", str(f), "-b", str(bam), "--genes", "--cells"]
    several = dict(os.environ, FASTF_DEVICES="0,1")
    cases = [([], "needs -m", None), (["-m", "5", "-u"], "umi.tsv.gz", None), (["-m", "0"], "at least 1", None), (["--umis", "3,3"], "listed twice", None),
             (["-m", ""], "empty element", None), (["-m", "5", "-c", "0.5,0.5001"], "both print as", None), (["-m", "5", "--bogus"], "unknown option", None),
             (["-m", "5"], "several devices", several), (["--umis=5,9", "--seeds", "1,2"], "several devices", several),
             (["-m", "5", "-b", str(tmp_path / "missing.bam")], "does not exist", None)]
    for k, (args, word, env) in enumerate(cases):
        out = tmp_path / ("out%d" % k)
        r = subprocess.run([_lib.cli_path(), "level", "-o", str(out)] + base + args, capture_output=True, text=True, timeout=60, env=env)
        assert r.returncode == 1, (args, r.stderr)
        assert word in r.stderr, (args, r.stderr)
        assert "reads per cell" not in r.stderr
        assert _no_table(out), (args, os.listdir(out))
    os.environ["FASTF_DEVICES"] = "0,1"
    try:
        with pytest.raises(F.FastfError) as ei:
            level.level(bam, tmp_path / "o", b, f, [1], [5])
        assert "no point-by-point form" in str(ei.value)
        with pytest.raises(F.FastfError):
            level.level_reps(bam, tmp_path / "o", b, f, [1], [5], [1, 2], genes=True)
    finally:
        del os.environ["FASTF_DEVICES"]
    with pytest.raises(F.FastfError):
        level.level(tmp_path / "missing.bam", tmp_path / "o", b, f, [1], [5])
    with pytest.raises(F.FastfError):
        level.level(bam, tmp_path / "o", b, f, [1], [0])
    assert _no_table(tmp_path / "o")


def test_help_lists_the_verb():
    r = subprocess.run([_lib.cli_path(), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "\n    level " in r.stdout and "at most M UMIs" in r.stdout
    r = subprocess.run([_lib.cli_path(), "level", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--umis" in r.stdout and "thresholds.tsv.gz" in r.stdout
    names = _lib.lib().fastf_kernel_names().decode().split(",")
    assert "level_step_kernel" in names
    for sym in ("fastf_level", "fastf_level_reps", "fastf_dev_level_init", "fastf_dev_level_step", "fastf_level_point_dir", "fastf_level_header"):
        assert sym in _lib.ABI_SYMBOLS
