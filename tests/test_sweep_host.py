"""Host pieces of `fastF sweep` (no GPU): the rate lists of -c / -r, the grid check, the point directories, and the summary
row of sweep.tsv from a hand-made COO against numpy."""
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, sweep


def test_rate_lists_parse_like_the_single_values_of_bam2db():
    np.testing.assert_array_equal(sweep.parse_rates("0.25,0.5,1", True), np.array([0.25, 0.5, 1], np.float32))
    np.testing.assert_array_equal(sweep.parse_rates("0,0.1,1e-1,2.5"), np.array([0, 0.1, 0.1, 2.5], np.float32))
    np.testing.assert_array_equal(sweep.parse_rates("1"), np.array([1], np.float32))
    np.testing.assert_array_equal(sweep.parse_rates(" 0.5"), np.array([0.5], np.float32))        # strtof skips leading blanks


@pytest.mark.parametrize("text,cells,word", [
    ("", False, "empty"), ("0.5,,1", False, "empty"), ("0.5,", False, "empty"), (",0.5", True, "empty"),
    ("-0.1", False, "negative"), ("0.5,-1", True, "negative"), ("-0", False, "negative"),
    ("nan", False, "not a number"), ("0.5,NaN", True, "not a number"),
    ("1.5", True, "sample size"), ("1.0000001", True, "sample size"),
    ("0.5x", False, "numerical"), ("abc", True, "numerical"), ("0.5 ", False, "numerical"), ("1e99", False, "out of range"),
])
def test_rate_lists_that_are_refused(text, cells, word):
    with pytest.raises(F.FastfError) as ei:
        sweep.parse_rates(text, cells)
    assert word in str(ei.value)


def test_a_depth_rate_above_one_is_taken_as_bam2db_takes_it():
    np.testing.assert_array_equal(sweep.parse_rates("1.5"), np.array([1.5], np.float32))


def test_rates_that_print_the_same_are_refused():
    sweep.check_grid([0.25, 0.5, 1], [0, 0.1, 0.5, 1])
    for rc, rd in (([0.5, 0.5], [1]), ([0.5], [0.1, 0.1004]), ([0.1234, 0.12341], [1]), ([1], [0.9996, 1.0])):
        with pytest.raises(F.FastfError) as ei:
            sweep.check_grid(rc, rd)
        assert "both print as" in str(ei.value)
    sweep.check_grid([0.5], [0.1, 0.1006])
    for rc, rd in (([], [1]), ([1], []), ([1.5], [1]), ([float("nan")], [1]), ([1], [-0.5])):
        with pytest.raises(F.FastfError):
            sweep.check_grid(rc, rd)


def test_point_directories_print_the_rates_as_the_matrix_header_does():
    assert sweep.point_dir(0.25, 1) == "c0.250_r1.000"
    assert sweep.point_dir(1, 0) == "c1.000_r0.000"
    assert sweep.point_dir(0.3, 0.1) == "c0.300_r0.100"
    assert sweep.point_dir(0.12345, 2.5) == "c0.123_r2.500"
    assert sweep.header().rstrip("\n").split("\t") == list(sweep.COLUMNS)


def _numpy_row(rate_cell, rate_depth, seed, counters, cell, count, n_cells):
    cell, count = np.asarray(cell, np.int64), np.asarray(count, np.int64)
    upc, gpc = np.zeros(n_cells, np.int64), np.zeros(n_cells, np.int64)
    np.add.at(upc, cell - 1, count)
    np.add.at(gpc, cell - 1, (count >= 1).astype(np.int64))
    umis = int(count.sum())
    sat = "%.6f" % (1.0 - umis / counters[2]) if counters[2] else "0.000000"
    med = lambda a: "%.1f" % (float(np.median(a)) if len(a) else 0.0)  # noqa: E731
    return "\t".join(["%.3f" % float(np.float32(rate_cell)), "%.3f" % float(np.float32(rate_depth)), str(seed), str(n_cells)] +
                     [str(c) for c in counters] + [str(len(cell)), str(umis), sat, med(upc), med(gpc)]) + "\n", upc, gpc, umis


@pytest.mark.parametrize("name,n_cells,cell,count,counters", [
    ("odd", 5, [1, 1, 2, 4, 4, 4, 5], [3, 1, 7, 2, 2, 9, 1], [100, 60, 40]),
    ("even", 4, [1, 1, 2, 4, 4, 4], [3, 1, 7, 2, 2, 10], [100, 60, 41]),
    ("even_middle_mean", 2, [1, 2, 2], [2, 3, 4], [9, 9, 9]),
    ("cells_without_rows", 6, [2, 5], [4, 6], [50, 20, 10]),
    ("count_zero_rows", 3, [1, 1, 2, 3, 3], [0, 2, 0, 0, 0], [30, 20, 12]),
    ("zero_denominator", 3, [], [], [30, 0, 0]),
    ("only_count_zero", 2, [1, 2], [0, 0], [5, 5, 2]),
    ("one_cell", 1, [1, 1, 1], [1, 2, 3], [6, 6, 6]),
    ("no_cells", 0, [], [], [7, 0, 0]),
    ("large_counts", 3, [1, 2, 3], [4_000_000_000, 4_000_000_000, 1], [2 ** 40, 2 ** 39, 2 ** 38]),
])
def test_summary_row_against_numpy(name, n_cells, cell, count, counters):
    upc, gpc, umis = sweep.cells_from_coo(cell, count, n_cells)
    want, w_upc, w_gpc, w_umis = _numpy_row(0.3, 0.1, 926, counters, cell, count, n_cells)
    np.testing.assert_array_equal(upc.astype(np.int64), w_upc)
    np.testing.assert_array_equal(gpc.astype(np.int64), w_gpc)
    assert umis == w_umis
    assert sweep.summary_row(0.3, 0.1, 926, counters, len(cell), umis, upc, gpc) == want


def test_summary_row_random_against_numpy():
    rng = np.random.default_rng(5)
    for n_cells in (1, 2, 7, 64, 1001):
        nnz = int(rng.integers(0, 5 * n_cells))
        cell = np.sort(rng.integers(1, n_cells + 1, size=nnz))
        count = rng.integers(0, 4, size=nnz)
        counters = [10 * nnz + 5, 5 * nnz + 3, int(count.sum()) + int(rng.integers(0, 50))]
        upc, gpc, umis = sweep.cells_from_coo(cell, count, n_cells)
        want = _numpy_row(0.5, 0.25, 1, counters, cell, count, n_cells)[0]
        assert sweep.summary_row(0.5, 0.25, 1, counters, nnz, umis, upc, gpc) == want


def test_a_row_that_names_a_cell_outside_the_list_is_an_error():
    with pytest.raises(F.FastfError):
        sweep.cells_from_coo([1, 9], [1, 1], 3)


def test_cli_refuses_before_anything_is_read(tmp_path):
    """-u, colliding rates, bad lists, a missing BAM: exit 1 with a message, no sweep.tsv"""
    cli = _lib.cli_path()
    out = tmp_path / "out"
    base = [cli, "sweep", "-b", str(tmp_path / "missing.bam"), "-a", str(tmp_path / "b.tsv"), "-f", str(tmp_path / "f.tsv"), "-o", str(out)]
    for extra, word in ((["-u"], "umi.tsv.gz"), (["-c", "0.5,0.5004"], "both print as"), (["--cell=0.5,"], "empty"),
                        (["-r", "nan"], "not a number"), (["-c", "1.5"], "sample size"), (["-c", "0.5", "-r", "0.5"], "does not exist")):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode == 1 and word in r.stderr, (extra, r.stderr)
        assert not (out / "sweep.tsv").exists()
    r = subprocess.run([cli, "sweep", "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "--summary-only" in r.stdout
    r = subprocess.run([cli, "-h"], capture_output=True, text=True)
    assert "sweep" in r.stdout
