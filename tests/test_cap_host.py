"""`fastF cap`, the parts that need no device: the per-cell thresholds against their numpy restatement, list parsing, directory
names, the cap.tsv header and a row, and the error exits of the command line — and the builder of the records
tests/test_gpu_cap.py counts at the last LDS range, with its census."""
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, cap
from cap_ref import draw_threshold, realised, thresholds


CAP_LDS_CELLS, CAP_LDS_RANGES = 32768, 8                                 # cap_kernels.hpp


def last_range_cells(n_cells):
    """the cell index (0: no hit) of every record for a table of n_cells cells, 8 x 32 768 or one more — the most the LDS form of
    cell_hits_kernel takes, and the first table of the general form: 600 records in a row on the last cell of the seventh range
    (two whole 256-record units of one cell), then, shuffled, 3000 random records, a third of them misses, and seven records each
    on the first and the last cell of every range and on no cell at all"""
    rng = np.random.default_rng(n_cells)
    special = [0]
    for lo in range(0, n_cells, CAP_LDS_CELLS):
        special += [lo + 1, min(lo + CAP_LDS_CELLS, n_cells)]
    c = np.concatenate([rng.integers(1, n_cells + 1, size=3000), np.repeat(np.array(special, np.int64), 7)])
    c[:3000][rng.random(3000) < 1 / 3] = 0
    return np.concatenate([np.full(600, 7 * CAP_LDS_CELLS), rng.permutation(c)])


@pytest.mark.parametrize("n_cells", [CAP_LDS_CELLS * CAP_LDS_RANGES, CAP_LDS_CELLS * CAP_LDS_RANGES + 1])
def test_census_of_the_last_range_records(n_cells):
    """np.bincount alone, against a plain loop over the records: every edge cell has its hits, a miss adds nothing"""
    cell = last_range_cells(n_cells)
    assert 3000 < len(cell) < 4000 and (cell[:600] == 7 * CAP_LDS_CELLS).all() and 800 < (cell == 0).sum() < 1300
    want = [0] * n_cells
    for c in cell.tolist():
        if c:
            want[c - 1] += 1
    assert np.bincount(cell[cell > 0] - 1, minlength=n_cells).tolist() == want
    for lo in range(0, n_cells, CAP_LDS_CELLS):                           # 8 ranges, or 8 and a ninth of one cell
        for c in (lo + 1, min(lo + CAP_LDS_CELLS, n_cells)):
            assert want[c - 1] >= (607 if c == 7 * CAP_LDS_CELLS else 7)
    assert (n_cells + CAP_LDS_CELLS - 1) // CAP_LDS_CELLS == (8 if n_cells == CAP_LDS_CELLS * CAP_LDS_RANGES else 9)


def test_draw_threshold_restatement_is_the_library_function():
    for r in [0.0, 1e-9, 0.1, 1 / 3, 0.5, 7 / 21, 0.999999, 1.0, 1.5, float(np.float32(1e6) / np.float32(2 ** 31))]:
        assert draw_threshold(r) == F.draw_threshold(float(np.float32(r))), r


@pytest.mark.parametrize("n", [1, 7, 10 ** 6])
def test_thresholds_against_numpy(n):
    h = np.array(sorted({0, 1, max(n - 1, 0), n, n + 1, 3 * n, 2 ** 31}), dtype=np.uint32)
    got = cap.thresholds(h, n)
    np.testing.assert_array_equal(got, thresholds(h, n))
    assert (got[h <= n] == np.uint64(1 << 32)).all()                      # a cell at or below the cap loses no read
    assert (got[h > n] < np.uint64(1 << 32)).all() and (got[h > n] > 0).all()
    t3 = int(got[list(h).index(3 * n)])
    assert abs(t3 / 2 ** 32 - 1 / 3) < 1e-6
    assert len(cap.thresholds(np.zeros(0, np.uint32), n)) == 0
    with pytest.raises(F.FastfError):
        cap.thresholds(h, 0)


def test_list_parsing():
    np.testing.assert_array_equal(cap.parse_caps("1,5,40,1000000"), [1, 5, 40, 1000000])
    np.testing.assert_array_equal(cap.parse_caps("18446744073709551615"), [2 ** 64 - 1])
    for bad in ["", ",", "1,", ",1", "1,,2", "0", "5,0", "-1", "+3", "1.5", "7 ", " 7", "x", "3,3", "18446744073709551616",
                ",".join(str(i) for i in range(1, 66))]:
        with pytest.raises(F.FastfError):
            cap.parse_caps(bad)
    cap.check_grid([0.5, 1], [1, 2])
    for rc, n in [([], [1]), ([1], []), ([1], [0]), ([1], [4, 4]), ([0.5, 0.5001], [1]), ([1.5], [1]), ([-0.1], [1])]:
        with pytest.raises(F.FastfError):
            cap.check_grid(rc, n)


def test_directory_names_and_header():
    assert cap.point_dir(0.5, 40) == "c0.500_n40" and cap.point_dir(1, 1000000) == "c1.000_n1000000"
    assert cap.point_dir(np.float32(0.3), 1) == "c0.300_n1"
    assert cap.header() == "\t".join(cap.COLUMNS) + "\n"
    from fastf_amd import sweep
    assert cap.COLUMNS[:12] == tuple("reads_per_cell" if c == "rate_depth" else c for c in sweep.COLUMNS)
    assert cap.COLUMNS[12:] == ("hits", "cells_capped", "realised_depth")


def test_one_row_against_numpy():
    rng = np.random.default_rng(5)
    upc = rng.integers(0, 900, size=1000).astype(np.uint64)
    gpc = rng.integers(0, 300, size=1000).astype(np.uint32)
    counters = (123456, 50000, 41000)
    umis, hits = int(upc.sum()), 77777
    row = cap.summary_row(0.5, 40, 926, counters, 31234, umis, upc, gpc, hits, 17)
    want = ["0.500", "40", "926", "1000", "123456", "50000", "41000", "31234", str(umis), "%.6f" % (1.0 - umis / 41000),
            "%.1f" % float(np.median(upc)), "%.1f" % float(np.median(gpc)), "77777", "17", "%.6f" % realised(50000, 77777)]
    assert row == "\t".join(want) + "\n"
    row0 = cap.summary_row(1, 3, 1, (0, 0, 0), 0, 0, np.zeros(0, np.uint64), np.zeros(0, np.uint32), 0, 0)
    assert row0.split("\t")[-1] == "1.000000\n" and row0.split("\t")[9] == "0.000000"
    assert cap.realised(0, 0) == 1.0 and cap.realised(1, 3) == realised(1, 3)


def test_error_exits_that_need_no_device(tmp_path):
    b, f = tmp_path / "b.tsv", tmp_path / "f.tsv"
    b.write_text("AAAA-1\n"); f.write_text("ENSG00000000001\tG\tGene Expression\n")
    base = ["-a", str(b), "-f", str(f), "-b", str(tmp_path / "missing.bam")]
    for k, (args, word) in enumerate([(["-n", "0"], "at least 1"), (["-n", ""], "empty element"), (["-n", "3,3"], "listed twice"),
                                      ([], "needs -n"), (["-n", "5", "-c", "0.5,0.5001"], "both print as"), (["-n", "5", "-u"], "umi.tsv.gz"),
                                      (["-n", "5"], "does not exist"), (["-n", "5", "--bogus"], "unknown option")]):
        out = tmp_path / ("out%d" % k)
        r = subprocess.run([_lib.cli_path(), "cap", "-o", str(out)] + base + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1, (args, r.stderr)
        assert word in r.stderr, (args, r.stderr)
        assert not (out / "cap.tsv").exists() and not (out / "cap.tsv.partial").exists()
    r = subprocess.run([_lib.cli_path(), "cap", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--reads" in r.stdout
    with pytest.raises(F.FastfError):
        cap.cap(tmp_path / "missing.bam", tmp_path / "o", b, f, [1], [5])
    with pytest.raises(F.FastfError):
        cap.cap(tmp_path / "missing.bam", tmp_path / "o", b, f, [1], [0])
    assert "fastf_cap" in _lib.ABI_SYMBOLS and "cell_hits_kernel" in _lib.lib().fastf_kernel_names().decode()
