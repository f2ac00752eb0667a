"""--fidelity, the parts that need no device: the host twin of the join against the numpy reference, the missing-partner error, the
rows and headers, the NA rules, the median and p10 rule, the flag on the three verbs and the refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, cap, level, sweep, synth
import fidelity_ref as R


def nested_pair(rng, n_cells, n_features, density, keep, zero_rate=0.1, big=False):
    """a full COO ascending by (cell, feature) and a point that keeps a row subset with counts <= the full counts; rows with count 0
    on either side"""
    mask = rng.random((n_cells, n_features)) < density
    cell, feature = np.nonzero(mask)
    count = rng.integers(1, 60, size=len(cell))
    count[rng.random(len(cell)) < zero_rate] = 0
    if big:
        count[0] = 4_000_000_000                            # a product beyond 2^63 (the sum of all counts stays below 2^32)
    sel = rng.random(len(cell)) < keep
    y = np.minimum(count[sel], rng.integers(0, 60, size=int(sel.sum())))
    if big and sel[0]:
        y[0] = 4_000_000_000
    full = (feature + 1, cell + 1, count)
    point = (feature[sel] + 1, cell[sel] + 1, y)
    return full, point


@pytest.mark.parametrize("shape", [(1, 1, 1.0, 1.0), (1, 40, 0.5, 0.5), (7, 1, 0.6, 0.7), (50, 30, 0.3, 0.5), (300, 200, 0.05, 0.2), (40, 25, 0.4, 0.0),
                                   (40, 25, 0.4, 1.0)])
def test_the_host_twin_against_the_reference(shape):
    n_cells, n_features, density, keep = shape
    rng = np.random.default_rng(n_cells * 1000 + n_features)
    full, point = nested_pair(rng, n_cells, n_features, density, keep, big=n_cells == 50)
    mom = R.moments(full, point, n_cells)
    sxy, syy = sweep.fidelity_from_coo(full, point, n_cells)
    assert [int(v) for v in sxy] == mom["sum_xy"] and [int(v) for v in syy] == mom["sum_yy"]
    sxx, sxx2 = sweep.fidelity_from_coo(full, full, n_cells)
    assert [int(v) for v in sxx] == mom["sum_xx"] and (sxx == sxx2).all()
    if n_cells == 50:
        assert max(mom["sum_xx"]) > 2 ** 63
    # the other five are the per-cell summary's
    u, g, _ = sweep.cells_from_coo(point[1], point[2], n_cells)
    uf, gf, _ = sweep.cells_from_coo(full[1], full[2], n_cells)
    assert [int(v) for v in u] == mom["umis"] and [int(v) for v in g] == mom["genes"]
    assert [int(v) for v in uf] == mom["umis_full"] and [int(v) for v in gf] == mom["genes_full"]


def test_a_missing_partner_is_an_error():
    full = (np.array([1, 3, 5, 2]), np.array([1, 1, 1, 2]), np.array([4, 5, 6, 7]))
    ok = (np.array([3, 2]), np.array([1, 2]), np.array([1, 1]))
    sweep.fidelity_from_coo(full, ok, 2)
    for bad in [(np.array([2]), np.array([1]), np.array([1])),            # between two full rows
                (np.array([1]), np.array([3]), np.array([1])),            # behind the last full row
                (np.array([3, 4]), np.array([1, 2]), np.array([1, 1])),   # the second row
                (np.array([1]), np.array([0]), np.array([1]))]:           # before the first
        with pytest.raises(F.FastfError, match="no partner"):
            sweep.fidelity_from_coo(full, bad, 2)
    with pytest.raises(F.FastfError, match="no partner"):
        sweep.fidelity_from_coo((np.zeros(0), np.zeros(0), np.zeros(0)), ok, 2)
    sxy, syy = sweep.fidelity_from_coo(full, (np.zeros(0), np.zeros(0), np.zeros(0)), 2)
    assert not sxy.any() and not syy.any()


def test_headers_and_the_mirrors_column_tuples():
    assert sweep.fidelity_header() == "\t".join(sweep.POINT_FIDELITY_COLUMNS) + "\n"
    assert sweep.POINT_FIDELITY_COLUMNS == ("barcode",) + R.INT_COLUMNS + ("pearson", "cosine")
    assert sweep.fidelity_header("sweep") == "\t".join(sweep.FIDELITY_COLUMNS) + "\n"
    assert cap.fidelity_header() == "\t".join(cap.FIDELITY_COLUMNS) + "\n" and level.fidelity_header() == "\t".join(level.FIDELITY_COLUMNS) + "\n"
    tail = ("seed", "n_cells", "cells_defined", "median_pearson", "p10_pearson", "mean_pearson", "median_cosine", "umis_kept", "genes_kept")
    assert sweep.FIDELITY_COLUMNS == ("rate_cell", "rate_depth") + tail and cap.FIDELITY_COLUMNS == ("rate_cell", "reads_per_cell") + tail
    assert level.FIDELITY_COLUMNS == ("rate_cell", "umi_cap") + tail
    assert (sweep.FIDELITY, cap.FIDELITY, level.FIDELITY) == (32, 32, 32)
    for sym in ("fastf_dev_fidelity", "fastf_fidelity_from_coo", "fastf_fidelity_row", "fastf_fidelity_header"):
        assert sym in _lib.ABI_SYMBOLS
    assert "fidelity_kernel" in _lib.lib().fastf_kernel_names().decode().split(",")
    assert hasattr(F.Engine, "dev_fidelity")


def _row(ints, G, name="AAAC-1"):
    return sweep.fidelity_row(name, *ints, G).rstrip("\n").split("\t")


def test_rows_and_the_na_rules():
    rng = np.random.default_rng(3)
    G = 40
    full, point = nested_pair(rng, 30, G, 0.5, 0.6)
    mom = R.moments(full, point, 30)
    want = R.cell_rows(["bc%d" % k for k in range(30)], mom, G)
    for k in range(30):
        line = sweep.fidelity_row("bc%d" % k, *[mom[c][k] for c in R.INT_COLUMNS], G)
        assert line.endswith("\n")
        R.assert_fields(line[:-1].split("\t"), want[k], 8, k)
    # a cell with no rows at all
    assert _row((0, 0, 0, 0, 0, 0, 0), 40) == ["AAAC-1", "0", "0", "0", "0", "0", "0", "0", "NA", "NA"]
    # a cell whose point rows all count 0: y constant zero
    assert _row((10, 0, 3, 0, 38, 0, 0), 40)[8:] == ["NA", "NA"]
    # x constant over all G genes (every gene 2): no variance, yet a cosine
    got = _row((80, 40, 40, 40, 160, 40, 80), 40)
    assert got[8] == "NA" and got[9] == "1.000000"
    # G = 1: one gene has no variance on either side
    got = _row((7, 3, 1, 1, 49, 9, 21), 1)
    assert got[8] == "NA" and got[9] == "1.000000"
    # point == full: both 1
    assert _row((6, 6, 2, 2, 20, 20, 20), 40)[8:] == ["1.000000", "1.000000"]
    # a negative pearson: G = 2, x = (5, 1), y = (0, 1)
    p, c = R.metrics(6, 1, 26, 1, 1, 2)
    assert p == -1.0 and _row((6, 1, 2, 1, 26, 1, 1), 2)[8] == "-1.000000"
    # sums beyond 2^63 stay exact
    big = (4_000_000_001, 4_000_000_000, 2, 1, 16 * 10 ** 18 + 1, 16 * 10 ** 18, 16 * 10 ** 18)      # x = (4e9, 1, 0), y = (4e9, -, -)
    R.assert_fields(_row(big, 3), R.cell_rows(["AAAC-1"], {c: [v] for c, v in zip(R.INT_COLUMNS, big)}, 3)[0], 8)


@pytest.mark.parametrize("n_defined", [0, 1, 2, 5])
def test_the_median_and_p10_rule(n_defined):
    rng = np.random.default_rng(50 + n_defined)
    G, n_cells = 12, n_defined + 3
    full, point = nested_pair(rng, n_cells, G, 0.9, 0.7, zero_rate=0.0)
    mom = R.moments(full, point, n_cells)
    for k in range(n_defined, n_cells):                    # the last three cells: undefined (y constant zero; x constant zero; no rows)
        for c in R.INT_COLUMNS:
            mom[c][k] = 0
    if n_cells > n_defined:
        mom["umis_full"][n_defined], mom["genes_full"][n_defined], mom["sum_xx"][n_defined] = 9, 2, 41
    want = R.summary_fields(["0.500", "0.100"], 926, mom, G)
    arr = {c: np.array(mom[c], dtype=np.uint64) for c in R.INT_COLUMNS}
    args = (arr["umis_full"], arr["umis"], arr["genes_full"], arr["genes"], arr["sum_xx"], arr["sum_yy"], arr["sum_xy"], G)
    got = sweep.fidelity_summary_row(0.5, 0.1, 926, *args)
    assert got.endswith("\n")
    R.assert_fields(got[:-1].split("\t"), want, 5, n_defined)
    assert want[4] == str(n_defined) and want[3] == str(n_cells)
    if n_defined == 0:
        assert want[5:9] == ["NA"] * 4 and want[9] != "NA"
    else:
        assert "NA" not in want
        pe = sorted(p for p in (R.metrics(mom["umis_full"][k], mom["umis"][k], mom["sum_xx"][k], mom["sum_yy"][k], mom["sum_xy"][k], G)[0] for k in range(n_defined)))
        assert want[6] == "%.6f" % pe[0]                  # floor(0.1 * (n - 1)) == 0 up to 10 cells
        assert want[5] == "%.6f" % (pe[0] if n_defined == 1 else (pe[0] + pe[1]) / 2 if n_defined == 2 else pe[2])
    # the second column of cap and level; a point with nothing at all
    assert cap.fidelity_summary_row(0.5, 40, 926, *args).split("\t")[:3] == ["0.500", "40", "926"]
    assert level.fidelity_summary_row(1, 7, 5, *args).split("\t")[:3] == ["1.000", "7", "5"]
    z = np.zeros(0, np.uint64)
    assert sweep.fidelity_summary_row(1, 1, 1, z, z, z, z, z, z, z, G) == "1.000\t1.000\t1\t0\t0\tNA\tNA\tNA\tNA\tNA\tNA\n"


def test_p10_beyond_ten_cells():
    G = 5
    cells = 25
    rng = np.random.default_rng(9)
    full, point = nested_pair(rng, cells, G, 1.0, 0.8, zero_rate=0.0)
    mom = R.moments(full, point, cells)
    want = R.summary_fields(["1.000", "3"], 1, mom, G)
    arr = {c: np.array(mom[c], dtype=np.uint64) for c in R.INT_COLUMNS}
    got = cap.fidelity_summary_row(1, 3, 1, arr["umis_full"], arr["umis"], arr["genes_full"], arr["genes"], arr["sum_xx"], arr["sum_yy"], arr["sum_xy"], G)
    R.assert_fields(got[:-1].split("\t"), want, 5)
    assert int(want[4]) > 11


def test_the_flag_bits_and_the_refusals(tmp_path):
    one, p_one = sweep._floats([1])
    caps = np.array([5], np.uint64)
    L = _lib.lib()
    # bits 4 and 16 are still nobody's (two existing tests pin them as the unknown bits), alone and beside the new bit; bit 64 is unknown
    for flags in (4, 16, 4 | 32, 16 | 32, 64, 32 | 64):
        for call in (lambda fl: L.fastf_sweep(b"x", b"y", b"b", b"f", p_one, 1, p_one, 1, 926, fl),
                     lambda fl: L.fastf_cap(b"x", b"y", b"b", b"f", p_one, 1, caps.ctypes.data, 1, 926, fl),
                     lambda fl: L.fastf_level(b"x", b"y", b"b", b"f", p_one, 1, caps.ctypes.data, 1, 926, fl)):
            with pytest.raises(F.FastfError, match="unknown flags"):
                _lib.check(call(flags))
    # bit 32 is known: the call gets as far as the missing file
    for call in (lambda: L.fastf_sweep(b"x", b"y", b"b", b"f", p_one, 1, p_one, 1, 926, 32),
                 lambda: L.fastf_cap(b"x", b"y", b"b", b"f", p_one, 1, caps.ctypes.data, 1, 926, 32 | 8 | 2 | 1),
                 lambda: L.fastf_level(b"x", b"y", b"b", b"f", p_one, 1, caps.ctypes.data, 1, 926, 32)):
        with pytest.raises(F.FastfError, match="does not exist"):
            _lib.check(call())
    bt, ft, bar, genes = synth.make_lists(5, 3)
    fl, xf, cb, gx, ub = synth.make_records(20, bar, genes)
    bam, b, f = tmp_path / "x.bam", tmp_path / "b.tsv", tmp_path / "f.tsv"
    synth.write_bam(str(bam), fl, xf, cb, gx, ub)
    b.write_bytes(bt); f.write_bytes(ft)
    several = dict(os.environ, FASTF_DEVICES="0,1")
    for k, (verb, extra) in enumerate([("sweep", ["-r", "0.5"]), ("cap", ["-n", "5"]), ("level", ["-m", "5"])]):
        out = tmp_path / ("out%d" % k)
        r = subprocess.run([_lib.cli_path(), verb, "--fidelity", "-o", str(out), "-a", str(b), "-f", str(f), "-b", str(bam)] + extra,
                           capture_output=True, text=True, timeout=60, env=several)
        assert r.returncode == 1 and "several devices" in r.stderr, r.stderr
        assert not out.exists()                             # refused before the output directory is made
        r = subprocess.run([_lib.cli_path(), verb, "--help"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and "--fidelity" in r.stdout and "RAW counts" in r.stdout and "ALL genes" in r.stdout
        r = subprocess.run([_lib.cli_path(), verb, "-F", "-o", str(out)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "unknown option" in r.stderr
    os.environ["FASTF_DEVICES"] = "0,1"
    try:
        with pytest.raises(F.FastfError, match="--fidelity needs the resident form"):
            sweep.sweep(bam, tmp_path / "o", b, f, [1], [1], fidelity=True)
        with pytest.raises(F.FastfError, match="several devices"):
            cap.cap_reps(bam, tmp_path / "o", b, f, [1], [5], [1, 2], fidelity=True)
        with pytest.raises(F.FastfError, match="several devices"):
            level.level(bam, tmp_path / "o", b, f, [1], [5], fidelity=True)
    finally:
        del os.environ["FASTF_DEVICES"]
    assert not (tmp_path / "o").exists()
