"""`--cells` of sweep and cap, the parts that need no device: the host twin of the copy summary against numpy, the row and header
text, the help texts, the refusals, and the census of the fixtures tests/test_gpu_cells.py runs on the device."""
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, cap, sweep
import cells_ref as R
import sortreduce_ref as S


def _twin(name):
    keys, k, n_cells = R.fixture(name)
    lay = R.layout_of(name)
    cell = (keys >> np.uint64(lay.cs)).astype(np.uint32)
    nn = ((keys >> np.uint64(lay.fs - 1)) & np.uint64(1)).astype(np.uint8)
    return sweep.copies_from_umi_rows(cell, k, nn, n_cells), R.from_keys(keys, k, n_cells, lay)


@pytest.mark.parametrize("name", R.fixture_names())
def test_host_twin_against_numpy(name):
    (r, nr, sg, h), (wr, wn, ws, wh) = _twin(name)
    assert r.dtype == np.uint32 and nr.dtype == np.uint32 and sg.dtype == np.uint32 and h.dtype == np.uint64 and len(h) == R.BINS + 1
    np.testing.assert_array_equal(r.astype(np.int64), wr)
    np.testing.assert_array_equal(nr.astype(np.int64), wn)
    np.testing.assert_array_equal(sg.astype(np.int64), ws)
    assert [int(x) for x in h] == wh


def test_host_twin_rules():
    # cell 0 and cell 4 of 3 add nothing per cell but are counted; n_copy 0 is in no bin; NULL rows are in no bin
    r, nr, sg, h = sweep.copies_from_umi_rows([0, 1, 1, 1, 3, 4], [7, 3, 1, 0, 32, 31], [1, 0, 1, 1, 1, 1], 3)
    assert r.tolist() == [4, 0, 32] and nr.tolist() == [3, 0, 0] and sg.tolist() == [1, 0, 0]
    assert int(h[0]) == 1 and int(h[6]) == 1 and int(h[30]) == 1 and int(h[31]) == 1 and int(h[32]) == 32 and int(h.sum()) == 36
    assert cap.copies_from_umi_rows is sweep.copies_from_umi_rows
    r0 = sweep.copies_from_umi_rows([1, 2], [1, 1], [1, 1], 0)
    assert len(r0[0]) == 0 and int(r0[3][0]) == 2
    rows = _lib.UmiRows()
    with pytest.raises(F.FastfError, match="null argument"):
        _lib.check(_lib.lib().fastf_copies_from_umi_rows(None, 1, 0, 0, 0, 0))
    with pytest.raises(F.FastfError, match="null argument"):
        _lib.check(_lib.lib().fastf_copies_from_umi_rows(rows, 1, 0, 0, 0, 0))


def test_header_and_row_text():
    assert sweep.cells_header() == "\t".join(sweep.CELLS_COLUMNS) + "\n"
    assert cap.cells_header() == "\t".join(cap.CELLS_COLUMNS) + "\n"
    want = (["rate_cell", "rate_depth", "seed", "valid_reads", "null_umi_reads", "umis", "singleton_umis", "median_reads_per_cell"] +
            ["copies_%d" % k for k in range(1, 32)] + ["copies_32_plus", "reads_copies_32_plus"])
    assert list(sweep.CELLS_COLUMNS) == want and len(want) == 41
    assert cap.CELLS_COLUMNS == tuple("reads_per_cell" if c == "rate_depth" else c for c in sweep.CELLS_COLUMNS)
    assert sweep.POINT_CELLS_COLUMNS == ("barcode", "reads", "null_umi_reads", "umis", "genes", "singleton_umis", "saturation")
    reads = np.array([10, 0, 4, 2 ** 32 - 1], np.uint32)
    nulls = np.array([1, 0, 0, 5], np.uint32)
    single = np.array([2, 0, 1, 0], np.uint32)
    hist = np.arange(100, 133, dtype=np.uint64); hist[32] = 2 ** 40 + 3
    row = sweep.cells_summary_row(0.25, 0.5, 926, reads, nulls, single, hist)
    f = row.rstrip("\n").split("\t")
    assert row.endswith("\n") and len(f) == 41
    assert f[:8] == ["0.250", "0.500", "926", str(10 + 4 + 2 ** 32 - 1), "6", str(sum(range(100, 132))), "3", "7.0"]      # median of 0, 4, 10, 2^32 - 1
    assert f[8:] == [str(x) for x in range(100, 132)] + [str(2 ** 40 + 3)]
    crow = cap.cells_summary_row(1, 40, 1, reads, nulls, single, hist).rstrip("\n").split("\t")
    assert crow[:3] == ["1.000", "40", "1"] and crow[3:] == f[3:]
    empty = sweep.cells_summary_row(1, 0, 1, np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(33, np.uint64))
    assert empty == "1.000\t0.000\t1\t0\t0\t0\t0\t0.0" + "\t0" * 33 + "\n"
    rng = np.random.default_rng(5)
    reads = rng.integers(0, 5000, size=4001); nulls = rng.integers(0, 3, size=4001); single = rng.integers(0, 9, size=4001)
    h = [int(x) for x in rng.integers(0, 10 ** 6, size=33)]
    assert sweep.cells_summary_row(0.3, 1, 7, reads, nulls, single, h).rstrip("\n").split("\t") == R.table_row(["0.300", "1.000"], 7, reads, nulls, single, h)


def test_saturation_column_of_the_reference_lines():
    """the %.6f column as tests/cells_ref.py restates it, reads == 0 included (the device file is compared against these lines)"""
    matrix = b'%%MatrixMarket matrix coordinate integer general\n%\t"total_n_FastQ": 9,\n%\t"sampled_n_FastQ": 9,\n%\t"sampled_valid_n_FastQ": 8,\n3 3 2\n1 1 2\n2 3 1\n'
    lines = R.point_lines(b"A-1\nC-1\nG-1\n", matrix, np.array([3, 0, 1]), np.array([1, 0, 0]), np.array([1, 0, 1]))
    assert lines == ["barcode\treads\tnull_umi_reads\tumis\tgenes\tsingleton_umis\tsaturation", "A-1\t3\t1\t2\t1\t1\t0.333333",
                     "C-1\t0\t0\t0\t0\t0\t0.000000", "G-1\t1\t0\t1\t1\t1\t0.000000"]


def test_abi_pieces_are_there():
    assert sweep.CELLS == 8 and cap.CELLS == 8 and sweep.COPY_BINS == 32
    for name in ("fastf_dev_copy_summary", "fastf_copies_from_umi_rows", "fastf_cells_summary_row", "fastf_sweep_cells_header", "fastf_cap_cells_header"):
        assert name in _lib.ABI_SYMBOLS
    assert "copy_summary_kernel" in _lib.lib().fastf_kernel_names().decode().split(",")
    assert hasattr(F.Engine, "dev_copy_summary")


def test_help_texts_and_refusals_leave_no_cells_file(tmp_path):
    for verb in ("sweep", "cap"):
        r = subprocess.run([_lib.cli_path(), verb, "--help"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and "--cells" in r.stdout and "%s_cells.tsv" % verb in r.stdout and "cells.tsv.gz" in r.stdout
    b, f = tmp_path / "b.tsv", tmp_path / "f.tsv"
    b.write_text("AAAA-1\n"); f.write_text("ENSG00000000001\tG\tGene Expression\n")
    base = ["-a", str(b), "-f", str(f), "-b", str(tmp_path / "missing.bam"), "--cells"]
    jobs = [("sweep", ["-r", "0.5"], "does not exist"), ("sweep", ["-c", "0.5,0.5001"], "both print as"), ("sweep", ["-u"], "umi.tsv.gz"),
            ("cap", ["-n", "5"], "does not exist"), ("cap", ["-n", "0"], "at least 1"), ("cap", [], "needs -n"), ("cap", ["-n", "5", "-u"], "umi.tsv.gz"),
            ("cap", ["-n", "5", "--cellz"], "unknown option"), ("sweep", ["-C"], "unknown option")]
    for k, (verb, args, word) in enumerate(jobs):
        out = tmp_path / ("out%d" % k)
        r = subprocess.run([_lib.cli_path(), verb, "-o", str(out)] + base + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and word in r.stderr, (verb, args, r.stderr)
        for name in ("%s_cells.tsv", "%s_cells.tsv.partial", "%s.tsv", "%s.tsv.partial"):
            assert not (out / (name % verb)).exists(), (verb, args, name)
    with pytest.raises(F.FastfError):
        sweep.sweep(tmp_path / "missing.bam", tmp_path / "o", b, f, [1], [1], cells=True)
    with pytest.raises(F.FastfError):
        cap.cap(tmp_path / "missing.bam", tmp_path / "o", b, f, [1], [5], cells=True)
    assert not (tmp_path / "o" / "sweep_cells.tsv").exists() and not (tmp_path / "o" / "cap_cells.tsv").exists()
    one, p_one = sweep._floats([1])
    caps = np.array([5], np.uint64)
    for flags in (8, 11):                                    # the flag is known, alone and beside the others: the call gets as far as the bam file
        with pytest.raises(F.FastfError, match="does not exist"):
            _lib.check(_lib.lib().fastf_sweep(b"x", b"y", b"b", b"f", p_one, 1, p_one, 1, 926, flags))
        with pytest.raises(F.FastfError, match="does not exist"):
            _lib.check(_lib.lib().fastf_cap(b"x", b"y", b"b", b"f", p_one, 1, caps.ctypes.data, 1, 926, flags))
    with pytest.raises(F.FastfError, match="unknown flags"):
        _lib.check(_lib.lib().fastf_sweep(b"x", b"y", b"b", b"f", p_one, 1, p_one, 1, 926, 16))
    with pytest.raises(F.FastfError, match="unknown flags"):
        _lib.check(_lib.lib().fastf_cap(b"x", b"y", b"b", b"f", p_one, 1, caps.ctypes.data, 1, 926, 16))


def test_several_devices_are_refused_with_cells_before_anything_is_written(tmp_path, monkeypatch):
    """sweep without --cells would run such a job point by point; with it the job is refused before the output directory exists"""
    b, f, bam = tmp_path / "b.tsv", tmp_path / "f.tsv", tmp_path / "in.bam"
    b.write_text("AAAA-1\n"); f.write_text("ENSG00000000001\tG\tGene Expression\n"); bam.write_bytes(b"")
    out = tmp_path / "o"
    monkeypatch.setenv("FASTF_DEVICES", "0,0")
    with pytest.raises(F.FastfError, match="several devices"):
        sweep.sweep(bam, out, b, f, [1], [1], cells=True)
    assert not out.exists()
    with pytest.raises(F.FastfError, match="several devices"):
        cap.cap(bam, out, b, f, [1], [5], cells=True)
    assert not out.exists()


# ---- the census: what the GPU tests feed the kernel, asserted here so that a GPU test cannot pass by missing its own edge ----
def test_census_of_the_gpu_fixtures():
    w = R.launch_waves()
    assert w == 2048 and R.row_counts() == [0, 1, 63, 64, 65, w * 64 - 1, w * 64 + 1]
    names = R.fixture_names()
    assert {"rows_%d_1000" % n for n in R.row_counts()} <= set(names) and {"rows_5001_%d" % c for c in (1, 3, 1000, 70_000)} <= set(names)
    for name in names:
        keys, k, n_cells = R.fixture(name)
        keys2, k2, _ = R.fixture(name)
        lay = R.layout_of(name)
        assert keys.dtype == np.uint64 and k.dtype == np.uint32 and len(keys) == len(k)
        assert (keys == keys2).all() and (k == k2).all()     # deterministic: both test files see the same rows
        assert (np.diff(keys.astype(np.int64)) > 0).all() if len(keys) > 1 else True      # what K3u leaves: distinct, ascending
        cell = (keys >> np.uint64(lay.cs)).astype(np.int64)
        nn = ((keys >> np.uint64(lay.fs - 1)) & np.uint64(1)).astype(bool)
        reads, nulls, single, hist = R.from_keys(keys, k, n_cells, lay)
        assert reads.max(initial=0) < 2 ** 32                # the ABI's precondition
        # the histogram accounts for every read of the non-NULL rows
        assert sum(b * hist[b - 1] for b in range(1, R.BINS)) + hist[R.BINS] == int(k[nn].astype(np.int64).sum())
        if name.startswith("rows_"):
            n, nc = int(name.split("_")[1]), int(name.split("_")[2])
            assert len(keys) == n and n_cells == nc and (n == 0 or (cell.min() >= 1 and cell.max() <= nc))
            if n >= 5001:
                first = np.r_[True, np.diff(cell) != 0]
                assert (~nn & first).any() and not (~nn & ~first).any() and hist[R.BINS - 1] > 0 and nulls.sum() > 0      # NULL rows at the head of a group; a tail
            if nc == 70_000:
                assert cell.max() > 65_535 and lay is R.BIG and (reads == 0).sum() > 60_000
        elif name == "one_cell":
            assert len(keys) == w * 64 + 1 and set(cell.tolist()) == {2} and n_cells == 3 and not nn[0] and nn[1:].all()
        elif name == "one_row_each":
            assert cell.tolist() == list(range(1, 1001)) and n_cells == 1000 and (~nn).any() and nn.any()
        elif name == "gaps":
            assert n_cells == 1000 and set(cell.tolist()) == {3, 4, 5, 400, 998}       # nothing at the front, in the middle, at n_cells
            assert reads[:2].sum() == 0 and reads[5:399].sum() == 0 and reads[998:].sum() == 0 and reads[997] > 0
        elif name == "lane63":
            assert len(keys) == w * 128                       # two turns a wave: a carry inside every span
            starts = np.flatnonzero(np.r_[True, np.diff(cell) != 0]); ends = np.r_[starts[1:], len(cell)] - 1
            inside = [(s, e) for s, e in zip(starts, ends) if s % 64 == 63 and e == s + 1 and s % 128 == 63]
            across = [(s, e) for s, e in zip(starts, ends) if s % 128 == 127 and e == s + 1]
            assert len(inside) >= 3 and len(across) >= 2
        elif name == "copies":
            assert {1, 31, 32, 33, 1 << 31} <= set(int(x) for x in k) and hist[R.BINS] > 2 ** 32 and hist[0] == 1 and hist[30] == 1 and hist[31] == 6
        elif name == "hot_bin":
            assert len(keys) == 100_001 and hist[0] == 100_001 and sum(hist[1:]) == 0
        elif name == "out_of_range":
            assert n_cells == 3 and {0, 1, 3, 4, 1023} == set(cell.tolist())
            assert int(k.sum()) > int(reads.sum()) > 0 and sum(hist[:R.BINS]) == int(nn.sum())      # counted in the histogram, not per cell
    # the source of NULL rows at the head of a group through K3u, and the chained fixture
    nk = S.null_run_keys()
    uk, uc = S.umi_rows_ref(nk)
    nn = ((uk >> np.uint64(R.NN_BIT)) & np.uint64(1)).astype(bool)
    first = np.r_[True, np.diff((uk >> np.uint64(S.FS)).astype(np.int64)) != 0]
    assert (~nn).sum() == 5 and (~nn == first).all() and {1, 3, 2048, 2500, 2} == set(int(x) for x in uc[~nn]) and 2047 in uc[nn]
    lk = S.layout_keys(np.random.default_rng(11), 50_000)
    uk, uc = S.umi_rows_ref(np.sort(lk))
    assert len(uk) > 40_000 and uc.max() >= 2 and (((uk >> np.uint64(R.NN_BIT)) & np.uint64(1)) == 0).any()
