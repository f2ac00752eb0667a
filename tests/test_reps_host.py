"""Host pieces of the replicate runs of `fastF sweep` and `fastF cap` (no GPU): the seed lists of --seeds and --reps, the option
conflicts (refused before any file is touched), the help texts, the rows of <verb>_reps.tsv and <verb>_genes_reps.tsv and the
per-gene accumulators against tests/reps_ref.py, the row order and the directory names."""
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, cap, sweep
import reps_ref


def test_seed_lists_parse_like_the_single_value_of_s():
    np.testing.assert_array_equal(sweep.parse_seeds("926,927,5"), np.array([926, 927, 5], np.uint32))
    np.testing.assert_array_equal(sweep.parse_seeds("0"), np.array([0], np.uint32))
    np.testing.assert_array_equal(sweep.parse_seeds("4294967295,0"), np.array([4294967295, 0], np.uint32))
    np.testing.assert_array_equal(sweep.parse_seeds("0x10,010,10"), np.array([16, 8, 10], np.uint32))       # strtol(.., 0)
    np.testing.assert_array_equal(sweep.parse_seeds(",".join(str(k) for k in range(64))), np.arange(64, dtype=np.uint32))
    assert cap.parse_seeds is sweep.parse_seeds


@pytest.mark.parametrize("text,word", [
    ("", "empty"), ("1,,2", "empty"), ("1,", "empty"), (",1", "empty"),
    ("1x", "integer"), ("1 ", "integer"), ("abc", "integer"), ("1.5", "integer"), ("1;2", "integer"),
    ("7,7", "twice"), ("16,0x10", "twice"), ("1,2,3,1", "twice"),
    (",".join(str(k) for k in range(65)), "more than 64"),
    ("99999999999999999999", "out of range"),
])
def test_seed_lists_that_are_refused(text, word):
    with pytest.raises(F.FastfError) as ei:
        sweep.parse_seeds(text)
    assert word in str(ei.value) and "--seeds" in str(ei.value)


def test_reps_count_up_from_the_seed_and_do_not_wrap():
    np.testing.assert_array_equal(sweep.reps_seeds(926, 3), np.array([926, 927, 928], np.uint32))
    np.testing.assert_array_equal(sweep.reps_seeds(926, 1), np.array([926], np.uint32))
    np.testing.assert_array_equal(sweep.reps_seeds(4294967295, 1), np.array([4294967295], np.uint32))
    np.testing.assert_array_equal(sweep.reps_seeds(4294967295 - 63, 64), np.arange(4294967295 - 63, 4294967296, dtype=np.uint64).astype(np.uint32))
    for first, n, word in ((4294967295, 2, "wrap"), (4294967295 - 62, 64, "wrap"), (926, 0, "--reps"), (926, 65, "--reps")):
        with pytest.raises(F.FastfError) as ei:
            sweep.reps_seeds(first, n)
        assert word in str(ei.value)


@pytest.mark.parametrize("verb,own", [("sweep", ["-r", "0.5"]), ("cap", ["-n", "5"])])
def test_cli_refuses_conflicts_before_anything_is_read(tmp_path, verb, own):
    """the inputs do not exist: every refusal below comes from the options alone, exit 1, the message names the option, nothing is written"""
    cli = _lib.cli_path()
    out = tmp_path / "out"
    base = [cli, verb, "-b", str(tmp_path / "missing.bam"), "-a", str(tmp_path / "b.tsv"), "-f", str(tmp_path / "f.tsv"), "-o", str(out)] + own
    for extra, words in ((["--seeds", "1,2", "--reps", "2"], ("--seeds", "--reps")), (["--reps=2", "--seeds=1,2"], ("--seeds", "--reps")),
                         (["--seeds", "1,2", "-s", "3"], ("--seeds", "-s")), (["-s3", "--seeds=1"], ("--seeds", "-s")),
                         (["--seeds", "1,,2"], ("--seeds", "empty")), (["--seeds", "1,2x"], ("--seeds", "integer")),
                         (["--seeds=4,4"], ("--seeds", "twice")), (["--seeds", ",".join(str(k) for k in range(65))], ("--seeds", "more than 64")),
                         (["--reps", "0"], ("--reps",)), (["--reps", "65"], ("--reps",)), (["--reps", "2x"], ("--reps",)),
                         (["-s", "4294967295", "--reps", "2"], ("--reps", "wrap")), (["--seeds"], ("--seeds", "requires a value")),
                         (["-s", "1,2"], ("-s", "expects an integer value"))):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode == 1, (extra, r.stderr)
        for w in words:
            assert w in r.stderr, (extra, r.stderr)
        assert not out.exists()
    # accepted forms reach the input check
    for extra in (["--seeds", "1,2"], ["--reps", "3"], ["-s", "7", "--reps=2"], ["--seeds=0x10"]):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "does not exist" in r.stderr, (extra, r.stderr)
        assert not out.exists()


@pytest.mark.parametrize("verb", ["sweep", "cap"])
def test_help_names_the_options(verb):
    r = subprocess.run([_lib.cli_path(), verb, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "--seeds" in r.stdout and "--reps" in r.stdout and "%s_reps.tsv" % verb in r.stdout


def test_in_process_calls_refuse_bad_seed_lists(tmp_path):
    for seeds in ([], [1, 1], list(range(65))):
        with pytest.raises(F.FastfError):
            sweep.sweep_reps(tmp_path / "x.bam", tmp_path / "o", tmp_path / "b", tmp_path / "f", [1], [1], seeds)
        with pytest.raises(F.FastfError):
            cap.cap_reps(tmp_path / "x.bam", tmp_path / "o", tmp_path / "b", tmp_path / "f", [1], [5], seeds)
    assert not (tmp_path / "o").exists()


def test_headers_and_names():
    assert sweep.reps_header().rstrip("\n").split("\t") == list(sweep.REPS_COLUMNS)
    assert cap.reps_header().rstrip("\n").split("\t") == list(cap.REPS_COLUMNS)
    assert sweep.REPS_COLUMNS[:4] == ("rate_cell", "rate_depth", "n_reps", "n_cells") and cap.REPS_COLUMNS[1] == "reads_per_cell"
    assert sweep.REPS_COLUMNS[4:8] == ("sampled_reads_mean", "sampled_reads_sd", "sampled_reads_min", "sampled_reads_max")
    assert [c[:-5] for c in sweep.REPS_COLUMNS[4::4]] == list(reps_ref.METRICS)
    assert sweep.genes_reps_header().rstrip("\n").split("\t") == list(sweep.GENES_REPS_COLUMNS)
    assert cap.genes_reps_header().rstrip("\n").split("\t") == list(cap.GENES_REPS_COLUMNS)
    assert sweep.GENES_REPS_COLUMNS[2:] == ("n_reps", "genes_detected_mean", "genes_detected_sd", "genes_detected_min", "genes_detected_max",
                                            "genes_in_all_reps", "genes_in_any_rep")
    assert sweep.reps_point_dir(sweep.point_dir(0.5, 0.1), 927) == "c0.500_r0.100_s927" == reps_ref.point_name(0.5, 0.1, 927)
    assert sweep.reps_point_dir(cap.point_dir(1, 40), 4294967295) == "c1.000_n40_s4294967295" == reps_ref.point_name(1, 40, 4294967295, caps=True)
    assert sweep.reps_point_dir(sweep.point_dir(1, 0), 0) == "c1.000_r0.000_s0"
    for name in ("fastf_sweep_reps", "fastf_cap_reps", "fastf_parse_seeds", "fastf_dev_gene_reps_add"):
        assert name in _lib.ABI_SYMBOLS
    assert "gene_reps_kernel" in _lib.lib().fastf_kernel_names().decode().split(",")


def test_row_order_is_cell_rates_then_seeds_then_the_list():
    got = reps_ref.order([0.5, 1], [926, 5], [0, 0.1, 1])
    assert got[:4] == [(0.5, 926, 0), (0.5, 926, 0.1), (0.5, 926, 1), (0.5, 5, 0)] and got[6] == (1, 926, 0) and len(got) == 12
    assert [reps_ref.point_name(rc, rd, s) for rc, s, rd in got[2:4]] == ["c0.500_r1.000_s926", "c0.500_r0.000_s5"]


def _table_rows(rng, n_reps, n_cells):
    """n_reps rows of sweep.tsv (text fields) of one grid point, made through the library's own row function"""
    rows = []
    for k in range(n_reps):
        nnz = int(rng.integers(0, 4 * n_cells + 1))
        cell = np.sort(rng.integers(1, n_cells + 1, size=nnz))
        count = rng.integers(0, 4, size=nnz)
        upc, gpc, umis = sweep.cells_from_coo(cell, count, n_cells)
        valid = umis + int(rng.integers(0, 50))
        counters = [10 * valid + 7, valid + int(rng.integers(0, 90)), valid]
        rows.append(sweep.summary_row(0.3, 0.1, 926 + k, counters, nnz, umis, upc, gpc).rstrip("\n").split("\t"))
    return rows


@pytest.mark.parametrize("n_reps", [1, 2, 3, 5, 64])
def test_reps_row_against_the_reference(n_reps):
    rng = np.random.default_rng(n_reps)
    for n_cells in (1, 2, 7, 300):
        rows = _table_rows(rng, n_reps, n_cells)
        metrics = [reps_ref.metrics_of(r) for r in rows]
        got = sweep.reps_summary_row(0.3, 0.1, n_cells, metrics)
        assert got.endswith("\n")
        got = got[:-1].split("\t")
        want = reps_ref.reps_row(["0.300", "0.100"], rows)
        assert len(got) == len(sweep.REPS_COLUMNS)
        reps_ref.assert_reps_row(got, want, (n_reps, n_cells))
        sds = got[5::4]
        assert (sds == ["NA"] * 7) == (n_reps == 1) and ("NA" in sds) == (n_reps == 1)
        capped = cap.reps_summary_row(0.3, 40, n_cells, metrics)[:-1].split("\t")
        assert capped[:2] == ["0.300", "40"] and capped[2:] == got[2:]


def test_reps_row_by_hand():
    """two replicates: mean 11, sample sd sqrt(2); the saturation min and max print six decimals, the medians one"""
    m = [[10, 9, 5, 7, 0.25, 3.0, 2.5], [12, 9, 6, 8, 0.5, 4.0, 2.5]]
    assert sweep.reps_summary_row(0.5, 0.1, 300, m) == "\t".join(
        ["0.500", "0.100", "2", "300", "11.000000", "1.414214", "10", "12", "9.000000", "0.000000", "9", "9", "5.500000", "0.707107", "5", "6",
         "7.500000", "0.707107", "7", "8", "0.375000", "0.176777", "0.250000", "0.500000", "3.500000", "0.707107", "3.0", "4.0",
         "2.500000", "0.000000", "2.5", "2.5"]) + "\n"
    with pytest.raises(F.FastfError):
        sweep.reps_summary_row(0.5, 0.1, 300, np.zeros((0, 7)))
    with pytest.raises(F.FastfError):
        sweep.reps_summary_row(0.5, 0.1, 300, np.zeros((65, 7)))


@pytest.mark.parametrize("n_features", [1, 63, 64, 65, 1000])
def test_gene_accumulators_and_their_row_against_the_reference(n_features):
    rng = np.random.default_rng(n_features)
    for n_reps in (1, 3, 64):
        cells = [rng.integers(0, 4, size=n_features).astype(np.uint32) for _ in range(n_reps)]
        cells[0][0] = 2 ** 31                                  # its square needs 64 bits
        never = n_features - 1                                 # never detected (at one feature that gene keeps the large count)
        for c in cells:
            if never:
                c[never] = 0
        det, tot, sq = (np.zeros(n_features, np.uint64) for _ in range(3))
        for c in cells:
            sweep.gene_reps_add_host(c, det, tot, sq)
        w_det, w_tot, w_sq = reps_ref.gene_accumulate(cells)
        assert [int(x) for x in det] == w_det and [int(x) for x in tot] == w_tot and [int(x) for x in sq] == w_sq
        assert int(sq[0]) >= 2 ** 62 and (not never or int(det[never]) == 0)
        got = sweep.genes_reps_row(1, 0.5, [int((c >= 1).sum()) for c in cells], det)[:-1].split("\t")
        want = reps_ref.genes_reps_row(["1.000", "0.500"], cells)
        reps_ref.assert_reps_row(got, want, (n_features, n_reps), lead=3)
        assert int(got[7]) <= int(got[5]) and int(got[8]) >= int(got[6])      # in all <= min, in any >= max
        assert (got[4] == "NA") == (n_reps == 1)
