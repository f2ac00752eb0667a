"""`--genes` of sweep and cap, the parts that need no device: the host twin of the per-gene summary against numpy, the row and
header text, the help texts, the refusals, and the census of the fixtures tests/test_gpu_genes.py runs on the device."""
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, cap, sweep
import genes_ref as G


@pytest.mark.parametrize("n_features", G.N_FEATURES)
def test_host_twin_against_numpy(n_features):
    for name in ["rows_0", "rows_1", "rows_65", "rows_5001", "edges", "one_gene", "big_sum"]:
        f, k = G.fixture(name, n_features)
        want_c, want_u = G.per_gene(f, k, n_features)
        got_c, got_u = sweep.genes_from_coo(f, k, n_features)
        assert got_c.dtype == np.uint32 and got_u.dtype == np.uint64
        np.testing.assert_array_equal(got_c.astype(np.int64), want_c, err_msg=name)
        np.testing.assert_array_equal(got_u.astype(np.int64), want_u, err_msg=name)
    c0, u0 = sweep.genes_from_coo([1, 2], [1, 1], 0)
    assert len(c0) == 0 and len(u0) == 0


def test_header_and_row_text():
    assert sweep.genes_header() == "\t".join(sweep.GENES_COLUMNS) + "\n"
    assert cap.genes_header() == "\t".join(cap.GENES_COLUMNS) + "\n"
    assert sweep.GENES_COLUMNS == ("rate_cell", "rate_depth", "seed", "genes_detected", "genes_min_cells_3", "genes_min_cells_10", "max_gene_umis")
    assert cap.GENES_COLUMNS == tuple("reads_per_cell" if c == "rate_depth" else c for c in sweep.GENES_COLUMNS)
    cells = np.array([0, 1, 2, 3, 9, 10, 11, 0, 400], np.uint32)
    umis = np.array([0, 1, 5, 3, 2 ** 33 + 7, 10, 11, 0, 400], np.uint64)
    assert sweep.genes_summary_row(0.25, 0.5, 926, cells, umis) == "0.250\t0.500\t926\t7\t5\t3\t%d\n" % (2 ** 33 + 7)
    assert sweep.genes_summary_row(1, 0, 1, cells, umis, reads_per_cell=40) == "1.000\t40\t1\t7\t5\t3\t%d\n" % (2 ** 33 + 7)
    assert sweep.genes_summary_row(1, 0, 1, np.zeros(0, np.uint32), np.zeros(0, np.uint64)) == "1.000\t0.000\t1\t0\t0\t0\t0\n"
    rng = np.random.default_rng(3)
    cells, umis = rng.integers(0, 14, size=5000), rng.integers(0, 10 ** 6, size=5000)
    assert sweep.genes_summary_row(0.3, 1, 7, cells, umis).rstrip("\n").split("\t")[3:] == G.table_fields(cells, umis)


def test_abi_pieces_are_there():
    assert sweep.GENES == 2 and cap.GENES == 2
    for name in ("fastf_dev_gene_summary", "fastf_sweep_genes_from_coo", "fastf_genes_summary_row", "fastf_sweep_genes_header",
                 "fastf_cap_genes_header"):
        assert name in _lib.ABI_SYMBOLS
    assert "gene_summary_kernel" in _lib.lib().fastf_kernel_names().decode().split(",")
    assert hasattr(F.Engine, "dev_gene_summary")


def test_help_texts_and_refusals_leave_no_genes_file(tmp_path):
    for verb in ("sweep", "cap"):
        r = subprocess.run([_lib.cli_path(), verb, "--help"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and "--genes" in r.stdout and "%s_gene_cells.tsv.gz" % verb in r.stdout
    b, f = tmp_path / "b.tsv", tmp_path / "f.tsv"
    b.write_text("AAAA-1\n"); f.write_text("ENSG00000000001\tG\tGene Expression\n")
    base = ["-a", str(b), "-f", str(f), "-b", str(tmp_path / "missing.bam"), "--genes"]
    jobs = [("sweep", ["-r", "0.5"], "does not exist"), ("sweep", ["-c", "0.5,0.5001"], "both print as"), ("sweep", ["-u"], "umi.tsv.gz"),
            ("cap", ["-n", "5"], "does not exist"), ("cap", ["-n", "0"], "at least 1"), ("cap", [], "needs -n"), ("cap", ["-n", "5", "-u"], "umi.tsv.gz"),
            ("cap", ["-n", "5", "--gene"], "unknown option")]
    for k, (verb, args, word) in enumerate(jobs):
        out = tmp_path / ("out%d" % k)
        r = subprocess.run([_lib.cli_path(), verb, "-o", str(out)] + base + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and word in r.stderr, (verb, args, r.stderr)
        for name in ("%s_genes.tsv", "%s_genes.tsv.partial", "%s_gene_cells.tsv.gz", "%s_gene_cells.tsv.gz.partial", "%s.tsv", "%s.tsv.partial"):
            assert not (out / (name % verb)).exists(), (verb, args, name)
    with pytest.raises(F.FastfError):
        sweep.sweep(tmp_path / "missing.bam", tmp_path / "o", b, f, [1], [1], genes=True)
    with pytest.raises(F.FastfError):
        cap.cap(tmp_path / "missing.bam", tmp_path / "o", b, f, [1], [5], genes=True)
    assert not (tmp_path / "o" / "sweep_genes.tsv").exists() and not (tmp_path / "o" / "cap_genes.tsv").exists()
    one, p_one = sweep._floats([1])
    caps = np.array([5], np.uint64)
    with pytest.raises(F.FastfError, match="unknown flags"):  # an unknown flag bit is still refused
        _lib.check(_lib.lib().fastf_sweep(b"x", b"y", b"b", b"f", p_one, 1, p_one, 1, 926, 4))
    with pytest.raises(F.FastfError, match="unknown flags"):
        _lib.check(_lib.lib().fastf_cap(b"x", b"y", b"b", b"f", p_one, 1, caps.ctypes.data, 1, 926, 4))


# ---- the census: what the GPU tests feed the kernel, asserted here so that a GPU test cannot pass by missing its own edge ----
def test_launch_model_and_row_counts():
    assert G.launch(1) == (True, 1, 512, 8192) and G.launch(16384) == (True, 1, 256, 4096)
    assert G.launch(16385) == (True, 2, 128, 2048) and G.launch(36601) == (True, 3, 85, 1360)
    assert G.launch(131072)[:2] == (True, 8) and G.launch(131073)[0] is False and G.launch(140_000) == (False, 1, 512, 8192)
    assert G.launch(36601, "0") == (False, 1, 512, 8192) and G.launch(36601, "2")[0] is False and G.launch(36601, "3")[0] is True
    for nf in G.N_FEATURES:
        rc = G.row_counts(nf)
        assert {0, 1, 63, 64, 65} <= set(rc)
        for env in (None, "0"):
            w = G.launch(nf, env)[3]
            assert w * 64 - 1 in rc and w * 64 + 1 in rc
        assert max(rc) <= 600_001                            # a few MB of rows at the most
    assert 1360 * 256 - 1 in G.row_counts(36601) and 1360 * 256 + 1 in G.row_counts(36601)


@pytest.mark.parametrize("n_features", G.N_FEATURES)
def test_census_of_the_gpu_fixtures(n_features):
    nf = n_features
    names = G.fixture_names(nf)
    assert names[:5] == ["rows_0", "rows_1", "rows_63", "rows_64", "rows_65"] and names[-3:] == ["edges", "one_gene", "big_sum"]
    for name in names:
        f, k = G.fixture(name, nf)
        f2, k2 = G.fixture(name, nf)
        assert f.dtype == np.uint32 and k.dtype == np.uint32 and len(f) == len(k)
        assert (f == f2).all() and (k == k2).all()           # the builders are deterministic: both test files see the same rows
        assert int(k.astype(np.uint64).sum()) < 2 ** 32      # the ABI's precondition
        if name.startswith("rows_"):
            n = int(name[5:])
            assert len(f) == n and (n == 0 or (f.min() >= 1 and f.max() <= nf))
            if n >= 63:
                assert (k == 0).any() and (k > 0).any()      # rows with count 0
        elif name == "edges":
            assert (k[f == 0] > 0).any() and (k[f == nf + 1] > 0).any() and (k[f == 0xFFFFFFFF] > 0).any()      # out of range, with counts that would show
            for g in [1, nf] + [g for g in (16384, 16385) if g <= nf] + [lo + 1 for lo in range(0, nf, G.LDS_GENES)]:
                assert (k[f == g] > 0).any() and (k[f == g] == 0).any(), g
            last_range_lo = (nf - 1) // G.LDS_GENES * G.LDS_GENES
            assert (f == nf).any() and nf > last_range_lo    # the last gene of the last range
            if nf >= 16385:
                assert (f == 16384).sum() >= 7 and (f == 16385).sum() >= 7
        elif name == "one_gene":
            assert len(f) == 100_001 and len(set(f.tolist())) == 1 and 1 <= int(f[0]) <= nf and (k == 0).any() and (k > 0).sum() > 64
        elif name == "big_sum":
            _, umis = G.per_gene(f, k, nf)
            assert umis.max() > 2 ** 31 and int(umis.sum()) < 2 ** 32
