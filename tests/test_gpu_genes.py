"""`--genes` of sweep and cap on the GPU: the per-gene summary (fastf_dev_gene_summary) against numpy on the fixtures whose census
tests/test_genes_host.py takes, and the commands — through the CLI and in process — with every number of the three genes files
against numpy on the oracle's matrix of each point, and every other output byte for byte what a run without --genes leaves."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, cap, hostmem, sweep
from helpers import Case
import cap_ref
import genes_ref as G
from test_gpu_sweep import _case as _sweep_case, _oracle, _write

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    cells = np.arange(1, 101, dtype=np.uint64) | (np.uint64(1) << np.uint64(62))
    feats = np.arange(1, 51, dtype=np.uint64) | (np.uint64(2) << np.uint64(62))
    e = F.Engine(cells, feats, umi_max_bases=12)
    yield torch, e
    e.close()


def _run(torch, e, f, k, nf, what):
    want_c, want_u = G.per_gene(f, k, nf)
    d_f = hostmem.to_device(np.concatenate([f, np.full(G.PAD, 1, np.uint32)]), "cuda")          # rows behind *d_nnz: never read
    d_k = hostmem.to_device(np.concatenate([k, np.full(G.PAD, 9, np.uint32)]), "cuda")
    d_nnz = hostmem.to_device(np.array([len(f)], np.uint64), "cuda")
    d_c = torch.full((nf + 2,), 0x55555555, dtype=torch.int32, device="cuda")
    d_u = torch.full((nf + 2,), -1, dtype=torch.int64, device="cuda")
    for _ in range(2):                                                      # the call clears what an earlier one left
        e.dev_gene_summary(d_f.data_ptr(), d_k.data_ptr(), d_nnz.data_ptr(), nf, d_c.data_ptr(), d_u.data_ptr())
        torch.cuda.synchronize()
    c, u = hostmem.to_host(d_c).view(np.uint32), hostmem.to_host(d_u).view(np.uint64)
    np.testing.assert_array_equal(c[:nf].astype(np.int64), want_c, err_msg=what)
    np.testing.assert_array_equal(u[:nf].astype(np.int64), want_u, err_msg=what)
    assert (c[nf:] == 0x55555555).all() and (u[nf:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "guard words behind the arrays were written: " + what
    return d_nnz, d_c, d_u


@pytest.mark.parametrize("lds_ranges", [None, "0"])
@pytest.mark.parametrize("n_features", G.N_FEATURES)
def test_gene_summary_against_numpy(eng, n_features, lds_ranges, monkeypatch):
    """one LDS range (1, 3, 16 384 genes), two (16 385), three (36 601), past the eight ranges (140 000: the general form), and
    every list on the general form (FASTF_GENE_LDS_RANGES=0)"""
    torch, e = eng
    if lds_ranges is None:
        monkeypatch.delenv("FASTF_GENE_LDS_RANGES", raising=False)
    else:
        monkeypatch.setenv("FASTF_GENE_LDS_RANGES", lds_ranges)
    for name in G.fixture_names(n_features):
        f, k = G.fixture(name, n_features)
        d_nnz, d_c, d_u = _run(torch, e, f, k, n_features, "%s, %d genes, ranges %s" % (name, n_features, lds_ranges))
    # no row buffer at all: the arrays are cleared, nothing else happens
    e.dev_gene_summary(0, 0, d_nnz.data_ptr(), n_features, d_c.data_ptr(), d_u.data_ptr())
    torch.cuda.synchronize()
    assert not hostmem.to_host(d_c)[:n_features].any() and not hostmem.to_host(d_u)[:n_features].any()
    assert (hostmem.to_host(d_c).view(np.uint32)[n_features:] == 0x55555555).all()


@pytest.mark.parametrize("n_features", [8 * G.LDS_GENES, 8 * G.LDS_GENES + 1])
def test_gene_summary_at_the_last_lds_range(eng, n_features, monkeypatch):
    """131 072 genes: eight ranges, the most the LDS form takes; one gene more goes to the general form"""
    torch, e = eng
    monkeypatch.delenv("FASTF_GENE_LDS_RANGES", raising=False)
    assert G.launch(n_features)[0] is (n_features == 8 * G.LDS_GENES)
    for name in ("edges", "rows_70001"):
        f, k = G.fixture(name, n_features)
        _run(torch, e, f, k, n_features, "%s, %d genes" % (name, n_features))


def test_gene_summary_refuses_null_outputs(eng):
    torch, e = eng
    d = torch.zeros(8, dtype=torch.int64, device="cuda")
    with pytest.raises(F.FastfError):
        e.dev_gene_summary(d.data_ptr(), d.data_ptr(), d.data_ptr(), 3, 0, d.data_ptr())
    with pytest.raises(F.FastfError):
        e.dev_gene_summary(d.data_ptr(), d.data_ptr(), 0, 3, d.data_ptr(), d.data_ptr())


# ---- the commands ----
RC, RD = [0.5, 1], [0.1, 1]
CAPS = {"edge": ([0.5, 1], [1, 5]), "mixed": ([1], [5, 40])}
FILES = ("matrix.mtx.gz", "barcodes.tsv.gz", "features.tsv.gz")


def _case(name):
    if name == "umi20":                                      # 20-base UMIs: outside the resident form, sweep runs point by point
        return Case(n=30_000, n_bar=400, n_gene=150, umi_len=20, umi_pool=512, p_n_umi=0.02, p_bad_xf=0.1, data_seed=35)
    return _sweep_case(name)


_PREPARED, _REF = {}, {}


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("genes")


def _grid(verb, name):
    """[(directory name, the first two columns, rate_cell, second)] in the table's order"""
    if verb == "sweep":
        return [(sweep.point_dir(rc, rd), ["%.3f" % rc, "%.3f" % rd], rc, rd) for rc in RC for rd in RD]
    rates, caps = CAPS[name]
    return [(cap.point_dir(rc, n), ["%.3f" % rc, str(n)], rc, n) for rc in rates for n in caps]


def _args(verb, name):
    if verb == "sweep":
        return ["-c", ",".join("%g" % r for r in RC), "-r", ",".join("%g" % r for r in RD)]
    rates, caps = CAPS[name]
    return ["-c", ",".join("%g" % r for r in rates), "-n", ",".join(str(n) for n in caps)]


def _prepared(work, verb, name):
    """the case, its files, and ONE run without --genes through the CLI: what every other output must stay equal to"""
    if name not in _PREPARED:
        d = work / name; d.mkdir()
        case = _case(name)
        _PREPARED[name] = (case,) + tuple(_write(d, case)) + (d,)
    case, bam, b, f, d = _PREPARED[name]
    base = d / ("base_" + verb)
    if not base.exists():
        r = subprocess.run([_lib.cli_path(), verb, "-b", str(bam), "-a", str(b), "-f", str(f), "-o", str(base)] + _args(verb, name),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
    return case, bam, b, f, d, base


def _reference(verb, name, case, bam, rc, second):
    """(decompressed matrix, decompressed features) of a point from the oracle (sweep) or cap_ref (the oracle on masked records)"""
    key = (verb, name, rc, second)
    if key not in _REF:
        ora = _oracle(case, bam, rc, second) if verb == "sweep" else cap_ref.point(case, str(bam).encode(), rc, second, case.seed)
        _REF[key] = (ora["matrix"], ora["features"])
    return _REF[key]


def _gz(p):
    return gzip.decompress(open(p, "rb").read())


def _check(out, verb, name, case, bam, base, summary_only=False):
    grid = _grid(verb, name)
    lines = open(out / ("%s_genes.tsv" % verb)).read().split("\n")
    cols = sweep.GENES_COLUMNS if verb == "sweep" else cap.GENES_COLUMNS
    assert lines[0].split("\t") == list(cols) and lines[-1] == "" and len(lines) == len(grid) + 2
    per_point, ids = [], None
    for (dname, lead, rc, second), line in zip(grid, lines[1:-1]):
        matrix, features = _reference(verb, name, case, bam, rc, second)
        want, cells, umis = G.expected_genes_row(matrix, lead, case.seed)
        assert line.split("\t") == want, dname
        ids = G.feature_ids(features)
        assert len(ids) == len(cells)
        per_point.append(cells)
        d = out / dname
        if summary_only:
            assert not d.exists()
            continue
        assert sorted(os.listdir(d)) == sorted(FILES + ("genes.tsv.gz",))
        rows = _gz(d / "genes.tsv.gz").decode().split("\n")
        assert rows[-1] == "" and [r.split("\t") for r in rows[:-1]] == [[i, str(int(c)), str(int(u))] for i, c, u in zip(ids, cells, umis)], dname
        for fn in FILES:                                                # byte for byte the files of a run without --genes
            assert open(d / fn, "rb").read() == open(base / dname / fn, "rb").read(), (dname, fn)
    table = _gz(out / ("%s_gene_cells.tsv.gz" % verb)).decode().split("\n")
    assert table[-1] == "" and table[0].split("\t") == ["feature"] + [g[0] for g in grid]
    body = [ln.split("\t") for ln in table[1:-1]]
    assert [r[0] for r in body] == ids
    got = np.array([[int(x) for x in r[1:]] for r in body], dtype=np.int64).reshape(len(ids), len(grid))
    np.testing.assert_array_equal(got, np.stack(per_point, axis=1))
    assert open(out / ("%s.tsv" % verb)).read() == open(base / ("%s.tsv" % verb)).read()
    top = ["%s.tsv" % verb, "%s_genes.tsv" % verb, "%s_gene_cells.tsv.gz" % verb]
    assert sorted(os.listdir(out)) == sorted(top + ([] if summary_only else [g[0] for g in grid]))
    return lines[1:-1]


@pytest.mark.parametrize("name", ["edge", "mixed", "umi20"])
def test_cli_sweep_genes(work, name):
    case, bam, b, f, d, base = _prepared(work, "sweep", name)
    out = d / "cli"
    r = subprocess.run([_lib.cli_path(), "sweep", "--genes", "-b", str(bam), "-a", str(b), "-f", str(f), "-o", str(out)] + _args("sweep", name),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert ("point by point" in r.stderr) == (name == "umi20")
    rows = _check(out, "sweep", name, case, bam, base)
    if name == "mixed":                                      # the numbers move with the depth: the table is not a constant
        assert int(rows[0].split("\t")[3]) > 0 and rows[0].split("\t")[3:] != rows[1].split("\t")[3:]


def test_cli_sweep_genes_on_the_general_forms(work):
    """the per-gene kernel on global atomics, behind the SoA records and the tile form of K1b"""
    case, bam, b, f, d, base = _prepared(work, "sweep", "mixed")
    out = d / "general"
    r = subprocess.run([_lib.cli_path(), "sweep", "-b", str(bam), "-a", str(b), "-f", str(f), "-o", str(out), "--genes"] + _args("sweep", "mixed"),
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, FASTF_GENE_LDS_RANGES="0", FASTF_NO_STREAM_K1B="1"))
    assert r.returncode == 0, r.stderr
    _check(out, "sweep", "mixed", case, bam, base)


@pytest.mark.parametrize("name", ["edge", "mixed", "umi20"])
def test_sweep_genes_in_process(work, name):
    case, bam, b, f, d, base = _prepared(work, "sweep", name)
    out = d / "inproc"
    rows = sweep.sweep(bam, out, b, f, RC, RD, seed=926, genes=True)
    assert rows == sweep.read_table(base / "sweep.tsv")
    lines = _check(out, "sweep", name, case, bam, base)
    table = sweep.read_genes_table(out / "sweep_genes.tsv")
    assert [list(t.values()) for t in table] == [ln.split("\t") for ln in lines]


@pytest.mark.parametrize("name", ["mixed", "umi20"])
def test_summary_only_genes_writes_the_grid_files_alone(work, name):
    case, bam, b, f, d, base = _prepared(work, "sweep", name)
    out = d / "summary"
    r = subprocess.run([_lib.cli_path(), "sweep", "--summary-only", "--genes", "-b", str(bam), "-a", str(b), "-f", str(f), "-o", str(out)] + _args("sweep", name),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    _check(out, "sweep", name, case, bam, base, summary_only=True)


@pytest.mark.parametrize("name", ["edge", "mixed"])
def test_cap_genes(work, name):
    case, bam, b, f, d, base = _prepared(work, "cap", name)
    out = d / "cap_cli"
    r = subprocess.run([_lib.cli_path(), "cap", "--genes", "-b", str(bam), "-a", str(b), "-f", str(f), "-o", str(out)] + _args("cap", name),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = _check(out, "cap", name, case, bam, base)
    rates, caps = CAPS[name]
    out2 = d / "cap_inproc"
    rows = cap.cap(bam, out2, b, f, rates, caps, seed=926, genes=True)
    assert rows == cap.read_table(base / "cap.tsv")
    _check(out2, "cap", name, case, bam, base)
    assert [list(t.values()) for t in cap.read_genes_table(out2 / "cap_genes.tsv")] == [ln.split("\t") for ln in lines]
    out3 = d / "cap_summary"
    cap.cap(bam, out3, b, f, rates, caps, seed=926, summary_only=True, genes=True)
    _check(out3, "cap", name, case, bam, base, summary_only=True)


def test_cap_refusal_leaves_no_genes_file(work):
    """20-base UMIs: a cap has no point-by-point form, with --genes as without"""
    case, bam, b, f, d, _ = _prepared(work, "sweep", "umi20")
    out = d / "cap_refused"
    r = subprocess.run([_lib.cli_path(), "cap", "--genes", "-b", str(bam), "-a", str(b), "-f", str(f), "-o", str(out), "-n", "5,50"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "outside the resident form" in r.stderr, r.stderr
    assert [n for n in os.listdir(out) if "genes" in n or "gene_cells" in n or n.startswith("cap.tsv")] == []
