"""`--cells` of sweep and cap on the GPU: the copy summary (fastf_dev_copy_summary) against numpy on the fixtures whose census
tests/test_cells_host.py takes and behind sort + K3u, and the commands — through the CLI and in process — with every number of
<verb>_cells.tsv and cells.tsv.gz against numpy on the oracle's -u rows of each point, and every other output byte for byte what a
run without --cells leaves."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, cap, hostmem, sweep
from helpers import Case
from oracle import oracle as O
import cap_ref
import cells_ref as R
import sortreduce_ref as S
from test_gpu_sweep import _case as _sweep_case, _write

pytestmark = pytest.mark.gpu

GUARD32, GUARD64 = 0x55555555, np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def engs():
    import torch
    assert torch.cuda.is_available()
    feats = np.arange(1, 501, dtype=np.uint64) | (np.uint64(2) << np.uint64(62))
    small = F.Engine(np.arange(1, 1001, dtype=np.uint64) | (np.uint64(1) << np.uint64(62)), feats, umi_max_bases=12)
    big = F.Engine(np.arange(1, 70_001, dtype=np.uint64) | (np.uint64(1) << np.uint64(62)), feats, umi_max_bases=12)
    for e, lay, cell_bits in ((big, R.BIG, 17), (small, R.FIXTURE, 10)):      # the layouts tests/cells_ref.py builds its keys in
        assert (e.key_bits - e.cell_bits, e.key_bits - e.cell_bits - e.feature_bits, e.cell_bits) == (lay.cs, lay.fs, cell_bits)
    assert small.key_bits == S.KEY_BITS
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    yield torch, small, big, cus
    small.close(); big.close()


def _summary(torch, e, d_uk, d_nc, d_n, n_cells, want, what):
    wr, wn, ws, wh = want
    outs = [torch.full((n_cells + 2,), GUARD32, dtype=torch.int32, device="cuda") for _ in range(3)]
    d_h = torch.full((R.BINS + 3,), -1, dtype=torch.int64, device="cuda")
    for _ in range(2):                                                      # the call clears what an earlier one left
        e.dev_copy_summary(d_uk, d_nc, d_n, n_cells, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), d_h.data_ptr())
        torch.cuda.synchronize()
    assert e.dev_error_bits() == 0
    r, z, s = (hostmem.to_host(o).view(np.uint32) for o in outs)
    h = hostmem.to_host(d_h).view(np.uint64)
    np.testing.assert_array_equal(r[:n_cells].astype(np.int64), wr, err_msg=what + ": reads")
    np.testing.assert_array_equal(z[:n_cells].astype(np.int64), wn, err_msg=what + ": null reads")
    np.testing.assert_array_equal(s[:n_cells].astype(np.int64), ws, err_msg=what + ": singletons")
    assert [int(x) for x in h[:R.BINS + 1]] == wh, what
    for o in (r, z, s):
        assert (o[n_cells:] == GUARD32).all(), "guard words behind a per-cell array were written: " + what
    assert (h[R.BINS + 1:] == GUARD64).all(), "guard words behind the histogram were written: " + what


def test_copy_summary_against_numpy(engs):
    """every fixture of tests/cells_ref.py, built for this device's launch: row counts at the wave and launch edges, one cell over
    every span, one row a cell, cells without rows, cells across lane 63, NULL heads, the bins' edges, a tail past 2^32, the hot
    bin, lists of 1, 3, 1000 and 70 000 cells, cells outside the list"""
    torch, small, big, cus = engs
    for name in R.fixture_names(cus):
        keys, k, n_cells = R.fixture(name, cus)
        lay = R.layout_of(name)
        want = R.from_keys(keys, k, n_cells, lay)
        d_uk = hostmem.to_device(np.concatenate([keys, np.full(R.PAD, (3 << lay.cs) | (1 << (lay.fs - 1)), np.uint64)]), "cuda")      # rows behind *d_nrows: never read
        d_nc = hostmem.to_device(np.concatenate([k, np.full(R.PAD, 9, np.uint32)]), "cuda")
        d_n = hostmem.to_device(np.array([len(keys)], np.uint64), "cuda")
        _summary(torch, big if lay is R.BIG else small, d_uk.data_ptr(), d_nc.data_ptr(), d_n.data_ptr(), n_cells, want, name)


def _chain(torch, e, keys, n_cells):
    """sort -> dev_umi_rows -> dev_copy_summary on unsorted keys"""
    n = len(keys)
    d_a = hostmem.to_device(keys, "cuda"); d_b = hostmem.to_device(np.zeros(n, np.uint64), "cuda")
    d_n = hostmem.to_device(np.array([n], np.uint64), "cuda")
    s = torch.cuda.current_stream().cuda_stream
    in_tmp = e.dev_sort(d_a.data_ptr(), d_b.data_ptr(), d_n.data_ptr(), n, stream=s)
    src = d_b if in_tmp else d_a
    d_uk = hostmem.to_device(np.zeros(n + 1, np.uint64), "cuda"); d_nc = torch.zeros((n + 1,), dtype=torch.int32, device="cuda")
    d_rows = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    e.dev_umi_rows(src.data_ptr(), d_n.data_ptr(), n, d_uk.data_ptr(), d_nc.data_ptr(), d_rows.data_ptr(), stream=s)
    torch.cuda.synchronize()
    uk, uc = S.umi_rows_ref(np.sort(keys))
    assert int(d_rows.item()) == len(uk)
    _summary(torch, e, d_uk.data_ptr(), d_nc.data_ptr(), d_rows.data_ptr(), n_cells, R.from_keys(uk, uc, n_cells), "chain of %d keys" % n)
    return uk, uc


def test_sort_umi_rows_copy_summary_chain(engs):
    torch, small, big, cus = engs
    _chain(torch, small, S.layout_keys(np.random.default_rng(11), 50_000), 1000)
    uk, uc = _chain(torch, small, S.null_run_keys(), 1000)   # NULL runs at the head of their groups, through K3u
    assert 2500 in uc and 2047 in uc


def test_copy_summary_refusals(engs):
    torch, small, big, cus = engs
    d = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = d.data_ptr()
    for hole in range(7):                                                   # every pointer in turn
        args = [p, p, p, 3, p, p, p, p]
        args[hole if hole < 3 else hole + 1] = 0
        with pytest.raises(F.FastfError, match="null argument"):
            small.dev_copy_summary(*args)
    feats = np.arange(1, 70_001, dtype=np.uint64) | (np.uint64(2) << np.uint64(62))
    wide = F.Engine(np.arange(1, 70_001, dtype=np.uint64) | (np.uint64(1) << np.uint64(62)), feats, umi_max_bases=16)
    try:
        assert wide.wide
        with pytest.raises(F.FastfError, match="wider than 64 bits"):
            wide.dev_copy_summary(p, p, p, 3, p, p, p, p)
    finally:
        wide.close()
    torch.cuda.synchronize()
    assert not hostmem.to_host(d).any()


# ---- the commands ----
RC, RD = [0.5, 1], [0.1, 1]
CAPS = {"edge": ([0.5, 1], [1, 5]), "mixed": ([1], [5, 40]), "scratch_widths": ([0.5, 1], [3]), "deep_groups": ([1], [1000])}
FILES = ("matrix.mtx.gz", "barcodes.tsv.gz", "features.tsv.gz")


def _case(name):
    if name == "umi20":                                      # 20-base UMIs: outside the resident form
        return Case(n=30_000, n_bar=400, n_gene=150, umi_len=20, umi_pool=512, p_n_umi=0.02, p_bad_xf=0.1, data_seed=35)
    if name == "deep_groups":                                # few cells and genes, few UMIs: (cell, feature) groups of hundreds of reads
        return Case(n=90_000, n_bar=30, n_gene=20, umi_pool=64)
    return _sweep_case(name)


_PREPARED, _REF = {}, {}


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("cells")


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


def _cli(verb, bam, b, f, out, extra, env=None):
    return subprocess.run([_lib.cli_path(), verb, "-b", str(bam), "-a", str(b), "-f", str(f), "-o", str(out)] + extra,
                          capture_output=True, text=True, timeout=600, env=None if env is None else dict(os.environ, **env))


def _prepared(work, verb, name, genes=False):
    """the case, its files, and ONE run without --cells through the CLI: what every other output must stay equal to"""
    if name not in _PREPARED:
        d = work / name; d.mkdir()
        case = _case(name)
        _PREPARED[name] = (case,) + tuple(_write(d, case)) + (d,)
    case, bam, b, f, d = _PREPARED[name]
    base = d / ("base_%s%s" % (verb, "_genes" if genes else ""))
    if not base.exists():
        r = _cli(verb, bam, b, f, base, _args(verb, name) + (["--genes"] if genes else []))
        assert r.returncode == 0, r.stderr
    return case, bam, b, f, d, base


def _reference(verb, name, case, bam, rc, second):
    """the oracle's run of a point with its -u rows: the records as they are (sweep), or masked to the kept set as tests/cap_ref.py
    masks them (cap)"""
    key = (verb, name, rc, second)
    if key not in _REF:
        rcf = float(np.float32(rc))
        if verb == "sweep":
            ora = O.run_bam2db(case.bt, case.ft, case.flags, case.xf, case.cb, case.gx, case.ub, rcf, float(np.float32(second)), case.seed,
                               str(bam).encode(), True)
        else:
            probe, cell, h, skip = cap_ref.hits_of(case, rcf, case.seed, str(bam).encode())
            T = cap_ref.thresholds(h, second)
            stream = O.mt_stream(case.seed, int(h.sum()), skip).astype(np.uint64)
            assert not (stream == np.uint64(0xFFFFFFFF)).any()
            keep = stream < T[cell[cell > 0] - 1]
            flags = np.array(case.flags, dtype=np.uint8, copy=True)
            flags[np.nonzero(cell > 0)[0][~keep]] &= np.uint8(~O.HAS_CB & 0xFF)
            ora = O.run_bam2db(case.bt, case.ft, flags, case.xf, case.cb, case.gx, case.ub, rcf, 1.0, case.seed, str(bam).encode(), True)
            assert ora["sampled"] == int(keep.sum())
        _REF[key] = ora
    return _REF[key]


def _gz(p):
    return gzip.decompress(open(p, "rb").read())


def _check(out, verb, name, case, bam, base, summary_only=False, genes=False):
    grid = _grid(verb, name)
    cols = list(sweep.CELLS_COLUMNS if verb == "sweep" else cap.CELLS_COLUMNS)
    lines = open(out / ("%s_cells.tsv" % verb)).read().split("\n")
    assert lines[0].split("\t") == cols and lines[-1] == "" and len(lines) == len(grid) + 2
    main = (sweep if verb == "sweep" else cap).read_table(out / ("%s.tsv" % verb))
    assert open(out / ("%s.tsv" % verb)).read() == open(base / ("%s.tsv" % verb)).read()
    for (dname, lead, rc, second), line, mrow in zip(grid, lines[1:-1], main):
        ora = _reference(verb, name, case, bam, rc, second)
        n_cells = int(mrow["n_cells"])
        reads, nulls, single, hist = R.from_oracle(ora, n_cells)
        got = line.split("\t")
        assert got == R.table_row(lead, case.seed, reads, nulls, single, hist), dname
        row = dict(zip(cols, got))
        # the identities that tie the table to <verb>.tsv and to itself
        assert int(reads.sum()) == int(mrow["sampled_valid_reads"]) == int(row["valid_reads"]) == ora["valid"]
        assert int(row["umis"]) == int(mrow["umis"])
        copies = [int(row["copies_%d" % k]) for k in range(1, 32)] + [int(row["copies_32_plus"])]
        assert sum(copies) == int(row["umis"])
        assert sum(k * c for k, c in zip(range(1, 32), copies)) + int(row["reads_copies_32_plus"]) + int(row["null_umi_reads"]) == int(row["valid_reads"])
        d = out / dname
        if summary_only:
            assert not d.exists()
            continue
        assert sorted(os.listdir(d)) == sorted(FILES + ("cells.tsv.gz",) + (("genes.tsv.gz",) if genes else ()))
        text = _gz(d / "cells.tsv.gz").decode().split("\n")
        assert text[-1] == "" and text[0].split("\t") == list(sweep.POINT_CELLS_COLUMNS)
        assert text[:-1] == R.point_lines(_gz(base / dname / "barcodes.tsv.gz"), _gz(base / dname / "matrix.mtx.gz"), reads, nulls, single), dname
        assert sum(int(t.split("\t")[1]) for t in text[1:-1]) == int(mrow["sampled_valid_reads"])
        for fn in FILES + (("genes.tsv.gz",) if genes else ()):             # byte for byte the files of a run without --cells
            assert open(d / fn, "rb").read() == open(base / dname / fn, "rb").read(), (dname, fn)
    top = ["%s.tsv" % verb, "%s_cells.tsv" % verb] + (["%s_genes.tsv" % verb, "%s_gene_cells.tsv.gz" % verb] if genes else [])
    for fn in top:
        if fn != "%s_cells.tsv" % verb:
            assert open(out / fn, "rb").read() == open(base / fn, "rb").read(), fn
    assert sorted(os.listdir(out)) == sorted(top + ([] if summary_only else [g[0] for g in grid]))
    return lines[1:-1]


@pytest.mark.parametrize("name", ["edge", "mixed", "scratch_widths", "deep_groups"])
@pytest.mark.parametrize("verb", ["sweep", "cap"])
def test_cli_cells(work, verb, name):
    case, bam, b, f, d, base = _prepared(work, verb, name)
    out = d / ("cli_" + verb)
    r = _cli(verb, bam, b, f, out, ["--cells"] + _args(verb, name))
    assert r.returncode == 0, r.stderr
    assert "point by point" not in r.stderr and "%s_cells.tsv is generated." % verb in r.stdout
    rows = _check(out, verb, name, case, bam, base)
    if name == "mixed" and verb == "sweep":                  # the numbers move with the depth: the table is not a constant
        assert int(rows[0].split("\t")[3]) > 0 and rows[0].split("\t")[3:] != rows[1].split("\t")[3:]


@pytest.mark.parametrize("verb", ["sweep", "cap"])
def test_cli_cells_beside_genes(work, verb):
    """both flags: the genes files and the matrices are the bytes of a run with --genes alone"""
    case, bam, b, f, d, base = _prepared(work, verb, "mixed", genes=True)
    out = d / ("both_" + verb)
    r = _cli(verb, bam, b, f, out, ["--genes", "--cells"] + _args(verb, "mixed"))
    assert r.returncode == 0, r.stderr
    _check(out, verb, "mixed", case, bam, base, genes=True)


@pytest.mark.parametrize("env", [{"FASTF_NO_STREAM_K1B": "1"}, {"FASTF_SORT_SKIP_BITS": "0"}, {"FASTF_LDS_TABLES": "0"}, {"FASTF_BLOCK_WIDE": "1"}])
@pytest.mark.parametrize("verb", ["sweep", "cap"])
def test_cli_cells_on_the_general_paths(work, verb, env):
    """SoA records and the tile form of K1b, a full first sort, lists in L2, wide blocked runs"""
    case, bam, b, f, d, base = _prepared(work, verb, "mixed")
    out = d / ("general_%s_%s" % (verb, list(env)[0]))
    r = _cli(verb, bam, b, f, out, ["--cells"] + _args(verb, "mixed"), env=env)
    assert r.returncode == 0, r.stderr
    _check(out, verb, "mixed", case, bam, base)


@pytest.mark.parametrize("name", ["edge", "mixed", "scratch_widths"])
def test_cells_in_process(work, name):
    case, bam, b, f, d, base = _prepared(work, "sweep", name)
    out = d / "inproc_sweep"
    rows = sweep.sweep(bam, out, b, f, RC, RD, seed=926, cells=True)
    assert rows == sweep.read_table(base / "sweep.tsv")
    lines = _check(out, "sweep", name, case, bam, base)
    assert [list(t.values()) for t in sweep.read_cells_table(out / "sweep_cells.tsv")] == [ln.split("\t") for ln in lines]
    out2 = d / "inproc_sweep_summary"
    sweep.sweep(bam, out2, b, f, RC, RD, seed=926, cells=True, summary_only=True)
    _check(out2, "sweep", name, case, bam, base, summary_only=True)
    assert open(out2 / "sweep_cells.tsv").read() == open(out / "sweep_cells.tsv").read()
    case, bam, b, f, d, base = _prepared(work, "cap", name)
    rates, caps = CAPS[name]
    out3 = d / "inproc_cap"
    rows = cap.cap(bam, out3, b, f, rates, caps, seed=926, cells=True)
    assert rows == cap.read_table(base / "cap.tsv")
    lines = _check(out3, "cap", name, case, bam, base)
    assert [list(t.values()) for t in cap.read_cells_table(out3 / "cap_cells.tsv")] == [ln.split("\t") for ln in lines]
    out4 = d / "inproc_cap_summary"
    cap.cap(bam, out4, b, f, rates, caps, seed=926, cells=True, summary_only=True)
    _check(out4, "cap", name, case, bam, base, summary_only=True)


def test_jobs_outside_the_resident_form_are_refused_with_cells(work):
    """20-base UMIs: sweep would run point by point; with --cells it exits 1, names the reason and leaves no table and no point"""
    case, bam, b, f, d, _ = _prepared(work, "sweep", "umi20")
    for verb, extra in (("sweep", _args("sweep", "umi20")), ("cap", ["-n", "5,50"])):
        out = d / ("refused_" + verb)
        r = _cli(verb, bam, b, f, out, ["--cells"] + extra)
        assert r.returncode == 1 and "outside" in r.stderr and "resident form" in r.stderr and "UMIs beyond" in r.stderr, r.stderr
        assert "point by point" not in r.stderr
        assert os.listdir(out) == [], os.listdir(out)
