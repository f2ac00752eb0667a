"""`fastF sweep` on the GPU: the decision planes (fastf_dev_mt_decisions_multi), the per-cell summary (fastf_dev_cell_summary),
and the command — through the CLI and through fastf_sweep in process — against the oracle's bytes for every point of a grid."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, hostmem, synth, sweep
from helpers import Case
from oracle import oracle as O
from sweep_ref import expected_row

pytestmark = pytest.mark.gpu

T = {0.1: 429496736, 0.5: 2147483648, 1.0: 4294967295}          # fastf_draw_threshold (tests/golden/survey_8c.json)
THRESHOLDS = [0, T[0.1], T[0.5], T[1.0], 1 << 32]
N_DRAWS = [1, 63, 64, 65, 624 * 256 + 7, 3_000_001]


@pytest.fixture(scope="module")
def engines():
    import torch
    assert torch.cuda.is_available()
    cells = np.arange(1, 1001, dtype=np.uint64) | (np.uint64(1) << np.uint64(62))
    feats = np.arange(1, 501, dtype=np.uint64) | (np.uint64(2) << np.uint64(62))
    engs = [F.Engine(cells, feats, umi_max_bases=12, threshold=t) for t in THRESHOLDS]
    yield torch, engs
    for e in engs:
        e.close()


@pytest.mark.parametrize("seed", [926, 1])
@pytest.mark.parametrize("skip", [0, 3, 5000])
def test_decision_planes_are_the_stream_below_each_threshold(engines, seed, skip):
    """plane j = oracle.mt_stream(...) < T_j packed on the host, tail bits zero, and equal to what fastf_dev_mt_decisions gives
    an engine created with that threshold"""
    torch, engs = engines
    assert [F.draw_threshold(r) for r in (0.1, 0.5, 1.0)] == [T[0.1], T[0.5], T[1.0]]
    stream = O.mt_stream(seed, max(N_DRAWS), skip=skip).astype(np.uint64)
    for n in N_DRAWS:
        stride = (n + 63) // 64 * 2 + 6                      # words; planes 8-byte aligned, a gap between them that must stay untouched
        planes = torch.full((len(THRESHOLDS) * stride,), -1, dtype=torch.int32, device="cuda")
        engs[2].dev_mt_decisions_multi(seed, skip, n, THRESHOLDS, planes.data_ptr(), stride)
        torch.cuda.synchronize()
        got = hostmem.to_host(planes).view(np.uint32).reshape(len(THRESHOLDS), stride)
        used = (n + 63) // 64 * 2
        for j, t in enumerate(THRESHOLDS):
            bits = np.unpackbits(got[j, :used].copy().view(np.uint8), bitorder="little")
            want = (stream[:n] < np.uint64(t)).astype(np.uint8)
            np.testing.assert_array_equal(bits[:n], want, err_msg="n=%d threshold=%d" % (n, t))
            assert not bits[n:].any(), "tail bits of the last 64-bit word, n=%d threshold=%d" % (n, t)
            assert (got[j, used:] == 0xFFFFFFFF).all(), "words behind the plane were written"
            one = torch.full((used + 2,), -1, dtype=torch.int32, device="cuda")
            engs[j].dev_mt_decisions(seed, skip, n, one.data_ptr())
            torch.cuda.synchronize()
            np.testing.assert_array_equal(hostmem.to_host(one).view(np.uint32)[:used], got[j, :used])


def test_decision_planes_take_more_thresholds_than_one_launch_holds(engines):
    torch, engs = engines
    thr = [int(x) for x in np.linspace(0, 1 << 32, 37)]
    n = 100_001
    stride = (n + 63) // 64 * 2
    planes = torch.zeros((len(thr) * stride,), dtype=torch.int32, device="cuda")
    engs[0].dev_mt_decisions_multi(7, 11, n, thr, planes.data_ptr(), stride)
    got = hostmem.to_host(planes).view(np.uint32).reshape(len(thr), stride)
    stream = O.mt_stream(7, n, skip=11).astype(np.uint64)
    for j, t in enumerate(thr):
        bits = np.unpackbits(got[j].copy().view(np.uint8), bitorder="little")
        np.testing.assert_array_equal(bits[:n], (stream < np.uint64(t)).astype(np.uint8))
    with pytest.raises(F.FastfError):
        engs[0].dev_mt_decisions_multi(7, 11, n, thr, planes.data_ptr(), stride - 1)     # odd / too short
    with pytest.raises(F.FastfError):
        engs[0].dev_mt_decisions_multi(7, 11, n, [(1 << 32) + 1], planes.data_ptr(), stride)


def _summary_case(name):
    rng = np.random.default_rng(abs(hash(name)) % 1000 + 17)
    if name == "one_cell_only":
        n_cells, cell = 10, np.full(5000, 4)
    elif name == "every_cell_one_row":
        n_cells = 30_000; cell = np.arange(1, n_cells + 1)
    elif name == "a_cell_of_200000_rows":
        n_cells = 300; cell = np.sort(np.concatenate([rng.integers(1, 301, size=50_000), np.full(200_000, 150)]))
    elif name == "empty":
        n_cells, cell = 50, np.zeros(0, np.int64)
    else:
        n_cells = int(name.split("_")[1]); cell = np.sort(rng.integers(1, n_cells + 1, size=max(1, 3 * n_cells if n_cells > 1 else 777)))
    count = rng.integers(0, 5, size=len(cell))
    if len(count) > 3:
        count[:3] = [4_000_000_000, 4_000_000_000, 0]                  # sums beyond 32 bits
    return n_cells, cell.astype(np.uint32), count.astype(np.uint32)


@pytest.mark.parametrize("name", ["one_cell_only", "every_cell_one_row", "a_cell_of_200000_rows", "empty", "cells_1", "cells_65535",
                                  "cells_65536", "cells_100000"])
def test_cell_summary_against_numpy(engines, name):
    torch, engs = engines
    n_cells, cell, count = _summary_case(name)
    want_u = np.zeros(n_cells, np.uint64); np.add.at(want_u, cell.astype(np.int64) - 1, count.astype(np.uint64))
    want_g = np.zeros(n_cells, np.int64); np.add.at(want_g, cell.astype(np.int64) - 1, (count >= 1).astype(np.int64))
    pad = 1000                                                              # rows behind *d_nnz that must not be read
    d_cell = hostmem.to_device(np.concatenate([cell, np.full(pad, 1, np.uint32)]), "cuda")
    d_count = hostmem.to_device(np.concatenate([count, np.full(pad, 9, np.uint32)]), "cuda")
    d_nnz = hostmem.to_device(np.array([len(cell)], np.uint64), "cuda")
    d_u = torch.full((n_cells + 2,), -1, dtype=torch.int64, device="cuda")
    d_g = torch.full((n_cells + 1,), -1, dtype=torch.int32, device="cuda")
    for _ in range(2):                                                      # the call clears what an earlier one left
        engs[0].dev_cell_summary(d_cell.data_ptr(), d_count.data_ptr(), d_nnz.data_ptr(), n_cells, d_u.data_ptr(), d_g.data_ptr())
        torch.cuda.synchronize()
        u, g = hostmem.to_host(d_u).view(np.uint64), hostmem.to_host(d_g).view(np.uint32)
        np.testing.assert_array_equal(u[:n_cells], want_u)
        np.testing.assert_array_equal(g[:n_cells].astype(np.int64), want_g)
        assert int(u[n_cells]) == int(count.astype(np.uint64).sum())
        assert u[n_cells + 1] == np.uint64(0xFFFFFFFFFFFFFFFF) and g[n_cells] == 0xFFFFFFFF      # nothing behind the arrays
    hu, hg, htot = sweep.cells_from_coo(cell, count, n_cells)
    np.testing.assert_array_equal(hu, want_u); np.testing.assert_array_equal(hg.astype(np.int64), want_g)


# ---- the command ----
RATES_C, RATES_R = [0.3, 0.5, 1], [0, 0.1, 0.5, 1]
GRID = ["-c", "0.3,0.5,1", "-r", "0,0.1,0.5,1"]


class _Edge:
    """the 9-record edge case of SURVEY section 8c as a Case-like object"""
    def __init__(self):
        fx = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "survey_8c.json")))["edge_case"]
        self.bt, self.ft = fx["barcodes"].encode(), fx["features"].encode()
        recs = fx["records"]
        self.flags, self.xf = np.full(len(recs), 15, np.uint8), np.full(len(recs), 25, np.int32)
        self.cb = np.array([r[0].encode() for r in recs], dtype="S8")
        self.gx = np.array([r[1].encode() for r in recs], dtype="S8")
        self.ub = np.array([r[2].encode() for r in recs], dtype="S16")
        self.seed = 926


def _case(name):
    if name == "edge":
        return _Edge()
    if name == "mixed":
        return Case(n=200_000, n_bar=600, n_gene=500, umi_len=12, dup_factor=3.0, p_no_cb=0.05, p_unlisted_cb=0.05, p_bad_xf=0.15,
                    p_n_umi=0.01, p_multi_gene=0.02)
    if name == "scratch_widths":                         # 70 000 barcodes: 32-bit cell scratch at -c 1, 16-bit at -c 0.5
        return Case(n=150_000, n_bar=70_000, n_gene=300, umi_len=12, dup_factor=2.0, p_unlisted_cb=0.05, p_bad_xf=0.1, p_n_umi=0.01, data_seed=7)
    raise KeyError(name)


def _write(tmp_path, case):
    bam, b, f = tmp_path / "in.bam", tmp_path / "barcodes.in.tsv", tmp_path / "features.in.tsv"
    synth.write_bam(str(bam), case.flags, case.xf, case.cb, case.gx, case.ub)
    b.write_bytes(case.bt); f.write_bytes(case.ft)
    return bam, b, f


def _gz(p):
    return gzip.decompress(open(p, "rb").read())


def _oracle(case, bam, rc, rd):
    return O.run_bam2db(case.bt, case.ft, case.flags, case.xf, case.cb, case.gx, case.ub, float(np.float32(rc)), float(np.float32(rd)),
                        case.seed, str(bam).encode(), False)


def _check_outputs(out, case, bam, summary_only=False):
    rows = [ln.split("\t") for ln in open(out / "sweep.tsv").read().split("\n")]
    assert rows[0] == list(sweep.COLUMNS) and rows[-1] == [""]
    rows = rows[1:-1]
    assert len(rows) == len(RATES_C) * len(RATES_R)
    k = 0
    for rc in RATES_C:
        for rd in RATES_R:
            ora = _oracle(case, bam, rc, rd)
            d = out / sweep.point_dir(rc, rd)
            if summary_only:
                assert not d.exists()
            else:
                assert _gz(d / "matrix.mtx.gz") == ora["matrix"], d
                assert _gz(d / "barcodes.tsv.gz") == ora["barcodes"], d
                assert _gz(d / "features.tsv.gz") == ora["features"], d
            assert rows[k] == expected_row(ora["matrix"], rc, rd, case.seed), (rc, rd)
            if rd == 0:
                assert rows[k][5] == "0" and rows[k][7] == "0"            # -r 0: nothing sampled, a valid empty matrix
            k += 1
    assert not (out / "sweep.tsv.partial").exists()


@pytest.mark.parametrize("name", ["edge", "mixed", "scratch_widths"])
def test_cli_sweep_equals_bam2db_point_by_point(tmp_path, name):
    case = _case(name)
    bam, b, f = _write(tmp_path, case)
    out = tmp_path / "out"
    r = subprocess.run([_lib.cli_path(), "sweep", "-b", str(bam), "-a", str(b), "-f", str(f), "-o", str(out), "-d", str(tmp_path / "x.db")] + GRID,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "point by point" not in r.stderr
    _check_outputs(out, case, bam)
    # --summary-only: the identical table, no point directories
    out2 = tmp_path / "out2"
    r = subprocess.run([_lib.cli_path(), "sweep", "--bam", str(bam), "--barcode=" + str(b), "-f", str(f), "--out", str(out2), "--summary-only",
                        "--cell=0.3,0.5,1", "--depth", "0,0.1,0.5,1", "-s926"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert open(out2 / "sweep.tsv").read() == open(out / "sweep.tsv").read()
    assert sorted(os.listdir(out2)) == ["sweep.tsv"]


@pytest.mark.parametrize("env", [{"FASTF_LDS_TABLES": "0"}, {"FASTF_LDS_CELLS": "0"}, {"FASTF_NO_STREAM_K1B": "1"}, {"FASTF_SORT_SKIP_BITS": "0"},
                                 {"FASTF_GENES_NO_DIRECT": "1"}, {"FASTF_BLOCK_WIDE": "1"}, {"FASTF_GPU_PARSE": "0"}])
def test_cli_sweep_on_the_general_paths(tmp_path, env):
    """gene list in L2, no streaming K1b (SoA records, tile form), full sort, wide blocked runs, host-packed records"""
    case = _case("mixed")
    bam, b, f = _write(tmp_path, case)
    out = tmp_path / "out"
    r = subprocess.run([_lib.cli_path(), "sweep", "-b", str(bam), "-a", str(b), "-f", str(f), "-o", str(out)] + GRID,
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr
    assert "point by point" not in r.stderr
    _check_outputs(out, case, bam)


def test_sweep_in_process(tmp_path):
    case = _case("mixed")
    bam, b, f = _write(tmp_path, case)
    out = tmp_path / "out"
    rows = sweep.sweep(bam, out, b, f, RATES_C, RATES_R, seed=926)
    assert len(rows) == 12 and rows[0]["rate_cell"] == "0.300" and rows[-1]["rate_depth"] == "1.000"
    _check_outputs(out, case, bam)
    # -c 1 consumes no SampleInt draws: the point (1, 1) keeps every read with a listed barcode
    full = [r for r in rows if r["rate_cell"] == "1.000" and r["rate_depth"] == "1.000"][0]
    assert F.Lists(case.bt, case.ft, 1.0, 926).mt_skip == 0 and int(full["sampled_reads"]) > 0
    out2 = tmp_path / "out2"
    rows2 = sweep.sweep(bam, out2, b, f, RATES_C, RATES_R, seed=926, summary_only=True)
    assert rows2 == rows and sorted(os.listdir(out2)) == ["sweep.tsv"]
    # another seed is another grid
    rows3 = sweep.sweep(bam, tmp_path / "out3", b, f, [0.5], [0.5], seed=1, summary_only=True)
    ora = O.run_bam2db(case.bt, case.ft, case.flags, case.xf, case.cb, case.gx, case.ub, 0.5, 0.5, 1, str(bam).encode(), False)
    assert list(rows3[0].values()) == expected_row(ora["matrix"], 0.5, 0.5, 1)


def test_wide_jobs_run_point_by_point_with_the_same_bytes(tmp_path):
    """20-base UMIs do not fit a 64-bit key: every point goes through bam2db() itself, one line on stderr says so"""
    case = Case(n=30_000, n_bar=400, n_gene=150, umi_len=20, umi_pool=512, p_n_umi=0.02, p_bad_xf=0.1, data_seed=35)
    bam, b, f = _write(tmp_path, case)
    out = tmp_path / "out"
    r = subprocess.run([_lib.cli_path(), "sweep", "-b", str(bam), "-a", str(b), "-f", str(f), "-o", str(out), "-c", "0.5,1", "-r", "0.5,1"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "point by point" in r.stderr
    rows = [ln.split("\t") for ln in open(out / "sweep.tsv").read().split("\n")[1:-1]]
    k = 0
    for rc in (0.5, 1):
        for rd in (0.5, 1):
            d = out / sweep.point_dir(rc, rd)
            ref = tmp_path / ("ref_%d" % k); ref.mkdir()
            rr = subprocess.run([_lib.cli_path(), "bam2db", "-b", str(bam), "-a", str(b), "-f", str(f), "-o", str(ref), "-c", str(rc), "-r", str(rd)],
                                capture_output=True, text=True, timeout=600)
            assert rr.returncode == 0, rr.stderr
            for name in ("matrix.mtx.gz", "barcodes.tsv.gz", "features.tsv.gz"):
                assert _gz(d / name) == _gz(ref / name), (d, name)
            assert _gz(d / "matrix.mtx.gz") == _oracle(case, bam, rc, rd)["matrix"]
            assert rows[k] == expected_row(_gz(d / "matrix.mtx.gz"), rc, rd, 926)
            k += 1
    out2 = tmp_path / "out2"
    r = subprocess.run([_lib.cli_path(), "sweep", "-b", str(bam), "-a", str(b), "-f", str(f), "-o", str(out2), "-c", "0.5,1", "-r", "0.5,1", "--summary-only"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert open(out2 / "sweep.tsv").read() == open(out / "sweep.tsv").read() and sorted(os.listdir(out2)) == ["sweep.tsv"]


def test_errors_exit_1_and_leave_no_partial_table(tmp_path):
    case = Case(n=40_000, n_bar=100, n_gene=50)
    bam, b, f = _write(tmp_path, case)
    cut = tmp_path / "cut.bam"
    data = open(bam, "rb").read()
    cut.write_bytes(data[:len(data) * 2 // 3])
    base = ["-a", str(b), "-f", str(f)]
    for k, (args, word) in enumerate([
            (["-b", str(tmp_path / "missing.bam")], "does not exist"), (["-b", str(cut)], "truncated"),
            (["-b", str(bam), "-u"], "umi.tsv.gz"), (["-b", str(bam), "-c", "0.5,0.5001"], "both print as")]):
        out = tmp_path / ("out%d" % k)
        r = subprocess.run([_lib.cli_path(), "sweep", "-o", str(out)] + base + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 1, (args, r.stderr)
        assert "Error" in r.stderr and word in r.stderr.lower().replace("error", "Error") or word in r.stderr.lower(), (args, r.stderr)
        assert not (out / "sweep.tsv").exists() and not (out / "sweep.tsv.partial").exists()
    with pytest.raises(F.FastfError):
        sweep.sweep(cut, tmp_path / "outp", b, f, [1], [1])
    assert not (tmp_path / "outp" / "sweep.tsv").exists()
