"""--fidelity on the GPU: the join (fastf_dev_fidelity) on hand-built rows against fidelity_ref, and sweep, cap and level with the flag —
through the CLI and in process — every fidelity.tsv.gz and <verb>_fidelity.tsv row against the reference built on the unchanged
oracle: integer columns exactly, float columns within 1.5e-6 absolute."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, cap, hostmem, level, sweep
from helpers import Case
from oracle import oracle as O
import cap_ref
import fidelity_ref as R
import level_ref
from sweep_ref import parse_matrix
from test_gpu_sweep import _Edge, _write
from test_fidelity_host import nested_pair

pytestmark = pytest.mark.gpu

GUARD64 = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    cells = np.arange(1, 101, dtype=np.uint64) | (np.uint64(1) << np.uint64(62))
    feats = np.arange(1, 51, dtype=np.uint64) | (np.uint64(2) << np.uint64(62))
    e = F.Engine(cells, feats, umi_max_bases=12)
    yield e
    e.close()


def _waves():
    import torch
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count * 4      # FID_BLOCKS_PER_CU workgroups a CU, four waves each


def _dev_rows(rows, pad_key):
    """(feature, cell, count) on the device, 300 rows behind them that must not be read: their key is pad_key, their count 7"""
    f, c, k = (np.asarray(a, np.uint32) for a in rows)
    pad = 300
    return [hostmem.to_device(np.concatenate([a, np.full(pad, v, np.uint32)]), "cuda") for a, v in ((f, pad_key[1]), (c, pad_key[0]), (k, 7))]


def _run(eng, full, point, n_cells, expect_error=False):
    import torch
    n, m = len(point[0]), len(full[0])
    xd = _dev_rows(full, (1, 1))                            # behind the full rows: (cell 1, feature 1) again and again
    yd = _dev_rows(point, (n_cells + 5, 9))                 # behind the point rows: rows of a cell nobody has
    d_m, d_n = hostmem.to_device(np.array([m], np.uint64), "cuda"), hostmem.to_device(np.array([n], np.uint64), "cuda")
    d_xy = torch.full((n_cells + 2,), -1, dtype=torch.int64, device="cuda")
    d_yy = torch.full((n_cells + 2,), -1, dtype=torch.int64, device="cuda")
    d_err = hostmem.to_device(np.array([0, 0xFFFFFFFFFFFFFFFF], np.uint64), "cuda")
    call = lambda: eng.dev_fidelity(xd[0].data_ptr(), xd[1].data_ptr(), xd[2].data_ptr(), d_m.data_ptr(), yd[0].data_ptr(), yd[1].data_ptr(),  # noqa: E731
                                    yd[2].data_ptr(), d_n.data_ptr(), n_cells, d_xy.data_ptr(), d_yy.data_ptr(), d_err.data_ptr())
    if expect_error:
        with pytest.raises(F.FastfError, match="no partner"):
            call()
    else:
        call()
    torch.cuda.synchronize()
    xy, yy, err = (hostmem.to_host(t).view(np.uint64) for t in (d_xy, d_yy, d_err))
    assert (xy[n_cells:] == GUARD64).all() and (yy[n_cells:] == GUARD64).all() and err[1] == GUARD64, "words behind an array were written"
    assert int(err[0]) == (32 if expect_error else 0)
    return xy[:n_cells], yy[:n_cells]


def _check(eng, full, point, n_cells):
    mom = R.moments(full, point, n_cells)
    xy, yy = _run(eng, full, point, n_cells)
    assert [int(v) for v in xy] == mom["sum_xy"] and [int(v) for v in yy] == mom["sum_yy"]
    return mom


def _sorted_rows(rng, n_rows, n_cells, n_features=4000):
    """n_rows distinct (cell, feature) pairs ascending, counts 0 .. 50 with zeros among them"""
    keys = np.unique(rng.integers(0, n_cells * n_features, size=int(n_rows * 1.3) + 16))
    while len(keys) < n_rows:
        keys = np.unique(np.concatenate([keys, rng.integers(0, n_cells * n_features, size=n_rows)]))
    keys = np.sort(rng.choice(keys, size=n_rows, replace=False))
    count = rng.integers(0, 51, size=n_rows)
    return (keys % n_features + 1, keys // n_features + 1, count)


def _subset(rng, full, keep):
    sel = rng.random(len(full[0])) < keep if not isinstance(keep, np.ndarray) else keep
    y = np.minimum(full[2][sel], rng.integers(0, 51, size=int(sel.sum())))
    return (full[0][sel], full[1][sel], y)


def _row_counts():
    w = 64 * _waves()                                       # up to here every wave's span is 64 rows, one turn; behind it 128, two turns
    return [0, 1, 63, 64, 65, 255, 256, 257, w - 1, w, w + 1]


@pytest.mark.parametrize("which", range(11))
def test_the_join_at_the_sizes_where_the_path_changes(eng, which):
    """the point has exactly n rows (0, 1, around a wave's turn of 64, around a workgroup's four turns, around the row count at which
    the spans grow from one turn to two) out of a full matrix three times as large"""
    n = _row_counts()[which]
    rng = np.random.default_rng(1000 + which)
    n_cells = 700
    full = _sorted_rows(rng, 3 * n + 5, n_cells)
    sel = np.zeros(len(full[0]), bool)
    sel[rng.choice(len(sel), size=n, replace=False)] = True
    point = _subset(rng, full, sel)
    assert len(point[0]) == n
    mom = _check(eng, full, point, n_cells)
    assert n < 64 or (0 in point[2] and 0 in full[2])       # zero-count rows on both sides
    xx, xx2 = _run(eng, full, full, n_cells)                # the full rows with themselves: sum_xx
    assert [int(v) for v in xx] == mom["sum_xx"] and (xx == xx2).all()


def test_point_equals_full_and_single_rows(eng):
    rng = np.random.default_rng(5)
    n_cells = 90
    full = _sorted_rows(rng, 20_000, n_cells, n_features=900)
    _check(eng, full, full, n_cells)
    first = tuple(a[:1] for a in full)
    last = tuple(a[-1:] for a in full)
    for point in (first, last):
        point[2][0] = 3
        _check(eng, full, point, n_cells)
    _check(eng, full, tuple(a[:0] for a in full), n_cells)
    _check(eng, tuple(a[:0] for a in full), tuple(a[:0] for a in full), n_cells)


def test_one_cell_owning_every_row_over_several_spans(eng):
    rng = np.random.default_rng(6)
    n = 64 * _waves() * 2 + 777                             # spans of three turns; every span's cell reaches into both neighbours
    feature = np.arange(1, n + 1)
    full = (feature, np.full(n, 4), rng.integers(0, 20, size=n))
    point = _subset(rng, full, 0.7)
    mom = _check(eng, full, point, 10)
    assert mom["sum_xy"][3] > 0 and sum(mom["sum_xy"]) == mom["sum_xy"][3]
    _check(eng, full, point, 4)                             # the cell is the last the arrays have room for


def test_one_cell_only_and_big_counts(eng):
    full = (np.array([1, 2, 9]), np.array([1, 1, 1]), np.array([4_000_000_000, 5, 0]))
    point = (np.array([1, 9]), np.array([1, 1]), np.array([4_000_000_000, 0]))
    mom = _check(eng, full, point, 1)
    assert mom["sum_xy"] == [16 * 10 ** 18]


def test_70000_sparse_cells(eng):
    rng = np.random.default_rng(7)
    n_cells = 70_000
    full = _sorted_rows(rng, 150_000, n_cells, n_features=300)
    point = _subset(rng, full, 0.5)
    assert point[1].max() > 65_535 and len(np.unique(point[1])) < n_cells
    _check(eng, full, point, n_cells)


def test_a_window_of_full_rows_much_larger_than_the_span(eng):
    rng = np.random.default_rng(8)
    n_cells = 500
    full = _sorted_rows(rng, 400_000, n_cells, n_features=3000)
    sel = np.zeros(len(full[0]), bool)
    sel[::50] = True                                        # every 50th full row kept
    _check(eng, full, _subset(rng, full, sel), n_cells)


def test_a_missing_partner_is_reported_and_leaves_the_other_cells_right(eng):
    rng = np.random.default_rng(9)
    n_cells = 300
    full = _sorted_rows(rng, 30_000, n_cells, n_features=600)
    point = _subset(rng, full, 0.5)
    mom = R.moments(full, point, n_cells)
    for where in (0, len(point[0]) // 2, len(point[0]) - 1):
        bad_cell = int(point[1][where])
        gone = (full[1] == point[1][where]) & (full[0] == point[0][where])
        broken = tuple(a[~gone] for a in full)              # that row's partner leaves the full rows
        xy, yy = _run(eng, broken, point, n_cells, expect_error=True)
        ok = np.arange(1, n_cells + 1) != bad_cell
        assert [int(v) for v in xy[ok]] == [v for v, o in zip(mom["sum_xy"], ok) if o]
        assert [int(v) for v in yy] == mom["sum_yy"]
    with pytest.raises(F.FastfError):                       # the host twin says the same
        sweep.fidelity_from_coo(broken, point, n_cells)
    xy, yy = _run(eng, tuple(a[:0] for a in full), point, n_cells, expect_error=True)      # no full rows at all
    assert not xy.any() and [int(v) for v in yy] == mom["sum_yy"]


# ---- the commands ----
MIXED = dict(n=200_000, n_bar=600, n_gene=500, umi_len=12, dup_factor=3.0, p_no_cb=0.05, p_unlisted_cb=0.05, p_bad_xf=0.15, p_n_umi=0.01,
             p_multi_gene=0.02)
_CASES, _POINTS = {}, {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = _Edge() if name == "edge" else Case(**MIXED)
    return _CASES[name]


def _rows_of(matrix):
    _, _, _, f, c, k = parse_matrix(matrix)
    return f, c, k


def _point(name, verb, rc, value, seed=926):
    """the reference of one point: (the fields of its fidelity.tsv.gz rows, the fields of its table row)"""
    key = (name, verb, float(rc), float(value), seed)
    if key not in _POINTS:
        case = _case(name)
        full, n_cells, names, G, hits = R.full_matrix(name, case, rc, seed)
        if verb == "sweep":
            ora = O.run_bam2db(case.bt, case.ft, case.flags, case.xf, case.cb, case.gx, case.ub, float(np.float32(rc)), float(np.float32(value)), seed, b"x.bam", False)
            rows, lead = _rows_of(ora["matrix"]), ["%.3f" % rc, "%.3f" % value]
        elif verb == "cap":
            rows, lead = _rows_of(cap_ref.point(case, b"x.bam", rc, value, seed)["matrix"]), ["%.3f" % rc, str(int(value))]
        else:
            rows, lead = _rows_of(level_ref.point(hits, value)["matrix"]), ["%.3f" % rc, str(int(value))]
        mom = R.moments(full, rows, n_cells)
        _POINTS[key] = (R.cell_rows(names, mom, G), R.summary_fields(lead, seed, mom, G))
    return _POINTS[key]


def _grid(name, verb):
    if name == "edge":
        return [1], {"sweep": [0, 0.5, 1], "cap": [1, 2], "level": [1, 2]}[verb]
    if verb == "sweep":
        return [0.5, 1], [0.1, 1]
    hits = R.full_matrix("mixed", _case("mixed"), 0.5, 926)[4]
    if verb == "cap":
        return [0.5], [int(np.percentile(hits.h, 20)), int(hits.h.max())]
    return [0.5], [int(np.percentile(hits.u_full, 10)), int(hits.u_full.max())]


MOD = {"sweep": sweep, "cap": cap, "level": level}
OPT = {"sweep": "-r", "cap": "-n", "level": "-m"}


def _gz(p):
    return gzip.decompress(open(p, "rb").read())


def _check_outputs(out, name, verb, rates, values, seeds=(926,), reps=False, summary_only=False):
    lines = open(out / ("%s_fidelity.tsv" % verb)).read().split("\n")
    assert lines[0].split("\t") == list(MOD[verb].FIDELITY_COLUMNS) and lines[-1] == ""
    assert len(lines) - 2 == len(rates) * len(values) * len(seeds)
    k = 1
    for rc in rates:
        for seed in seeds:
            for v in values:
                cells, row = _point(name, verb, rc, v, seed)
                R.assert_fields(lines[k].split("\t"), row, 5, (verb, rc, seed, v))
                k += 1
                d = out / (MOD[verb].point_dir(rc, v) + ("_s%d" % seed if reps else ""))
                if summary_only:
                    assert not d.exists()
                    continue
                got = _gz(d / "fidelity.tsv.gz").decode().split("\n")
                assert got[0].split("\t") == list(sweep.POINT_FIDELITY_COLUMNS) and got[-1] == "" and len(got) - 2 == len(cells)
                for g, w in zip(got[1:-1], cells):
                    R.assert_fields(g.split("\t"), w, 8, (verb, rc, seed, v))
                assert sweep.read_point_fidelity(d / "fidelity.tsv.gz")[0]["barcode"] == cells[0][0]
    assert not [n for n in os.listdir(out) if n.endswith(".partial")]


def _args(verb, bam, b, f, out, rates, values):
    return [_lib.cli_path(), verb, "-b", str(bam), "-a", str(b), "-f", str(f), "-o", str(out), "-c", ",".join("%g" % r for r in rates),
            OPT[verb], ",".join(str(v) for v in values)]


def _tree(root):
    out = {}
    for dirpath, _, files in os.walk(root):
        for fn in files:
            p = os.path.join(dirpath, fn)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


@pytest.mark.parametrize("name", ["edge", "mixed"])
@pytest.mark.parametrize("verb", ["sweep", "cap", "level"])
def test_cli_with_the_flag_and_the_same_tree_without_it(tmp_path, verb, name):
    bam, b, f = _write(tmp_path, _case(name))
    rates, values = _grid(name, verb)
    out, out0 = tmp_path / "out", tmp_path / "out0"
    r = subprocess.run(_args(verb, bam, b, f, out, rates, values) + ["--fidelity"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, FASTF_PROFILE="1"))
    assert r.returncode == 0, r.stderr
    assert "%s_fidelity.tsv is generated." % verb in r.stdout and "[%s] --fidelity:" % verb in r.stderr
    _check_outputs(out, name, verb, rates, values)
    r = subprocess.run(_args(verb, bam, b, f, out0, rates, values), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    with_flag, without = _tree(out), _tree(out0)
    new = {n for n in with_flag if n == "%s_fidelity.tsv" % verb or os.path.basename(n) == "fidelity.tsv.gz"}
    assert len(new) == 1 + len(rates) * len(values) and not [n for n in without if "fidelity" in n]
    assert {n: v for n, v in with_flag.items() if n not in new} == without


@pytest.mark.parametrize("name", ["edge", "mixed"])
@pytest.mark.parametrize("verb", ["sweep", "cap", "level"])
def test_in_process(tmp_path, verb, name):
    bam, b, f = _write(tmp_path, _case(name))
    rates, values = _grid(name, verb)
    out = tmp_path / "out"
    MOD[verb].__dict__[verb](bam, out, b, f, rates, values, seed=926, fidelity=True)
    _check_outputs(out, name, verb, rates, values)
    rows = MOD[verb].read_fidelity_table(out / ("%s_fidelity.tsv" % verb))
    assert len(rows) == len(rates) * len(values) and rows[0]["seed"] == "926"
    if name == "mixed":                                     # the deepest point of the grid is the full matrix itself
        last = rows[-1]
        assert last["median_pearson"] == "1.000000" and last["p10_pearson"] == "1.000000" and last["umis_kept"] == "1.000000"
        assert float(rows[0]["median_pearson"]) < 1 and float(rows[0]["umis_kept"]) < 1
    out2 = tmp_path / "out2"
    MOD[verb].__dict__[verb](bam, out2, b, f, rates, values, seed=926, fidelity=True, summary_only=True)
    _check_outputs(out2, name, verb, rates, values, summary_only=True)
    assert sorted(os.listdir(out2)) == sorted(["%s.tsv" % verb, "%s_fidelity.tsv" % verb])
    assert open(out2 / ("%s_fidelity.tsv" % verb)).read() == open(out / ("%s_fidelity.tsv" % verb)).read()


@pytest.mark.parametrize("verb", ["sweep", "cap", "level"])
def test_with_cells_and_genes_together(tmp_path, verb):
    """--cells' K3u writes the row buffer the join reads: the join runs first, and every file of the other flags stays what it is"""
    bam, b, f = _write(tmp_path, _case("mixed"))
    rates, values = _grid("mixed", verb)
    out, out0 = tmp_path / "out", tmp_path / "out0"
    for o, extra in ((out, ["--fidelity"]), (out0, [])):
        r = subprocess.run(_args(verb, bam, b, f, o, rates, values) + ["--cells", "--genes"] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
    _check_outputs(out, "mixed", verb, rates, values)
    with_flag, without = _tree(out), _tree(out0)
    assert {n: v for n, v in with_flag.items() if "fidelity" not in n} == without and len(with_flag) == len(without) + 1 + len(rates) * len(values)
    assert any(n.endswith("cells.tsv.gz") for n in without) and any(n.endswith("genes.tsv.gz") for n in without)


def test_two_seeds_give_one_row_per_cell_rate_seed_and_value(tmp_path):
    bam, b, f = _write(tmp_path, _case("mixed"))
    out = tmp_path / "out"
    r = subprocess.run(_args("sweep", bam, b, f, out, [0.5], [0.1, 1]) + ["--fidelity", "--seeds", "926,5"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    _check_outputs(out, "mixed", "sweep", [0.5], [0.1, 1], seeds=(926, 5), reps=True)
    rows = sweep.read_fidelity_table(out / "sweep_fidelity.tsv")
    assert [x["seed"] for x in rows] == ["926", "926", "5", "5"] and rows[0] != rows[2]
    out2 = tmp_path / "out2"
    cap.cap_reps(bam, out2, b, f, [0.5], _grid("mixed", "cap")[1][:1], [926], fidelity=True, summary_only=True)
    _check_outputs(out2, "mixed", "cap", [0.5], _grid("mixed", "cap")[1][:1], seeds=(926,), reps=True, summary_only=True)


def test_refusal_of_20_base_umis_leaves_no_table(tmp_path):
    """20-base UMIs do not fit a 64-bit key: the full rows live on the device alone, so sweep does not fall back with the flag"""
    case = Case(n=30_000, n_bar=400, n_gene=150, umi_len=20, umi_pool=512, p_n_umi=0.02, p_bad_xf=0.1, data_seed=35)
    bam, b, f = _write(tmp_path, case)
    for verb, v in (("sweep", [0.5]), ("cap", [5]), ("level", [5])):
        out = tmp_path / ("out_" + verb)
        r = subprocess.run(_args(verb, bam, b, f, out, [1], v) + ["--fidelity"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 1 and "outside" in r.stderr and "point by point" not in r.stderr.replace("no point-by-point", ""), r.stderr
        assert [n for n in os.listdir(out) if n.startswith(verb)] == []
    with pytest.raises(F.FastfError, match="--fidelity needs the resident form"):
        sweep.sweep(bam, tmp_path / "outp", b, f, [1], [1], fidelity=True)
    assert not (tmp_path / "outp" / "sweep.tsv").exists()
