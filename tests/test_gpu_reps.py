"""Replicate seeds of `fastF sweep` and `fastF cap` on the GPU (--seeds, --reps; fastf_sweep_reps, fastf_cap_reps): the per-gene
accumulation kernel (fastf_dev_gene_reps_add) against exact integers, and the commands — every <point>_s<seed> directory against
the oracle at that seed, every <verb>.tsv row against numpy, every <verb>_reps.tsv field against tests/reps_ref.py."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, cap, hostmem, sweep
from helpers import Case
from oracle import oracle as O
from sweep_ref import expected_row
import cap_ref
import reps_ref
from test_gpu_sweep import _case, _write
import test_gpu_markers as TM
import test_labels_host as LH

pytestmark = pytest.mark.gpu

SEEDS = [926, 927, 5]
RATES_C, RATES_R = [0.5, 1], [0, 0.1, 1]                                   # 2 x 3, with -c 1 and -r 0
GRID = ["-c", "0.5,1", "-r", "0,0.1,1"]
FILES = ("matrix.mtx.gz", "barcodes.tsv.gz", "features.tsv.gz")
GUARD = 0x5555555555555555


# ---- the kernel ----
@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    cells = np.arange(1, 101, dtype=np.uint64) | (np.uint64(1) << np.uint64(62))
    feats = np.arange(1, 51, dtype=np.uint64) | (np.uint64(2) << np.uint64(62))
    e = F.Engine(cells, feats, umi_max_bases=12)
    yield torch, e
    e.close()


@pytest.mark.parametrize("n_features", [1, 63, 64, 65, 36_601])
def test_gene_reps_add_against_exact_integers(eng, n_features):
    """three successive adds; a gene no replicate detects, a gene one of three detects, a cell count of 2^31 (its square needs 64
    bits); guard words behind all three accumulators and the untouched input"""
    torch, e = eng
    rng = np.random.default_rng(n_features)
    reps = [rng.integers(0, 50_000, size=n_features).astype(np.uint32) for _ in range(3)]
    never, once, big = n_features - 1, n_features // 2, 0
    for k, c in enumerate(reps):
        if n_features > 2:
            c[never] = 0
            c[once] = 7 if k == 1 else 0
        c[big] = 2 ** 31
    acc = torch.full((3 * (n_features + 2),), GUARD, dtype=torch.int64, device="cuda")       # [detected | 2 guards][sum | ..][sumsq | ..]
    ptr = [acc.data_ptr() + 8 * j * (n_features + 2) for j in range(3)]
    for j in range(3):
        acc[j * (n_features + 2): j * (n_features + 2) + n_features] = 0
    for c in reps:
        d_c = hostmem.to_device(np.concatenate([c, np.full(3, 0xFFFFFFFF, np.uint32)]), "cuda")      # (entries behind the array: not read)
        e.dev_gene_reps_add(d_c.data_ptr(), n_features, ptr[0], ptr[1], ptr[2])
        torch.cuda.synchronize()
        np.testing.assert_array_equal(hostmem.to_host(d_c).view(np.uint32)[:n_features], c)
    got = hostmem.to_host(acc).view(np.uint64).reshape(3, n_features + 2)
    want = reps_ref.gene_accumulate(reps)
    for j in range(3):
        assert [int(x) for x in got[j, :n_features]] == want[j], ("detected", "sum", "sumsq")[j]
        assert (got[j, n_features:] == np.uint64(GUARD)).all(), "words behind an accumulator were written"
    assert int(got[2, big]) == 3 * 2 ** 62 and int(got[0, big]) == 3
    if n_features > 2:
        assert [int(got[j, never]) for j in range(3)] == [0, 0, 0] and [int(got[j, once]) for j in range(3)] == [1, 7, 49]
    host = [np.zeros(n_features, np.uint64) for _ in range(3)]
    for c in reps:
        sweep.gene_reps_add_host(c, *host)
    for j in range(3):
        np.testing.assert_array_equal(host[j], got[j, :n_features])
    e.dev_gene_reps_add(0, 0, 0, 0, 0)                                    # no features: nothing to do
    with pytest.raises(F.FastfError):
        e.dev_gene_reps_add(0, n_features, ptr[0], ptr[1], ptr[2])


# ---- the commands ----
@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """the inputs of the edge and the mixed case, written once; the oracle's runs, computed once per (case, rates, seed)"""
    root = tmp_path_factory.mktemp("reps")
    cases, points = {}, {}
    for name in ("edge", "mixed"):
        d = root / name
        d.mkdir()
        case = _case(name)
        cases[name] = (case,) + _write(d, case)

    def oracle(name, rc, rd, seed):
        key = (name, rc, rd, seed)
        if key not in points:
            case, bam, _, _ = cases[name]
            points[key] = O.run_bam2db(case.bt, case.ft, case.flags, case.xf, case.cb, case.gx, case.ub, float(np.float32(rc)), float(np.float32(rd)),
                                       seed, str(bam).encode(), False)
        return points[key]
    return root, cases, oracle


def _gz(p):
    return gzip.decompress(open(p, "rb").read())


def _rows(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    return [ln.split("\t") for ln in lines[:-1]]


def _run(verb, bam, b, f, out, extra, env=None):
    r = subprocess.run([_lib.cli_path(), verb, "-b", str(bam), "-a", str(b), "-f", str(f), "-o", str(out)] + extra, capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, **(env or {})))
    return r


def _check_sweep_reps(out, work, name, seeds, summary_only=False, rates_c=RATES_C, rates_r=RATES_R):
    _, cases, oracle = work
    rows = _rows(out / "sweep.tsv")
    assert rows[0] == list(sweep.COLUMNS)
    rows = rows[1:]
    order = reps_ref.order(rates_c, seeds, rates_r)
    assert len(rows) == len(order)
    by_point = {}
    for row, (rc, seed, rd) in zip(rows, order):
        ora = oracle(name, rc, rd, seed)
        d = out / reps_ref.point_name(rc, rd, seed)
        assert sweep.reps_point_dir(sweep.point_dir(rc, rd), seed) == d.name
        if summary_only:
            assert not d.exists()
        else:
            assert _gz(d / "matrix.mtx.gz") == ora["matrix"], d
            assert _gz(d / "barcodes.tsv.gz") == ora["barcodes"], d
            assert _gz(d / "features.tsv.gz") == ora["features"], d
        assert row == expected_row(ora["matrix"], rc, rd, seed), (rc, seed, rd)
        by_point.setdefault((rc, rd), []).append(row)
        assert not (out / sweep.point_dir(rc, rd)).exists()                # no unsuffixed directory in a replicate run
    reps = _rows(out / "sweep_reps.tsv")
    assert reps[0] == list(sweep.REPS_COLUMNS) and len(reps) == 1 + len(rates_c) * len(rates_r)
    k = 1
    for rc in rates_c:
        for rd in rates_r:
            want = reps_ref.reps_row(["%.3f" % float(np.float32(rc)), "%.3f" % float(np.float32(rd))], by_point[(rc, rd)])
            reps_ref.assert_reps_row(reps[k], want, (rc, rd))
            assert reps[k][2] == str(len(seeds))
            if rd == 0:
                assert reps[k][4:8] == ["0.000000", "0.000000" if len(seeds) > 1 else "NA", "0", "0"]
            k += 1
    assert not [n for n in os.listdir(out) if n.endswith(".partial")]
    return reps


@pytest.mark.parametrize("name", ["edge", "mixed"])
def test_cli_sweep_seeds_equals_bam2db_at_every_seed(work, tmp_path, name):
    _, cases, oracle = work
    case, bam, b, f = cases[name]
    out = tmp_path / "out"
    r = _run("sweep", bam, b, f, out, GRID + ["--seeds", "926,927,5"])
    assert r.returncode == 0, r.stderr
    assert "point by point" not in r.stderr and "x 3 seeds" in r.stdout and "sweep_reps.tsv is generated" in r.stdout
    reps = _check_sweep_reps(out, work, name, SEEDS)
    assert sorted(os.listdir(out)) == sorted(["sweep.tsv", "sweep_reps.tsv"] + [reps_ref.point_name(rc, rd, s) for rc, s, rd in reps_ref.order(RATES_C, SEEDS, RATES_R)])
    if name == "mixed":
        # the subsamples differ: some spread at the sparse point, and the seeds are what a plain run at that seed gives
        sparse = [x for x in reps if x[:2] == ["0.500", "0.100"]][0]
        assert float(sparse[5]) > 0 and sparse[6] != sparse[7]
        # a plain run beside it: the unsuffixed outputs are what they were
        out1 = tmp_path / "plain"
        r = _run("sweep", bam, b, f, out1, GRID + ["-s", "926"])
        assert r.returncode == 0, r.stderr
        assert "seeds" not in r.stdout
        assert sorted(os.listdir(out1)) == sorted(["sweep.tsv"] + [sweep.point_dir(rc, rd) for rc in RATES_C for rd in RATES_R])
        plain = _rows(out1 / "sweep.tsv")
        k = 1
        for rc in RATES_C:
            for rd in RATES_R:
                ora = oracle(name, rc, rd, 926)
                for fn, key in zip(FILES, ("matrix", "barcodes", "features")):
                    assert _gz(out1 / sweep.point_dir(rc, rd) / fn) == ora[key]
                    assert open(out1 / sweep.point_dir(rc, rd) / fn, "rb").read() == open(out / reps_ref.point_name(rc, rd, 926) / fn, "rb").read()
                assert plain[k] == expected_row(ora["matrix"], rc, rd, 926)
                k += 1


def test_reps_one_writes_the_files_of_the_plain_run_under_suffixed_names(work, tmp_path):
    _, cases, _ = work
    case, bam, b, f = cases["mixed"]
    out = tmp_path / "out"
    r = _run("sweep", bam, b, f, out, GRID + ["--reps", "1"])
    assert r.returncode == 0, r.stderr
    reps = _check_sweep_reps(out, work, "mixed", [926])
    for row in reps[1:]:
        assert row[2] == "1" and row[5::4] == ["NA"] * 7 and row[4::4] != ["NA"] * 7
        assert row[6] == row[7] and float(row[4]) == float(row[6])        # one value: mean = min = max
    # the seeds of --reps 2 from -s 926, in process
    out3 = tmp_path / "out3"
    rows = sweep.sweep_reps(bam, out3, b, f, [0.5], [0.1], sweep.reps_seeds(926, 2), summary_only=True)
    assert [x["seed"] for x in rows] == ["926", "927"]
    _check_sweep_reps(out3, work, "mixed", [926, 927], summary_only=True, rates_c=[0.5], rates_r=[0.1])


def test_summary_only_and_buffer_reuse_give_the_same_tables(work, tmp_path):
    """--summary-only: the two tables alone; FASTF_RES_NO_REUSE=1 (fresh buffers and a fresh blocked copy for every pair) and one
    env-forced general path (no streaming K1b: SoA records) give the same bytes; FASTF_RES_NO_REUSE=1 against buffer reuse again with
    every option of sweep, cap and level on"""
    _, cases, _ = work
    case, bam, b, f = cases["mixed"]
    out = tmp_path / "out"
    r = _run("sweep", bam, b, f, out, GRID + ["--seeds=926,927,5", "--summary-only"], env={"FASTF_PROFILE": "1"})
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(out)) == ["sweep.tsv", "sweep_reps.tsv"]
    _check_sweep_reps(out, work, "mixed", SEEDS, summary_only=True)
    assert "6 (cell rate, seed) pairs" in r.stderr and "laid out 1 times" in r.stderr      # (one layout serves both cell rates and every seed)
    for k, env in enumerate(({"FASTF_RES_NO_REUSE": "1", "FASTF_PROFILE": "1"}, {"FASTF_NO_STREAM_K1B": "1"}, {"FASTF_BLOCK_WIDE": "1"})):
        o = tmp_path / ("env%d" % k)
        r2 = _run("sweep", bam, b, f, o, GRID + ["--seeds=926,927,5", "--summary-only"], env=env)
        assert r2.returncode == 0, r2.stderr
        for t in ("sweep.tsv", "sweep_reps.tsv"):
            assert open(o / t).read() == open(out / t).read(), (env, t)
        if k == 0:
            assert "laid out 6 times" in r2.stderr
    # every comparison on, all three verbs, two seeds, the cell rates ascending: the buffers the first pair leaves serve the larger
    # pairs behind it, the carved blocks by the capacity they were allocated for — the same trees and the same stdout as with fresh
    # buffers for every pair (each run in a directory of its own, under the same relative -o)
    lcase = LH.labcase()
    for verb in ("sweep", "cap", "level"):
        got = []
        for k, env in enumerate(({}, {"FASTF_RES_NO_REUSE": "1"})):
            d = tmp_path / ("%s%d" % (verb, k))
            d.mkdir()
            lbam, lb, lfeat, labels = TM._write(d, lcase)
            r3 = subprocess.run(TM._args(verb, "in.bam", lb.name, lfeat.name, "out", [0.5, 1], TM.GRID[verb]) +
                                ["--seeds", "926,5", "--genes", "--cells", "--fidelity", "--gene-fidelity", "--neighbors", "--labels", labels.name, "--markers", "5"],
                                capture_output=True, text=True, timeout=600, cwd=d, env=dict(os.environ, **env))
            assert r3.returncode == 0, r3.stderr
            got.append((TM._tree(d / "out"), r3.stdout))
        assert sorted(got[0][0]) == sorted(got[1][0]) and len(got[0][0]) >= 8 * 11, verb      # (8 points, 11 files each at the least)
        assert got[0] == got[1], verb


def test_cap_seeds_against_the_masked_oracle_per_seed(work, tmp_path):
    _, cases, _ = work
    case, bam, b, f = cases["mixed"]
    rates, caps, seeds = [0.5, 1], [5, 1_000_000], [926, 5]
    out = tmp_path / "out"
    r = _run("cap", bam, b, f, out, ["-c", "0.5,1", "-n", "5,1000000", "--seeds", "926,5"])
    assert r.returncode == 0, r.stderr
    rows = _rows(out / "cap.tsv")
    assert rows[0] == list(cap.COLUMNS)
    by_point = {}
    for row, (rc, seed, n) in zip(rows[1:], reps_ref.order(rates, seeds, caps)):
        ref = cap_ref.point(case, str(bam).encode(), rc, n, seed)
        d = out / reps_ref.point_name(rc, n, seed, caps=True)
        for fn, key in zip(FILES, ("matrix", "barcodes", "features")):
            assert _gz(d / fn) == ref[key], d
        assert row == ref["row"], (rc, seed, n)
        by_point.setdefault((rc, n), []).append(row)
    assert len(rows) == 1 + 8
    reps = _rows(out / "cap_reps.tsv")
    assert reps[0] == list(cap.REPS_COLUMNS) and len(reps) == 5
    k = 1
    for rc in rates:
        for n in caps:
            reps_ref.assert_reps_row(reps[k], reps_ref.reps_row(["%.3f" % rc, str(n)], by_point[(rc, n)]), (rc, n))
            k += 1
    # in process, one seed, --summary-only: the same rows of that seed
    out2 = tmp_path / "out2"
    rows2 = cap.cap_reps(bam, out2, b, f, rates, caps, [5], summary_only=True)
    assert [list(x.values()) for x in rows2] == [x for x in rows[1:] if x[2] == "5"]
    assert sorted(os.listdir(out2)) == ["cap.tsv", "cap_reps.tsv"] and all(x["n_reps"] == "1" for x in cap.read_reps_table(out2 / "cap_reps.tsv"))


@pytest.mark.parametrize("verb", ["sweep", "cap"])
def test_genes_and_cells_of_a_replicate_run(work, tmp_path, verb):
    _, cases, _ = work
    case, bam, b, f = cases["mixed"]
    out, plain = tmp_path / "out", tmp_path / "plain"
    own = ["-c", "0.5,1", "-r", "0.1,1"] if verb == "sweep" else ["-c", "0.5,1", "-n", "5,40"]
    second = [0.1, 1] if verb == "sweep" else [5, 40]
    r = _run(verb, bam, b, f, out, own + ["--seeds", "926,927,5", "--genes", "--cells"])
    assert r.returncode == 0, r.stderr
    r1 = _run(verb, bam, b, f, plain, own + ["-s", "927", "--genes", "--cells"])
    assert r1.returncode == 0, r1.stderr
    names = [reps_ref.point_name(rc, x, s, caps=verb == "cap") for rc, s, x in reps_ref.order([0.5, 1], SEEDS, second)]
    top = ["%s.tsv" % verb, "%s_reps.tsv" % verb, "%s_genes.tsv" % verb, "%s_cells.tsv" % verb, "%s_genes_reps.tsv" % verb, "%s_gene_reps.tsv.gz" % verb]
    assert sorted(os.listdir(out)) == sorted(top + names)                 # no <verb>_gene_cells.tsv.gz
    assert "%s_gene_cells.tsv.gz" % verb in os.listdir(plain)
    # one row per (point, seed) in the order of <verb>.tsv, the seed in the third column; at seed 927 the rows of the plain run
    main, genes, cells = _rows(out / ("%s.tsv" % verb)), _rows(out / ("%s_genes.tsv" % verb)), _rows(out / ("%s_cells.tsv" % verb))
    assert len(main) == len(genes) == len(cells) == 13 and cells[0][2] == genes[0][2] == "seed"
    for t in (genes, cells):
        assert [x[:3] for x in t[1:]] == [x[:3] for x in main[1:]]
        assert [x for x in t[1:] if x[2] == "927"] == _rows(plain / ("%s_%s.tsv" % (verb, "genes" if t is genes else "cells")))[1:]
    assert [x[2] for x in cells[1:]] == [str(s) for _ in (0.5, 1) for s in SEEDS for _ in second]
    # the point files of seed 927 are the plain run's
    for n in names:
        assert sorted(os.listdir(out / n)) == sorted(FILES + ("genes.tsv.gz", "cells.tsv.gz"))
        if n.endswith("_s927"):
            for fn in ("genes.tsv.gz", "cells.tsv.gz", "matrix.mtx.gz"):
                assert _gz(out / n / fn) == _gz(plain / n[:-5] / fn), (n, fn)
    # the three columns per grid point against the accumulation of the per-seed genes.tsv.gz files
    table = [ln.split("\t") for ln in _gz(out / ("%s_gene_reps.tsv.gz" % verb)).decode().split("\n")[:-1]]
    greps = _rows(out / ("%s_genes_reps.tsv" % verb))
    assert greps[0] == list((sweep if verb == "sweep" else cap).GENES_REPS_COLUMNS) and len(greps) == 5
    feats = [ln.split("\t")[0] for ln in case.ft.decode().split("\n") if ln]
    assert [x[0] for x in table[1:]] == feats
    p = 0
    for rc in (0.5, 1):
        for x in second:
            base = (cap.point_dir(rc, x) if verb == "cap" else sweep.point_dir(rc, x))
            assert table[0][1 + 3 * p: 4 + 3 * p] == [base + ":reps_detected", base + ":cells_sum", base + ":cells_sumsq"]
            per_seed = []
            for s in SEEDS:
                g = [ln.split("\t") for ln in _gz(out / ("%s_s%d" % (base, s)) / "genes.tsv.gz").decode().split("\n")[:-1]]
                assert [y[0] for y in g] == feats
                per_seed.append([int(y[1]) for y in g])
            det, tot, sq = reps_ref.gene_accumulate(per_seed)
            assert [int(y[1 + 3 * p]) for y in table[1:]] == det and [int(y[2 + 3 * p]) for y in table[1:]] == tot
            assert [int(y[3 + 3 * p]) for y in table[1:]] == sq
            row = greps[1 + p]
            want = reps_ref.genes_reps_row(["%.3f" % rc, ("%d" % x) if verb == "cap" else "%.3f" % x], per_seed)
            reps_ref.assert_reps_row(row, want, (rc, x), lead=3)
            assert int(row[7]) <= int(row[5]) and int(row[8]) >= int(row[6])  # in all reps <= min, in any rep >= max
            assert [str(d) for d in (sum(1 for c in ps if c >= 1) for ps in per_seed)] == [y[3] for y in genes[1:] if y[0] == row[0] and y[1] == row[1]]
            p += 1
    assert len(table[0]) == 1 + 3 * p


def test_wide_jobs_run_point_by_point_and_seed_by_seed(tmp_path):
    """20-base UMIs do not fit a 64-bit key: every (point, seed) goes through bam2db() into the same names, the host twins fill the
    tables; --cells and cap refuse such a job as they do without replicates"""
    case = Case(n=30_000, n_bar=400, n_gene=150, umi_len=20, umi_pool=512, p_n_umi=0.02, p_bad_xf=0.1, data_seed=35)
    bam, b, f = _write(tmp_path, case)
    out = tmp_path / "out"
    r = _run("sweep", bam, b, f, out, ["-c", "0.5,1", "-r", "0.5", "--seeds", "926,5", "--genes"])
    assert r.returncode == 0, r.stderr
    assert "point by point" in r.stderr
    rows = _rows(out / "sweep.tsv")[1:]
    by_point, cells_by_point = {}, {}
    for row, (rc, seed, rd) in zip(rows, reps_ref.order([0.5, 1], [926, 5], [0.5])):
        ora = O.run_bam2db(case.bt, case.ft, case.flags, case.xf, case.cb, case.gx, case.ub, rc, rd, seed, str(bam).encode(), False)
        d = out / reps_ref.point_name(rc, rd, seed)
        assert _gz(d / "matrix.mtx.gz") == ora["matrix"] and _gz(d / "barcodes.tsv.gz") == ora["barcodes"]
        assert row == expected_row(ora["matrix"], rc, rd, seed)
        by_point.setdefault(rc, []).append(row)
        cells_by_point.setdefault(rc, []).append([int(ln.split("\t")[1]) for ln in _gz(d / "genes.tsv.gz").decode().split("\n")[:-1]])
    assert len(rows) == 4
    reps, greps = _rows(out / "sweep_reps.tsv"), _rows(out / "sweep_genes_reps.tsv")
    table = [ln.split("\t") for ln in _gz(out / "sweep_gene_reps.tsv.gz").decode().split("\n")[:-1]]
    for p, rc in enumerate((0.5, 1)):
        reps_ref.assert_reps_row(reps[1 + p], reps_ref.reps_row(["%.3f" % rc, "0.500"], by_point[rc]), rc)
        reps_ref.assert_reps_row(greps[1 + p], reps_ref.genes_reps_row(["%.3f" % rc, "0.500"], cells_by_point[rc]), rc, lead=3)
        det, tot, sq = reps_ref.gene_accumulate(cells_by_point[rc])
        assert [[int(y[1 + 3 * p]), int(y[2 + 3 * p]), int(y[3 + 3 * p])] for y in table[1:]] == [list(t) for t in zip(det, tot, sq)]
    assert not (out / "sweep_gene_cells.tsv.gz").exists()
    for k, (verb, extra) in enumerate((("sweep", ["-r", "0.5", "--cells"]), ("cap", ["-n", "5"]))):
        o = tmp_path / ("refused%d" % k)
        r = _run(verb, bam, b, f, o, ["-c", "1", "--seeds", "926,5"] + extra)
        assert r.returncode == 1 and "resident form" in r.stderr and "outside" in r.stderr, r.stderr
        assert not [n for n in os.listdir(o) if n.endswith(".tsv") or n.endswith(".partial")]


def test_a_failing_run_leaves_no_table(work, tmp_path):
    _, cases, _ = work
    case, bam, b, f = cases["mixed"]
    cut = tmp_path / "cut.bam"
    data = open(bam, "rb").read()
    cut.write_bytes(data[:len(data) * 2 // 3])
    for k, verb in enumerate(("sweep", "cap")):
        out = tmp_path / ("out%d" % k)
        own = ["-r", "0.5"] if verb == "sweep" else ["-n", "5"]
        r = _run(verb, cut, b, f, out, own + ["--seeds", "926,927", "--genes", "--cells"])
        assert r.returncode == 1 and "truncated" in r.stderr.lower(), r.stderr
        assert [n for n in os.listdir(out) if ".tsv" in n or n.endswith(".partial")] == []
    with pytest.raises(F.FastfError):
        sweep.sweep_reps(cut, tmp_path / "outp", b, f, [1], [1], [1, 2], genes=True)
    assert [n for n in os.listdir(tmp_path / "outp") if ".tsv" in n] == []
