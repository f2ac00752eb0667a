"""--coexpression on sweep, cap and level, through the CLI and in process: every row of coexpr.tsv.gz and <verb>_coexpr.tsv against a
reference built from the unchanged oracle's matrices — sweep.hvg_rank on the full rows, sweep.coexpression_from_coo (the host twin) on
the full rows and on the point's, coexpr_ref.per_gene and summary_fields: integer columns exactly, mean_kept within half a unit of its
last printed digit.  Alone, with --neighbors --fidelity, with two seeds, with --summary-only; without the flag the tree is what it was."""
import gzip
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, cap, level, sweep
from oracle import oracle as O
import cap_ref
import coexpr_ref as R
import level_ref
import neighbors_ref as N
from test_gpu_sweep import _write
import test_gpu_gene_fidelity as TG

pytestmark = pytest.mark.gpu

MOD, K = TG.MOD, sweep.COEXPRESSION_K
_POINTS, _PAIRS = {}, {}


def _sets(rows, n_cells, A, nf):
    idx, cnt, _, _ = sweep.coexpression_from_coo(rows, n_cells, R.slot_map([int(g) for g in A], nf), len(A), K)
    return [[int(v) for v in idx[g, :cnt[g]]] for g in range(len(A))]


def _pair(name, rc, seed):
    key = (name, float(rc), seed)
    if key not in _PAIRS:
        case = TG._case(name)
        full, n_cells, _, nf, hits = N.full_matrix(name, case, rc, seed)
        ids = [ln.split("\t")[0] for ln in hits.ora_full["features"].decode().split("\n")[:-1]]
        assert len(ids) == nf
        sx, sxx = np.zeros(nf, np.uint64), np.zeros(nf, np.uint64)
        np.add.at(sx, full[0] - 1, full[2].astype(np.uint64))
        np.add.at(sxx, full[0] - 1, (full[2] * full[2]).astype(np.uint64))
        A = sweep.hvg_rank(n_cells, sx, sxx)[0]
        _PAIRS[key] = (case, hits, ids, n_cells, nf, A, _sets(full, n_cells, A, nf))
    return _PAIRS[key]


def _point(name, verb, rc, value, seed=926):
    """the reference of one point: (the fields of its coexpr.tsv.gz rows, the fields of its table row with mean_kept as a Fraction)"""
    key = (name, verb, float(rc), float(value), seed)
    if key not in _POINTS:
        case, hits, ids, n_cells, nf, A, full_sets = _pair(name, rc, seed)
        if verb == "sweep":
            ora = O.run_bam2db(case.bt, case.ft, case.flags, case.xf, case.cb, case.gx, case.ub, float(np.float32(rc)), float(np.float32(value)), seed, b"x.bam", False)
            rows, lead = TG._rows_of(ora["matrix"]), ["%.3f" % rc, "%.3f" % value]
        elif verb == "cap":
            rows, lead = TG._rows_of(cap_ref.point(case, b"x.bam", rc, value, seed)["matrix"]), ["%.3f" % rc, str(int(value))]
        else:
            rows, lead = TG._rows_of(level_ref.point(hits, value)["matrix"]), ["%.3f" % rc, str(int(value))]
        kf, kp, sh = R.per_gene(full_sets, _sets(rows, n_cells, A, nf))
        genes = [[ids[int(A[g])], str(kf[g]), str(kp[g]), str(sh[g])] for g in range(len(A))]
        _POINTS[key] = (genes, R.summary_fields(lead, seed, n_cells, K, kf, kp, sh))
    return _POINTS[key]


def _assert_row(got, want, what):
    assert len(got) == len(want) == 12, (what, got, want)
    assert got[:10] == want[:10] and got[11] == want[11], (what, got, want)
    if want[10] is None:
        assert got[10] == "NA", (what, got)
    else:
        assert len(got[10].split(".")[1]) == 6 and abs(Fraction(got[10]) - want[10]) <= Fraction(1, 2000000), (what, got, want)


def _gz(p):
    return gzip.decompress(open(p, "rb").read())


def _check_outputs(out, name, verb, rates, values, seeds=(926,), reps=False, summary_only=False):
    lines = open(out / ("%s_coexpr.tsv" % verb)).read().split("\n")
    assert lines[0].split("\t") == list(MOD[verb].COEXPRESSION_COLUMNS) and lines[-1] == ""
    assert len(lines) - 2 == len(rates) * len(values) * len(seeds)
    at = 1
    for rc in rates:
        for seed in seeds:
            for v in values:
                genes, row = _point(name, verb, rc, v, seed)
                _assert_row(lines[at].split("\t"), row, (verb, rc, seed, v))
                at += 1
                d = out / (MOD[verb].point_dir(rc, v) + ("_s%d" % seed if reps else ""))
                if summary_only:
                    assert not d.exists()
                    continue
                got = _gz(d / "coexpr.tsv.gz").decode().split("\n")
                assert got[0].split("\t") == list(sweep.POINT_COEXPRESSION_COLUMNS) and got[-1] == "" and len(got) - 2 == len(genes)
                assert [g.split("\t") for g in got[1:-1]] == genes, (verb, rc, seed, v)
                assert [r["gene"] for r in MOD[verb].read_point_coexpression(d / "coexpr.tsv.gz")] == [g[0] for g in genes]
    assert not [n for n in os.listdir(out) if n.endswith(".partial")]


def test_the_mixed_case_is_beyond_one_selection_workgroup_and_off_the_tile():
    _, _, _, n_cells, _, A, full_sets = _pair("mixed", 0.5, 926)
    assert len(A) >= 65 and n_cells % 32 != 0 and max(len(s) for s in full_sets) == K


@pytest.mark.parametrize("name", ["edge", "mixed"])
@pytest.mark.parametrize("verb", ["sweep", "cap", "level"])
def test_cli_with_the_flag_and_the_same_tree_without_it(tmp_path, verb, name):
    bam, b, f = _write(tmp_path, TG._case(name))
    rates, values = TG._grid(name, verb)
    out, out0 = tmp_path / "out", tmp_path / "out0"
    r = subprocess.run(TG._args(verb, bam, b, f, out, rates, values) + ["--coexpression"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, FASTF_PROFILE="1"))
    assert r.returncode == 0, r.stderr
    assert "%s_coexpr.tsv is generated." % verb in r.stdout and "[%s] --coexpression:" % verb in r.stderr
    assert "neighbors.tsv is generated." not in r.stdout and "--neighbors:" not in r.stderr and "fidelity:" not in r.stderr
    _check_outputs(out, name, verb, rates, values)
    r = subprocess.run(TG._args(verb, bam, b, f, out0, rates, values), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    with_flag, without = TG._tree(out), TG._tree(out0)
    new = {n for n in with_flag if n == "%s_coexpr.tsv" % verb or os.path.basename(n) == "coexpr.tsv.gz"}
    assert len(new) == 1 + len(rates) * len(values) and not [n for n in without if "coexpr" in n or "neighbors" in n or "fidelity" in n]
    assert {n: v for n, v in with_flag.items() if n not in new} == without


@pytest.mark.parametrize("form", ["mfma", "plain"])
@pytest.mark.parametrize("verb", ["sweep", "cap", "level"])
def test_in_process_and_summary_only(tmp_path, verb, form, monkeypatch):
    if form == "plain":
        monkeypatch.setenv("FASTF_COEXPR_MFMA", "0")
        monkeypatch.setenv("FASTF_COEXPR_CHUNK", "64")      # 300 cells: five chunks
    bam, b, f = _write(tmp_path, TG._case("mixed"))
    rates, values = TG._grid("mixed", verb)
    out = tmp_path / "out"
    MOD[verb].__dict__[verb](bam, out, b, f, rates, values, seed=926, coexpression=True)
    _check_outputs(out, "mixed", verb, rates, values)
    rows = MOD[verb].read_coexpression_table(out / ("%s_coexpr.tsv" % verb))
    assert len(rows) == len(rates) * len(values) and rows[0]["seed"] == "926" and rows[0]["k"] == "15" and int(rows[0]["hvg_k"]) >= 65
    last = rows[-1]                                         # the deepest point of the grid is the full matrix itself
    assert last["sum_k_full"] == last["sum_k_point"] == last["sum_shared"] and last["mean_kept"] == "1.000000"
    assert int(rows[0]["sum_shared"]) < int(rows[0]["sum_k_full"])
    out2 = tmp_path / "out2"
    MOD[verb].__dict__[verb](bam, out2, b, f, rates, values, seed=926, coexpression=True, summary_only=True)
    _check_outputs(out2, "mixed", verb, rates, values, summary_only=True)
    assert sorted(os.listdir(out2)) == sorted(["%s.tsv" % verb, "%s_coexpr.tsv" % verb])
    assert open(out2 / ("%s_coexpr.tsv" % verb)).read() == open(out / ("%s_coexpr.tsv" % verb)).read()


@pytest.mark.parametrize("verb", ["sweep", "cap", "level"])
def test_with_neighbors_and_fidelity(tmp_path, verb):
    """--neighbors ranks the same genes and --fidelity keeps the same full rows: every file of the two stays what it is"""
    bam, b, f = _write(tmp_path, TG._case("mixed"))
    rates, values = TG._grid("mixed", verb)
    out, out0 = tmp_path / "out", tmp_path / "out0"
    for o, extra in ((out, ["--coexpression"]), (out0, [])):
        r = subprocess.run(TG._args(verb, bam, b, f, o, rates, values) + ["--neighbors", "--fidelity"] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
    _check_outputs(out, "mixed", verb, rates, values)
    with_flag, without = TG._tree(out), TG._tree(out0)
    assert {n: v for n, v in with_flag.items() if "coexpr" not in n} == without and len(with_flag) == len(without) + 1 + len(rates) * len(values)
    assert all(any(n.endswith(e) for n in without) for e in ("/neighbors.tsv.gz", "/fidelity.tsv.gz"))


def test_two_seeds_give_one_row_per_cell_rate_seed_and_value(tmp_path):
    bam, b, f = _write(tmp_path, TG._case("mixed"))
    out = tmp_path / "out"
    r = subprocess.run(TG._args("sweep", bam, b, f, out, [0.5], [0.1, 1]) + ["--coexpression", "--seeds", "1,2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    _check_outputs(out, "mixed", "sweep", [0.5], [0.1, 1], seeds=(1, 2), reps=True)
    rows = sweep.read_coexpression_table(out / "sweep_coexpr.tsv")
    assert [x["seed"] for x in rows] == ["1", "1", "2", "2"] and rows[0] != rows[2]
    assert not [n for n in os.listdir(out) if "coexpr_reps" in n]


@pytest.mark.parametrize("verb", ["cap", "level"])
def test_two_seeds_of_cap_and_level(tmp_path, verb):
    """the point files in <point>_s<seed>/ and the rows in the order (cell rate, seed, value), through the CLI; one seed in process"""
    bam, b, f = _write(tmp_path, TG._case("mixed"))
    rates, values = TG._grid("mixed", verb)
    out = tmp_path / "out"
    r = subprocess.run(TG._args(verb, bam, b, f, out, rates, values) + ["--coexpression", "--seeds", "926,5"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    _check_outputs(out, "mixed", verb, rates, values, seeds=(926, 5), reps=True)
    rows = MOD[verb].read_coexpression_table(out / ("%s_coexpr.tsv" % verb))
    assert [x["seed"] for x in rows] == ["926", "926", "5", "5"] and rows[0] != rows[2]
    assert not [n for n in os.listdir(out) if "coexpr_reps" in n]
    out2 = tmp_path / "out2"
    getattr(MOD[verb], verb + "_reps")(bam, out2, b, f, rates, values[:1], [926], coexpression=True, summary_only=True)
    _check_outputs(out2, "mixed", verb, rates, values[:1], seeds=(926,), reps=True, summary_only=True)


def test_flag_4096_is_accepted_and_the_unassigned_bits_beside_it_are_not(tmp_path):
    L = _lib.lib()
    one = np.ones(1, np.float32)
    caps = np.array([5], np.uint64)
    import ctypes as C
    p_one = one.ctypes.data_as(C.POINTER(C.c_float))
    calls = (lambda fl: L.fastf_sweep(b"x", b"y", b"b", b"f", p_one, 1, p_one, 1, 926, fl), lambda fl: L.fastf_cap(b"x", b"y", b"b", b"f", p_one, 1, caps.ctypes.data, 1, 926, fl),
             lambda fl: L.fastf_level(b"x", b"y", b"b", b"f", p_one, 1, caps.ctypes.data, 1, 926, fl))
    assert sweep.COEXPRESSION == cap.COEXPRESSION == level.COEXPRESSION == 4096
    for call in calls:
        with pytest.raises(F.FastfError, match="does not exist"):
            _lib.check(call(4096))
        for flags in (4096 | 1024, 4096 | 2048):
            with pytest.raises(F.FastfError, match="unknown flags"):
                _lib.check(call(flags))
