"""--markers on the GPU: fastf_dev_marker_auc at one and two planes, with the accumulators in LDS and by global atomics
(FASTF_MARKERS_LDS=0, and what does not fit), against markers_ref and the host twin — guard words behind every output, outputs
pre-filled with garbage, 0x7F in the padding rows and slots of the planes, and behind the planes rows that would change the result
if read — the hand-built fixtures of test_markers_host, the three-plane refusal, and sweep, cap and level with --labels F --markers 5
through the CLI and in process: every markers file against markers_ref applied to the point's own written matrix, the full-depth
matrix and the labels file; every other file byte-identical to the run without --markers."""
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, cap, hostmem, level, sweep
import labels_ref as LR
import markers_ref as MR
import neighbors_ref as NR
from sweep_ref import parse_matrix
import test_labels_host as LH
import test_markers_host as H

pytestmark = pytest.mark.gpu

FORMS = ("lds", "global")
G64, G32 = 0x5EEDBEEF5EEDBEEF, 0x5EEDBEEF


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    cells = np.arange(1, 101, dtype=np.uint64) | (np.uint64(1) << np.uint64(62))
    feats = np.arange(1, 51, dtype=np.uint64) | (np.uint64(2) << np.uint64(62))
    e = F.Engine(cells, feats, umi_max_bases=12)
    yield e
    e.close()


def _form(monkeypatch, form):
    if form == "global":
        monkeypatch.setenv("FASTF_MARKERS_LDS", "0")
    else:
        monkeypatch.delenv("FASTF_MARKERS_LDS", raising=False)


def _device_buffers(fx):
    """device copies of a fixture: the planes with 0x7F in every padding row and slot and, behind them, one more plane-sized block of
    0x55 (a kernel that read a row or a plane too many would count it); every output pre-filled with garbage, 8 guard words behind"""
    import torch
    counts, lab, L, P = fx
    n, K = counts.shape
    planes = sweep.marker_planes(counts, P, 0x7F)
    trailer = np.full(planes[0].size, 0x55, np.uint8)
    d_planes = hostmem.to_device(np.concatenate([planes.reshape(-1), trailer]), "cuda")
    d_lab = hostmem.to_device(lab if n else np.zeros(1, np.uint8), "cuda")
    W = L * K
    outs = [torch.full((W + 8,), G64, dtype=torch.int64, device="cuda"), torch.full((W + 8,), G32, dtype=torch.int32, device="cuda"),
            torch.full((W + 8,), G64, dtype=torch.int64, device="cuda"), torch.full((L + 8,), G32, dtype=torch.int32, device="cuda")]
    return d_planes, d_lab, outs


def _device_tables(eng, fx):
    import torch
    counts, lab, L, P = fx
    n, K = counts.shape
    d_planes, d_lab, outs = _device_buffers(fx)
    eng.dev_marker_auc(d_planes.data_ptr(), P, n, K, d_lab.data_ptr(), L, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr())
    torch.cuda.synchronize()
    assert eng.dev_error_bits() == 0
    s2u, det, tot, npl = (hostmem.to_host(o).view(u) for o, u in zip(outs, (np.uint64, np.uint32, np.uint64, np.uint32)))
    W = L * K
    assert (s2u[W:] == G64).all() and (det[W:] == G32).all() and (tot[W:] == G64).all() and (npl[L:] == G32).all(), "words behind a table were written"
    return s2u[:W].reshape(L, K), det[:W].reshape(L, K), tot[:W].reshape(L, K), npl[:L]


def _same(a, b):
    assert all((x == y).all() for x, y in zip(a, b))


# n: one cell, two, a wave's rows and their neighbours, one step of a workgroup (32 rows at one plane, 256 at two) and the unrolled four,
# several of them; K: one slot, the edges of the 32-slot tile and of K_pad, several tiles, the full gene set; L: one label, two (the
# identity), three, 128 (LDS at either P) and 255 (at one plane the accumulators no longer fit: 226 and more go by global atomics)
SHAPES = [(n, 33, 3) for n in (1, 2, 63, 64, 65, 129, 257, 1000)] + [(129, K, 3) for K in (1, 31, 32, 500, 2000)] + \
         [(257, 33, L) for L in (1, 2, 128, 255)] + [(1000, 2000, 30)]
_REF = {}


def _case(n, K, L, P):
    """the fixture and its reference, made once: the whole tables by the row form of the brute force, at the largest shapes on eight slots"""
    key = (n, K, L, P)
    if key not in _REF:
        fx = H.random_fixture(n, K, L, P, seed=n * 131 + K * 7 + L + P, p_nonzero=0.1 if K >= 500 else 0.3)
        columns = None if n * K <= 129 * 500 else sorted({0, 1, 31, 32, 33, K // 2, K - 2, K - 1})
        _REF[key] = (fx, MR.tables_rows(fx[0], fx[1], L, columns), columns, H.twin(fx))
    return _REF[key]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("n,K,L", SHAPES)
def test_tables_against_the_reference(eng, n, K, L, P, form, monkeypatch):
    _form(monkeypatch, form)
    fx, ref, columns, twin = _case(n, K, L, P)
    assert sweep.marker_auc_form(P, L) == (1 if form == "lds" and (P == 2 or L <= 225) else 0)      # the form this call takes
    got = _device_tables(eng, fx)
    H.check_tables(got, ref, columns)
    H.check_tables(twin, ref, columns)
    _same(got, twin)                                         # every slot, every label


def test_both_sides_of_the_lds_edge_at_one_plane(eng, monkeypatch):
    _form(monkeypatch, "lds")
    for L in (225, 226):
        fx, ref, columns, twin = _case(65, 33, L, 1)
        assert sweep.marker_auc_form(1, L) == (1 if L == 225 else 0)
        got = _device_tables(eng, fx)
        H.check_tables(got, ref)
        _same(got, twin)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", H.HAND)
def test_the_hand_built_fixtures(eng, name, form, monkeypatch):
    _form(monkeypatch, form)
    fx = H.hand_fixture(name)
    ref = MR.tables(fx[0].tolist(), fx[1], fx[2])
    H.check_tables(_device_tables(eng, fx), ref)
    if fx[3] == 1:                                           # the same counts through two planes
        H.check_tables(_device_tables(eng, fx[:3] + (2,)), ref)


def test_two_labels_add_up_and_no_cells(eng):
    for P in (1, 2):
        counts, lab, _, _ = H.random_fixture(300, 40, 2, P, seed=3, p_unlabelled=0.3)
        lab[lab > 2] = 0
        s2u, _, _, npl = _device_tables(eng, (counts, lab, 2, P))
        assert (s2u[0] + s2u[1] == 2 * int(npl[0]) * int(npl[1])).all()
        empty = (np.zeros((0, 5), np.int64), np.zeros(0, np.uint8), 3, P)
        assert not any(t.any() for t in _device_tables(eng, empty))      # no cells: the tables are cleared all the same


def test_three_planes_are_refused_before_anything_is_launched(eng):
    import torch
    fx = H.random_fixture(65, 33, 3, 2, seed=1)
    d_planes, d_lab, outs = _device_buffers(fx)
    for P, L, message in ((3, 3, "FASTF_ERR_MARKER_COUNT.*3 planes"), (1, 0, "0 labels, from 1 to 255"), (2, 256, "256 labels, from 1 to 255")):
        with pytest.raises(F.FastfError, match=message):
            eng.dev_marker_auc(d_planes.data_ptr(), P, 65, 33, d_lab.data_ptr(), L, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr())
    torch.cuda.synchronize()
    assert eng.dev_error_bits() == 0
    s2u, det, tot, npl = (hostmem.to_host(o).view(u) for o, u in zip(outs, (np.uint64, np.uint32, np.uint64, np.uint32)))
    assert (s2u == G64).all() and (det == G32).all() and (tot == G64).all() and (npl == G32).all()      # not even cleared


# ---- the commands ----
MOD = {"sweep": sweep, "cap": cap, "level": level}
OPT = {"sweep": "-r", "cap": "-n", "level": "-m"}
GRID = {"sweep": [0.1, 0.5], "cap": [3, 8], "level": [2, 6]}
TOP = 5


def _write(tmp_path, case):
    from fastf_amd import synth
    bam, b, f, lf = tmp_path / "in.bam", tmp_path / "barcodes.in.tsv", tmp_path / "features.in.tsv", tmp_path / "labels.in.tsv"
    synth.write_bam(str(bam), case.flags, case.xf, case.cb, case.gx, case.ub)
    b.write_bytes(case.bt); f.write_bytes(case.ft); lf.write_bytes(case.labels_text)
    return bam, b, f, lf


def _args(verb, bam, b, f, out, rates, values):
    return [_lib.cli_path(), verb, "-b", str(bam), "-a", str(b), "-f", str(f), "-o", str(out), "-c", ",".join("%g" % r for r in rates),
            OPT[verb], ",".join(str(v) for v in values)]


def _gz(p):
    import gzip
    return gzip.decompress(open(p, "rb").read())


def _tree(root):
    out = {}
    for dirpath, _, files in os.walk(root):
        for fn in files:
            p = os.path.join(dirpath, fn)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def _is_new(name, verb):
    return name == "%s_markers.tsv" % verb or os.path.basename(name) == "markers.tsv.gz"


def _reference(case, full_rows, point_rows, barcodes, feat_ids, n_features=45):
    """(names, gene ids of A by slot, full, point, rank_full, rank_point) by the references alone: A recomputed from the full rows"""
    names, ids = LR.label_ids(case.pairs)
    lab = [ids.get(bc, 0) for bc in barcodes]
    n, L = len(barcodes), len(names) - 1
    A = [int(g) for g in NR.hvg_of_rows(full_rows, n, n_features)]
    full = MR.tables(NR.dense(full_rows, n, A).tolist(), lab, L)
    point = MR.tables(NR.dense(point_rows, n, A).tolist(), lab, L)
    return names, [feat_ids[g] for g in A], full, point, MR.ranks(full[0], full[3], A), MR.ranks(point[0], point[3], A)


def _check_outputs(out, case, verb, rates, values, seeds=(926,), reps=False, written=None):
    """written: a tree of the same run without --summary-only whose matrices give the reference (summary_only runs write none)"""
    lines = open(out / ("%s_markers.tsv" % verb)).read().split("\n")
    assert lines[0].split("\t") == list(MOD[verb].MARKERS_COLUMNS) and lines[-1] == "" and len(lines) - 2 == 4 * len(rates) * len(values) * len(seeds)
    at = 1
    for rc in rates:
        for seed in seeds:
            full_rows, barcodes = case.matrix(rc, 1, seed)
            for v in values:
                name = MOD[verb].point_dir(rc, v) + ("_s%d" % seed if reps else "")
                d = (written or out) / name
                point_rows = parse_matrix(_gz(d / "matrix.mtx.gz"))[3:]
                assert _gz(d / "barcodes.tsv.gz").decode().split("\n")[:-1] == barcodes
                feat_ids = [ln.split("\t")[0] for ln in _gz(d / "features.tsv.gz").decode().split("\n")[:-1]]
                names, gene_ids, full, point, rf, rp = _reference(case, full_rows, point_rows, barcodes, feat_ids)
                lead = ["%.3f" % rc, "%.3f" % v if verb == "sweep" else str(int(v))]
                assert [ln.split("\t") for ln in lines[at:at + 4]] == MR.summary_rows(lead, seed, names, len(gene_ids), TOP, full, point, rf, rp), (verb, rc, seed, v)
                at += 4
                if written:
                    assert not (out / name).exists()
                    continue
                got = _gz(d / "markers.tsv.gz").decode().split("\n")
                want = MR.point_rows(names, gene_ids, TOP, full, point, rf, rp)
                assert got[0].split("\t") == list(sweep.POINT_MARKERS_COLUMNS) and got[-1] == ""
                assert [g.split("\t") for g in got[1:-1]] == want
                assert len(sweep.read_point_markers(d / "markers.tsv.gz")) == len(want) >= 3 * TOP
    assert not [n for n in os.listdir(out) if n.endswith(".partial")]


@pytest.mark.parametrize("verb", ["sweep", "cap", "level"])
def test_cli_with_markers_and_the_same_tree_without(tmp_path, verb):
    case = LH.labcase()
    bam, b, f, lf = _write(tmp_path, case)
    rates, values = [0.5, 1], GRID[verb]
    out, out0 = tmp_path / "out", tmp_path / "out0"
    r = subprocess.run(_args(verb, bam, b, f, out, rates, values) + ["--labels", str(lf), "--markers", str(TOP)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, FASTF_PROFILE="1"))
    assert r.returncode == 0, r.stderr
    assert "%s_markers.tsv is generated." % verb in r.stdout and "[%s] --markers: top 5 of the genes per label;" % verb in r.stderr
    _check_outputs(out, case, verb, rates, values)
    r = subprocess.run(_args(verb, bam, b, f, out0, rates, values) + ["--labels", str(lf)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "markers" not in r.stdout
    with_opt, without = _tree(out), _tree(out0)
    new = {n for n in with_opt if _is_new(n, verb)}
    assert len(new) == 1 + len(rates) * len(values)
    assert {n: v for n, v in with_opt.items() if n not in new} == without and not [n for n in without if "markers" in n]


@pytest.mark.parametrize("verb,form", [("sweep", "lds"), ("sweep", "global"), ("cap", "lds"), ("level", "global")])
def test_in_process_and_summary_only(tmp_path, verb, form, monkeypatch):
    _form(monkeypatch, form)
    case = LH.labcase()
    bam, b, f, lf = _write(tmp_path, case)
    rates, values = [1], GRID[verb]
    out, out2 = tmp_path / "out", tmp_path / "out2"
    MOD[verb].__dict__[verb](bam, out, b, f, rates, values, seed=926, labels=lf, markers=TOP)
    _check_outputs(out, case, verb, rates, values)
    rows = MOD[verb].read_markers_table(out / ("%s_markers.tsv" % verb))
    assert [r["label"] for r in rows] == ["B", "T", "T cell", "all"] * len(values) and rows[0]["seed"] == "926" and rows[0]["top"] == "5"
    MOD[verb].__dict__[verb](bam, out2, b, f, rates, values, seed=926, labels=lf, markers=TOP, summary_only=True)
    _check_outputs(out2, case, verb, rates, values, written=out)
    assert sorted(os.listdir(out2)) == sorted(["%s.tsv" % verb, "%s_labels.tsv" % verb, "%s_label_classes.tsv" % verb, "%s_markers.tsv" % verb])
    assert open(out2 / ("%s_markers.tsv" % verb)).read() == open(out / ("%s_markers.tsv" % verb)).read()


@pytest.mark.parametrize("verb", ["sweep", "cap", "level"])
def test_beside_the_other_options(tmp_path, verb):
    case = LH.labcase()
    bam, b, f, lf = _write(tmp_path, case)
    rates, values = [0.5], GRID[verb]
    out, out0 = tmp_path / "out", tmp_path / "out0"
    for o, extra in ((out, ["--markers=%d" % TOP]), (out0, [])):
        r = subprocess.run(_args(verb, bam, b, f, o, rates, values) + ["--labels=" + str(lf), "--neighbors", "--fidelity", "--gene-fidelity", "--genes", "--cells"] + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
    _check_outputs(out, case, verb, rates, values)
    with_opt, without = _tree(out), _tree(out0)
    assert {n: v for n, v in with_opt.items() if not _is_new(n, verb)} == without and len(with_opt) == len(without) + 1 + len(values)
    assert all(any(n.endswith(e) for n in without) for e in ("_neighbors.tsv", "_labels.tsv", "cells.tsv.gz", "genes.tsv.gz", "/fidelity.tsv.gz", "/gene_fidelity.tsv.gz"))


def test_two_seeds_give_the_rows_per_cell_rate_seed_and_value(tmp_path):
    case = LH.labcase()
    bam, b, f, lf = _write(tmp_path, case)
    out = tmp_path / "out"
    r = subprocess.run(_args("sweep", bam, b, f, out, [0.5], [0.1, 0.5]) + ["--labels", str(lf), "--markers", str(TOP), "--seeds", "926,5"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    _check_outputs(out, case, "sweep", [0.5], [0.1, 0.5], seeds=(926, 5), reps=True)
    rows = sweep.read_markers_table(out / "sweep_markers.tsv")
    assert [x["seed"] for x in rows] == ["926"] * 8 + ["5"] * 8 and rows[:4] != rows[8:12]
    assert not [n for n in os.listdir(out) if "markers_reps" in n]
    for k, (verb, mod) in enumerate((("cap", cap), ("level", level))):
        o = tmp_path / ("reps%d" % k)
        mod.__dict__[verb + "_reps"](bam, o, b, f, [0.5], GRID[verb][1:], [5], labels=lf, markers=TOP)
        _check_outputs(o, case, verb, [0.5], GRID[verb][1:], seeds=(5,), reps=True)
