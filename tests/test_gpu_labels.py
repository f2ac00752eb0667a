"""--labels on the GPU: fastf_dev_label_votes in both forms (the confusion counts through LDS, and by global atomics alone under
FASTF_LABELS_LDS=0) on the fixtures of test_labels_host against labels_ref — guard words behind every output, conf pre-filled with
garbage, no index out of range anywhere — and sweep, cap and level with --labels through the CLI and in process: every labels file
against labels_ref applied to the point's own written matrix and the full-depth matrix, every other file byte-identical to the run
without the option."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, cap, hostmem, level, sweep, synth
import labels_ref as LR
from sweep_ref import parse_matrix
import test_labels_host as H

pytestmark = pytest.mark.gpu

FORMS = ("lds", "global")
GUARD = 0xA5


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
        monkeypatch.setenv("FASTF_LABELS_LDS", "0")
    else:
        monkeypatch.delenv("FASTF_LABELS_LDS", raising=False)


def _device_votes(eng, fx):
    """one call on device copies of a fixture: every output array has 64 guard bytes behind it, conf comes in as garbage"""
    import torch
    idx, cnt, lab, k, L = fx
    n = len(cnt)
    assert int(cnt.max(initial=0)) <= k and all(int(v) < n for row, c in zip(idx, cnt) for v in row[:c])      # no index out of range is handed over
    words = L * (L + 1)
    d_idx = hostmem.to_device(np.ascontiguousarray(idx, np.uint32).reshape(-1) if n else np.zeros(1, np.uint32), "cuda")
    d_cnt = hostmem.to_device(cnt if n else np.zeros(1, np.uint32), "cuda")
    d_lab = hostmem.to_device(lab if n else np.zeros(1, np.uint8), "cuda")
    outs = [torch.full((n + 64,), GUARD, dtype=torch.uint8, device="cuda") for _ in range(3)]
    d_conf = torch.full((words + 16,), 0x5EEDBEEF, dtype=torch.int32, device="cuda")
    eng.dev_label_votes(d_idx.data_ptr(), d_cnt.data_ptr(), d_lab.data_ptr(), n, k, L, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), d_conf.data_ptr())
    torch.cuda.synchronize()
    host = [hostmem.to_host(o) for o in outs]
    conf = hostmem.to_host(d_conf).view(np.uint32)
    assert all((h[n:] == GUARD).all() for h in host) and (conf[words:] == 0x5EEDBEEF).all(), "bytes behind an array were written"
    return host[0][:n], host[1][:n], host[2][:n], conf[:words]


# n: one cell, a group, a wave and a workgroup's pass and their neighbours, several workgroups and their LDS flushes; k: the edges of the
# lane groups of 16, 32 and 64; L: one label, 127 and 128 (64 KB of counts), 201 and 202 (the last that fits the LDS and the first that
# does not), 255
SHAPES = [(n, 15, 30) for n in (1, 2, 15, 16, 17, 63, 64, 65, 257, 1000)] + [(65, k, 7) for k in (1, 16, 17, 32, 33, 64)] + \
         [(257, 15, L) for L in (1, 2, 127, 128, 201, 202, 255)] + [(1000, 33, 201), (1000, 64, 128)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n,k,L", SHAPES)
def test_votes_against_the_reference(eng, n, k, L, form, monkeypatch):
    _form(monkeypatch, form)
    fx = H.random_fixture(n, k, L, seed=n * 131 + k * 7 + L)
    H.check_against_reference(_device_votes(eng, fx), fx)
    H.check_against_reference(sweep.label_votes(*fx), fx)       # the host twin agrees


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", H.HAND)
def test_the_hand_built_sets_and_their_overwritten_pads(eng, name, form, monkeypatch):
    _form(monkeypatch, form)
    fx = H.hand_fixture(name)
    got = _device_votes(eng, fx)
    H.check_against_reference(got, fx)
    assert [int(v) for v in got[0]] == H.HAND_PRED[name]
    H.check_against_reference(_device_votes(eng, H.overwritten_pads(fx)), fx)


@pytest.mark.parametrize("form", FORMS)
def test_pads_cnt_zero_and_no_cells(eng, form, monkeypatch):
    _form(monkeypatch, form)
    fx = H.pads_fixture()
    assert [int(v) for v in _device_votes(eng, fx)[0]] == [1] * 5
    for shape in ((257, 33, 9), (1000, 15, 128)):
        big = H.random_fixture(*shape, seed=9)
        H.check_against_reference(_device_votes(eng, H.overwritten_pads(big)), big)
    idx, cnt, lab, k, L = H.random_fixture(100, 15, 4, seed=2)
    none = (np.full_like(idx, H.NONE), np.zeros_like(cnt), lab, k, L)       # all cnt zero: every prediction 0, conf in column 0
    got = _device_votes(eng, none)
    H.check_against_reference(got, none)
    assert not got[0].any() and got[3].reshape(L, L + 1)[:, 0].sum() == int((lab > 0).sum())
    empty = (np.zeros((0, 15), np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint8), 15, 3)
    assert not _device_votes(eng, empty)[3].any()           # no cells: conf is zeroed all the same
    for bad_k in (0, 65):
        with pytest.raises(F.FastfError, match="from 1 to 64"):
            eng.dev_label_votes(0, 0, 0, 0, bad_k, 3, 0, 0, 0, 0)
    with pytest.raises(F.FastfError, match="256 labels, at most 255"):
        eng.dev_label_votes(0, 0, 0, 0, 15, 256, 0, 0, 0, 0)


# ---- the commands ----
MOD = {"sweep": sweep, "cap": cap, "level": level}
OPT = {"sweep": "-r", "cap": "-n", "level": "-m"}
GRID = {"sweep": [0.1, 0.5], "cap": [3, 8], "level": [2, 6]}


def _write(tmp_path, case):
    bam, b, f, lf = tmp_path / "in.bam", tmp_path / "barcodes.in.tsv", tmp_path / "features.in.tsv", tmp_path / "labels.in.tsv"
    synth.write_bam(str(bam), case.flags, case.xf, case.cb, case.gx, case.ub)
    b.write_bytes(case.bt); f.write_bytes(case.ft); lf.write_bytes(case.labels_text)
    return bam, b, f, lf


def _args(verb, bam, b, f, out, rates, values):
    return [_lib.cli_path(), verb, "-b", str(bam), "-a", str(b), "-f", str(f), "-o", str(out), "-c", ",".join("%g" % r for r in rates),
            OPT[verb], ",".join(str(v) for v in values)]


def _gz(p):
    return gzip.decompress(open(p, "rb").read())


def _tree(root):
    out = {}
    for dirpath, _, files in os.walk(root):
        for fn in files:
            p = os.path.join(dirpath, fn)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def _is_new(name, verb):
    return name in ("%s_labels.tsv" % verb, "%s_label_classes.tsv" % verb) or os.path.basename(name) in ("labels.tsv.gz", "label_confusion.tsv.gz")


def _check_outputs(out, case, verb, rates, values, seeds=(926,), reps=False, written=None):
    """written: a tree of the same run without --summary-only whose matrices give the reference (summary_only runs write none)"""
    lines = open(out / ("%s_labels.tsv" % verb)).read().split("\n")
    classes = open(out / ("%s_label_classes.tsv" % verb)).read().split("\n")
    assert lines[0].split("\t") == list(MOD[verb].LABELS_COLUMNS) and lines[-1] == "" and len(lines) - 2 == len(rates) * len(values) * len(seeds)
    assert classes[0].split("\t") == list(MOD[verb].LABEL_CLASSES_COLUMNS) and classes[-1] == "" and len(classes) - 2 == 3 * (len(lines) - 2)
    at = 1
    for rc in rates:
        for seed in seeds:
            full_rows, barcodes = case.matrix(rc, 1, seed)
            for v in values:
                name = MOD[verb].point_dir(rc, v) + ("_s%d" % seed if reps else "")
                d = (written or out) / name
                point_rows = parse_matrix(_gz(d / "matrix.mtx.gz"))[3:]
                assert _gz(d / "barcodes.tsv.gz").decode().split("\n")[:-1] == barcodes
                names, lab, full, point = H.reference_point(case, full_rows, point_rows, barcodes)
                lead = ["%.3f" % rc, "%.3f" % v if verb == "sweep" else str(int(v))]
                assert lines[at].split("\t") == LR.summary_fields(lead, seed, 15, 3, lab, full, point), (verb, rc, seed, v)
                assert [c.split("\t") for c in classes[3 * at - 2:3 * at + 1]] == LR.classes_fields(lead, seed, names, lab, full, point)
                at += 1
                if written:
                    assert not (out / name).exists()
                    continue
                got = _gz(d / "labels.tsv.gz").decode().split("\n")
                assert got[0].split("\t") == list(sweep.POINT_LABELS_COLUMNS) and got[-1] == ""
                assert [g.split("\t") for g in got[1:-1]] == LR.cell_rows(barcodes, names, lab, full, point)
                assert [r["barcode"] for r in sweep.read_point_labels(d / "labels.tsv.gz")] == barcodes
                conf = _gz(d / "label_confusion.tsv.gz").decode().split("\n")
                assert conf[-1] == "" and [c.split("\t") for c in conf[:-1]] == LR.confusion_rows(names, lab, point[3])
    assert not [n for n in os.listdir(out) if n.endswith(".partial")]


@pytest.mark.parametrize("verb", ["sweep", "cap", "level"])
def test_cli_with_labels_alone_and_the_same_tree_without(tmp_path, verb):
    case = H.labcase()
    bam, b, f, lf = _write(tmp_path, case)
    rates, values = [0.5, 1], GRID[verb]
    out, out0 = tmp_path / "out", tmp_path / "out0"
    r = subprocess.run(_args(verb, bam, b, f, out, rates, values) + ["--labels", str(lf)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, FASTF_PROFILE="1"))
    assert r.returncode == 0, r.stderr
    assert "%s_labels.tsv and %s_label_classes.tsv are generated." % (verb, verb) in r.stdout
    assert "[%s] --labels: 3 labels, labels_unknown 2;" % verb in r.stderr and "neighbors.tsv is generated." not in r.stdout and "] --neighbors:" not in r.stderr
    _check_outputs(out, case, verb, rates, values)
    r = subprocess.run(_args(verb, bam, b, f, out0, rates, values), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    with_opt, without = _tree(out), _tree(out0)
    new = {n for n in with_opt if _is_new(n, verb)}
    assert len(new) == 2 + 2 * len(rates) * len(values) and not [n for n in with_opt if "neighbors" in n]      # no --neighbors file without --neighbors
    assert {n: v for n, v in with_opt.items() if n not in new} == without


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("verb", ["sweep", "cap", "level"])
def test_in_process_and_summary_only(tmp_path, verb, form, monkeypatch):
    _form(monkeypatch, form)
    case = H.labcase()
    bam, b, f, lf = _write(tmp_path, case)
    rates, values = [1], GRID[verb]
    out, out2 = tmp_path / "out", tmp_path / "out2"
    MOD[verb].__dict__[verb](bam, out, b, f, rates, values, seed=926, labels=lf)
    _check_outputs(out, case, verb, rates, values)
    rows = MOD[verb].read_labels_table(out / ("%s_labels.tsv" % verb))
    assert len(rows) == len(values) and rows[0]["seed"] == "926" and rows[0]["k"] == "15" and rows[0]["n_labels"] == "3" and rows[0]["n_cells"] == "60"
    assert [r["label"] for r in MOD[verb].read_label_classes_table(out / ("%s_label_classes.tsv" % verb))] == ["B", "T", "T cell"] * len(values)
    MOD[verb].__dict__[verb](bam, out2, b, f, rates, values, seed=926, labels=lf, summary_only=True)
    _check_outputs(out2, case, verb, rates, values, written=out)
    assert sorted(os.listdir(out2)) == sorted(["%s.tsv" % verb, "%s_labels.tsv" % verb, "%s_label_classes.tsv" % verb])
    for t in ("%s_labels.tsv", "%s_label_classes.tsv"):
        assert open(out2 / (t % verb)).read() == open(out / (t % verb)).read()


@pytest.mark.parametrize("verb", ["sweep", "cap", "level"])
def test_beside_the_other_options(tmp_path, verb):
    case = H.labcase()
    bam, b, f, lf = _write(tmp_path, case)
    rates, values = [0.5], GRID[verb]
    out, out0 = tmp_path / "out", tmp_path / "out0"
    for o, extra in ((out, ["--labels=" + str(lf)]), (out0, [])):
        r = subprocess.run(_args(verb, bam, b, f, o, rates, values) + ["--neighbors", "--fidelity", "--gene-fidelity", "--genes", "--cells"] + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
    _check_outputs(out, case, verb, rates, values)
    with_opt, without = _tree(out), _tree(out0)
    assert {n: v for n, v in with_opt.items() if not _is_new(n, verb)} == without and len(with_opt) == len(without) + 2 + 2 * len(values)
    assert all(any(n.endswith(e) for n in without) for e in ("_neighbors.tsv", "/neighbors.tsv.gz", "cells.tsv.gz", "genes.tsv.gz", "/fidelity.tsv.gz", "/gene_fidelity.tsv.gz"))


def test_two_seeds_give_one_row_per_cell_rate_seed_and_value(tmp_path):
    case = H.labcase()
    bam, b, f, lf = _write(tmp_path, case)
    out = tmp_path / "out"
    r = subprocess.run(_args("sweep", bam, b, f, out, [0.5], [0.1, 0.5]) + ["--labels", str(lf), "--seeds", "926,5"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    _check_outputs(out, case, "sweep", [0.5], [0.1, 0.5], seeds=(926, 5), reps=True)
    rows = sweep.read_labels_table(out / "sweep_labels.tsv")
    assert [x["seed"] for x in rows] == ["926", "926", "5", "5"] and rows[0] != rows[2]
    assert not [n for n in os.listdir(out) if "labels_reps" in n or "neighbors" in n]
    for k, (verb, mod) in enumerate((("cap", cap), ("level", level))):
        o = tmp_path / ("reps%d" % k)
        mod.__dict__[verb + "_reps"](bam, o, b, f, [0.5], GRID[verb][:1], [5], labels=lf)
        _check_outputs(o, case, verb, [0.5], GRID[verb][:1], seeds=(5,), reps=True)
