"""--mapping on the host: the census of the shared fixtures (mapping_ref), the host twin (fastf_mapping_from_coo) against the reference on
every fixture and on shuffled rows, the rows, headers and NA rules of both files, both halves of the 2^42 refusal, k outside 1 .. 64, the
help texts, the refusals before the output directory is made, and the Python mirrors."""
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, cap, level, sweep
import labels_ref as LR
import mapping_ref as M
import neighbors_ref as N
import test_neighbors_host as H

MOD = {"sweep": sweep, "cap": cap, "level": level}


def test_census_of_the_fixtures():
    M.census()


def _twin(name, shuffle=None):
    full, point, n, nf, genes, k = M.fixture(name)
    if shuffle is not None:
        rng = np.random.default_rng(shuffle)
        full, point = (tuple(a[o] for a in rows) for rows, o in ((full, rng.permutation(len(full[0]))), (point, rng.permutation(len(point[0])))))
    return sweep.mapping_from_coo(full, point, n, sweep.neighbors_slot_map(genes, nf), k)


@pytest.mark.parametrize("name", M.FIXTURES)
def test_the_host_twin_against_the_reference(name):
    lists, sd, rank, _ = M.reference(name)
    n = M.fixture(name)[2]
    idx, cnt, got_sd, got_rank = _twin(name)
    assert H.as_lists(idx, cnt) == lists
    assert [int(v) for v in got_sd] == sd
    assert [None if int(v) == M.NONE else int(v) for v in got_rank] == rank
    assert all((idx[i, cnt[i]:] == M.NONE).all() for i in range(n))
    again = _twin(name, shuffle=1)                          # the rows in any order
    assert all((a == b).all() for a, b in zip(again, (idx, cnt, got_sd, got_rank)))


def test_the_mapping_is_not_the_neighbour_set_of_either_side():
    full, point, n, nf, genes, k = M.fixture("asymmetric")
    lists = M.reference("asymmetric")[0]
    assert lists != N.neighbor_sets(full, n, genes, k)[0] and lists != N.neighbor_sets(point, n, genes, k)[0]


def test_both_halves_of_the_norm_refusal_and_k():
    genes, nf = np.array([0, 1]), 2
    sm = sweep.neighbors_slot_map(genes, nf)
    ok = (np.array([1, 2], np.uint32), np.array([1, 1], np.uint32), np.array([(1 << 21) - 1, 1], np.uint32))      # norm 2^42 - 2^22 + 2
    big = (np.array([1, 2], np.uint32), np.array([1, 1], np.uint32), np.array([(1 << 21) - 1, 1 << 11], np.uint32))      # norm 2^42 + 1
    assert int(ok[2][0]) ** 2 + 1 < 1 << 42 <= int(big[2][0]) ** 2 + int(big[2][1]) ** 2
    idx, cnt, sd, rank = sweep.mapping_from_coo(ok, ok, 2, sm, 15)
    assert int(sd[0]) == ((1 << 21) - 1) ** 2 + 1 and int(rank[0]) == 0 and int(rank[1]) == M.NONE
    for full, point in ((big, ok), (ok, big)):              # the full side, the point side
        with pytest.raises(F.FastfError, match="FASTF_ERR_NEIGHBOR_NORM"):
            sweep.mapping_from_coo(full, point, 2, sm, 15)
    for k in (0, 65):
        with pytest.raises(F.FastfError, match="mapping: k = %d, from 1 to 64" % k):
            sweep.mapping_from_coo(ok, ok, 2, sm, k)
    assert sweep.mapping_from_coo(ok, ok, 2, sm, 64)[0].shape == (2, 64)


def test_headers_and_columns():
    assert sweep.mapping_header() == "\t".join(sweep.POINT_MAPPING_COLUMNS) + "\n"
    assert sweep.POINT_MAPPING_COLUMNS == ("barcode", "self_dot", "self_rank", "k_map", "k_full", "hood", "pred_map")
    for verb, second in (("sweep", "rate_depth"), ("cap", "reads_per_cell"), ("level", "umi_cap")):
        cols = MOD[verb].MAPPING_COLUMNS
        assert MOD[verb].mapping_header(verb) == sweep.mapping_header(verb) == "\t".join(cols) + "\n"
        assert verb == "sweep" or MOD[verb].mapping_header() == sweep.mapping_header(verb)      # (cap and level name themselves)
        assert cols == ("rate_cell", second, "seed", "n_cells", "hvg_k", "k", "cells_defined", "self_top1", "self_topk", "median_self_rank", "p90_self_rank",
                        "mean_hood", "cells_labelled", "accuracy_map")
    assert sweep.MAPPING_K == 15 and cap.POINT_MAPPING_COLUMNS == level.POINT_MAPPING_COLUMNS == sweep.POINT_MAPPING_COLUMNS


def test_the_rows_and_their_na_rules():
    assert sweep.mapping_row("AAA-1", 7, 0, 15, 15, 9, "T cell") == "AAA-1\t7\t0\t15\t15\t9\tT cell\n"
    assert sweep.mapping_row(b"AAA-1", 0, None, 0, 3, 0) == "AAA-1\t0\tNA\t0\t3\t0\tNA\n"
    assert sweep.mapping_row("C", 1 << 41, sweep.MAPPING_NO_RANK, 2, 0, 0, None) == "C\t%d\tNA\t2\t0\t0\tNA\n" % (1 << 41)
    # no cell defined, no full neighbour, no labels: NA in every ratio
    assert sweep.mapping_summary_row(0.5, 0.25, 926, 0, [0, 0], [M.NONE] * 2, [0, 0], [0, 0]) == "0.500\t0.250\t926\t2\t0\t15\t0\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n"
    assert sweep.mapping_summary_row(1, 1, 5, 3, [], [], [], []) == "1.000\t1.000\t5\t0\t3\t15\t0\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n"
    # labels, but no labelled cell / no labelled neighbour: cells_labelled is a number, the accuracy NA
    assert sweep.mapping_summary_row(1, 1, 5, 3, [1], [0], [2], [1], [0], [0], [0]).endswith("\t1.000000\t1.000000\t0.000000\t0\t0.500000\t0\tNA\n")
    assert cap.mapping_summary_row(1, 40, 5, 3, [1], [0], [2], [1], [2], [0], [0]).endswith("\t0.500000\t1\tNA\n")
    assert cap.mapping_summary_row(1, 40, 5, 3, [1], [0], [2], [1], [2], [0], [0]).startswith("1.000\t40\t5\t1\t3\t15\t1\t")
    assert level.mapping_summary_row(0.5, 7, 5, 3, [1], [3], [2], [2], [2], [1], [4]).startswith("0.500\t7\t")


@pytest.mark.parametrize("name", ["same", "outside_A", "asymmetric", "k1", "zero_point"])
def test_the_summary_row_against_the_reference(name):
    full, point, n, nf, genes, k = M.fixture(name)
    lists, sd, rank, _ = M.reference(name)
    full_sets = N.neighbor_sets(full, n, genes, k)[0]
    hd = M.hood(lists, full_sets)
    rk = [M.NONE if r is None else r for r in rank]
    kf = [len(s) for s in full_sets]
    lab = [(i * 7) % 4 for i in range(n)]                   # 0 .. 3: a quarter unlabelled
    votes = LR.votes(lists, lab, 3)
    for lead, kw, mod in ((["0.500", "0.250"], dict(list_value=0), None), (["0.500", "12"], dict(list_value=12), None)):
        got = sweep.mapping_summary_row(0.5, 0.25, 926, len(genes), sd, rk, kf, hd, k=k, **kw).rstrip("\n").split("\t")
        N.assert_fields(got, M.summary_fields(lead, 926, len(genes), k, lists, sd, rank, full_sets), 5, name)
        got = sweep.mapping_summary_row(0.5, 0.25, 926, len(genes), sd, rk, kf, hd, lab, votes[1], votes[2], k=k, **kw).rstrip("\n").split("\t")
        N.assert_fields(got, M.summary_fields(lead, 926, len(genes), k, lists, sd, rank, full_sets, lab, votes), 5, name)
    names = ["NA", "a", "b", "c"]
    rows = M.cell_rows(["bc%d" % i for i in range(n)], lists, sd, rank, full_sets, names, votes[0])
    for i, want in enumerate(rows):
        got = sweep.mapping_row("bc%d" % i, sd[i], rank[i], len(lists[i]), kf[i], hd[i], names[votes[0][i]] if votes[0][i] else None)
        assert got.rstrip("\n").split("\t") == want


def test_the_vote_of_the_host_twin_takes_the_lists_unchanged():
    """M(i) is in the layout of the neighbour sets: fastf_label_votes and fastf_neighbors_shared read it as it is"""
    full, point, n, nf, genes, k = M.fixture("asymmetric")
    idx, cnt, _, _ = _twin("asymmetric")
    lab = np.array([(i * 7) % 4 for i in range(n)], np.uint8)
    pred, same, labelled = (np.zeros(n, np.uint8) for _ in range(3))
    conf = np.zeros(3 * 4, np.uint32)
    _lib.check(_lib.lib().fastf_label_votes(idx.ctypes.data, cnt.ctypes.data, lab.ctypes.data, n, k, 3, pred.ctypes.data, same.ctypes.data, labelled.ctypes.data, conf.ctypes.data))
    want = LR.votes(M.reference("asymmetric")[0], lab.tolist(), 3)
    assert (pred.tolist(), same.tolist(), labelled.tolist()) == (want[0], want[1], want[2])
    fidx, fcnt, _ = sweep.neighbors_from_coo(full, n, sweep.neighbors_slot_map(genes, nf), k)
    shared = [int(_lib.lib().fastf_neighbors_shared(idx[i].ctypes.data, int(cnt[i]), fidx[i].ctypes.data, int(fcnt[i]))) for i in range(n)]
    assert shared == M.hood(M.reference("asymmetric")[0], N.neighbor_sets(full, n, genes, k)[0])


# ---- the command line ----
@pytest.mark.parametrize("verb", ["sweep", "cap", "level"])
def test_the_help_text_names_the_option_and_its_table(verb):
    r = subprocess.run([_lib.cli_path(), verb, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "--mapping " in r.stdout and "%s_mapping.tsv" % verb in r.stdout and "mapping.tsv.gz" in r.stdout
    assert "-P" not in r.stdout                             # the long form alone


def _inputs(tmp_path):
    paths = [tmp_path / n for n in ("in.bam", "b.tsv", "f.tsv")]
    for p in paths:
        p.write_bytes(b"x\n")
    return paths


@pytest.mark.parametrize("verb,opt,val", [("sweep", "-r", "0.5"), ("cap", "-n", "5"), ("level", "-m", "5")])
def test_refused_with_several_devices_before_the_directory_is_made(tmp_path, verb, opt, val):
    bam, b, f = _inputs(tmp_path)
    out = tmp_path / "out"
    r = subprocess.run([_lib.cli_path(), verb, "-b", str(bam), "-a", str(b), "-f", str(f), "-o", str(out), "-c", "1", opt, val, "--mapping"], capture_output=True, text=True,
                       env=dict(os.environ, FASTF_DEVICES="0,1"))
    assert r.returncode == 1 and "%s: --mapping needs the resident form, and this job is outside it (several devices)" % verb in r.stderr, r.stderr
    assert not out.exists()
    r = subprocess.run([_lib.cli_path(), verb, "-b", str(bam), "-a", str(b), "-f", str(f), "-o", str(out), "-c", "1", opt, val, "--neighbors"], capture_output=True, text=True,
                       env=dict(os.environ, FASTF_DEVICES="0,1"))
    assert "%s: --neighbors needs the resident form, and this job is outside it (several devices)" % verb in r.stderr      # the same words
    r = subprocess.run([_lib.cli_path(), verb, "-b", str(bam), "-a", str(b), "-f", str(f), "-o", str(out), "-c", "1", opt, val, "-P"], capture_output=True, text=True)
    assert r.returncode == 1 and "unknown option `-P`" in r.stderr and not out.exists()


def test_the_entry_points_refuse_before_anything_is_written(tmp_path, monkeypatch):
    bam, b, f = _inputs(tmp_path)
    monkeypatch.setenv("FASTF_DEVICES", "0,1")
    for verb, values in (("sweep", [0.5]), ("cap", [5]), ("level", [5])):
        out = tmp_path / ("out_" + verb)
        with pytest.raises(F.FastfError, match="--mapping needs the resident form"):
            MOD[verb].__dict__[verb](bam, out, b, f, [1], values, mapping=True)
        with pytest.raises(F.FastfError, match="--mapping needs the resident form"):
            MOD[verb].__dict__[verb + "_reps"](bam, out, b, f, [1], values, [926, 5], mapping=True)
        assert not out.exists()
    monkeypatch.delenv("FASTF_DEVICES")
    L = _lib.lib()
    rc, rd = np.array([1], np.float32), np.array([0.5], np.float32)
    fp = rc.ctypes.data_as(_lib.C.POINTER(_lib.C.c_float))
    enc = lambda p: str(p).encode()      # noqa: E731
    out = tmp_path / "out_flags"
    for bit in (1024, 2048, 8192):                          # the path takes no flag bit: the unassigned bits stay refused
        assert L.fastf_sweep_mapping(enc(bam), enc(out), enc(b), enc(f), fp, 1, rd.ctypes.data_as(_lib.C.POINTER(_lib.C.c_float)), 1, None, 0, bit, 926, None, 0, 1) == 1
        assert "unknown flags" in F.lib().fastf_last_error().decode()
    assert L.fastf_sweep_mapping(enc(bam), enc(out), enc(b), enc(f), fp, 1, rd.ctypes.data_as(_lib.C.POINTER(_lib.C.c_float)), 1, None, 0, 0, 926, None, 0, 2) == 1
    assert "--mapping: 2, 0 or 1" in F.lib().fastf_last_error().decode()
    assert L.fastf_sweep_mapping(enc(bam), enc(out), enc(b), enc(f), fp, 1, rd.ctypes.data_as(_lib.C.POINTER(_lib.C.c_float)), 1, None, 0, 0, 926, None, 5, 1) == 1
    assert "--markers needs --labels" in F.lib().fastf_last_error().decode()
    assert not out.exists()
