"""--neighbors on the GPU: the three device calls (fastf_dev_neighbor_planes, fastf_dev_neighbors in its MFMA and its plain form,
fastf_dev_neighbors_shared) on the fixtures of test_neighbors_host against neighbors_ref — guard words behind every output, rows behind
every input that must not be read — and sweep, cap and level with the flag, through the CLI and in process: every row of
neighbors.tsv.gz and <verb>_neighbors.tsv against the reference built on the unchanged oracle (integer columns exactly, the printed
ratios within fidelity_ref.TOL absolute)."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import cap, hostmem, level, sweep
from helpers import Case
from oracle import oracle as O
import cap_ref
import level_ref
import neighbors_ref as N
from test_gpu_sweep import _write
import test_gpu_gene_fidelity as TG
import test_neighbors_host as H

pytestmark = pytest.mark.gpu

GUARD32, GUARD64 = np.uint32(0xFFFFFFFF), np.uint64(0xFFFFFFFFFFFFFFFF)
FORMS = ("mfma", "plain")


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
    if form == "plain":
        monkeypatch.setenv("FASTF_NEIGHBORS_MFMA", "0")
    else:
        monkeypatch.delenv("FASTF_NEIGHBORS_MFMA", raising=False)


def _device_sets(eng, rows, n, nf, genes, k, want_planes=None):
    """the planes and the neighbour sets of one row set: (lists, norms, max norm, the device tensors of idx and cnt)"""
    import torch
    K = len(genes)
    sm = sweep.neighbors_slot_map(genes, nf)
    # behind the rows: 300 rows of a gene of A in cell 1 whose count needs a fourth plane — read, they fail the call
    pads = (int(genes[0]) + 1 if K else 1, 1, 1 << 22)
    dev = [hostmem.to_device(np.concatenate([np.asarray(a, np.uint32), np.full(300, v, np.uint32)]), "cuda") for a, v in zip(rows, pads)]
    d_nnz = hostmem.to_device(np.array([len(rows[0])], np.uint64), "cuda")
    d_map = hostmem.to_device(np.concatenate([sm, np.zeros(64, np.uint16)]).view(np.uint8), "cuda")     # (slot 0 behind the map)
    args = (dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), d_nnz.data_ptr(), d_map.data_ptr(), nf, n, K)
    P = eng.dev_neighbor_planes(*args)
    assert 1 <= P <= 3 and (want_planes is None or P == want_planes)
    n_pad, K_pad = sweep.neighbors_pad(n, K)
    assert n_pad % 128 == 0 and K_pad % 32 == 0 and n_pad >= n and K_pad >= K
    size = P * n_pad * K_pad
    d_planes = torch.full((size + 256,), 0xEE, dtype=torch.uint8, device="cuda")
    with pytest.raises(F.FastfError, match="the buffer has"):
        eng.dev_neighbor_planes(*args, d_planes.data_ptr(), size - 1)
    assert eng.dev_neighbor_planes(*args, d_planes.data_ptr(), size) == P
    torch.cuda.synchronize()
    planes = hostmem.to_host(d_planes)
    assert (planes[size:] == 0xEE).all(), "bytes behind the planes were written"
    m = N.dense(rows, n, genes).astype(np.int64)
    want = np.zeros((P, n_pad, K_pad), np.uint8)
    for p in range(P):
        want[p, :n, :max(K, 1)] = (m >> (7 * p)) & 127
    assert (planes[:size].reshape(P, n_pad, K_pad) == want).all()
    d_idx = torch.full((n * k + 64,), -1, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((n + 64,), -1, dtype=torch.int32, device="cuda")
    d_norms = torch.full((n + 8,), -1, dtype=torch.int64, device="cuda")
    max_norm = eng.dev_neighbors(d_planes.data_ptr(), P, n, K, k, d_idx.data_ptr(), d_cnt.data_ptr(), d_norms.data_ptr())
    torch.cuda.synchronize()
    idx, cnt, norms = hostmem.to_host(d_idx).view(np.uint32), hostmem.to_host(d_cnt).view(np.uint32), hostmem.to_host(d_norms).view(np.uint64)
    assert (idx[n * k:] == GUARD32).all() and (cnt[n:] == GUARD32).all() and (norms[n:] == GUARD64).all(), "words behind an array were written"
    idx2 = idx[:n * k].reshape(n, k)
    assert (cnt[:n] <= k).all() and all((idx2[i, cnt[i]:] == GUARD32).all() for i in range(n))
    return H.as_lists(idx2, cnt[:n]), [int(v) for v in norms[:n]], max_norm, (d_idx, d_cnt)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sorted(H.DEVICE_FIXTURES))
def test_planes_and_neighbours_against_the_reference(eng, name, form, monkeypatch):
    _form(monkeypatch, form)
    rows, n, nf, genes, k = H.fixture(name)
    sets, norms = H.reference(name)
    got, got_norms, max_norm, _ = _device_sets(eng, rows, n, nf, genes, k, H.planes_needed(name))
    assert got_norms == norms and max_norm == max(norms, default=0)
    assert got == sets


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["n65", "n257", "duplicates", "scaled", "zero_and_outside", "count16384"])
def test_shared_counts_and_the_host_twin(eng, name, form, monkeypatch):
    """the point: every count above 1 lowered by one, every third row dropped — its sets against the full ones on the device"""
    import torch
    _form(monkeypatch, form)
    rows, n, nf, genes, k = H.fixture(name)
    keep = np.arange(len(rows[0])) % 3 != 2
    point = (rows[0][keep], rows[1][keep], (rows[2] - (rows[2] > 1))[keep])
    full_sets, _ = H.reference(name)
    point_sets, _ = N.neighbor_sets(point, n, genes, k)
    a, _, _, (ai, ac) = _device_sets(eng, rows, n, nf, genes, k)
    b, _, _, (bi, bc) = _device_sets(eng, point, n, nf, genes, k)
    assert a == full_sets and b == point_sets
    d_sh = torch.full((n + 64,), -1, dtype=torch.int32, device="cuda")
    eng.dev_neighbors_shared(ai.data_ptr(), ac.data_ptr(), bi.data_ptr(), bc.data_ptr(), n, k, d_sh.data_ptr())
    torch.cuda.synchronize()
    sh = hostmem.to_host(d_sh).view(np.uint32)
    assert (sh[n:] == GUARD32).all()
    assert [int(v) for v in sh[:n]] == N.per_cell(full_sets, point_sets)[2]
    idx, cnt, _ = sweep.neighbors_from_coo(point, n, sweep.neighbors_slot_map(genes, nf), k)
    assert H.as_lists(idx, cnt) == point_sets


def test_the_refusals_of_the_device_calls(eng):
    rows, n, nf, genes, k = H.fixture("n33")
    big = (rows[0], rows[1], np.where(np.arange(len(rows[2])) == 5, 1 << 21, rows[2]).astype(np.uint32))
    dev = [hostmem.to_device(np.asarray(a, np.uint32), "cuda") for a in big]
    d_nnz = hostmem.to_device(np.array([len(big[0])], np.uint64), "cuda")
    d_map = hostmem.to_device(sweep.neighbors_slot_map(genes, nf).view(np.uint8), "cuda")
    assert big[0][5] - 1 in genes
    with pytest.raises(F.FastfError, match="FASTF_ERR_NEIGHBOR_COUNT"):
        eng.dev_neighbor_planes(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), d_nnz.data_ptr(), d_map.data_ptr(), nf, n, len(genes))
    for bad_k in (0, 65):
        with pytest.raises(F.FastfError, match="from 1 to 64"):
            eng.dev_neighbors(d_map.data_ptr(), 1, n, len(genes), bad_k, d_map.data_ptr(), d_map.data_ptr(), d_map.data_ptr())
    with pytest.raises(F.FastfError, match="planes, from 1 to 3"):
        eng.dev_neighbors(d_map.data_ptr(), 4, n, len(genes), 15, d_map.data_ptr(), d_map.data_ptr(), d_map.data_ptr())
    assert eng.dev_neighbors(0, 1, 0, 5, 15, 0, 0, 0) == 0  # no cells: nothing is launched


# ---- the commands ----
_POINTS, _PAIRS = {}, {}
MOD, OPT = TG.MOD, TG.OPT


def _pair(name, rc, seed):
    key = (name, float(rc), seed)
    if key not in _PAIRS:
        case = TG._case(name)
        full, n_cells, _, nf, hits = N.full_matrix(name, case, rc, seed)
        barcodes = hits.ora_full["barcodes"].decode().split("\n")[:-1]
        assert len(barcodes) == n_cells
        A = N.hvg_of_rows(full, n_cells, nf)
        _PAIRS[key] = (case, hits, barcodes, n_cells, A, N.neighbor_sets(full, n_cells, A)[0])
    return _PAIRS[key]


def _point(name, verb, rc, value, seed=926):
    """the reference of one point: (the fields of its neighbors.tsv.gz rows, the fields of its table row)"""
    key = (name, verb, float(rc), float(value), seed)
    if key not in _POINTS:
        case, hits, barcodes, n_cells, A, full_sets = _pair(name, rc, seed)
        if verb == "sweep":
            ora = O.run_bam2db(case.bt, case.ft, case.flags, case.xf, case.cb, case.gx, case.ub, float(np.float32(rc)), float(np.float32(value)), seed, b"x.bam", False)
            rows, lead = TG._rows_of(ora["matrix"]), ["%.3f" % rc, "%.3f" % value]
        elif verb == "cap":
            rows, lead = TG._rows_of(cap_ref.point(case, b"x.bam", rc, value, seed)["matrix"]), ["%.3f" % rc, str(int(value))]
        else:
            rows, lead = TG._rows_of(level_ref.point(hits, value)["matrix"]), ["%.3f" % rc, str(int(value))]
        kf, kp, sh = N.per_cell(full_sets, N.neighbor_sets(rows, n_cells, A)[0])
        _POINTS[key] = (N.cell_rows(barcodes, kf, kp, sh), N.summary_fields(lead, seed, len(A), 15, kf, kp, sh))
    return _POINTS[key]


def _gz(p):
    return gzip.decompress(open(p, "rb").read())


def _check_outputs(out, name, verb, rates, values, seeds=(926,), reps=False, summary_only=False):
    lines = open(out / ("%s_neighbors.tsv" % verb)).read().split("\n")
    assert lines[0].split("\t") == list(MOD[verb].NEIGHBORS_COLUMNS) and lines[-1] == ""
    assert len(lines) - 2 == len(rates) * len(values) * len(seeds)
    at = 1
    for rc in rates:
        for seed in seeds:
            for v in values:
                cells, row = _point(name, verb, rc, v, seed)
                N.assert_fields(lines[at].split("\t"), row, 7, (verb, rc, seed, v))
                at += 1
                d = out / (MOD[verb].point_dir(rc, v) + ("_s%d" % seed if reps else ""))
                if summary_only:
                    assert not d.exists()
                    continue
                got = _gz(d / "neighbors.tsv.gz").decode().split("\n")
                assert got[0].split("\t") == list(sweep.POINT_NEIGHBORS_COLUMNS) and got[-1] == "" and len(got) - 2 == len(cells)
                for g, w in zip(got[1:-1], cells):
                    N.assert_fields(g.split("\t"), w, 4, (verb, rc, seed, v))
                assert _gz(d / "barcodes.tsv.gz").decode().split("\n")[:-1] == [c[0] for c in cells]
                assert [r["barcode"] for r in sweep.read_point_neighbors(d / "neighbors.tsv.gz")] == [c[0] for c in cells]
    assert not [n for n in os.listdir(out) if n.endswith(".partial")]


@pytest.mark.parametrize("name", ["edge", "mixed"])
@pytest.mark.parametrize("verb", ["sweep", "cap", "level"])
def test_cli_with_the_flag_and_the_same_tree_without_it(tmp_path, verb, name):
    bam, b, f = _write(tmp_path, TG._case(name))
    rates, values = TG._grid(name, verb)
    out, out0 = tmp_path / "out", tmp_path / "out0"
    r = subprocess.run(TG._args(verb, bam, b, f, out, rates, values) + ["--neighbors"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, FASTF_PROFILE="1"))
    assert r.returncode == 0, r.stderr
    assert "%s_neighbors.tsv is generated." % verb in r.stdout and "[%s] --neighbors:" % verb in r.stderr
    assert "fidelity.tsv is generated." not in r.stdout and "fidelity:" not in r.stderr
    _check_outputs(out, name, verb, rates, values)
    r = subprocess.run(TG._args(verb, bam, b, f, out0, rates, values), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    with_flag, without = TG._tree(out), TG._tree(out0)
    new = {n for n in with_flag if n == "%s_neighbors.tsv" % verb or os.path.basename(n) == "neighbors.tsv.gz"}
    assert len(new) == 1 + len(rates) * len(values) and not [n for n in without if "neighbors" in n or "fidelity" in n]
    assert {n: v for n, v in with_flag.items() if n not in new} == without


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["edge", "mixed"])
@pytest.mark.parametrize("verb", ["sweep", "cap", "level"])
def test_in_process(tmp_path, verb, name, form, monkeypatch):
    _form(monkeypatch, form)
    bam, b, f = _write(tmp_path, TG._case(name))
    rates, values = TG._grid(name, verb)
    out = tmp_path / "out"
    MOD[verb].__dict__[verb](bam, out, b, f, rates, values, seed=926, neighbors=True)
    _check_outputs(out, name, verb, rates, values)
    rows = MOD[verb].read_neighbors_table(out / ("%s_neighbors.tsv" % verb))
    assert len(rows) == len(rates) * len(values) and rows[0]["seed"] == "926" and rows[0]["k"] == "15"
    if name == "mixed":                                     # the deepest point of the grid is the full matrix itself
        last = rows[-1]
        assert last["median_overlap"] == "1.000000" and last["p10_overlap"] == "1.000000" and last["mean_overlap"] == "1.000000"
        assert float(rows[0]["mean_overlap"]) < 1 and int(rows[0]["hvg_k"]) > 100
    out2 = tmp_path / "out2"
    MOD[verb].__dict__[verb](bam, out2, b, f, rates, values, seed=926, neighbors=True, summary_only=True)
    _check_outputs(out2, name, verb, rates, values, summary_only=True)
    assert sorted(os.listdir(out2)) == sorted(["%s.tsv" % verb, "%s_neighbors.tsv" % verb])
    assert open(out2 / ("%s_neighbors.tsv" % verb)).read() == open(out / ("%s_neighbors.tsv" % verb)).read()


@pytest.mark.parametrize("verb", ["sweep", "cap", "level"])
def test_with_the_other_flags_together(tmp_path, verb):
    """--cells' K3u writes the row buffer the planes are made from, --gene-fidelity shares the pair's per-gene sums, --fidelity the full
    rows: every file of the other flags stays what it is"""
    bam, b, f = _write(tmp_path, TG._case("mixed"))
    rates, values = TG._grid("mixed", verb)
    out, out0 = tmp_path / "out", tmp_path / "out0"
    for o, extra in ((out, ["--neighbors"]), (out0, [])):
        r = subprocess.run(TG._args(verb, bam, b, f, o, rates, values) + ["--fidelity", "--gene-fidelity", "--cells", "--genes"] + extra, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr
    _check_outputs(out, "mixed", verb, rates, values)
    with_flag, without = TG._tree(out), TG._tree(out0)
    assert {n: v for n, v in with_flag.items() if "neighbors" not in n} == without and len(with_flag) == len(without) + 1 + len(rates) * len(values)
    assert all(any(n.endswith(e) for n in without) for e in ("cells.tsv.gz", "genes.tsv.gz", "/fidelity.tsv.gz", "/gene_fidelity.tsv.gz"))


def test_two_seeds_give_one_row_per_cell_rate_seed_and_value(tmp_path):
    bam, b, f = _write(tmp_path, TG._case("mixed"))
    out = tmp_path / "out"
    r = subprocess.run(TG._args("sweep", bam, b, f, out, [0.5], [0.1, 1]) + ["--neighbors", "--seeds", "926,5"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    _check_outputs(out, "mixed", "sweep", [0.5], [0.1, 1], seeds=(926, 5), reps=True)
    rows = sweep.read_neighbors_table(out / "sweep_neighbors.tsv")
    assert [x["seed"] for x in rows] == ["926", "926", "5", "5"] and rows[0] != rows[2]
    assert not [n for n in os.listdir(out) if "neighbors_reps" in n]
    out2 = tmp_path / "out2"
    cap.cap_reps(bam, out2, b, f, [0.5], TG._grid("mixed", "cap")[1][:1], [926], neighbors=True, summary_only=True)
    _check_outputs(out2, "mixed", "cap", [0.5], TG._grid("mixed", "cap")[1][:1], seeds=(926,), reps=True, summary_only=True)


def test_refusal_of_20_base_umis_leaves_no_table(tmp_path):
    """20-base UMIs do not fit a 64-bit key: the full rows live on the device alone, so sweep does not fall back with the flag"""
    case = Case(n=30_000, n_bar=400, n_gene=150, umi_len=20, umi_pool=512, p_n_umi=0.02, p_bad_xf=0.1, data_seed=35)
    bam, b, f = _write(tmp_path, case)
    for verb, v in (("sweep", [0.5]), ("cap", [5]), ("level", [5])):
        out = tmp_path / ("out_" + verb)
        r = subprocess.run(TG._args(verb, bam, b, f, out, [1], v) + ["--neighbors"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 1 and "outside" in r.stderr and "point by point" not in r.stderr.replace("no point-by-point", ""), r.stderr
        assert "%s: --neighbors needs the resident form" % verb in r.stderr
        assert [n for n in os.listdir(out) if n.startswith(verb)] == []
    with pytest.raises(F.FastfError, match="--neighbors needs the resident form"):
        sweep.sweep(bam, tmp_path / "outp", b, f, [1], [1], neighbors=True)
    assert not (tmp_path / "outp" / "sweep.tsv").exists()
