"""--mapping on the GPU: fastf_dev_mapping in its MFMA and its plain form on the fixtures of mapping_ref against the reference and,
element by element, against the host twin — every (point planes, full planes) pair that is instantiated, guard words behind every
output, values behind every input that fail the call or change its result if read — and sweep, cap and level with the option, through
the CLI and in process: every row of mapping.tsv.gz and <verb>_mapping.tsv against mapping_ref on the decoded matrices of the tree."""
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import cap, hostmem, sweep
import labels_ref as LR
import mapping_ref as M
import neighbors_ref as N
import test_gpu_labels as TL
import test_labels_host as LH
import test_neighbors_host as H
from sweep_ref import parse_matrix

pytestmark = pytest.mark.gpu

GUARD32, GUARD64 = np.uint32(0xFFFFFFFF), np.uint64(0xFFFFFFFFFFFFFFFF)
FORMS = ("mfma", "plain")
MOD = TL.MOD


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
        monkeypatch.setenv("FASTF_MAPPING_MFMA", "0")
    else:
        monkeypatch.delenv("FASTF_MAPPING_MFMA", raising=False)


def _planes(eng, rows, n, nf, genes):
    """(the planes of a row set with 4096 bytes of 0x7F behind them, P)"""
    import torch
    K = len(genes)
    # behind the rows: rows of a gene of A in cell 1 whose count needs a fourth plane — read, they fail the call
    pads = (int(genes[0]) + 1 if K else 1, 1, 1 << 22)
    dev = [hostmem.to_device(np.concatenate([np.asarray(a, np.uint32), np.full(64, v, np.uint32)]), "cuda") for a, v in zip(rows, pads)]
    d_nnz = hostmem.to_device(np.array([len(rows[0])], np.uint64), "cuda")
    d_map = hostmem.to_device(sweep.neighbors_slot_map(genes, nf).view(np.uint8), "cuda")
    args = (dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), d_nnz.data_ptr(), d_map.data_ptr(), nf, n, K)
    P = eng.dev_neighbor_planes(*args)
    n_pad, K_pad = sweep.neighbors_pad(n, K)
    size = P * n_pad * K_pad
    d_planes = torch.full((size + 4096,), 0x7F, dtype=torch.uint8, device="cuda")
    assert eng.dev_neighbor_planes(*args, d_planes.data_ptr(), size) == P
    return d_planes, P


def _device_mapping(eng, full, point, n, nf, genes, k, want_planes=None):
    """(lists, self_dot, self_rank, hood against the full sets on the device, the raw idx and cnt) of one pair of row sets"""
    import torch
    K = len(genes)
    d_pf, PF = _planes(eng, full, n, nf, genes)
    d_pq, PQ = _planes(eng, point, n, nf, genes)
    assert want_planes is None or (PQ, PF) == want_planes
    d_fidx = torch.zeros((n * k + 1,), dtype=torch.int32, device="cuda")
    d_fcnt = torch.zeros((n + 1,), dtype=torch.int32, device="cuda")
    d_norms = torch.full((n + 64,), 1 << 50, dtype=torch.int64, device="cuda")      # (behind the norms: words that fail the range check if read)
    eng.dev_neighbors(d_pf.data_ptr(), PF, n, K, k, d_fidx.data_ptr(), d_fcnt.data_ptr(), d_norms.data_ptr())
    d_idx = torch.full((n * k + 64,), -1, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((n + 64,), -1, dtype=torch.int32, device="cuda")
    d_sd = torch.full((n + 8,), -1, dtype=torch.int64, device="cuda")
    d_rank = torch.full((n + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    max_q = eng.dev_mapping(d_pq.data_ptr(), PQ, d_pf.data_ptr(), PF, n, K, k, d_norms.data_ptr(), d_idx.data_ptr(), d_cnt.data_ptr(), d_sd.data_ptr(), d_rank.data_ptr())
    torch.cuda.synchronize()
    idx, cnt = hostmem.to_host(d_idx).view(np.uint32), hostmem.to_host(d_cnt).view(np.uint32)
    sd, rank = hostmem.to_host(d_sd).view(np.uint64), hostmem.to_host(d_rank).view(np.uint32)
    assert (idx[n * k:] == GUARD32).all() and (cnt[n:] == GUARD32).all() and (sd[n:] == GUARD64).all() and (rank[n:] == 0x5A5A5A5A).all(), "words behind an array were written"
    idx2 = idx[:n * k].reshape(n, k)
    assert (cnt[:n] <= k).all() and all((idx2[i, cnt[i]:] == GUARD32).all() for i in range(n))
    d_hood = torch.full((n + 64,), -1, dtype=torch.int32, device="cuda")
    eng.dev_neighbors_shared(d_idx.data_ptr(), d_cnt.data_ptr(), d_fidx.data_ptr(), d_fcnt.data_ptr(), n, k, d_hood.data_ptr())
    torch.cuda.synchronize()
    hood = hostmem.to_host(d_hood).view(np.uint32)
    assert (hood[n:] == GUARD32).all()
    my = N.dense(point, n, genes)
    assert max_q == max([int(v.dot(v)) for v in my], default=0)
    return H.as_lists(idx2, cnt[:n]), sd[:n], rank[:n], [int(v) for v in hood[:n]], idx2, cnt[:n]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", M.FIXTURES)
def test_the_fixtures_against_the_reference_and_the_host_twin(eng, name, form, monkeypatch):
    """`asymmetric` is the fixture with e_ij != e_ji for most pairs (census in mapping_ref): a swapped A/B operand or a transposed C/D row
    map gives other lists, ranks and self_dot there"""
    _form(monkeypatch, form)
    full, point, n, nf, genes, k = M.fixture(name)
    lists, sd, rank, _ = M.reference(name)
    got, got_sd, got_rank, hood, idx, cnt = _device_mapping(eng, full, point, n, nf, genes, k, (M.planes_needed(point, genes), M.planes_needed(full, genes)))
    assert got == lists
    assert [int(v) for v in got_sd] == sd and [None if int(v) == M.NONE else int(v) for v in got_rank] == rank
    assert hood == M.hood(lists, N.neighbor_sets(full, n, genes, k)[0])
    t_idx, t_cnt, t_sd, t_rank = sweep.mapping_from_coo(full, point, n, sweep.neighbors_slot_map(genes, nf), k)
    assert (idx == t_idx).all() and (cnt == t_cnt).all() and (got_sd == t_sd).all() and (got_rank == t_rank).all()


# the shapes: cells around the wave's 32 rows, the workgroup's 128 and two workgroups; genes around the K step of 32 bytes and the verbs'
# 2000; k at both ends; the plane pair (point, full) and k rotate through the shapes, so that every instantiated pair meets every kind of size
N_SIZES, K_SIZES, KS = (1, 2, 31, 32, 33, 63, 64, 65, 129, 257), (1, 31, 32, 33, 2000), (1, 15, 64)
PAIRS = ((1, 1), (1, 2), (2, 2), (1, 3), (2, 3), (3, 3))
PLANT = {1: 100, 2: 9000, 3: 300_000}                      # a count that needs exactly that many planes; 300000^2 + the rest stays below 2^42
SHAPES = [(n, K, KS[(5 * a + b) % 3], PAIRS[(5 * a + b) // 3 % 6]) for a, n in enumerate(N_SIZES) for b, K in enumerate(K_SIZES)]


_SHAPE_FIXTURES = {}


def _shape_fixture(n, K, planes):
    if (n, K) not in _SHAPE_FIXTURES:
        _SHAPE_FIXTURES[n, K] = _shape_fixture_build(n, K, planes)
    return _SHAPE_FIXTURES[n, K]


def _shape_fixture_build(n, K, planes):
    rng = np.random.default_rng(1000 * n + K)
    genes = rng.permutation(K + 5)[:K]
    density = 0.4 if K < 100 else 0.03
    mx = (rng.integers(1, 5, (n, K)) * (rng.random((n, K)) < density)).astype(np.int64)
    my = rng.binomial(mx, 0.5)
    at = int(rng.integers(0, K))
    mx[0, at], my[0, at] = PLANT[planes[1]], PLANT[planes[0]]      # cell 0 decides the planes of both sides
    return H.rows_of_dense(mx, genes, K + 5), H.rows_of_dense(my, genes, K + 5), K + 5, genes


def test_the_shapes_cover_every_pair_of_planes_and_every_k():
    assert {s[3] for s in SHAPES} == set(PAIRS) and {s[2] for s in SHAPES} == set(KS) and len(SHAPES) == 50
    assert {(s[3], s[2]) for s in SHAPES} == {(p, k) for p in PAIRS for k in KS}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n,K,k,planes", SHAPES)
def test_the_shapes_against_the_host_twin(eng, n, K, k, planes, form, monkeypatch):
    _form(monkeypatch, form)
    full, point, nf, genes = _shape_fixture(n, K, planes)
    got, got_sd, got_rank, hood, idx, cnt = _device_mapping(eng, full, point, n, nf, genes, k, planes)
    t_idx, t_cnt, t_sd, t_rank = sweep.mapping_from_coo(full, point, n, sweep.neighbors_slot_map(genes, nf), k)
    assert (got_sd == t_sd).all() and (got_rank == t_rank).all()
    assert (cnt == t_cnt).all() and (idx == t_idx).all()
    f_idx, f_cnt, _ = sweep.neighbors_from_coo(full, n, sweep.neighbors_slot_map(genes, nf), k)
    assert hood == [len(set(a) & set(b)) for a, b in zip(got, H.as_lists(f_idx, f_cnt))]


def test_the_refusals_of_the_device_call(eng):
    import torch
    full, point, n, nf, genes, k = M.fixture("asymmetric")
    K = len(genes)
    d_pf, PF = _planes(eng, full, n, nf, genes)
    d_out = torch.zeros((n * 64 + 64,), dtype=torch.int64, device="cuda")
    p = d_out.data_ptr()
    ok = torch.full((n,), 5, dtype=torch.int64, device="cuda")
    for bad_k in (0, 65):
        with pytest.raises(F.FastfError, match="k = %d, from 1 to 64" % bad_k):
            eng.dev_mapping(d_pf.data_ptr(), 1, d_pf.data_ptr(), 1, n, K, bad_k, ok.data_ptr(), p, p, p, p)
    with pytest.raises(F.FastfError, match="planes of the full rows, from 1 to 3"):
        eng.dev_mapping(d_pf.data_ptr(), 1, d_pf.data_ptr(), 4, n, K, 15, ok.data_ptr(), p, p, p, p)
    with pytest.raises(F.FastfError, match="2 planes of the point, from 1 to the 1 of the full rows"):
        eng.dev_mapping(d_pf.data_ptr(), 2, d_pf.data_ptr(), 1, n, K, 15, ok.data_ptr(), p, p, p, p)
    big = torch.full((n,), 5, dtype=torch.int64, device="cuda")
    big[n - 1] = 1 << 42                                    # the full side of the range rule: nothing is written
    with pytest.raises(F.FastfError, match="FASTF_ERR_NEIGHBOR_NORM"):
        eng.dev_mapping(d_pf.data_ptr(), 1, d_pf.data_ptr(), 1, n, K, 15, big.data_ptr(), p, p, p, p)
    # the point side: one cell with the counts 2^21 - 1 and 2^11 (norm 2^42 + 1) against a full side below the bound
    genes2, sm_nf = np.array([0, 1]), 2
    rows_big = (np.array([1, 2], np.uint32), np.array([1, 1], np.uint32), np.array([(1 << 21) - 1, 1 << 11], np.uint32))
    rows_ok = (np.array([1, 2], np.uint32), np.array([1, 1], np.uint32), np.array([(1 << 21) - 1, 1], np.uint32))
    d_q, PQ = _planes(eng, rows_big, 2, sm_nf, genes2)
    d_f, PF2 = _planes(eng, rows_ok, 2, sm_nf, genes2)
    norms = torch.tensor([((1 << 21) - 1) ** 2 + 1, 0], dtype=torch.int64, device="cuda")
    assert (PQ, PF2) == (3, 3)
    with pytest.raises(F.FastfError, match="FASTF_ERR_NEIGHBOR_NORM"):
        eng.dev_mapping(d_q.data_ptr(), 3, d_f.data_ptr(), 3, 2, 2, 15, norms.data_ptr(), p, p, p, p)
    torch.cuda.synchronize()
    assert int(d_out.abs().sum()) == 0
    assert eng.dev_mapping(d_f.data_ptr(), 3, d_f.data_ptr(), 3, 2, 2, 15, norms.data_ptr(), p, p + 4096, p + 8192, p + 12288) == ((1 << 21) - 1) ** 2 + 1
    assert eng.dev_mapping(0, 1, 0, 1, 0, 5, 15, 0, 0, 0, 0, 0) == 0      # no cells: nothing is launched


# ---- the commands ----
_REF = {}


def _reference_point(case, full_rows, point_rows, barcodes, with_labels):
    key = (full_rows[2].tobytes(), point_rows[0].tobytes(), point_rows[1].tobytes(), point_rows[2].tobytes(), with_labels)
    if key not in _REF:
        n = len(barcodes)
        A = N.hvg_of_rows(full_rows, n, 45)
        lists, sd, rank, _ = M.mapping(full_rows, point_rows, n, A)
        full_sets = N.neighbor_sets(full_rows, n, A)[0]
        names, ids = LR.label_ids(case.pairs)
        lab = [ids.get(bc, 0) for bc in barcodes] if with_labels else None
        votes = LR.votes(lists, lab, len(names) - 1) if with_labels else None
        _REF[key] = (len(A), lists, sd, rank, full_sets, names if with_labels else None, lab, votes)
    return _REF[key]


def _check_outputs(out, case, verb, rates, values, with_labels, seeds=(926,), reps=False, written=None):
    """written: a tree of the same run without --summary-only whose matrices give the reference (summary-only runs write none)"""
    lines = open(out / ("%s_mapping.tsv" % verb)).read().split("\n")
    assert lines[0].split("\t") == list(MOD[verb].MAPPING_COLUMNS) and lines[-1] == "" and len(lines) - 2 == len(rates) * len(values) * len(seeds)
    at = 1
    for rc in rates:
        for seed in seeds:
            full_rows, barcodes = case.matrix(rc, 1, seed)
            for v in values:
                name = MOD[verb].point_dir(rc, v) + ("_s%d" % seed if reps else "")
                d = (written or out) / name
                point_rows = parse_matrix(TL._gz(d / "matrix.mtx.gz"))[3:]
                assert TL._gz(d / "barcodes.tsv.gz").decode().split("\n")[:-1] == barcodes
                hvg_k, lists, sd, rank, full_sets, names, lab, votes = _reference_point(case, full_rows, point_rows, barcodes, with_labels)
                lead = ["%.3f" % rc, "%.3f" % v if verb == "sweep" else str(int(v))]
                N.assert_fields(lines[at].split("\t"), M.summary_fields(lead, seed, hvg_k, 15, lists, sd, rank, full_sets, lab, votes), 7, (verb, rc, seed, v))
                at += 1
                if written:
                    assert not (out / name).exists()
                    continue
                got = TL._gz(d / "mapping.tsv.gz").decode().split("\n")
                assert got[0].split("\t") == list(sweep.POINT_MAPPING_COLUMNS) and got[-1] == ""
                assert [g.split("\t") for g in got[1:-1]] == M.cell_rows(barcodes, lists, sd, rank, full_sets, names, votes[0] if votes else None)
                assert [r["barcode"] for r in sweep.read_point_mapping(d / "mapping.tsv.gz")] == barcodes
    assert not [n for n in os.listdir(out) if n.endswith(".partial")]


def _is_new(name, verb):
    return name == "%s_mapping.tsv" % verb or os.path.basename(name) == "mapping.tsv.gz"


@pytest.mark.parametrize("verb", ["sweep", "cap", "level"])
def test_cli_with_the_option_alone_and_the_same_tree_without(tmp_path, verb):
    case = LH.labcase()
    bam, b, f, lf = TL._write(tmp_path, case)
    rates, values = [0.5, 1], TL.GRID[verb]
    out, out0 = tmp_path / "out", tmp_path / "out0"
    r = subprocess.run(TL._args(verb, bam, b, f, out, rates, values) + ["--mapping"], capture_output=True, text=True, timeout=600, env=dict(os.environ, FASTF_PROFILE="1"))
    assert r.returncode == 0, r.stderr
    assert "%s_mapping.tsv is generated." % verb in r.stdout and "[%s] --mapping:" % verb in r.stderr
    assert "neighbors.tsv is generated." not in r.stdout and "] --neighbors:" not in r.stderr
    _check_outputs(out, case, verb, rates, values, False)
    rows = MOD[verb].read_mapping_table(out / ("%s_mapping.tsv" % verb))
    assert rows[0]["cells_labelled"] == "NA" and rows[0]["accuracy_map"] == "NA" and rows[0]["k"] == "15"
    r = subprocess.run(TL._args(verb, bam, b, f, out0, rates, values), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    with_opt, without = TL._tree(out), TL._tree(out0)
    new = {n for n in with_opt if _is_new(n, verb)}
    assert len(new) == 1 + len(rates) * len(values) and not [n for n in with_opt if "neighbors" in n or "labels" in n]
    assert {n: v for n, v in with_opt.items() if n not in new} == without


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("verb", ["sweep", "cap", "level"])
def test_in_process_with_labels_and_summary_only(tmp_path, verb, form, monkeypatch):
    _form(monkeypatch, form)
    case = LH.labcase()
    bam, b, f, lf = TL._write(tmp_path, case)
    rates, values = [1], TL.GRID[verb]
    out, out2 = tmp_path / "out", tmp_path / "out2"
    MOD[verb].__dict__[verb](bam, out, b, f, rates, values, seed=926, labels=lf, mapping=True)
    _check_outputs(out, case, verb, rates, values, True)
    rows = MOD[verb].read_mapping_table(out / ("%s_mapping.tsv" % verb))
    assert rows[0]["cells_labelled"] != "NA" and rows[0]["accuracy_map"] != "NA"
    MOD[verb].__dict__[verb](bam, out2, b, f, rates, values, seed=926, labels=lf, mapping=True, summary_only=True)
    _check_outputs(out2, case, verb, rates, values, True, written=out)
    assert sorted(os.listdir(out2)) == sorted(["%s.tsv" % verb, "%s_mapping.tsv" % verb, "%s_labels.tsv" % verb, "%s_label_classes.tsv" % verb])
    assert open(out2 / ("%s_mapping.tsv" % verb)).read() == open(out / ("%s_mapping.tsv" % verb)).read()


@pytest.mark.parametrize("verb", ["sweep", "cap", "level"])
def test_beside_the_other_comparisons(tmp_path, verb):
    """the plane buffer, the norms and the neighbour sets are shared with --neighbors, --labels and --markers: their files stay what they are"""
    case = LH.labcase()
    bam, b, f, lf = TL._write(tmp_path, case)
    rates, values = [0.5], TL.GRID[verb]
    out, out0 = tmp_path / "out", tmp_path / "out0"
    others = ["--neighbors", "--labels", str(lf), "--markers", "5", "--coexpression", "--fidelity"]
    for o, extra in ((out, ["--mapping"]), (out0, [])):
        r = subprocess.run(TL._args(verb, bam, b, f, o, rates, values) + others + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
    _check_outputs(out, case, verb, rates, values, True)
    with_opt, without = TL._tree(out), TL._tree(out0)
    assert {n: v for n, v in with_opt.items() if not _is_new(n, verb)} == without and len(with_opt) == len(without) + 1 + len(rates) * len(values)
    assert all(any(n.endswith(e) for n in without) for e in ("neighbors.tsv.gz", "labels.tsv.gz", "markers.tsv.gz", "coexpr.tsv.gz", "/fidelity.tsv.gz"))


def test_two_seeds_give_one_row_per_cell_rate_seed_and_value(tmp_path):
    case = LH.labcase()
    bam, b, f, lf = TL._write(tmp_path, case)
    out = tmp_path / "out"
    r = subprocess.run(TL._args("sweep", bam, b, f, out, [0.5], [0.1, 1]) + ["--mapping", "--seeds", "926,5"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    _check_outputs(out, case, "sweep", [0.5], [0.1, 1], False, seeds=(926, 5), reps=True)
    rows = sweep.read_mapping_table(out / "sweep_mapping.tsv")
    assert [x["seed"] for x in rows] == ["926", "926", "5", "5"] and rows[0] != rows[2]
    assert not [n for n in os.listdir(out) if "mapping_reps" in n]
    out2 = tmp_path / "out2"
    cap.cap_reps(bam, out2, b, f, [0.5], TL.GRID["cap"][:1], [926], mapping=True)
    _check_outputs(out2, case, "cap", [0.5], TL.GRID["cap"][:1], False, seeds=(926,), reps=True)
