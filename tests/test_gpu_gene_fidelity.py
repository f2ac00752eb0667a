"""--gene-fidelity on the GPU: the partner counts (fastf_dev_partner_counts) and the per-gene moments (fastf_dev_gene_moments, both forms)
on the hand-built rows of test_gene_fidelity_host against gene_fidelity_ref, and sweep, cap and level with the flag — through the CLI
and in process — every gene_fidelity.tsv.gz and <verb>_gene_fidelity.tsv row against the reference built on the unchanged oracle:
integer columns exactly, float columns within fidelity_ref.TOL absolute."""
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
import gene_fidelity_ref as G
import level_ref
from sweep_ref import parse_matrix
from test_gpu_sweep import _Edge, _write
import test_gene_fidelity_host as H

pytestmark = pytest.mark.gpu

GUARD32, GUARD64 = np.uint32(0xFFFFFFFF), np.uint64(0xFFFFFFFFFFFFFFFF)


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
    return [hostmem.to_device(np.concatenate([a, np.full(300, v, np.uint32)]), "cuda") for a, v in ((f, pad_key[1]), (c, pad_key[0]), (k, 7))]


def _partners(eng, full, point, expect_error=False):
    import torch
    n, m = len(point[0]), len(full[0])
    xd = _dev_rows(full, (1, 1))                            # behind the full rows: (cell 1, feature 1) again and again
    yd = _dev_rows(point, (0xFFFFFFF0, 9))                  # behind the point rows: rows of a cell nobody has
    d_m, d_n = hostmem.to_device(np.array([m], np.uint64), "cuda"), hostmem.to_device(np.array([n], np.uint64), "cuda")
    d_x = torch.full((n + 64,), -1, dtype=torch.int32, device="cuda")
    d_err = hostmem.to_device(np.array([0, 0xFFFFFFFFFFFFFFFF], np.uint64), "cuda")
    call = lambda: eng.dev_partner_counts(xd[0].data_ptr(), xd[1].data_ptr(), xd[2].data_ptr(), d_m.data_ptr(), yd[0].data_ptr(), yd[1].data_ptr(),  # noqa: E731
                                          d_n.data_ptr(), d_x.data_ptr(), d_err.data_ptr())
    if expect_error:
        with pytest.raises(F.FastfError, match="no partner"):
            call()
    else:
        call()
    torch.cuda.synchronize()
    x, err = hostmem.to_host(d_x).view(np.uint32), hostmem.to_host(d_err).view(np.uint64)
    assert (x[n:] == GUARD32).all() and err[1] == GUARD64, "words behind an array were written"
    assert int(err[0]) == (32 if expect_error else 0)
    return x[:n]


@pytest.mark.parametrize("name", H.PARTNER_FIXTURES)
def test_partner_counts(eng, name):
    full, point = H.partner_fixture(name, _waves())
    want = G.partner_counts(full, point)
    got = _partners(eng, full, point)
    assert len(got) == len(want) and (got.astype(np.int64) == want).all()
    if name.startswith("rows"):
        assert len(point[0]) == H.partner_row_counts(_waves())[int(name[4:])]


@pytest.mark.parametrize("name", H.MISSING_FIXTURES)
def test_a_missing_partner_is_reported_stores_zero_and_leaves_the_other_rows_right(eng, name):
    full, point = H.partner_fixture(name, _waves())
    kx, ky = G.R._keys(full[1], full[0]), G.R._keys(point[1], point[0])
    has = np.isin(ky, kx)
    want = np.zeros(len(ky), np.int64)
    if len(kx):
        want[has] = np.asarray(full[2], np.int64)[np.searchsorted(kx, ky[has])]
    got = _partners(eng, full, point, expect_error=True)
    assert (got.astype(np.int64) == want).all() and (~has).sum() == (len(ky) if name == "no_full_rows" else 1)
    with pytest.raises(F.FastfError, match="no partner"):   # the host twin says the same
        sweep.gene_fidelity_from_coo(full, point, 900)


def _moments(eng, f, a, b, nf, want_ab=True):
    import torch
    n = len(f)
    dev = [hostmem.to_device(np.concatenate([np.asarray(v, np.uint32), np.full(300, pad, np.uint32)]), "cuda") for v, pad in ((f, 1), (a, 7), (b, 7))]
    d_n = hostmem.to_device(np.array([n], np.uint64), "cuda")
    d_ab = torch.full((nf + 2,), -1, dtype=torch.int64, device="cuda")
    d_bb = torch.full((nf + 2,), -1, dtype=torch.int64, device="cuda")
    eng.dev_gene_moments(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), d_n.data_ptr(), nf, d_ab.data_ptr() if want_ab else 0, d_bb.data_ptr())
    torch.cuda.synchronize()
    ab, bb = (hostmem.to_host(t).view(np.uint64) for t in (d_ab, d_bb))
    if not want_ab:                                         # no sum_ab asked for: its array is not touched
        assert (ab == GUARD64).all() and (bb[nf:] == GUARD64).all()
        return None, [int(v) for v in bb[:nf]]
    assert (ab[nf:] == GUARD64).all() and (bb[nf:] == GUARD64).all(), "words behind an array were written"
    return [int(v) for v in ab[:nf]], [int(v) for v in bb[:nf]]


_MOMENT_REFS = {}


@pytest.mark.parametrize("form", ["lds", "general"])
@pytest.mark.parametrize("name", H.MOMENT_FIXTURES)
def test_gene_moments(eng, name, form, monkeypatch):
    f, a, b, nf = H.moments_fixture(name)
    if name not in _MOMENT_REFS:
        _MOMENT_REFS[name] = G.gene_sums(f, a, b, nf)
    if form == "general":
        monkeypatch.setenv("FASTF_GENE_MOMENTS_LDS_RANGES", "0")
    else:
        monkeypatch.delenv("FASTF_GENE_MOMENTS_LDS_RANGES", raising=False)
    assert _moments(eng, f, a, b, nf) == _MOMENT_REFS[name]


def test_gene_moments_with_fewer_ranges_allowed_than_the_list_needs(eng, monkeypatch):
    """five ranges needed, four allowed: the general form; five allowed: the LDS form — the same sums"""
    f, a, b, nf = H.moments_fixture("list36601")
    want = G.gene_sums(f, a, b, nf)
    for k in ("4", "5"):
        monkeypatch.setenv("FASTF_GENE_MOMENTS_LDS_RANGES", k)
        assert _moments(eng, f, a, b, nf) == want


@pytest.mark.parametrize("form", ["lds", "general"])
@pytest.mark.parametrize("name", ["list3", "list8193", "list36601", "one_gene", "big", "rows65"])
def test_gene_moments_without_sum_ab(eng, name, form, monkeypatch):
    """d_sum_ab == NULL (the once-per-pair sum_xx call): sum_bb alone, the same numbers"""
    f, a, b, nf = H.moments_fixture(name)
    if form == "general":
        monkeypatch.setenv("FASTF_GENE_MOMENTS_LDS_RANGES", "0")
    else:
        monkeypatch.delenv("FASTF_GENE_MOMENTS_LDS_RANGES", raising=False)
    assert _moments(eng, f, a, b, nf, want_ab=False)[1] == G.gene_sums(f, a, b, nf)[1]


@pytest.mark.parametrize("want_ab", [True, False])
@pytest.mark.parametrize("n_features", [H.LDS_LIMIT, H.LDS_LIMIT + 1])
def test_gene_moments_at_the_last_lds_range(eng, n_features, want_ab, monkeypatch):
    """131 072 genes: sixteen ranges, the most the LDS form takes; one gene more goes to the general form"""
    monkeypatch.delenv("FASTF_GENE_MOMENTS_LDS_RANGES", raising=False)
    f, a, b = H.last_range_fixture(n_features)
    if n_features not in _MOMENT_REFS:
        _MOMENT_REFS[n_features] = G.gene_sums(f, a, b, n_features)
    want = _MOMENT_REFS[n_features]
    got = _moments(eng, f, a, b, n_features, want_ab=want_ab)
    assert got == want if want_ab else got[1] == want[1]


def test_the_three_calls_give_the_seven_arrays_of_the_host_twin(eng):
    """partner counts, then the moments on (Y, x of y, y) and (X, x, x): what resident.c chains behind a point"""
    import torch
    rng = np.random.default_rng(11)
    nf = 900
    full = H.sorted_rows(rng, 20_000, 90, n_features=nf)
    point = H.subset(rng, full, 0.5)
    mom = G.moments(full, point, nf)
    x = _partners(eng, full, point)
    assert _moments(eng, point[0], x, point[2], nf) == (mom["sum_xy"], mom["sum_yy"])
    assert _moments(eng, full[0], full[2], full[2], nf) == (mom["sum_xx"], mom["sum_xx"])
    assert _moments(eng, full[0], full[2], full[2], nf, want_ab=False)[1] == mom["sum_xx"]
    twin = sweep.gene_fidelity_from_coo(full, point, nf)
    assert all([int(v) for v in twin[k]] == mom[c] for k, c in enumerate(G.INT_COLUMNS))
    torch.cuda.synchronize()


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
    """the reference of one point: (the fields of its gene_fidelity.tsv.gz rows, the fields of its table row)"""
    key = (name, verb, float(rc), float(value), seed)
    if key not in _POINTS:
        case = _case(name)
        full, n_cells, _, nf, hits = G.full_matrix(name, case, rc, seed)
        ids = [ln.split("\t")[0] for ln in hits.ora_full["features"].decode().split("\n")[:-1]]
        assert len(ids) == nf
        if verb == "sweep":
            ora = O.run_bam2db(case.bt, case.ft, case.flags, case.xf, case.cb, case.gx, case.ub, float(np.float32(rc)), float(np.float32(value)), seed, b"x.bam", False)
            rows, lead = _rows_of(ora["matrix"]), ["%.3f" % rc, "%.3f" % value]
        elif verb == "cap":
            rows, lead = _rows_of(cap_ref.point(case, b"x.bam", rc, value, seed)["matrix"]), ["%.3f" % rc, str(int(value))]
        else:
            rows, lead = _rows_of(level_ref.point(hits, value)["matrix"]), ["%.3f" % rc, str(int(value))]
        mom = G.moments(full, rows, nf)
        _POINTS[key] = (G.gene_rows(ids, n_cells, mom), G.summary_fields(lead, seed, n_cells, mom))
    return _POINTS[key]


def _grid(name, verb):
    if name == "edge":
        return [1], {"sweep": [0, 0.5, 1], "cap": [1, 2], "level": [1, 2]}[verb]
    if verb == "sweep":
        return [0.5, 1], [0.1, 1]
    hits = G.full_matrix("mixed", _case("mixed"), 0.5, 926)[4]
    if verb == "cap":
        return [0.5], [int(np.percentile(hits.h, 20)), int(hits.h.max())]
    return [0.5], [int(np.percentile(hits.u_full, 10)), int(hits.u_full.max())]


MOD = {"sweep": sweep, "cap": cap, "level": level}
OPT = {"sweep": "-r", "cap": "-n", "level": "-m"}


def _gz(p):
    return gzip.decompress(open(p, "rb").read())


def _check_outputs(out, name, verb, rates, values, seeds=(926,), reps=False, summary_only=False):
    lines = open(out / ("%s_gene_fidelity.tsv" % verb)).read().split("\n")
    assert lines[0].split("\t") == list(MOD[verb].GENE_FIDELITY_COLUMNS) and lines[-1] == ""
    assert len(lines) - 2 == len(rates) * len(values) * len(seeds)
    k = 1
    for rc in rates:
        for seed in seeds:
            for v in values:
                genes, row = _point(name, verb, rc, v, seed)
                G.assert_fields(lines[k].split("\t"), row, 6, (verb, rc, seed, v))
                k += 1
                d = out / (MOD[verb].point_dir(rc, v) + ("_s%d" % seed if reps else ""))
                if summary_only:
                    assert not d.exists()
                    continue
                got = _gz(d / "gene_fidelity.tsv.gz").decode().split("\n")
                assert got[0].split("\t") == list(sweep.POINT_GENE_FIDELITY_COLUMNS) and got[-1] == "" and len(got) - 2 == len(genes)
                for g, w in zip(got[1:-1], genes):
                    G.assert_fields(g.split("\t"), w, 8, (verb, rc, seed, v))
                assert sweep.read_point_gene_fidelity(d / "gene_fidelity.tsv.gz")[0]["feature"] == genes[0][0]
                assert _gz(d / "features.tsv.gz").decode().split("\n")[0].split("\t")[0] == genes[0][0]
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
    r = subprocess.run(_args(verb, bam, b, f, out, rates, values) + ["--gene-fidelity"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, FASTF_PROFILE="1"))
    assert r.returncode == 0, r.stderr
    assert "%s_gene_fidelity.tsv is generated." % verb in r.stdout and "[%s] --gene-fidelity:" % verb in r.stderr
    assert "_fidelity.tsv is generated." not in r.stdout.replace("_gene_fidelity", "") and "[%s] --fidelity:" % verb not in r.stderr
    _check_outputs(out, name, verb, rates, values)
    r = subprocess.run(_args(verb, bam, b, f, out0, rates, values), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    with_flag, without = _tree(out), _tree(out0)
    new = {n for n in with_flag if n == "%s_gene_fidelity.tsv" % verb or os.path.basename(n) == "gene_fidelity.tsv.gz"}
    assert len(new) == 1 + len(rates) * len(values) and not [n for n in without if "fidelity" in n]
    assert {n: v for n, v in with_flag.items() if n not in new} == without


@pytest.mark.parametrize("name", ["edge", "mixed"])
@pytest.mark.parametrize("verb", ["sweep", "cap", "level"])
def test_in_process(tmp_path, verb, name):
    bam, b, f = _write(tmp_path, _case(name))
    rates, values = _grid(name, verb)
    out = tmp_path / "out"
    MOD[verb].__dict__[verb](bam, out, b, f, rates, values, seed=926, gene_fidelity=True)
    _check_outputs(out, name, verb, rates, values)
    rows = MOD[verb].read_gene_fidelity_table(out / ("%s_gene_fidelity.tsv" % verb))
    assert len(rows) == len(rates) * len(values) and rows[0]["seed"] == "926"
    if name == "mixed":                                     # the deepest point of the grid is the full matrix itself
        last = rows[-1]
        assert last["median_pearson"] == "1.000000" and last["p10_pearson"] == "1.000000" and last["hvg_overlap"] == "1.000000"
        assert float(rows[0]["median_pearson"]) < 1 and int(rows[0]["hvg_k"]) > 100
    out2 = tmp_path / "out2"
    MOD[verb].__dict__[verb](bam, out2, b, f, rates, values, seed=926, gene_fidelity=True, summary_only=True)
    _check_outputs(out2, name, verb, rates, values, summary_only=True)
    assert sorted(os.listdir(out2)) == sorted(["%s.tsv" % verb, "%s_gene_fidelity.tsv" % verb])
    assert open(out2 / ("%s_gene_fidelity.tsv" % verb)).read() == open(out / ("%s_gene_fidelity.tsv" % verb)).read()


@pytest.mark.parametrize("verb", ["sweep", "cap", "level"])
def test_with_fidelity_cells_and_genes_together(tmp_path, verb):
    """--cells' K3u writes the row buffer the partner counts read, --genes lends its two arrays, --fidelity shares the full rows: every
    file of the other flags stays what it is"""
    bam, b, f = _write(tmp_path, _case("mixed"))
    rates, values = _grid("mixed", verb)
    out, out0 = tmp_path / "out", tmp_path / "out0"
    for o, extra in ((out, ["--gene-fidelity"]), (out0, [])):
        r = subprocess.run(_args(verb, bam, b, f, o, rates, values) + ["--fidelity", "--cells", "--genes"] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
    _check_outputs(out, "mixed", verb, rates, values)
    with_flag, without = _tree(out), _tree(out0)
    assert {n: v for n, v in with_flag.items() if "gene_fidelity" not in n} == without and len(with_flag) == len(without) + 1 + len(rates) * len(values)
    assert all(any(n.endswith(e) for n in without) for e in ("cells.tsv.gz", "genes.tsv.gz", "/fidelity.tsv.gz", "%s_fidelity.tsv" % verb))


def test_two_seeds_give_one_row_per_cell_rate_seed_and_value(tmp_path):
    bam, b, f = _write(tmp_path, _case("mixed"))
    out = tmp_path / "out"
    r = subprocess.run(_args("sweep", bam, b, f, out, [0.5], [0.1, 1]) + ["--gene-fidelity", "--seeds", "926,5"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    _check_outputs(out, "mixed", "sweep", [0.5], [0.1, 1], seeds=(926, 5), reps=True)
    rows = sweep.read_gene_fidelity_table(out / "sweep_gene_fidelity.tsv")
    assert [x["seed"] for x in rows] == ["926", "926", "5", "5"] and rows[0] != rows[2]
    assert not [n for n in os.listdir(out) if "gene_fidelity_reps" in n]
    out2 = tmp_path / "out2"
    cap.cap_reps(bam, out2, b, f, [0.5], _grid("mixed", "cap")[1][:1], [926], gene_fidelity=True, summary_only=True)
    _check_outputs(out2, "mixed", "cap", [0.5], _grid("mixed", "cap")[1][:1], seeds=(926,), reps=True, summary_only=True)


def test_refusal_of_20_base_umis_leaves_no_table(tmp_path):
    """20-base UMIs do not fit a 64-bit key: the full rows live on the device alone, so sweep does not fall back with the flag"""
    case = Case(n=30_000, n_bar=400, n_gene=150, umi_len=20, umi_pool=512, p_n_umi=0.02, p_bad_xf=0.1, data_seed=35)
    bam, b, f = _write(tmp_path, case)
    for verb, v in (("sweep", [0.5]), ("cap", [5]), ("level", [5])):
        out = tmp_path / ("out_" + verb)
        r = subprocess.run(_args(verb, bam, b, f, out, [1], v) + ["--gene-fidelity"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 1 and "outside" in r.stderr and "point by point" not in r.stderr.replace("no point-by-point", ""), r.stderr
        assert "%s: --gene-fidelity needs the resident form" % verb in r.stderr
        assert [n for n in os.listdir(out) if n.startswith(verb)] == []
    with pytest.raises(F.FastfError, match="--gene-fidelity needs the resident form"):
        sweep.sweep(bam, tmp_path / "outp", b, f, [1], [1], gene_fidelity=True)
    assert not (tmp_path / "outp" / "sweep.tsv").exists()
