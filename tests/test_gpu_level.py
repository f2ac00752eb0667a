"""`fastF level` on the GPU: the step of the threshold search (fastf_dev_level_init / fastf_dev_level_step) against a numpy twin of
its state rules and, driven through a whole search, against the (M + 1)-th smallest birth of every cell; and the command — through
the CLI and in process — with every point's files against level_ref (the unchanged oracle on masked records, T proved against the
definition) and every level.tsv row against numpy."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, hostmem, level
from helpers import Case
import cells_ref
import genes_ref
import level_ref
import reps_ref
from sweep_ref import parse_matrix
from test_gpu_sweep import _Edge, _write

pytestmark = pytest.mark.gpu

FULL = 1 << 32
GUARD = np.uint64(0xFFFFFFFFFFFFFFFF)
N_CELLS = [1, 63, 64, 65, 70_000]


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    cells = np.arange(1, 101, dtype=np.uint64) | (np.uint64(1) << np.uint64(62))
    feats = np.arange(1, 51, dtype=np.uint64) | (np.uint64(2) << np.uint64(62))
    e = F.Engine(cells, feats, umi_max_bases=12)
    yield e
    e.close()


# ---- the numpy twin of the state rules (include/fastf_amd.h) ----
def _probes(lo, hi):
    open_ = hi - lo > 1
    return np.where(open_, (lo + hi) // 2, 0), open_


def twin_init(u_full, M):
    capped = u_full > M
    lo = np.where(capped, 0, FULL).astype(np.int64)
    hi = np.full(len(u_full), FULL, np.int64)
    probe, open_ = _probes(lo, hi)
    return lo, hi, probe, int(open_.sum()), int(capped.sum())


def twin_step(u, M, lo, hi):
    probe, open_ = _probes(lo, hi)
    lo = np.where(open_ & (u <= M), probe, lo)
    hi = np.where(open_ & (u > M), probe, hi)
    probe, open_ = _probes(lo, hi)
    return lo, hi, probe, int(open_.sum())


class _State:
    """lo, hi, probe (n_cells u64 each) and the result block on the device, each with two guard words behind it"""

    def __init__(self, n_cells):
        import torch
        self.torch, self.n = torch, n_cells
        mk = lambda k: torch.full((k + 2,), -1, dtype=torch.int64, device="cuda")  # noqa: E731
        self.lo, self.hi, self.probe, self.out = mk(n_cells), mk(n_cells), mk(n_cells), mk(4)

    def ptrs(self):
        return self.lo.data_ptr(), self.hi.data_ptr(), self.probe.data_ptr(), self.out.data_ptr()

    def read(self):
        self.torch.cuda.synchronize()
        arrs = [hostmem.to_host(t).view(np.uint64) for t in (self.lo, self.hi, self.probe, self.out)]
        for a in arrs:
            assert (a[-2:] == GUARD).all(), "words behind an array were written"
        lo, hi, probe, out = (a[:-2] for a in arrs)
        return lo.astype(np.int64), hi.astype(np.int64), probe.astype(np.int64), out


def _dev_u64(a):
    return hostmem.to_device(np.ascontiguousarray(a, dtype=np.uint64), "cuda")


@pytest.mark.parametrize("n_cells", N_CELLS)
def test_init_against_the_twin(eng, n_cells):
    """U_full straddling M (M - 1, M, M + 1), cells with 0 UMIs, random ones; then an M above every U_full: nobody is capped"""
    rng = np.random.default_rng(n_cells)
    M = 40
    u_full = rng.integers(0, 3 * M, size=n_cells)
    u_full[::5] = np.resize([M - 1, M, M + 1, 0, 2 ** 40], len(u_full[::5]))
    if n_cells == 1:
        u_full[0] = M + 1
    d_u = _dev_u64(np.concatenate([u_full, [2 ** 50]]))                  # (an entry behind the cells that must not be read as one)
    for cap_m in (M, 2 ** 41):
        st = _State(n_cells)
        eng.dev_level_init(d_u.data_ptr(), n_cells, cap_m, *st.ptrs())
        lo, hi, probe, out = st.read()
        wlo, whi, wprobe, wopen, wcapped = twin_init(u_full, cap_m)
        np.testing.assert_array_equal(lo, wlo); np.testing.assert_array_equal(hi, whi); np.testing.assert_array_equal(probe, wprobe)
        assert list(out) == [wopen, wcapped, 0, 0]
        assert wopen == wcapped == int((u_full > cap_m).sum())
        if cap_m == 2 ** 41:
            assert wopen == 0 and (lo == FULL).all() and (probe == 0).all()
        else:
            assert wcapped > 0 and (probe[u_full > M] == 1 << 31).all() and (lo[u_full == M] == FULL).all()
    with pytest.raises(F.FastfError):
        eng.dev_level_init(d_u.data_ptr(), n_cells, 0, *_State(n_cells).ptrs())


def _births(rng, n_cells, M):
    """per cell a sorted array of u32 births — 0 and 0xFFFFFFFE among them, equal births inside a cell, cells with none, with exactly
    M, M + 1 and many — padded to a matrix with 2^33 (below no threshold)"""
    counts = rng.integers(0, 4 * M + 2, size=n_cells)
    counts[::7] = np.resize([4 * M + 1, 0, M, M + 1, 1], len(counts[::7]))
    B = rng.integers(0, 0xFFFFFFFF, size=(n_cells, 4 * M + 1), dtype=np.int64)
    B[rng.random(B.shape) < 0.2] = 0                                      # many births at 0 ...
    B[rng.random(B.shape) < 0.2] = 0xFFFFFFFE                             # ... and at the largest draw the tests' seeds give
    dup = rng.random(B.shape) < 0.3
    B[:, 1:][dup[:, 1:]] = B[:, :-1][dup[:, 1:]]                          # equal births inside a cell
    if n_cells >= 3:                                                      # the (M + 1)-th smallest birth at either end of the range
        counts[1], counts[2] = M + 2, M + 2
        B[1, :M + 2] = [0] * (M + 1) + [7]
        B[2, :M + 2] = list(range(1, M + 1)) + [0xFFFFFFFE, 0xFFFFFFFE]
    B[np.arange(B.shape[1])[None, :] >= counts[:, None]] = 1 << 33
    B.sort(axis=1)
    return B, counts


@pytest.mark.parametrize("n_cells", N_CELLS)
def test_a_whole_search_finds_the_m_plus_first_birth(eng, n_cells):
    M = 3
    rng = np.random.default_rng(100 + n_cells)
    B, counts = _births(rng, n_cells, M)
    U = lambda T: (B < np.asarray(T, np.int64)[:, None]).sum(axis=1)  # noqa: E731
    want = np.where(counts > M, B[:, M], FULL)
    u_full = U(np.full(n_cells, FULL))
    np.testing.assert_array_equal(u_full, counts)
    st = _State(n_cells)
    d_u = _dev_u64(u_full)
    eng.dev_level_init(d_u.data_ptr(), n_cells, M, *st.ptrs())
    lo, hi, probe, out = st.read()
    wlo, whi, wprobe, wopen, wcapped = twin_init(u_full, M)
    assert list(out) == [wopen, wcapped, 0, 0] and wcapped == int((counts > M).sum())
    steps = 0
    while out[0]:
        np.testing.assert_array_equal(probe, wprobe)
        u = U(probe)                                                       # U_k at this pass's thresholds: 0 for every cell that is not open
        d_u = _dev_u64(u)
        eng.dev_level_step(d_u.data_ptr(), n_cells, M, *st.ptrs())
        lo, hi, probe, out = st.read()
        wlo, whi, wprobe, wopen = twin_step(u, M, wlo, whi)
        steps += 1
        assert list(out) == [wopen, wcapped, 0, 0], steps                 # (cells_capped is the init's: a step leaves it)
        np.testing.assert_array_equal(lo, wlo); np.testing.assert_array_equal(hi, whi)
        assert steps <= 32
    np.testing.assert_array_equal(lo, want)
    assert (probe == 0).all() and ((hi - lo <= 1)).all()
    assert (U(lo) <= M).all() and (U(np.minimum(lo + 1, FULL))[counts > M] > M).all()     # the definition, directly
    if n_cells >= 63:
        assert steps == 32 and want[1] == 0 and want[2] == 0xFFFFFFFE and (want == FULL).any()


def test_a_step_that_finds_error_bits_holds_the_state(eng):
    n_cells, M = 130, 5
    u_full = np.arange(n_cells)
    st = _State(n_cells)
    d_full, d_zero, d_bits, d_clean = _dev_u64(u_full), _dev_u64(np.zeros(n_cells)), _dev_u64([16]), _dev_u64([0])
    eng.dev_level_init(d_full.data_ptr(), n_cells, M, *st.ptrs())
    lo, hi, probe, out = st.read()
    eng.dev_level_step(d_zero.data_ptr(), n_cells, M, *st.ptrs(), d_err_in=d_bits.data_ptr())
    lo2, hi2, probe2, out2 = st.read()
    np.testing.assert_array_equal(lo2, lo); np.testing.assert_array_equal(hi2, hi); np.testing.assert_array_equal(probe2, probe)
    assert list(out2) == [0, out[1], 16, 1]
    eng.dev_level_step(d_zero.data_ptr(), n_cells, M, *st.ptrs(), d_err_in=d_clean.data_ptr())
    lo3, _, _, out3 = st.read()
    assert list(out3) == [out[0], out[1], 0, 0] and (lo3[u_full > M] == 1 << 31).all()


# ---- the command ----
MIXED = dict(n=200_000, n_bar=600, n_gene=500, umi_len=12, dup_factor=3.0, p_no_cb=0.05, p_unlisted_cb=0.05, p_bad_xf=0.15, p_n_umi=0.01,
             p_multi_gene=0.02)
_CASES, _HITS, _POINTS = {}, {}, {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = _Edge() if name == "edge" else Case(**MIXED)
    return _CASES[name]


def _hits(name, bam, rc, seed=926):
    key = (name, str(bam), float(rc), seed)
    if key not in _HITS:
        _HITS[key] = level_ref.Hits(_case(name), str(bam).encode(), rc, seed)
    return _HITS[key]


def _point(name, bam, rc, m, seed=926):
    key = (name, str(bam), float(rc), int(m), seed)
    if key not in _POINTS:
        _POINTS[key] = level_ref.point(_hits(name, bam, rc, seed), m)
    return _POINTS[key]


def _mixed_caps(bam):
    """from the reference's U_full: an M that caps most cells, one that caps a few, one that caps none — at both cell rates (the
    cells of -c 0.5 are among those of -c 1, and U_k(2^32) is a cell's own)"""
    half, whole = _hits("mixed", bam, 0.5).u_full, _hits("mixed", bam, 1).u_full
    caps = [int(np.percentile(whole, 10)), int(np.sort(half)[-3]), int(whole.max())]
    for u in (half, whole):
        assert (u > caps[0]).sum() > len(u) // 2 and 0 < (u > caps[1]).sum() <= len(u) // 10 and (u > caps[2]).sum() == 0
    return caps


def _gz(p):
    return gzip.decompress(open(p, "rb").read())


def _args(bam, b, f, out, rates, caps):
    return ["-b", str(bam), "-a", str(b), "-f", str(f), "-o", str(out), "-c", ",".join("%g" % r for r in rates), "-m", ",".join(str(m) for m in caps)]


def _check_outputs(out, name, bam, rates, caps, summary_only=False, extra_files=()):
    rows = [ln.split("\t") for ln in open(out / "level.tsv").read().split("\n")]
    assert rows[0] == list(level.COLUMNS) and rows[-1] == [""]
    rows = rows[1:-1]
    assert len(rows) == len(rates) * len(caps)
    k = 0
    for rc in rates:
        for m in caps:
            ref = _point(name, bam, rc, m)
            d = out / level.point_dir(rc, m)
            if summary_only:
                assert not d.exists()
            else:
                assert sorted(os.listdir(d)) == sorted(("matrix.mtx.gz", "barcodes.tsv.gz", "features.tsv.gz", "thresholds.tsv.gz") + tuple(extra_files))
                assert _gz(d / "matrix.mtx.gz") == ref["matrix"], d
                assert _gz(d / "barcodes.tsv.gz") == ref["barcodes"], d
                assert _gz(d / "features.tsv.gz") == ref["features"], d
                assert _gz(d / "thresholds.tsv.gz") == ref["thresholds"], d
                # directly from the matrix: every column sum <= M; an uncapped cell's column is the depth-1 run's
                _, _, n_cells, feature, cell, count = parse_matrix(_gz(d / "matrix.mtx.gz"))
                sums = np.zeros(n_cells, np.int64); np.add.at(sums, cell - 1, count)
                assert (sums <= m).all()
                np.testing.assert_array_equal(sums, ref["u"])
                full = _hits(name, bam, rc).ora_full
                keep_g, keep_f = ~ref["capped"][cell - 1], ~ref["capped"][full["cell"].astype(np.int64) - 1]
                for got, want in ((feature, full["feature"]), (cell, full["cell"]), (count, full["count"])):
                    np.testing.assert_array_equal(got[keep_g], want.astype(np.int64)[keep_f])
                names, thr, u_full, u = level.read_thresholds(d / "thresholds.tsv.gz")
                np.testing.assert_array_equal(u, sums); np.testing.assert_array_equal(thr, ref["T"])
            assert rows[k] == ref["row"], (rc, m)
            k += 1
    assert not [n for n in os.listdir(out) if n.endswith(".partial")]
    return rows


@pytest.mark.parametrize("name", ["edge", "mixed"])
def test_cli_level_against_the_reference(tmp_path, name):
    case = _case(name)
    bam, b, f = _write(tmp_path, case)
    rates, caps = ([1], [1, 2]) if name == "edge" else ([0.5, 1], _mixed_caps(bam))
    out = tmp_path / "out"
    r = subprocess.run([_lib.cli_path(), "level", "-d", str(tmp_path / "x.db")] + _args(bam, b, f, out, rates, caps), capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, FASTF_PROFILE="1"))
    assert r.returncode == 0, r.stderr
    rows = _check_outputs(out, name, bam, rates, caps)
    assert "[level] search:" in r.stderr and "probing passes" in r.stderr
    if name == "mixed":
        for rc in rates:                                   # the M that caps nobody: `bam2db -r 1`, whose rate_depth reads 1.000 too
            d = out / level.point_dir(rc, caps[2])
            ora = _hits(name, bam, rc).ora_full
            assert b'"rate_depth": 1.000,' in ora["matrix"]
            assert (_gz(d / "matrix.mtx.gz"), _gz(d / "barcodes.tsv.gz"), _gz(d / "features.tsv.gz")) == (ora["matrix"], ora["barcodes"], ora["features"])
        none = [x for x in rows if x[1] == str(caps[2])]
        assert len(none) == 2 and all(x[13] == "0" and x[14] == "1.000000" and x[5] == x[12] for x in none)
        assert all(int(x[13]) > int(x[3]) // 2 for x in rows if x[1] == str(caps[0]))
    else:
        assert [x[13] for x in rows] == ["1", "0"]


def test_summary_only_writes_no_point_directories(tmp_path):
    bam, b, f = _write(tmp_path, _case("edge"))
    out = tmp_path / "out"
    r = subprocess.run([_lib.cli_path(), "level", "--summary-only", "-s926"] + _args(bam, b, f, out, [1], [1, 2]), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    _check_outputs(out, "edge", bam, [1], [1, 2], summary_only=True)
    assert sorted(os.listdir(out)) == ["level.tsv"]


def test_genes_and_cells_tables_on_the_references_kept_set(tmp_path):
    case = _case("mixed")
    bam, b, f = _write(tmp_path, case)
    caps = _mixed_caps(bam)[:2]
    out = tmp_path / "out"
    r = subprocess.run([_lib.cli_path(), "level", "--genes", "--cells"] + _args(bam, b, f, out, [1], caps), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    _check_outputs(out, "mixed", bam, [1], caps, extra_files=("genes.tsv.gz", "cells.tsv.gz"))
    assert sorted(os.listdir(out)) == sorted(["level.tsv", "level_genes.tsv", "level_gene_cells.tsv.gz", "level_cells.tsv"] + [level.point_dir(1, m) for m in caps])
    glines = open(out / "level_genes.tsv").read().split("\n")
    clines = open(out / "level_cells.tsv").read().split("\n")
    assert glines[0].split("\t") == list(level.GENES_COLUMNS) and clines[0].split("\t") == list(level.CELLS_COLUMNS)
    assert len(glines) == len(clines) == len(caps) + 2
    grid = _gz(out / "level_gene_cells.tsv.gz").decode().split("\n")
    assert grid[0].split("\t") == ["feature"] + [level.point_dir(1, m) for m in caps]
    hits = _hits("mixed", bam, 1)
    for j, m in enumerate(caps):
        ref = _point("mixed", bam, 1, m)
        lead = ["1.000", str(m)]
        d = out / level.point_dir(1, m)
        want, cells_g, umis_g = genes_ref.expected_genes_row(ref["matrix"], lead, 926)
        assert glines[1 + j].split("\t") == want
        ids = genes_ref.feature_ids(ref["features"])
        assert _gz(d / "genes.tsv.gz").decode() == "".join("%s\t%d\t%d\n" % (i, c, u) for i, c, u in zip(ids, cells_g, umis_g))
        assert [ln.split("\t")[1 + j] for ln in grid[1:-1]] == [str(int(c)) for c in cells_g]
        ora_u, _, _ = hits.run(ref["T"], umi_copies=True)                 # the kept set of the reference, with its -u rows
        reads, nulls, single, hist = cells_ref.from_oracle(ora_u, hits.n_cells)
        assert clines[1 + j].split("\t") == cells_ref.table_row(lead, 926, reads, nulls, single, hist)
        assert _gz(d / "cells.tsv.gz").decode().split("\n")[:-1] == cells_ref.point_lines(ref["barcodes"], ref["matrix"], reads, nulls, single)


def test_two_seeds_give_suffixed_directories_and_the_replicate_table(tmp_path):
    case = _case("mixed")
    bam, b, f = _write(tmp_path, case)
    m = _mixed_caps(bam)[0]
    seeds = [926, 5]
    out = tmp_path / "out"
    r = subprocess.run([_lib.cli_path(), "level", "--seeds", "926,5"] + _args(bam, b, f, out, [0.5], [m]), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    names = ["%s_s%d" % (level.point_dir(0.5, m), s) for s in seeds]
    assert sorted(os.listdir(out)) == sorted(["level.tsv", "level_reps.tsv"] + names)
    rows = [ln.split("\t") for ln in open(out / "level.tsv").read().split("\n")[1:-1]]
    refs = [_point("mixed", bam, 0.5, m, seed=s) for s in seeds]
    for row, ref, s, nm in zip(rows, refs, seeds, names):
        assert row == ref["row"] and row[2] == str(s)
        assert _gz(out / nm / "matrix.mtx.gz") == ref["matrix"] and _gz(out / nm / "thresholds.tsv.gz") == ref["thresholds"]
    assert (refs[0]["T"] != refs[1]["T"]).any()                           # another seed, other draws, other thresholds
    reps = open(out / "level_reps.tsv").read().split("\n")
    assert reps[0].split("\t") == list(level.REPS_COLUMNS) and len(reps) == 3 and reps[-1] == ""
    reps_ref.assert_reps_row(reps[1].split("\t"), reps_ref.reps_row(["0.500", str(m)], [ref["row"] for ref in refs]), "level_reps.tsv")


@pytest.mark.parametrize("env", [{"FASTF_NO_STREAM_K1B": "1"}])
def test_cli_level_on_a_general_path(tmp_path, env):
    """no streaming K1b: SoA records and the tile form, the cell scratch as a plain array"""
    bam, b, f = _write(tmp_path, _case("mixed"))
    caps = _mixed_caps(bam)[:2]
    out = tmp_path / "out"
    r = subprocess.run([_lib.cli_path(), "level"] + _args(bam, b, f, out, [1], caps), capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr
    _check_outputs(out, "mixed", bam, [1], caps)


def test_level_in_process(tmp_path):
    bam, b, f = _write(tmp_path, _case("mixed"))
    caps = _mixed_caps(bam)[1:]
    out = tmp_path / "out"
    rows = level.level(bam, out, b, f, [0.5], caps, seed=926)
    assert len(rows) == 2 and rows[0]["rate_cell"] == "0.500" and rows[0]["umi_cap"] == str(caps[0]) and rows[1]["cells_capped"] == "0"
    _check_outputs(out, "mixed", bam, [0.5], caps)
    out2 = tmp_path / "out2"
    rows2 = level.level(bam, out2, b, f, [0.5], caps, seed=926, summary_only=True)
    assert rows2 == rows and sorted(os.listdir(out2)) == ["level.tsv"]


def test_refusal_of_20_base_umis_leaves_no_table(tmp_path):
    """20-base UMIs do not fit a 64-bit key and a UMI cap has no point-by-point form"""
    case = Case(n=30_000, n_bar=400, n_gene=150, umi_len=20, umi_pool=512, p_n_umi=0.02, p_bad_xf=0.1, data_seed=35)
    bam, b, f = _write(tmp_path, case)
    out = tmp_path / "out"
    r = subprocess.run([_lib.cli_path(), "level", "--genes", "--seeds", "1,2", "-b", str(bam), "-a", str(b), "-f", str(f), "-o", str(out), "-m", "5,50"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 1, r.stderr
    assert "outside the resident form" in r.stderr, r.stderr
    assert [n for n in os.listdir(out) if n.startswith("level")] == []
    with pytest.raises(F.FastfError):
        level.level(bam, tmp_path / "outp", b, f, [1], [5])
    assert not (tmp_path / "outp" / "level.tsv").exists()
