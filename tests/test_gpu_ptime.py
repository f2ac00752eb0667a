"""--pseudotime on the GPU: fastf_dev_ptime_medians and fastf_dev_ptime_census against the host twins (and, at the small sizes, against
ptime_ref) — guard words behind every output, values behind every input that change the answer if read — and sweep, cap and level with
the option, through the CLI and in process: every row of pseudotime.tsv.gz and <verb>_pseudotime.tsv against ptime_ref driven from the
matrices the run wrote."""
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, cap, hostmem, level, sweep
import mapping_ref as M
import neighbors_ref as N
import ptime_ref as R
import test_gpu_labels as TL
import test_labels_host as LH
import test_ptime_host as H
from sweep_ref import parse_matrix

pytestmark = pytest.mark.gpu

GUARD = 0xA5A5A5A5
TILE = sweep.PTIME_TILE
SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
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


def _dev(a, tail):
    """a device copy of an array with `tail` behind it"""
    return hostmem.to_device(np.concatenate([np.ascontiguousarray(a).reshape(-1), tail]), "cuda")


def _device_medians(eng, idx, cnt, t, k):
    """one call on device copies: 64 guard words behind both outputs; behind the inputs rows that would be a 65th .. cell with full lists
    of valued neighbours, and behind t values an index of n and beyond would find"""
    import torch
    n = len(cnt)
    d_idx = _dev(idx.astype(np.uint32), np.zeros(64 * k, np.uint32))
    d_cnt = _dev(cnt.astype(np.uint32), np.full(64, k, np.uint32))
    d_t = _dev(t.astype(np.uint32), np.full(256, 2 * n + 2, np.uint32))
    outs = [torch.full((n + 64,), GUARD - (1 << 32), dtype=torch.int32, device="cuda") for _ in range(2)]
    eng.dev_ptime_medians(d_idx.data_ptr(), d_cnt.data_ptr(), d_t.data_ptr(), n, k, outs[0].data_ptr(), outs[1].data_ptr())
    torch.cuda.synchronize()
    host = [hostmem.to_host(o).view(np.uint32) for o in outs]
    assert all((h[n:] == GUARD).all() for h in host), "words behind an output were written"
    return host[0][:n], host[1][:n]


def _device_census(eng, est, t):
    """one call on device copies: the result block comes in as garbage with 8 guard words behind it; behind est and t a tile of cells
    that would take part"""
    import torch
    n = len(t)
    d_est = _dev(est.astype(np.uint32), np.arange(1, TILE + 1, dtype=np.uint32))
    d_t = _dev(t.astype(np.uint32), np.arange(TILE, 0, -1, dtype=np.uint32))
    d_out = torch.full((sweep.PTIME_OUT_WORDS + 8,), 0x5EEDBEEF5EEDBEEF, dtype=torch.int64, device="cuda")
    eng.dev_ptime_census(d_est.data_ptr(), d_t.data_ptr(), n, d_out.data_ptr())
    torch.cuda.synchronize()
    out = hostmem.to_host(d_out).view(np.uint64)
    assert (out[sweep.PTIME_OUT_WORDS:] == 0x5EEDBEEF5EEDBEEF).all(), "words behind the result block were written"
    return [int(x) for x in out[:sweep.PTIME_OUT_WORDS]]


_TWIN = {}


def _fixture(n, k, ties):
    """computed once and shared: (fx, the poisoned form, the twin's medians)"""
    key = (n, k, ties)
    if key not in _TWIN:
        fx = H.random_fixture(n, k, seed=n * 131 + k * 7 + ties, ties=ties)
        _TWIN[key] = (fx, H.poisoned(fx, n), sweep.ptime_medians(fx[1], fx[2], fx[3], k))
    return _TWIN[key]


# k: below, at and above the edges of the lane groups of 16, 32 and 64
@pytest.mark.parametrize("n,k", [(n, 15) for n in SIZES] + [(65, k) for k in (1, 2, 16, 17, 32, 33, 64)] + [(TILE + 1, k) for k in (17, 64)])
def test_medians_against_the_twin(eng, n, k):
    for ties in (0, 1):
        fx, bad, twin = _fixture(n, k, ties)
        for f in (fx, bad):
            est, valued = _device_medians(eng, f[1], f[2], f[3], k)
            assert (est == twin[0]).all() and (valued == twin[1]).all()
        if n <= 257:
            H.check_medians(twin, fx)


@pytest.mark.parametrize("k", [9, 15, 17, 33, 64])
def test_medians_of_the_hand_built_lists_and_indices_out_of_range(eng, k):
    lists, t, want = H.hand_fixture()
    idx, cnt = H._slots(lists, k)
    for f_idx in (idx, H.poisoned((lists, idx, cnt, t, k), 10)[1]):
        est, valued = _device_medians(eng, f_idx, cnt, t, k)
        assert ([int(x) for x in est], [int(x) for x in valued]) == want
    # an index of n and beyond INSIDE the valid slots has no value; cnt beyond k counts as k
    idx2 = idx.copy()
    idx2[9, :3] = [10, 11, 0xFFFFFFFE]                      # cells 0, 1, 2 leave list 9: 6 10 12 14 16 are left -> 12
    cnt2 = cnt.copy(); cnt2[9] = 9 if k == 9 else 200
    for got in (_device_medians(eng, idx2, cnt2, t, k), sweep.ptime_medians(idx2, cnt2, t, k)):
        assert (int(got[0][9]), int(got[1][9])) == (12, 5) and [int(x) for x in got[0][:9]] == want[0][:9]


def test_medians_with_no_cells_and_the_refusals(eng):
    eng.dev_ptime_medians(0, 0, 0, 0, 15, 0, 0)             # no cells: nothing is launched
    for bad_k in (0, 65):
        with pytest.raises(F.FastfError, match="k = %d, from 1 to 64" % bad_k):
            eng.dev_ptime_medians(0, 0, 0, 0, bad_k, 0, 0)
    with pytest.raises(F.FastfError, match="null argument"):
        eng.dev_ptime_medians(0, 0, 0, 5, 15, 0, 0)
    with pytest.raises(F.FastfError, match="null argument"):
        eng.dev_ptime_census(0, 0, 5, 0)
    assert _device_census(eng, np.zeros(0, np.uint32), np.zeros(0, np.uint32)) == [0] * 7      # the block is zeroed all the same


def _census_inputs(n, kind):
    rng = np.random.default_rng(n * 7 + len(kind))
    if kind == "random":                                    # few ties, a fifth of the cells absent on either side
        est, t = (rng.integers(1, 2 * n + 2, size=n).astype(np.uint32) for _ in range(2))
        est[rng.random(n) < 0.1] = 0; t[rng.random(n) < 0.1] = 0
    elif kind == "ties":                                    # three values a side: most pairs tie, many on both sides; counting the diagonal tile
        est, t = (rng.integers(1, 4, size=n).astype(np.uint32) for _ in range(2))      # twice, or j < i as well, changes tie_both
    else:                                                   # every second cell absent, by est and by t in turn
        est, t = (rng.integers(1, 50, size=n).astype(np.uint32) for _ in range(2))
        est[0::4] = 0; t[2::4] = 0
    return est, t


@pytest.mark.parametrize("kind", ["random", "ties", "absent"])
@pytest.mark.parametrize("n", SIZES)
def test_census_against_the_twin(eng, n, kind):
    est, t = _census_inputs(n, kind)
    twin = [int(x) for x in sweep.ptime_census(est, t)]
    assert _device_census(eng, est, t) == twin
    cells = int(((est > 0) & (t > 0)).sum())
    assert twin[5] == cells and sum(twin[:5]) == cells * (cells - 1) // 2
    if kind == "ties" and n >= 64:
        assert twin[4] > cells                              # (a second count of the diagonal would show)
    if kind == "absent":
        assert cells == n - len(range(0, n, 4)) - len(range(2, n, 4))
    if n <= 257:
        assert twin == R.census([int(x) for x in est], [int(x) for x in t])


def test_census_of_the_named_orders(eng):
    for name, (est, t, want) in H.census_cases().items():
        got = _device_census(eng, est, t)
        assert got == [int(x) for x in sweep.ptime_census(est, t)], name
        if want:
            assert all(w is None or w == g for w, g in zip(want, got)), name
    n = 2 * TILE + 1
    up = np.arange(1, n + 1, dtype=np.uint32) * 2
    assert _device_census(eng, up, up) == [n * (n - 1) // 2, 0, 0, 0, 0, n, 0]
    assert _device_census(eng, up[::-1].copy(), up)[:6] == [0, n * (n - 1) // 2, 0, 0, 0, n]
    assert _device_census(eng, np.full(n, 4, np.uint32), up)[:6] == [0, 0, n * (n - 1) // 2, 0, 0, n]
    assert _device_census(eng, up, np.full(n, 4, np.uint32))[:6] == [0, 0, 0, n * (n - 1) // 2, 0, n]
    assert _device_census(eng, np.full(n, 4, np.uint32), np.full(n, 4, np.uint32)) == [0, 0, 0, 0, n * (n - 1) // 2, n, 0]
    # the largest ranks a u32 holds, every pair discordant, and a shift sum beyond 32 bits
    hi = np.array([0xFFFFFFFF, 1, 0xFFFFFFFE, 2], np.uint32)
    lo = np.array([1, 0xFFFFFFFF, 2, 0xFFFFFFFE], np.uint32)
    assert _device_census(eng, hi, lo) == [int(x) for x in sweep.ptime_census(hi, lo)] == [0, 6, 0, 0, 0, 4, 2 * 0xFFFFFFFE + 2 * 0xFFFFFFFC]


def test_census_of_100000_cells_in_closed_form(eng):
    """e = t = 2 (i + 1): every pair is concordant, n (n - 1) / 2 = 4 999 950 000 of them, beyond 32 bits: no 32-bit sum crosses a workgroup"""
    n = 100_000
    up = np.arange(1, n + 1, dtype=np.uint32) * 2
    assert _device_census(eng, up, up) == [4_999_950_000, 0, 0, 0, 0, n, 0]


# ---- the commands ----
_PT_TEXT = []


def _pt_text(case):
    """one value per barcode of the synthetic BAM — the cell's type (i % 3, which its genes follow) plus quarter steps with ties —, every 7th cell NA, every 11th without a line, two barcodes
    nobody lists, the rows in reverse order under a header"""
    if not _PT_TEXT:
        lines = []
        for i, bc in enumerate(case.bar.tolist()):
            if i % 11 == 10:
                continue
            lines.append("%s\t%s" % (bc.decode(), "NA" if i % 7 == 6 else repr((i % 3) * 10 + (i * 37 % 60 // 6) / 4 - 3)))
        lines += ["NOBODY-1\t0.5", "NOBODY-2\tNA"]
        _PT_TEXT.append(("barcode\tpseudotime\n" + "\n".join(lines[::-1]) + "\n").encode())
    return _PT_TEXT[0]


def _write(tmp_path, case):
    bam, b, f, lf = TL._write(tmp_path, case)
    pf = tmp_path / "pseudotime.in.tsv"
    pf.write_bytes(_pt_text(case))
    return bam, b, f, lf, pf


_REF = {}


def _reference_point(case, full_rows, point_rows, barcodes, with_map):
    """(t, m, full, point, mapped, the three censuses) by the reference alone: A from the full rows, both neighbour sets, the mapping lists"""
    key = (full_rows[2].tobytes(), point_rows[0].tobytes(), point_rows[1].tobytes(), point_rows[2].tobytes(), with_map)
    if key not in _REF:
        n = len(barcodes)
        values = R.parse_file(_pt_text(case), [b.decode() for b in case.bar.tolist()])[0]
        t, m = R.midranks([values.get(bc) for bc in barcodes])
        A = N.hvg_of_rows(full_rows, n, 45)
        full = R.medians(N.neighbor_sets(full_rows, n, A)[0], t)
        point = R.medians(N.neighbor_sets(point_rows, n, A)[0], t)
        mapped = R.medians(M.mapping(full_rows, point_rows, n, A)[0], t) if with_map else None
        _REF[key] = (t, m, full, point, mapped, [None if x is None else R.census(x[0], t) for x in (full, point, mapped)])
    return _REF[key]


def _check_outputs(out, case, verb, rates, values, with_map, seeds=(926,), reps=False, written=None):
    """written: a tree of the same run without --summary-only whose matrices give the reference (summary-only runs write none)"""
    lines = open(out / ("%s_pseudotime.tsv" % verb)).read().split("\n")
    assert lines[0].split("\t") == list(MOD[verb].PSEUDOTIME_COLUMNS) and lines[-1] == "" and len(lines) - 2 == len(rates) * len(values) * len(seeds)
    at = 1
    for rc in rates:
        for seed in seeds:
            full_rows, barcodes = case.matrix(rc, 1, seed)
            for v in values:
                name = MOD[verb].point_dir(rc, v) + ("_s%d" % seed if reps else "")
                d = (written or out) / name
                point_rows = parse_matrix(TL._gz(d / "matrix.mtx.gz"))[3:]
                assert TL._gz(d / "barcodes.tsv.gz").decode().split("\n")[:-1] == barcodes
                t, m, full, point, mapped, cen = _reference_point(case, full_rows, point_rows, barcodes, with_map)
                lead = ["%.3f" % rc, "%.3f" % v if verb == "sweep" else str(int(v))]
                assert lines[at].split("\t") == R.summary_fields(lead, seed, len(barcodes), 15, m, *cen), (verb, rc, seed, v)
                at += 1
                if written:
                    assert not (out / name).exists()
                    continue
                got = TL._gz(d / "pseudotime.tsv.gz").decode().split("\n")
                assert got[0].split("\t") == list(sweep.POINT_PSEUDOTIME_COLUMNS) and got[-1] == ""
                assert [g.split("\t") for g in got[1:-1]] == R.cell_rows(barcodes, t, full, point, mapped)
                assert [r["barcode"] for r in sweep.read_point_pseudotime(d / "pseudotime.tsv.gz")] == barcodes
    assert not [n for n in os.listdir(out) if n.endswith(".partial")]
    return lines


def _is_new(name, verb):
    return name == "%s_pseudotime.tsv" % verb or os.path.basename(name) == "pseudotime.tsv.gz"


@pytest.mark.parametrize("verb", ["sweep", "cap", "level"])
def test_cli_with_the_option_alone_and_the_same_tree_without(tmp_path, verb):
    case = LH.labcase()
    bam, b, f, lf, pf = _write(tmp_path, case)
    rates, values = [0.5, 1], TL.GRID[verb]
    out, out0 = tmp_path / "out", tmp_path / "out0"
    r = subprocess.run(TL._args(verb, bam, b, f, out, rates, values) + ["--pseudotime", str(pf)], capture_output=True, text=True, timeout=600, env=dict(os.environ, FASTF_PROFILE="1"))
    assert r.returncode == 0, r.stderr
    assert "%s_pseudotime.tsv is generated." % verb in r.stdout and "[%s] --pseudotime: 47 values, pseudotime_unknown 2;" % verb in r.stderr
    assert "neighbors.tsv is generated." not in r.stdout and "] --neighbors:" not in r.stderr
    lines = _check_outputs(out, case, verb, rates, values, False)
    rows = MOD[verb].read_pseudotime_table(out / ("%s_pseudotime.tsv" % verb))
    assert all(rows[0][c] == "NA" for c in sweep.PSEUDOTIME_COLUMNS[-5:]) and rows[-1]["k"] == "15" and rows[-1]["cells_valued"] == "47" and rows[-1]["n_cells"] == "60"
    assert rows[-1]["tau_full"] not in ("NA", "1.000000") and int(rows[-1]["conc_full"]) > int(rows[-1]["disc_full"]) > 0      # the fixture has an order to lose
    assert len(set(lines[1:-1])) == len(lines) - 2
    # pseudotime_path == NULL is the run without the option, byte for byte
    r = subprocess.run(TL._args(verb, bam, b, f, out0, rates, values), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    with_opt, without = TL._tree(out), TL._tree(out0)
    new = {n for n in with_opt if _is_new(n, verb)}
    assert len(new) == 1 + len(rates) * len(values) and not [n for n in with_opt if "neighbors" in n or "labels" in n or "mapping" in n]
    assert {n: v for n, v in with_opt.items() if n not in new} == without
    out1 = tmp_path / "out1"
    one, p_one = sweep._floats(rates)
    lv = np.ascontiguousarray(values, np.float32 if verb == "sweep" else np.uint64)
    enc = lambda p: os.fspath(p).encode()  # noqa: E731
    _lib.check(getattr(_lib.lib(), "fastf_%s_pseudotime" % verb)(enc(bam), enc(out1), enc(b), enc(f), p_one, len(rates), lv.ctypes.data_as(sweep.C.POINTER(sweep.C.c_float))
                                                                 if verb == "sweep" else lv.ctypes.data, len(lv), None, 0, 0, 926, None, 0, 0, None))
    assert TL._tree(out1) == without


@pytest.mark.parametrize("verb", ["sweep", "cap", "level"])
def test_in_process_with_mapping_and_summary_only(tmp_path, verb):
    case = LH.labcase()
    bam, b, f, lf, pf = _write(tmp_path, case)
    rates, values = [1], TL.GRID[verb]
    out, out2 = tmp_path / "out", tmp_path / "out2"
    MOD[verb].__dict__[verb](bam, out, b, f, rates, values, seed=926, mapping=True, pseudotime=pf)
    _check_outputs(out, case, verb, rates, values, True)
    rows = MOD[verb].read_pseudotime_table(out / ("%s_pseudotime.tsv" % verb))
    assert all(rows[0][c] != "NA" for c in ("cells_map", "conc_map", "disc_map", "tau_map", "shift_map"))
    MOD[verb].__dict__[verb](bam, out2, b, f, rates, values, seed=926, mapping=True, pseudotime=pf, summary_only=True)
    _check_outputs(out2, case, verb, rates, values, True, written=out)
    assert sorted(os.listdir(out2)) == sorted(["%s.tsv" % verb, "%s_mapping.tsv" % verb, "%s_pseudotime.tsv" % verb])
    assert open(out2 / ("%s_pseudotime.tsv" % verb)).read() == open(out / ("%s_pseudotime.tsv" % verb)).read()


@pytest.mark.parametrize("verb", ["sweep", "cap", "level"])
def test_beside_the_other_comparisons(tmp_path, verb):
    """the neighbour sets, the mapping list and the label arrays are shared with --neighbors, --labels and --mapping: their files stay what they are"""
    case = LH.labcase()
    bam, b, f, lf, pf = _write(tmp_path, case)
    rates, values = [0.5], TL.GRID[verb]
    out, out0 = tmp_path / "out", tmp_path / "out0"
    others = ["--neighbors", "--labels", str(lf), "--mapping", "--markers", "5", "--fidelity"]
    for o, extra in ((out, ["--pseudotime=" + str(pf)]), (out0, [])):
        r = subprocess.run(TL._args(verb, bam, b, f, o, rates, values) + others + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
    _check_outputs(out, case, verb, rates, values, True)
    with_opt, without = TL._tree(out), TL._tree(out0)
    assert {n: v for n, v in with_opt.items() if not _is_new(n, verb)} == without and len(with_opt) == len(without) + 1 + len(rates) * len(values)
    assert all(any(n.endswith(e) for n in without) for e in ("neighbors.tsv.gz", "labels.tsv.gz", "mapping.tsv.gz", "markers.tsv.gz", "/fidelity.tsv.gz"))


def test_two_seeds_give_one_row_per_cell_rate_seed_and_value(tmp_path):
    case = LH.labcase()
    bam, b, f, lf, pf = _write(tmp_path, case)
    out = tmp_path / "out"
    r = subprocess.run(TL._args("sweep", bam, b, f, out, [0.5], [0.1, 1]) + ["--pseudotime", str(pf), "--labels", str(lf), "--seeds", "926,5"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    _check_outputs(out, case, "sweep", [0.5], [0.1, 1], False, seeds=(926, 5), reps=True)
    rows = sweep.read_pseudotime_table(out / "sweep_pseudotime.tsv")
    assert [x["seed"] for x in rows] == ["926", "926", "5", "5"] and rows[0] != rows[2]
    assert [(x["rate_cell"], x["rate_depth"], x["seed"]) for x in rows] == [(x["rate_cell"], x["rate_depth"], x["seed"]) for x in sweep.read_labels_table(out / "sweep_labels.tsv")]
    assert not [n for n in os.listdir(out) if "pseudotime_reps" in n]
    for k, (verb, mod) in enumerate((("cap", cap), ("level", level))):
        o = tmp_path / ("reps%d" % k)
        mod.__dict__[verb + "_reps"](bam, o, b, f, [0.5], TL.GRID[verb][:1], [5], pseudotime=pf)
        _check_outputs(o, case, verb, [0.5], TL.GRID[verb][:1], False, seeds=(5,), reps=True)
