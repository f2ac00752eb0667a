"""--markers without a GPU: the host twin fastf_marker_auc and fastf_marker_rank against the brute force of markers_ref on random and
hand-built fixtures, the two-label identity, garbage in the padding of the planes, the refusals, the rows, headers and NA rules, the
command line, and a census: every fixture's expected output changes under at least one deliberately wrong rule."""
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, cap, level, sweep, synth
import markers_ref as MR


# ---- fixtures: (counts n x K int64, lab u8[n], n_labels, n_planes) ----
def random_fixture(n, K, L, P, seed, p_unlabelled=0.2, p_nonzero=0.3):
    rng = np.random.default_rng(seed)
    lab = rng.integers(1, L + 1, size=n)
    lab[rng.random(n) < p_unlabelled] = 0
    if n > 4:
        lab[rng.integers(0, n)] = min(L + 1, 255) if L < 255 else 0     # a label above n_labels counts as unlabelled
    small = rng.integers(1, 6, size=(n, K))
    edge = rng.choice([126, 127] if P == 1 else [126, 127, 128, 129, 255, 256, 16383], size=(n, K))
    wide = rng.integers(1, 128 ** P, size=(n, K))
    pick = rng.random((n, K))
    counts = np.where(pick < 0.7, small, np.where(pick < 0.85, edge, wide))
    counts[rng.random((n, K)) >= p_nonzero] = 0
    return counts.astype(np.int64), lab.astype(np.uint8), L, P


def hand_fixture(name):
    """small enough for the pure-int double loop"""
    z = np.zeros
    if name == "all_counts_equal":
        return np.full((9, 3), 7, np.int64), np.array([1, 1, 2, 2, 2, 3, 0, 3, 1], np.uint8), 3, 1
    if name == "detected_in_one_label":
        c = z((8, 2), np.int64); c[[0, 1, 2], 0] = [3, 1, 2]; c[:, 1] = 1
        return c, np.array([1, 1, 1, 2, 2, 2, 2, 0], np.uint8), 2, 1
    if name == "two_genes_equal_2u":
        c = z((6, 4), np.int64); c[:3, 1] = 5; c[:3, 2] = 9; c[3:, 3] = 2     # slots 1 and 2 tie for label 1
        return c, np.array([1, 1, 1, 2, 2, 2], np.uint8), 2, 1
    if name == "unlabelled_large_counts":
        c = z((8, 3), np.int64); c[:, 0] = [1, 2, 3, 4, 100, 120, 127, 90]; c[:, 1] = [0, 1, 0, 1, 127, 127, 127, 127]; c[4:, 2] = 99
        return c, np.array([1, 1, 2, 2, 0, 0, 3, 0], np.uint8), 2, 1      # (label 3 is above n_labels = 2: unlabelled too)
    if name == "label_without_cells":
        c = np.arange(18, dtype=np.int64).reshape(6, 3) % 5
        return c, np.array([1, 1, 3, 3, 3, 0], np.uint8), 3, 1
    if name == "all_cells_in_one_label":
        c = np.arange(12, dtype=np.int64).reshape(4, 3)
        return c, np.array([2, 2, 2, 2], np.uint8), 2, 1
    if name == "plane_edges":
        vals = [0, 1, 126, 127, 128, 16383]
        c = np.array([[vals[(i + g) % 6] for g in range(4)] for i in range(12)], np.int64); c[:, 3] = [vals[i % 6] for i in range(12)]
        return c, np.array([1, 2, 1, 2, 1, 2, 2, 1, 0, 1, 2, 2], np.uint8), 2, 2
    raise KeyError(name)


HAND = ("all_counts_equal", "detected_in_one_label", "two_genes_equal_2u", "unlabelled_large_counts", "label_without_cells", "all_cells_in_one_label",
        "plane_edges")


def twin(fx, pad_byte=0):
    counts, lab, L, P = fx
    n, K = counts.shape
    return sweep.marker_auc(sweep.marker_planes(counts, P, pad_byte), P, n, K, lab, L)


def as_lists(got):
    return [[[int(v) for v in row] for row in t] for t in got[:3]] + [[int(v) for v in got[3]]]


def check_tables(got, ref, columns=None):
    """got: arrays (s2u, det, sum, n_per_label); ref: markers_ref tables, whole or only at `columns`"""
    g = as_lists(got)
    assert g[3] == ref[3]
    for k in range(3):
        for a in range(len(ref[3])):
            if columns is None:
                assert g[k][a] == ref[k][a], (k, a)
            else:
                assert [g[k][a][c] for c in columns] == [ref[k][a][c] for c in columns], (k, a)


# ---- the host twin against the brute force ----
@pytest.mark.parametrize("name", HAND)
def test_the_host_twin_on_the_hand_built_fixtures(name):
    fx = hand_fixture(name)
    ref = MR.tables(fx[0].tolist(), fx[1], fx[2])
    check_tables(twin(fx), ref)
    check_tables(MR.tables_rows(fx[0], fx[1], fx[2]), ref)         # the two forms of the reference agree
    r = sweep.marker_rank(twin(fx)[0], twin(fx)[3])
    assert r.tolist() == MR.ranks(ref[0], ref[3])


def test_what_the_hand_built_fixtures_pin():
    s2u, det, tot, npl = as_lists(twin(hand_fixture("all_counts_equal")))
    assert npl == [3, 3, 2] and s2u == [[3 * 5] * 3, [3 * 5] * 3, [2 * 6] * 3]          # every pair ties: 2U = n_a n_out, AUC one half
    s2u, det, tot, npl = as_lists(twin(hand_fixture("detected_in_one_label")))
    assert det == [[3, 3], [0, 4]] and tot == [[6, 3], [0, 4]] and s2u[0][0] == 2 * 3 * 4 and s2u[1][0] == 0 and s2u[0][1] == 3 * 4
    fx = hand_fixture("two_genes_equal_2u")
    got = twin(fx)
    assert int(got[0][0][1]) == int(got[0][0][2]) == 18
    assert sweep.marker_rank(got[0], got[3]).tolist()[0] == [3, 1, 2, 4]                 # the tie goes to the lower feature number
    assert sweep.marker_rank(got[0], got[3], genes=[7, 9, 2, 1]).tolist()[0] == [3, 2, 1, 4]     # ... which is the gene's, not the slot's
    c, lab, L, P = hand_fixture("unlabelled_large_counts")
    quiet = c.copy(); quiet[lab == 0] = 0; quiet[lab > L] = 0
    check_tables(twin((quiet, lab, L, P)), MR.tables(c.tolist(), lab, L))                 # unlabelled cells change nothing
    got = twin(hand_fixture("label_without_cells"))
    assert got[3].tolist() == [2, 0, 3] and not got[0][1].any() and sweep.marker_rank(got[0], got[3]).tolist()[1] == [0, 0, 0]
    got = twin(hand_fixture("all_cells_in_one_label"))
    assert got[3].tolist() == [0, 4] and not got[0].any() and not sweep.marker_rank(got[0], got[3]).any()      # n_out == 0: no ranking


@pytest.mark.parametrize("n,K,L,P", [(1, 1, 1, 1), (2, 3, 2, 1), (40, 5, 3, 1), (40, 5, 3, 2), (33, 7, 5, 2), (64, 2, 255, 1)])
def test_the_host_twin_on_random_fixtures(n, K, L, P):
    fx = random_fixture(n, K, L, P, seed=n * 7 + K + L + P)
    ref = MR.tables(fx[0].tolist(), fx[1], L)
    check_tables(twin(fx), ref)
    check_tables(MR.tables_rows(fx[0], fx[1], L), ref)
    genes = np.random.default_rng(3).permutation(K + 5)[:K]
    assert sweep.marker_rank(twin(fx)[0], twin(fx)[3], genes).tolist() == MR.ranks(ref[0], ref[3], genes)


@pytest.mark.parametrize("n,K,L,P", [(300, 40, 4, 1), (257, 33, 30, 2)])
def test_larger_shapes_against_the_row_form(n, K, L, P):
    fx = random_fixture(n, K, L, P, seed=n + P)
    check_tables(twin(fx), MR.tables_rows(fx[0], fx[1], L))


@pytest.mark.parametrize("P", [1, 2])
def test_the_identity_of_two_labels(P):
    counts, lab, _, _ = random_fixture(90, 12, 2, P, seed=5 + P, p_unlabelled=0.3)
    lab[lab > 2] = 0
    s2u, _, _, npl = twin((counts, lab, 2, P))
    assert npl.min() > 0 and (s2u[0] + s2u[1] == 2 * int(npl[0]) * int(npl[1])).all()


@pytest.mark.parametrize("P", [1, 2])
def test_garbage_in_the_padding_changes_nothing(P):
    fx = random_fixture(37, 5, 3, P, seed=8)
    clean = as_lists(twin(fx))
    for pad in (0x7F, 0xFF, 0x01):
        assert as_lists(twin(fx, pad_byte=pad)) == clean
    planes = sweep.marker_planes(fx[0], P)
    planes[:, :37, :5] |= 0x80                                # bit 7 of a plane byte is not part of the count
    assert as_lists(sweep.marker_auc(planes, P, 37, 5, fx[1], 3)) == clean


def test_the_refusals():
    fx = random_fixture(10, 4, 3, 1, seed=1)
    planes = np.zeros(3 * 128 * 32, np.uint8)
    with pytest.raises(F.FastfError, match="FASTF_ERR_MARKER_COUNT.*3 planes"):
        sweep.marker_auc(planes, 3, 10, 4, fx[1], 3)
    with pytest.raises(F.FastfError, match="FASTF_ERR_MARKER_COUNT"):
        sweep.marker_auc(planes, 0, 10, 4, fx[1], 3)
    for L in (0, 256):
        with pytest.raises(F.FastfError, match="%d labels, from 1 to 255" % L):
            sweep.marker_auc(planes, 1, 10, 4, fx[1], L)
        assert sweep.marker_auc_form(1, L) == -1
    assert sweep.marker_auc_form(3, 5) == -1
    got = sweep.marker_auc(planes, 1, 0, 4, np.zeros(0, np.uint8), 3)        # no cells: the tables are cleared all the same
    assert not any(t.any() for t in got)


def test_the_form_a_device_call_takes(monkeypatch):
    monkeypatch.delenv("FASTF_MARKERS_LDS", raising=False)
    assert [sweep.marker_auc_form(1, L) for L in (1, 128, 225, 226, 255)] == [1, 1, 1, 0, 0]      # 19 456 + 640 L bytes against 160 KB
    assert [sweep.marker_auc_form(2, L) for L in (1, 128, 255)] == [1, 1, 1]                       # two slots: every L fits
    monkeypatch.setenv("FASTF_MARKERS_LDS", "0")
    assert [sweep.marker_auc_form(P, L) for P in (1, 2) for L in (1, 255)] == [0] * 4


@pytest.mark.parametrize("K,N", [(1, 1), (1, 5), (3, 2), (3, 3), (3, 2000), (2000, 5), (2000, 2000)])
def test_marker_rank_and_the_rows_at_the_edges_of_k(K, N):
    rng = np.random.default_rng(K + N)
    L, npl = 3, [4, 0, 5]
    s2u = rng.integers(0, 6, size=(L, K)).astype(np.uint64)             # many ties
    s2p = rng.integers(0, 6, size=(L, K)).astype(np.uint64)
    genes = rng.permutation(K)
    rf, rp = sweep.marker_rank(s2u, npl, genes), sweep.marker_rank(s2p, npl, genes)
    ref_f, ref_p = MR.ranks(s2u.tolist(), npl, genes), MR.ranks(s2p.tolist(), npl, genes)
    assert rf.tolist() == ref_f and rp.tolist() == ref_p
    assert sorted(rf[0].tolist()) == list(range(1, K + 1)) and not rf[1].any()
    names = ["NA", "a", "b", "c"]
    zeros = [[0] * K] * L
    full, point = (s2u.tolist(), zeros, zeros, npl), (s2p.tolist(), zeros, zeros, npl)
    text = sweep.markers_summary_rows(0.5, 0.25, 926, names, N, npl, rf, rp, s2u, s2p)
    assert [r.split("\t") for r in text.split("\n")[:-1]] == MR.summary_rows(["0.500", "0.250"], 926, names, K, N, full, point, ref_f, ref_p)
    assert text.split("\n")[0].split("\t")[6] == str(min(N, K))         # top is N_eff


# ---- rows, headers, NA ----
def test_headers_rows_and_the_na_rules():
    assert sweep.markers_header().rstrip("\n").split("\t") == MR.POINT_HEADER == list(sweep.POINT_MARKERS_COLUMNS)
    for verb, mod, second in (("sweep", sweep, "rate_depth"), ("cap", cap, "reads_per_cell"), ("level", level, "umi_cap")):
        cols = sweep.markers_header(verb).rstrip("\n").split("\t")
        assert cols == ["rate_cell", second] + MR.SUMMARY_TAIL == list(mod.MARKERS_COLUMNS)
    assert sweep.markers_row("T", "G1", 3, 4, 1, 7, 18, 12, 3, 1, 2, 0, 7) == "T\tG1\t1\t7\t0.750000\t0.500000\t3\t1\t2\t0\t2.333333\n"
    assert sweep.markers_row("T", None, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0) == "T" + "\tNA" * 10 + "\n"
    assert sweep.markers_row("T", "G1", 4, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0) == "T" + "\tNA" * 10 + "\n"
    fx = hand_fixture("label_without_cells")
    full = MR.tables(fx[0].tolist(), fx[1], 3)
    point = MR.tables((fx[0] // 2).tolist(), fx[1], 3)
    rf, rp = MR.ranks(full[0], full[3]), MR.ranks(point[0], point[3])
    names = ["NA", "x", "y", "z"]
    rows = MR.summary_rows(["1.000", "7"], 5, names, 3, 2, full, point, rf, rp)
    assert rows[1] == ["1.000", "7", "5", "y", "0", "5", "2", "NA", "NA", "NA"] and rows[3][3:7] == ["all", "5", "10", "4"]
    text = sweep.markers_summary_rows(1, 0, 5, names, 2, full[3], rf, rp, np.array(full[0], np.uint64), np.array(point[0], np.uint64), list_value=7)
    assert [r.split("\t") for r in text.split("\n")[:-1]] == rows
    solo = (full[0], full[1], full[2], [0, 0, 6])            # every labelled cell in one label: nothing is ranked
    none = MR.ranks(full[0], solo[3])
    rows = MR.summary_rows(["1.000", "0.500"], 5, names, 3, 2, solo, solo, none, none)
    assert rows[-1] == ["1.000", "0.500", "5", "all", "6", "12", "0", "0", "NA", "NA"] and all(r[7:] == ["NA"] * 3 for r in rows[:3])
    text = sweep.markers_summary_rows(1, 0.5, 5, names, 2, solo[3], none, none, np.array(full[0], np.uint64), np.array(full[0], np.uint64))
    assert [r.split("\t") for r in text.split("\n")[:-1]] == rows
    assert MR.point_rows(names, ["g0", "g1", "g2"], 2, solo, solo, none, none) == [[n] + ["NA"] * 10 for n in names[1:]]


# ---- the interface ----
def test_the_entry_points_the_spellings_and_the_refusals(tmp_path):
    one, p_one = sweep._floats([1])
    caps = np.array([5], np.uint64)
    L = _lib.lib()
    for name in ("fastf_sweep_markers", "fastf_cap_markers", "fastf_level_markers", "fastf_dev_marker_auc", "fastf_marker_auc", "fastf_marker_rank",
                 "fastf_marker_auc_form"):
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name)
    assert "marker_auc_kernel" in L.fastf_kernel_names().decode().split(",")
    assert hasattr(F.Engine, "dev_marker_auc") and sweep.MARKERS_MAX == 2000
    calls = (lambda n, lf: L.fastf_sweep_markers(b"x", b"y", b"b", b"f", p_one, 1, p_one, 1, None, 0, 0, 926, lf, n),
             lambda n, lf: L.fastf_cap_markers(b"x", b"y", b"b", b"f", p_one, 1, caps.ctypes.data, 1, None, 0, 0, 926, lf, n),
             lambda n, lf: L.fastf_level_markers(b"x", b"y", b"b", b"f", p_one, 1, caps.ctypes.data, 1, None, 0, 0, 926, lf, n))
    for verb, call in zip(("sweep", "cap", "level"), calls):
        for n in (0, 2001, 1 << 31):
            with pytest.raises(F.FastfError, match="%s: --markers: N = %d, from 1 to 2000" % (verb, n)):
                _lib.check(call(n, b"labels.tsv"))
        with pytest.raises(F.FastfError, match="%s: --markers needs --labels" % verb):
            _lib.check(call(5, None))
        with pytest.raises(F.FastfError, match="does not exist"):
            _lib.check(call(5, b"labels.tsv"))
    bt, ft, bar, genes = synth.make_lists(5, 3)
    fl, xf, cb, gx, ub = synth.make_records(20, bar, genes)
    bam, b, f, lf = tmp_path / "x.bam", tmp_path / "b.tsv", tmp_path / "f.tsv", tmp_path / "labels.tsv"
    synth.write_bam(str(bam), fl, xf, cb, gx, ub)
    b.write_bytes(bt); f.write_bytes(ft)
    lf.write_bytes(b"".join(x + b"\tT\n" for x in bar.tolist()))
    for k, (verb, extra) in enumerate([("sweep", ["-r", "0.5"]), ("cap", ["-n", "5"]), ("level", ["-m", "5"])]):
        out = tmp_path / ("out%d" % k)
        base = [_lib.cli_path(), verb, "-o", str(out), "-a", str(b), "-f", str(f), "-b", str(bam)] + extra
        r = subprocess.run(base + ["--markers", "5"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "`--markers` needs `--labels`" in r.stderr and not out.exists()
        for bad in ("0", "2001", "-3", "five", "5x", ""):
            r = subprocess.run(base + ["--labels", str(lf), "--markers=" + bad], capture_output=True, text=True, timeout=60)
            assert r.returncode == 1 and "option `--markers` expects an integer from 1 to 2000" in r.stderr and not out.exists(), (bad, r.stderr)
        r = subprocess.run(base + ["--labels", str(lf), "--markers"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "option `--markers` requires a value" in r.stderr and not out.exists()
        for opt in (["-M", "5"], ["--marker", "5"], ["--marker=5"]):    # the long form alone
            r = subprocess.run([_lib.cli_path(), verb] + opt + ["-o", str(out)], capture_output=True, text=True, timeout=60)
            assert r.returncode == 1 and "unknown option" in r.stderr
        r = subprocess.run([_lib.cli_path(), verb, "--help"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and "--markers=<N>" in r.stdout and "%s_markers.tsv" % verb in r.stdout and "markers.tsv.gz" in r.stdout
        several = dict(os.environ, FASTF_DEVICES="0,1")
        r = subprocess.run(base + ["--labels", str(lf), "--markers", "5"], capture_output=True, text=True, timeout=60, env=several)
        assert r.returncode == 1 and "several devices" in r.stderr and not out.exists()
    with pytest.raises(F.FastfError, match="sweep: --markers needs --labels"):
        sweep.sweep(bam, tmp_path / "o", b, f, [1], [1], markers=5)
    with pytest.raises(F.FastfError, match="cap: --markers: N = 0, from 1 to 2000"):
        cap.cap_reps(bam, tmp_path / "o", b, f, [1], [5], [1, 2], labels=lf, markers=2.5)
    with pytest.raises(F.FastfError, match="level: --markers: N = 2001"):
        level.level(bam, tmp_path / "o", b, f, [1], [5], labels=lf, markers=2001)
    assert not (tmp_path / "o").exists()


# ---- the census ----
def _outputs(fx, wrong=None):
    t = MR.tables(fx[0].tolist(), fx[1], fx[2], wrong)
    return t, MR.ranks(t[0], t[3], None, wrong)


CENSUS = [hand_fixture(n) for n in HAND] + [random_fixture(40, 5, 3, 1, seed=40 * 7 + 5 + 3 + 1), random_fixture(33, 7, 5, 2, seed=33 * 7 + 7 + 5 + 2)]


@pytest.mark.parametrize("k", range(len(CENSUS)))
def test_census_every_fixture_tells_a_wrong_rule(k):
    fx = CENSUS[k]
    right = _outputs(fx)
    told = [w for w in MR.WRONG if _outputs(fx, w) != right]
    assert told, "no wrong rule changes what this fixture expects"


def test_census_every_wrong_rule_is_told_by_some_fixture():
    for w in MR.WRONG:
        assert any(_outputs(fx, w) != _outputs(fx) for fx in CENSUS), w
