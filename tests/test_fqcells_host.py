"""fqcells without a GPU: fastf_fqcells_call against the definition (tests/fqcells_ref.py) on hand tables, the refusals of the
command line (each with a message, exit 1, nothing created), the help text, and the census of the fixtures
tests/test_gpu_fqcells.py runs — asserted on the reference alone."""
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib

import fqcells_ref as Q

OURS = _lib.cli_path()
RULE_ARG = {"e": "expect", "k": "top", "m": "min_umis"}


def check_call(rows, rule, arg):
    """rows: [(packed barcode, reads, umis)] in any order"""
    bc = np.array([r[0] for r in rows], dtype=np.uint64)
    reads = np.array([r[1] for r in rows], dtype=np.uint64)
    umis = np.array([r[2] for r in rows], dtype=np.uint32)
    rank, called, thr = F.fqcells_call(bc, reads, umis, **{RULE_ARG[rule]: arg})
    want_rank, want_called, want_thr = Q.call(rows, rule, arg)
    assert thr == want_thr, (rule, arg, thr, want_thr)
    assert [int(x) for x in rank] == [want_rank[r[0]] for r in rows], (rule, arg)
    assert [bool(x) for x in called] == [want_called[r[0]] for r in rows], (rule, arg)
    return rank, called, thr


RULES = [("e", 1), ("e", 99), ("e", 100), ("e", 250), ("e", 3000), ("e", 2 ** 64 - 1), ("k", 1), ("k", 2), ("k", 3), ("k", 7), ("k", 2 ** 64 - 1),
         ("m", 1), ("m", 2), ("m", 5), ("m", 6), ("m", 2 ** 32), ("m", 2 ** 64 - 1)]


@pytest.mark.parametrize("rule,arg", RULES)
def test_call_on_hand_tables(rule, arg):
    tables = {
        "B=0": [],
        "B=1": [(5, 9, 4)],
        "all umis equal": [(k, 1 + (k * 7) % 4, 6) for k in range(1, 12)],
        "tie on umis and reads at ranks 3 to 5": [(9, 50, 40), (2, 30, 20), (7, 30, 20), (4, 30, 20), (1, 8, 8), (3, 2 ** 40, 20)],
        "E / 100 + 1 beyond B, m below 5": [(3, 4, 4), (8, 3, 3), (1, 1, 1), (2, 1, 1)],
        "-u 0: umis all 1, the order is by reads": [(k, (k * 5) % 13 + 1, 1) for k in range(20)],
        "rounding: m = 55, 54, 45 at rank 1, 2, 3": [(1, 99, 55), (2, 99, 54), (3, 99, 45), (4, 9, 6), (5, 9, 5), (6, 9, 4)],
    }
    for name, rows in tables.items():
        rank, called, thr = check_call(rows, rule, arg)
        if rows:
            assert sorted(int(x) for x in rank) == list(range(1, len(rows) + 1)), name
    # what the names promise
    if (rule, arg) == ("k", 2):
        _, called, thr = check_call(tables["tie on umis and reads at ranks 3 to 5"], rule, arg)
        assert list(called) == [True, False, False, False, False, True] and thr == 20      # (reads 2^40 ranks before the tied three)
        _, called, _ = check_call(tables["tie on umis and reads at ranks 3 to 5"], "k", 3)
        assert list(called) == [True, True, False, False, False, True]                     # of the tie, the lower barcode bytes first
    if (rule, arg) == ("e", 3000):
        assert check_call(tables["E / 100 + 1 beyond B, m below 5"], rule, arg)[2] == 1
        assert check_call(tables["B=0"], rule, arg)[2] == 1
    if (rule, arg) == ("e", 1):
        assert check_call(tables["rounding: m = 55, 54, 45 at rank 1, 2, 3"], "e", 1)[2] == 6       # rank 1: (55 + 5) / 10
        assert check_call(tables["rounding: m = 55, 54, 45 at rank 1, 2, 3"], "e", 100)[2] == 5     # rank 2: (54 + 5) / 10
        assert check_call(tables["rounding: m = 55, 54, 45 at rank 1, 2, 3"], "e", 200)[2] == 5     # rank 3: (45 + 5) / 10


@pytest.mark.parametrize("threads", ["1", "3", "16", "37"])
def test_call_sorts_large_tables_on_every_thread_count(monkeypatch, threads):
    monkeypatch.setenv("FASTF_HOST_THREADS", threads)            # (read at every call)
    rng = np.random.default_rng(1)
    n = 150001                                                   # above the size from which the sort is split over the host threads
    bc = rng.permutation(n).astype(np.uint64)
    reads = rng.integers(1, 40, size=n).astype(np.uint64)
    umis = np.minimum(reads, rng.integers(1, 12, size=n)).astype(np.uint32)
    order = np.lexsort((bc, -reads.astype(np.int64), -umis.astype(np.int64)))
    want = np.empty(n, dtype=np.uint32)
    want[order] = np.arange(1, n + 1, dtype=np.uint32)
    rank, called, thr = F.fqcells_call(bc, reads, umis, top=777)
    assert np.array_equal(rank, want) and called.sum() == 777 and (rank[called] <= 777).all() and thr == umis[order[776]]


def test_call_refuses_bad_rules():
    with pytest.raises(ValueError):
        F.fqcells_call([1], [1], [1], top=0)
    with pytest.raises(ValueError):
        F.fqcells_call([1], [1], [1], top=1, expect=5)
    with pytest.raises(ValueError):
        F.fqcells_call([1, 2], [1], [1], top=1)
    one = np.ones(1, np.uint64)
    thr = _lib.C.c_uint64()
    ptr = lambda a: a.ctypes.data_as(_lib.C.c_void_p)  # noqa: E731
    for rule, arg in ((ord("x"), 1), (0, 1), (ord("e"), 0), (ord("k"), 0), (ord("m"), 0)):
        assert _lib.lib().fastf_fqcells_call(ptr(one), ptr(one), ptr(one.astype(np.uint32)), 1, rule, arg, None, None, _lib.C.byref(thr)) == 1


def run(args, cwd=None):
    return subprocess.run([OURS, "fqcells"] + [str(a) for a in args], capture_output=True, text=True, cwd=cwd, timeout=120)


@pytest.fixture()
def inputs(tmp_path):
    r1 = tmp_path / "r1.fq"
    r1.write_bytes(Q.fastq_fixture())
    out = tmp_path / "out"
    out.mkdir()
    return str(r1), out


def refused(p, out, *words):
    assert p.returncode == 1, (p.returncode, p.stdout, p.stderr)
    for w in words:
        assert w in p.stderr, (w, p.stderr)
    assert os.listdir(out) == []


def test_refusals_with_nothing_created(inputs, tmp_path):
    r1, out = inputs
    base = ["-R", r1, "-o", out]
    refused(run(["-o", out]), out, "-R")
    refused(run(base + ["-l", 16, "-u", 16]), out, "-l 16 -u 16", "31")
    refused(run(base + ["-l", 31, "-u", 1]), out, "31")
    refused(run(base + ["-l", 2147483647, "-u", 10]), out, "-l 2147483647 -u 10", "31")   # (the sum does not wrap)
    refused(run(base + ["-l", 0]), out, "-l 0")
    refused(run(base + ["-l", -3]), out, "negative")
    refused(run(base + ["-u", -1]), out, "negative")
    for a, b in (("-e", "-k"), ("-k", "-m"), ("-m", "-e"), ("--expect", "--top")):
        refused(run(base + [a, 5, b, 5]), out, "one calling rule")
    for opt in ("-e", "-k", "-m", "--expect", "--top", "--min"):
        for bad in ("0", "00", "-5", "+5", "5x", "1e3", "", "99999999999999999999999"):
            refused(run(base + [opt, bad]), out, "digits")
    p = run(base + ["-a"])
    refused(p, out, "-a")
    assert "unknown option" in p.stderr
    refused(run(["-R", r1, "-o", tmp_path / "missing"]), out, "-o", str(tmp_path / "missing"))
    f = tmp_path / "a_file"
    f.write_bytes(b"")
    refused(run(["-R", r1, "-o", f]), out, "-o")
    refused(run(["-R", tmp_path / "none.fq", "-o", out]), out, "none.fq")
    for kw in (dict(len_cb=0), dict(len_cb=20, len_umi=12), dict(len_umi=-1), dict(top=0), dict(top=3, min_umis=3)):
        with pytest.raises(ValueError):
            F.fqcells(r1, out=out, **kw)
    assert os.listdir(out) == []


def test_help_names_every_option():
    p = run(["-h"])
    assert p.returncode == 0
    for opt in ("-h, --help", "-R, --R1", "-o, --out", "-l, --len", "-u, --umi", "-e, --expect", "-k, --top", "-m, --min"):
        assert opt in p.stdout, opt
    for word in ("fqcells.tsv.gz", "whitelist.txt", "fqcells_summary.tsv", "3000", "filter -w", "fqcap -w"):
        assert word in p.stdout, word
    top = subprocess.run([OURS, "-h"], capture_output=True, text=True)
    assert top.returncode == 0 and "\n    fqcells " in top.stdout
    for sym in ("fastf_fqcells", "fastf_fqcells_call", "fastf_fqcells_reduce", "fastf_fqcells_tile"):
        assert sym in _lib.ABI_SYMBOLS
    names = _lib.lib().fastf_kernel_names().decode().split(",")
    assert "fqc_heads_kernel" in names and "fqc_rows_kernel" in names
    assert _lib.lib().fastf_fqcells_tile() >= 64


def test_each_wrong_rule_changes_some_gpu_fixture():
    """every DEFECTS entry is noticed by a fixture tests/test_gpu_fqcells.py runs: the seam tables (at the reduce's own tile
    size) or the end-to-end cases — by the reference alone"""
    T = _lib.lib().fastf_fqcells_tile()
    seam = Q.seam_fixtures(T)
    e2e = Q.e2e_cases()
    good_seam = {f[0]: Q.reduce_ref(f[1], f[2], f[3]) for f in seam}
    good_e2e = {c[0]: Q.py_fqcells(*c[1:]) for c in e2e}
    for defect in Q.DEFECTS:
        caught = [f[0] for f in seam if Q.reduce_ref(f[1], f[2], f[3], tile=T, defect=defect) != good_seam[f[0]]]
        caught += [c[0] for c in e2e if {k: v for k, v in Q.py_fqcells(*c[1:], defect=defect).items()} != good_e2e[c[0]]]
        assert caught, "no fixture notices the defect %s" % defect
        print("%s: noticed by %d fixtures: %s" % (defect, len(caught), "; ".join(caught[:6])))


def test_the_fixtures_hold_what_they_are_named_for():
    T = _lib.lib().fastf_fqcells_tile()
    seam = {f[0]: f for f in Q.seam_fixtures(T)}
    assert sorted({len(f[1]) for f in seam.values()}) == sorted(set(Q.seam_sizes(T)))
    assert {f[3] for f in seam.values()} == {0, 1, 10, 15}
    k = seam["straddle m1=%d" % (T + 1)][1]
    assert (int(k[T - 1]) >> 20) == (int(k[T]) >> 20) != (int(k[T - 2]) >> 20)
    bc, reads, umis = Q.reduce_ref(*seam["long_run m1=%d" % (3 * T + 7)][1:4])
    assert max(umis) > 2 * T and umis[:3] == [1, 2, 1] and umis[4] <= 3
    bc, reads, umis = Q.reduce_ref(*seam["wide_counts m1=63"][1:4])
    assert max(reads) >= 3 * 0xffffffff > 2 ** 33
    assert int(seam["u=15 l+u=31 m1=65"][1][-1]) >> 30 == (1 << 33) | (4 ** 16 - 1)      # the highest barcode: every key bit in use
    # the end-to-end text: every kind of uncounted read, a tie at the K the -k case uses, thresholds with neighbours on both sides
    n_reads, other, per = Q.read_table(Q.fastq_fixture(), 16, 10)
    assert 3000 < n_reads < 6000 and other == 48 and len(per) > 250
    ref = Q.py_fqcells(Q.fastq_fixture(), 16, 10, "e", 1100)["dict"]
    assert ref["threshold"] == 6 and {5, 6, 7, 8} <= {m for _, m in per.values()}
    assert Q.py_fqcells(Q.fastq_fixture(), 16, 10, "e", 10 ** 6)["dict"]["called"] == len(per)
    k = Q.py_fqcells(Q.fastq_fixture(), 16, 10, "k", Q.tie_rank())["dict"]
    assert k["called"] == Q.tie_rank() and k["threshold"] == 30
    assert Q.py_fqcells(Q.e2e_cases()[8][1])["dict"]["counted"] == 0
