"""--pseudotime on the host: the loader of the file against ptime_ref (every refusal by name and line, header, CR, NA, -0, ties of
spellings, unknown barcodes, file order), the doubled midranks, the two host twins against ptime_ref on random and hand-built lists, the
rows and headers, and what the commands refuse and print without a device."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, cap, level, sweep, synth
import ptime_ref as R

NONE = 0xFFFFFFFF
LISTED = ("AAA-1", "CCC-1", "GGG-1", "TTT-1", "ACG-1", "TGC-1")


def _files(tmp_path, text, barcodes=LISTED):
    pf, b = tmp_path / "pt.tsv", tmp_path / "barcodes.tsv.gz"
    pf.write_bytes(text if isinstance(text, bytes) else text.encode())
    b.write_bytes(gzip.compress(("\n".join(barcodes) + "\n").encode()))
    return pf, b


def _load_both(tmp_path, text, barcodes=LISTED):
    """(t, m, known, unknown, valued) by the library and the same by ptime_ref, which must agree"""
    pf, b = _files(tmp_path, text, barcodes)
    P = sweep.Pseudotime(pf, b)
    t, m = P.assign(list(barcodes))
    values, known, unknown = R.parse_file(pf.read_bytes(), barcodes)
    rt, rm = R.midranks([values.get(bc) for bc in barcodes])
    assert [int(x) for x in t] == rt and m == rm
    assert (P.known, P.unknown) == (known, unknown) and P.valued == sum(1 for v in values.values() if v is not None)
    P.close()
    return rt, rm, known, unknown


# ---- the loader ----
def test_header_cr_na_and_the_ranks(tmp_path):
    text = "barcode\tpseudotime\r\nGGG-1\t0.5\r\n\nAAA-1\t-2\nNOBODY-1\t7\nTTT-1\tNA\r\nCCC-1\t1e3\nACG-1\t1000\nNOBODY-2\tNA\n"
    t, m, known, unknown = _load_both(tmp_path, text)
    # AAA -2 < GGG 0.5 < CCC 1e3 == ACG 1000; TTT NA and TGC without a line have none
    assert t == [2, 7, 4, 0, 7, 0] and m == 4 and (known, unknown) == (5, 2)
    # no header: the first line is data; a first field that merely starts with `barcode` is data too
    t, m, known, unknown = _load_both(tmp_path, "barcodeX\t3\nAAA-1\t1\nCCC-1\t2", barcodes=LISTED + ("barcodeX",))
    assert t == [2, 4, 0, 0, 0, 0, 6] and m == 3 and unknown == 0
    # a header line alone is no data: no line names a barcode
    pf, b = _files(tmp_path, "barcode\tx\n")
    with pytest.raises(F.FastfError, match="pseudotime: .*pt.tsv: no line names a barcode of"):
        sweep.Pseudotime(pf, b)


def test_minus_zero_the_spellings_of_a_number_and_their_ties(tmp_path):
    text = "AAA-1\t-0\nCCC-1\t0\nGGG-1\t0.0e5\nTTT-1\t+.5\nACG-1\t0x1p-1\nTGC-1\t  5.\n"
    t, m, _, _ = _load_both(tmp_path, text)
    assert t == [4, 4, 4, 9, 9, 12] and m == 6             # -0 == 0 == 0.0e5; .5 == 0x1p-1; blanks in front are strtod's
    t, m, _, _ = _load_both(tmp_path, "AAA-1\t1e-400\nCCC-1\t0\nGGG-1\t-1e-400\n")      # underflow is a finite number: three zeros
    assert t[:3] == [4, 4, 4]
    t, m, _, _ = _load_both(tmp_path, "AAA-1\t%s\n" % ("0" * 62 + "7"))                  # 63 bytes
    assert t[0] == 2 and m == 1


def test_the_ranks_do_not_depend_on_the_order_of_the_file(tmp_path):
    rng = np.random.default_rng(5)
    bcs = ["BC%03d-1" % i for i in range(200)]
    vals = rng.integers(0, 40, size=200)                    # many ties
    lines = ["%s\t%s" % (bc, "NA" if v == 0 else repr(float(v) / 4)) for bc, v in zip(bcs, vals) if v != 1] + ["ZZ%d-1\t3" % i for i in range(5)]
    first = _load_both(tmp_path, "\n".join(lines) + "\n", tuple(bcs))
    for seed in (1, 2):
        order = np.random.default_rng(seed).permutation(len(lines))
        assert _load_both(tmp_path, "\n".join(lines[i] for i in order) + "\n", tuple(bcs)) == first
    t, m = first[0], first[1]
    assert m == int((vals > 1).sum()) and first[3] == 5 and 0 in t and len(set(t)) < m      # holes and ties
    assert sorted(x for x in t if x) == sorted(R.midranks([float(v) for v in vals if v > 1])[0])
    # a subset of the cells ranks among itself: what a (cell rate, seed) pair does
    pf, b = _files(tmp_path, "\n".join(lines) + "\n", tuple(bcs))
    P = sweep.Pseudotime(pf, b)
    sub = bcs[::3]
    got, gm = P.assign(sub)
    values = R.parse_file(pf.read_bytes(), bcs)[0]
    assert ([int(x) for x in got], gm) == R.midranks([values.get(bc) for bc in sub])
    assert P.assign([])[1] == 0 and [int(x) for x in P.assign(["NOT-LISTED", "ZZ1-1"])[0]] == [0, 2]      # (assign looks the file up, not the list)
    P.close()


REFUSALS = [
    ("AAA-1\t1\nCCC-1\n", "fields", 2, "line 2 has 1 fields, not barcode<TAB>value"),
    ("AAA-1\t1\t2\n", "fields", 1, "line 1 has 3 fields, not barcode<TAB>value"),
    ("barcode\n", "fields", 1, "line 1 has 1 fields"),
    ("AAA-1\t1\n\nCCC-1\t\n", "empty", 3, "line 3: the value is empty"),
    ("AAA-1\t%s\n" % ("1" * 64), "long", 1, "line 1: the value has 64 bytes, at most 63"),
    ("AAA-1\t1\nCCC-1\t1.5x\n", "number", 2, "line 2: the value `1.5x` is not a number"),
    ("AAA-1\tna\n", "number", 1, "line 1: the value `na` is not a number"),
    ("AAA-1\t1,5\n", "number", 1, "line 1: the value `1,5` is not a number"),
    ("AAA-1\t1e\n", "number", 1, "is not a number"),
    ("AAA-1\t1 \n", "number", 1, "is not a number"),
    ("AAA-1\t0x\n", "number", 1, "is not a number"),
    ("AAA-1\t--1\n", "number", 1, "is not a number"),
    ("AAA-1\t1\nCCC-1\tnan\n", "finite", 2, "line 2: the value `nan` is not finite"),
    ("AAA-1\t-inf\n", "finite", 1, "line 1: the value `-inf` is not finite"),
    ("AAA-1\tInfinity\n", "finite", 1, "is not finite"),
    ("AAA-1\tNAN(7)\n", "finite", 1, "is not finite"),
    ("AAA-1\t1e999\n", "finite", 1, "line 1: the value `1e999` is not finite"),
    ("AAA-1\t1\nCCC-1\t2\nAAA-1\tNA\n", "twice", 3, "line 3 names barcode AAA-1 again (first on line 1)"),
    ("NOBODY\t1\nNOBODY\t1\nAAA-1\t2\n", "twice", 2, "line 2 names barcode NOBODY again (first on line 1)"),
    ("NOBODY-1\t1\nNOBODY-2\tNA\n", "none", 0, "no line names a barcode of"),
    ("", "none", 0, "no line names a barcode of"),
    (b"AAA-1\t1\0\n", "nul", 1, "line 1 holds a NUL byte"),
]


@pytest.mark.parametrize("text,why,line,message", REFUSALS)
def test_the_refusals_of_the_loader(tmp_path, text, why, line, message):
    pf, b = _files(tmp_path, text)
    with pytest.raises(R.Refused) as ri:
        R.parse_file(pf.read_bytes(), LISTED)
    assert (ri.value.why, ri.value.line) == (why, line)
    with pytest.raises(F.FastfError) as ei:
        sweep.Pseudotime(pf, b)
    assert message in str(ei.value) and "pseudotime:" in str(ei.value) and "pt.tsv" in str(ei.value)


def test_a_missing_file_a_gzip_file_and_null_arguments(tmp_path):
    pf, b = _files(tmp_path, gzip.compress(b"AAA-1\t1\n"))
    with pytest.raises(R.Refused, match="gzip"):
        R.parse_file(pf.read_bytes(), LISTED)
    with pytest.raises(F.FastfError, match="pseudotime: .*pt.tsv starts with the gzip magic: a pseudotime file is plain text"):
        sweep.Pseudotime(pf, b)
    with pytest.raises(F.FastfError, match="pseudotime file: .*none.tsv does not exist"):
        sweep.Pseudotime(tmp_path / "none.tsv", b)
    L = _lib.lib()
    h = C.c_void_p(5)
    assert L.fastf_ptime_load(None, b"x", C.byref(h)) == 1 and not h.value
    assert L.fastf_ptime_known(None) == 0 and L.fastf_ptime_unknown(None) == 0 and L.fastf_ptime_valued(None) == 0
    L.fastf_ptime_free(None)
    assert L.fastf_ptime_assign(None, None, 0, None, None) == 1


# ---- the host twins ----
def _slots(lists, k, pad=NONE):
    idx = np.full((len(lists), k), pad, np.uint32)
    for i, nb in enumerate(lists):
        idx[i, :len(nb)] = nb
    return idx, np.array([len(nb) for nb in lists], np.uint32)


def random_fixture(n, k, seed, p_unvalued=0.25, ties=False):
    """(lists, idx, cnt, t, k): neighbour lists of every length from 0 to k; t with holes (and, ties: few distinct values)"""
    rng = np.random.default_rng(seed)
    t = rng.integers(1, 6 if ties else 2 * n + 1, size=n).astype(np.uint32) * 2
    t[rng.random(n) < p_unvalued] = 0
    lists = []
    for i in range(n):
        c = [0, 1, 2, k, k - 1][i % 5] if i < 10 else int(rng.integers(0, k + 1))
        lists.append(sorted(int(x) for x in rng.choice(n, size=min(max(c, 0), k, n), replace=False)))
    idx, cnt = _slots(lists, k)
    return lists, idx, cnt, t, k


def poisoned(fx, n):
    """the same lists with the slots from cnt[i] on filled with valid-looking indices of valued cells, and indices of n and beyond put
    into some lists: none of them may count"""
    lists, idx, cnt, t, k = fx
    idx = idx.copy()
    valued = np.flatnonzero(t)
    for i in range(len(cnt)):
        for s in range(int(cnt[i]), k):
            idx[i, s] = valued[(i + s) % len(valued)] if len(valued) and s % 2 else n + s
    return lists, idx, cnt, t, k


def check_medians(got, fx):
    lists, idx, cnt, t, k = fx
    est, valued = R.medians(lists, [int(x) for x in t])
    assert [int(x) for x in got[0]] == est and [int(x) for x in got[1]] == valued


@pytest.mark.parametrize("k", [1, 2, 15, 16, 17, 64])
@pytest.mark.parametrize("n", [1, 2, 65, 300])
def test_the_median_twin_on_random_lists(n, k):
    for ties in (False, True):
        fx = random_fixture(n, k, seed=n * 131 + k, ties=ties)
        check_medians(sweep.ptime_medians(fx[1], fx[2], fx[3], k), fx)
        check_medians(sweep.ptime_medians(*poisoned(fx, n)[1:4], k), fx)


def hand_fixture():
    """cells 0 .. 9, t = 2 (i + 1) but cells 8 and 9 without a value and cells 2, 3 tied at 6"""
    t = np.array([2, 4, 6, 6, 10, 12, 14, 16, 0, 0], np.uint32)
    lists = [[],                       # cnt 0
             [4],                      # one
             [0, 5],                   # even: the lower of the two
             [0, 1, 4, 5],             # even, four
             [2, 3, 7],                # duplicates below the median
             [0, 2, 3, 7],             # duplicates straddling the median: 2 | 6 6 | 16 -> 6
             [1, 2, 3, 4, 5],          # duplicates at the median
             [8, 9],                   # all neighbours unvalued
             [8, 0, 9, 6],             # unvalued among valued: 2 14 -> 2
             [0, 1, 2, 3, 4, 5, 6, 7, 8]]
    want = ([0, 10, 2, 4, 6, 6, 6, 0, 2, 6], [0, 1, 2, 4, 3, 4, 5, 0, 2, 8])
    return lists, t, want


@pytest.mark.parametrize("k", [9, 15, 64])
def test_the_median_twin_on_the_hand_built_lists(k):
    lists, t, want = hand_fixture()
    assert R.medians(lists, [int(x) for x in t]) == want
    idx, cnt = _slots(lists, k)
    fx = (lists, idx, cnt, t, k)
    for f in (fx, poisoned(fx, 10)):
        est, valued = sweep.ptime_medians(f[1], f[2], f[3], k)
        assert ([int(x) for x in est], [int(x) for x in valued]) == want
    over = cnt.copy(); over[9] = 200                        # more than k counts as k: the slots behind hold NONE, which is no index
    assert [int(x) for x in sweep.ptime_medians(idx, over, t, k)[0]] == want[0]
    for bad in (0, 65):
        with pytest.raises(F.FastfError, match="k = %d, from 1 to 64" % bad):
            _lib.check(_lib.lib().fastf_ptime_medians(idx.ctypes.data, cnt.ctypes.data, t.ctypes.data, 10, bad, idx.ctypes.data, idx.ctypes.data))


def census_cases():
    n = 40
    up = np.arange(1, n + 1, dtype=np.uint32) * 2
    rng = np.random.default_rng(3)
    mixed_e, mixed_t = rng.integers(0, 7, size=97).astype(np.uint32), rng.integers(0, 7, size=97).astype(np.uint32)
    return {
        "identity": (up, up, [n * (n - 1) // 2, 0, 0, 0, 0, n, 0]),
        "reversal": (up[::-1].copy(), up, [0, n * (n - 1) // 2, 0, 0, 0, n, None]),
        "all_e_equal": (np.full(n, 8, np.uint32), up, [0, 0, n * (n - 1) // 2, 0, 0, n, None]),
        "all_t_equal": (up, np.full(n, 8, np.uint32), [0, 0, 0, n * (n - 1) // 2, 0, n, None]),
        "all_equal": (np.full(n, 8, np.uint32), np.full(n, 8, np.uint32), [0, 0, 0, 0, n * (n - 1) // 2, n, 0]),
        "one_pair": (np.array([0, 4, 0, 2, 9], np.uint32), np.array([3, 2, 0, 6, 0], np.uint32), [0, 1, 0, 0, 0, 2, 6]),
        "one_cell": (np.array([0, 4, 0], np.uint32), np.array([3, 2, 0], np.uint32), [0, 0, 0, 0, 0, 1, 2]),
        "no_cells": (np.zeros(0, np.uint32), np.zeros(0, np.uint32), [0] * 7),
        "all_absent": (np.array([0, 4, 0], np.uint32), np.array([3, 0, 0], np.uint32), [0] * 7),
        "mixed": (mixed_e, mixed_t, None),
    }


@pytest.mark.parametrize("name", sorted(census_cases()))
def test_the_census_twin(name):
    est, t, want = census_cases()[name]
    ref = R.census([int(x) for x in est], [int(x) for x in t])
    got = [int(x) for x in sweep.ptime_census(est, t)]
    assert got == ref and sum(ref[:5]) == ref[5] * (ref[5] - 1) // 2
    if want:
        assert all(w is None or w == g for w, g in zip(want, got))
    tau = {"identity": "1.000000", "reversal": "-1.000000", "all_e_equal": "NA", "all_t_equal": "NA", "all_equal": "NA", "one_pair": "-1.000000",
           "one_cell": "NA", "no_cells": "NA", "all_absent": "NA"}
    if name in tau:
        assert R.tau_text(ref) == tau[name]
        row = sweep.ptime_summary_row(0.5, 0.25, 9, len(t), 7, got, got).rstrip("\n").split("\t")
        assert row[9] == tau[name] and row[14] == tau[name]


# ---- rows and headers ----
def test_headers_rows_and_the_na_rules():
    assert sweep.pseudotime_header() == "\t".join(sweep.POINT_PSEUDOTIME_COLUMNS) + "\n"
    for verb, mod in (("sweep", sweep), ("cap", cap), ("level", level)):
        assert sweep.pseudotime_header(verb) == "\t".join(mod.PSEUDOTIME_COLUMNS) + "\n"
    assert sweep.PSEUDOTIME_COLUMNS[:2] == ("rate_cell", "rate_depth") and cap.PSEUDOTIME_COLUMNS[1] == "reads_per_cell" and level.PSEUDOTIME_COLUMNS[1] == "umi_cap"
    assert sweep.PSEUDOTIME_COLUMNS[2:6] == ("seed", "n_cells", "k", "cells_valued") and sweep.PSEUDOTIME_COLUMNS[6:11] == ("cells_full", "conc_full", "disc_full", "tau_full", "shift_full")
    assert sweep.PSEUDOTIME_COLUMNS[-5:] == ("cells_map", "conc_map", "disc_map", "tau_map", "shift_map") and len(sweep.PSEUDOTIME_COLUMNS) == 21
    assert sweep.ptime_row("AAA-1", 6, 4, 3, 0, 0) == "AAA-1\t6\t4\t3\tNA\t0\tNA\tNA\n"
    assert sweep.ptime_row("AAA-1", 0, 0, 0, 8, 15, 0, 0) == "AAA-1\tNA\tNA\t0\t8\t15\tNA\t0\n"
    assert sweep.ptime_row("AAA-1", 4294967294, 2, 1, 2, 1, 10, 2) == "AAA-1\t4294967294\t2\t1\t2\t1\t10\t2\n"
    assert [r for r in R.cell_rows(["AAA-1"], [6], ([4], [3]), ([0], [0]))] == [sweep.ptime_row("AAA-1", 6, 4, 3, 0, 0).rstrip("\n").split("\t")]
    rng = np.random.default_rng(8)
    for trial in range(30):
        c = [[int(x) for x in rng.integers(0, 1 << int(rng.integers(1, 40)), size=7)] for _ in range(3)]
        if trial % 5 == 0:
            c[0][0] = c[0][1] = c[0][2] = 0                 # a zero denominator on one side
        if trial % 7 == 0:
            c[1][5] = 0
        m = int(rng.integers(0, 3)) * int(rng.integers(1, 1 << 20))
        for with_map in (False, True):
            row = sweep.ptime_summary_row(0.5, 0.25, 926, 1000, m, c[0], c[1], c[2] if with_map else None)
            assert row.rstrip("\n").split("\t") == R.summary_fields(["0.500", "0.250"], 926, 1000, 15, m, c[0], c[1], c[2] if with_map else None)
        row = sweep.ptime_summary_row(1, 0, 5, 10, m, c[0], c[1], list_value=12)
        assert row.split("\t")[:3] == ["1.000", "12", "5"]
    # conc below disc: the difference is taken as a signed 64-bit number
    neg = [1, 3, 0, 0, 0, 4, 0]
    assert sweep.ptime_summary_row(1, 1, 1, 1, 3, neg, neg).split("\t")[9] == R.tau_text(neg) == "-0.500000"


# ---- the interface ----
def test_the_entry_points_the_spellings_and_the_refusals(tmp_path):
    one, p_one = sweep._floats([1])
    caps = np.array([5], np.uint64)
    seeds = caps.astype(np.uint32)
    L = _lib.lib()
    for name in ("fastf_sweep_pseudotime", "fastf_cap_pseudotime", "fastf_level_pseudotime", "fastf_dev_ptime_medians", "fastf_dev_ptime_census", "fastf_ptime_medians",
                 "fastf_ptime_census", "fastf_ptime_load", "fastf_ptime_assign"):
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name)
    names = L.fastf_kernel_names().decode().split(",")
    assert "pt_median_kernel" in names and "pt_pairs_kernel" in names
    calls = (lambda fl, ns, mp: L.fastf_sweep_pseudotime(b"x", b"y", b"b", b"f", p_one, 1, p_one, 1, seeds.ctypes.data, ns, fl, 926, None, 0, mp, None),
             lambda fl, ns, mp: L.fastf_cap_pseudotime(b"x", b"y", b"b", b"f", p_one, 1, caps.ctypes.data, 1, seeds.ctypes.data, ns, fl, 926, None, 0, mp, None),
             lambda fl, ns, mp: L.fastf_level_pseudotime(b"x", b"y", b"b", b"f", p_one, 1, caps.ctypes.data, 1, seeds.ctypes.data, ns, fl, 926, None, 0, mp, None))
    for call in calls:                                      # pseudotime_path == NULL: exactly the _mapping calls, plain and replicate
        for ns in (0, 1):
            with pytest.raises(F.FastfError, match="does not exist"):
                _lib.check(call(4096 | 512 | 128 | 32 | 8 | 2 | 1, ns, 1))
            with pytest.raises(F.FastfError, match="--mapping: 2, 0 or 1"):
                _lib.check(call(0, ns, 2))
            for flags in (4, 16, 64, 256, 1024, 2048, 8192):      # no new bit
                with pytest.raises(F.FastfError, match="unknown flags"):
                    _lib.check(call(flags, ns, 0))
    bt, ft, bar, genes = synth.make_lists(5, 3)
    fl, xf, cb, gx, ub = synth.make_records(20, bar, genes)
    bam, b, f, pf = tmp_path / "x.bam", tmp_path / "b.tsv", tmp_path / "f.tsv", tmp_path / "pt.tsv"
    synth.write_bam(str(bam), fl, xf, cb, gx, ub)
    b.write_bytes(bt); f.write_bytes(ft)
    pf.write_bytes(b"".join(x + b"\t%d\n" % i for i, x in enumerate(bar.tolist())))
    with pytest.raises(F.FastfError, match="bam file: .* does not exist"):
        sweep.sweep(tmp_path / "no.bam", tmp_path / "o", b, f, [1], [1], pseudotime=pf)
    several = dict(os.environ, FASTF_DEVICES="0,1")
    for k, (verb, extra) in enumerate([("sweep", ["-r", "0.5"]), ("cap", ["-n", "5"]), ("level", ["-m", "5"])]):
        out = tmp_path / ("out%d" % k)
        base = [_lib.cli_path(), verb, "-o", str(out), "-a", str(b), "-f", str(f), "-b", str(bam)] + extra
        for more in ([], ["--fidelity", "--summary-only"], ["--seeds", "1,2"]):
            r = subprocess.run(base + ["--pseudotime", str(pf)] + more, capture_output=True, text=True, timeout=60, env=several)
            assert r.returncode == 1 and "several devices" in r.stderr, r.stderr
            assert "%s: --pseudotime needs the resident form" % verb in r.stderr
            assert not out.exists()                         # refused before the output directory is made
        for text, message in (("nobody\t1\n", "no line names a barcode"), ("%s\t1\t2\n" % bar[0].decode(), "line 1 has 3 fields"),
                              ("%s\t1\n%s\tone\n" % (bar[0].decode(), bar[1].decode()), "line 2: the value `one` is not a number"),
                              ("%s\tinf\n" % bar[0].decode(), "line 1: the value `inf` is not finite")):
            bad = tmp_path / "bad.tsv"
            bad.write_text(text)
            r = subprocess.run(base + ["--pseudotime=" + str(bad)], capture_output=True, text=True, timeout=60)
            assert r.returncode == 1 and message in r.stderr and "bad.tsv" in r.stderr and not out.exists(), r.stderr
        r = subprocess.run(base + ["--pseudotime", str(tmp_path / "none.tsv")], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "pseudotime file:" in r.stderr and "does not exist" in r.stderr and not out.exists()
        r = subprocess.run([_lib.cli_path(), verb, "--help"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and "--pseudotime=<file>" in r.stdout and "%s_pseudotime.tsv" % verb in r.stdout and "pseudotime.tsv.gz" in r.stdout
        for opt in (["-T", str(pf)], ["--pseudo", str(pf)], ["--pseudo=" + str(pf)]):    # the long form alone
            r = subprocess.run([_lib.cli_path(), verb] + opt + ["-o", str(out)], capture_output=True, text=True, timeout=60)
            assert r.returncode == 1 and "unknown option" in r.stderr
        r = subprocess.run([_lib.cli_path(), verb, "-o", str(out), "--pseudotime"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "option `--pseudotime` requires a value" in r.stderr and not out.exists()
    os.environ["FASTF_DEVICES"] = "0,1"
    try:
        with pytest.raises(F.FastfError, match="sweep: --pseudotime needs the resident form.*several devices"):
            sweep.sweep(bam, tmp_path / "o", b, f, [1], [1], pseudotime=pf)
        with pytest.raises(F.FastfError, match="cap: --pseudotime needs the resident form.*several devices"):
            cap.cap_reps(bam, tmp_path / "o", b, f, [1], [5], [1, 2], pseudotime=pf)
        with pytest.raises(F.FastfError, match="level: --mapping needs the resident form.*several devices"):      # (the first of the order that is set is named)
            level.level(bam, tmp_path / "o", b, f, [1], [5], pseudotime=pf, mapping=True)
    finally:
        del os.environ["FASTF_DEVICES"]
    assert not (tmp_path / "o").exists()


def test_the_tile_of_the_census_is_told():
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fastf_amd", "csrc", "ptime_kernels.hpp")).read()
    assert int(re.search(r"constexpr u32 PT_TILE = (\d+);", hdr).group(1)) == sweep.PTIME_TILE
