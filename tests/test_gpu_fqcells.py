"""fqcells on the MI355X against its definition in Python (tests/fqcells_ref.py): the per-barcode reduce on hand-built sorted
tables through its seam (fqc_heads_kernel, flt_sums_scan_kernel, fqc_rows_kernel; guard entries behind the three arrays), the
command through the CLI and in process for all three files byte for byte, and fqcells -k followed by fqcap -w against
tests/fqcap_ref.py fed the reference's own whitelist.  Every comparison is exact: bytes and integers."""
import ctypes as C
import functools
import gzip
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib

import filter_ref as R
import fqcap_ref as P
import fqcells_ref as Q

pytestmark = pytest.mark.gpu

OURS = _lib.cli_path()
GUARD = 16
RULE_ARG = {"e": "expect", "k": "top", "m": "min_umis"}
FILES = ("fqcells.tsv.gz", "whitelist.txt", "fqcells_summary.tsv")


# ---------------------------------------------------------------- 1. the seam
def reduce_dev(keys, counts, u):
    m1 = len(keys)
    bc, reads, umis = (np.full(m1 + GUARD, 0x11, dtype=t) for t in (np.uint64, np.uint64, np.uint32))
    n = C.c_size_t()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if len(a) else None  # noqa: E731
    _lib.check(_lib.lib().fastf_fqcells_reduce(ptr(keys), ptr(counts), m1, u, ptr(bc), ptr(reads), ptr(umis), C.byref(n)))
    B = n.value
    assert B <= m1
    for a, word in ((bc, 0xa5a5a5a5a5a5a5a5), (reads, 0xa5a5a5a5a5a5a5a5), (umis, 0xa5a5a5a5)):
        assert (a[B:B + GUARD] == word).all(), ("guard entries", a[B:B + GUARD])
    return [int(x) for x in bc[:B]], [int(x) for x in reads[:B]], [int(x) for x in umis[:B]]


def test_seam_tables_at_every_size_and_pattern():
    T = _lib.lib().fastf_fqcells_tile()
    fx = Q.seam_fixtures(T)
    assert len(fx) > 50
    for name, keys, counts, u in fx:
        got = reduce_dev(keys, counts, u)
        want = Q.reduce_ref(keys, counts, u)
        assert got[0] == want[0], name
        assert got[2] == want[2], name
        assert got[1] == want[1], name
        assert sum(got[2]) == len(keys) and sum(got[1]) == int(counts.astype(np.uint64).sum()), name


def test_seam_ignores_the_tag_bit_and_refuses_a_long_umi():
    keys = Q.keys_of_runs([3, 1, 2], 8, 4)
    counts = np.arange(1, 7, dtype=np.uint32)
    assert reduce_dev(keys & np.uint64(Q.TAG - 1), counts, 4) == reduce_dev(keys, counts, 4) == Q.reduce_ref(keys, counts, 4)
    with pytest.raises(F.FastfError):
        reduce_dev(keys, counts, 31)


# ---------------------------------------------------------------- 2. the command
def write(tmp, name, data):
    p = os.path.join(str(tmp), name)
    with open(p, "wb") as f:
        f.write(data)
    return p


@functools.lru_cache(maxsize=None)
def reference(name):
    case = {c[0]: c for c in Q.e2e_cases()}[name]
    return case, Q.py_fqcells(*case[1:])


def read_files(out):
    got = {n: open(os.path.join(str(out), n), "rb").read() for n in FILES}
    assert sorted(os.listdir(out)) == sorted(FILES)
    return dict(tsv=gzip.decompress(got[FILES[0]]), whitelist=got[FILES[1]], summary=got[FILES[2]])


def run_cli(r1, out, l, u, rule, arg, env=None, default_rule=False):
    os.makedirs(out, exist_ok=True)
    cmd = [OURS, "fqcells", "-R", r1, "-o", str(out), "-l", str(l), "-u", str(u)] + ([] if default_rule else ["-" + rule, str(arg)])
    p = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=300)
    assert p.returncode == 0, p.stderr
    return p


def check_files(out, ref):
    got = read_files(out)
    for k in ("summary", "whitelist", "tsv"):
        assert got[k] == ref[k], k
    return got


@pytest.mark.parametrize("name", [c[0] for c in Q.e2e_cases()])
def test_cases_cli(tmp_path, name):
    (_, text, l, u, rule, arg), ref = reference(name)
    p = run_cli(write(tmp_path, "r1.fq", text), tmp_path / "out", l, u, rule, arg, default_rule=name.startswith("default"))
    check_files(tmp_path / "out", ref)
    d = ref["dict"]
    assert p.stdout == "fqcells: %d reads, %d counted, %d barcodes, %d called (-%s %d: at least %d UMIs)\n" % (
        d["reads"], d["counted"], d["barcodes"], d["called"], rule, arg, d["threshold"])
    if name == "no_counted_read":
        assert ref["tsv"] == Q.HEADER and ref["whitelist"] == b"" and d["other"] == d["reads"] == 41


@pytest.mark.parametrize("name", ["e1100_rounds_up", "k_at_a_tie", "m8", "no_counted_read"])
def test_python_api_equals_cli(tmp_path, name):
    (_, text, l, u, rule, arg), ref = reference(name)
    r1 = write(tmp_path, "r1.fq", text)
    run_cli(r1, tmp_path / "a", l, u, rule, arg)
    os.makedirs(tmp_path / "b")
    d = F.fqcells(r1, out=tmp_path / "b", len_cb=l, len_umi=u, **{RULE_ARG[rule]: arg})
    assert d == ref["dict"]
    assert check_files(tmp_path / "b", ref) == read_files(tmp_path / "a")


def test_framings_and_small_windows_give_the_same_bytes(tmp_path):
    (_, text, l, u, rule, arg), ref = reference("e1100_rounds_up")
    for fmt in ("plain", "bgzf", "gzip"):
        run_cli(write(tmp_path, "r1." + fmt, R.encode(text, fmt)), tmp_path / fmt, l, u, rule, arg)
        check_files(tmp_path / fmt, ref)
    # sequence lines and the reads of one barcode straddle the windows
    for fmt, window in (("plain", 4096), ("bgzf", 4099)):
        out = tmp_path / ("w_" + fmt)
        run_cli(os.path.join(str(tmp_path), "r1." + fmt), out, l, u, rule, arg, env={"FASTF_FQ_WINDOW": str(window)})
        check_files(out, ref)


def test_refusals_that_need_the_device(tmp_path):
    """freq's declared divergences, each refused for its own reason (the message names the read) with nothing created"""
    text = Q.fastq_fixture()
    recs = R.records(text)
    long_line = [list(r) for r in recs]
    long_line[57][3] = b"F" * 1100 + b"\n"                       # read 58; the message names the read's first line, 229
    corrupt = bytearray(R.encode(text, "gzip"))
    corrupt[len(corrupt) // 2] ^= 0xff
    cases = [
        ("long_line.fq", b"".join(b"".join(r) for r in long_line), ("read 58 (line 229 of the file)", "longer than 1023 bytes")),
        ("long_open_last_line.fq", text + b"@last\n" + b"A" * 1024, ("read %d " % (len(recs) + 1), "longer than 1023 bytes")),
        ("truncated.fq", b"".join(b"".join(r) for r in recs[:100]) + b"@extra\n", ("ends after the header line of read 101",)),
        ("truncated_open.fq", b"".join(b"".join(r) for r in recs[:100]) + b"@extra", ("ends after the header line of read 101",)),
        ("corrupt.gz", bytes(corrupt), ("corrupt or truncated gzip stream",)),
    ]
    for name, data, words in cases:
        bad = write(tmp_path, name, data)
        out = tmp_path / ("o_" + name)
        out.mkdir()
        p = subprocess.run([OURS, "fqcells", "-R", bad, "-o", str(out)], capture_output=True, text=True, timeout=300)
        assert p.returncode == 1 and "ERROR: fastF fqcells: " in p.stderr, (name, p.stderr)
        for w in words:
            assert w in p.stderr, (name, w, p.stderr)
        assert os.listdir(out) == [], name


# ---------------------------------------------------------------- 3. fqcells -k, then fqcap -w: the -a that fqcap left out
def test_fqcells_then_fqcap(tmp_path):
    texts, pool, _ = P.triple()
    K, N = 25, 5
    cells = Q.py_fqcells(texts["R1"], 16, 12, "k", K)
    assert cells["whitelist"].count(b"\n") == K
    paths = {n: write(tmp_path, n + ".fq", texts[n]) for n in R.NAMES}
    run_cli(paths["R1"], tmp_path / "cells", 16, 12, "k", K)
    check_files(tmp_path / "cells", cells)
    out = tmp_path / "capped"
    out.mkdir()
    p = subprocess.run([OURS, "fqcap", "-R", paths["R1"], "-I", paths["I1"], "-r", paths["R2"], "-o", str(out), "-w",
                        str(tmp_path / "cells" / "whitelist.txt"), "-n", str(N)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    ref = P.py_fqcap(texts, cells["whitelist"], 16, 926, None, N)
    assert R.read_outputs(str(out), R.NAMES) == ref["out"] and P.read_tsv(out) == ref["tsv"]
    # the cap sees the cells fqcells counted: every DNA-form barcode's reads in fqcap_cells.tsv.gz are fqcells' reads
    reads = {r.split(b"\t")[0]: int(r.split(b"\t")[1]) for r in cells["tsv"].split(b"\n")[1:-1]}
    rows = [r.split(b"\t") for r in ref["tsv"].split(b"\n")[1:-1]]
    assert len(rows) == K and all(int(r[1]) >= reads[r[0]] for r in rows) and 0 < ref["n_kept"] < ref["n_matched"]
