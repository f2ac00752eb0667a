"""fqcap without a GPU: fastf_fqcap_rate against numpy, the refusals of the command line (each by name, exit 1, nothing created),
the help text, and the census of the fixtures tests/test_gpu_fqcap.py caps — asserted on the reference (tests/fqcap_ref.py) alone."""
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib

import fqcap_ref as Q

OURS = _lib.cli_path()


def bits(x):
    return int(np.float32(x).view(np.uint32))


@pytest.mark.parametrize("t", [0.0, 0.1, 1.0, 2.0])
def test_rate_equals_the_numpy_restatement(t):
    for cap in (1, 2, 5, 50, 51, 10 ** 9, 2 ** 32 - 1):
        hs = {0, 1, cap - 1, cap, cap + 1, 2 * cap, 2 * cap + 1, 3 * cap + 1, 7 * cap, 2 ** 32 - 1}
        for h in sorted(x for x in hs if 0 <= x < 2 ** 32):
            got = F.fqcap_rate(cap, h, t)
            assert bits(got) == bits(Q.rate_of(cap, h, t)), (cap, h, t, got)
            if h <= cap:
                assert bits(got) == bits(t)
            else:
                assert got <= float(np.float32(t)) and got <= cap / h * (1 + 2.0 ** -23)
    # N = 1 against the largest count a 32-bit counter holds: 2^-32 exactly
    assert F.fqcap_rate(1, 2 ** 32 - 1, 2.0) == float(np.float32(1.0 / (2 ** 32 - 1))) == 2.0 ** -32


def run(args, cwd=None):
    return subprocess.run([OURS, "fqcap"] + [str(a) for a in args], capture_output=True, text=True, cwd=cwd, timeout=120)


@pytest.fixture()
def inputs(tmp_path):
    texts, pool, wl = Q.triple(n=1300, seed=2, n_cells=10)
    d = tmp_path / "in"
    d.mkdir()
    (d / "r1.fq").write_bytes(texts["R1"])
    (d / "wl.txt").write_bytes(wl)
    out = tmp_path / "out"
    out.mkdir()
    return str(d / "r1.fq"), str(d / "wl.txt"), out


def refused(p, out, *words):
    assert p.returncode == 1, (p.returncode, p.stdout, p.stderr)
    for w in words:
        assert w in p.stderr, (w, p.stderr)
    assert os.listdir(out) == []


def test_refusals_by_name_with_nothing_created(inputs, tmp_path):
    r1, wl, out = inputs
    base = ["-R", r1, "-w", wl, "-o", out]
    refused(run(base), out, "-n")                                         # no -n
    for bad in ("0", "00", "-5", "+5", "5x", "1e3", "0x10", "", " 5", "5.0", "99999999999999999999999"):
        refused(run(base + ["-n", bad]), out, "-n", "digits")
    refused(run(["-R", r1, "-o", out, "-n", "5"]), out, "-w")            # no -w
    p = run(base + ["-n", "5", "-a"])                                     # -a is filter's, not this verb's
    refused(p, out, "-a")
    assert "unknown option" in p.stderr
    refused(run(base + ["-n", "5", "--allcells"]), out, "--allcells")
    refused(run(["-w", wl, "-o", out, "-n", "5"]), out, "-R")
    refused(run(base + ["-n", "5", "-l", "-1"]), out, "-l", "negative")
    refused(run(["-R", r1, "-w", wl, "-n", "5", "-o", tmp_path / "missing"]), out, "-o", str(tmp_path / "missing"))
    f = tmp_path / "a_file"
    f.write_bytes(b"")
    refused(run(["-R", r1, "-w", wl, "-n", "5", "-o", f]), out, "-o")
    if os.geteuid() != 0:                                                 # (root writes anywhere)
        ro = tmp_path / "ro"
        ro.mkdir()
        os.chmod(ro, 0o555)
        refused(run(["-R", r1, "-w", wl, "-n", "5", "-o", ro]), ro, "-o")
    refused(run(["-R", tmp_path / "none.fq", "-w", wl, "-o", out, "-n", "5"]), out, "none.fq")
    with pytest.raises(ValueError):
        F.fqcap(r1, out=out, whitelist=wl, cap=0)
    with pytest.raises(ValueError):
        F.fqcap(r1, out=out, whitelist=None, cap=5)
    assert os.listdir(out) == []


def test_help_names_every_option_and_says_in_expectation():
    p = run(["-h"])
    assert p.returncode == 0
    for opt in ("-h, --help", "-I, --I1", "-R, --R1", "-r, --R2", "-o, --out", "-w, --whitelist", "-n, --reads", "-l, --len", "-s, --seed",
                "-t, --rate"):
        assert opt in p.stdout, opt
    assert "--allcells" not in p.stdout and "in expectation" in p.stdout and "fqcap_cells.tsv.gz" in p.stdout
    top = subprocess.run([OURS, "-h"], capture_output=True, text=True)
    assert top.returncode == 0 and "\n    fqcap " in top.stdout
    assert "fastf_fqcap" in _lib.ABI_SYMBOLS
    names = _lib.lib().fastf_kernel_names().decode().split(",")
    assert "fcp_count_kernel" in names and "fcp_rec_kernel" in names


@pytest.mark.parametrize("cap", Q.CAPS)
def test_census_of_the_gpu_fixtures(cap):
    """every fixture the GPU tests cap has cells on both sides of the cap, one at it, one just above it and an escape-form cell
    above it — by the reference alone.  (The fourth cap of the GPU tests, 10^9, is above every cell on purpose: the no-cap case.)"""
    fx = Q.fixtures()
    assert [f[0] for f in fx] == ["main", "duplicates", "shared_prefixes"]
    for name, texts, wl, len_cb in fx:
        c = Q.census(texts, wl, len_cb, cap)
        assert c["above"] >= 5 and c["at_or_below"] >= 1 and c["exact"] >= 1 and c["plus_one"] >= 1 and c["esc_above"] >= 1, (name, c)
        assert Q.census(texts, wl, len_cb, 10 ** 9)["above"] == 0


def test_reference_consequences_and_cell_count():
    """the reference itself: no cap = filter, a cap keeps a subset, duplicate and prefix-sharing lines make no extra cells"""
    import filter_ref as R
    fx = Q.fixtures()
    name, texts, wl, len_cb = fx[0]
    for t in (None, 0.5):
        full = Q.py_fqcap(texts, wl, len_cb, 926, t, 10 ** 9)
        assert full["out"] == R.py_filter(texts, wl, len_cb, 926, 2.0 if t is None else t)
        for cap in Q.CAPS:
            r = Q.py_fqcap(texts, wl, len_cb, 926, t, cap)
            assert all(f or not k for k, f in zip(r["keep"], full["keep"])) and r["n_kept"] <= full["n_kept"]
            assert r["n_kept"] < full["n_kept"] or (t == 0.5 and cap == 50)      # (50 / h > 0.5 for every cell of the fixture)
            assert sum(r["kept"].values()) == r["n_kept"] and r["n_matched"] == sum(r["h"].values())
    plain = b"".join(c[:12] + b"\n" for c in sorted(Q.py_fqcap(texts, wl, 16, 926, None, 5)["h"]))
    want = Q.py_fqcap(texts, plain, 12, 926, None, 5)
    for name, texts, w, len_cb in fx[1:]:
        got = Q.py_fqcap(texts, w, len_cb, 926, None, 5)
        assert got["tsv"] == want["tsv"] and got["out"] == want["out"], name
