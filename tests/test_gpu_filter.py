"""filter on the MI355X: decompressed I1/R1/R2.fastq.gz and stdout of `fastF filter` against the reference's own filter loop run
sequentially (tests/filter_ref.py: ref_driver, through oracle/_ref/libfastf_ref_tree.so) and against the plain-Python
restatement (py_filter), across input framings, whitelist forms, barcode lengths, rates, seeds, mate lengths, window sizes and
the refusals; the device draw stream, the Python binding, the drop-in fastF() and the freq -> filter pipeline."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib

import filter_ref as R

pytestmark = pytest.mark.gpu

OURS = _lib.cli_path()


def need_ref():
    if not os.path.exists(R.REF_TREE):
        pytest.skip("oracle/_ref/libfastf_ref_tree.so not built")


def write(tmp, name, data):
    p = os.path.join(str(tmp), name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def run_cli(paths, outdir, wl=None, args=(), env=None):
    os.makedirs(outdir, exist_ok=True)
    cmd = [OURS, "filter", "-R", paths["R1"], "-o", str(outdir)]
    if paths.get("I1"):
        cmd += ["-I", paths["I1"]]
    if paths.get("R2"):
        cmd += ["-r", paths["R2"]]
    if wl is not None:
        cmd += ["-w", wl]
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run(cmd + [str(a) for a in args], capture_output=True, text=True, env=e, timeout=900)


def check_case(tmp, texts, fmts, wl_bytes=None, len_cb=16, seed=926, rate=0.5, all_cells=False, env=None, use_ref=True):
    """write the inputs in the given framings, run the CLI, compare with the driver and the restatement"""
    paths = {}
    for name in R.NAMES:
        if texts.get(name) is None:
            paths[name] = None
            continue
        paths[name] = write(tmp, "%s.in.%s" % (name, fmts[name]), R.encode(texts[name], fmts[name]))
    wl = write(tmp, "wl.txt", wl_bytes) if wl_bytes is not None else None
    args = ["-l", len_cb, "-s", seed, "-t", repr(float(rate))] + (["-a"] if all_cells else [])
    out = os.path.join(str(tmp), "out")
    p = run_cli(paths, out, wl, args, env)
    assert p.returncode == 0, p.stderr
    nrow = len(R.lines(wl_bytes)) if wl_bytes is not None else 0
    assert p.stdout == R.ref_stdout(wl, nrow, r2=paths["R2"] is not None)
    present = [n for n in R.NAMES if paths[n]]
    got = R.read_outputs(out, present)
    exp = R.py_filter({n: texts.get(n) for n in R.NAMES}, wl_bytes, len_cb, seed, rate, all_cells)
    for n in present:
        assert got[n] == exp[n], n
    if use_ref and os.path.exists(R.REF_TREE):
        ref = R.ref_driver(paths, wl, len_cb, seed, rate, all_cells)
        for n in present:
            assert got[n] == ref[n], n
    for n in ("I1", "R2"):
        if not paths[n]:
            assert not os.path.exists(os.path.join(out, "%s.fastq.gz" % n))
    return got


def small_triple(n=3000, seed=5, n_cells=40):
    texts, pool = R.tenx_triple(n, seed=seed, n_cells=n_cells, p_other=0.3)
    return texts, pool


@pytest.mark.parametrize("names,fmts", [
    (("R1",), {"R1": "plain"}),
    (("R1", "R2"), {"R1": "gzip", "R2": "bgzf"}),
    (("I1", "R1", "R2"), {"I1": "members", "R1": "bgzf", "R2": "plain"}),
    (("I1", "R1", "R2"), {"I1": "plain", "R1": "members", "R2": "gzip"}),
])
def test_file_sets_and_framings(tmp_path, names, fmts):
    need_ref()
    texts, pool = small_triple()
    texts = {n: (texts[n] if n in names else None) for n in R.NAMES}
    fm = {n: fmts.get(n, "plain") for n in R.NAMES}
    wl = b"".join(b + b"\n" for b in pool[::2])
    check_case(tmp_path, texts, fm, wl, rate=0.5)


WHITELISTS = {
    "tenx": lambda pool: b"".join(b + b"\n" for b in pool[::2]),
    "barcodes_tsv": lambda pool: b"".join(b + b"-1\n" for b in pool[1::2]),
    "freq_whitelist": lambda pool: b"".join(b + b"ACGTACGTACGT,%d\n" % i for i, b in enumerate(pool[::3])),
    "odd": lambda pool: (pool[0] + b"\n" + b"ACGTNACGTACGTACG\n" + b"\n" + b"AC\n" + pool[1] + b"\r\n" + b"GGGG\n" +
                         pool[2][:10] + b"N\n" + pool[3]),
    "empty": lambda pool: b"",
}


@pytest.mark.parametrize("wl_kind", sorted(WHITELISTS))
@pytest.mark.parametrize("len_cb", [0, 12, 16, 31, 32, 40])
def test_whitelist_forms_and_lengths(tmp_path, wl_kind, len_cb):
    need_ref()
    texts, pool = small_triple(n=1500, seed=len_cb + 11)
    # reads whose sequence line is short, holds N, lowercase or CR: the escape path
    odd = [b"ACGT\n", b"AC\n", b"ACGTNNNNACGTACGTACGT\n", b"acgtacgtacgtacgtacgt\n", pool[1] + b"\r\n", b"\n", b"GGGG\n",
           pool[2][:10] + b"N" + b"A" * 20 + b"\n"]
    r1 = R.records(texts["R1"])
    for k, s in enumerate(odd * 10):
        r1[k * 7 + 3][1] = s
    texts["R1"] = b"".join(b"".join(r) for r in r1)
    check_case(tmp_path, {"I1": texts["I1"], "R1": texts["R1"], "R2": None}, {"I1": "gzip", "R1": "plain", "R2": "plain"},
               WHITELISTS[wl_kind](pool), len_cb=len_cb, rate=0.9)


@pytest.mark.parametrize("rate", [0.0, 0.1, 0.5, 1.0, 2.0])
@pytest.mark.parametrize("seed", [0, 926, -1])
def test_rates_and_seeds(tmp_path, rate, seed):
    need_ref()
    texts, pool = small_triple(n=2000, seed=3)
    wl = b"".join(b + b"\n" for b in pool[::2])
    check_case(tmp_path, {"I1": None, "R1": texts["R1"], "R2": texts["R2"]}, {"I1": "plain", "R1": "bgzf", "R2": "gzip"}, wl,
               seed=seed, rate=rate)


@pytest.mark.parametrize("with_wl", [False, True])
def test_all_cells(tmp_path, with_wl):
    need_ref()
    texts, pool = small_triple(n=2000, seed=4)
    wl = b"".join(b + b"\n" for b in pool[:3]) if with_wl else None
    check_case(tmp_path, texts, {"I1": "plain", "R1": "plain", "R2": "plain"}, wl, rate=0.3, all_cells=True)


@pytest.mark.parametrize("i1_n,r2_n", [(1000, 3000), (2500, 1200)])
def test_mates_shorter_and_longer(tmp_path, i1_n, r2_n):
    need_ref()
    texts, pool = small_triple(n=2000, seed=6)
    big, _ = R.tenx_triple(3000, seed=7)
    cut = lambda t, n: b"".join(b"".join(r) for r in R.records(t)[:n])  # noqa: E731
    texts["I1"] = cut(big["I1"], i1_n)
    texts["R2"] = cut(big["R2"], r2_n)
    wl = b"".join(b + b"\n" for b in pool[::2])
    check_case(tmp_path, texts, {"I1": "gzip", "R1": "plain", "R2": "members"}, wl, rate=0.7)


def test_last_qual_line_without_newline(tmp_path):
    need_ref()
    texts, pool = small_triple(n=500, seed=8)
    for n in R.NAMES:
        texts[n] = texts[n][:-1]
    check_case(tmp_path, texts, {"I1": "plain", "R1": "gzip", "R2": "bgzf"}, None, rate=1.0, all_cells=True)


@pytest.mark.parametrize("window", [4096, 4099, 6151, 65537])
def test_odd_windows(tmp_path, window):
    need_ref()
    texts, pool = small_triple(n=4000, seed=9)
    # uneven record lengths so that records straddle window ends at every offset
    rng = np.random.default_rng(window)
    for n in R.NAMES:
        rs = R.records(texts[n])
        for r in rs:
            r[0] = b"@" + b"x" * int(rng.integers(1, 300)) + b"\n"
        texts[n] = b"".join(b"".join(r) for r in rs)
    wl = b"".join(b + b"\n" for b in pool[::2])
    check_case(tmp_path, texts, {"I1": "bgzf", "R1": "plain", "R2": "gzip"}, wl, rate=0.6,
               env={"FASTF_FQ_WINDOW": str(window)})


def test_rate_one_drops_the_draw_that_rounds_to_one(tmp_path):
    need_ref()
    # a seed whose draws among the first 100 000 reads include one at or above 2^31 - 64 (rounds to 2^31: draw == 1.0)
    seed, hit = None, None
    for s in range(1, 2000):
        d = F.filter_draws(s, 0, 100_000, device=False)
        k = np.nonzero(d >= (1 << 31) - 64)[0]
        if len(k):
            seed, hit = s, int(k[0])
            break
    assert seed is not None
    texts, pool = R.tenx_triple(hit + 10, seed=10)
    got = check_case(tmp_path, {"I1": None, "R1": texts["R1"], "R2": None}, {"I1": "plain", "R1": "plain", "R2": "plain"}, None,
                     seed=seed, rate=1.0, all_cells=True, use_ref=hit < 20000)
    n_out = len(R.records(got["R1"]))
    assert n_out == hit + 10 - 1
    assert b"@r%-*d\n" % (len("@r%d\n" % (hit + 9)) - 3, hit) not in got["R1"]


def test_refusals(tmp_path):
    texts, pool = small_triple(n=200, seed=12)
    good = write(tmp_path, "good.fq", texts["R1"])
    head = b"".join(b"".join(r) for r in R.records(texts["R1"])[:100])       # ends inside the 200 reads of the other file
    cases = {
        "long_line": texts["R1"].replace(R.records(texts["R1"])[57][3], b"F" * 1100 + b"\n", 1),
        "truncated": head + b"@extra\nACGT\n",
        "trailing_blank": head + b"\n",
    }
    for name, data in cases.items():
        for fmt in ("plain", "gzip"):
            bad = write(tmp_path, "%s.%s" % (name, fmt), R.encode(data, fmt))
            for role in ("R1", "R2"):
                paths = {"R1": bad, "R2": good} if role == "R1" else {"R1": good, "R2": bad}
                p = run_cli(paths, tmp_path / ("o_%s_%s_%s" % (name, fmt, role)), None, ["-a", "-t", "1"])
                assert p.returncode == 1, (name, fmt, role, p.stderr)
                assert os.path.basename(bad) in p.stderr and "read " in p.stderr, p.stderr
    corrupt = bytearray(gzip.compress(texts["R1"]))
    corrupt[len(corrupt) // 2] ^= 0xff
    p = run_cli({"R1": write(tmp_path, "corrupt.gz", bytes(corrupt))}, tmp_path / "o_c", None, ["-a"])
    assert p.returncode == 1 and "corrupt.gz" in p.stderr
    truncated = gzip.compress(texts["R1"])[:-100]
    p = run_cli({"R1": write(tmp_path, "trunc.gz", truncated)}, tmp_path / "o_t", None, ["-a"])
    assert p.returncode == 1 and "trunc.gz" in p.stderr


def test_2m_reads_tenx(tmp_path):
    texts, pool = R.tenx_triple(2_000_000, seed=13, n_cells=5000)
    wl = b"".join(b + b"-1\n" for b in pool[::2])
    check_case(tmp_path, texts, {"I1": "bgzf", "R1": "bgzf", "R2": "plain"}, wl, rate=0.4, use_ref=False)


def test_8m_reads_same_bytes_in_every_framing(tmp_path):
    n = 8_000_000
    texts, pool = R.tenx_triple(n, seed=14, n_cells=20000)
    wl = write(tmp_path, "wl.txt", b"".join(b + b"\n" for b in pool[::2]))
    first = None
    for fmt in ("plain", "bgzf", "members"):
        paths = {k: write(tmp_path, "%s.%s" % (k, fmt), R.encode(texts[k], fmt)) for k in R.NAMES}
        out = tmp_path / ("o_" + fmt)
        p = run_cli(paths, out, wl, ["-t", "0.5"])
        assert p.returncode == 0, p.stderr
        got = R.read_outputs(str(out), R.NAMES)
        for k in R.NAMES:
            os.remove(paths[k])
        if first is None:
            first = got
            n_kept = len(R.records(got["R1"]))
            assert 0.2 * n < n_kept < 0.45 * n
            assert len(R.records(got["I1"])) == len(R.records(got["R2"])) == n_kept
        else:
            assert got == first, fmt


@pytest.mark.parametrize("first", [0, 123_456_789])
def test_device_draws_equal_host_stream(first):
    n = 50_000_000
    dev = F.filter_draws(926, first, n)
    host = F.filter_draws(926, first, n, device=False)
    assert np.array_equal(dev, host)
    assert int(dev[0]) == F.filter_rand_at(926, first) and int(dev[-1]) == F.filter_rand_at(926, first + n - 1)


def test_python_api_and_dropin_equal_cli(tmp_path):
    need_ref()
    texts, pool = small_triple(n=5000, seed=15)
    paths = {k: write(tmp_path, "%s.fq.gz" % k, R.encode(texts[k], "gzip")) for k in R.NAMES}
    wl = write(tmp_path, "wl.txt", b"".join(b + b"\n" for b in pool[::2]) + b"AC\n")
    p = run_cli(paths, tmp_path / "cli", wl, ["-l", 16, "-s", 77, "-t", 0.5])
    assert p.returncode == 0, p.stderr
    cli = R.read_outputs(str(tmp_path / "cli"), R.NAMES)
    os.makedirs(tmp_path / "py")
    nr, nk = F.filter(paths["R1"], paths["I1"], paths["R2"], out=tmp_path / "py", whitelist=wl, len_cb=16, seed=77, rate=0.5)
    assert nr == 5000 and nk == len(R.records(cli["R1"]))
    assert R.read_outputs(str(tmp_path / "py"), R.NAMES) == cli
    # drop-in fastF(): libz gzFiles, the reference's own tree
    z = R._zlib()
    tree, _ = R.ref_tree(wl)
    fin, fout = (C.c_void_p * 3)(), (C.c_void_p * 3)()
    os.makedirs(tmp_path / "dropin")
    for k, name in enumerate(R.NAMES):
        fin[k] = z.gzopen(paths[name].encode(), b"r")
        fout[k] = z.gzopen(str(tmp_path / "dropin" / ("%s.fastq.gz" % name)).encode(), b"w")
    L = _lib.lib()
    L.fastF.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_float, C.c_bool]
    L.fastF.restype = None
    L.fastF(fin, fout, tree, 16, 77, 0.5, False)
    for k in range(3):
        z.gzclose(fin[k])
        z.gzclose(fout[k])
    assert R.read_outputs(str(tmp_path / "dropin"), R.NAMES) == cli


def test_freq_whitelist_feeds_filter(tmp_path):
    need_ref()
    texts, pool = small_triple(n=20000, seed=16, n_cells=300)
    r1 = write(tmp_path, "R1.fq", texts["R1"])
    p = subprocess.run([OURS, "freq", "-R", r1, "-o", str(tmp_path), "-l", "16", "-u", "0"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    wl_bytes = open(tmp_path / "whitelist.txt", "rb").read()
    # keep the barcodes seen at least 20 times, as a user would
    kept = b"".join(ln for ln in R.lines(wl_bytes) if int(ln.rsplit(b",", 1)[1]) >= 20)
    assert kept
    check_case(tmp_path, {"I1": None, "R1": texts["R1"], "R2": texts["R2"]}, {"I1": "plain", "R1": "plain", "R2": "gzip"}, kept,
               len_cb=16, rate=0.8)
