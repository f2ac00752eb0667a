"""fqcap on the MI355X against its definition in Python (tests/fqcap_ref.py, built on filter_ref.py): the device seam window by
window (fcp_count_kernel, fcp_rec_kernel; guard words behind hits, kept and rate), the command through the CLI and in process
across caps, rates, seeds, barcode lengths, whitelist forms, framings, window sizes and mate lengths, the two consequences of the
definition (no cap = filter's bytes, run here; any cap keeps a subset of filter's reads), fqcap_cells.tsv.gz and the refusals
that need the device.  Every comparison is exact: bytes and integers."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib

import filter_ref as R
import fltwin_ref as W
import fqcap_ref as Q
from test_gpu_filter import WHITELISTS
from test_gpu_filter_windows import Dev, Esc, random_states

pytestmark = pytest.mark.gpu

OURS = _lib.cli_path()
HDR, NONE, GUARD, GUARD_WORD = W.FLT_HDR, W.NONE, 16, 0xa5a5a5a5


# ---------------------------------------------------------------- 1. the window seam
def seam_api(L):
    vp, u32, u64, sz = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t
    L.fastf_fcpdev_begin.argtypes = [vp]
    L.fastf_fcpdev_count.argtypes = [vp, u32, C.POINTER(C.POINTER(Esc)), C.POINTER(u32)]
    L.fastf_fcpdev_set_rates.argtypes = [vp, vp, sz]
    L.fastf_fcpdev_decide.argtypes = [vp, u32, C.c_float, vp, C.POINTER(C.POINTER(Esc)), C.POINTER(u32)]
    L.fastf_fcpdev_draws.argtypes = [vp, vp, u64]
    L.fastf_fcpdev_read.argtypes = [vp, C.c_int, vp, sz]
    return L


def stage(dev, t, a, ln, tv):
    """the staging of one window as filter_cmds.c builds it (test_gpu_filter_windows.Dev.feed does the same)"""
    st, n = dev.stage, ln - (tv != NONE)
    h = min(a, HDR)
    st[:HDR - h] = 0
    st[HDR - h:HDR] = t[a - h:a]
    st[HDR:HDR + n] = t[a:a + n]
    if tv != NONE:
        st[HDR + n] = 10
    st[HDR + ln:HDR + ln + 64] = 0


def read_words(dev, which, n_keys):
    out = np.zeros(n_keys + GUARD, dtype=np.uint32)
    _lib.check(dev.L.fastf_fcpdev_read(dev.h, which, out.ctypes.data_as(C.c_void_p), len(out)))
    assert (out[n_keys:] == GUARD_WORD).all(), ("guard words", which, out[n_keys:])
    return out[:n_keys]


def seam_case(reads_cb, keys_cb, cap, t, lens0, lens1, L=16, Wb=1 << 16):
    """reads_cb: the 16-base barcode (or any bytes) of every read; keys_cb: the whitelist's DNA-form barcodes.  Pass 0 through the
    windows lens0, pass 1 through lens1 (byte counts; None: one window), against the definition element by element"""
    text = b"".join(b"@r%d\n" % i + cb + b"ACGTACGTACGT\n+\n" + b"F" * (len(cb) + 12) + b"\n" for i, cb in enumerate(reads_cb))
    tarr = np.frombuffer(text, dtype=np.uint8)
    fr = W.Framing(text) if text else None
    n = len(reads_cb)
    keys = sorted({W.dna_key(cb, L) for cb in keys_cb})
    assert all(keys)
    index = {k: j for j, k in enumerate(keys)}
    key_of = [W.dna_key(cb + b"ACGTACGTACGT", L) for cb in reads_cb]
    want_h = np.zeros(len(keys), dtype=np.uint32)
    for k in key_of:
        if k in index:
            want_h[index[k]] += 1
    want_esc = [r for r, k in enumerate(key_of) if not k]
    with Dev(Wb) as dev:
        seam_api(dev.L)
        dev.set_whitelist(keys)
        _lib.check(dev.L.fastf_fcpdev_begin(dev.h))
        assert (read_words(dev, 2, len(keys)) == GUARD_WORD).all()
        # ---- pass 0
        dev.poison()
        wins0 = fr.windows(lens0 or [len(text)]) if text else [(0, 0, NONE, 0, 0)]
        got_esc = []
        for a, ln, tv, r_lo, n_rec in wins0:
            stage(dev, tarr, a, ln, tv)
            assert dev.parse(ln, a, tv, NONE) == (r_lo, n_rec)
            pe, ne = C.POINTER(Esc)(), C.c_uint32()
            _lib.check(dev.L.fastf_fcpdev_count(dev.h, L, C.byref(pe), C.byref(ne)))
            got_esc += [r_lo + pe[q].i for q in range(ne.value)]
            for q in range(ne.value):                                   # s1: where the read's sequence line stands in the buffer
                assert pe[q].s1 == int(fr.start[4 * (r_lo + pe[q].i) + 1]) - a + HDR
        assert np.array_equal(read_words(dev, 0, len(keys)), want_h)
        assert sorted(got_esc) == want_esc
        assert (read_words(dev, 1, len(keys)) == 0).all()
        # ---- between: the rates of the definition
        rates = np.array([Q.rate_of(cap, int(h), t) for h in want_h], dtype=np.float32)
        assert np.array_equal(rates.view(np.uint32), np.array([np.float32(F.fqcap_rate(cap, int(h), t)) for h in want_h],
                                                              dtype=np.float32).view(np.uint32))
        _lib.check(dev.L.fastf_fcpdev_set_rates(dev.h, rates.ctypes.data_as(C.c_void_p) if len(rates) else None, len(rates)))
        assert np.array_equal(read_words(dev, 2, len(keys)), rates.view(np.uint32))
        # ---- pass 1
        _lib.check(dev.L.fastf_fltdev_reset(dev.h))
        wins1 = fr.windows(lens1 or [len(text)]) if text else [(0, 0, NONE, 0, 0)]
        want_kept = np.zeros(len(keys), dtype=np.uint32)
        n_kept = 0
        for a, ln, tv, r_lo, n_rec in wins1:
            stage(dev, tarr, a, ln, tv)
            assert dev.parse(ln, a, tv, NONE) == (r_lo, n_rec)
            states = random_states(r_lo, n_rec)
            if n_rec:
                s = np.ascontiguousarray(states, dtype=np.uint32).reshape(-1)
                dev.cs[:len(s)] = s
            draws = W.chunk_draws(states, n_rec) if n_rec else np.zeros(0, np.uint32)
            pe, ne = C.POINTER(Esc)(), C.c_uint32()
            _lib.check(dev.L.fastf_fcpdev_decide(dev.h, L, t, dev.p_cs, C.byref(pe), C.byref(ne)))
            esc = sorted(pe[q].i for q in range(ne.value))
            if n_rec:
                back = np.zeros(n_rec, dtype=np.uint32)
                _lib.check(dev.L.fastf_fcpdev_draws(dev.h, back.ctypes.data_as(C.c_void_p), n_rec))
                assert np.array_equal(back, draws)
            pass_t = W.passes(draws, t)
            assert esc == [i for i in range(n_rec) if not key_of[r_lo + i] and pass_t[i]]
            keep = []
            for i in range(n_rec):
                j = index.get(key_of[r_lo + i])
                if j is not None and pass_t[i] and W.passes(draws[i:i + 1], rates[j])[0]:
                    keep.append(r_lo + i)
                    want_kept[j] += 1
            po, tot = C.c_void_p(), C.c_size_t()
            _lib.check(dev.L.fastf_fltdev_emit(dev.h, None, 0, C.byref(po), C.byref(tot)))
            out = C.string_at(po.value, tot.value) if tot.value else b""
            assert out == b"".join(fr.out(r) for r in keep), (a, ln)
            n_kept += len(keep)
        assert np.array_equal(read_words(dev, 1, len(keys)), want_kept)
        assert np.array_equal(read_words(dev, 0, len(keys)), want_h)
        n_nl, kept, err, err_rec = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint64()
        _lib.check(dev.L.fastf_fltdev_end(dev.h, C.byref(n_nl), C.byref(kept), C.byref(err), C.byref(err_rec), None))
        assert (n_nl.value, kept.value, err.value) == (4 * n, n_kept, 0)
    return want_h, want_kept


def barcode(k):
    return bytes(b"ACGT"[(k >> (2 * j)) & 3] for j in range(16))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_seam_read_counts(n):
    rng = np.random.default_rng(n)
    cells = [barcode(int(k)) for k in rng.integers(0, 1 << 32, size=9)]
    pick = rng.integers(0, 12, size=n)                          # 9 listed cells, 2 unlisted, one escape form
    reads = [cells[p] if p < 9 else (barcode(7 + int(p)) if p < 11 else b"ACGTNACGTACGTACG") for p in pick]
    h, kept = seam_case(reads, cells, cap=5, t=2.0, lens0=None, lens1=None)
    if n >= 255:
        assert h.max() > 6 and 0 < kept.sum() < h.sum()


def test_seam_one_cell_owns_every_read():
    h, kept = seam_case([barcode(99)] * 300, [barcode(5), barcode(99), barcode(1 << 31)], cap=50, t=2.0, lens0=None, lens1=None)
    assert h.max() == 300 and 20 < kept.sum() < 90


def test_seam_every_read_its_own_cell():
    cells = [barcode(1000 + 17 * k) for k in range(300)]
    h, kept = seam_case(cells, cells, cap=1, t=0.5, lens0=None, lens1=None)
    assert (h == 1).all() and 100 < kept.sum() < 200            # h = N: the global rate alone


def test_seam_two_cells_alternating_lane_by_lane():
    a, b = barcode(3), barcode(0xfffffffe)
    h, kept = seam_case([a, b] * 160, [a, b, barcode(77)], cap=16, t=2.0, lens0=None, lens1=None)
    assert sorted(h) == [0, 160, 160] and 8 < kept.sum() < 70


def test_seam_passes_cut_differently_and_cells_span_windows():
    rng = np.random.default_rng(11)
    cells = [barcode(int(k)) for k in rng.integers(0, 1 << 32, size=6)]
    reads = [cells[int(p)] if p < 6 else b"NNNN" for p in rng.integers(0, 7, size=400)]
    n_bytes = sum(len(b"@r%d\n" % i) + 2 * (len(cb) + 12) + 4 for i, cb in enumerate(reads))
    cut = lambda w: [w] * (n_bytes // w) + [n_bytes % w]  # noqa: E731
    seam_case(reads, cells, cap=20, t=0.9, lens0=cut(4096), lens1=cut(4099) + [0], Wb=8192)


# ---------------------------------------------------------------- 2. the command
def write(tmp, name, data):
    p = os.path.join(str(tmp), name)
    with open(p, "wb") as f:
        f.write(data)
    return p


@functools.lru_cache(maxsize=None)
def main_fixture():
    return Q.triple()


@functools.lru_cache(maxsize=None)
def reference(i1, r1, r2, wl, len_cb, seed, rate, cap):
    """py_fqcap of a case, computed once and shared by the tests that run it"""
    return Q.py_fqcap({"I1": i1, "R1": r1, "R2": r2}, wl, len_cb, seed, rate, cap)


def args_of(len_cb, seed, rate, cap):
    return ["-l", len_cb, "-s", seed, "-n", cap] + ([] if rate is None else ["-t", repr(float(rate))])


def run_cli(verb, paths, outdir, wl, args, env=None):
    os.makedirs(outdir, exist_ok=True)
    cmd = [OURS, verb, "-R", paths["R1"], "-o", str(outdir), "-w", wl]
    if paths.get("I1"):
        cmd += ["-I", paths["I1"]]
    if paths.get("R2"):
        cmd += ["-r", paths["R2"]]
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run(cmd + [str(a) for a in args], capture_output=True, text=True, env=e, timeout=300)


def check_outputs(outdir, ref, present, counts=None):
    got = R.read_outputs(str(outdir), present)
    for n in present:
        assert got[n] == ref["out"][n], n
    for n in R.NAMES:
        if n not in present:
            assert not os.path.exists(os.path.join(str(outdir), "%s.fastq.gz" % n))
    tsv = Q.read_tsv(outdir)
    assert tsv == ref["tsv"]
    rows = [ln.split(b"\t") for ln in tsv.split(b"\n")[1:-1]]
    assert sum(int(r[2]) for r in rows) == ref["n_kept"] and sum(int(r[1]) for r in rows) == ref["n_matched"]
    if counts is not None:
        assert tuple(counts) == (ref["n_reads"], ref["n_matched"], ref["n_kept"])
    return got


def check_case(tmp, texts, wl_bytes, len_cb=16, seed=926, rate=None, cap=5, fmts=None, env=None, cli=True):
    fmts = fmts or {}
    paths = {n: (write(tmp, "%s.in" % n, R.encode(texts[n], fmts.get(n, "plain"))) if texts.get(n) is not None else None)
             for n in R.NAMES}
    wl = write(tmp, "wl.txt", wl_bytes)
    ref = reference(texts.get("I1"), texts["R1"], texts.get("R2"), wl_bytes, len_cb, seed, rate, cap)
    present = [n for n in R.NAMES if paths[n]]
    out = os.path.join(str(tmp), "out")
    if cli:
        p = run_cli("fqcap", paths, out, wl, args_of(len_cb, seed, rate, cap), env)
        assert p.returncode == 0, p.stderr
        assert p.stdout == "fqcap: %d reads, %d matched, %d kept (cap %d reads per cell)\n" % (
            ref["n_reads"], ref["n_matched"], ref["n_kept"], cap)
        counts = None
    else:
        os.makedirs(out)
        counts = F.fqcap(paths["R1"], paths["I1"], paths["R2"], out=out, whitelist=wl, len_cb=len_cb, seed=seed,
                         rate=2.0 if rate is None else rate, cap=cap)
    return check_outputs(out, ref, present, counts), ref, paths, wl


@pytest.mark.parametrize("rate", [None, 0.5])
@pytest.mark.parametrize("cap", [1, 5, 50, 10 ** 9])
def test_caps_and_rates_cli(tmp_path, cap, rate):
    texts, pool, wl = main_fixture()
    got, ref, paths, wlp = check_case(tmp_path, texts, wl, rate=rate, cap=cap)
    # n_matched = n_kept of filter -t 2; with no cell above the cap the bytes are filter's; under any cap a subset of filter's reads
    t = 2.0 if rate is None else rate
    flt = R.py_filter(texts, wl, 16, 926, t)
    kept_by_filter = {b"".join(r) for r in R.records(flt["R1"])}
    assert all(b"".join(r) in kept_by_filter for r in R.records(got["R1"]))
    assert ref["n_matched"] == len(R.records(R.py_filter(texts, wl, 16, 926, 2.0)["R1"]))
    if cap == 10 ** 9:
        p = run_cli("filter", paths, tmp_path / "flt", wlp, ["-l", 16, "-s", 926, "-t", repr(t)])
        assert p.returncode == 0, p.stderr
        assert R.read_outputs(str(tmp_path / "flt"), R.NAMES) == got
    else:
        assert ref["n_kept"] < len(kept_by_filter) or (cap == 50 and rate == 0.5)


@pytest.mark.parametrize("seed", [0, 926, -1])
def test_seeds_in_process(tmp_path, seed):
    texts, pool, wl = main_fixture()
    check_case(tmp_path, texts, wl, seed=seed, cap=5, rate=0.5, cli=False)


ODD = [b"ACGT\n", b"AC\n", b"ACGTNNNNACGTACGTACGT\n", b"acgtacgtacgtacgtacgt\n", None, b"\n", b"GGGG\n", None]


@functools.lru_cache(maxsize=None)
def odd_texts():
    """the main fixture with reads whose sequence line is short, holds N, lower case or a CR: the escape path"""
    texts, pool, wl = main_fixture()
    odd = list(ODD)
    odd[4], odd[7] = pool[1] + b"\r\n", pool[2][:10] + b"N" + b"A" * 20 + b"\n"
    r1 = R.records(texts["R1"])
    for k, s in enumerate(odd * 10):
        r1[k * 7 + 5][1] = s
    return dict(I1=texts["I1"], R1=b"".join(b"".join(r) for r in r1), R2=None), pool


@pytest.mark.parametrize("wl_kind", sorted(WHITELISTS))
@pytest.mark.parametrize("len_cb", [0, 12, 16, 31, 32, 40])
def test_whitelist_forms_and_lengths_in_process(tmp_path, wl_kind, len_cb):
    texts, pool = odd_texts()
    wl = WHITELISTS[wl_kind](pool) + (b"" if wl_kind == "empty" else b"\n" + Q.ESC_CELL + b"\n")
    got, ref, _, _ = check_case(tmp_path, texts, wl, len_cb=len_cb, cap=5, rate=0.9, fmts={"I1": "gzip"}, cli=False)
    if len_cb == 16 and wl_kind in ("tenx", "barcodes_tsv", "odd"):
        assert 0 < ref["n_kept"] < ref["n_matched"] and any(not set(c) <= set(b"ACGT") for c in ref["h"])


@pytest.mark.parametrize("kind", ["duplicates", "shared_prefixes"])
def test_duplicate_and_prefix_sharing_lines_make_no_extra_cells(tmp_path, kind):
    texts, pool, wl = main_fixture()
    w = Q.prefix_whitelists(pool)[kind]
    got, ref, _, _ = check_case(tmp_path, texts, w, len_cb=12, cap=5, cli=False)
    plain = b"".join(c + b"\n" for c in sorted(ref["h"]))
    assert Q.py_fqcap(texts, plain, 12, 926, None, 5)["tsv"] == ref["tsv"]
    assert len(ref["h"]) == len(set(ref["h"])) == ref["tsv"].count(b"\n") - 1


def test_framings_give_the_same_bytes(tmp_path):
    texts, pool, wl = main_fixture()
    first = None
    for fmt in ("plain", "bgzf", "gzip", "members"):
        d = tmp_path / fmt
        d.mkdir()
        got, _, _, _ = check_case(d, texts, wl, cap=5, fmts={n: fmt for n in R.NAMES}, cli=False)
        first = first or got
        assert got == first, fmt


@pytest.mark.parametrize("window", [4096, 4099, 6151, 65537])
def test_odd_windows_cli(tmp_path, window):
    texts, pool, wl = main_fixture()
    rng = np.random.default_rng(window)
    texts = dict(texts)
    for n in R.NAMES:                                           # uneven record lengths: records straddle window ends at every offset
        rs = R.records(texts[n])
        for r in rs:
            r[0] = b"@" + b"x" * int(rng.integers(1, 300)) + b"\n"
        texts[n] = b"".join(b"".join(r) for r in rs)
    check_case(tmp_path, texts, wl, cap=5, rate=0.6, fmts={"I1": "bgzf", "R2": "gzip"}, env={"FASTF_FQ_WINDOW": str(window)})


@pytest.mark.parametrize("i1_n,r2_n", [(1000, 3500), (2500, 1200)])
def test_mates_shorter_and_longer(tmp_path, i1_n, r2_n):
    texts, pool, wl = main_fixture()
    big, _ = R.tenx_triple(3500, seed=7)
    cut = lambda t, n: b"".join(b"".join(r) for r in R.records(t)[:n])  # noqa: E731
    texts = dict(texts, I1=cut(big["I1"], i1_n), R2=cut(big["R2"], r2_n)[:-1])       # (R2's last line without its newline)
    check_case(tmp_path, texts, wl, cap=5, fmts={"I1": "gzip", "R2": "members"}, cli=False)


def test_r1_only_and_last_line_open(tmp_path):
    texts, pool, wl = main_fixture()
    check_case(tmp_path, dict(I1=None, R1=texts["R1"][:-1], R2=None), wl, cap=5)


def test_python_api_equals_cli(tmp_path):
    texts, pool, wl = main_fixture()
    a = tmp_path / "a"
    b = tmp_path / "b"
    a.mkdir()
    b.mkdir()
    g1, _, _, _ = check_case(a, texts, wl, cap=5, rate=0.5, seed=77, fmts={n: "gzip" for n in R.NAMES}, cli=True)
    g2, _, _, _ = check_case(b, texts, wl, cap=5, rate=0.5, seed=77, fmts={n: "gzip" for n in R.NAMES}, cli=False)
    assert g1 == g2 and Q.read_tsv(a / "out") == Q.read_tsv(b / "out")


def test_refusals_that_need_the_device(tmp_path):
    texts, pool, wl = main_fixture()
    wlp = write(tmp_path, "wl.txt", wl)
    good = write(tmp_path, "good.fq", texts["R1"])
    head = b"".join(b"".join(r) for r in R.records(texts["R1"])[:100])
    cases = {
        "long_line": texts["R1"].replace(R.records(texts["R1"])[57][3], b"F" * 1100 + b"\n", 1),
        "truncated": head + b"@extra\nACGT\n",
    }
    for name, data in cases.items():
        for fmt in ("plain", "gzip"):
            bad = write(tmp_path, "%s.%s" % (name, fmt), R.encode(data, fmt))
            out = tmp_path / ("o_%s_%s" % (name, fmt))
            p = run_cli("fqcap", {"R1": bad, "R2": good}, out, wlp, ["-n", 5])
            assert p.returncode == 1 and os.path.basename(bad) in p.stderr and "read " in p.stderr, p.stderr
            assert os.listdir(out) == []
            # the same fault in a mate shows only after R1 was written: refused by name, and nothing is left behind
            out2 = tmp_path / ("m_%s_%s" % (name, fmt))
            p = run_cli("fqcap", {"R1": good, "R2": bad}, out2, wlp, ["-n", 5])
            assert p.returncode == 1 and os.path.basename(bad) in p.stderr, p.stderr
            assert os.listdir(out2) == []
    corrupt = bytearray(R.encode(texts["R1"], "gzip"))
    corrupt[len(corrupt) // 2] ^= 0xff
    out = tmp_path / "o_c"
    p = run_cli("fqcap", {"R1": write(tmp_path, "corrupt.gz", bytes(corrupt))}, out, wlp, ["-n", 5])
    assert p.returncode == 1 and "corrupt.gz" in p.stderr and os.listdir(out) == []
