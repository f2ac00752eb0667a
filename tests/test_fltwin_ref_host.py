"""tests/fltwin_ref.py (the expectations of tests/test_gpu_filter_windows.py) against what the project already trusts, without a GPU:
its concatenated window output against filter_ref.py_filter on the 10x-shaped inputs with odd sequence lines of
test_gpu_filter.py::test_whitelist_forms_and_lengths, fed the host's draw stream through `draws=`; its chunk twin against
F.filter_draws(device=False).

The chunk twin: BOTH checks the issue names were done.  The stream's true 31-word states are reachable from Python — glibc's
TYPE_3 seeding is public (r_0 = seed, r_i = 16807 r_{i-1} mod 2^31 - 1 by Schrage's split, r_31..33 = r_0..2, then
r_i = r_{i-3} + r_{i-31}; output k is r_{k+344} >> 1) — so the twin is seeded with the words r_{first+344 .. first+374} and must
equal filter_draws(926, first, n, device=False); and it is compared with the bare recurrence over 10 000 steps from random words."""
import numpy as np
import pytest

import fastf_amd as F

import filter_ref as R
import fltwin_ref as W


def glibc_words(seed, n):
    """r_0 .. r_{n-1} of glibc's TYPE_3 generator after srand(seed)"""
    r = np.zeros(n, dtype=np.uint64)
    x = seed or 1
    r[0] = x
    for i in range(1, 31):
        hi, lo = divmod(x, 127773)
        x = 16807 * lo - 2836 * hi
        if x < 0:
            x += 2147483647
        r[i] = x
    r[31:34] = r[0:3]
    for i in range(34, n):
        r[i] = (r[i - 3] + r[i - 31]) & 0xFFFFFFFF
    return r.astype(np.uint32)


def true_states(words, first, n):
    nch = (n + W.CHUNK - 1) // W.CHUNK
    return np.stack([words[first + 344 + c * W.CHUNK:first + 344 + c * W.CHUNK + 31] for c in range(nch)])


@pytest.mark.parametrize("first,n", [(0, 100_000), (4097, 5000), (4097, 2048), (0, 2049), (0, 1)])
def test_chunk_twin_equals_host_stream(first, n):
    words = glibc_words(926, first + n + 344 + 31 + W.CHUNK)
    got = W.chunk_draws(true_states(words, first, n), n)
    assert np.array_equal(got, F.filter_draws(926, first, n, device=False))


def test_chunk_twin_equals_bare_recurrence():
    rng = np.random.default_rng(1)
    n = 10_000
    r = np.zeros(n + 31, dtype=np.uint64)
    r[:31] = rng.integers(0, 1 << 32, size=31, dtype=np.uint64)
    for i in range(31, n + 31):
        r[i] = (r[i - 3] + r[i - 31]) & 0xFFFFFFFF
    states = np.stack([r[c * W.CHUNK:c * W.CHUNK + 31] for c in range((n + W.CHUNK - 1) // W.CHUNK)]).astype(np.uint32)
    assert np.array_equal(W.chunk_draws(states, n), (r[:n] >> 1).astype(np.uint32))


def test_vector_keep_rule_equals_scalar():
    rng = np.random.default_rng(2)
    d = np.concatenate([np.array([0, 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 2, 2 ** 30, 2 ** 31 - 65, 2 ** 31 - 64, 2 ** 31 - 1], dtype=np.uint32),
                        rng.integers(0, 1 << 31, size=2000, dtype=np.uint32)])
    for rate in (0.0, 0.5, 1.0, 2.0, float(np.float32(2 ** 24 + 1) / np.float32(2 ** 31)), 0.3):
        assert np.array_equal(W.passes(d, rate), np.array([R.draw_passes(int(x), rate) for x in d])), rate


def test_dna_key_form():
    assert W.dna_key(b"", 0) == W.DNA_TAG and W.dna_key(b"NNN", 0) == W.DNA_TAG
    assert W.dna_key(b"ACGT", 4) == W.DNA_TAG | 0b00011011
    assert W.dna_key(b"ACGTA", 4) == W.dna_key(b"ACGT", 4)
    assert W.dna_key(b"ACG", 4) == 0 and W.dna_key(b"ACGN", 4) == 0 and W.dna_key(b"acgt", 4) == 0 and W.dna_key(b"ACG\r", 4) == 0
    assert W.dna_key(b"T" * 31, 31) == W.DNA_TAG | ((1 << 62) - 1) and W.dna_key(b"T" * 40, 32) == 0
    keys = [W.dna_key(s, 3) for s in (b"AAA", b"AAC", b"ACA", b"CAA", b"GTT", b"TTT")]
    assert keys == sorted(keys)                               # key order is string order


def test_framing_of_small_texts():
    fr = W.Framing(b"")
    assert fr.n_nl == 0 and fr.n_reads == 0 and fr.tv is None and fr.windows([0]) == [(0, 0, W.NONE, 0, 0)]
    fr = W.Framing(b"@a\nAC\n+\nII")
    assert fr.tv == 10 and fr.n_nl == 4 and fr.n_reads == 1 and fr.out(0) == b"@a\nAC\n+\nII"
    assert list(fr.line_bytes) == [3, 3, 2, 2]
    assert fr.windows([4, 6]) == [(0, 4, W.NONE, 0, 0), (4, 7, 10, 0, 1)]
    assert fr.windows([10, 0]) == [(0, 10, W.NONE, 0, 0), (10, 1, 10, 0, 1)]
    fr = W.Framing(b"@a\nAC\n+\nII\n@b\n")
    assert fr.tv is None and fr.n_nl == 5 and fr.n_reads == 1 and fr.out(0) == b"@a\nAC\n+\nII\n"
    assert fr.windows([11, 3]) == [(0, 11, W.NONE, 0, 1), (11, 3, W.NONE, 1, 0)]
    # 1023 bytes with the newline pass, 1024 do not; an unterminated 1023 pass, 1024 do not
    for body, term, bad in ((1022, True, False), (1023, True, True), (1023, False, False), (1024, False, True)):
        fr = W.Framing(b"@a\nAC\n+\nII\n@b\nA\n+\n" + b"I" * body + (b"\n" if term else b""))
        assert fr.first_long() == ((1, 1) if bad else (0, W.NONE)), (body, term)
        assert fr.first_long(limit=1) == (0, W.NONE)


def odd_triple(len_cb):
    """the inputs of test_gpu_filter.py::test_whitelist_forms_and_lengths"""
    texts, pool = R.tenx_triple(1500, seed=len_cb + 11, n_cells=40, p_other=0.3)
    odd = [b"ACGT\n", b"AC\n", b"ACGTNNNNACGTACGTACGT\n", b"acgtacgtacgtacgtacgt\n", pool[1] + b"\r\n", b"\n", b"GGGG\n",
           pool[2][:10] + b"N" + b"A" * 20 + b"\n"]
    r1 = R.records(texts["R1"])
    for k, s in enumerate(odd * 10):
        r1[k * 7 + 3][1] = s
    texts["R1"] = b"".join(b"".join(r) for r in r1)
    return texts, pool


def split_whitelist(wl_bytes, L):
    """(DNA-form keys, every prefix as py_filter keeps it) of a whitelist file"""
    strings = {R.c_str(ln)[:L] for ln in R.lines(wl_bytes)}
    keys = {W.dna_key(s, L) for s in strings if len(s) == L and W.dna_key(s, L)}
    return keys, strings


def both_files(texts, lens_of, wl_bytes, L, seed, rate, all_cells):
    """R1 through mode 0 and I1 through mode 1 of the reference -> {"R1", "I1"} concatenated outputs, reads kept"""
    f1 = W.Framing(texts["R1"])
    draws = F.filter_draws(seed, 0, f1.n_reads, device=False)
    keys, strings = split_whitelist(wl_bytes, L) if wl_bytes is not None else (set(), set())
    judge = lambda r, line: R.c_str(line)[:L] in strings  # noqa: E731
    w1, end1, keep = W.run(f1, lens_of(len(texts["R1"])), 0, all_cells, L, rate, draws, keys, judge)
    assert end1["kept"] == int(keep.sum()) == w1[-1]["kept"] and end1["n_nl"] == f1.n_nl and end1["err"] == 0
    assert sum(w["n_rec"] for w in w1) == f1.n_reads
    res = {"R1": b"".join(w["out"] for w in w1)}
    if texts.get("I1") is not None:
        f0 = W.Framing(texts["I1"])
        w0, end0, _ = W.run(f0, lens_of(len(texts["I1"])), 1, bitmap=keep, limit=f1.n_reads)
        assert end0["kept"] == 0
        res["I1"] = b"".join(w["out"] for w in w0)
    return res


def one_window(n):
    return [n]


def windows_of(w):
    return lambda n: [w] * (n // w) + [n % w]                 # (a last window of 0 bytes where w divides n)


WL = {
    "tenx": lambda pool: b"".join(b + b"\n" for b in pool[::2]),
    "odd": lambda pool: (pool[0] + b"\n" + b"ACGTNACGTACGTACG\n" + b"\n" + b"AC\n" + pool[1] + b"\r\n" + b"GGGG\n" + pool[2][:10] + b"N\n" + pool[3]),
}


@pytest.mark.parametrize("wl_kind", sorted(WL))
@pytest.mark.parametrize("len_cb", [0, 12, 16, 31, 32])
def test_whitelist_lengths_equal_py_filter(wl_kind, len_cb):
    texts, pool = odd_triple(len_cb)
    wl = WL[wl_kind](pool)
    want = R.py_filter({"I1": texts["I1"], "R1": texts["R1"], "R2": None}, wl, len_cb, 926, 0.9, False)
    for lens_of in (one_window, windows_of(4099)):
        got = both_files(texts, lens_of, wl, len_cb, 926, 0.9, False)
        assert got["R1"] == want["R1"] and got["I1"] == want["I1"]
    if len_cb == 32:                                          # every read whose draw passes is an escape
        f1 = W.Framing(texts["R1"])
        draws = F.filter_draws(926, 0, f1.n_reads, device=False)
        w1, _, _ = W.run(f1, [len(texts["R1"])], 0, False, 32, 0.9, draws, (), None)
        assert len(w1[0]["esc"]) == int(W.passes(draws, 0.9).sum()) > 1000


@pytest.mark.parametrize("rate", [0.0, 0.5, 1.0, 2.0])
@pytest.mark.parametrize("all_cells", [False, True])
def test_rates_and_all_cells_equal_py_filter(rate, all_cells):
    texts, pool = odd_triple(16)
    wl = WL["tenx"](pool)
    want = R.py_filter({"I1": texts["I1"], "R1": texts["R1"], "R2": None}, wl, 16, 77, rate, all_cells)
    got = both_files(texts, windows_of(6151), wl, 16, 77, rate, all_cells)
    assert got["R1"] == want["R1"] and got["I1"] == want["I1"]
    n = len(R.records(want["R1"]))
    assert (n == 0) == (rate == 0.0) and (rate < 2.0 or not all_cells or n == 1500)


@pytest.mark.parametrize("lens_of,k", [(one_window, 1500), (windows_of(4096), 1500), (windows_of(1), 60)], ids=["one", "4096", "1"])
def test_unterminated_last_line_equals_py_filter(lens_of, k):
    texts, pool = odd_triple(16)
    cut = lambda t, k: b"".join(b"".join(r) for r in R.records(t)[:k])[:-1]  # noqa: E731
    texts = {"R1": cut(texts["R1"], k), "I1": cut(texts["I1"], k)}
    wl = WL["tenx"](pool)
    for all_cells, rate in ((True, 1.0), (False, 2.0)):
        want = R.py_filter({"I1": texts["I1"], "R1": texts["R1"], "R2": None}, wl, 16, 926, rate, all_cells)
        got = both_files(texts, lens_of, wl, 16, 926, rate, all_cells)
        assert got["R1"] == want["R1"] and got["I1"] == want["I1"]
        assert not got["R1"].endswith(b"\n") or not all_cells
