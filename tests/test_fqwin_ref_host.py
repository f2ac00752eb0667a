"""tests/fqwin_ref.py, the definition the device parse of freq is held to in tests/test_gpu_freq_windows.py, checked on the CPU:
its per-read keys and escape strings against fastq_kernels.hpp's own per-lane functions compiled for the host
(build/libfq_host.so, themselves checked against the reference's get_fastq + substring in test_freq_host.py); its per-read result
the same however the text is cut into windows; and every wrong rule of fqwin_ref.DEFECTS changing the expected output of some
fixture, so that the device test would fail for a device with that bug."""
import ctypes as C
import os

import numpy as np
import pytest

import fqwin_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FQ_HOST = os.path.join(ROOT, "build", "libfq_host.so")


@pytest.fixture(scope="module")
def fq():
    L = C.CDLL(FQ_HOST)
    L.fq_host_key.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_char_p, C.POINTER(C.c_int)]
    L.fq_host_key.restype = C.c_int
    L.fq_host_pack.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32]
    L.fq_host_pack.restype = C.c_uint64
    return L


def texts():
    """(fixture, text as a contiguous array) once per distinct (text, L)"""
    seen, out = set(), []
    for f in Q.fixtures():
        if (id(f.text), f.L) not in seen:
            seen.add((id(f.text), f.L))
            out.append((f, np.ascontiguousarray(Q.as_u8(f.text))))
    return out


def test_per_read_keys_and_escape_strings_match_the_host_build_of_the_kernels_functions(fq):
    out, dna = C.create_string_buffer(2048), C.c_int()
    n_dna = n_esc = 0
    for f, t in texts():
        base, n = t.ctypes.data, len(t)
        L = min(f.L, Q.FQ_HDR)
        per_read = Q.reads(t, f.L)
        assert len(per_read) == Q.n_reads(t), f
        for r, (s, key) in enumerate(per_read):
            want, is_dna = Q.key_string(t, s, f.L)
            k = fq.fq_host_key(base + s, n - s, f.L, out, C.byref(dna))
            assert (out.raw[:k], bool(dna.value)) == (want, is_dna) and is_dna == bool(key), (f, r, s)
            if L <= Q.MAX_DNA:
                # the packer at the line's own misalignment, as the device's nine aligned words give it
                assert fq.fq_host_pack(base + s, n - s, s & 3, L) == key, (f, r, s)
            if key:
                assert key >> 63 == 1 and len(want) == L
                n_dna += 1
            else:
                assert len(want) == Q.escape_len(t, s, n, L) <= min(L, Q.MAX_LINE)
                n_esc += 1
    assert n_dna > 1000 and n_esc > 1000


def merged(wins):
    keys, esc = {}, []
    for w in wins:
        assert not set(keys) & set(w["keys"])
        keys.update(w["keys"])
        esc += w["esc"]
    return keys, sorted(esc)


def cuts_for(f):
    n = len(f.text)
    if f.group == "big":
        return [f.lens, [4 << 20, 4 << 20, n - (8 << 20)]]
    m = n // 1500
    # (a window that is not the last holds at least 1024 bytes, so that it can resolve what it is handed; the first may be short)
    out = [f.lens, [n], [n, 0], [n // 3, n - n // 3], [1500] * m + [n - 1500 * m], [n - 1500 * m] + [1500] * m + [0]]
    if n > 7:
        k = (n - 7) // 1024
        out.append([7] + [1024] * k + [n - 7 - 1024 * k])
    return out


def test_per_read_result_is_the_same_for_every_cut_into_windows():
    for f in Q.fixtures():
        per_read = Q.reads(f.text, f.L)
        want_keys = {r: k for r, (s, k) in enumerate(per_read) if k}
        want_esc = sorted((s, r) for r, (s, k) in enumerate(per_read) if not k)
        ends = set()
        for lens in cuts_for(f):
            wins, end = Q.run(f.text, lens, f.L)
            assert merged(wins) == (want_keys, want_esc), (f, lens[:4])
            assert all(w["n_nl"] == int((Q.as_u8(f.text)[:w["a"] + w["len"]] == 10).sum()) for w in wins)
            ends.add(tuple(sorted(end.items())))
        assert len(ends) == 1, f


def observable(exp):
    wins, end = exp
    return [(w["keys"], w["esc"], w["n_nl"], w["err"]) for w in wins], end


def test_each_wrong_rule_changes_some_fixture():
    fxs = Q.fixtures()
    good = {repr(f): observable(f.expected()) for f in fxs}
    for defect in Q.DEFECTS:
        caught = [repr(f) for f in fxs if observable(f.expected(defect)) != good[repr(f)]]
        assert caught, "no fixture notices the defect %s" % defect
        print("%s: caught by %d fixtures, first %s" % (defect, len(caught), "; ".join(caught[:3])))


def test_the_fixtures_take_the_branches_they_are_named_for():
    g = {name: [(f, f.expected()) for f in Q.group(name)] for name in ("dna_sweep", "esc_sweep", "max_pend", "zero_last", "many_windows",
                                                                        "key_kinds", "long_lines", "big")}
    # DNA sweep: handed on exactly when the cut lies inside the L bytes (or right in front of them), at every alignment
    handed = [(f, wins[0]["pend"]) for f, (wins, _) in g["dna_sweep"] if "cut=s" in f.name]
    assert len(handed) == 4 * 31 and sum(1 for _, p in handed if p) == 4 * 26
    assert {p[0][0] & 3 for _, p in handed if p} == {0, 1, 2, 3}
    assert any(p and p[0][0] == f.lens[0] for f, p in handed)                    # a line that starts at a + len
    # escape sweep: the line is handed on for cuts up to s + 1023 and then reported by the next window with s < a
    for f, (wins, _) in g["esc_sweep"]:
        d = int(f.name.split("cut=s")[1])
        assert (300, 2) in (wins[1]["esc"] if 0 <= d <= 1023 else wins[0]["esc"]) or d == -1, f
        if 0 <= d <= 1023:
            assert (300, 2) in wins[0]["pend"] and 300 <= wins[1]["a"] <= 300 + 1023
    assert any(wins[1]["a"] - 300 == 1023 for f, (wins, _) in g["esc_sweep"])     # as far back as the header reaches
    # the most lines one window hands on
    most = {L: max(len(wins[0]["pend"]) for f, (wins, _) in g["max_pend"] if f.L == L) for L in (40, 5)}
    assert most == {40: 256, 5: 2}, most
    for f, (wins, _) in g["max_pend"]:
        taken = [e for e in wins[1]["esc"] if e[0] <= wins[1]["a"]] + [(s, r) for s, r in wins[0]["pend"] if r in wins[1]["keys"]]
        assert sorted(taken) == sorted(wins[0]["pend"]) and len(wins) == 4           # (the empty lines of the tail: escapes)
    # an empty last window resolves what it is handed, all of it as escapes
    for f, (wins, _) in g["zero_last"]:
        assert wins[1]["len"] == 0 and wins[0]["pend"] and wins[1]["esc"] == sorted(wins[0]["pend"]) and not wins[1]["keys"]
    for f, (wins, _) in g["many_windows"]:
        assert len(wins) >= 6 and all(w["esc"] for w in wins)
    errs = {f.name: end for f, (_, end) in g["long_lines"]}
    for which in range(4):
        assert errs["line %d of read 2 has 1023 bytes" % which] == dict(errs["line %d of read 2 has 1023 bytes" % which], err=0, err_rec=Q.NONE)
        assert (errs["line %d of read 2 has 1024 bytes, cut" % which]["err"], errs["line %d of read 2 has 1024 bytes" % which]["err_rec"]) == (1, 2)
    assert errs["window without newline"]["err"] == 1 and errs["one line over two boundaries"]["err"] == 1
    (f, (wins, end)), = g["big"]
    for w, nt in zip(wins, Q.BIG_TILES):
        tiles = {(s - w["a"]) // Q.TILE for s in Q.seq_starts(Q.as_u8(f.text)) if w["a"] <= s < w["a"] + w["len"]}
        assert {0, 1023, nt - 1} <= tiles and (nt <= 1024 or 1024 in tiles) and (nt <= 1025 or 1025 in tiles)
