"""freq on the CPU: the per-lane line -> key / escape functions of fastq_kernels.hpp (compiled for the host as
build/libfq_host.so) against the reference's own get_fastq + substring (filter.c:15-37, 260-275), the command line of
`fastF freq` against the reference's main.c + argparse.c, and the symbols the library exports for it."""
import ctypes as C
import os
import random
import subprocess

import pytest

from fastf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FQ_HOST = os.path.join(ROOT, "build", "libfq_host.so")
REF_TREE = os.path.join(ROOT, "oracle", "_ref", "libfastf_ref_tree.so")
REFMAIN = os.path.join(ROOT, "oracle", "_ref", "fastF_refmain")
OURS = os.path.join(ROOT, "fastf_amd", "bin", "fastF")


@pytest.fixture(scope="module")
def fq():
    L = C.CDLL(FQ_HOST)
    L.fq_host_key.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_char_p, C.POINTER(C.c_int)]
    L.fq_host_key.restype = C.c_int
    L.fq_host_pack.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32]
    L.fq_host_pack.restype = C.c_uint64
    return L


def host_key(fq, tail: bytes, L: int):
    out = C.create_string_buffer(2048)
    dna = C.c_int()
    n = fq.fq_host_key(tail, len(tail), L, out, C.byref(dna))
    return out.raw[:n], bool(dna.value)


class Fastq(C.Structure):
    _fields_ = [("id", C.c_void_p), ("seq", C.c_void_p), ("qual", C.c_void_p)]


@pytest.fixture(scope="module")
def ref():
    if not os.path.exists(REF_TREE):
        pytest.skip("oracle/_ref/libfastf_ref_tree.so not built (reference sources absent)")
    L = C.CDLL(REF_TREE)
    z = C.CDLL("libz.so.1")
    z.gzopen.argtypes = [C.c_char_p, C.c_char_p]
    z.gzopen.restype = C.c_void_p
    z.gzclose.argtypes = [C.c_void_p]
    L.get_fastq.argtypes = [C.c_void_p]
    L.get_fastq.restype = C.POINTER(Fastq)
    L.substring.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.substring.restype = C.c_void_p
    L.free_fastq.argtypes = [C.POINTER(Fastq)]
    return L, z


def ref_key(ref, path, L):
    lib, z = ref
    g = z.gzopen(path.encode(), b"r")
    rec = lib.get_fastq(g)
    s = lib.substring(rec.contents.seq, 0, L)
    out = C.string_at(s)
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(s)
    lib.free_fastq(rec)
    z.gzclose(g)
    return out


def fuzz_seq(rng, L):
    kind = rng.randrange(8)
    n = max(0, L + rng.randrange(-3, 4)) if kind < 6 else rng.randrange(0, 40)
    alpha = b"ACGT" if kind < 3 else rng.choice([b"ACGTN", b"ACGTacgtN", b"ACGT\r", b"ACGT\x00", b"ACGT\x01~ ", bytes(range(1, 256))])
    s = bytes(rng.choice(alpha) for _ in range(min(n, 1000)))
    return s.replace(b"\n", b"A")


@pytest.mark.parametrize("L", [0, 1, 26, 28, 31, 32, 40, 1100])
def test_line_to_key_matches_reference_substring(fq, ref, tmp_path, L):
    rng = random.Random(L * 7919 + 1)
    path = str(tmp_path / "r.fq")
    for i in range(300):
        seq = fuzz_seq(rng, L)
        end = rng.randrange(6)
        if end == 0:
            rest = b""                                   # the file ends inside the sequence line (no newline)
        elif end == 1:
            rest = b"\n"                                 # ... right after it
        elif end == 2:
            rest = b"\r\n+\r\nIIII\r\n"
        else:
            rest = b"\n+\n" + b"I" * len(seq) + b"\n@next\nACGT\n+\nIIII\n"
        tail = seq + rest
        if not tail:
            tail = b"\n"                                # (a file that ends after the header line is refused: undefined here)
        with open(path, "wb") as f:
            f.write(b"@r%d\n" % i + tail)
        want = ref_key(ref, path, L)
        got, dna = host_key(fq, tail, L)
        assert got == want, (L, tail[:80])
        if dna:
            assert L <= 31 and len(got) == L and set(got) <= set(b"ACGT")


def test_dna_form_orders_like_strcmp_at_every_alignment(fq):
    rng = random.Random(5)
    for L in (1, 16, 26, 31):
        seqs = [bytes(rng.choice(b"ACGT") for _ in range(L)) for _ in range(200)]
        keys = {}
        for s in seqs:
            k = [fq.fq_host_pack(s + b"\n+\n", len(s) + 3, off, L) for off in range(4)]
            assert len(set(k)) == 1 and k[0] >> 63 == 1, s
            keys[s] = k[0]
        srt = sorted(set(seqs))
        assert [keys[s] for s in srt] == sorted(keys[s] for s in srt)
    # anything but exactly L bases of ACGT is an escape (0), whatever the alignment
    for bad in (b"ACGN", b"acgt", b"AC\nT", b"AC\x00T", b"AC"):
        for off in range(4):
            assert fq.fq_host_pack(bad, len(bad), off, 4) == 0, bad


BAD_ARGS = [
    [], ["-x"], ["--bogus=1"], ["-R"], ["-o"], ["-l"], ["-u"], ["--len"], ["-l", "abc", "-R", "{fq}"], ["-l", "1x"],
    ["--len=z"], ["-u", "99999999999999999999"], ["--umi=0x"], ["-R", "/nonexistent"], ["--R1=/nonexistent", "-o", "."],
    ["-R", "{fq}"], ["-R", "{fq}", "-o", "/nonexistent"], ["-R", "{fq}", "-o", "{fq}"], ["-l0x10", "-R", "/nonexistent"],
    ["--umi", "7", "--len=3", "-R", "/nonexistent"], ["stray", "-R", "/nonexistent"], ["-o", ".", "--", "-R", "{fq}"],
]


@pytest.mark.parametrize("args", BAD_ARGS, ids=[" ".join(a) or "-" for a in BAD_ARGS])
def test_cmd_freq_parsing_matches_the_reference_cli(tmp_path, args):
    """exit status and stderr of `fastF freq` for option errors (argparse.c:36-117, 221-287) and the checks of
    main.c:56-85 that come before any read is processed"""
    if not os.path.exists(REFMAIN):
        pytest.skip("oracle/_ref/fastF_refmain not built (reference sources absent)")
    fqp = tmp_path / "e.fq"
    fqp.write_bytes(b"")
    argv = [a.format(fq=fqp) for a in args]
    our = subprocess.run([OURS, "freq"] + argv, capture_output=True, text=True, cwd=tmp_path)
    ref = subprocess.run([REFMAIN, "freq"] + argv, capture_output=True, text=True, cwd=tmp_path)
    assert our.returncode == ref.returncode
    assert our.stderr == ref.stderr


def test_freq_help_and_dispatch():
    r = subprocess.run([OURS, "freq", "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "--R1" in r.stdout and "--umi" in r.stdout
    r = subprocess.run([OURS, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "freq" in r.stdout and "freq/filter are not part" not in r.stdout


def test_library_exports_freq_and_not_the_reference_tree_code():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for sym in ("fastf_freq_text", "cmd_freq", "cell_counts", "fastf_taghist_push_device", "fastf_taghist_reserve_device"):
        assert sym in names, sym
    # fastF_refmain links the reference's filter.o: the library must not interpose on any of its names
    for sym in ("print_tree", "insert_tree", "substring", "get_fastq", "free_fastq", "new_node", "construct_tree",
                "free_tree_node", "print_tree_gz", "get_comb_fastq", "flag"):
        assert sym not in names, sym
