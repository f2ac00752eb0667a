"""freq on the MI355X: whitelist.txt of `fastF freq` byte for byte against the reference's own cmd_freq -> cell_counts
-> insert_tree -> print_tree (oracle/_ref/fastF_refmain, main.c + filter.c + count.c compiled in place), for every input
framing gzopen() reads, window boundaries at every offset, the refusals, the in-process drop-in cell_counts and the Python
binding.  Inputs compared with the reference are unsorted (its BST is unbalanced and recursive)."""
import ctypes as C
import gzip
import os
import random
import subprocess
import zlib

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFMAIN = os.path.join(ROOT, "oracle", "_ref", "fastF_refmain")
REF_TREE = os.path.join(ROOT, "oracle", "_ref", "libfastf_ref_tree.so")
OURS = _lib.cli_path()


def need_ref():
    if not os.path.exists(REFMAIN):
        pytest.skip("oracle/_ref/fastF_refmain not built")


def fastq_text(seqs, ids=None):
    out = []
    for i, s in enumerate(seqs):
        out.append(b"@%s\n%s\n+\n%s\n" % (ids[i] if ids else b"r%d" % i, s, b"I" * len(s.rstrip(b"\r"))))
    return b"".join(out)


def encode(text: bytes, fmt: str) -> bytes:
    if fmt == "plain":
        return text
    if fmt == "gzip":
        return gzip.compress(text, 6)
    if fmt == "members":
        k = len(text) // 3
        return b"".join(gzip.compress(p, 1) for p in (text[:k], text[k:2 * k], text[2 * k:]))
    if fmt == "bgzf":
        out = [synth._bgzf_block(text[o:o + 0xff00]) for o in range(0, len(text), 0xff00)]
        return b"".join(out) + synth._bgzf_block(b"")
    raise ValueError(fmt)


def run(binary, path, outdir, args=(), env=None):
    os.makedirs(outdir, exist_ok=True)
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([binary, "freq", "-R", str(path), "-o", str(outdir)] + list(args), capture_output=True, text=True,
                       env=e, timeout=900)
    wl = os.path.join(outdir, "whitelist.txt")
    return p, (open(wl, "rb").read() if os.path.exists(wl) else None)


def assert_same(tmp_path, path, args=(), env=None, tag="x"):
    need_ref()
    po, ours = run(OURS, path, tmp_path / ("o_" + tag), args, env)
    assert po.returncode == 0, po.stderr
    pr, ref = run(REFMAIN, path, tmp_path / ("r_" + tag), args)
    assert pr.returncode == 0, pr.stderr
    assert ours == ref
    return ours


def rand_seqs(rng, n, L, n_distinct=None, alphabet=b"ACGT", length_jitter=0):
    pool = None
    if n_distinct:
        pool = [bytes(rng.choice(alphabet) for _ in range(L)) for _ in range(n_distinct)]
    out = []
    for _ in range(n):
        s = rng.choice(pool) if pool else bytes(rng.choice(alphabet) for _ in range(L))
        if length_jitter:
            s = s[:max(0, L + rng.randrange(-length_jitter, length_jitter + 1))]
        out.append(s + b"TTTTTTTTTT")
    return out


def tenx_text(n, seed, n_bc=3000, umi_pool=200_000, umi_len=12, p_random=0.05, tail=45):
    """10x-shaped R1 reads: a few thousand barcodes, Zipf-distributed UMIs, 5 % random barcodes, ~115 bytes per read"""
    g = np.random.default_rng(seed)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    bcs = lut[g.integers(0, 4, size=(n_bc, 16))]
    umis = lut[g.integers(0, 4, size=(umi_pool, umi_len))]
    bc = bcs[g.integers(0, n_bc, size=n)]
    rnd = g.random(n) < p_random
    bc[rnd] = lut[g.integers(0, 4, size=(int(rnd.sum()), 16))]
    z = np.minimum(g.zipf(1.3, size=n), umi_pool) - 1
    umi = umis[g.permutation(umi_pool)[z]]
    rest = lut[g.integers(0, 4, size=(n, tail - 16 - umi_len))]
    rest[g.random(n) < 0.01, 0] = ord("N")
    seq = np.concatenate([bc, umi, rest], axis=1)
    nl = np.full((n, 1), ord("\n"), dtype=np.uint8)
    hdr = np.frombuffer(b"@A00:1:HXX:1:1101:10\n", dtype=np.uint8)
    rec = np.concatenate([np.broadcast_to(hdr, (n, len(hdr))), seq, nl, np.broadcast_to(np.frombuffer(b"+\n", dtype=np.uint8), (n, 2)),
                          np.full((n, tail), ord("F"), dtype=np.uint8), nl], axis=1)
    return rec.tobytes()


@pytest.fixture(scope="module")
def mixed_text():
    rng = random.Random(11)
    seqs = rand_seqs(rng, 3000, 26, n_distinct=400)
    seqs += [b"ACGTNACGTACGTACGTACGTACGTA" + b"TT", b"acgtacgtacgtacgtacgtacgtac", b"ACGT", b"", b"ACGTACGT\x00ACGTACGTACGTACGTACGT",
             b"ACGTACGTACGTACGTACGTACGTAC\r", b"\x01\x02weird bytes , with comma"]
    seqs += rand_seqs(rng, 2000, 28, alphabet=b"ACGTN", length_jitter=4)
    rng.shuffle(seqs)
    return fastq_text(seqs)


@pytest.mark.parametrize("fmt", ["plain", "gzip", "members", "bgzf"])
def test_framings_match_reference(tmp_path, mixed_text, fmt):
    p = tmp_path / ("in." + fmt)
    p.write_bytes(encode(mixed_text, fmt))
    assert_same(tmp_path, p)


@pytest.mark.parametrize("lu", [("16", "10"), ("16", "12"), ("0", "0"), ("20", "11"), ("20", "12"), ("1000", "40"), ("-3", "5")])
def test_lengths_match_reference(tmp_path, mixed_text, lu):
    p = tmp_path / "in.fq"
    p.write_bytes(mixed_text)
    assert_same(tmp_path, p, ["-l", lu[0], "-u", lu[1]])


def test_crlf_short_reads_and_a_last_record_without_qual(tmp_path):
    rng = random.Random(3)
    seqs = rand_seqs(rng, 500, 26, n_distinct=50, length_jitter=6)
    text = b"".join(b"@r%d\r\n%s\r\n+\r\nIII\r\n" % (i, s) for i, s in enumerate(seqs))
    for tail in (b"@last\nACGTACGTACGTACGTACGTACGTAC\n", b"@last\nACGTACGTACGTACGTACGTACGTAC", b"@last\nACGT\n+\n", b"@last\nACG"):
        p = tmp_path / "in.fq"
        p.write_bytes(text + tail)
        assert_same(tmp_path, p, tag=str(len(tail)))


def test_empty_file(tmp_path):
    p = tmp_path / "empty.fq"
    p.write_bytes(b"")
    assert assert_same(tmp_path, p) == b""
    g = tmp_path / "empty.fq.gz"
    g.write_bytes(gzip.compress(b""))
    assert assert_same(tmp_path, g, tag="gz") == b""


@pytest.mark.parametrize("window", ["4096", "4097", "5003", "8191", "70001"])
def test_window_boundaries(tmp_path, window):
    rng = random.Random(int(window))
    seqs = rand_seqs(rng, 4000, 26, n_distinct=300, length_jitter=3)
    seqs += rand_seqs(rng, 1000, 28, alphabet=b"ACGTN")
    rng.shuffle(seqs)
    text = fastq_text(seqs, ids=[b"id%d" % (i * 7919 % 100003) + b"x" * (i % 37) for i in range(len(seqs))])
    for fmt in ("plain", "bgzf"):
        p = tmp_path / ("w." + fmt)
        p.write_bytes(encode(text, fmt))
        base = assert_same(tmp_path, p, tag=fmt)
        for lu in (("16", "10"), ("16", "20")):
            _, ours = run(OURS, p, tmp_path / ("win" + fmt + lu[1]), ["-l", lu[0], "-u", lu[1]], {"FASTF_FQ_WINDOW": window})
            _, ref = run(REFMAIN, p, tmp_path / ("winr" + fmt + lu[1]), ["-l", lu[0], "-u", lu[1]])
            assert ours == ref, (fmt, lu)
        _, ours = run(OURS, p, tmp_path / ("wd" + fmt), [], {"FASTF_FQ_WINDOW": window})
        assert ours == base


def test_tenx_2m_reads(tmp_path):
    text = tenx_text(2_000_000, seed=7)
    for fmt in ("bgzf", "plain"):
        p = tmp_path / ("tenx." + fmt)
        p.write_bytes(encode(text, fmt))
        out = assert_same(tmp_path, p, tag=fmt)
        assert sum(int(ln.rpartition(b",")[2]) for ln in out.split(b"\n")[:-1]) == 2_000_000


def test_large_file_same_bytes_in_every_framing(tmp_path):
    n = 8_000_000
    text = tenx_text(n, seed=9)
    outs = []
    for fmt in ("plain", "members", "bgzf"):
        p = tmp_path / ("big." + fmt)
        p.write_bytes(encode(text, fmt))
        pr, out = run(OURS, p, tmp_path / ("big_" + fmt))
        assert pr.returncode == 0, pr.stderr
        outs.append(out)
        p.unlink()
    assert outs[0] == outs[1] == outs[2]
    assert sum(int(ln.rpartition(b",")[2]) for ln in outs[0].split(b"\n")[:-1]) == n


def test_refusals(tmp_path):
    ok = fastq_text([b"ACGTACGTACGTACGTACGTACGTAC"] * 10)
    cases = {
        "long_line": (ok + b"@long\n" + b"A" * 1023 + b"\n+\nI\n", "longer than 1023 bytes"),
        "long_last_line": (ok + b"@long\nACGT\n+\n" + b"I" * 1024, "longer than 1023 bytes"),
        "ends_after_id": (ok + b"@last\n", "ends after the header line"),
        "ends_after_id_no_nl": (ok + b"@last", "ends after the header line"),
        "corrupt_gzip": (gzip.compress(ok)[:-12] + b"\x00" * 12, "gzip"),
    }
    for name, (data, msg) in cases.items():
        p = tmp_path / (name + ".fq")
        p.write_bytes(data)
        pr, out = run(OURS, p, tmp_path / ("o" + name))
        assert pr.returncode == 1, (name, pr.stderr)
        assert msg in pr.stderr, (name, pr.stderr)
        assert out is None
    # the longest line gzgets takes whole (1022 bytes + newline) is fine
    p = tmp_path / "edge.fq"
    p.write_bytes(ok + b"@e\n" + b"C" * 1022 + b"\n+\nI\n")
    assert_same(tmp_path, p, tag="edge")


def test_cell_counts_in_process_prints_like_the_reference(tmp_path):
    need_ref()
    if not os.path.exists(REF_TREE):
        pytest.skip("oracle/_ref/libfastf_ref_tree.so not built")
    rng = random.Random(21)
    p = tmp_path / "cc.fq.gz"
    p.write_bytes(encode(fastq_text(rand_seqs(rng, 20000, 26, n_distinct=2000, length_jitter=1)), "bgzf"))
    _, ref = run(REFMAIN, p, tmp_path / "ref")
    L = C.CDLL(_lib.lib_path())
    T = C.CDLL(REF_TREE)
    z = C.CDLL("libz.so.1")
    libc = C.CDLL(None)
    z.gzopen.argtypes = [C.c_char_p, C.c_char_p]; z.gzopen.restype = C.c_void_p
    z.gzclose.argtypes = [C.c_void_p]
    L.cell_counts.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t]; L.cell_counts.restype = C.c_void_p
    T.print_tree.argtypes = [C.c_void_p, C.c_void_p]
    T.free_tree_node.argtypes = [C.c_void_p]
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]; libc.fopen.restype = C.c_void_p
    libc.fclose.argtypes = [C.c_void_p]
    g = z.gzopen(str(p).encode(), b"r")
    root = L.cell_counts(g, 16, 10)
    z.gzclose(g)
    out = tmp_path / "cc.txt"
    f = libc.fopen(str(out).encode(), b"w")
    T.print_tree(root, f)
    libc.fclose(f)
    T.free_tree_node(root)
    assert out.read_bytes() == ref
    assert L.fastf_debug_live_registrations() == 0


def test_python_binding_matches_the_cli(tmp_path, mixed_text):
    p = tmp_path / "py.fq.gz"
    p.write_bytes(encode(mixed_text, "gzip"))
    pr, cli = run(OURS, p, tmp_path / "cli", ["-l", "16", "-u", "12"])
    assert pr.returncode == 0, pr.stderr
    assert F.freq_text(str(p), 16, 12) == cli
    rows = F.freq(str(p), 16, 12)
    assert sum(c for _, c in rows) == mixed_text.count(b"\n") // 4
    assert _lib.lib().fastf_debug_live_registrations() == 0
