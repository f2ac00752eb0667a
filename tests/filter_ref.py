"""Expectations for `fastF filter` (tests/test_filter_host.py, tests/test_gpu_filter.py).

ref_driver: the reference's own filter loop run sequentially — get_row / read_txt / construct_tree / get_comb_fastq / substring
/ in of oracle/_ref/libfastf_ref_tree.so (filter.c compiled in place) through ctypes, libc's srand seeded from this process.
fastF() itself is not called: its OpenMP tasks share one block pointer and crash.

py_filter: a plain-Python restatement of the same semantics that needs nothing built."""
import ctypes as C
import gzip
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_TREE = os.path.join(ROOT, "oracle", "_ref", "libfastf_ref_tree.so")
REFMAIN = os.path.join(ROOT, "oracle", "_ref", "fastF_refmain")
NAMES = ("I1", "R1", "R2")
_libc = C.CDLL("libc.so.6")
_libc.srand.argtypes = [C.c_uint]
_libc.rand.restype = C.c_int

_LINE = re.compile(rb"[^\n]*\n|[^\n]+\Z")


def lines(text: bytes):
    return _LINE.findall(text)


def records(text: bytes):
    ls = lines(text)
    return [ls[i:i + 4] for i in range(0, len(ls) - len(ls) % 4, 4)]


def c_str(b: bytes) -> bytes:
    """what a C string function sees of a gzgets / fgets buffer: up to the first NUL"""
    k = b.find(b"\0")
    return b if k < 0 else b[:k]


def draw_passes(r: int, rate: float) -> bool:
    return float(np.float32(r) / np.float32(2147483647)) < float(np.float32(rate))


def py_filter(texts, whitelist=None, len_cb=16, seed=926, rate=0.0, all_cells=False):
    """texts: {"I1": bytes or None, "R1": bytes, "R2": bytes or None} (decompressed); whitelist: bytes of the file or None.
    Returns {name: decompressed output bytes} for the present inputs."""
    wl = set()
    if whitelist is not None:
        wl = {c_str(ln)[:len_cb] for ln in lines(whitelist)}
    recs = {k: records(v) for k, v in texts.items() if v is not None}
    out = {k: [] for k in recs}
    _libc.srand(seed % (1 << 32))
    for i, r1 in enumerate(recs["R1"]):
        d = _libc.rand()
        if not draw_passes(d, rate):
            continue
        if not all_cells and c_str(r1[1])[:len_cb] not in wl:
            continue
        for k, rs in recs.items():
            if i < len(rs):
                rec = rs[i]
                out[k].append(c_str(rec[0]) + c_str(rec[1]) + b"+\n" + c_str(rec[3]))
    return {k: b"".join(v) for k, v in out.items()}


class _Fastq(C.Structure):
    _fields_ = [("id", C.c_char_p), ("seq", C.c_char_p), ("qual", C.c_char_p)]


class _Comb(C.Structure):
    _fields_ = [("I1", C.POINTER(_Fastq)), ("R1", C.POINTER(_Fastq)), ("R2", C.POINTER(_Fastq)), ("random_number", C.c_double)]


def ref_lib():
    L = C.CDLL(REF_TREE)
    L.get_row.argtypes = [C.c_char_p]
    L.get_row.restype = C.c_int
    L.read_txt.argtypes = [C.c_char_p, C.c_size_t]
    L.read_txt.restype = C.c_void_p
    L.construct_tree.argtypes = [C.c_void_p, C.c_size_t]
    L.construct_tree.restype = C.c_void_p
    L.get_comb_fastq.argtypes = [C.c_void_p, C.POINTER(C.POINTER(_Comb))]
    L.get_comb_fastq.restype = C.c_int
    L.substring.argtypes = [C.c_char_p, C.c_int, C.c_int]
    L.substring.restype = C.c_void_p
    getattr(L, "in").argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    getattr(L, "in").restype = C.c_bool
    return L


def _zlib():
    z = C.CDLL("libz.so.1")
    z.gzopen.argtypes = [C.c_char_p, C.c_char_p]
    z.gzopen.restype = C.c_void_p
    z.gzclose.argtypes = [C.c_void_p]
    return z


def ref_tree(whitelist_path):
    """the reference's own whitelist tree (get_row + read_txt + construct_tree) and its row count"""
    L = ref_lib()
    n = L.get_row(os.fsencode(whitelist_path))
    rows = L.read_txt(os.fsencode(whitelist_path), n)
    return L.construct_tree(rows, n), n


def ref_driver(paths, whitelist=None, len_cb=16, seed=926, rate=0.0, all_cells=False):
    """paths: {"I1": path or None, "R1": path, "R2": path or None}.  Returns {name: decompressed output bytes}."""
    L, z = ref_lib(), _zlib()
    tree = None
    if whitelist is not None:
        tree, _ = ref_tree(whitelist)
    files = (C.c_void_p * 3)()
    for k, name in enumerate(NAMES):
        files[k] = z.gzopen(os.fsencode(paths[name]), b"r") if paths.get(name) else None
    out = {name: [] for name in NAMES if paths.get(name)}
    block = _Comb()
    pb = C.pointer(block)
    rate32 = float(np.float32(rate))
    _libc.srand(seed % (1 << 32))
    inf = getattr(L, "in")
    while L.get_comb_fastq(files, C.byref(pb)) != -1:
        b = pb.contents
        cb = L.substring(b.R1.contents.seq, 0, len_cb)
        if b.random_number < rate32 and (all_cells or inf(tree, cb, len_cb)):
            for name, ptr in (("I1", b.I1), ("R1", b.R1), ("R2", b.R2)):
                if name in out and ptr:
                    f = ptr.contents
                    out[name].append(f.id + f.seq + b"+\n" + f.qual)
    for k in range(3):
        if files[k]:
            z.gzclose(files[k])
    return {k: b"".join(v) for k, v in out.items()}


def ref_stdout(whitelist=None, nrow=0, r2=True):
    s = "whitelist: %s\n" % (whitelist if whitelist is not None else "(null)")
    if not r2:
        s += "TRUE\n"
    if whitelist is not None:
        s += "Reading whitelist...\nnrow = %d\nProcessing fastq files...\n" % nrow
    else:
        s += "Subsample fastq files directly without cell barcode whitelist...\nProcessing fastq files...\n"
    return s


def read_outputs(outdir, names):
    res = {}
    for name in names:
        p = os.path.join(outdir, "%s.fastq.gz" % name)
        res[name] = gzip.decompress(open(p, "rb").read()) if os.path.exists(p) else None
    return res


def encode(text: bytes, fmt: str) -> bytes:
    """text in one of the framings gzopen() reads: plain, gzip, several gzip members, BGZF"""
    from fastf_amd import synth
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


def tenx_triple(n, seed=1, n_cells=500, p_other=0.2):
    """a 10x-shaped triple: R1 = 16 bp barcode + 12 bp UMI, I1 10 bp, R2 90 bp; most barcodes from a pool of n_cells.
    Returns (texts, barcodes) with texts = {"I1", "R1", "R2"} bytes."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    pool = acgt[rng.integers(0, 4, size=(n_cells, 16))]
    pick = rng.integers(0, n_cells, size=n)
    cb = pool[pick]
    other = rng.random(n) < p_other
    cb[other] = acgt[rng.integers(0, 4, size=(int(other.sum()), 16))]
    umi = acgt[rng.integers(0, 4, size=(n, 12))]
    seq1 = np.concatenate([cb, umi], axis=1)
    texts = {}
    idw = len("@r%d\n" % (n - 1))
    head = np.frombuffer(b"".join(b"@r%-*d\n" % (idw - 3, i) for i in range(n)), dtype=np.uint8).reshape(n, idw)
    nl = np.full((n, 1), ord("\n"), dtype=np.uint8)
    plus = np.frombuffer(b"+\n" * n, dtype=np.uint8).reshape(n, 2)
    for name, seq in (("R1", seq1), ("I1", acgt[rng.integers(0, 4, size=(n, 10))]), ("R2", acgt[rng.integers(0, 4, size=(n, 90))])):
        L = seq.shape[1]
        qual = np.full((n, L), ord("F"), dtype=np.uint8)
        texts[name] = np.concatenate([head, seq, nl, plus, qual, nl], axis=1).tobytes()
    return texts, [bytes(r) for r in pool]
