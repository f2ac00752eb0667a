"""Python mirror of `fastF freq` (include/fastf_amd.h: fastf_freq_text): the cell barcode + UMI prefixes of an R1 FASTQ
(plain, gzip or BGZF) and their frequencies, counted on the device; and of `fastF filter` (fastf_filter): FASTQ triples
subsampled by cell barcode whitelist and read depth on the device."""
import ctypes as C
import os
import re

import numpy as np

from . import _lib
from .engine import _libc_free


def freq_text(path, len_cb: int = 16, len_umi: int = 10, device=None) -> bytes:
    """the bytes `fastF freq -R path -l len_cb -u len_umi` writes to whitelist.txt.  device: only 0 (or None) — the
    histogram of freq runs on the process's device 0 (FASTF_DEVICE / ROCR_VISIBLE_DEVICES choose which card that is)"""
    if device not in (None, 0):
        raise ValueError("freq_text runs on device 0 of the process")
    p, n, nr = C.c_void_p(), C.c_size_t(), C.c_uint64()
    _lib.check(_lib.lib().fastf_freq_text(str(path).encode(), len_cb, len_umi, C.byref(p), C.byref(n), C.byref(nr)))
    txt = C.string_at(p.value, n.value)
    _libc_free(p)
    return txt


_ROW = re.compile(rb"(.*?),([0-9]+)\n", re.S)


def freq(path, len_cb: int = 16, len_umi: int = 10, device=None):
    """[(prefix, count)] in whitelist.txt order.  A prefix is the read's first len_cb + len_umi bytes as the reference keeps
    them: a shorter sequence line keeps its newline, so rows are split at the first ",<count>\n" (a prefix that itself holds
    ",<digits>\n" cannot be told apart from a row end; use freq_text for such input)"""
    return [(m.group(1), int(m.group(2))) for m in _ROW.finditer(freq_text(path, len_cb, len_umi, device))]


def filter(r1, i1=None, r2=None, out=".", whitelist=None, len_cb: int = 16, seed: int = 926, rate: float = 0.0,
           all_cells: bool = False):
    """`fastF filter -R r1 [-I i1] [-r r2] -o out [-w whitelist] -l len_cb -s seed -t rate [-a]`: writes out/R1.fastq.gz (and
    I1 / R2) and returns (reads in R1, reads kept).  seed is taken modulo 2^32 (-1 is 4294967295, as the reference's
    (unsigned) cast); runs on the process's device 0"""
    if whitelist is None and not all_cells:
        raise ValueError("filter needs a whitelist or all_cells=True")
    if len_cb < 0:
        raise ValueError("len_cb must not be negative")
    enc = lambda p: None if p is None else os.fspath(p).encode()  # noqa: E731
    nr, nk = C.c_uint64(), C.c_uint64()
    _lib.check(_lib.lib().fastf_filter(enc(r1), enc(i1), enc(r2), enc(out), enc(whitelist), len_cb, seed % (1 << 32),
                                       float(rate), int(bool(all_cells)), C.byref(nr), C.byref(nk)))
    return nr.value, nk.value


def fqcap(r1, i1=None, r2=None, out=".", whitelist=None, len_cb: int = 16, seed: int = 926, rate: float = 2.0, cap: int = 0):
    """`fastF fqcap -R r1 [-I i1] [-r r2] -o out -w whitelist -n cap [-t rate] -l len_cb -s seed`: filter with every cell of the
    whitelist capped at `cap` reads (in expectation; include/fastf_amd.h has the definition).  Writes out/R1.fastq.gz (and I1 /
    R2) and out/fqcap_cells.tsv.gz and returns (reads in R1, reads matched, reads kept).  rate 2.0: no thinning beside the cap"""
    if whitelist is None:
        raise ValueError("fqcap needs a whitelist")
    if int(cap) < 1 or int(cap) >= 1 << 64:
        raise ValueError("cap must be a whole number of reads, at least 1")
    if len_cb < 0:
        raise ValueError("len_cb must not be negative")
    enc = lambda p: None if p is None else os.fspath(p).encode()  # noqa: E731
    nr, nm, nk = C.c_uint64(), C.c_uint64(), C.c_uint64()
    _lib.check(_lib.lib().fastf_fqcap(enc(r1), enc(i1), enc(r2), enc(out), enc(whitelist), len_cb, seed % (1 << 32), float(rate),
                                      int(cap), C.byref(nr), C.byref(nm), C.byref(nk)))
    return nr.value, nm.value, nk.value


def fqcap_rate(cap: int, hits: int, rate: float = 2.0) -> float:
    """the keep rate of a cell with `hits` matched reads under the cap and the global rate (fastf_fqcap_rate)"""
    return float(_lib.lib().fastf_fqcap_rate(int(cap), int(hits), float(rate)))


def _fqcells_rule(expect, top, min_umis):
    given = [(r, v) for r, v in (("e", expect), ("k", top), ("m", min_umis)) if v is not None]
    if len(given) > 1:
        raise ValueError("fqcells takes one calling rule: expect, top or min_umis")
    rule, arg = given[0] if given else ("e", 3000)
    if int(arg) < 1 or int(arg) >= 1 << 64:
        raise ValueError("the rule's argument must be a whole number, at least 1")
    return rule, int(arg)


def fqcells(r1, out=".", len_cb: int = 16, len_umi: int = 10, expect=None, top=None, min_umis=None) -> dict:
    """`fastF fqcells -R r1 -o out -l len_cb -u len_umi [-e expect | -k top | -m min_umis]` (none: -e 3000): the cells of an R1
    FASTQ called by UMIs per barcode (include/fastf_amd.h has the definition).  Writes out/fqcells.tsv.gz, out/whitelist.txt and
    out/fqcells_summary.tsv and returns the summary row as a dict (rule as its letter)"""
    rule, arg = _fqcells_rule(expect, top, min_umis)
    if len_cb < 1 or len_umi < 0 or len_cb + len_umi > 31:
        raise ValueError("len_cb >= 1, len_umi >= 0 and len_cb + len_umi <= 31")
    s = _lib.FqcellsSummary()
    _lib.check(_lib.lib().fastf_fqcells(os.fspath(r1).encode(), os.fspath(out).encode(), len_cb, len_umi, ord(rule), arg, C.byref(s)))
    d = {n: int(getattr(s, n)) for n, _ in s._fields_}
    d["rule"] = chr(d["rule"])
    return d


def fqcells_call(bc, reads, umis, expect=None, top=None, min_umis=None):
    """the order and the calling rule of fqcells on a table of barcodes (fastf_fqcells_call, on the host): bc = distinct barcodes
    packed 2 bits a base (uint64), reads (uint64), umis (uint32).  Returns (rank uint32 1-based, called bool, threshold)"""
    rule, arg = _fqcells_rule(expect, top, min_umis)
    bc = np.ascontiguousarray(bc, dtype=np.uint64)
    reads = np.ascontiguousarray(reads, dtype=np.uint64)
    umis = np.ascontiguousarray(umis, dtype=np.uint32)
    if not len(bc) == len(reads) == len(umis):
        raise ValueError("bc, reads and umis are one table")
    rank, called, thr = np.zeros(len(bc), dtype=np.uint32), np.zeros(len(bc), dtype=np.uint8), C.c_uint64()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _lib.check(_lib.lib().fastf_fqcells_call(ptr(bc), ptr(reads), ptr(umis), len(bc), ord(rule), arg, ptr(rank), ptr(called), C.byref(thr)))
    return rank, called.astype(bool), thr.value


def filter_draws(seed: int, first: int, n: int, device: bool = True) -> np.ndarray:
    """rand() outputs first .. first + n - 1 after srand(seed) (uint32): as filter's device kernel computes them, or
    (device=False) by the host's jump-ahead and recurrence"""
    out = np.empty(n, dtype=np.uint32)
    fn = _lib.lib().fastf_filter_draws if device else _lib.lib().fastf_filter_draws_host
    _lib.check(fn(seed % (1 << 32), first, n, out.ctypes.data_as(C.c_void_p)))
    return out


def filter_rand_at(seed: int, index: int) -> int:
    """the rand() output with this index after srand(seed), by the host's jump-ahead"""
    return _lib.lib().fastf_filter_rand_at(seed % (1 << 32), index)
