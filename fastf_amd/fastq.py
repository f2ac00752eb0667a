"""Python mirror of `fastF freq` (include/fastf_amd.h: fastf_freq_text): the cell barcode + UMI prefixes of an R1 FASTQ
(plain, gzip or BGZF) and their frequencies, counted on the device."""
import ctypes as C
import re

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
