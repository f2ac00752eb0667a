"""The definition of `fastF fqcap` (include/fastf_amd.h) in Python, for tests/test_fqcap_host.py and tests/test_gpu_fqcap.py.

Built on the unchanged filter_ref.py: py_filter(..., rate=2.0) says which reads are matched (that rule is pinned against the
reference's own functions there), numpy's float32 / float64 reproduce rate_k, draw_passes decides.  Also the fixture builders."""
import collections
import gzip
import os

import numpy as np

import filter_ref as R

HEADER = b"barcode\treads\tkept\n"


def rate_of(cap, h, t=2.0):
    """rate_k: t where h <= N, min(t, (float)((double)N / (double)h)) otherwise, as a numpy float32"""
    t = np.float32(t)
    if h <= cap:
        return t
    c = np.float32(np.float64(cap) / np.float64(h))
    return c if c < t else t


def cell_bytes(seq_line, len_cb):
    """the first len_cb bytes of a sequence line as strncmp sees a gzgets buffer: with its newline, cut at a NUL"""
    return R.c_str(seq_line)[:len_cb]


def matched_mask(r1_text, whitelist, len_cb):
    """[bool per R1 read]: filter -w would match it.  Read off py_filter's output at rate 2.0 (every draw passes): its records are
    the matched ones in order, and records that are equal byte for byte are decided alike"""
    recs = R.records(r1_text)
    out = R.records(R.py_filter({"I1": None, "R1": r1_text, "R2": None}, whitelist, len_cb, 0, 2.0)["R1"])
    forms = [R.c_str(r[0]) + R.c_str(r[1]) + b"+\n" + R.c_str(r[3]) for r in recs]
    kept_forms = {b"".join(o) for o in out}
    mask = [f in kept_forms for f in forms]
    assert sum(mask) == len(out)
    return mask


def draws_of(seed, n):
    R._libc.srand(seed % (1 << 32))
    return [R._libc.rand() for _ in range(n)]


def tsv_field(b):
    return b"".join(bytes([c]) if 0x20 < c < 0x7f and c != 0x5c else b"\\x%02X" % c for c in b)


def py_fqcap(texts, whitelist, len_cb=16, seed=926, rate=None, cap=1):
    """texts as py_filter takes them.  Returns dict(out {name: bytes}, h, kept (Counters by cell bytes), keep [bool per read],
    n_reads, n_matched, n_kept, tsv (the decompressed bytes of fqcap_cells.tsv.gz))"""
    t = 2.0 if rate is None else rate
    recs = {k: R.records(v) for k, v in texts.items() if v is not None}
    r1 = recs["R1"]
    mask = matched_mask(texts["R1"], whitelist, len_cb)
    cells = [cell_bytes(r[1], len_cb) if m else None for r, m in zip(r1, mask)]
    h = collections.Counter(c for c in cells if c is not None)
    draws = draws_of(seed, len(r1))
    rates = {c: rate_of(cap, n, t) for c, n in h.items()}
    keep = [c is not None and R.draw_passes(d, rates[c]) for c, d in zip(cells, draws)]
    kept = collections.Counter(c for c, k in zip(cells, keep) if k)
    out = {k: [] for k in recs}
    for i, k_i in enumerate(keep):
        if not k_i:
            continue
        for k, rs in recs.items():
            if i < len(rs):
                rec = rs[i]
                out[k].append(R.c_str(rec[0]) + R.c_str(rec[1]) + b"+\n" + R.c_str(rec[3]))
    tsv = HEADER + b"".join(tsv_field(c) + b"\t%d\t%d\n" % (h[c], kept[c]) for c in sorted(h))
    return dict(out={k: b"".join(v) for k, v in out.items()}, h=h, kept=kept, keep=keep, n_reads=len(r1), n_matched=sum(mask),
                n_kept=sum(keep), tsv=tsv)


def read_tsv(outdir):
    return gzip.decompress(open(os.path.join(str(outdir), "fqcap_cells.tsv.gz"), "rb").read())


# ---------------------------------------------------------------- fixtures
# cells of exactly these read counts beside the pool's: h = N and h = N + 1 for every cap the GPU tests use below the pool's depth
SPECIAL_H = (1, 2, 5, 6, 50, 51)
ESC_CELL, ESC_H = b"ACGTNACGTACGTACG", 60            # an escape-form cell (an N inside) above every such cap
CAPS = (1, 5, 50)                                    # (10^9, the fourth cap of the GPU tests, is above every cell: the no-cap case)


def special_cells():
    """16-base barcodes, distinct in their first 12 bases, that no pool of tenx_triple holds (they end in a fixed tail)"""
    acgt = b"ACGT"
    return [bytes(acgt[(k >> (2 * j)) & 3] for j in range(6)) + b"GATTACAGAT" for k in range(1, len(SPECIAL_H) + 1)]


def triple(n=3000, seed=5, n_cells=40):
    """a 10x-shaped triple of n reads over n_cells pool cells, plus the special cells and the escape-form cell at their exact read
    counts.  Returns (texts, pool, whitelist bytes): the whitelist holds every second pool cell, the special cells and the
    escape-form cell"""
    texts, pool = R.tenx_triple(n, seed=seed, n_cells=n_cells, p_other=0.3)
    r1 = R.records(texts["R1"])
    plan = [c for c, hh in zip(special_cells(), SPECIAL_H) for _ in range(hh)] + [ESC_CELL] * ESC_H
    assert 7 * len(plan) + 3 < n
    for k, cb in enumerate(plan):
        r1[7 * k + 3][1] = cb + r1[7 * k + 3][1][16:]
    texts["R1"] = b"".join(b"".join(r) for r in r1)
    wl = b"".join(b + b"\n" for b in pool[::2] + special_cells() + [ESC_CELL])
    return texts, pool, wl


def prefix_whitelists(pool):
    """at len_cb = 12: duplicate lines, and lines that share their first 12 bytes — no extra cells either way"""
    base = pool[::2] + special_cells() + [ESC_CELL]
    return {
        "duplicates": b"".join(b + b"\n" for b in base + base[::3] + [ESC_CELL]),
        "shared_prefixes": b"".join(b[:12] + tail + b"\n" for b in base for tail in (b"AAAA", b"CCCC-1", b"")),
    }


# (name, builder of (texts, whitelist), len_cb): every fixture the GPU tests cap at CAPS; tests/test_fqcap_host.py takes their census
def fixtures():
    texts, pool, wl = triple()
    fx = [("main", texts, wl, 16)]
    for kind, w in prefix_whitelists(pool).items():
        fx.append((kind, texts, w, 12))
    return fx


def census(texts, whitelist, len_cb, cap):
    """what the fixture offers a cap: cells above it, at or below it, at exactly N and N + 1, escape-form cells above it"""
    ref = py_fqcap(texts, whitelist, len_cb, 926, None, cap)
    h = ref["h"]
    dna = lambda c: len(c) == len_cb and len_cb <= 31 and all(x in b"ACGT" for x in c)  # noqa: E731
    return dict(above=sum(v > cap for v in h.values()), at_or_below=sum(v <= cap for v in h.values()),
                exact=sum(v == cap for v in h.values()), plus_one=sum(v == cap + 1 for v in h.values()),
                esc_above=sum(v > cap and not dna(c) for c, v in h.items()))
