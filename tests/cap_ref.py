"""The reference for one point of `fastF cap`, built on the unchanged oracle.

numpy computes who is kept: the sampled cells and the SampleInt draws (skip) as the oracle samples them, the CB hits in file order
and the hits per cell h, the thresholds T (fastf_draw_threshold restated in float32 / float64: SURVEY section 7.3), and
keep = mt_stream(seed, H, skip) < T[cell].  The has-CB flag of every hit that is not kept is then cleared and the oracle runs on
the masked records with rate_depth 1.0: a masked record still counts in `total` and draws nothing, so the oracle's hit i is kept
hit i, and rate 1.0 drops nothing but a draw of 0xFFFFFFFF — which the callers' seeds do not produce (asserted here)."""
import re

import numpy as np

from oracle import oracle as O
from sweep_ref import expected_row

_C = 1.0 / 4294967295.0


def draw_threshold(rate) -> int:
    """fastf_draw_threshold: the number of 32-bit draws d with d * (1 / 4294967295) < (double)(float)rate (genrand_real1 against the
    float rate promoted to double); 2^32 when no draw is dropped, 0 when every one is"""
    r = float(np.float32(rate))
    if not (0xFFFFFFFF * _C >= r):
        return 1 << 32
    if 0 * _C >= r:
        return 0
    t = int(np.ceil(r / _C))
    t = min(max(t, 2), 0xFFFFFFFF)
    for cand in range(t - 2, t + 3):                       # the smallest dropped draw, exactly, by the very expression
        if cand >= 1 and cand * _C >= r and not ((cand - 1) * _C >= r):
            return cand
    raise AssertionError("no threshold for rate %r" % rate)


def thresholds(h, cap):
    h = np.asarray(h, dtype=np.uint64)
    out = np.full(len(h), 1 << 32, dtype=np.uint64)
    for k in np.nonzero(h > np.uint64(cap))[0]:
        out[k] = draw_threshold(np.float32(np.float64(cap) / np.float64(h[k])))
    return out


def realised(sampled, hits) -> float:
    return float(np.float32(np.float64(sampled) / np.float64(hits))) if hits else 1.0


def hits_of(case, rate_cell, seed, bam_label=b"x.bam"):
    """(the oracle's run at depth 1.0, cell index per record (0: no hit), h per sampled cell, skip) — all from the oracle's side: the
    sampled cells are its sampled_lines (cell index = place in its barcodes output), skip = the draws its SampleInt consumed: one per
    sampled line, none when every line is taken (utils.c:48-62)"""
    rc = float(np.float32(rate_cell))
    probe = O.run_bam2db(case.bt, case.ft, case.flags, case.xf, case.cb, case.gx, case.ub, rc, 1.0, seed, bam_label, False)
    lines = case.bt.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    sampled = probe["sampled_lines"]
    names = probe["barcodes"].split(b"\n")[:-1]
    assert names == [lines[int(i)] for i in sampled] and len(set(names)) == len(names)
    skip = len(sampled) if len(sampled) < len(lines) else 0
    index = {b: i + 1 for i, b in enumerate(names)}
    has_cb = (np.asarray(case.flags) & O.HAS_CB) != 0
    cell = np.array([index.get(bytes(c), 0) if ok else 0 for c, ok in zip(case.cb, has_cb)], dtype=np.int64)
    h = np.bincount(cell[cell > 0] - 1, minlength=len(names)).astype(np.uint64)
    return probe, cell, h, skip


def point(case, bam_label, rate_cell, cap, seed):
    """dict: matrix / barcodes / features (expected bytes), hits, cells_capped, sampled, realised, row (the cap.tsv fields)"""
    rc = float(np.float32(rate_cell))
    probe, cell, h, skip = hits_of(case, rc, seed, bam_label)
    H = int(h.sum())
    T = thresholds(h, cap)
    stream = O.mt_stream(seed, H, skip).astype(np.uint64)
    assert not (stream == np.uint64(0xFFFFFFFF)).any(), "seed %d draws 0xFFFFFFFF among the first %d: pick another" % (seed, H)
    hit_cells = cell[cell > 0]
    keep = stream < T[hit_cells - 1]
    flags = np.array(case.flags, dtype=np.uint8, copy=True)
    hit_at = np.nonzero(cell > 0)[0]
    flags[hit_at[~keep]] &= np.uint8(~O.HAS_CB & 0xFF)
    ora = O.run_bam2db(case.bt, case.ft, flags, case.xf, case.cb, case.gx, case.ub, rc, 1.0, seed, bam_label, False)
    sampled = int(keep.sum())
    assert ora["sampled"] == sampled and ora["total"] == len(flags)
    frac = realised(sampled, H)
    matrix, n_sub = re.subn(rb'(%\t"rate_depth": )[^,\n]*,', lambda m: m.group(1) + b"%.3f," % frac, ora["matrix"], count=1)
    assert n_sub == 1
    capped = int((h > np.uint64(cap)).sum())
    row = expected_row(matrix, rc, 0.0, seed)
    row[1] = str(int(cap))
    row += [str(H), str(capped), "%.6f" % frac]
    return dict(matrix=matrix, barcodes=ora["barcodes"], features=ora["features"], hits=H, cells_capped=capped, sampled=sampled,
                realised=frac, row=row, h=h, keep=keep)
