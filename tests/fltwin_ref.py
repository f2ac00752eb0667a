"""What filter's device windows (csrc/filter_kernels.hpp, the fastf_fltdev_* handle) must return, restated in plain Python / numpy
over the WHOLE byte string of a file: no tiles, no carries, no scans (tests/test_fltwin_ref_host.py, tests/test_gpu_filter_windows.py).

Framing   line j ends at the j-th '\n'; a non-empty text that does not end in '\n' gets a virtual newline at offset len(text) that
          closes the last line and is no part of it.  Read r is lines 4r .. 4r + 3; its output is id + seq + "+\n" + qual, and qual
          loses its newline only when that newline is the virtual one.
Lengths   gzgets(buf, 1024) hands back a line with its real newline: more than 1023 such bytes is an error of the line's read
          (reads >= limit are exempt), the first offending read is recorded.
Draws     chunk_draws: 2048 outputs per 31-word state S: output S[0] >> 1, then S = S[1:] + [(S[0] + S[28]) mod 2^32].
Key       L <= 31 and the sequence line holds L bytes of ACGT before its newline: bit 63 | 2 bits per base (A < C < G < T);
          anything else is an escape, which the caller judges.
Windows   a read belongs to the window its last newline lies in; a read of such a window that begins more than FLT_HDR bytes in
          front of the window begins before the device buffer: error bit 2, no decision, no output."""
import numpy as np

import filter_ref as R

FLT_HDR = 4096
CHUNK = 2048
DEG = 31
MAX_LINE = 1023
MAX_DNA = 31
DNA_TAG = 1 << 63
ERR_LONG_LINE, ERR_REC_START, ERR_ESCAPES = 1, 2, 4
NONE = (1 << 64) - 1


def chunk_draws(states, n):
    """the first n outputs of the chunks whose start states are the rows of `states` ((ceil(n / 2048), 31) words), chunk after chunk"""
    S = np.asarray(states, dtype=np.uint32).reshape(-1, DEG)
    nch = (n + CHUNK - 1) // CHUNK
    assert len(S) >= nch
    w = np.zeros((nch, CHUNK + DEG), dtype=np.uint32)
    w[:, :DEG] = S[:nch]
    for u in range(CHUNK if nch > 1 else n):                  # S[0] + S[28] of the state at step u are words u and u + 28
        w[:, u + DEG] = w[:, u] + w[:, u + 28]
    return (w[:, :CHUNK] >> 1).reshape(-1)[:n].copy()


def passes(draws, rate):
    """filter_ref.draw_passes for an array of draws: float32(int32(r)) * 2^-31 < float32(rate)"""
    f = np.asarray(draws).astype(np.int32).astype(np.float32) * np.float32(2.0 ** -31)
    return f < np.float32(rate)


def dna_key(body, L):
    """body: the sequence line without its newline.  The DNA-form key of its first L bytes, or 0: an escape"""
    if L > MAX_DNA or len(body) < L:
        return 0
    v = 0
    for c in body[:L]:
        k = b"ACGT".find(bytes([c]))
        if k < 0:
            return 0
        v = (v << 2) | k
    return DNA_TAG | v


class Framing:
    """the lines and reads of a text"""

    def __init__(self, text):
        self.text = bytes(text)
        t = np.frombuffer(self.text, dtype=np.uint8)
        nl = np.flatnonzero(t == 10).astype(np.int64)
        self.tv = None
        if len(t) and t[-1] != 10:
            self.tv = len(t)
            nl = np.append(nl, len(t))
        self.nl = nl
        self.n_nl = len(nl)
        self.n_reads = len(nl) // 4
        self.start = np.concatenate([np.zeros(1, np.int64), nl[:-1] + 1])[:len(nl)]
        self.line_bytes = nl - self.start + 1                 # what gzgets hands back
        if self.tv is not None:
            self.line_bytes[-1] -= 1
        self.last = nl[3::4][:self.n_reads]                   # the newline that ends read r

    def line(self, j):
        """line j with its real newline"""
        return self.text[self.start[j]:self.start[j] + self.line_bytes[j]]

    def body(self, j):
        ln = self.line(j)
        return ln[:-1] if ln.endswith(b"\n") else ln

    def out(self, r):
        return self.line(4 * r) + self.line(4 * r + 1) + b"+\n" + self.line(4 * r + 3)

    def first_long(self, limit=NONE):
        """(error bit, first read with a line of more than 1023 bytes among the reads below limit)"""
        bad = np.flatnonzero(self.line_bytes > MAX_LINE) // 4
        bad = bad[bad < limit]
        return (ERR_LONG_LINE, int(bad[0])) if len(bad) else (0, NONE)

    def windows(self, lens):
        """[(a, len, tv, r_lo, n_rec)] of the windows with these byte counts (their sum is the text); len and tv as the host passes
        them: the last window holds the virtual newline"""
        assert sum(lens) == len(self.text)
        res, a = [], 0
        for k, n in enumerate(lens):
            tv, ln = NONE, n
            if k == len(lens) - 1 and self.tv is not None:
                tv, ln = self.tv, n + 1
            r_lo = int(np.searchsorted(self.last, a, side="left"))
            r_hi = int(np.searchsorted(self.last, a + ln, side="left"))
            res.append((a, ln, tv, r_lo, r_hi - r_lo))
            a += n
        return res


def run(fr, lens, mode=0, all_cells=True, L=16, rate=2.0, draws=None, wl_keys=(), judge=None, bitmap=None, limit=NONE):
    """One file through the windows `lens`.  mode 0: draws[r] is read r's draw, wl_keys the DNA-form keys of the whitelist,
    judge(r, line) the verdict on an escape (line: the sequence line with its real newline); mode 1: bitmap[r] decides.
    Returns (per window dict(a, len, tv, r_lo, n_rec, out, total, esc {(i, s1)}, esc_keep {i}, kept), end dict(n_nl, kept, err,
    err_rec), keep: bool per read)."""
    wl_keys = set(int(k) for k in wl_keys)
    keep = np.zeros(fr.n_reads, dtype=bool)
    err, err_rec = fr.first_long(limit) if lens else (0, NONE)
    kept, wins = 0, []
    for a, ln, tv, r_lo, n_rec in fr.windows(lens):
        out, esc, esc_keep = [], set(), set()
        for i in range(n_rec):
            r = r_lo + i
            if r >= limit:
                continue
            if fr.start[4 * r] < a - FLT_HDR:                  # begins before the buffer
                err |= ERR_REC_START
                err_rec = min(err_rec, r)
                continue
            if mode == 1:
                k = bool(bitmap[r]) if r < len(bitmap) else False
            elif not R.draw_passes(int(draws[r]), rate):
                k = False
            elif all_cells:
                k = True
            else:
                key = dna_key(fr.body(4 * r + 1), L)
                if key:
                    k = key in wl_keys
                else:
                    esc.add((i, int(fr.start[4 * r + 1]) - a + FLT_HDR))
                    k = bool(judge(r, fr.line(4 * r + 1))) if judge else False
                    if k:
                        esc_keep.add(i)
            if k:
                keep[r] = True
                out.append(fr.out(r))
        out = b"".join(out)
        if mode == 0:
            kept += int(keep[r_lo:r_lo + n_rec].sum())
        wins.append(dict(a=a, len=ln, tv=tv, r_lo=r_lo, n_rec=n_rec, out=out, total=len(out), esc=esc, esc_keep=esc_keep, kept=kept))
    n_nl = int(np.searchsorted(fr.nl, wins[-1]["a"] + wins[-1]["len"], side="left")) if wins else 0
    return wins, dict(n_nl=n_nl, kept=kept, err=err, err_rec=err_rec), keep
