"""freq's device parse (csrc/fastq_kernels.hpp: count / scan / pending / emit) in plain Python: what the device must leave after
every window and at the end, for a text cut into windows [(a, len)] that tile it, the last one with last = 1 (it may be empty).

Per read r, independent of the windows: sequence line r starts at s_r, the byte after the (4r + 1)-th '\\n'; avail = bytes from
s_r to the end of the text.  L <= 31, avail >= L and L bytes of ACGT -> DNA_TAG | 2 bits per base (A<C<G<T, first base highest);
anything else -> the escape (s_r, r), whose string the host cuts with strncpy semantics (escape_len).  L = 0: DNA_TAG for every read.

Per window: a sequence line is handed to the next window when the window is not the last and s + need > a + len, need = L
(L <= 31) or 1024 (escape path: the host must see a whole gzgets buffer); the next window resolves it.  What a window resolves
it measures against its own end, so a window that takes lines over must hold `need` bytes behind each unless it is the last
(the product's windows are full but for the last; run() asserts it).  The line index of a '\\n' comes from its tile's base as the
scan builds it (4096-byte tiles; 1024 lanes of ceil(n_tiles / 1024) tiles each, then across the lanes).

`defect` turns one rule into a wrong one (DEFECTS); tests/test_fqwin_ref_host.py shows that every one of them changes the
expected output of some fixture below, i.e. that tests/test_gpu_freq_windows.py would fail for a device with that bug."""
import numpy as np

FQ_HDR, MAX_LINE, MAX_DNA, TILE, PEND_CAP = 1024, 1023, 31, 4096, 1024
DNA_TAG = 1 << 63
ERR_LONG_LINE, ERR_PENDING, ERR_ESCAPES, ERR_KEY_CAP = 1, 2, 4, 8
NONE = (1 << 64) - 1

DEFECTS = (
    "closed_line",        # the sequence-line test and r taken from the line the '\n' closes, not from the one it opens (with r alone
                          # the shift by two bits hides the difference: 4r and 4r + 1 name the same read)
    "need_L_on_escape",   # need = L on the escape path: an escape whose 1024 bytes run past the window is reported a window early
    "pend_avail_prev",    # a line taken over resolved with avail measured to the end of the window that handed it on
    "err_rec_last",       # err_rec = the last offending read
    "line_start_dropped",  # a window without a '\n' leaves its own start as the open line's start
    "scan_first_level",   # tiles beyond the first 1024: base from the lane's own tiles alone
    "pack_reversed",      # first base in the lowest two bits
    "n_is_a_base",        # N accepted (the packer's bit trick gives it A's code)
)


def as_u8(text):
    return np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text


def dna_key(t, s, end, L, defect=None):
    """fq_pack_dna of the line at s with the data ending at `end`: the DNA-form key, or 0"""
    if L > MAX_DNA or end < s or end - s < L:
        return 0
    v = 0
    for i, c in enumerate(t[s:s + L].tolist()):
        code = b"ACGT".find(c)
        if code < 0 and c == 78 and defect == "n_is_a_base":
            code = 0
        if code < 0:
            return 0
        v = v | code << 2 * i if defect == "pack_reversed" else v << 2 | code
    return DNA_TAG | v


def escape_len(t, s, end, L):
    """fq_escape_len: bytes of the key string strncpy leaves of the gzgets buffer"""
    n = min(L, max(end - s, 0), MAX_LINE)
    for i, c in enumerate(t[s:s + n].tolist()):
        if c == 0:
            return i
        if c == 10:
            return i + 1
    return n


def bases(v, L):
    return bytes(b"ACGT"[(v >> 2 * (L - 1 - i)) & 3] for i in range(L))


def seq_starts(t):
    """s_r of every read whose sequence line is opened"""
    nl = np.flatnonzero(t == 10)
    return (nl[0::4] + 1).tolist()


def reads(text, L, defect=None):
    """[(s_r, key)] per read from the whole text; key 0: the escape (s_r, r)"""
    t = as_u8(text)
    L = min(L, FQ_HDR)
    return [(s, dna_key(t, s, len(t), L, defect)) for s in seq_starts(t)]


def key_string(text, s, L):
    """the read's key string as the histogram's rows show it, and whether it took the DNA form"""
    t = as_u8(text)
    L = min(L, FQ_HDR)
    k = dna_key(t, s, len(t), L)
    if k:
        return bases(k & ~DNA_TAG, L), True
    return t[s:s + escape_len(t, s, len(t), L)].tobytes(), False


def run(text, lens, L, bound=None, defect=None):
    """-> ([per window dict(a, len, last, keys {r: key}, esc sorted [(s, r)], pend [(s, r)] handed on, n_nl, err)],
    dict(n_nl, line_start, err, err_rec)).  bound: key_bound of every window (None: no read is refused)"""
    t = as_u8(text)
    assert sum(lens) == len(t) and len(lens) >= 1
    L = min(L, FQ_HDR)
    need_true = L if L <= MAX_DNA else FQ_HDR
    need = L if defect == "need_L_on_escape" else need_true
    n_nl, line_start, err, err_rec, pend, a, out = 0, 0, 0, NONE, [], 0, []
    for k, ln in enumerate(lens):
        last, end = k == len(lens) - 1, a + ln
        keys, esc, pend_out = {}, [], []

        def resolve(s, r, end_):
            nonlocal err
            if bound is not None and r >= bound:
                err |= ERR_KEY_CAP
                return
            key = dna_key(t, s, end_, L, defect)
            if key:
                assert defect is not None or r not in keys
                keys[r] = key
            else:
                esc.append((s, r))
        for s, r in pend:
            assert a - s < FQ_HDR
            assert defect is not None or last or end - s >= need_true, "window %d is too short for the lines handed to it" % k
            resolve(s, r, a if defect == "pend_avail_prev" else end)
        nl = np.flatnonzero(t[a:end] == 10) + a
        if len(nl):
            n_tiles = (ln + TILE - 1) // TILE
            tile = (nl - a) // TILE
            cnt = np.bincount(tile, minlength=n_tiles)
            first = np.concatenate(([0], np.cumsum(cnt)[:-1]))
            base = n_nl + first
            if defect == "scan_first_level" and n_tiles > 1024:
                per = (n_tiles + 1023) // 1024
                for i in range(1024, n_tiles):
                    base[i] = n_nl + cnt[i // per * per:i].sum()
            j = base[tile] + (np.arange(len(nl)) - first[tile])
            ls = line_start
            for p, jc in zip(nl.tolist(), j.tolist()):       # the '\n' at p closes line jc, which began at ls
                if p + 1 - ls > MAX_LINE:
                    err |= ERR_LONG_LINE
                    rec = jc >> 2
                    err_rec = rec if defect == "err_rec_last" else min(err_rec, rec)
                ls = p + 1
                jo = jc if defect == "closed_line" else jc + 1
                if (jo & 3) == 1:
                    s, r = p + 1, jo >> 2
                    if not last and s + need > end:
                        pend_out.append((s, r))
                    else:
                        resolve(s, r, end)
            n_nl += len(nl)
            line_start = max(line_start, int(nl[-1]) + 1)
        elif defect == "line_start_dropped":
            line_start = a
        assert len(pend_out) <= PEND_CAP
        out.append(dict(a=a, len=ln, last=int(last), keys=keys, esc=sorted(esc), pend=pend_out, n_nl=n_nl, err=err))
        pend, a = pend_out, end
    return out, dict(n_nl=n_nl, line_start=line_start, err=err, err_rec=err_rec)


def n_reads(text):
    return (int((as_u8(text) == 10).sum()) + 3) // 4


# ---------------------------------------------------------------- fixtures
def seq_for(r, n):
    """n bases that name read r: 31 digits of a hash of r, repeated"""
    v = ((r + 1) * 0x9E3779B97F4A7C15) & ((1 << 62) - 1)
    b = bases(v, 31)
    return (b * (n // 31 + 1))[:n]


class Text:
    """FASTQ text line by line; seq lines name the read they belong to"""

    def __init__(self):
        self.parts, self.n, self.lines = [], 0, 0

    def line(self, body):
        assert b"\n" not in body
        self.parts.append(body + b"\n")
        self.n += len(body) + 1
        self.lines += 1
        return self

    def raw(self, b):
        """bytes as they are (the caller counts the lines)"""
        self.parts.append(b)
        self.n += len(b)
        self.lines += b.count(b"\n")
        return self

    def auto(self, n):
        """a line of n bytes that suits its place in the four-line framing"""
        k, r = self.lines & 3, self.lines >> 2
        return self.line(seq_for(r, n) if k == 1 else ((b"@", b"", b"+", b"I")[k] + (b"h", b"", b"+", b"I")[k] * n)[:n])

    def read(self, seq=None, n=30, hdr=None, qual=None):
        assert self.lines % 4 == 0
        r = self.lines // 4
        seq = seq_for(r, n) if seq is None else seq
        self.line(b"@r%d" % r if hdr is None else hdr).line(seq).line(b"+")
        return self.line(b"I" * len(seq) if qual is None else qual)

    def reads(self, k, n=30):
        for _ in range(k):
            self.read(n=n)
        return self

    def read_at(self, s, seq=None, n=30, qual=None):
        """a read whose sequence line starts at offset s: the header is padded"""
        pad = s - self.n - 2
        assert 0 <= pad <= MAX_LINE - 2, (s, self.n)
        return self.read(seq=seq, n=n, hdr=b"@" + b"h" * pad, qual=qual)

    def fill_to(self, n, step=400):
        """whole reads until the text is at least n bytes long"""
        while self.n < n:
            self.read(n=min(step, max(1, (n - self.n) // 2)))
        return self

    def bytes(self):
        return b"".join(self.parts)


class Fixture:
    def __init__(self, group, name, text, lens, L, W=4096, bound=None):
        self.group, self.name, self.text, self.lens, self.L, self.W = group, name, text, list(lens), L, W
        assert sum(self.lens) == len(text) and all(0 <= x <= W for x in self.lens), name
        self.bound = n_reads(text) + 2 if bound is None else bound

    def expected(self, defect=None):
        return run(self.text, self.lens, self.L, self.bound, defect)

    def __repr__(self):
        return "%s/%s" % (self.group, self.name)


def cut(n, *cuts):
    c = [0] + list(cuts) + [n]
    assert all(x <= y for x, y in zip(c, c[1:])), c
    return [y - x for x, y in zip(c, c[1:])]


def _dna_sweep():
    out, L = [], 26
    for al in range(4):
        s = 260 + al
        text = Text().reads(3).read_at(s).reads(3).bytes()
        assert seq_starts(as_u8(text))[3] == s and s & 3 == al
        for c in range(s - 2, s + L + 3):
            out.append(Fixture("dna_sweep", "s&3=%d cut=s%+d" % (al, c - s), text, cut(len(text), c), L))
    for s in (4095, 4096, 4097):
        t = Text().fill_to(s - 600).read_at(s).fill_to(3 * TILE - 300)
        text = t.bytes()
        assert 2 * TILE < len(text) <= 3 * TILE and s in seq_starts(as_u8(text)) and text[s - 1:s] == b"\n"
        out.append(Fixture("dna_sweep", "tile edge s=%d" % s, text, [len(text)], L, W=3 * TILE))
        out.append(Fixture("dna_sweep", "tile edge s=%d cut at 8192" % s, text, cut(len(text), 2 * TILE), L, W=3 * TILE))
    # the header's '\n' is the last byte of a full window: the line starts at a + len, handed on with no byte seen
    text = Text().fill_to(TILE - 600).read_at(TILE).reads(3).bytes()
    assert text[TILE - 1:TILE] == b"\n" and TILE in seq_starts(as_u8(text))
    out.append(Fixture("dna_sweep", "newline ends the full window", text, cut(len(text), TILE), L))
    return out


def _esc_sweep():
    out = []
    for L in (40, 1024):
        s = 300
        text = Text().reads(2).read_at(s, n=50).fill_to(s + 1400, step=60).bytes()
        assert seq_starts(as_u8(text))[2] == s
        for d in (-1, 0, 1, 1022, 1023, 1024, 1025):
            out.append(Fixture("esc_sweep", "L=%d cut=s%+d" % (L, d), text, cut(len(text), s + d), L))
    return out


def _max_pend():
    out = []
    for L in (40, 5):
        for phase in range(4):
            t = Text().fill_to(TILE - 1023 - 700)
            for _ in range(phase):                            # the four-line framing moves by `phase` against the tail
                t.auto(1)
            pad = TILE - 1023 - t.n
            assert 1 <= pad <= MAX_LINE - 1
            t.raw(seq_for(t.lines >> 2, pad) if (t.lines & 3) == 1 else b"x" * pad).raw(b"\n" * 1023)
            assert t.n == TILE
            while t.n < 3 * TILE + 500:
                t.auto(30)
            text = t.bytes()
            assert text[TILE - 1023:TILE] == b"\n" * 1023 and text[TILE - 1024:TILE - 1023] != b"\n"
            out.append(Fixture("max_pend", "L=%d phase %d" % (L, phase), text, cut(len(text), TILE, 2 * TILE, 3 * TILE), L))
    return out


def _zero_last():
    out = []
    for L in (26, 40):
        # two sequence lines in the last L bytes of a full window, the file ending inside the second
        tail = b"ACGT\n+\nII\n@h\nAC"
        t = Text().fill_to(TILE - 700)
        s = TILE - len(tail)
        t.read_at(s, seq=b"ACGT", qual=b"II").raw(b"@h\nAC")
        text = t.bytes()
        assert len(text) == TILE and text.endswith(tail)
        out.append(Fixture("zero_last", "L=%d two lines handed to an empty last window" % L, text, [TILE, 0], L))
        # the sequence line starts at the very end of the data
        t = Text().fill_to(TILE - 700).read_at(TILE)
        text = t.bytes()[:TILE]
        assert text.endswith(b"h\n")
        out.append(Fixture("zero_last", "L=%d line starts at the end" % L, text, [TILE, 0], L))
    return out


def _many_windows():
    t = Text()
    while t.n < 14000:
        r = t.lines // 4
        if r % 3 == 0:
            seq = seq_for(r, 30)
            t.read(seq=seq[:r % 26] + b"N" + seq[r % 26 + 1:])
        else:
            t.read(n=30 + r % 5)
    text = t.bytes()
    lens = cut(len(text), 1500, 3548, 5000, 9096, 10200, 11300, 12400)
    return [Fixture("many_windows", "eight windows", text, lens, 26),
            Fixture("many_windows", "eight windows L=40", text, lens, 40)]


KINDS = [b"", b"A", b"N", b"ACGTACGTACGTACGTACGTACGTACGTACGTACGT", b"ACGTACGTACGTACGTACGTACGTACGTACGTACGN", b"acgtacgtacgtacgtacgtacgtacgtacgtacgt",
         b"ACGTACGTAC\x00TACGTACGTACGTACGTACGTACGTACG", b"\x00", b"ACGTACGTACGTACGTACGTACGTACGTACG\r", b"ACGTACGTACGTACGTACGTACGTA\r",
         b"ACGT\x80ACGTACGTACGTACGTACGTACGTACGTACGT", b"\xffCGTACGTACGTACGTACGTACGTACGTACGTACGT", b"ACGTACGTACGTACGTACGTACGTACGTACGTACG\xc1",
         b"ACGTACGTACGTACGTACGTACGTACGTAC", b"ACGTACGTACGTACGTACGTACGTACGTACG", b"ACGTACGTACGTACGTACGTACGTACGTACGT", b"ACGTACGTACGTACGTACGTACGTA",
         b"ACGTACGTACGTACGTACGTACGTAC", b"ACGTACGTACGTACGTACGTACGTACG", b"TTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTT", b"T", b"G", b"C", b"GATTACA"]


def _key_kinds():
    out = []
    for L in (0, 1, 26, 31, 32):
        t = Text()
        for i, k in enumerate(KINDS):
            t.read(seq=k, hdr=b"@" + b"x" * (i % 4))
            t.read(n=36)
        t.read(n=36)
        text = t.bytes()
        assert {s & 3 for s in seq_starts(as_u8(text))} == {0, 1, 2, 3}
        last_s = seq_starts(as_u8(text))[-1]
        ends = {"whole": len(text), "ends inside the sequence line": last_s + 20, "ends after the header": last_s,
                "ends one byte into the sequence line": last_s + 1}
        for name, n in ends.items():
            out.append(Fixture("key_kinds", "L=%d %s" % (L, name), text[:n], [n], L))
            out.append(Fixture("key_kinds", "L=%d %s, two windows" % (L, name), text[:n], cut(n, 1111), L))
    return out


def _long_lines():
    out, L = [], 26
    for n in (1022, 1023):                                    # bodies: 1023 / 1024 bytes with the '\n'
        for which in range(4):
            t = Text().reads(2)
            body = [b"@" + b"h" * (n - 1), seq_for(2, n), b"+" * n, b"I" * n][which]
            lines = [b"@r2", seq_for(2, 30), b"+", b"I" * 30]
            lines[which] = body
            for ln in lines:
                t.line(ln)
            text = t.reads(2).bytes()
            out.append(Fixture("long_lines", "line %d of read 2 has %d bytes" % (which, n + 1), text, [len(text)], L))
            out.append(Fixture("long_lines", "line %d of read 2 has %d bytes, cut" % (which, n + 1), text, cut(len(text), 700), L))
    # one offender over two window boundaries and several tiles
    W = 2 * TILE
    t = Text().fill_to(5000).line(b"@r").line(seq_for(0, 30)).line(b"+").line(b"I" * 12000).fill_to(3 * W + 100)
    text = t.bytes()
    lens = cut(len(text), W, 2 * W, 3 * W)
    assert not (as_u8(text)[W:2 * W] == 10).any()
    out.append(Fixture("long_lines", "one line over two boundaries", text, lens, L, W=W))
    # three offenders: the first closes in the last tile of window 0, the others in later windows
    t = Text().fill_to(TILE + 200, step=300)
    first = t.lines // 4
    t.line(b"@r").line(seq_for(first, 30)).line(b"+").line(b"I" * 1500)
    assert TILE < t.n < W
    t.fill_to(W + 300).line(b"@" + b"h" * 1023).line(seq_for(1, 30)).line(b"+").line(b"I" * 30)
    t.fill_to(2 * W + 300).line(b"@r").line(seq_for(2, 1100)).line(b"+").line(b"I" * 30).reads(2)
    text = t.bytes()
    f = Fixture("long_lines", "three offenders", text, cut(len(text), W, 2 * W), L, W=W)
    assert f.expected()[1]["err_rec"] == first
    out.append(f)
    # a window without a '\n' between two others: only the carried line_start shows that the line is too long
    t = Text().fill_to(TILE - 1300)
    r = t.lines // 4
    t.line(b"@r").line(seq_for(r, 30)).line(b"+")
    q0 = t.n
    t.line(b"I" * 1100).reads(3)
    text = t.bytes()
    c0 = q0 + 600
    assert c0 <= TILE
    out.append(Fixture("long_lines", "window without newline", text, cut(len(text), c0, c0 + 300), L))
    # ... and as the last window: line_start at the end
    text = Text().reads(4).bytes() + b"@open line"
    out.append(Fixture("long_lines", "last window without newline", text, cut(len(text), len(text) - 6), L))
    return out


BIG_W = 1027 * TILE
BIG_TILES = (1024, 1025, 1027)


def big_text():
    """three windows of 1024, 1025 and 1027 tiles: lines of 1023 bytes, and 33 lines of 31 bytes in their place in the first tile,
    in tiles 1023 / 1024 / 1025 and in the last tile of every window; every sequence line begins with its read's bases"""
    total = sum(BIG_TILES) * TILE
    special = set()
    t0 = 0
    for nt in BIG_TILES:
        special |= {t0 + x for x in (0, 1023, 1024, 1025, nt - 1) if x < nt}
        t0 += nt
    parts, n, j = [], 0, 0
    while total - n >= 1023:
        if n // TILE in special or (n + 1022) // TILE in special:
            for _ in range(33):
                parts.append((seq_for(j >> 2, 30) if (j & 3) == 1 else b"@" + b"d" * 29) + b"\n")
                j += 1
        else:
            parts.append((seq_for(j >> 2, 1022) if (j & 3) == 1 else b"f" * 1022) + b"\n")
            j += 1
        n += 1023
    parts.append(b"e" * (total - n))
    text = np.frombuffer(b"".join(parts), dtype=np.uint8)
    assert len(text) == total
    return text


def _big():
    return [Fixture("big", "1024, 1025 and 1027 tiles", big_text(), [nt * TILE for nt in BIG_TILES], 26, W=BIG_W)]


_FIXTURES = None


def fixtures():
    global _FIXTURES
    if _FIXTURES is None:
        _FIXTURES = _dna_sweep() + _esc_sweep() + _max_pend() + _zero_last() + _many_windows() + _key_kinds() + _long_lines() + _big()
        assert len({repr(f) for f in _FIXTURES}) == len(_FIXTURES)
    return _FIXTURES


def group(name):
    return [f for f in fixtures() if f.group == name]
