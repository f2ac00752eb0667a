"""A DEFLATE writer driven by tokens, a model of the device's match resolver, and the fixture set both test files of the
inflate share (tests/test_inflate_tokens_host.py on the CPU, tests/test_gpu_inflate.py on the device).

zlib's encoder decides by itself which matches it emits; the resolver (bgzf_resolve_kernel, gpu_frontend.hpp) branches on
things an encoder never lets a caller choose: the alignment of a match's source and destination, the distance against the
length, which matches of a 64-token batch read each other's output.  Here the caller writes the tokens, the stream is plain
RFC 1951, and what it must inflate to is whatever zlib's INFLATE says (`inflate_ref`): expand() is only the cross-check of the
writer.

A token list holds `bytes` (literals) and `(length, distance)` pairs (3..258, 1..32768); `("sym", "L" | "D", n)` writes the
bare code of literal/length or distance symbol n (no extra bits: for the streams that must be declined)."""
import zlib

import numpy as np

# ---- bits ----


class BitWriter:
    """LSB-first bit stream (RFC 1951 3.1.1), flushed to bytes as it grows"""

    def __init__(self):
        self.out = bytearray(); self.acc = 0; self.n = 0

    def put(self, v, w):
        self.acc |= v << self.n; self.n += w
        if self.n >= 64:
            k = self.n >> 3
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k; self.n -= 8 * k

    def align(self):
        if self.n & 7: self.put(0, 8 - (self.n & 7))

    def raw(self, data):
        self.align()
        if self.n:
            self.out += self.acc.to_bytes(self.n >> 3, "little"); self.acc = 0; self.n = 0
        self.out += data

    def bytes(self):
        return bytes(self.out) + self.acc.to_bytes((self.n + 7) >> 3, "little")


def _rev(c, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (c & 1); c >>= 1
    return r


def canonical(lengths):
    """code lengths -> [(code as written: first bit in bit 0, length)] per symbol (RFC 1951 3.2.2); None where the length is 0"""
    cnt = [0] * 16
    for l in lengths: cnt[l] += 1
    cnt[0] = 0
    nxt = [0] * 16; code = 0
    for l in range(1, 16):
        code = (code + cnt[l - 1]) << 1; nxt[l] = code
    out = []
    for l in lengths:
        if l == 0: out.append(None); continue
        out.append((_rev(nxt[l], l), l)); nxt[l] += 1
    return out


def _len_table():
    t = {}
    for ls in range(29):
        if ls < 8: base, extra = 3 + ls, 0
        elif ls == 28: base, extra = 258, 0
        else: extra = (ls - 4) >> 2; base = 3 + ((4 + (ls & 3)) << extra)
        for e in range(1 << extra):
            if base + e <= 258 and base + e not in t or ls == 28: t[base + e] = (257 + ls, e, extra)
    return t


def _dist_table():
    t = [None] * 32769
    for ds in range(30):
        if ds < 4: base, extra = 1 + ds, 0
        else: extra = (ds >> 1) - 1; base = 1 + ((2 + (ds & 1)) << extra)
        for e in range(1 << extra): t[base + e] = (ds, e, extra)
    return t


LEN_SYM, DIST_SYM = _len_table(), _dist_table()
assert LEN_SYM[258] == (285, 0, 0) and LEN_SYM[257] == (284, 30, 5) and LEN_SYM[3] == (257, 0, 0) and LEN_SYM[11] == (265, 0, 1)
assert DIST_SYM[32768] == (29, 8191, 13) and DIST_SYM[1] == (0, 0, 0) and DIST_SYM[5] == (4, 0, 1)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def _symbols(w, tokens, lit_codes, dist_codes):
    put = w.put
    for t in tokens:
        if isinstance(t, (bytes, bytearray)):
            for b in t: put(*lit_codes[b])
        elif t[0] == "sym":
            put(*(lit_codes if t[1] == "L" else dist_codes)[t[2]])
        else:
            length, dist = t
            assert 3 <= length <= 258 and 1 <= dist <= 32768, t
            s, e, eb = LEN_SYM[length]
            put(*lit_codes[s])
            if eb: put(e, eb)
            s, e, eb = DIST_SYM[dist]
            put(*dist_codes[s])
            if eb: put(e, eb)
    put(*lit_codes[256])


_FIXED_CODES = (canonical(FIXED_LIT), canonical(FIXED_DIST))


def fixed_block(tokens, final=True, w=None):
    """one block with the fixed codes (RFC 1951 3.2.6); returns the bytes, or appends to the BitWriter `w` and returns it"""
    own = w is None
    w = w or BitWriter()
    w.put(1 if final else 0, 1); w.put(1, 2)
    _symbols(w, tokens, *_FIXED_CODES)
    return w.bytes() if own else w


def stored_block(data, final, w=None):
    own = w is None
    w = w or BitWriter()
    assert len(data) <= 65535
    w.put(1 if final else 0, 1); w.put(0, 2)
    w.raw(len(data).to_bytes(2, "little") + (len(data) ^ 0xFFFF).to_bytes(2, "little") + bytes(data))
    return w.bytes() if own else w


CLORD = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def dynamic_block(tokens, lit_lengths, dist_lengths, final=True, w=None):
    """one block with the caller's code lengths (257..286 literal/length symbols, 1..30 distance symbols).  The header spells
    every length out with the code-length symbols 0..15, all of them 4 bits long (a complete code; 16..18 are not used)."""
    own = w is None
    w = w or BitWriter()
    assert 257 <= len(lit_lengths) <= 286 and 1 <= len(dist_lengths) <= 30
    w.put(1 if final else 0, 1); w.put(2, 2)
    w.put(len(lit_lengths) - 257, 5); w.put(len(dist_lengths) - 1, 5); w.put(19 - 4, 4)
    for s in CLORD: w.put(4 if s < 16 else 0, 3)
    for l in list(lit_lengths) + list(dist_lengths): w.put(_rev(l, 4), 4)
    _symbols(w, tokens, canonical(lit_lengths), canonical(dist_lengths))
    return w.bytes() if own else w


def complete_lengths(n, order):
    """n code lengths that form a complete code with two 15-bit codes: the chain 1, 2, .., 14, 15, 15, its shortest code split in two
    until there are n.  `order[i]` = the symbol that gets the i-th longest code."""
    ls = list(range(1, 15)) + [15, 15]
    assert n >= len(ls)
    while len(ls) < n:
        ls.sort(); l = ls.pop(0); ls += [l + 1, l + 1]
    ls.sort(reverse=True)
    assert sum(1 << (15 - l) for l in ls) == 1 << 15 and ls[0] == 15
    out = [0] * n
    for l, s in zip(ls, order): out[s] = l
    return out


def expand(tokens):
    """LZ77 by its definition, a byte at a time"""
    out = bytearray()
    for t in tokens:
        if isinstance(t, (bytes, bytearray)): out += t
        else:
            length, dist = t
            assert 1 <= dist <= len(out), (t, len(out))
            for _ in range(length): out.append(out[-dist])
    return bytes(out)


def inflate_ref(stream):
    """the expected output of every test: zlib's INFLATE of the raw stream"""
    d = zlib.decompressobj(-15)
    out = d.decompress(stream)
    assert d.eof and not d.unused_data
    return out


def zlib_declines(stream, isize):
    """zlib rejects the stream (an error, a stream that does not end) or inflates it to another length than the block claims"""
    try:
        return len(zlib.decompress(stream, -15)) != isize
    except zlib.error:
        return True


# ---- the resolver's schedule, restated ----
TOK_SKIP = 1 << 15
DEFECTS = ("no_deps", "plain_overlap", "no_rotate3", "lit8_skip", "batch_pos", "deps_len")


def token_cap(isize):
    return isize // 3 + isize // 256 + 4


def place(tokens_u32, defect=None):
    """the placement of bgzf_resolve_kernel: per batch of 64 tokens the lanes' (lit, len, dist, dst, src) as int64 arrays
    (len 0: a step-over, or a lane past the last token)"""
    tk = np.asarray(tokens_u32, dtype=np.int64)
    pos = 0
    for t0 in range(0, len(tk), 64):
        t = np.full(64, TOK_SKIP, dtype=np.int64); t[:len(tk) - t0] = tk[t0:t0 + 64]
        skip = (t & TOK_SKIP) != 0
        lit = np.where(skip, t >> (24 if defect == "lit8_skip" else 16), t >> 24)
        ln = np.where(skip, 0, ((t >> 16) & 255) + 3)
        dist = (t & 0x7FFF) + 1
        dend = pos + np.cumsum(lit + ln)
        dst = dend - ln
        pos = pos + int(lit[63] + ln[63]) if defect == "batch_pos" else int(dend[63])
        yield lit, ln, dist, dst, dst - dist


def batch_deps(ln, dist, dst, src, defect=None):
    """deps[i, j]: lane i reads what lane j (< i, a match) writes"""
    rd_end = src + (dist if defect == "deps_len" else np.minimum(ln, dist))
    dend = dst + ln
    deps = (dend[None, :] > src[:, None]) & (dst[None, :] < rd_end[:, None]) & (ln[None, :] != 0)
    deps &= np.tri(64, 64, -1, dtype=bool)
    if defect == "no_deps": deps[:] = False
    return deps


def rounds(ln, deps):
    """the lanes that copy in each round of a batch"""
    pending = ln != 0
    while pending.any():
        ready = pending & ~(deps & pending[None, :]).any(axis=1)
        assert ready.any()
        yield np.flatnonzero(ready)
        pending &= ~ready


def resolve_batched(out, tokens_u32, defect=None):
    """What the kernel computes, by its own schedule: `out` holds the literals (phase 1), the result is the inflated block.
    Every lane that is ready in a round reads the buffer as it stood when the round began; a lane with dist < len repeats its
    first `dist` bytes.  `defect` turns one rule into a wrong one (DEFECTS; "deps_len" is wrong only in being cautious)."""
    buf = bytearray(out)
    n = len(buf)
    for lit, ln, dist, dst, src in place(tokens_u32, defect):
        deps = batch_deps(ln, dist, dst, src, defect)
        for lanes in rounds(ln, deps):
            writes = []
            for i in lanes:
                s, d, l, k = int(src[i]), int(dst[i]), int(ln[i]), int(dist[i])
                if s < 0 or d + l > n:                                 # (only a defective placement gets here)
                    writes.append((min(d, n), b"")); continue
                if k >= l or defect == "plain_overlap": data = bytes(buf[s:s + l])
                else:
                    pat = bytes(buf[s:s + k])
                    if k == 3 and defect == "no_rotate3": data = (((pat * 6)[:16]) * (l // 16 + 1))[:l]
                    else: data = (pat * (l // k + 1))[:l]
                writes.append((d, data))
            for d, data in writes: buf[d:d + len(data)] = data
    return bytes(buf[:n])


# ---- fixtures ----
GRID_LENS = tuple(range(3, 21)) + (31, 32, 33, 47, 48, 49, 255, 256, 257, 258)
SHORT_LENS = tuple(range(3, 51)) + (255, 256, 257, 258)
LONG_DISTS = (4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 257)


class _Tok:
    """a token list under construction that knows its output position"""

    def __init__(self, rng):
        self.rng = rng; self.t = []; self.pos = 0

    def lits(self, n):
        """n bytes of which no two within a distance of 2 are equal (a repeated pattern of 1..3 bytes never looks rotated right by chance)"""
        if n == 0: return self
        b = bytearray(self.rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        prev = self.t[-1][-2:] if self.t and isinstance(self.t[-1], bytes) else b""
        h = bytearray(prev) + b
        for i in range(len(prev), len(h)):
            while (i >= 1 and h[i] == h[i - 1]) or (i >= 2 and h[i] == h[i - 2]): h[i] = (h[i] + 1) & 255
        b = bytes(h[len(prev):])
        if self.t and isinstance(self.t[-1], bytes): self.t[-1] += b
        else: self.t.append(b)
        self.pos += n
        return self

    def match(self, length, dist):
        assert 1 <= dist <= self.pos and 3 <= length <= 258, (length, dist, self.pos)
        self.t.append((length, dist)); self.pos += length
        return self

    def to_phase(self, phase, at_least=0):
        """literals until pos & 3 == phase (at least `at_least` of them)"""
        return self.lits(at_least + ((phase - self.pos - at_least) & 3))


def _grid(rng, far):
    """mode 0 at every (src & 3, dst & 3, length): the source right behind the output (it reads the match before: chains) or,
    `far`, in the literals at the block's head"""
    k = _Tok(rng).lits(300 if far else 64)
    for length in GRID_LENS:
        for sp in range(4):
            for dp in range(4):
                k.to_phase(dp, at_least=int(rng.integers(0, 2)))
                if far:
                    src = int(rng.integers(0, 8)) * 4 + sp
                    k.match(length, k.pos - src)
                else:
                    k.match(length, length + ((k.pos - sp - length) & 3))
                assert (k.pos - length) & 3 == dp and (k.pos - length - k.t[-1][1]) & 3 == sp and k.t[-1][1] >= length
    return k.t


def _short_overlap(rng):
    k = _Tok(rng)
    for dist in (1, 2, 3):
        for length in SHORT_LENS:
            if length <= dist: continue
            for dp in range(4):
                k.to_phase(dp, at_least=3).match(length, dist)
    return k.t


def _long_overlap(rng, dp):
    """mode 2 beside mode 1 and mode 0 matches that copy in the same round"""
    k = _Tok(rng).lits(40)
    for dist in LONG_DISTS:
        for length in sorted({dist + 1, min(2 * dist, 258), 258}):
            if length <= dist: continue
            k.to_phase(dp, at_least=dist).match(length, dist)
            k.lits(int(rng.integers(3, 7))).match(int(rng.integers(4, 40)), int(rng.integers(1, 4)))
            k.lits(int(rng.integers(0, 4))); k.match(int(rng.integers(3, 20)), k.pos - int(rng.integers(0, 20)))   # (from the head's literals)
    return k.t


def _chain(rng, n, overlap=None):
    """n matches of which each reads the output of the one before.  overlap: None = plain copies, True = every link repeats
    (dist < len), "mix" = both"""
    k = _Tok(rng).lits(12).match(9, 4 if overlap is True else 11)
    prev = 9
    for i in range(n - 1):
        lit = int(rng.integers(0, 3)) if i % 5 == 4 else 0
        k.lits(lit)
        ov = overlap is True or (overlap == "mix" and rng.random() < 0.5)
        if ov:
            dist = lit + int(rng.integers(1, min(prev, 9) + 1))
            length = max(3, dist + int(rng.integers(1, 21)))
        else:
            dist = lit + int(rng.integers(3, prev + 1))
            length = int(rng.integers(3, min(dist, 12) + 1))
        k.match(length, dist); prev = length
    return k.t


def _fan_out(rng):
    k = _Tok(rng).lits(200).match(258, 199)
    a0 = k.pos - 258
    for _ in range(63):
        k.lits(int(rng.integers(0, 3)))
        length = int(rng.integers(3, 12))
        k.match(length, k.pos - (a0 + int(rng.integers(0, 258 - length + 1))))
    return k.t


def _straddle(rng):
    k = _Tok(rng).lits(100)
    for _ in range(5): k.lits(2).match(5, 60)
    x = k.pos; k.match(6, 70).lits(3).match(6, 50).lits(2)
    k.match(10, k.pos - (x + 2))                                       # 4 bytes of the first, the 3 literals, 3 bytes of the second
    for _ in range(4): k.lits(1).match(4, 80)
    return k.t


def _n_tokens(rng, n, head=60, tail=5):
    k = _Tok(rng).lits(head)
    for _ in range(n): k.lits(int(rng.integers(0, 4))).match(int(rng.integers(3, 9)), int(rng.integers(20, head)))
    return k.lits(tail).t


def _random_tokens(rng, n, max_dist=32768):
    k = _Tok(rng).lits(5)
    for _ in range(n):
        k.lits(int(rng.integers(0, 6)))
        k.match(int(rng.integers(3, 259)) if rng.random() < 0.3 else int(rng.integers(3, 12)), int(rng.integers(1, min(k.pos, max_dist) + 1)))
    return k.lits(int(rng.integers(0, 4))).t


def resolver_fixtures(rng):
    """[(name, raw DEFLATE stream, inflated length)]: every stream well-formed, every block at most 65 536 bytes.
    What the format rules out inside 65 536 bytes, and what stands in for it: a literal run of 65 535 or 65 536 in front of a
    match (the longest that fits is 65 533 in front of a match of 3: `lit65533`; the step-over of 65 535 comes from
    `stored65535+1`), and a whole batch of 64 step-overs (a step-over needs 256 literals and a match behind it, or 60 001
    stored bytes: `stepover_batch` has a batch that holds nothing but one)."""
    fx = []

    def add(name, stream, tokens=None):
        exp = inflate_ref(stream)
        if tokens is not None: assert exp == expand(tokens), name
        assert len(exp) <= 65536, name
        fx.append((name, stream, len(exp)))

    def fixed(name, tokens): add(name, fixed_block(tokens), tokens)

    fixed("grid/near", _grid(rng, False))
    fixed("grid/far", _grid(rng, True))
    fixed("short_overlap", _short_overlap(rng))
    for dp in range(4): fixed("long_overlap/dst%d" % dp, _long_overlap(rng, dp))
    fixed("chain/64", _chain(rng, 64))
    fixed("chain/200", _chain(rng, 200))
    fixed("chain/overlap64", _chain(rng, 64, True))
    fixed("chain/mixed130", _chain(rng, 130, "mix"))
    fixed("chain/fan_out", _fan_out(rng))
    fixed("chain/straddle", _straddle(rng))
    for n in (0, 1, 63, 64, 65, 128, 129): fixed("tokens/%d" % n, _n_tokens(rng, n))
    # step-overs: in lane 0 (a long literal run opens the block), in lane 63, in lane 0 of the second batch, alone in the last batch
    fixed("stepover/lane0", _Tok(rng).lits(300).match(7, 33).lits(4).match(5, 9).t)
    k = _Tok(rng).lits(50)
    for _ in range(63): k.lits(1).match(4, 30)
    fixed("stepover/lane63", k.lits(256).match(6, 400).lits(3).match(3, 2).t)
    k = _Tok(rng).lits(50)
    for _ in range(64): k.lits(2).match(5, 40)
    fixed("stepover/lane64", k.lits(777).match(9, 1000).lits(3).match(8, 3).t)
    k = _Tok(rng).lits(50)
    for _ in range(64): k.lits(1).match(3, 25)
    w = fixed_block(k.t, final=False, w=BitWriter())
    tail = rng.integers(0, 256, 60001, dtype=np.uint8).tobytes()
    add("stepover_batch", stored_block(tail, True, w).bytes(), k.t + [tail])
    for n in (254, 255, 256, 257, 511, 512):
        fixed("lit%d" % n, _Tok(rng).lits(n).match(5, n).lits(2).match(4, 7).t)
    fixed("lit65533", _Tok(rng).lits(65533).match(3, 65533 - 32765).t)
    fixed("lit65536", _Tok(rng).lits(65536).t)
    big = rng.integers(0, 256, 65536, dtype=np.uint8).tobytes()
    add("stored65535+1", stored_block(big[65535:], True, stored_block(big[:65535], False, BitWriter())).bytes())
    # 60 001 stored bytes (a step-over with no match of its own), then matches
    w = stored_block(big[:60001], False, BitWriter())
    t = [(258, 32768), b"xy", (30, 32767), (4, 1), b"q", (100, 29000)]
    add("stored60001+match", fixed_block(t, True, w).bytes(), [big[:60001]] + t)
    # the token cap: 4 literals and 21 844 matches of 3 are 65 536 bytes
    k = _Tok(rng).lits(4)
    ds = (3, 4, 7, 3, 12, 100, 1000, 5, 3, 31000)
    for i in range(21844): k.match(3, next(d for d in (ds[i % 10], 4, 3) if d <= k.pos))
    assert k.pos == 65536
    fixed("token_cap", k.t)
    for n in (0, 1, 2, 3): fixed("isize%d" % n, _Tok(rng).lits(n).t)
    # distance limits: a source at byte 0, the longest distance the format has, a match that ends the block
    w = stored_block(big[:32768], False, BitWriter())
    k = _Tok(rng); k.pos = 32768
    k.match(3, 32768).match(258, 32768)
    for d in (32506, 32507, 32767, 32768):
        for length in (3, 258): k.lits(int(rng.integers(0, 4))).match(length, d)
    k.lits(5).match(258, 32768)
    add("dist_limits", fixed_block(k.t, True, w).bytes(), [big[:32768]] + k.t)
    # phase 1: dynamic blocks whose codes reach 15 bits, the one incomplete code zlib takes, several blocks in a stream
    t = _random_tokens(rng, 300)
    lit_a = complete_lengths(286, [97, 257, 0, 285] + [s for s in rng.permutation(286) if s not in (97, 257, 0, 285)])
    dist_a = complete_lengths(30, [0, 29] + [s for s in rng.permutation(30) if s not in (0, 29)])
    t = [b"a\x00a", (3, 2), (258, 1), (4, 1)] + t
    add("dyn15/a", dynamic_block(t, lit_a, dist_a), t)
    t = _random_tokens(rng, 500, max_dist=600)
    lit_b = complete_lengths(286, list(rng.permutation(286)))
    dist_b = complete_lengths(30, list(range(30)))
    add("dyn15/b", dynamic_block(t, lit_b, dist_b), t)
    t = _Tok(rng).lits(9).match(5, 1).lits(3).match(258, 1).lits(1).match(3, 1).lits(2).t
    add("dyn_one_dist", dynamic_block(t, complete_lengths(286, list(range(286))), [1]), t)
    t1, t2 = _random_tokens(rng, 40), _random_tokens(rng, 80, max_dist=100)
    mid = rng.integers(0, 256, 700, dtype=np.uint8).tobytes()
    w = fixed_block(t1, False, BitWriter()); stored_block(mid, False, w); dynamic_block([b"zz"], lit_b, dist_b, False, w)
    stored_block(b"", False, w)
    # (the second token list stands alone: its distances stay inside its own bytes)
    add("multi_block", fixed_block(t2, True, w).bytes())
    for i in range(4): fixed("random/%d" % i, _random_tokens(rng, 150 + 100 * i, max_dist=(40, 700, 5000, 32768)[i]))
    assert len({n for n, _, _ in fx}) == len(fx)
    return fx


def declined_fixtures():
    """[(name, stream, isize)]: well-formed up to the point where zlib itself gives up (zlib_declines)"""
    ok = fixed_block([b"abcdefgh", (5, 3), b"xyz", (4, 11)])
    return [
        ("decline/dist_too_far", fixed_block([b"ab", (3, 3), b"cdef"]), 9),
        ("decline/overrun", fixed_block([b"abcd", (10, 4)]), 10),
        ("decline/length_sym_286", fixed_block([b"abc", ("sym", "L", 286), ("sym", "D", 0), b"d"]), 8),
        ("decline/dist_sym_30", fixed_block([b"abc", ("sym", "L", 257), ("sym", "D", 30), b"d"]), 7),
        ("decline/one_byte_short", ok[:-1], 20),
    ]


def layout(entries, phase0=0, gap=24):
    """uoff per block: ascending, `gap`..`gap`+6 guard bytes between neighbours, block i at uoff & 3 == (phase0 + i) & 3;
    returns (uoffs, end) with `gap` guard bytes behind the last block"""
    uoffs = []; at = gap
    for i, (_, _, n) in enumerate(entries):
        at = ((at + 3) & ~3) + ((phase0 + i) & 3)
        uoffs.append(at); at += n + gap
    return uoffs, at


def device_order(fx):
    """the blocks of one launch: a first wave of phase 1 with one 65 536-byte block beside 63 blocks of 0..3 bytes, then every
    fixture four times (with layout(): at the four values of uoff & 3, the period being odd)"""
    by = {n: e for e in fx for n in [e[0]]}
    order = [by["lit65536"]] + [by["isize%d" % (i & 3)] for i in range(63)]
    rest = list(fx) if len(fx) % 2 == 0 else list(fx) + [by["isize1"]]
    for r in range(4): order += rest + [by["isize2"]]
    return order
