"""filter's device windows (csrc/filter_kernels.hpp and the count / scan kernels it borrows from fastq_kernels.hpp) driven through
the handle API fastf_fltdev_create / set_whitelist / reset / parse / decide / emit / end with hand-built FASTQ text, window by
window, against tests/fltwin_ref.py (proved against filter_ref.py_filter in tests/test_fltwin_ref_host.py).  No subprocess, no gzip,
no host window loop, no oracle binaries: the staging is built here as filter_cmds.c builds it (FLT_HDR bytes of what preceded, the
window, 64 zero bytes; a '\\n' at tv when the last line is open), and the window lengths are whatever a case asks for.

Before every pass the device buffer is poisoned: one window of W newlines goes through parse, then reset.  Every byte of the
buffer behind a later, shorter window is then a stale newline, and a count that reads past `len` shows as extra lines.

Everything compared is integers and bytes; every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from fastf_amd import _lib

import fltwin_ref as W

pytestmark = pytest.mark.gpu

HDR, NONE = W.FLT_HDR, W.NONE


class Esc(C.Structure):
    _fields_ = [("i", C.c_uint32), ("s1", C.c_uint32)]


def api():
    L = _lib.lib()
    vp, u64, u32, sz = C.c_void_p, C.c_uint64, C.c_uint32, C.c_size_t
    L.fastf_fltdev_create.argtypes = [C.c_int, sz, C.POINTER(vp)]
    L.fastf_fltdev_destroy.argtypes = [vp]
    L.fastf_fltdev_destroy.restype = None
    L.fastf_fltdev_set_whitelist.argtypes = [vp, vp, sz]
    L.fastf_fltdev_reset.argtypes = [vp]
    L.fastf_fltdev_parse.argtypes = [vp, vp, sz, u64, u64, u64, C.POINTER(u64), C.POINTER(u64)]
    L.fastf_fltdev_decide.argtypes = [vp, C.c_int, C.c_int, u32, C.c_float, vp, C.POINTER(C.POINTER(Esc)), C.POINTER(u32)]
    L.fastf_fltdev_emit.argtypes = [vp, vp, u32, C.POINTER(vp), C.POINTER(sz)]
    L.fastf_fltdev_end.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u32), C.POINTER(u64), C.POINTER(C.c_double)]
    return L


def random_states(r_lo, n_rec):
    """chunk start states of a window: arbitrary words, a function of where the window's reads begin"""
    return np.random.default_rng(1000 + r_lo).integers(0, 1 << 32, size=((n_rec + W.CHUNK - 1) // W.CHUNK, W.DEG), dtype=np.uint32)


class Dev:
    """one handle of window size Wb, its pinned staging, and the keep bitmap its mode-0 passes have left on the device"""

    def __init__(self, Wb):
        self.L, self.Wb = api(), Wb
        self.h = C.c_void_p()
        _lib.check(self.L.fastf_fltdev_create(0, Wb, C.byref(self.h)))
        self.n_stage = HDR + Wb + 128
        self.n_cs = ((Wb + 1) // 4 + 2 + W.CHUNK - 1) // W.CHUNK * W.DEG
        self.p_stage = self.L.fastf_pinned_alloc(self.n_stage)
        self.p_cs = self.L.fastf_pinned_alloc(self.n_cs * 4)
        assert self.p_stage and self.p_cs
        self.stage = np.ctypeslib.as_array(C.cast(self.p_stage, C.POINTER(C.c_uint8)), shape=(self.n_stage,))
        self.cs = np.ctypeslib.as_array(C.cast(self.p_cs, C.POINTER(C.c_uint32)), shape=(self.n_cs,))
        self.bitmap = np.zeros(0, dtype=bool)
        self.wl = None

    def close(self):
        self.L.fastf_fltdev_destroy(self.h)
        self.L.fastf_pinned_free(self.p_stage)
        self.L.fastf_pinned_free(self.p_cs)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_whitelist(self, keys):
        self.wl = np.ascontiguousarray(sorted(int(k) for k in keys), dtype=np.uint64)
        _lib.check(self.L.fastf_fltdev_set_whitelist(self.h, self.wl.ctypes.data_as(C.c_void_p) if len(self.wl) else None, len(self.wl)))

    def parse(self, ln, a, tv, limit):
        r_lo, n_rec = C.c_uint64(), C.c_uint64()
        _lib.check(self.L.fastf_fltdev_parse(self.h, self.p_stage, ln, a, tv, limit, C.byref(r_lo), C.byref(n_rec)))
        return r_lo.value, n_rec.value

    def poison(self):
        self.stage[:HDR] = 0
        self.stage[HDR:HDR + self.Wb] = 10
        self.parse(self.Wb, 0, NONE, NONE)
        _lib.check(self.L.fastf_fltdev_reset(self.h))

    def feed(self, text, wins, mode, all_cells=True, L=16, rate=2.0, states_fn=random_states, hits_fn=None, limit=NONE):
        """one file: text (bytes or uint8 array) through the windows [(a, len, tv, ...)] -> (per window dict(r_lo, n_rec, out,
        total, esc), end dict)"""
        t = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
        self.poison()
        st, res = self.stage, []
        for k, win in enumerate(wins):
            a, ln, tv = win[:3]
            n = ln - (tv != NONE)
            assert a + n <= len(t) and ln <= self.Wb + 1
            h = min(a, HDR)
            st[:HDR - h] = 0
            st[HDR - h:HDR] = t[a - h:a]
            st[HDR:HDR + n] = t[a:a + n]
            if tv != NONE:
                assert tv == a + n
                st[HDR + n] = 10
            st[HDR + ln:HDR + ln + 64] = 0
            r_lo, n_rec = self.parse(ln, a, tv, limit)
            if mode == 0 and n_rec:
                s = np.ascontiguousarray(states_fn(r_lo, n_rec), dtype=np.uint32).reshape(-1)
                assert len(s) == (n_rec + W.CHUNK - 1) // W.CHUNK * W.DEG <= self.n_cs
                self.cs[:len(s)] = s
            pe, ne = C.POINTER(Esc)(), C.c_uint32()
            _lib.check(self.L.fastf_fltdev_decide(self.h, mode, int(all_cells), L, rate, self.p_cs, C.byref(pe), C.byref(ne)))
            esc = sorted((pe[q].i, pe[q].s1) for q in range(ne.value))      # copied at once: valid until the next call
            hits = np.ascontiguousarray(hits_fn(k, esc, n_rec) if hits_fn else [], dtype=np.uint32)
            po, tot = C.c_void_p(), C.c_size_t()
            _lib.check(self.L.fastf_fltdev_emit(self.h, hits.ctypes.data_as(C.c_void_p) if len(hits) else None, len(hits),
                                                C.byref(po), C.byref(tot)))
            out = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint8)), shape=(tot.value,)).copy() if tot.value else np.zeros(0, np.uint8)
            res.append(dict(r_lo=r_lo, n_rec=n_rec, out=out, total=tot.value, esc=esc))
        n_nl, kept, err, err_rec = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint64()
        _lib.check(self.L.fastf_fltdev_end(self.h, C.byref(n_nl), C.byref(kept), C.byref(err), C.byref(err_rec), None))
        return res, dict(n_nl=n_nl.value, kept=kept.value, err=err.value, err_rec=err_rec.value)

    def note_kept(self, keep):
        if len(keep) > len(self.bitmap):
            self.bitmap = np.concatenate([self.bitmap, np.zeros(len(keep) - len(self.bitmap), dtype=bool)])
        self.bitmap[:len(keep)] |= keep


def check(dev, text, lens, mode=0, all_cells=True, L=16, rate=2.0, states_fn=random_states, judge=None, limit=NONE, bogus_hits=False,
          tag=""):
    """one pass of `text` through the windows `lens` on the device against the reference, window by window; returns the reference's
    (windows, end, keep)"""
    fr = W.Framing(text)
    wins = fr.windows(lens)
    draws = np.zeros(fr.n_reads, dtype=np.uint32)
    if mode == 0:
        for a, ln, tv, r_lo, n_rec in wins:
            if n_rec:
                draws[r_lo:r_lo + n_rec] = W.chunk_draws(states_fn(r_lo, n_rec), n_rec)
    want, end, keep = W.run(fr, lens, mode, all_cells, L, rate, draws, dev.wl if dev.wl is not None else (), judge, dev.bitmap, limit)

    def hits_fn(k, esc, n_rec):
        return [i for i, _ in esc if i in want[k]["esc_keep"]] + ([n_rec, n_rec + 1] if bogus_hits else [])
    got, gend = dev.feed(text, wins, mode, all_cells, L, rate, states_fn, hits_fn, limit)
    for k, (g, w) in enumerate(zip(got, want)):
        where = "%s window %d of %d (a=%d len=%d)" % (tag, k, len(want), w["a"], w["len"])
        assert (g["r_lo"], g["n_rec"]) == (w["r_lo"], w["n_rec"]), where
        assert g["esc"] == sorted(w["esc"]), where
        assert g["total"] == w["total"], where
        assert g["out"].tobytes() == w["out"], where
    assert gend == end, tag
    if mode == 0:
        dev.note_kept(keep)
    return want, end, keep


def fastq(reads):
    """reads: [(id, seq, plus, qual)] line bodies -> text, every line closed"""
    return b"".join(b"".join(ln + b"\n" for ln in r) for r in reads)


def letters(rng, n, alphabet=b"ACGTNacgt@+#IJF!~ \r\t"):
    return bytes(np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), size=n)])


# ---------------------------------------------------------------- 1. every split position
def split_text():
    """40 reads, line bodies of 0, 1, 15, 16, 17, 255 and 1022 bytes, the last line open; about 4.4 KiB"""
    rng = np.random.default_rng(7)
    sizes = [0, 1, 15, 16, 17] * 30 + [255] * 7 + [1022, 1, 17]
    order = rng.permutation(len(sizes))
    bodies = [letters(rng, sizes[k]) for k in order]
    assert len(bodies) == 160
    text = b"".join(b + b"\n" for b in bodies)[:-1]
    assert 4096 + 300 < len(text) < 5200 and not text.endswith(b"\n")
    return text


SPLIT_TEXT = split_text()


def ones(n):
    return [1] * n


def _aligned(n):
    fr = W.Framing(SPLIT_TEXT)
    cut = int(fr.last[19]) + 1                                # a window that ends on the last newline of read 19
    return [cut, n - cut]


SPLITS = {
    "all 1": ones,
    "all 16": lambda n: [16] * (n // 16) + [n % 16],
    "all 17": lambda n: [17] * (n // 17) + [n % 17],
    "4095 then 1s": lambda n: [4095] + [1] * (n - 4095),
    "4096, rest": lambda n: [4096, n - 4096],
    "1, 4096, rest": lambda n: [1, 4096, n - 4097],
    "zeros": lambda n: [0, 0, 100, 0, 1000, 0, 0, 2996, 0, n - 4096, 0],
    "read-aligned": _aligned,
}
# the list of the mode-1 pass that follows each mode-0 list
SECOND = {"all 1": "all 17", "all 16": "zeros", "all 17": "1, 4096, rest", "4095 then 1s": "all 16", "4096, rest": "all 1",
          "1, 4096, rest": "4095 then 1s", "zeros": "read-aligned", "read-aligned": "4096, rest"}


@pytest.mark.parametrize("first", sorted(SPLITS))
def test_every_split_position(first):
    text, n = SPLIT_TEXT, len(SPLIT_TEXT)
    with Dev(4096) as dev:
        # R1, all cells, every draw passes; then a second file of the same text through other windows against the bitmap
        w0, end0, keep = check(dev, text, SPLITS[first](n), mode=0, all_cells=True, rate=2.0, tag=first)
        assert keep.all() and end0 == dict(n_nl=160, kept=40, err=0, err_rec=NONE)
        check(dev, text, SPLITS[SECOND[first]](n), mode=1, tag=first + " / mode 1 " + SECOND[first])
    with Dev(4096) as dev:
        # the same with draws that drop about half of the reads, so that the bitmap is not all ones (the 1-byte windows, 3 calls per
        # byte, are not fed twice)
        a, b = ("all 17" if first == "all 1" else first), ("zeros" if SECOND[first] == "all 1" else SECOND[first])
        _, _, keep = check(dev, text, SPLITS[a](n), mode=0, all_cells=True, rate=0.5, tag=a + " rate 0.5")
        assert 8 < keep.sum() < 32
        w1, end1, _ = check(dev, text, SPLITS[b](n), mode=1, tag=a + " rate 0.5 / mode 1 " + b)
        assert end1["kept"] == 0 and sum(w["total"] for w in w1) > 0


# ---------------------------------------------------------------- 2. tile, wave and lane edges in one window
EDGES = (0, 15, 16, 1023, 1024, 4095, 4096, 8191, 8192)


def edge_text(n, skip_tile):
    """n bytes with '\\n' exactly at the EDGES below n and at n - 1, and enough others that no line is too long; skip_tile: no
    newline at all inside tile 1 (bytes 4097 .. 8190 — its neighbours end at 4096 and begin at 8191)"""
    rng = np.random.default_rng(n)
    t = np.frombuffer(letters(rng, n, b"ACGTN@+IF"), dtype=np.uint8).copy()
    at = sorted({o for o in EDGES if o < n} | {n - 1})
    fill, prev = [], -1
    for o in at + [n]:
        while o - prev > 1000:
            prev += 1000 - int(rng.integers(0, 7))
            if not (skip_tile and 4096 < prev < 8191):
                fill.append(prev)
        prev = o
    t[at + fill] = 10
    assert (t[list(EDGES[:sum(o < n for o in EDGES)])] == 10).all() and t[n - 1] == 10
    if skip_tile and n > 8191:
        assert not (t[4097:8191] == 10).any()
    return t.tobytes()


@pytest.mark.parametrize("skip_tile", [False, True], ids=["every tile", "tile 1 empty"])
def test_tile_wave_and_lane_edges(skip_tile):
    with Dev(16384) as dev:
        for k in (1, 2, 3, 4):
            for d in (0, -1, 1, 15, 16):
                n = 4096 * k + d
                if n > 16384 or (skip_tile and n <= 8192):
                    continue
                text = edge_text(n, skip_tile)
                _, end, _ = check(dev, text, [n], mode=0, all_cells=True, rate=2.0, tag="len %d" % n)
                assert (end["err"] == 1) == skip_tile        # a tile without a newline lies inside a line of 4 KiB
                # the same bytes with the last line open: the virtual newline is the window's last byte
                check(dev, text[:-1], [n - 1], mode=0, all_cells=True, rate=2.0, tag="len %d open" % n)


# ---------------------------------------------------------------- 3. the largest legal read
def test_largest_legal_read():
    rng = np.random.default_rng(3)
    big = [letters(rng, 1022, b"ACGTNIF#") for _ in range(4)]
    short = (b"@", b"", b"", b"")
    text = fastq([short, big, (b"@t", b"ACGT", b"+", b"IIII")])
    assert len(fastq([short])) == 5 and len(fastq([big])) == 4092 and text[4096:4097] == b"\n"
    with Dev(4096) as dev:
        # its last newline is byte 0 of the second window: the read begins at buffer offset 5
        w, end, keep = check(dev, text, [4096, len(text) - 4096], tag="closed")
        assert end["err"] == 0 and end["err_rec"] == NONE and keep.all() and w[1]["r_lo"] == 1 and w[1]["n_rec"] == 2
        check(dev, text, [4096, 1, len(text) - 4097], mode=1, tag="closed / mode 1")
    big[3] = letters(rng, 1023, b"IF#")                      # 1023 bytes and no newline: gzgets hands back 1023
    text = fastq([short]) + b"".join(b + b"\n" for b in big)[:-1]
    assert len(text) == 5 + 4092
    with Dev(4096) as dev:
        w, end, keep = check(dev, text, [4096, 1, 0], tag="open")
        assert end["err"] == 0 and end["err_rec"] == NONE and keep.all() and end["n_nl"] == 8
        assert (w[2]["len"], w[2]["tv"], w[2]["n_rec"], w[2]["total"]) == (1, len(text), 1, 3 * 1023 + 2)
        check(dev, text, [4096, 1, 0], mode=1, tag="open / mode 1")


# ---------------------------------------------------------------- 4. line-length refusals
def plain_reads(rng, n):
    return [[b"@r%d" % i, letters(rng, 20, b"ACGT"), b"+", letters(rng, 20, b"IF")] for i in range(n)]


def test_line_length_refusals():
    rng = np.random.default_rng(4)
    reads = plain_reads(rng, 10)
    reads[5][1] = letters(rng, 1023, b"ACGT")                # 1023 bytes and a newline: gzgets hands back 1024
    reads[9][3] = letters(rng, 1024, b"IF")                  # the open last line: 1024 bytes
    both = fastq(reads)[:-1]
    reads[5][1] = letters(rng, 1022, b"ACGT")
    only9 = fastq(reads)[:-1]
    lens_of = lambda t: [4096] * (len(t) // 4096) + [len(t) % 4096]  # noqa: E731
    with Dev(4096) as dev:
        _, end, keep = check(dev, both, lens_of(both), tag="reads 5 and 9")
        assert end["err"] == 1 and end["err_rec"] == 5 and keep.all()
        for limit, first in ((5, NONE), (6, 5), (9, 5), (10, 5)):
            _, end, _ = check(dev, both, lens_of(both), mode=1, limit=limit, tag="limit %d" % limit)
            assert (end["err"], end["err_rec"]) == ((1, first) if first != NONE else (0, NONE))
        _, end, _ = check(dev, only9, [1000] * (len(only9) // 1000) + [len(only9) % 1000], tag="read 9")
        assert end["err"] == 1 and end["err_rec"] == 9
        for limit, first in ((9, NONE), (10, 9)):
            _, end, _ = check(dev, only9, lens_of(only9), mode=1, limit=limit, tag="read 9, limit %d" % limit)
            assert (end["err"], end["err_rec"]) == ((1, first) if first != NONE else (0, NONE))


def test_read_that_begins_before_the_buffer():
    rng = np.random.default_rng(5)
    reads = plain_reads(rng, 8)
    reads[3][1] = letters(rng, 5000, b"ACGT")
    text = fastq(reads)
    fr = W.Framing(text)
    with Dev(4096) as dev:
        # windows of 4096: read 3 ends in the window at 4096 and begins at its buffer's front: too long, yet whole
        w, end, keep = check(dev, text, [4096, len(text) - 4096], tag="whole")
        assert end["err"] == 1 and end["err_rec"] == 3 and keep.all()
        # its last newline in a window that begins 5096 bytes into the file: the read begins before that window's buffer
        lens = [4096, 1000, len(text) - 5096]
        assert 5096 - HDR > fr.start[12] and fr.last[3] >= 5096
        w, end, keep = check(dev, text, lens, tag="cut")
        assert end["err"] == 3 and end["err_rec"] == 3 and end["kept"] == 7 and not keep[3] and keep.sum() == 7
        assert w[2]["r_lo"] == 3 and w[2]["n_rec"] == 5 and w[2]["out"] == b"".join(fr.out(r) for r in range(4, 8))
        w, end, _ = check(dev, text, [4096, 1000, 100, len(text) - 5196], mode=1, tag="cut / mode 1")
        assert end["err"] == 3 and end["err_rec"] == 3
        # beyond the limit nothing of it is looked at
        _, end, _ = check(dev, text, lens, mode=1, limit=3, tag="cut, limit 3")
        assert end["err"] == 0 and end["err_rec"] == NONE


# ---------------------------------------------------------------- 5. whitelist lookup
def bases(key, L):
    return bytes(b"ACGT"[(key >> (2 * (L - 1 - i))) & 3] for i in range(L))


def whitelist(L, n_wl, rng):
    if L == 0:
        return [W.DNA_TAG][:n_wl]
    if L > W.MAX_DNA:
        return []
    space = 1 << (2 * L)
    vals = set()
    while len(vals) < min(n_wl, space - 2):
        vals.add(int(rng.integers(1, space - 1)))            # (AAA.. and TTT.. stay unlisted: probes below and above)
    return sorted(W.DNA_TAG | v for v in vals)


def probe_lines(L, keys, rng):
    """sequence line bodies around the listed keys and around the forms that are no key"""
    Lb = min(L, 40)
    seqs = [b"A" * Lb, b"T" * Lb, b"A" * Lb + b"CGT", b""]
    for k in ([keys[0], keys[-1]] if keys else []) + [keys[int(i)] for i in rng.integers(0, max(len(keys), 1), size=12) if keys]:
        v = k & ~W.DNA_TAG
        s = bases(v, L)
        seqs += [s, s + b"ACGTN", bases(max(v - 1, 0), L), bases(min(v + 1, (1 << (2 * L)) - 1), L)]
        if L:
            seqs += [bytes([b"CGTA"[b"ACGT".index(s[0])]]) + s[1:], s[:-1] + bytes([b"CGTA"[b"ACGT".index(s[-1])]]),
                     s[:-1], s[:-1] + b"N", s[:-1] + b"\r", s.lower(), s[:L // 2] + b"N" + s[L // 2 + 1:]]
    for _ in range(40):
        seqs.append(letters(rng, Lb + int(rng.integers(0, 4)), b"ACGT"))
    if L:
        seqs += [b"C" * (Lb - 1), b"C" * (Lb - 1) + b"N", b"C" * (Lb - 1) + b"\r", b"c" * Lb, b"C" * Lb]
    return seqs


@pytest.mark.parametrize("L,n_wl", [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (16, 0), (16, 1), (16, 2), (16, 1000), (31, 1), (31, 2),
                                    (31, 1000), (32, 0), (32, 1000)])
def test_whitelist_lookup(L, n_wl):
    rng = np.random.default_rng(100 * L + n_wl)
    keys = whitelist(31 if L == 32 else L, n_wl, rng)         # (L = 32: the list still holds keys; no read may reach them)
    seqs = probe_lines(L, keys if L != 32 else [], rng)
    reads = [(b"@" + b"x" * (i % 4), s, b"+" * (1 + (i // 4) % 3), b"I" * len(s)) for i, s in enumerate(seqs)]
    text = fastq(reads)
    fr = W.Framing(text)
    assert {int(fr.start[4 * r + 1]) & 3 for r in range(fr.n_reads)} == {0, 1, 2, 3}
    n_seen = [0]

    def judge(r, line):                                       # every second escape, in read order
        n_seen[0] += 1
        return n_seen[0] % 2 == 1
    with Dev(4096) as dev:
        dev.set_whitelist(keys)
        lens = [4096] * (len(text) // 4096) + [len(text) % 4096]
        want, end, keep = check(dev, text, lens, mode=0, all_cells=False, L=L, rate=2.0, judge=judge, bogus_hits=True, tag="L %d" % L)
        n_esc = sum(len(w["esc"]) for w in want)
        assert n_esc == n_seen[0] and end["kept"] == keep.sum()
        hit = [r for r in range(fr.n_reads) if W.dna_key(fr.body(4 * r + 1), L) in set(keys) and W.dna_key(fr.body(4 * r + 1), L)]
        if L == 32:
            assert n_esc == fr.n_reads and not hit
        elif L == 0:
            assert n_esc == 0 and keep.sum() == (fr.n_reads if n_wl else 0)
        else:
            assert n_esc >= 5 and (len(hit) >= 2 * min(n_wl, 5)) and (n_wl == 0 or 0 < len(hit) < fr.n_reads - n_esc)
        check(dev, text, [len(text) % 4096] + [4096] * (len(text) // 4096), mode=1, tag="L %d / mode 1" % L)


# ---------------------------------------------------------------- 6. chosen draws
def rows9(n):
    """n reads of 9 bytes: @X\\nA\\n+\\nI\\n, X from the read index modulo 91"""
    t = np.tile(np.frombuffer(b"@X\nA\n+\nI\n", dtype=np.uint8), (n, 1))
    t[:, 1] = 33 + np.arange(n) % 91
    return t


def chosen_states(n_rec):
    """words whose draws pass at rate 1.0 everywhere but where a case puts its own"""
    s = np.random.default_rng(n_rec).integers(0, 1 << 31, size=((n_rec + W.CHUNK - 1) // W.CHUNK, W.DEG), dtype=np.uint32)
    s[0, 3] = ((1 << 31) - 64) << 1                           # rounds to 2^31: 1.0 < 1.0 fails
    s[0, 4] = (((1 << 31) - 65) << 1) | 1                     # rounds to 2^31 - 128: kept
    s[0, 5] = ((1 << 24) - 1) << 1                            # against the rate 2^24 / 2^31: kept
    s[0, 6] = (1 << 24) << 1                                  # equal: dropped
    s[0, 7] = (((1 << 24) + 1) << 1) | 1                      # rounds to 2^24: dropped
    s[-1, 0] = ((1 << 31) - 1) << 1                           # the first draw of the last chunk: dropped at 1.0
    return s


@pytest.mark.parametrize("n", [2047, 2048, 2049, 256 * 2048 + 1])
def test_chosen_draws_and_chunk_edges(n):
    rows = rows9(n)
    text = rows.reshape(-1)
    wins = [(0, len(text), NONE)]
    states = chosen_states(n)
    draws = W.chunk_draws(states, n)
    assert draws[3] == (1 << 31) - 64 and draws[4] == (1 << 31) - 65 and draws[(n - 1) // 2048 * 2048] == (1 << 31) - 1
    with Dev(5 << 20) as dev:
        for rate in (1.0, (2 ** 24 + 1) / 2 ** 31, 0.5):
            keep = W.passes(draws, rate)
            if rate == 1.0:
                assert not keep[3] and keep[4] and not keep[(n - 1) // 2048 * 2048] and keep.sum() >= n - 3
            elif rate < 0.5:
                assert keep[5] and not keep[6] and not keep[7]
            got, end = dev.feed(text, wins, 0, True, 16, rate, lambda r_lo, n_rec: states)
            assert (got[0]["r_lo"], got[0]["n_rec"], got[0]["total"]) == (0, n, 9 * int(keep.sum())), rate
            assert np.array_equal(got[0]["out"], rows[keep].reshape(-1)), rate
            assert end == dict(n_nl=4 * n, kept=int(keep.sum()), err=0, err_rec=NONE), rate


# ---------------------------------------------------------------- 7. scan blocks and output expansion
def rows8(n):
    t = np.tile(np.frombuffer(b"@\nX\n+\nI\n", dtype=np.uint8), (n, 1))
    t[:, 2] = 33 + np.arange(n) % 91
    return t


def mode1_rows(dev, rows, keep, limit=NONE):
    """a second file of fixed-width rows against the bitmap: exactly the rows the first pass kept"""
    text, w = rows.reshape(-1), rows.shape[1]
    lens = [dev.Wb] * (len(text) // dev.Wb) + [len(text) % dev.Wb]
    a, wins = 0, []
    for ln in lens:
        wins.append((a, ln, NONE))
        a += ln
    got, end = dev.feed(text, wins, 1, limit=limit)
    r = 0
    for g, (a, ln, _) in zip(got, wins):
        r_hi = (a + ln) // w                                  # reads whose last byte lies below a + ln
        assert (g["r_lo"], g["n_rec"]) == (r, r_hi - r), a
        assert np.array_equal(g["out"], rows[r:r_hi][keep[r:r_hi]].reshape(-1)), a
        r = r_hi
    assert end == dict(n_nl=4 * len(rows), kept=0, err=0, err_rec=NONE)


@pytest.mark.parametrize("n,Wb", [(1023, 8192), (1024, 8192), (1025, 8192), ((4 << 20) // 4 + 1024, (4 << 20) + 4096)])
def test_scan_blocks_and_output_expansion(n, Wb):
    text = np.full(4 * n, 10, dtype=np.uint8)                 # reads of four empty lines: 5 bytes out for 4 in
    wins = [(0, len(text), NONE)]
    five = np.frombuffer(b"\n\n+\n\n", dtype=np.uint8)
    assert (n + 1023) // 1024 > 1024 or n <= 1025
    with Dev(Wb) as dev:
        keep = W.passes(W.chunk_draws(random_states(0, n), n), 0.5)
        assert 0.45 * n < keep.sum() < 0.55 * n
        got, end = dev.feed(text, wins, 0, True, 16, 0.5)
        assert (got[0]["r_lo"], got[0]["n_rec"], got[0]["total"]) == (0, n, 5 * int(keep.sum()))
        assert np.array_equal(got[0]["out"], np.tile(five, int(keep.sum())))
        assert end == dict(n_nl=4 * n, kept=int(keep.sum()), err=0, err_rec=NONE)
        mode1_rows(dev, rows8(n), keep)                       # which reads they were: the bitmap against rows that differ
        # every read kept: 1.25 x the window comes back
        got, end = dev.feed(text, wins, 0, True, 16, 2.0)
        assert got[0]["total"] == 5 * n and (4 * n < Wb or 5 * n > Wb + Wb // 4 - 8)
        assert np.array_equal(got[0]["out"], np.tile(five, n))
        assert end == dict(n_nl=4 * n, kept=n, err=0, err_rec=NONE)


# ---------------------------------------------------------------- 8. bitmap growth
def test_bitmap_growth_keeps_the_bits_set_before():
    n, Wb = 8_400_000, 8 << 20
    rows = rows9(n)
    text = rows.reshape(-1)
    assert (n + 31) // 32 + 1 > (1 << 20) // 4 >= (8_000_000 + 31) // 32 + 1      # the first allocation covers 8 000 000 reads, not these
    a, wins = 0, []
    while a < len(text):
        ln = min(Wb, len(text) - a)
        wins.append((a, ln, NONE))
        a += ln
    keep = np.zeros(n, dtype=bool)
    with Dev(Wb) as dev:
        got, end = dev.feed(text, wins, 0, True, 16, 0.5)
        r = 0
        for g, (a, ln, _) in zip(got, wins):
            r_hi = (a + ln) // 9
            assert (g["r_lo"], g["n_rec"]) == (r, r_hi - r), a
            keep[r:r_hi] = W.passes(W.chunk_draws(random_states(r, r_hi - r), r_hi - r), 0.5)
            assert g["total"] == 9 * int(keep[r:r_hi].sum()), a
            assert np.array_equal(g["out"], rows[r:r_hi][keep[r:r_hi]].reshape(-1)), a
            r = r_hi
        assert r == n and 0.49 * n < keep.sum() < 0.51 * n
        assert end == dict(n_nl=4 * n, kept=int(keep.sum()), err=0, err_rec=NONE)
        # a second file of 10-byte reads against the bitmap: the rows kept above, those of before the reallocation included
        rows10 = np.tile(np.frombuffer(b"@Xy\nC\n+\nJ\n", dtype=np.uint8), (n, 1))
        rows10[:, 1] = 33 + np.arange(n) % 91
        rows10[:, 2] = 40 + np.arange(n) % 83
        assert keep[:8_000_000].sum() > 3_900_000
        mode1_rows(dev, rows10, keep)
