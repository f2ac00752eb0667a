"""K1b's per-record gating (bam2db_ds.c:385-416) as include/fastf_amd.h states it for fastf_dev_probe_pack, in plain numpy, and the
hand-built record and decision streams that tests/test_gpu_k1b_gating.py runs on the device.  Nothing here is shared with the
kernels; tests/test_k1b_ref_host.py checks the reference against the oracle and takes a census of the fixtures.

The contract.  Record i has a cell index (0: no CB hit), a feature index (0: none), umi and meta.  The j-th hit in record order
has rank draw_base + j and is kept iff bit (rank & 31) of word rank >> 5 of the decision stream is set; a rank >= n_draws is
dropped and raises bit 2.  hits = records with a cell, sampled = hits whose bit is set, valid = sampled records with XF_OK, a
feature and HAS_UB; a key is emitted exactly for the valid records, into the list of the cell's shard; a valid record whose UMI
does not fit raises bit 4; a shard with more keys than shard_stride raises bit 8.

place_units() restates the same decisions the way a kernel that walks 256-record units has to find them (the unit's first rank
from the hits in front of it, nine 32-bit words from the word of that rank on, clamped to the stream's last word); its defect=
switch turns one rule into a wrong one (DEFECTS), and with defect=None it must agree with the plain rule."""
import numpy as np

from fastf_amd.dist import owner_of_cell

U = np.uint64
XF_OK, HAS_UB, UMI_NONNULL, UMI_TOOLONG, LEN_SHIFT = 1, 2, 4, 8, 4
ERR_DRAWS_SHORT, ERR_UMI_TOOLONG, ERR_KEYS_FULL = 2, 4, 8
UNIT, TILE = 256, 4096
GUARD_WORDS = 64                          # words of 0xFFFFFFFF behind a decision stream on the device

DEFECTS = ("sbit_off_by_one", "own_half_hits", "no_ninth_word", "no_draw_base", "last_clamp", "flags_before_draw")


def bits_for(v):
    return int(v).bit_length()


class Layout:
    """[cell][feature][nonnull 1][umi 2 * bases][blob bytes]; wide (more than 64 bits, or more than 16 bases): the group word
    cell << feature_bits | feature and the rest of the key side by side"""

    def __init__(self, cell_bits, feature_bits, umi_max_bases):
        self.cell_bits, self.feature_bits, self.bases = cell_bits, feature_bits, umi_max_bases
        self.ub, self.max_bytes = 2 * umi_max_bases, (umi_max_bases + 3) // 4
        self.lb = bits_for(self.max_bytes)
        self.fs = 1 + self.ub + self.lb
        self.cs = self.fs + feature_bits
        self.key_bits = self.cs + cell_bits
        self.wide = self.key_bits > 64 or umi_max_bases > 16
        assert umi_max_bases <= 24

    @classmethod
    def of_engine(cls, eng, umi_max_bases):
        L = cls(eng.cell_bits, eng.feature_bits, umi_max_bases)
        assert eng.umi_bits == L.fs and eng.key_bits == L.key_bits and eng.wide == L.wide      # (umi_bits: flag + UMI + length)
        return L

    def ident(self):
        return (self.cell_bits, self.feature_bits, self.bases)


def _umi64(umi, ext):
    return (np.asarray(umi).astype(U) << U(32)) | (np.zeros(len(umi), U) if ext is None else np.asarray(ext).astype(U))


def low_part(L, umi, meta, ext=None):
    """the key below the feature: flag, UMI (first base on top), blob bytes; 0 for a NULL UMI"""
    meta = np.asarray(meta).astype(U)
    nn = (meta >> U(2)) & U(1)
    ln = (meta >> U(LEN_SHIFT)) & U(15)
    return ((nn << U(L.ub + L.lb)) | ((_umi64(umi, ext) >> U(64 - L.ub)) << U(L.lb)) | ln) * nn


def too_long(L, umi, meta, ext=None):
    """a UMI the layout cannot hold: flagged so by the packer, more blob bytes than the length field counts, or bases beyond umi_max_bases"""
    meta = np.asarray(meta).astype(np.int64)
    nn = (meta & UMI_NONNULL) != 0
    ln = (meta >> LEN_SHIFT) & 15
    tail = (_umi64(umi, ext) << U(L.ub)) != 0
    return ((meta & UMI_TOOLONG) != 0) | (nn & ((ln > L.max_bytes) | tail))


def pack_bits(bits):
    """0/1 array -> the u32 words of the device layout: 8-byte granules, the tail of the last 64 bits zero"""
    b = np.zeros((len(bits) + 63) // 64 * 64, np.uint8)
    b[:len(bits)] = bits
    return np.packbits(b, bitorder="little").view(np.uint32).copy()


def plain_decisions(hit, bits, draw_base, n_draws):
    """(kept, beyond the stream) per record by the rule of the header: the i-th hit has rank draw_base + i"""
    hit = np.asarray(hit, bool)
    rank = draw_base + np.cumsum(hit) - 1
    inside = hit & (rank < n_draws)
    keep = np.zeros(len(hit), bool)
    keep[inside] = np.asarray(bits, np.uint8)[rank[inside]] != 0
    return keep, hit & ~inside


def place_units(hit, bits, draw_base, n_draws, defect=None):
    """the same two arrays, unit by unit: rank0 = draw_base + the hits in front of the unit (its tile's base + the units in front of
    it in the tile); the unit reads bits sbit + local rank of the nine words from word rank0 >> 5 on, none behind the last word
    that holds a decision; a hit with local rank >= n_draws - rank0 is beyond the stream"""
    hit = np.asarray(hit, bool)
    n = len(hit)
    words = pack_bits(np.asarray(bits, np.uint8)[:n_draws]) if n_draws else np.zeros(2, np.uint32)
    keep, short = np.zeros(n, bool), np.zeros(n, bool)
    n_units = (n + UNIT - 1) // UNIT
    per_unit = np.array([int(hit[u * UNIT:(u + 1) * UNIT].sum()) for u in range(n_units)], np.int64)
    for u in range(n_units):
        t0 = u // 16 * 16
        tile_base = int(per_unit[:t0].sum())
        in_tile = int(per_unit[t0:u + (1 if defect == "own_half_hits" else 0)].sum())
        rank0 = tile_base + in_tile + (0 if defect == "no_draw_base" else draw_base)
        avail = max(0, n_draws - rank0)
        sbit = (rank0 + (1 if defect == "sbit_off_by_one" else 0)) & 31
        last = (n_draws - 1) >> 5 if n_draws else 0
        if defect == "last_clamp":
            last = max(last - 1, 0)
        first = rank0 >> 5
        room = min(last - first, 15) if first < last else 0
        lane_word = [words[min(first, last) + min(l, room)] for l in range(16)]
        idx = np.nonzero(hit[u * UNIT:(u + 1) * UNIT])[0] + u * UNIT
        for rl, i in enumerate(idx.tolist()):
            bpos = sbit + rl
            sel = bpos >> 5
            if defect == "no_ninth_word":
                sel = min(sel, 7)
            if rl >= avail:
                short[i] = True
            else:
                keep[i] = (int(lane_word[sel]) >> (bpos & 31)) & 1
    return keep, short


class Result:
    def __init__(self, keys, vals, counters, err):
        self.keys, self.vals, self.counters, self.err = keys, vals, counters, err      # per shard: sorted keys (wide: pairs sorted by (key, val))


def k1b(cell, feat, umi, meta, bits, draw_base, n_draws, L, n_shards=1, shard_stride=None, ext=None, defect=None):
    """per shard the multiset of keys (sorted), {hits, sampled, valid}, the error bits.  shard_stride: one number or one per shard
    (None: no bound).  A shard over its bound raises bit 8; its whole multiset is returned, of which at most shard_stride keys,
    any of them, may have been written"""
    cell, feat, meta = np.asarray(cell, np.int64), np.asarray(feat, np.int64), np.asarray(meta, np.int64)
    hit = cell > 0
    if defect in (None, "flags_before_draw"):
        keep, short = plain_decisions(hit, bits, draw_base, n_draws)
    else:
        keep, short = place_units(hit, bits, draw_base, n_draws, defect)
    xf = (meta & XF_OK) != 0
    sampled = hit & keep
    valid = sampled & xf & (feat > 0) & ((meta & HAS_UB) != 0)
    n_sampled = int((sampled & xf).sum()) if defect == "flags_before_draw" else int(sampled.sum())
    err = (ERR_DRAWS_SHORT if short.any() else 0) | (ERR_UMI_TOOLONG if (valid & too_long(L, umi, meta, ext)).any() else 0)
    c, f = cell[valid].astype(U), feat[valid].astype(U)
    low = low_part(L, np.asarray(umi)[valid], meta[valid], None if ext is None else np.asarray(ext)[valid])
    if L.wide:
        k, v = (c << U(L.feature_bits)) | f, low
    else:
        k, v = (c << U(L.cs)) | (f << U(L.fs)) | low, np.zeros(len(c), U)
    own = owner_of_cell(cell[valid], n_shards) if n_shards > 1 else np.zeros(len(c), np.int64)
    strides = [None] * n_shards if shard_stride is None else (list(shard_stride) if np.ndim(shard_stride) else [shard_stride] * n_shards)
    keys, vals = [], []
    for s in range(n_shards):
        ks, vs = k[own == s], v[own == s]
        o = np.lexsort((vs, ks))
        keys.append(ks[o]); vals.append(vs[o])
        if strides[s] is not None and len(ks) > strides[s]:
            err |= ERR_KEYS_FULL
    return Result(keys, vals, (int(hit.sum()), n_sampled, int(valid.sum())), err)


# ---------------------------------------------------------------------------------------------------------------------
# fixtures: record streams, hit patterns, decision streams
# ---------------------------------------------------------------------------------------------------------------------
LENGTHS = [1, 255, 256, 257, 4095, 4096, 4097, 12 * 256 + 1, 40_001]
BASES = [0, 1, 31, 32, 33, 63, 1_000_003]
BIT_PATTERNS = ["ones", "zeros", "alt", "one_set", "one_clear", "random"]
HIT_PATTERNS = ["all", "none", "one@0", "one@255", "one@256", "one@4095", "one@4096", "one@last", "alt_full_empty", "alt_empty_full",
                "unit1_lo", "unit1_hi", "unit31", "unit32", "unit33", "unit255", "hi_lanes", "period3", "tile0_empty"]
N_MAX = LENGTHS[-1]
FLAG_PERIOD = 67                          # coprime to 64 and to 3: every combination meets both values of every periodic decision bit


def hit_mask(pattern, n):
    i = np.arange(n)
    if pattern == "all": return np.ones(n, bool)
    if pattern == "none": return np.zeros(n, bool)
    if pattern.startswith("one@"):
        p = n - 1 if pattern == "one@last" else int(pattern[4:])
        return i == min(p, n - 1)
    if pattern == "alt_full_empty": return (i // UNIT) % 2 == 0
    if pattern == "alt_empty_full": return (i // UNIT) % 2 == 1
    if pattern == "unit1_hi": return i % UNIT == UNIT - 1
    if pattern == "unit1_lo": return i % UNIT == 0
    if pattern.startswith("unit"): return i % UNIT < int(pattern[4:])
    if pattern == "hi_lanes": return i % 64 >= 32
    if pattern == "period3": return i % 3 == 0
    if pattern == "tile0_empty": return i >= TILE
    raise KeyError(pattern)


def stream_bits(pattern, n_draws, base, seed=0):
    """the decisions of ranks 0 .. n_draws - 1: the pattern by absolute word, random filler in front of `base`"""
    nw = (n_draws + 31) // 32
    w = np.arange(nw, dtype=np.int64)
    one = (np.int64(1) << ((7 * w) % 32)).astype(np.uint32)
    rng = np.random.default_rng(1000 + seed)
    words = {"ones": np.full(nw, 0xFFFFFFFF, np.uint32), "zeros": np.zeros(nw, np.uint32), "alt": np.full(nw, 0x55555555, np.uint32),
             "one_set": one, "one_clear": ~one, "random": rng.integers(0, 1 << 32, size=nw, dtype=np.uint64).astype(np.uint32)}[pattern]
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:n_draws].copy()
    bits[:base] = np.random.default_rng(7).integers(0, 2, size=base, dtype=np.uint8)
    return bits


class Fixture:
    def __init__(self, n, hits, bits, base):
        self.n, self.hits, self.bits, self.base = n, hits, bits, base
        self.name = "n%d-%s-%s-b%d" % (n, hits, bits, base)

    def mask(self):
        return hit_mask(self.hits, self.n)

    def n_draws(self):
        return self.base + int(self.mask().sum())

    def stream(self):
        return stream_bits(self.bits, self.n_draws(), self.base, seed=self.n)


def fixtures():
    out, seen, k = [], set(), [0]

    def add(n, hits, bits=None, base=None):
        fx = Fixture(n, hits, BIT_PATTERNS[k[0] % 6] if bits is None else bits, BASES[k[0] % 7] if base is None else base)
        k[0] += 1
        if fx.name not in seen:
            seen.add(fx.name); out.append(fx)
    for n in LENGTHS:                                            # every length: all hits, none, period 3
        add(n, "all", "random"); add(n, "none"); add(n, "period3")
    for pat in HIT_PATTERNS:                                     # every hit pattern where a tile ends and where a unit does
        add(4097, pat); add(12 * 256 + 1, pat)
    for b in BIT_PATTERNS:                                       # every decision pattern on full units that start inside a word
        add(4097, "all", b, 33)
    for base in BASES:
        add(4097, "all", "random", base); add(12 * 256 + 1, "hi_lanes", "random", base)
    add(40_001, "all", "random", 1_000_003); add(40_001, "alt_full_empty", "random", 33); add(40_001, "alt_empty_full", "one_set", 31)
    add(40_001, "period3", "alt", 63); add(40_001, "tile0_empty", "one_clear", 32); add(40_001, "unit33", "random", 1)
    add(256, "all", "random", 0); add(4096, "all", "one_clear", 0)          # streams of a multiple of 64 decisions
    return out


def flag_table():
    """67 entries (xf, ub, nonnull, listed GX, too long): the 16 combinations of the first four, the same with a too-long UMI — but
    never on a record that xf, GX and UB would keep: those raise bit 4 and have tests of their own — and 35 records that pass"""
    t = []
    for j in range(FLAG_PERIOD):
        c = j & 15 if j < 32 else 15
        xf, ub, nn, listed = c & 1, (c >> 1) & 1, (c >> 2) & 1, (c >> 3) & 1
        t.append((xf, ub, nn, listed, 1 if 16 <= j < 32 and not (xf and ub and listed) else 0))
    return t


def build_records(n_cells, listed_gx, unlisted_gx, n=N_MAX, blob_bytes=3):
    """gx, umi, meta, umi_ext of n records and the cell index a record has IF its CB hits (i % n_cells + 1).  Every non-NULL UMI is
    unique (number i + 1 in the top 24 bits), so a key names its record; a NULL record gets feature i // n_cells + 1, a
    (cell, feature) pair of its own.  The flags cycle through flag_table() scattered by 29 i mod 67."""
    i = np.arange(n, dtype=np.int64)
    tab = np.array(flag_table(), np.int64)[(29 * i) % FLAG_PERIOD]
    xf, ub, nn, listed, tl = tab.T
    f = np.where(nn == 1, (7 * i) % len(listed_gx), i // n_cells)
    assert int(f.max()) < len(listed_gx)
    gx = np.where(listed == 1, np.asarray(listed_gx, U)[f], np.asarray(unlisted_gx, U)[i % len(unlisted_gx)])
    umi = (((i + 1) << 8) * nn).astype(np.uint32)
    ext = ((((i * 0x9E37) & 0xFF) << 24) * nn).astype(np.uint32) if blob_bytes > 4 else None
    meta = (xf * XF_OK | ub * HAS_UB | nn * UMI_NONNULL | tl * UMI_TOOLONG | (nn * blob_bytes) << LEN_SHIFT).astype(np.uint32)
    return gx.astype(U), umi, meta, ext, (i % n_cells + 1)


def cb_keys(mask, cell_if_hit, cell_keys, unlisted_cb):
    """CB keys of a hit pattern: the listed key of the record's cell, else key 0 and unlisted keys by turns"""
    n = len(mask)
    i = np.arange(n)
    miss = np.where(i % 2 == 0, U(0), np.asarray(unlisted_cb, U)[(i // 2) % len(unlisted_cb)])
    return np.where(mask, np.asarray(cell_keys, U)[cell_if_hit[:n] - 1], miss).astype(U)
