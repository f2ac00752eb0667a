"""Plain numpy / Python restatements of the barcode (K1a) and gene (K1b) lookups, and builders of near-miss keys for the image and
tables an engine builds from a given list.  Restated from the comments and host mirrors in fastf_amd/csrc/umi_engine.hip and
umi_kernels.hpp; 64-bit unsigned arithmetic with explicit masks.  Used by tests/test_lookup_host.py (CPU) and
tests/test_gpu_lookup.py (GPU): the expected cell index of a near miss is 0, the expected feature index is a dictionary lookup.

Key packing (host_prims.c): DNA form  [63:62]=1 [61:57] length [56:49] suffix+1 [47:0] bases, first base on top;
                            ID form   [63:62]=2 [61:48] prefix id [47:44] digit count [43:0] value."""
import numpy as np

import fastf_amd as F
from fastf_amd import synth

U64 = np.uint64
M32 = U64(0xFFFFFFFF)
C1, C2, C3 = 0x9E3779B1, 0x85EBCA77, 0xC2B2AE3D
C1_INV, C2_INV = pow(C1, -1, 1 << 32), pow(C2, -1, 1 << 32)
HAS_CB, HAS_XF, HAS_GX, HAS_UB = 1, 2, 4, 8


def _u64(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64))


def _mul32(a, c):
    """(a * c) mod 2^32 for a < 2^32 (the product fits 64 bits)"""
    return (a * U64(c)) & M32


# ---- the hashes ----
def slot_hash(key):
    k = _u64(key)
    h = (_mul32(k & M32, C1) + _mul32(k >> U64(32), C2)) & M32
    return h ^ (h >> U64(15))


def filter_bit(key):
    k = _u64(key)
    h = (_mul32(k & M32, C2) + _mul32(k >> U64(32), C3)) & M32
    return h ^ (h >> U64(13))


def cell_mix(code, seed):
    h = _mul32((_u64(code) ^ U64(seed)) & M32, C1)
    h = h ^ (h >> U64(15))
    h = _mul32(h, C2)
    return h ^ (h >> U64(13))


def cell_mix_inv(h, seed):
    """odd multipliers and xor-shifts are invertible: y = x ^ (x >> s) gives x = y ^ (y >> s) ^ (y >> 2 s) ^ .. in 32 bits"""
    h = _u64(h)
    h = h ^ (h >> U64(13)) ^ (h >> U64(26))
    h = _mul32(h, C2_INV)
    h = h ^ (h >> U64(15)) ^ (h >> U64(30))
    return _mul32(h, C1_INV) ^ U64(seed)


def code_of(key):
    return (_u64(key) >> U64(16)) & M32


# ---- the LDS cell image: u32 slot[1 << S] | u16 disp[bucket_mask + 1]; slot = (lo << S) | index, 0 = empty ----
CHECKS = ("all", "no_lo", "no_family", "no_low16")


def image_parts(image, params):
    S, bm = int(params[0]), int(params[1])
    image = np.ascontiguousarray(image, dtype=np.uint8)
    slots = image[:4 << S].view(np.uint32).astype(np.uint64)
    disp = image[4 << S:(4 << S) + 2 * (bm + 1)].view(np.uint16).astype(np.uint64)
    return slots, disp


def image_probe(image, params, key, check="all"):
    """the probe of probe_cells_lds_kernel; `check` names the one test that is left out (the weakened forms only prove that a set
    of keys is adversarial: a probe without that test would call them hits)"""
    assert check in CHECKS
    S, bm, family, seed = int(params[0]), int(params[1]), int(params[2]), int(params[4])
    slots, disp = image_parts(image, params)
    k = _u64(key)
    smask, lo_mask = U64((1 << S) - 1), U64((1 << (32 - S)) - 1)
    h = cell_mix(code_of(k), seed)
    lo = h & lo_mask
    e = slots[((h >> U64(32 - S)) + disp[lo & U64(bm)]) & smask]
    ok = np.ones(len(k), bool)
    if check != "no_family":
        ok &= (k >> U64(49)) == U64(family)
    if check != "no_low16":
        ok &= (k & U64(0xFFFF)) == 0
    if check != "no_lo":
        ok &= (e >> U64(S)) == lo
    return np.where(ok, e & smask, U64(0)).astype(np.uint32)


# ---- the L2 open-addressed table (build_table) and the miss filter (build_cell_filter) ----
def l2_table(keys):
    """(slot keys u64[cap], slot values u32[cap]): cap a power of two >= 2 n and >= 64, linear probing, value = index + 1"""
    keys = _u64(keys)
    cap = 64
    while cap < 2 * len(keys):
        cap <<= 1
    tk, tv = [0] * cap, [0] * cap
    home = (slot_hash(keys) & U64(cap - 1)).tolist()
    for i, (k, h) in enumerate(zip(keys.tolist(), home)):
        assert k != 0
        while tk[h]:
            assert tk[h] != k, "duplicate key"
            h = (h + 1) & (cap - 1)
        tk[h], tv[h] = k, i + 1
    return np.array(tk, dtype=np.uint64), np.array(tv, dtype=np.uint32)


def l2_probe(table, key):
    """(value or 0, slots inspected) of one key: table_probe()"""
    tk, tv = table
    key = int(key)
    if key == 0:
        return 0, 0
    mask = len(tk) - 1
    h = int(slot_hash(key)[0]) & mask
    for i in range(len(tk)):
        k = int(tk[h])
        if k == key:
            return int(tv[h]), i + 1
        if k == 0:
            return 0, i + 1
        h = (h + 1) & mask
    return 0, len(tk)


def filter_bits(keys):
    """the bit set of build_cell_filter as a bool array: 2^15 bits, doubled while below 10 n, 2^18 at most"""
    keys = _u64(keys)
    bits = 1 << 15
    while bits < 10 * len(keys) and bits < (1 << 18):
        bits <<= 1
    f = np.zeros(bits, bool)
    f[(filter_bit(keys) & U64(bits - 1)).astype(np.int64)] = True
    return f


def in_filter(filt, key):
    return filt[(filter_bit(key) & U64(len(filt) - 1)).astype(np.int64)]


def occupied_runs(table):
    """maximal runs of occupied slots of the (circular) table: list of (head, length); head + length > cap: the run wraps"""
    occ = table[0] != 0
    cap = len(occ)
    empty = np.nonzero(~occ)[0]
    assert len(empty)
    e0 = int(empty[0])
    rot = np.roll(occ, -(e0 + 1))                          # rot[j] = occ[(e0 + 1 + j) % cap]; rot[cap - 1] is empty
    d = np.diff(np.concatenate([[0], rot.astype(np.int8), [0]]))
    starts, ends = np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]
    return [((int(s) + e0 + 1) % cap, int(e - s)) for s, e in zip(starts, ends)]


def displaced_past_the_end(table):
    """listed keys that linear probing carried from the last slots round to the first ones"""
    tk = table[0]
    pos = np.nonzero(tk)[0]
    home = (slot_hash(tk[pos]) & U64(len(tk) - 1)).astype(np.int64)
    return tk[pos[home > pos]]


def keys_for_slot(head, mask, n, rng):
    """n arbitrary 64-bit keys whose slot_hash & mask is `head`: the hash is solved for the key's low word"""
    t = (rng.integers(0, 1 << 32, size=n, dtype=np.uint64) & ~U64(mask) & M32) | U64(head)
    h0 = t ^ (t >> U64(15)) ^ (t >> U64(30))
    hi = rng.integers(1, 1 << 32, size=n, dtype=np.uint64)
    lo = _mul32((h0 + (U64(1) << U64(32)) - _mul32(hi, C2)) & M32, C1_INV)
    k = (hi << U64(32)) | lo
    assert ((slot_hash(k) & U64(mask)) == U64(head)).all()
    return k


# ---- lists ----
def barcode_text(n, seed, k=16, suffix=b"-1"):
    """n distinct random k-mers + suffix, one per line"""
    rng = np.random.default_rng(seed)
    codes = np.unique(rng.integers(0, 1 << (2 * k), size=int(n * 1.2) + 16, dtype=np.uint64))
    rng.shuffle(codes)
    assert len(codes) >= n
    m = synth._kmers(codes[:n], k)
    return b"".join(bytes(r) + suffix + b"\n" for r in m)


def feature_text(ids):
    return b"".join(g + b"\tGene" + str(i + 1).encode() + b"\tGene Expression\n" for i, g in enumerate(ids))


def id_strings(prefix, digits, values):
    return [b"%s%0*d" % (prefix, digits, int(v)) for v in values]


def _cstr(strs):
    return synth.as_cstr(np.array(list(strs), dtype="S"))


def pack_cb(lists, strs):
    """CB strings -> keys through the product's own packer"""
    n = len(strs)
    z = np.zeros(n, "S2")
    return F.pack_records(lists, np.full(n, HAS_CB | HAS_XF, np.uint8), np.full(n, 25, np.int32), _cstr(strs), z, z)[0]


def pack_gx(lists, strs):
    n = len(strs)
    z = np.zeros(n, "S2")
    return F.pack_records(lists, np.full(n, HAS_XF | HAS_GX, np.uint8), np.full(n, 25, np.int32), z, _cstr(strs), z)[1]


def cell_index(cell_keys, key):
    """the truth of K1a: 1-based position in the list, 0 for everything else"""
    ck = _u64(cell_keys)
    order = np.argsort(ck, kind="stable")
    sk = ck[order]
    k = _u64(key)
    at = np.minimum(np.searchsorted(sk, k), len(sk) - 1)
    return np.where(sk[at] == k, order[at] + 1, 0).astype(np.int64)


def gene_lookup(feature_keys, key):
    """the truth of K1b's feature lookup: a dictionary from listed key to 1-based index (key 0 matches nothing)"""
    d = {int(k): i + 1 for i, k in enumerate(_u64(feature_keys).tolist())}
    d.pop(0, None)
    return np.array([d.get(int(k), 0) for k in _u64(key).tolist()], dtype=np.int64)


# ---- adversarial CB keys; every builder returns keys whose expected cell index is 0 ----
def _family_key(params, code):
    return (U64(int(params[2])) << U64(49)) | (_u64(code) << U64(16))


def _unlisted(cell_keys, keys):
    keys = np.unique(_u64(keys))
    return keys[(cell_index(cell_keys, keys) == 0) & (keys != 0)]


def slot_twins(cell_keys, image, params, n, rng):
    """unlisted codes whose mix lands in an OCCUPIED slot — hi and bucket chosen, cell_mix inverted — with another lo than the
    slot keeps: only the quotient compare tells them from the slot's owner"""
    S, bm, seed = int(params[0]), int(params[1]), int(params[4])
    slots, disp = image_parts(image, params)
    occ = np.nonzero(slots)[0]
    s = occ[rng.integers(0, len(occ), size=n)].astype(np.uint64)
    lo = rng.integers(0, 1 << (32 - S), size=n, dtype=np.uint64)
    lo = np.where(lo == (slots[s.astype(np.int64)] >> U64(S)), lo ^ U64(1), lo)
    hi = (s + U64(1 << S) - disp[lo & U64(bm)]) & U64((1 << S) - 1)
    keys = _family_key(params, cell_mix_inv((hi << U64(32 - S)) | lo, seed))
    return _unlisted(cell_keys, keys)


def lo_twins(cell_keys, image, params, n, rng):
    """unlisted codes that share a listed key's lo — its bucket, its displacement — with another hi"""
    S, seed = int(params[0]), int(params[4])
    ck = _u64(cell_keys)
    if len(ck) * ((1 << S) - 1) <= 4 * n:                                     # a tiny list: every other hi of every key
        which, other = np.repeat(np.arange(len(ck)), (1 << S) - 1), np.tile(np.arange(1, 1 << S, dtype=np.uint64), len(ck))
    else:
        which, other = rng.integers(0, len(ck), size=n), rng.integers(1, 1 << S, size=n, dtype=np.uint64)
    h = cell_mix(code_of(ck[which]), seed)                                    # (other is added to hi mod 2^S: never the same hi)
    hi = ((h >> U64(32 - S)) + other) & U64((1 << S) - 1)
    keys = _family_key(params, cell_mix_inv((hi << U64(32 - S)) | (h & U64((1 << (32 - S)) - 1)), seed))
    return _unlisted(cell_keys, keys)


def family_near_misses(lists, sample, rng):
    """keys that keep a listed barcode's 32-bit code (and zero low 16 bits) and differ above it: another suffix / none, the
    (k - 1)-base prefix of a listed k-mer ending in A (same base bits, another length), the listed barcode followed by A's (up to
    24 bases), and the code under the top two bits of another key form"""
    bars = lists.barcodes
    pick = [bars[i] for i in (range(len(bars)) if len(bars) <= sample else rng.choice(len(bars), size=sample, replace=False))]
    strs = []
    for b in pick:
        base, _, suf = b.partition(b"-")
        tail = (b"-" + suf) if suf else b""
        strs += [base + s for s in (b"-2", b"-254", b"-0", b"-1", b"") if s != tail]
        if base.endswith(b"A") and len(base) > 1:
            strs.append(base[:-1] + tail)
        strs += [base + b"A" * j + tail for j in range(1, 24 - len(base) + 1)]
    keys = [pack_cb(lists, strs)]
    ck = _u64(lists.cell_keys)
    some = ck[rng.integers(0, len(ck), size=min(3 * sample, 600))]
    for form in (0, 2, 3):
        keys.append((some & ~(U64(3) << U64(62))) | (U64(form) << U64(62)))
    return _unlisted(ck, np.concatenate(keys))


def low16_near_misses(cell_keys, n, rng):
    """a listed key with something in its low 16 bits (bases 17.. of a longer barcode live there)"""
    ck = _u64(cell_keys)
    r = rng.integers(1, 1 << 16, size=n, dtype=np.uint64)
    r[:3] = [1, 0x8000, 0xFFFF]
    return _unlisted(ck, ck[rng.integers(0, len(ck), size=n)] | r)


def filter_passers(cell_keys, filt, n, rng):
    """unlisted barcodes of the list's own family whose bit in the miss filter is set: they reach the L2 table, which must miss"""
    ck = _u64(cell_keys)
    out, have = [], 0
    for _ in range(40):
        code = rng.integers(0, 1 << 32, size=200_000, dtype=np.uint64)
        k = _unlisted(ck, (ck[0] & ~(M32 << U64(16))) | (code << U64(16)))
        k = k[in_filter(filt, k)]
        out.append(k); have += len(k)
        if have >= n:
            break
    return np.concatenate(out)[:n]


def chain_keys(cell_keys, table, filt, rng, per_head=8):
    """unlisted keys (any form) whose first slot is the head of the longest occupied run of the table and of the longest run that
    wraps past the last slot; filt: only keys the miss filter lets through.  Returns (keys, heads probed)"""
    runs = occupied_runs(table)
    cap = len(table[0])
    longest = max(runs, key=lambda r: r[1])
    wrapping = [r for r in runs if r[0] + r[1] > cap]
    assert wrapping, "no occupied run crosses the end of the table: choose another list seed"
    heads = [longest, max(wrapping, key=lambda r: r[1])]
    out = []
    for head, _ in heads:
        k = _unlisted(cell_keys, keys_for_slot(head, cap - 1, 4000, rng))
        if filt is not None:
            k = k[in_filter(filt, k)]
        assert len(k) >= 3
        out.append(k[:per_head])
    return np.concatenate(out), heads


def cb_near_misses(lists, image, params, rng, table=None, filt=None, twins=1500):
    """name -> keys (expected index 0 each).  image / params: the LDS image of the list (None: the list has none);
    table / filt: the restated L2 table and miss filter (None: leave their sets out)"""
    ck = _u64(lists.cell_keys)
    sets = {"zero": np.zeros(1, np.uint64),
            "family": family_near_misses(lists, 300, rng),
            "low16": low16_near_misses(ck, 600, rng)}
    if image is not None:
        sets["slot_twins"] = slot_twins(ck, image, params, twins, rng)
        sets["lo_twins"] = lo_twins(ck, image, params, twins, rng)
    if filt is not None:
        sets["filter_passers"] = filter_passers(ck, filt, 1500, rng)
    if table is not None:
        sets["chain"] = chain_keys(ck, table, filt, rng)[0]
    return sets


# ---- adversarial GX strings for a list whose majority family is <prefix><digits digits> ----
def family_values(lists, prefix, digits):
    ids = [f[0] for f in lists.features]
    return np.array(sorted(int(s[len(prefix):]) for s in ids if s.startswith(prefix) and len(s) == len(prefix) + digits
                           and s[len(prefix):].isdigit()), dtype=np.int64)


def bitmap_words(values):
    """the bitmap build_gene_lds lays over [vmin, vmax]"""
    o = values - values.min()
    w = np.zeros(int(o.max()) // 32 + 1, np.uint32)
    np.bitwise_or.at(w, o // 32, (np.uint32(1) << (o % 32).astype(np.uint32)))
    return w


def gx_near_miss_strings(lists, prefix, digits, other_prefixes=(), sample=200, rng=None):
    rng = rng or np.random.default_rng(0)
    vals = family_values(lists, prefix, digits)
    vmin, vmax = int(vals.min()), int(vals.max())
    listed = set(vals.tolist())
    o = vals - vmin
    near = set()
    for v in vals[o % 32 == 0].tolist():
        near.update((v + 1, v - 1))
    for v in vals[o % 32 == 31].tolist():
        near.update((v - 1, v + 1))
    near = sorted(v for v in near if vmin < v < vmax and v not in listed)
    if len(near) > 2 * sample:
        near = [near[i] for i in sorted(rng.choice(len(near), size=2 * sample, replace=False))]
    holes = [v for v in range(vmin, min(vmax, vmin + 20000)) if v not in listed][:sample]
    edge = [vmin, vmax, vmin - 1, vmax + 1, 0, (1 << 32) - 2, (1 << 32) - 1, 1 << 32]
    edge = [v for v in edge if 0 <= v < 10 ** digits]
    strs = id_strings(prefix, digits, edge + near + holes)
    strs.append(prefix + b"9" * 13)                                          # the largest 13-digit value: another family
    some = vals[rng.integers(0, len(vals), size=sample)].tolist() + [vmin, vmax]
    for d in (digits - 1, digits + 1, digits + 2):                            # the same numbers with another digit count
        strs += [s for s in id_strings(prefix, d, some) if len(s) == len(prefix) + d and d <= 13]
    for p in other_prefixes:                                                  # ... and with another (registered) prefix
        strs += id_strings(p, digits, some)
    strs += [b"", b"ENSG", b"no_such_gene", prefix]
    return strs
