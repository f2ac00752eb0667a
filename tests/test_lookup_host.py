"""The perfect-hash builder of the LDS barcode table (make_cell_image, through the host-only hook fastf_debug_cell_image) against
the restated probe of tests/lookup_ref.py, and the conditions that make the near-miss keys of lookup_ref adversarial: a probe
that left out one of its tests would call them hits.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib
import lookup_ref as R

GENES = R.feature_text(R.id_strings(b"ENSG", 11, range(1, 41)))
# list seeds for which the restated L2 table has an occupied run across its last slot (asserted where they are used)
WRAP_SEED = {1000: 17, 40_000: 4, 70_000: 6}


def cell_image(cell_keys):
    """(image bytes as uint8 array, params[5] = slot_bits, bucket_mask, family, bytes, seed), or (None, None): the list does not qualify"""
    L = _lib.lib()
    L.fastf_debug_cell_image.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]
    L.fastf_debug_cell_image.restype = C.c_size_t
    keys = np.ascontiguousarray(cell_keys, dtype=np.uint64)
    params = np.zeros(5, np.uint32)
    size = L.fastf_debug_cell_image(keys.ctypes.data, len(keys), None, 0, params.ctypes.data)
    if size == 0:
        return None, None
    img = np.zeros(size, np.uint8)
    assert L.fastf_debug_cell_image(keys.ctypes.data, len(keys), img.ctypes.data, size, params.ctypes.data) == size
    assert params[3] == size
    return img, params


_LISTS = {}


def lists_of(n, k=16, suffix=b"-1"):
    key = (n, k, suffix)
    if key not in _LISTS:
        _LISTS[key] = F.Lists(R.barcode_text(n, WRAP_SEED.get(n, 100 + n), k, suffix), GENES, 1.0, 926)
        assert len(_LISTS[key].cell_keys) == n
    return _LISTS[key]


def test_the_mix_is_a_bijection_and_its_inverse_is_right():
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.integers(0, 1 << 32, size=200_000, dtype=np.uint64), np.array([0, 1, 0xFFFFFFFF, 0x80000000], np.uint64)])
    for seed in (0, 0x632BE5AB, (5 * 0x632BE5AB) & 0xFFFFFFFF):
        h = R.cell_mix(x, seed)
        assert (h <= 0xFFFFFFFF).all()
        np.testing.assert_array_equal(R.cell_mix_inv(h, seed), x)
        np.testing.assert_array_equal(R.cell_mix(R.cell_mix_inv(x, seed), seed), x)


QUALIFYING = [(1, 16, b"-1"), (2, 16, b"-1"), (1023, 16, b"-1"), (1024, 16, b"-1"), (16383, 16, b"-1"), (16384, 16, b"-1"),
              (32767, 16, b"-1"), (3000, 12, b"-1"), (3000, 16, b"")]


@pytest.mark.parametrize("n,k,suffix", QUALIFYING)
def test_image_of_a_qualifying_list(n, k, suffix):
    lists = lists_of(n, k, suffix)
    img, p = cell_image(lists.cell_keys)
    assert img is not None
    S, bm = int(p[0]), int(p[1])
    assert S >= 10 and n <= (1 << S) - 1 and (S == 10 or n > (1 << (S - 1)) - 1)
    assert len(img) == (4 << S) + 2 * (bm + 1) and (bm & (bm + 1)) == 0
    assert int(p[2]) == int(lists.cell_keys[0]) >> 49
    slots, _ = R.image_parts(img, p)
    idx = slots & np.uint64((1 << S) - 1)
    np.testing.assert_array_equal(np.sort(idx[idx != 0]), np.arange(1, n + 1, dtype=np.uint64))
    assert ((slots == 0) == (idx == 0)).all()
    np.testing.assert_array_equal(R.image_probe(img, p, lists.cell_keys), np.arange(1, n + 1, dtype=np.uint32))


def _keys(text):
    return F.Lists(text, GENES, 1.0, 926).cell_keys


def test_lists_the_hook_declines(monkeypatch):
    monkeypatch.delenv("FASTF_LDS_CELLS_MAX", raising=False)
    good = R.barcode_text(2000, 5)
    assert cell_image(_keys(good))[0] is not None
    assert cell_image(lists_of(32767).cell_keys)[0] is not None
    declined = {
        "32768 cells": _keys(R.barcode_text(32768, 6)),
        "mixed suffixes": _keys(good + b"ACGTACGTACGTACGT-2\n"),
        "a 17-base barcode": _keys(good + b"ACGTACGTACGTACGTA-1\n"),
        "a DNA+N key": _keys(good + b"ACGTACGTACGNACGT-1\n"),
        "an ID-form key": _keys(good + b"CELL0001\n"),
    }
    assert len(declined["32768 cells"]) == 32768
    for what, keys in declined.items():
        assert len(keys) >= 2001 and (keys != 0).all()
        assert cell_image(keys) == (None, None), what
    k0 = _keys(good)
    assert (declined["a DNA+N key"][-1] >> np.uint64(62)) == 3 and (declined["an ID-form key"][-1] >> np.uint64(62)) == 2
    monkeypatch.setenv("FASTF_LDS_CELLS_MAX", "1999")
    assert cell_image(k0) == (None, None)
    monkeypatch.setenv("FASTF_LDS_CELLS_MAX", "2000")
    assert cell_image(k0)[0] is not None


@pytest.mark.parametrize("n,k,suffix", QUALIFYING)
def test_near_misses_probe_to_zero_and_are_adversarial(n, k, suffix):
    """every near-miss set misses under the full probe; without the quotient compare every slot twin is a hit, without the family
    test every family near miss, without the low-bits test every key that differs from a listed one in its low 16 bits only"""
    lists = lists_of(n, k, suffix)
    img, p = cell_image(lists.cell_keys)
    rng = np.random.default_rng(n)
    sets = R.cb_near_misses(lists, img, p, rng)
    ck = lists.cell_keys
    for name, keys in sets.items():
        assert len(keys) and (R.cell_index(ck, keys) == 0).all(), name
        assert not R.image_probe(img, p, keys).any(), name
    assert len(sets["slot_twins"]) >= 1000 and len(sets["lo_twins"]) >= 1000
    assert R.image_probe(img, p, sets["slot_twins"], "no_lo").all()
    assert R.image_probe(img, p, sets["family"], "no_family").all()
    assert R.image_probe(img, p, sets["low16"], "no_low16").all()
    # what the sets are made of: a family near miss keeps a listed code and zero low bits, and differs in bits 63:49 only
    listed_codes = set(R.code_of(ck).tolist())
    fam = sets["family"]
    assert all(c in listed_codes for c in R.code_of(fam).tolist()) and not (fam & np.uint64(0xFFFF)).any()
    assert ((fam >> np.uint64(49)) != np.uint64(int(p[2]))).all()
    assert len(fam) >= (10 if n <= 2 else 1000)
    low = sets["low16"]
    assert (R.cell_index(ck, low & ~np.uint64(0xFFFF)) > 0).all() and (low & np.uint64(0xFFFF)).all()
    # a lo twin lands on its listed key's displacement: same lo, another hi
    S, seed = int(p[0]), int(p[4])
    lo_of = lambda keys: set((R.cell_mix(R.code_of(keys), seed) & np.uint64((1 << (32 - S)) - 1)).tolist())
    assert lo_of(sets["lo_twins"]) <= lo_of(ck)


@pytest.mark.parametrize("n", [1000, 40_000, 70_000])
def test_l2_table_filter_and_chain_keys(n):
    """the restated open-addressed table finds every listed key; filter passers have their bit set; chain keys walk at least
    three slots to an empty one, and one chain crosses the end of the table, where listed keys were carried round"""
    lists = lists_of(n)
    ck = lists.cell_keys
    table, filt = R.l2_table(ck), R.filter_bits(ck)
    cap = len(table[0])
    assert cap >= 64 and cap >= 2 * n and cap < 4 * n + 128 and cap & (cap - 1) == 0
    assert len(filt) == {1000: 1 << 15, 40_000: 1 << 18, 70_000: 1 << 18}[n]
    for i in list(range(0, n, max(1, n // 500))) + [n - 1]:
        assert R.l2_probe(table, ck[i])[0] == i + 1
    assert R.in_filter(filt, ck).all()
    assert len(R.displaced_past_the_end(table)) >= 1
    rng = np.random.default_rng(n)
    passers = R.filter_passers(ck, filt, 1500, rng)
    assert len(passers) == 1500 and R.in_filter(filt, passers).all() and (R.cell_index(ck, passers) == 0).all()
    assert ((passers >> np.uint64(49)) == (ck[0] >> np.uint64(49))).all()
    for f in (None, filt):
        keys, heads = R.chain_keys(ck, table, f, rng)
        assert len(keys) >= 6 and any(h + ln > cap for h, ln in heads)
        crossed = 0
        for key in keys.tolist():
            v, seen = R.l2_probe(table, key)
            assert v == 0 and seen >= 3
            first = int(R.slot_hash(key)[0]) & (cap - 1)
            crossed += first + seen > cap
            assert f is None or R.in_filter(f, np.uint64(key)).all()
        assert crossed >= 3


def test_gene_lookup_is_the_dictionary():
    lists = lists_of(1000)
    fk = lists.feature_keys
    np.testing.assert_array_equal(R.gene_lookup(fk, fk), np.arange(1, len(fk) + 1))
    strs = R.gx_near_miss_strings(lists, b"ENSG", 11)
    keys = R.pack_gx(lists, strs)
    want = np.array([int(s[4:]) if s.startswith(b"ENSG") and len(s) == 15 and 1 <= int(s[4:]) <= 40 else 0 for s in strs])
    np.testing.assert_array_equal(R.gene_lookup(fk, keys), want)
    assert (want > 0).sum() == 2                              # vmin and vmax; everything else is a miss
    assert len(set(keys[keys != 0].tolist())) > 3 * 40        # ... of distinct non-zero keys: 40 numbers x 3 other digit counts, the edges
