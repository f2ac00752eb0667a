"""The barcode lookup (K1a) and the gene lookup (K1b) per record, against tests/lookup_ref.py, on keys built to be near misses for
the very image and tables the engine built from its lists: slot and lo twins of the LDS perfect hash, keys that keep a listed
32-bit code under another family, keys the miss filter lets through, keys that walk the longest and the wrapping probe chain of
the L2 table; gene numbers at the edges of the id range and of the bitmap words, other prefixes and digit counts.

K1a: the cell index of every record is read back from the scratch slices of a blocked buffer.  K1b: with every record a listed
CB hit, a good xf, rate 1 and a UMI that is unique in its cell, every output key names one record and its feature index."""
import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import hostmem, synth
import lookup_ref as R
from test_lookup_host import WRAP_SEED, cell_image, lists_of

pytestmark = pytest.mark.gpu

NARROW_RUNS, WIDE_RUNS = (2560, 3072), (4608, 5120)
KNOBS = ["FASTF_CELL_SCRATCH_32", "FASTF_NO_CELL_FILTER", "FASTF_LDS_CELLS", "FASTF_LDS_CELLS_MAX", "FASTF_LDS_TABLES", "FASTF_GENES_NO_DIRECT",
         "FASTF_GENES_LDS_MAX_KB", "FASTF_BLOCK_WIDE", "FASTF_NO_STREAM_K1B", "FASTF_PUSH_TILE_FORM", "FASTF_FORCE_WIDE_KEYS"]


def _engine(monkeypatch, lists, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return F.Engine.from_lists(lists, umi_max_bases=12)


# ------------------------------------------------------------------ K1a
# name, cells, environment, LDS perfect hash, workgroups per CU of the LDS kernel (by make_cell_image's size rule), scratch bytes
K1A_CASES = [
    ("lds two per CU", 1000, {}, True, 2, 2),
    ("lds two per CU, largest image", 12288, {}, True, 2, 2),         # 64 KB of slots + 8 KB of displacements
    ("lds 16383 cells", 16383, {}, True, 1, 2),                       # 64 KB + 16 KB (+ 64) is over the 80 KB of the two-per-CU build
    ("lds one per CU", 32767, {}, True, 1, 2),
    ("lds one per CU, uint2 stores", 32767, {"FASTF_CELL_SCRATCH_32": "1"}, True, 1, 4),
    ("filter + L2", 40_000, {}, False, 0, 2),
    ("plain L2", 40_000, {"FASTF_NO_CELL_FILTER": "1"}, False, 0, 2),
    ("filter + L2, small table", 1000, {"FASTF_LDS_CELLS": "0"}, False, 0, 2),
    ("32-bit scratch by necessity", 70_000, {}, False, 0, 4),
]
K1A_LENGTHS = [1, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 8193]       # unit (256), chunk (512) and tile (4096) edges


def _k1a_streams(ck, sets, rng):
    """record streams of CB keys: near misses interleaved with listed keys at the edge lengths (from 4095 on behind 700 hits
    and 700 misses in a row: whole chunks of hits, whole chunks without one), and one of about 70 000 records that holds every
    listed key in list order, every near miss, and the interleaved part"""
    miss = np.concatenate([sets[k] for k in sorted(sets)])
    miss = miss[rng.permutation(len(miss))]
    m = max(len(miss), len(ck), 4200)
    inter = np.empty(2 * m, np.uint64)
    inter[0::2], inter[1::2] = np.resize(miss, m), np.resize(ck, m)
    runs = np.concatenate([np.resize(ck, 700), np.resize(miss, 700), inter])
    out = [(inter if n < 4095 else runs)[:n] for n in K1A_LENGTHS]
    big = np.concatenate([ck, miss, inter[:2000]])
    out.append(np.resize(big, max(len(big), 70_001)))
    return out


def _k1a_run(torch, eng, n_cells, csb, cb, want, unaligned):
    n = len(cb)
    if unaligned:                                            # cb 8 bytes into a larger tensor: the kernel's 16-byte loads are out
        d_cb = hostmem.to_device(np.concatenate([np.full(1, 0x4000000000000000, np.uint64), cb]), "cuda")[1:]
    else:
        d_cb = hostmem.to_device(cb, "cuda")
    assert d_cb.data_ptr() % 16 == (8 if unaligned else 0)
    rb, units = eng.block_bytes(256), (n + 255) // 256
    assert rb in NARROW_RUNS and rb == 2048 + 256 * csb and eng.block_bytes(n) == units * rb
    blk = torch.full((units * rb,), 0xA5, dtype=torch.uint8, device="cuda")
    z8, z4 = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    hits = torch.zeros(1, dtype=torch.int64, device="cuda")
    eng.dev_block_records(z8.data_ptr(), z4.data_ptr(), z4.data_ptr(), n, blk.data_ptr())
    eng.dev_count_hits_blocked(d_cb.data_ptr(), n, blk.data_ptr(), hits.data_ptr())
    torch.cuda.synchronize()
    raw = np.ascontiguousarray(hostmem.to_host(blk).reshape(units, rb)[:, rb - 256 * csb:])
    scratch = raw.view(np.uint16 if csb == 2 else np.uint32).reshape(-1).astype(np.int64)
    bad = np.nonzero(scratch[:n] != want)[0]
    assert len(bad) == 0, "n=%d: %d records differ, first at %d: key %#x got %d want %d" % (
        n, len(bad), bad[0], int(cb[bad[0]]), scratch[bad[0]], want[bad[0]])
    assert (scratch[n:] == (0xA5A5 if csb == 2 else 0xA5A5A5A5)).all(), "scratch entries behind the last record were written"
    assert int(hits.item()) == int((want > 0).sum())
    # the SoA form of the same pass: hits per cell from the engine's own scratch array
    hits.zero_()
    eng.dev_count_hits(d_cb.data_ptr(), n, hits.data_ptr())
    d_h = torch.full((n_cells + 2,), 0x55555555, dtype=torch.int32, device="cuda")
    eng.dev_cell_hits(n, 0, d_h.data_ptr())
    torch.cuda.synchronize()
    got = hostmem.to_host(d_h).view(np.uint32).astype(np.int64)
    np.testing.assert_array_equal(got[:n_cells], np.bincount(want[want > 0] - 1, minlength=n_cells), err_msg="n=%d" % n)
    assert (got[n_cells:] == 0x55555555).all() and int(hits.item()) == int((want > 0).sum())
    assert eng.dev_error_bits() == 0


@pytest.mark.parametrize("name,n_cells,env,lds,per_cu,csb", K1A_CASES, ids=[c[0] for c in K1A_CASES])
def test_k1a_cell_index_of_every_record(name, n_cells, env, lds, per_cu, csb, monkeypatch):
    import torch
    lists = lists_of(n_cells)
    ck = lists.cell_keys
    eng = _engine(monkeypatch, lists, env)
    try:
        assert eng.table_modes.split(" genes:")[0] == ("cells:LDS perfect hash" if lds else "cells:L2 open addressing")
        assert eng.cell_scratch_bytes == csb
        img, p = cell_image(ck)
        assert (img is not None) == (n_cells <= 32767)
        if lds:
            assert (2 if len(img) + 64 <= 80 * 1024 else 1) == per_cu
        table = filt = None
        if not lds:
            assert n_cells in WRAP_SEED
            table = R.l2_table(ck)
            filt = None if "FASTF_NO_CELL_FILTER" in env else R.filter_bits(ck)
        rng = np.random.default_rng(n_cells)
        sets = R.cb_near_misses(lists, img, p, rng, table, filt)
        if img is not None:
            assert len(sets["slot_twins"]) >= 1000 and len(sets["lo_twins"]) >= 1000
            assert R.image_probe(img, p, sets["slot_twins"], "no_lo").all() and R.image_probe(img, p, sets["family"], "no_family").all()
            assert R.image_probe(img, p, sets["low16"], "no_low16").all()
        if table is not None:
            assert all(R.l2_probe(table, k)[1] >= 3 for k in sets["chain"].tolist())
            assert len(R.displaced_past_the_end(table)) >= 1
        if filt is not None:
            assert R.in_filter(filt, sets["filter_passers"]).all() and R.in_filter(filt, sets["chain"]).all()
        for cb in _k1a_streams(ck, sets, rng):
            want = R.cell_index(ck, cb)
            if len(cb) > 70_000:
                assert set(want.tolist()) == set(range(n_cells + 1))       # every index is returned, 0 and n included
            _k1a_run(torch, eng, n_cells, csb, cb, want, False)
            if lds:
                _k1a_run(torch, eng, n_cells, csb, cb, want, True)
    finally:
        eng.close()


# ------------------------------------------------------------------ K1b
N_CELLS_K1B, K1B_LENGTHS = 1000, [1, 257, 4097, 40_001]
# offsets from vmin of the listed ids of the dense family: [0, 5013) without four holes — next to a listed bit 0 (offset 96) and a
# listed bit 31 (191), at bit 0 (224) and at bit 31 (319) of a word; word 2 is full, the last word holds 21 ids
DENSE_HOLES = (97, 190, 224, 319)
DENSE = [o for o in range(5013) if o not in DENSE_HOLES]
# every eighth id (the sparse range of a real list), one stretch of 64 consecutive ids (two full words), and bit 31 of a word
SPARSE = sorted(set(range(0, 8 * 30_000, 8)) | set(range(3200, 3264)) | {32 * 200 + 31})


def _plain_names(n):
    return [b"plain_" + bytes(97 + (i // 26 ** j) % 26 for j in range(3)) for i in range(n)]


def _gene_ids(kind):
    if kind in ("dense", "l2"):
        return R.id_strings(b"ENSG", 11, [1000 + o for o in DENSE])
    if kind == "sparse":
        return R.id_strings(b"ENSG", 11, [1000 + o for o in SPARSE])
    if kind == "high":                                       # the id range ends at 2^32 - 2: the last number a NARROW run can carry
        return R.id_strings(b"ENSG", 11, [(1 << 32) - 2 - 5012 + o for o in DENSE])
    if kind == "mixed":                                      # a majority family, a minority prefix, another digit count, plain names
        ids = R.id_strings(b"ENSG", 11, [1000 + o for o in DENSE[:3000]])
        mus = R.id_strings(b"ENSMUSG", 11, range(1000, 1500))
        short = R.id_strings(b"ENSG", 9, range(1000, 1100))
        rng = np.random.default_rng(3)
        ids = ids + mus + short + _plain_names(200)
        return [ids[i] for i in rng.permutation(len(ids))]
    raise KeyError(kind)


# structure -> (list kind, environment, table mode of the genes, one ID family)
GENE_CASES = {
    "direct table": ("dense", {}, "LDS direct table", True),
    "bitmap": ("dense", {"FASTF_GENES_NO_DIRECT": "1"}, "LDS bitmap+rank", True),
    "bitmap, one workgroup per CU": ("sparse", {}, "LDS bitmap+rank", True),
    "L2 table": ("l2", {"FASTF_LDS_TABLES": "0"}, "L2 open addressing", True),
    "minority family and plain names": ("mixed", {}, "LDS direct table", False),
    "ids up to 2^32 - 2": ("high", {}, "LDS direct table", True),
}
_K1B = {}


def _k1b_data(kind):
    """lists and N packed records: record i is a hit of cell i % 1000 + 1 with UMI number i; its GX is a listed id or a near miss"""
    if kind in _K1B:
        return _K1B[kind]
    ids = _gene_ids(kind)
    lists = F.Lists(R.barcode_text(N_CELLS_K1B, WRAP_SEED[N_CELLS_K1B]), R.feature_text(ids), 1.0, 926)
    assert len(lists.feature_keys) == len(ids) and len(lists.cell_keys) == N_CELLS_K1B
    rng = np.random.default_rng(len(ids))
    vals = R.family_values(lists, b"ENSG", 11)
    words = R.bitmap_words(vals)
    assert (words == 0xFFFFFFFF).any() and (words & 1).any() and (words >> 31).any() and (int(vals.max()) - int(vals.min()) + 1) % 32 != 0
    near = R.gx_near_miss_strings(lists, b"ENSG", 11, other_prefixes=(b"ENSMUSG",) if kind == "mixed" else (), rng=rng)
    rest = near + ids[1:]
    seq = [ids[0]] + [rest[i] for i in rng.permutation(len(rest))]
    n = K1B_LENGTHS[-1]
    assert len(seq) <= n                                      # the long stream holds every listed id and every near miss
    gx = synth.as_cstr(np.resize(np.array(seq, dtype="S"), n))
    cell = np.arange(n) % N_CELLS_K1B + 1
    cb = synth.as_cstr(np.array(lists.barcodes, dtype="S")[cell - 1])
    ub = synth._as_S(synth._kmers(np.arange(n, dtype=np.uint64), 12), 13)
    cbk, gxk, umi, meta = F.pack_records(lists, np.full(n, 15, np.uint8), np.full(n, 25, np.int32), cb, gx, ub)
    np.testing.assert_array_equal(cbk, lists.cell_keys[cell - 1])
    assert ((meta & 0xF) == 0x7).all() and len(np.unique(umi)) == n
    feat = R.gene_lookup(lists.feature_keys, gxk)
    assert set(feat.tolist()) == set(range(len(ids) + 1))     # every feature index is expected at least once, and misses
    miss_keys = np.unique(gxk[feat == 0])
    assert len(miss_keys) > 400 and miss_keys[0] == 0
    _K1B[kind] = (lists, cell, feat, (cbk, gxk, umi, meta))
    return _K1B[kind]


def _k1b_expected(eng, cell, feat, umi, meta, n):
    """make_key of (cell, feature, umi, meta) for the records with a feature: [cell][feature][nonnull 1][umi 24][len 2]"""
    ub, lb = 24, 2                                           # 12 bases; the blob length (0..3 bytes) takes two bits
    fs = eng.umi_bits                                        # (the engine reports the whole field below the feature: flag + UMI + length)
    cs = fs + eng.feature_bits
    assert fs == 1 + ub + lb and eng.key_bits == cs + eng.cell_bits <= 64
    U = np.uint64
    nn = ((meta[:n] >> 2) & 1).astype(U)
    low = (nn << U(ub + lb)) | ((umi[:n].astype(U) >> U(32 - ub)) << U(lb)) | ((meta[:n].astype(U) & U(0xF0)) >> U(4))
    keys = (cell[:n].astype(U) << U(cs)) | (feat[:n].astype(U) << U(fs)) | (low * nn)
    return keys[feat[:n] > 0]


def _k1b_run(torch, eng, d, n, form):
    s = torch.cuda.current_stream().cuda_stream
    small = torch.zeros(16, dtype=torch.int64, device="cuda")
    kc, ctr = small[0:1], small[8:12]
    draws = torch.zeros(n, dtype=torch.int32, device="cuda")              # rate 1: the threshold is 2^32, every draw keeps its record
    if form == "tile":
        d_keys = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        eng.dev_probe_pack(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, draws.data_ptr(), n,
                           d_keys.data_ptr(), n, kc.data_ptr(), ctr.data_ptr(), stream=s)
        src = d_keys
    else:
        slots = max(n, eng.probe_capacity(n))
        assert eng.probe_capacity(n) > 0 and eng.block_bytes(n) > 0
        d_keys = torch.full((slots,), -1, dtype=torch.int64, device="cuda")
        d_tmp = torch.full((slots,), -1, dtype=torch.int64, device="cuda")
        blk = torch.zeros(eng.block_bytes(n), dtype=torch.uint8, device="cuda")
        eng.dev_block_records(d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, blk.data_ptr(), s)
        eng.dev_probe_pack(d[0].data_ptr(), blk.data_ptr(), 0, 0, n, draws.data_ptr(), n, d_keys.data_ptr(), slots, kc.data_ptr(),
                           ctr.data_ptr(), stream=s, segmented=True, blocked=True)
        in_tmp = eng.dev_sort(d_keys.data_ptr(), d_tmp.data_ptr(), kc.data_ptr(), n, stream=s, skip_low=True, segmented=True)
        src = d_tmp if in_tmp else d_keys
    torch.cuda.synchronize()
    sm = hostmem.to_host(small)
    count = int(sm[0])
    assert 0 <= count <= n
    return hostmem.to_host(src).view(np.uint64)[:count], count, [int(x) for x in sm[8:12]]


# (the streaming form reads the gene image in LDS: the L2 structure has the tile form only)
K1B_RUNS = [(s, f) for s in GENE_CASES for f in ("tile", "stream narrow", "stream wide") if f == "tile" or GENE_CASES[s][2] != "L2 open addressing"]


@pytest.mark.parametrize("structure,form", K1B_RUNS, ids=["%s-%s" % r for r in K1B_RUNS])
def test_k1b_feature_index_of_every_record(structure, form, monkeypatch):
    import torch
    kind, env, mode, one_family = GENE_CASES[structure]
    lists, cell, feat, packed = _k1b_data(kind)
    eng = _engine(monkeypatch, lists, dict(env, **({"FASTF_BLOCK_WIDE": "1"} if form == "stream wide" else {})))
    try:
        assert eng.table_modes == "cells:%s genes:%s" % ("L2 open addressing" if "FASTF_LDS_TABLES" in env else "LDS perfect hash", mode)
        if mode == "L2 open addressing":
            assert eng.block_bytes(256) == 0 and eng.probe_capacity(256) == 0          # no streaming K1b without the LDS image
        else:
            narrow = form != "stream wide" and one_family
            assert eng.block_bytes(256) == (NARROW_RUNS if narrow else WIDE_RUNS)[0]
        if kind == "sparse":                                     # bitmap + rank + permutation: over 78 KB, one workgroup per CU
            vals = R.family_values(lists, b"ENSG", 11)
            words = len(R.bitmap_words(vals))
            assert 4 * words + 2 * ((words + 1) & ~1) + 2 * len(vals) > 78 * 1024
        d = [hostmem.to_device(x, "cuda") for x in packed]
        for n in K1B_LENGTHS:
            want = _k1b_expected(eng, cell, feat, packed[2], packed[3], n)
            got, count, counters = _k1b_run(torch, eng, d, n, form)
            assert counters == [n, n, len(want), 0], "n=%d" % n
            assert count == len(want), "n=%d" % n
            np.testing.assert_array_equal(np.sort(got), np.sort(want), err_msg="n=%d" % n)
            assert eng.dev_error_bits() == 0
    finally:
        eng.close()
