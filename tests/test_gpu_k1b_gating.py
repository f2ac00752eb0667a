"""K1b's per-record gating (filter_pack_kernel, filter_pack_stream_kernel) against tests/k1b_ref.py on hand-built record and decision
streams: which decision bit a hit reads (its rank, *d_draw_base, the word and the bit), the META_* flags, the gene lookup, the shard
lists, the three counters and the error bits.  The streams are k1b_ref.fixtures() (tests/test_k1b_ref_host.py takes their census and
shows that each wrong placement rule changes some expected output); the decisions are passed as bits (FASTF_PROBE_DRAW_BITS) with 64
words of ones behind the stream: a word read from there keeps records the reference drops.

Every record carries a unique UMI (a NULL one a (cell, feature) pair of its own), so the sorted keys of a shard name its records."""
import time

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import hostmem
import k1b_ref as K
import lookup_ref as R
from test_gpu_lookup import DENSE, KNOBS, N_CELLS_K1B, SPARSE
from test_lookup_host import WRAP_SEED

pytestmark = pytest.mark.gpu

PRE = 3                                   # what d_key_counts holds before a call: the tile form appends, the streaming form sets
GUARD = 0x5A5A5A5A5A5A5A5A
EMPTY = -1                                # every key slot before a call

# form -> (list, environment, engine arguments, how K1b is called, table modes, block_bytes(256), cell scratch bytes)
LDS, L2 = "cells:LDS perfect hash genes:", "cells:L2 open addressing genes:L2 open addressing"
FORMS = {
    "tile, LDS genes, direct table": ("dense", {}, {}, "tile", LDS + "LDS direct table", 2560, 2),
    "tile, LDS genes, bitmap": ("dense", {"FASTF_GENES_NO_DIRECT": "1"}, {}, "tile", LDS + "LDS bitmap+rank", 2560, 2),
    "tile, L2 genes": ("dense", {"FASTF_LDS_TABLES": "0"}, {}, "tile", L2, 0, 2),
    "stream SoA": ("dense", {}, {}, "soa", LDS + "LDS direct table", 2560, 2),
    "stream blocked wide": ("dense", {"FASTF_BLOCK_WIDE": "1"}, {}, "blocked", LDS + "LDS direct table", 4608, 2),
    "stream blocked narrow": ("dense", {}, {}, "blocked", LDS + "LDS direct table", 2560, 2),
    "stream, 32-bit cell scratch": ("dense", {"FASTF_CELL_SCRATCH_32": "1"}, {}, "blocked", LDS + "LDS direct table", 3072, 4),
    "stream, sparse list": ("sparse", {}, {}, "blocked", LDS + "LDS bitmap+rank", 2560, 2),
    "tile, 2 shards": ("dense", {"FASTF_NO_STREAM_K1B": "1"}, {"n_shards": 2}, "tile", LDS + "LDS direct table", 0, 2),
    "tile, 8 shards": ("dense", {"FASTF_NO_STREAM_K1B": "1"}, {"n_shards": 8, "shard_rank": 5}, "tile", LDS + "LDS direct table", 0, 2),
    "stream + partition, 8 shards": ("dense", {}, {"n_shards": 8}, "tile", LDS + "LDS direct table", 4608, 2),
    "wide pairs, 20 bases": ("dense", {}, {"umi_max_bases": 20}, "wide", LDS + "LDS direct table", 0, 2),
}
_DATA, _WANT = {}, {}


def _data(kind, blob_bytes):
    """the lists and the records of one list kind: (lists, gx, umi, meta, ext, cell of a hit, feature of every record, unlisted CB keys)"""
    if (kind, blob_bytes) in _DATA:
        return _DATA[(kind, blob_bytes)]
    offs = DENSE if kind == "dense" else SPARSE
    lists = F.Lists(R.barcode_text(N_CELLS_K1B, WRAP_SEED[N_CELLS_K1B]), R.feature_text(R.id_strings(b"ENSG", 11, [1000 + o for o in offs])), 1.0, 926)
    assert lists.n_cells == N_CELLS_K1B and lists.n_features == len(offs)
    miss = [o for o in (97, 190, 3, 9, 5013, 8 * 30_000 + 1) if o not in set(offs)] + [-1]
    unlisted_gx = np.concatenate([np.zeros(1, np.uint64), R.pack_gx(lists, R.id_strings(b"ENSG", 11, [1000 + o for o in miss]))]).astype(np.uint64)
    other = R.barcode_text(8, 31337).split(b"\n")[:8]
    unlisted_cb = R.pack_cb(lists, other)
    assert (R.cell_index(lists.cell_keys, unlisted_cb) == 0).all() and (unlisted_cb != 0).all()
    gx, umi, meta, ext, cell_if_hit = K.build_records(N_CELLS_K1B, lists.feature_keys, unlisted_gx, blob_bytes=blob_bytes)
    feat = R.gene_lookup(lists.feature_keys, gx)
    tab = np.array(K.flag_table())[(29 * np.arange(len(gx))) % K.FLAG_PERIOD]
    assert ((feat > 0) == (tab[:, 3] == 1)).all() and len(unlisted_gx) >= 4          # listed keys are found, the others are not
    _DATA[(kind, blob_bytes)] = (lists, gx, umi, meta, ext, cell_if_hit, feat, unlisted_cb)
    return _DATA[(kind, blob_bytes)]


class Rig:
    """one engine of one form, its records on the device, and the guarded buffers of a call"""

    def __init__(self, monkeypatch, form):
        import torch
        self.torch, self.form = torch, form
        kind, env, kw, self.call, modes, bb, csb = FORMS[form]
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        self.bases = kw.get("umi_max_bases", 12)
        self.kind, self.blob = kind, (self.bases + 3) // 4
        self.lists, self.gx, self.umi, self.meta, self.ext, self.cell_if_hit, self.feat, self.unlisted_cb = _data(kind, self.blob)
        self.eng = F.Engine.from_lists(self.lists, rate_depth=0.5, **kw)
        try:
            eng = self.eng
            self.G = eng.n_shards
            # the instantiation this form names
            assert eng.table_modes == modes and eng.cell_scratch_bytes == csb and eng.block_bytes(256) == bb, (eng.table_modes, eng.block_bytes(256))
            assert (eng.probe_capacity(256) > 0) == (bb > 0 and self.G == 1)
            if kind == "sparse":                                     # over 78 KB of gene image: one workgroup per CU, the ROOMY build
                words = len(R.bitmap_words(R.family_values(self.lists, b"ENSG", 11)))
                assert 4 * words + 2 * ((words + 1) & ~1) + 2 * len(SPARSE) > 78 * 1024
            self.L = K.Layout.of_engine(eng, self.bases)
            assert self.L.wide == (self.call == "wide")
            dev = lambda a: hostmem.to_device(a, "cuda")
            self.d_gx, self.d_umi, self.d_meta = dev(self.gx), dev(self.umi), dev(self.meta)
            self.d_ext = dev(self.ext) if self.ext is not None else None
            self.blk = {}
            self.s = torch.cuda.current_stream().cuda_stream
        except BaseException:
            self.eng.close()
            raise

    def close(self):
        self.eng.close()

    def cb(self, mask):
        return K.cb_keys(mask, self.cell_if_hit, self.lists.cell_keys, self.unlisted_cb)

    def bits_on_device(self, bits):
        words = K.pack_bits(bits)
        buf = np.concatenate([words, np.full(K.GUARD_WORDS, 0xFFFFFFFF, np.uint32)])
        d = hostmem.to_device(buf, "cuda")
        assert d.data_ptr() % 8 == 0
        return d

    def run(self, n, cb, d_bits, n_draws, base, stride=None, draw_bits=True, pre=PRE):
        """one K1b call over records [0, n) -> (per shard: sorted keys [, values], key counts, counters); checks every guard word"""
        torch, eng, G, s = self.torch, self.eng, self.G, self.s
        d_cb = hostmem.to_device(cb, "cuda")
        small = torch.full((48,), GUARD, dtype=torch.int64, device="cuda")        # key counts at 0, counters at 16, the draw base at 32
        small[0:G] = pre; small[16:20] = 0; small[32] = base
        kc, ctr, db = small[0:G], small[16:20], small[32:33]
        streaming = self.call in ("soa", "blocked")
        if streaming:
            slots = max(n, eng.probe_capacity(n))
            assert eng.probe_capacity(n) > 0
        else:
            slots = n + pre if stride is None else stride
        d_keys = torch.full((G * slots + 64,), EMPTY, dtype=torch.int64, device="cuda")
        d_vals = torch.full((G * slots + 64,), EMPTY, dtype=torch.int64, device="cuda")
        if self.call == "tile":
            eng.dev_probe_pack(d_cb.data_ptr(), self.d_gx.data_ptr(), self.d_umi.data_ptr(), self.d_meta.data_ptr(), n, d_bits.data_ptr(), n_draws,
                               d_keys.data_ptr(), slots, kc.data_ptr(), ctr.data_ptr(), stream=s, d_draw_base=db.data_ptr(), draw_bits=draw_bits)
        elif self.call == "wide":
            eng.dev_probe_pack_wide(d_cb.data_ptr(), self.d_gx.data_ptr(), self.d_umi.data_ptr(), self.d_meta.data_ptr(), self.d_ext.data_ptr(), n,
                                    d_bits.data_ptr(), n_draws, d_keys.data_ptr(), d_vals.data_ptr(), slots, kc.data_ptr(), ctr.data_ptr(), stream=s,
                                    d_draw_base=db.data_ptr(), draw_bits=draw_bits)
        else:
            blocked = self.call == "blocked"
            if blocked and n not in self.blk:
                self.blk[n] = torch.zeros(eng.block_bytes(n), dtype=torch.uint8, device="cuda")
                eng.dev_block_records(self.d_gx.data_ptr(), self.d_umi.data_ptr(), self.d_meta.data_ptr(), n, self.blk[n].data_ptr(), s)
            d_tmp = torch.full((slots + 64,), EMPTY, dtype=torch.int64, device="cuda")
            if blocked:
                eng.dev_probe_pack(d_cb.data_ptr(), self.blk[n].data_ptr(), 0, 0, n, d_bits.data_ptr(), n_draws, d_keys.data_ptr(), slots, kc.data_ptr(),
                                   ctr.data_ptr(), stream=s, d_draw_base=db.data_ptr(), segmented=True, blocked=True, draw_bits=draw_bits)
            else:
                eng.dev_probe_pack(d_cb.data_ptr(), self.d_gx.data_ptr(), self.d_umi.data_ptr(), self.d_meta.data_ptr(), n, d_bits.data_ptr(), n_draws,
                                   d_keys.data_ptr(), slots, kc.data_ptr(), ctr.data_ptr(), stream=s, d_draw_base=db.data_ptr(), segmented=True,
                                   draw_bits=draw_bits)
            torch.cuda.synchronize()
            raw = hostmem.to_host(d_keys)
            count = int(hostmem.to_host(small)[0])
            assert (raw[slots:] == EMPTY).all(), "key slots behind the regions were written"
            assert 0 <= count <= n and int((raw != EMPTY).sum()) == count, "the regions hold another number of keys than d_key_counts says"
            in_tmp = eng.dev_sort(d_keys.data_ptr(), d_tmp.data_ptr(), kc.data_ptr(), n, stream=s, skip_low=True, segmented=True)
            torch.cuda.synchronize()
            assert (hostmem.to_host(d_tmp)[slots:] == EMPTY).all() and (hostmem.to_host(d_keys)[slots:] == EMPTY).all()
            sm = hostmem.to_host(small)
            assert (sm[1:16] == GUARD).all() and (sm[20:32] == GUARD).all() and (sm[33:] == GUARD).all() and sm[32] == base
            keys = np.sort(hostmem.to_host(d_tmp if in_tmp else d_keys).view(np.uint64)[:count])
            return [keys], [np.zeros(count, np.uint64)], [count], [int(x) for x in sm[16:20]]
        torch.cuda.synchronize()
        sm = hostmem.to_host(small)
        assert (sm[G:16] == GUARD).all() and (sm[20:32] == GUARD).all() and (sm[33:] == GUARD).all() and sm[32] == base
        raw, rawv = hostmem.to_host(d_keys), hostmem.to_host(d_vals)
        assert (raw[G * slots:] == EMPTY).all() and (rawv[G * slots:] == EMPTY).all(), "slots behind the last list were written"
        keys, vals, counts = [], [], []
        for sh in range(G):
            lst, lv = raw[sh * slots:(sh + 1) * slots], rawv[sh * slots:(sh + 1) * slots]
            c = int(sm[sh]) - pre
            counts.append(c)
            used = lst != EMPTY
            if c + pre <= slots:                                     # the list holds its keys behind what it held before, and nothing else
                assert not used[:pre].any() and used[pre:pre + c].all() and not used[pre + c:].any(), "shard %d" % sh
            if self.call == "wide":
                assert ((lv != EMPTY) == used).all()
                o = np.lexsort((lv[used].view(np.uint64), lst[used].view(np.uint64)))
                keys.append(lst[used].view(np.uint64)[o]); vals.append(lv[used].view(np.uint64)[o])
            else:
                assert (rawv == EMPTY).all()
                keys.append(np.sort(lst[used].view(np.uint64))); vals.append(np.zeros(int(used.sum()), np.uint64))
        return keys, vals, counts, [int(x) for x in sm[16:20]]

    def want(self, n, mask, bits, base, n_draws, stride=None, meta=None, cache=None):
        key = (self.kind, self.L.ident(), self.G, cache)
        if cache is not None and key in _WANT:
            return _WANT[key]
        cell = np.where(mask, self.cell_if_hit[:n], 0)
        assert (R.cell_index(self.lists.cell_keys, self.cb(mask)) == cell).all()
        r = K.k1b(cell, self.feat[:n], self.umi[:n], (self.meta if meta is None else meta)[:n], bits, base, n_draws, self.L, n_shards=self.G,
                  shard_stride=stride, ext=None if self.ext is None else self.ext[:n])
        if cache is not None:
            _WANT[key] = r
        return r

    def check(self, got, want, what):
        keys, vals, counts, counters = got
        assert counters[:3] == list(want.counters), what
        assert counts == [len(k) for k in want.keys], what
        for sh in range(self.G):
            np.testing.assert_array_equal(keys[sh], want.keys[sh], err_msg="%s, shard %d" % (what, sh))
            np.testing.assert_array_equal(vals[sh], want.vals[sh], err_msg="%s, shard %d" % (what, sh))


@pytest.mark.parametrize("form", list(FORMS))
def test_k1b_gating_on_every_fixture(form, monkeypatch):
    rig = Rig(monkeypatch, form)
    try:
        t0, n_keys = time.time(), 0
        for fx in K.fixtures():
            mask, bits, nd = fx.mask(), fx.stream(), fx.n_draws()
            want = rig.want(fx.n, mask, bits, fx.base, nd, cache=fx.name)
            assert want.err == 0
            got = rig.run(fx.n, rig.cb(mask), rig.bits_on_device(bits), nd, fx.base)
            rig.check(got, want, fx.name)
            assert got[3][3] == 0 and rig.eng.dev_error_bits() == 0, fx.name
            n_keys += sum(got[2])
        print("%s: %d fixtures, %d keys, %.2f s" % (form, len(K.fixtures()), n_keys, time.time() - t0))
        assert n_keys > 20_000
    finally:
        rig.close()


ERR_FX = K.Fixture(4097, "all", "random", 33)


@pytest.mark.parametrize("form", list(FORMS))
def test_a_stream_one_decision_short_raises_bit_2(form, monkeypatch):
    """n_draws = draw_base + hits - 1.  Both kernels count the last hit in `hits` (filter_pack_kernel: n_hit++ on the branch that
    drops it; filter_pack_stream_kernel: w_hit += H in front of the clamp) and neither in `sampled`: one expectation for both"""
    rig = Rig(monkeypatch, form)
    try:
        fx = ERR_FX
        mask, bits, nd = fx.mask(), fx.stream()[:-1], fx.n_draws() - 1
        want = rig.want(fx.n, mask, bits, fx.base, nd)
        full = rig.want(fx.n, mask, fx.stream(), fx.base, nd + 1, cache=fx.name)
        assert want.err == K.ERR_DRAWS_SHORT and want.counters[0] == full.counters[0] == fx.n
        got = rig.run(fx.n, rig.cb(mask), rig.bits_on_device(bits), nd, fx.base)
        rig.check(got, want, "one decision short")
        assert got[3][3] == K.ERR_DRAWS_SHORT and rig.eng.dev_error_bits() == 0      # (the bit goes to the caller's counters)
        # no key of the last hit: its UMI number is in no key
        if not rig.L.wide:
            umis = np.concatenate(got[0]) >> np.uint64(rig.L.lb) & np.uint64((1 << 24) - 1)
            assert fx.n not in set(umis.tolist()) and fx.n - 1 in set(umis.tolist())
        rig.eng.dev_clear_error_bits(0xFFFF)
    finally:
        rig.close()


@pytest.mark.parametrize("form", list(FORMS))
def test_a_too_long_umi_raises_bit_4_only_where_the_record_is_kept(form, monkeypatch):
    """one record that passes xf, GX and UB carries a UMI the key cannot hold — flagged so by the packer, or with more blob bytes than
    the length field counts: silent while the draw drops it (the LDS-genes path looks its gene up ahead of the draw), bit 4 when its
    decision bit is set"""
    rig = Rig(monkeypatch, form)
    try:
        fx = ERR_FX
        mask = fx.mask()
        tab = np.array(K.flag_table())[(29 * np.arange(fx.n)) % K.FLAG_PERIOD]
        cand = np.nonzero((tab[:, 0] == 1) & (tab[:, 1] == 1) & (tab[:, 2] == 1) & (tab[:, 3] == 1))[0]
        for at, how in ((int(cand[3]), "flag"), (int(cand[len(cand) // 2]), "length"), (fx.n - 1 if fx.n - 1 in set(cand.tolist()) else int(cand[-1]), "flag")):
            meta = rig.meta.copy()
            if how == "flag":
                meta[at] |= K.UMI_TOOLONG
            else:
                meta[at] = (meta[at] & ~np.uint32(0xF0)) | np.uint32((rig.L.max_bytes + 1) << K.LEN_SHIFT)
            d_meta, blk = rig.d_meta, rig.blk
            rig.d_meta, rig.blk = hostmem.to_device(meta, "cuda"), {}
            try:
                for bit in (0, 1):
                    bits = fx.stream()
                    bits[fx.base + at] = bit                        # (all records hit: record `at` has rank base + at)
                    want = rig.want(fx.n, mask, bits, fx.base, fx.n_draws(), meta=meta)
                    assert want.err == (K.ERR_UMI_TOOLONG if bit else 0)
                    got = rig.run(fx.n, rig.cb(mask), rig.bits_on_device(bits), fx.n_draws(), fx.base)
                    assert got[3][:3] == list(want.counters), (how, at, bit)
                    assert got[3][3] == want.err, "record %d (%s), decision bit %d: error bits %d" % (at, how, bit, got[3][3])
                    if not bit:
                        rig.check(got, want, "too long, dropped by the draw")
            finally:
                rig.d_meta, rig.blk = d_meta, blk
        assert rig.eng.dev_error_bits() == 0
        rig.eng.dev_clear_error_bits(0xFFFF)
    finally:
        rig.close()


@pytest.mark.parametrize("form", ["tile, LDS genes, direct table", "tile, L2 genes", "tile, 8 shards"])
def test_a_full_shard_list_raises_bit_8_and_writes_nothing_past_it(form, monkeypatch):
    rig = Rig(monkeypatch, form)
    try:
        fx = ERR_FX
        mask, bits, nd = fx.mask(), fx.stream(), fx.n_draws()
        free = rig.want(fx.n, mask, bits, fx.base, nd, cache=fx.name)
        sizes = [len(k) for k in free.keys]
        stride = max(sizes) - 1                                      # one below the fullest shard's key count
        want = rig.want(fx.n, mask, bits, fx.base, nd, stride=stride)
        assert want.err == K.ERR_KEYS_FULL and stride > 0
        keys, vals, counts, counters = rig.run(fx.n, rig.cb(mask), rig.bits_on_device(bits), nd, fx.base, stride=stride, pre=0)
        assert counters == list(want.counters) + [K.ERR_KEYS_FULL]
        over = [sh for sh in range(rig.G) if sizes[sh] > stride]
        assert over and (rig.G == 1 or len(over) < rig.G)
        for sh in range(rig.G):
            if sh in over:                                           # whole tiles of keys are left out, none is invented or doubled
                assert len(keys[sh]) <= stride and len(np.unique(keys[sh])) == len(keys[sh]) and np.isin(keys[sh], want.keys[sh]).all()
            else:
                assert counts[sh] == sizes[sh]
                np.testing.assert_array_equal(keys[sh], want.keys[sh])
        assert rig.eng.dev_error_bits() == 0
        rig.eng.dev_clear_error_bits(0xFFFF)
    finally:
        rig.close()


DRAW_NS = [1, 63, 64, 65, 2049]


def test_draw_bits_against_numpy_and_the_32_bit_draws_path(monkeypatch):
    import torch
    rig = Rig(monkeypatch, "tile, LDS genes, direct table")
    try:
        eng = rig.eng
        t = F.draw_threshold(0.5)
        assert 0 < t < 1 << 32
        cyc = np.array([t - 1, t, 0, 0xFFFFFFFF], np.uint64).astype(np.uint32)
        for n in DRAW_NS:
            draws = np.resize(cyc, n)
            if n > 64:
                draws = np.concatenate([draws[:64], np.random.default_rng(n).integers(0, 1 << 32, size=n - 64, dtype=np.uint64).astype(np.uint32)])
                draws[-1] = t - 1
            words = (n + 63) // 64 * 2
            d_out = torch.full((words + 2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            assert d_out.data_ptr() % 8 == 0
            eng.dev_draw_bits(hostmem.to_device(draws, "cuda").data_ptr(), n, d_out.data_ptr())
            torch.cuda.synchronize()
            got = hostmem.to_host(d_out).view(np.uint32)
            np.testing.assert_array_equal(got[:words], K.pack_bits((draws.astype(np.uint64) < np.uint64(t)).astype(np.uint8)), err_msg="n=%d" % n)
            assert (got[words:] == 0x5A5A5A5A).all()
        # the same call with 32-bit draws and with their decisions made by numpy
        fx = K.Fixture(4097, "period3", "random", 33)
        mask, nd = fx.mask(), fx.n_draws()
        draws = np.resize(cyc, nd)
        bits = (draws.astype(np.uint64) < np.uint64(t)).astype(np.uint8)
        assert bits[:4].tolist() == [1, 0, 1, 0]
        want = rig.want(fx.n, mask, bits, fx.base, nd)
        d_draws = hostmem.to_device(np.concatenate([draws, np.zeros(64, np.uint32)]), "cuda")          # (zeros behind: draws that would keep)
        for d, as_bits in ((d_draws, False), (rig.bits_on_device(bits), True)):
            got = rig.run(fx.n, rig.cb(mask), d, nd, fx.base, draw_bits=as_bits)
            rig.check(got, want, "draw_bits=%s" % as_bits)
            assert got[3][3] == 0
        assert eng.dev_error_bits() == 0
    finally:
        rig.close()
