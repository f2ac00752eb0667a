"""`fastF cap` on the GPU: the hits per cell (fastf_dev_cell_hits) against np.bincount, the per-cell decision plane
(fastf_dev_cell_decisions) against mt_stream < T[cell], and the command — through the CLI and in process — with every point's
three files against cap_ref (the unchanged oracle on masked records) and every cap.tsv row against numpy."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, cap, hostmem, synth
from helpers import Case
from oracle import oracle as O
import cap_ref
from test_gpu_sweep import _Edge, _write
import test_cap_host as H

pytestmark = pytest.mark.gpu

NARROW_RUNS, WIDE_RUNS = (2560, 3072), (4608, 5120)
MT_PAR_MIN = 4 * 624 * 256


@pytest.fixture(params=["soa", "narrow", "wide"])
def layout(request, monkeypatch):
    if request.param == "wide":
        monkeypatch.setenv("FASTF_BLOCK_WIDE", "1")
    else:
        monkeypatch.delenv("FASTF_BLOCK_WIDE", raising=False)
    return request.param


_LISTS = {}


def _lists(n_bar):
    if n_bar not in _LISTS:
        bt, ft, _, _ = synth.make_lists(n_bar, 40, seed=1000 + n_bar)
        _LISTS[n_bar] = F.Lists(bt, ft, 1.0, 926)
    return _LISTS[n_bar]


class _Dev:
    """records whose cell index is cell[i] (0: a CB that is absent or not listed) on the device, K1a run over them"""

    def __init__(self, eng, lists, layout, cell):
        import torch
        self.torch, self.eng, self.n = torch, eng, len(cell)
        n = self.n
        keys = np.concatenate([[0], lists.cell_keys]).astype(np.uint64)
        cb = keys[cell]
        unlisted = (cell == 0) & (np.arange(n) % 3 == 1)                 # a third of the misses carry a key nobody listed
        cb[unlisted] = np.uint64(0x7FFF000000000123)
        pad = max(n, 1)
        self.d_cb = hostmem.to_device(np.resize(cb, pad) if n else np.zeros(1, np.uint64), "cuda")
        self.d_hits_total = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.blk = None
        if layout != "soa":
            rb = eng.block_bytes(256)
            assert rb in (NARROW_RUNS if layout == "narrow" else WIDE_RUNS), rb
            self.blk = torch.full((max(eng.block_bytes(n), 8) // 8,), -1, dtype=torch.int64, device="cuda")   # (garbage where no record is)
            z8, z4 = torch.zeros(pad, dtype=torch.int64, device="cuda"), torch.zeros(pad, dtype=torch.int32, device="cuda")
            eng.dev_block_records(z8.data_ptr(), z4.data_ptr(), z4.data_ptr(), n, self.blk.data_ptr())
            eng.dev_count_hits_blocked(self.d_cb.data_ptr(), n, self.blk.data_ptr(), self.d_hits_total.data_ptr())
        else:
            eng.dev_count_hits(self.d_cb.data_ptr(), n, self.d_hits_total.data_ptr())
        torch.cuda.synchronize()
        assert int(self.d_hits_total.item()) == int((cell > 0).sum())

    @property
    def blk_ptr(self):
        return self.blk.data_ptr() if self.blk is not None else 0


def _cells(rng, n, n_cells, pattern):
    if pattern == "none":
        return np.zeros(n, np.int64)
    if pattern == "one_cell":
        return np.full(n, min(2, n_cells), np.int64)
    # log-normal popularity, 30 % misses
    w = rng.lognormal(0.0, 1.5, size=n_cells); w /= w.sum()
    c = rng.choice(n_cells, size=n, p=w) + 1
    c[rng.random(n) < 0.3] = 0
    return c.astype(np.int64)


N_HITS = [0, 1, 255, 256, 257, 4095, 4096, 4097, 200_000]


@pytest.mark.parametrize("lds_ranges", [None, "0"])
@pytest.mark.parametrize("n_cells", [3, 50_000, 70_000])
def test_cell_hits_against_bincount(layout, n_cells, lds_ranges, monkeypatch):
    """the unit (256) and K1a tile (4096) edges; SoA scratch, wide and narrow runs; LDS counters in one range (3 cells), two
    (50 000) and three ranges (70 000 cells, with the 32-bit scratch), and the same tables past any LDS budget
    (FASTF_CAP_LDS_RANGES=0: the general form, wave-aggregated global atomics); every hit in one cell; no hit at all"""
    if lds_ranges is not None:
        monkeypatch.setenv("FASTF_CAP_LDS_RANGES", lds_ranges)
    lists = _lists(n_cells)
    assert len(lists.cell_keys) == n_cells
    eng = F.Engine.from_lists(lists, umi_max_bases=12)
    import torch
    try:
        assert eng.cell_scratch_bytes == (2 if n_cells <= 65535 else 4)
        rng = np.random.default_rng(n_cells)
        for n in N_HITS:
            for pattern in (["mixed", "one_cell", "none"] if n in (257, 200_000) else ["mixed"]):
                cell = _cells(rng, n, n_cells, pattern)
                dev = _Dev(eng, lists, layout, cell)
                d_h = torch.full((n_cells + 2,), 0x55555555, dtype=torch.int32, device="cuda")
                for _ in range(2):                                        # the call clears what an earlier one left
                    eng.dev_cell_hits(n, dev.blk_ptr, d_h.data_ptr())
                    torch.cuda.synchronize()
                got = hostmem.to_host(d_h).view(np.uint32)
                want = np.bincount(cell[cell > 0] - 1, minlength=n_cells)
                np.testing.assert_array_equal(got[:n_cells].astype(np.int64), want, err_msg="n=%d %s" % (n, pattern))
                assert (got[n_cells:] == 0x55555555).all(), "entries behind the counters were written"
    finally:
        eng.close()


def test_cell_hits_with_lds_counters_at_the_budget(layout):
    """32 768 cells: the largest table that takes the LDS form (128 KiB of counters)"""
    n_cells = 32_768
    lists = _lists(n_cells)
    eng = F.Engine.from_lists(lists, umi_max_bases=12)
    import torch
    try:
        rng = np.random.default_rng(3)
        cell = _cells(rng, 150_001, n_cells, "mixed")
        cell[:5] = [n_cells, 1, n_cells, 0, 1]
        dev = _Dev(eng, lists, layout, cell)
        d_h = torch.zeros(n_cells, dtype=torch.int32, device="cuda")
        eng.dev_cell_hits(len(cell), dev.blk_ptr, d_h.data_ptr())
        np.testing.assert_array_equal(hostmem.to_host(d_h).view(np.uint32).astype(np.int64), np.bincount(cell[cell > 0] - 1, minlength=n_cells))
    finally:
        eng.close()


@pytest.mark.parametrize("n_cells", [H.CAP_LDS_CELLS * H.CAP_LDS_RANGES, H.CAP_LDS_CELLS * H.CAP_LDS_RANGES + 1])
def test_cell_hits_at_the_last_lds_range(layout, n_cells, monkeypatch):
    """262 144 cells: eight ranges, the most the LDS form takes; one cell more goes to the general form"""
    monkeypatch.delenv("FASTF_CAP_LDS_RANGES", raising=False)
    lists = _lists(n_cells)
    eng = F.Engine.from_lists(lists, umi_max_bases=12)
    import torch
    try:
        cell = H.last_range_cells(n_cells)
        dev = _Dev(eng, lists, layout, cell)
        d_h = torch.full((n_cells + 2,), 0x55555555, dtype=torch.int32, device="cuda")
        eng.dev_cell_hits(len(cell), dev.blk_ptr, d_h.data_ptr())
        torch.cuda.synchronize()
        got = hostmem.to_host(d_h).view(np.uint32)
        np.testing.assert_array_equal(got[:n_cells].astype(np.int64), np.bincount(cell[cell > 0] - 1, minlength=n_cells))
        assert (got[n_cells:] == 0x55555555).all(), "entries behind the counters were written"
    finally:
        eng.close()


_STREAMS = {}


def _stream(seed, skip, n):
    key = (seed, skip)
    if key not in _STREAMS or len(_STREAMS[key]) < n:
        _STREAMS[key] = O.mt_stream(seed, max(n, MT_PAR_MIN + 70_000), skip=skip).astype(np.uint64)
    return _STREAMS[key][:n]


def _hit_layout(rng, H, n_cells):
    """a cell array with exactly H hits: random places among 3 H + 600 records, and two stretches of 200 records without a hit
    (longer than a wave's 64 records: some waves contribute no bit)"""
    if H > 100_000:                                                       # the large case: nearly every record a hit
        n = H + 3 * 700
        cell = rng.integers(1, n_cells + 1, size=n)
        gaps = np.zeros(n, bool)
        for g in (1000, n // 2, n - 900):
            gaps[g:g + 700] = True
        cell[gaps] = 0
        assert int((cell > 0).sum()) == H
        return cell.astype(np.int64)
    n = 3 * H + 600
    ok = np.ones(n, bool); ok[100:300] = False; ok[n - 250:n - 50] = False
    at = np.sort(rng.choice(np.nonzero(ok)[0], size=H, replace=False))
    cell = np.zeros(n, np.int64)
    cell[at] = rng.integers(1, n_cells + 1, size=H)
    return cell


@pytest.mark.parametrize("skip", [0, 3])
def test_cell_decisions_against_the_stream_below_each_cells_threshold(layout, skip):
    n_cells, seed = 1000, 926
    lists = _lists(n_cells)
    eng = F.Engine.from_lists(lists, umi_max_bases=12)
    import torch
    try:
        rng = np.random.default_rng(11 + skip)
        T = rng.integers(0, (1 << 32) + 1, size=n_cells).astype(np.uint64)
        T[::4] = [0, 1, 1 << 31, 1 << 32] * (n_cells // 16) + [0, 1, 1 << 31, 1 << 32][:n_cells // 4 % 4]
        d_T = hostmem.to_device(T, "cuda")
        for H in [0, 1, 63, 64, 65, 4097, MT_PAR_MIN + 61_025]:
            if H > 100_000 and (layout == "wide" or skip == 3 and layout == "soa"):
                continue                                                  # (the jump-ahead generator feeds one layout per skip)
            cell = _hit_layout(rng, H, n_cells)
            dev = _Dev(eng, lists, layout, cell)
            used = (H + 63) // 64 * 2
            plane = torch.full((used + 6,), -1, dtype=torch.int32, device="cuda")
            eng.dev_cell_decisions(len(cell), dev.blk_ptr, seed, skip, H, d_T.data_ptr(), plane.data_ptr())
            torch.cuda.synchronize()
            got = hostmem.to_host(plane).view(np.uint32)
            bits = np.unpackbits(got[:used].copy().view(np.uint8), bitorder="little")
            want = (_stream(seed, skip, H) < T[cell[cell > 0] - 1]).astype(np.uint8)
            np.testing.assert_array_equal(bits[:H], want, err_msg="H=%d" % H)
            assert not bits[H:].any(), "tail bits of the last 64-bit word, H=%d" % H
            assert (got[used:] == 0xFFFFFFFF).all(), "words behind the plane were written, H=%d" % H
            if H == 4097:                                                 # the counters of the same K1a pass are still there
                d_h = torch.zeros(n_cells, dtype=torch.int32, device="cuda")
                eng.dev_cell_hits(len(cell), dev.blk_ptr, d_h.data_ptr())
                np.testing.assert_array_equal(hostmem.to_host(d_h).view(np.uint32).astype(np.int64), np.bincount(cell[cell > 0] - 1, minlength=n_cells))
    finally:
        eng.close()


# ---- the command ----
def _case(name):
    if name == "edge":
        return _Edge(), [0.5, 1], [1, 2, 5]
    if name == "mixed":
        return (Case(n=200_000, n_bar=600, n_gene=500, umi_len=12, dup_factor=3.0, p_no_cb=0.05, p_unlisted_cb=0.05, p_bad_xf=0.15,
                     p_n_umi=0.01, p_multi_gene=0.02), [0.5, 1], [1, 5, 40, 1_000_000])
    if name == "scratch_widths":                         # 70 000 barcodes: 32-bit cell scratch and global counters at -c 1, 16-bit at -c 0.5
        return (Case(n=150_000, n_bar=70_000, n_gene=300, umi_len=12, dup_factor=2.0, p_unlisted_cb=0.05, p_bad_xf=0.1, p_n_umi=0.01, data_seed=7),
                [0.5, 1], [1, 3])
    raise KeyError(name)


_POINTS = {}


def _point(name, case, bam, rc, n):
    key = (name, str(bam), rc, n)
    if key not in _POINTS:
        _POINTS[key] = cap_ref.point(case, str(bam).encode(), rc, n, case.seed)
    return _POINTS[key]


def _gz(p):
    return gzip.decompress(open(p, "rb").read())


def _check_outputs(out, name, case, bam, rates, caps, summary_only=False):
    rows = [ln.split("\t") for ln in open(out / "cap.tsv").read().split("\n")]
    assert rows[0] == list(cap.COLUMNS) and rows[-1] == [""]
    rows = rows[1:-1]
    assert len(rows) == len(rates) * len(caps)
    k = 0
    for rc in rates:
        for n in caps:
            ref = _point(name, case, bam, rc, n)
            d = out / cap.point_dir(rc, n)
            if summary_only:
                assert not d.exists()
            else:
                assert _gz(d / "matrix.mtx.gz") == ref["matrix"], d
                assert _gz(d / "barcodes.tsv.gz") == ref["barcodes"], d
                assert _gz(d / "features.tsv.gz") == ref["features"], d
            assert rows[k] == ref["row"], (rc, n)
            k += 1
    assert not (out / "cap.tsv.partial").exists()
    return rows


def _args(bam, b, f, out, rates, caps):
    return ["-b", str(bam), "-a", str(b), "-f", str(f), "-o", str(out), "-c", ",".join("%g" % r for r in rates), "-n", ",".join(str(n) for n in caps)]


def test_reference_keeps_what_the_semantics_say():
    """cap_ref on the CPU: a cell at or below the cap keeps every read, a cell above it keeps about N; the last cap of the mixed
    case exceeds every cell"""
    case, rates, caps = _case("mixed")
    for n in caps:
        ref = cap_ref.point(case, b"x.bam", 1.0, n, case.seed)
        _, cell, h, _ = cap_ref.hits_of(case, 1.0, case.seed)
        kept = np.bincount(cell[cell > 0][ref["keep"]] - 1, minlength=len(h))
        assert (kept[h <= n] == h[h <= n]).all() and (kept <= h).all()
        assert ref["cells_capped"] == int((h > n).sum())
        if n == 1_000_000:
            assert ref["cells_capped"] == 0 and ref["sampled"] == ref["hits"] and ref["realised"] == 1.0
        elif n == 40:
            big = h > 200
            assert big.any() and (np.abs(kept[big] - 40.0) < 6 * np.sqrt(40.0)).all()


@pytest.mark.parametrize("name", ["edge", "mixed", "scratch_widths"])
def test_cli_cap_against_the_reference(tmp_path, name):
    case, rates, caps = _case(name)
    bam, b, f = _write(tmp_path, case)
    out = tmp_path / "out"
    r = subprocess.run([_lib.cli_path(), "cap", "-d", str(tmp_path / "x.db")] + _args(bam, b, f, out, rates, caps), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    rows = _check_outputs(out, name, case, bam, rates, caps)
    if name == "mixed":
        last = [x for x in rows if x[1] == "1000000"]
        assert len(last) == 2 and all(x[13] == "0" and x[14] == "1.000000" and x[5] == x[12] for x in last)
        assert all(int(x[13]) > 0 for x in rows if x[1] == "1")
    out2 = tmp_path / "out2"
    r = subprocess.run([_lib.cli_path(), "cap", "--summary-only", "-s926"] + _args(bam, b, f, out2, rates, caps), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert open(out2 / "cap.tsv").read() == open(out / "cap.tsv").read()
    assert sorted(os.listdir(out2)) == ["cap.tsv"]


@pytest.mark.parametrize("env", [{"FASTF_LDS_TABLES": "0"}, {"FASTF_LDS_CELLS": "0"}, {"FASTF_NO_STREAM_K1B": "1"}, {"FASTF_SORT_SKIP_BITS": "0"},
                                 {"FASTF_GENES_NO_DIRECT": "1"}, {"FASTF_BLOCK_WIDE": "1"}, {"FASTF_GPU_PARSE": "0"}])
def test_cli_cap_on_the_general_paths(tmp_path, env):
    case, rates, caps = _case("mixed")
    bam, b, f = _write(tmp_path, case)
    out = tmp_path / "out"
    r = subprocess.run([_lib.cli_path(), "cap"] + _args(bam, b, f, out, rates, caps), capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr
    _check_outputs(out, "mixed", case, bam, rates, caps)


def test_cap_in_process(tmp_path):
    case, rates, caps = _case("mixed")
    bam, b, f = _write(tmp_path, case)
    out = tmp_path / "out"
    rows = cap.cap(bam, out, b, f, rates, caps, seed=926)
    assert len(rows) == 8 and rows[0]["rate_cell"] == "0.500" and rows[-1]["reads_per_cell"] == "1000000"
    _check_outputs(out, "mixed", case, bam, rates, caps)
    out2 = tmp_path / "out2"
    rows2 = cap.cap(bam, out2, b, f, rates, caps, seed=926, summary_only=True)
    assert rows2 == rows and sorted(os.listdir(out2)) == ["cap.tsv"]
    # another seed is another grid
    rows3 = cap.cap(bam, tmp_path / "out3", b, f, [0.5], [5], seed=1, summary_only=True)
    assert list(rows3[0].values()) == cap_ref.point(case, str(bam).encode(), 0.5, 5, 1)["row"]


def test_refusals_exit_1_and_leave_no_table(tmp_path):
    """20-base UMIs do not fit a 64-bit key and a cap has no point-by-point form; -n 0"""
    case = Case(n=30_000, n_bar=400, n_gene=150, umi_len=20, umi_pool=512, p_n_umi=0.02, p_bad_xf=0.1, data_seed=35)
    bam, b, f = _write(tmp_path, case)
    for k, (caps, word) in enumerate([("5,50", "outside the resident form"), ("0", "at least 1")]):
        out = tmp_path / ("out%d" % k)
        r = subprocess.run([_lib.cli_path(), "cap", "-b", str(bam), "-a", str(b), "-f", str(f), "-o", str(out), "-n", caps],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 1, r.stderr
        assert word in r.stderr, r.stderr
        assert not (out / "cap.tsv").exists() and not (out / "cap.tsv.partial").exists()
    with pytest.raises(F.FastfError):
        cap.cap(bam, tmp_path / "outp", b, f, [1], [5])
    assert not (tmp_path / "outp" / "cap.tsv").exists()
