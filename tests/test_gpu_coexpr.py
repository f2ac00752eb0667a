"""--coexpression on the GPU, stage by stage: fastf_dev_coexpr_sums (the gene-major planes byte for byte, D and S exactly against
coexpr_ref.sums) in its MFMA and its plain form and with chunks of 32 cells and the default, fastf_dev_coexpr_select against
coexpr_ref.partner_sets, fastf_dev_neighbors_shared on the sets against coexpr_ref.per_gene, and the refusals.  Guard words stand behind
every output, rows that must not be read behind every input."""
import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import hostmem, sweep
import coexpr_ref as R
import coexpr_dev_ref as X

pytestmark = pytest.mark.gpu

GUARD32, GUARD64 = np.uint32(0xFFFFFFFF), np.uint64(0xFFFFFFFFFFFFFFFF)
FORMS = ("mfma", "plain")
CHUNKS = ("32", None)                                       # FASTF_COEXPR_CHUNK: three chunks at n = 65; the default


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    cells = np.arange(1, 101, dtype=np.uint64) | (np.uint64(1) << np.uint64(62))
    feats = np.arange(1, 51, dtype=np.uint64) | (np.uint64(2) << np.uint64(62))
    e = F.Engine(cells, feats, umi_max_bases=12)
    yield e
    e.close()


def _knobs(monkeypatch, form, chunk):
    if form == "plain":
        monkeypatch.setenv("FASTF_COEXPR_MFMA", "0")
    else:
        monkeypatch.delenv("FASTF_COEXPR_MFMA", raising=False)
    if chunk is None:
        monkeypatch.delenv("FASTF_COEXPR_CHUNK", raising=False)
    else:
        monkeypatch.setenv("FASTF_COEXPR_CHUNK", chunk)


def _rows_on_device(rows, genes, nf):
    """the rows, behind them 300 rows of a gene of A in cell 1 whose count would change every sum of that gene; the count word; the map"""
    pads = (int(genes[0]) + 1 if len(genes) else 1, 1, 1 << 20)
    dev = [hostmem.to_device(np.concatenate([np.asarray(a, np.uint32), np.full(300, v, np.uint32)]), "cuda") for a, v in zip(rows, pads)]
    d_nnz = hostmem.to_device(np.array([len(rows[0])], np.uint64), "cuda")
    d_map = hostmem.to_device(np.concatenate([R.slot_map(genes, nf), np.zeros(64, np.uint16)]).view(np.uint8), "cuda")     # (slot 0 behind the map)
    return dev, d_nnz, d_map


def _device_sums(eng, rows, n, nf, genes, want_planes=None, want_chunk=None):
    """planes, D and S of one row set as the device leaves them: (D, S as lists of ints, the device tensors of D and S)"""
    import torch
    K = len(genes)
    dev, d_nnz, d_map = _rows_on_device(rows, genes, nf)
    P = eng.dev_neighbor_planes(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), d_nnz.data_ptr(), d_map.data_ptr(), nf, n, K)
    assert 1 <= P <= 3 and (want_planes is None or P == want_planes)
    K_pad, n_pad, chunk = sweep.coexpression_pad(n, K)
    n32 = max(32, (n + 31) // 32 * 32)
    assert K_pad % 32 == 0 and K_pad >= K and chunk % 32 == 0 and n_pad % chunk == 0 and n32 <= n_pad < n32 + chunk
    assert want_chunk is None or chunk == want_chunk
    size = sweep.coexpression_work_bytes(n, K, P)
    assert size == P * K_pad * n_pad
    d_work = torch.full((size + 256,), 0xEE, dtype=torch.uint8, device="cuda")
    d_D = torch.full((K * K + 64,), -1, dtype=torch.int64, device="cuda")
    d_S = torch.full((K + 64,), -1, dtype=torch.int64, device="cuda")
    args = (dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), d_nnz.data_ptr(), d_map.data_ptr(), nf, n, K, P)
    with pytest.raises(F.FastfError, match="the buffer has"):
        eng.dev_coexpr_sums(*args, d_work.data_ptr(), size - 1, d_D.data_ptr(), d_S.data_ptr())
    torch.cuda.synchronize()
    assert (hostmem.to_host(d_work) == 0xEE).all() and (hostmem.to_host(d_D) == -1).all() and (hostmem.to_host(d_S) == -1).all(), "a refused call wrote"
    eng.dev_coexpr_sums(*args, d_work.data_ptr(), size, d_D.data_ptr(), d_S.data_ptr())
    torch.cuda.synchronize()
    planes = hostmem.to_host(d_work)
    assert (planes[size:] == 0xEE).all(), "bytes behind the planes were written"
    m = np.array(R.columns(rows, n, genes, nf), np.int64).reshape(K, n)
    want = np.zeros((P, K_pad, n_pad), np.uint8)
    for p in range(P):
        want[p, :K, :n] = (m >> (7 * p)) & 127
    assert (planes[:size].reshape(P, K_pad, n_pad) == want).all()
    D, S = hostmem.to_host(d_D).view(np.uint64), hostmem.to_host(d_S).view(np.uint64)
    assert (D[K * K:] == GUARD64).all() and (S[K:] == GUARD64).all(), "words behind an array were written"
    return [[int(v) for v in row] for row in D[:K * K].reshape(K, K)], [int(v) for v in S[:K]], (d_D, d_S)


def _device_select(eng, d_D, d_S, n, K, k):
    """the partner sets of D and S on the device: (lists, the device tensors of idx and cnt)"""
    import torch
    d_idx = torch.full((K * k + 64,), -1, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((K + 64,), -1, dtype=torch.int32, device="cuda")
    eng.dev_coexpr_select(d_D.data_ptr(), d_S.data_ptr(), n, K, k, d_idx.data_ptr(), d_cnt.data_ptr())
    torch.cuda.synchronize()
    idx, cnt = hostmem.to_host(d_idx).view(np.uint32), hostmem.to_host(d_cnt).view(np.uint32)
    assert (idx[K * k:] == GUARD32).all() and (cnt[K:] == GUARD32).all(), "words behind an array were written"
    idx2 = idx[:K * k].reshape(K, k)
    assert (cnt[:K] <= k).all() and all((idx2[g, cnt[g]:] == GUARD32).all() for g in range(K))
    return X.as_lists(idx2, cnt[:K]), (d_idx, d_cnt)


def _on_device(D, S):
    K = len(S)
    d_D = hostmem.to_device(np.concatenate([np.array(D, np.uint64).reshape(K * K), np.full(64, GUARD64)]).view(np.int64), "cuda")
    d_S = hostmem.to_device(np.concatenate([np.array(S, np.uint64), np.full(64, GUARD64)]).view(np.int64), "cuda")
    return d_D, d_S


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sorted(X.ALL))
def test_planes_sums_and_sets_against_the_reference(eng, name, form, chunk, monkeypatch):
    _knobs(monkeypatch, form, chunk)
    rows, n, nf, genes, k = X.fixture(name)
    D, S = X.reference(name)
    n32 = max(32, (n + 31) // 32 * 32)
    gD, gS, (d_D, d_S) = _device_sums(eng, rows, n, nf, genes, X.planes_of(rows, n, nf, genes), min(32 if chunk else sweep.COEXPRESSION_CHUNK, n32))
    assert gS == S
    assert gD == D
    if len(genes):
        assert _device_select(eng, d_D, d_S, n, len(genes), k)[0] == X.sets(name, k)


@pytest.mark.parametrize("k", [1, 64])
@pytest.mark.parametrize("name", ["K65_n65", "K97_n31", "tie_63_64", "wide", "k64", "duplicates", "proportional"])
def test_selection_on_handed_sums(eng, name, k):
    """D and S of the reference handed to the selection directly: the sets do not depend on where the sums came from"""
    D, S = X.reference(name)
    d_D, d_S = _on_device(D, S)
    assert _device_select(eng, d_D, d_S, X.fixture(name)[1], len(S), k)[0] == X.sets(name, k)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["K65_n65", "K33_n65", "k15", "duplicates", "edges"])
def test_shared_counts_of_a_point_against_the_full_sets(eng, name, form, monkeypatch):
    import torch
    _knobs(monkeypatch, form, "32")
    rows, n, nf, genes, k = X.fixture(name)
    K = len(genes)
    point = X.point_rows(rows)
    pD, pS = R.sums(R.columns(point, n, genes, nf), n)
    full_sets, point_sets = X.sets(name, k), R.partner_sets(pD, pS, n, k)
    _, _, (fD, fS) = _device_sums(eng, rows, n, nf, genes)
    gD, gS, (qD, qS) = _device_sums(eng, point, n, nf, genes)
    assert gD == pD and gS == pS
    a, (ai, ac) = _device_select(eng, fD, fS, n, K, k)
    b, (bi, bc) = _device_select(eng, qD, qS, n, K, k)
    assert a == full_sets and b == point_sets
    d_sh = torch.full((K + 64,), -1, dtype=torch.int32, device="cuda")
    eng.dev_neighbors_shared(ai.data_ptr(), ac.data_ptr(), bi.data_ptr(), bc.data_ptr(), K, k, d_sh.data_ptr())
    torch.cuda.synchronize()
    sh = hostmem.to_host(d_sh).view(np.uint32)
    assert (sh[K:] == GUARD32).all()
    assert [int(v) for v in sh[:K]] == R.per_gene(full_sets, point_sets)[2]


@pytest.mark.parametrize("form", FORMS)
def test_full_accumulators(eng, form, monkeypatch):
    """every digit 127: 3 * 96 * 127^2 in the middle accumulator of one chunk of 96 cells; then a full chunk of the true default and
    one step of 32 cells behind it"""
    _knobs(monkeypatch, form, "96")
    rows, n, nf, genes, k = X.fixture("saturated")
    D, S = X.reference("saturated")
    gD, gS, (d_D, d_S) = _device_sums(eng, rows, n, nf, genes, 3, 96)
    assert gD == D and gS == S
    assert _device_select(eng, d_D, d_S, n, 2, k)[0] == X.sets("saturated", k) == [[], []]
    _knobs(monkeypatch, form, None)
    n = sweep.COEXPRESSION_CHUNK + 32
    rows = (np.repeat(np.array([1, 2], np.uint32), n), np.tile(np.arange(1, n + 1, dtype=np.uint32), 2), np.full(2 * n, X.TOP3, np.uint32))
    dev, d_nnz, d_map = _rows_on_device(rows, [0, 1], 2)
    import torch
    K_pad, n_pad, chunk = sweep.coexpression_pad(n, 2)
    assert chunk == sweep.COEXPRESSION_CHUNK and n_pad == 2 * chunk
    size = sweep.coexpression_work_bytes(n, 2, 3)
    d_work = torch.full((size + 256,), 0xEE, dtype=torch.uint8, device="cuda")
    d_D = torch.full((4 + 64,), -1, dtype=torch.int64, device="cuda")
    d_S = torch.full((2 + 64,), -1, dtype=torch.int64, device="cuda")
    eng.dev_coexpr_sums(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), d_nnz.data_ptr(), d_map.data_ptr(), 2, n, 2, 3, d_work.data_ptr(), size,
                        d_D.data_ptr(), d_S.data_ptr())
    torch.cuda.synchronize()
    assert (hostmem.to_host(d_work[size:]) == 0xEE).all()
    gD, gS = hostmem.to_host(d_D).view(np.uint64), hostmem.to_host(d_S).view(np.uint64)
    assert [int(v) for v in gD[:4]] == [n * X.TOP3 * X.TOP3] * 4 and [int(v) for v in gS[:2]] == [n * X.TOP3] * 2
    assert (gD[4:] == GUARD64).all() and (gS[2:] == GUARD64).all()


def test_the_refusals_of_the_device_calls(eng):
    import torch
    rows, n, nf, genes, k = X.fixture("K33_n65")
    K = len(genes)
    D, S = X.reference("K33_n65")
    d_D, d_S = _on_device(D, S)
    d_idx = torch.full((K * 64 + 64,), -1, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((K + 64,), -1, dtype=torch.int32, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return (hostmem.to_host(d_idx) == -1).all() and (hostmem.to_host(d_cnt) == -1).all()
    for bad_k in (0, 65):
        with pytest.raises(F.FastfError, match="from 1 to 64"):
            eng.dev_coexpr_select(d_D.data_ptr(), d_S.data_ptr(), n, K, bad_k, d_idx.data_ptr(), d_cnt.data_ptr())
    with pytest.raises(F.FastfError, match="4097 genes, at most 4096"):
        eng.dev_coexpr_select(d_D.data_ptr(), d_S.data_ptr(), n, 4097, 15, d_idx.data_ptr(), d_cnt.data_ptr())
    with pytest.raises(F.FastfError, match="4097 genes, at most 4096"):
        eng.dev_coexpr_sums(0, 0, 0, d_cnt.data_ptr(), 0, nf, n, 4097, 1, d_idx.data_ptr(), 1 << 40, d_D.data_ptr(), d_S.data_ptr())
    # n * max Q = 2 * 2^62: the largest D_gg is read back and the selection is not launched
    wide = [[1 << 62, 5], [5, 7]]
    w_D, w_S = _on_device(wide, [1 << 31, 3])
    assert not R.in_range(wide, 2) and R.in_range(wide, 1)
    with pytest.raises(F.FastfError, match="FASTF_ERR_COEXPR_RANGE"):
        eng.dev_coexpr_select(w_D.data_ptr(), w_S.data_ptr(), 2, 2, 15, d_idx.data_ptr(), d_cnt.data_ptr())
    assert untouched()
    # three planes over more than 2^22 cells: a sum of products would leave 64 bits; nothing is read or launched
    with pytest.raises(F.FastfError, match="FASTF_ERR_COEXPR_CELLS"):
        eng.dev_coexpr_sums(0, 0, 0, d_cnt.data_ptr(), 0, nf, (1 << 22) + 5, K, 3, d_idx.data_ptr(), 1 << 40, d_D.data_ptr(), d_S.data_ptr())
    with pytest.raises(F.FastfError, match="planes, from 1 to 3"):
        eng.dev_coexpr_sums(0, 0, 0, d_cnt.data_ptr(), 0, nf, n, K, 4, d_idx.data_ptr(), 1 << 40, d_D.data_ptr(), d_S.data_ptr())
    torch.cuda.synchronize()
    gD = hostmem.to_host(d_D).view(np.uint64)
    assert [int(v) for v in gD[:K * K]] == [v for row in D for v in row] and untouched()
    eng.dev_coexpr_select(0, 0, 5, 0, 15, 0, 0)             # no genes: nothing is launched
    names = F._lib.lib().fastf_kernel_names().decode().split(",")
    assert {"coex_planes_kernel", "coex_gram_kernel", "coex_sums_kernel", "coex_var_kernel", "coex_select_kernel"} <= set(names)
